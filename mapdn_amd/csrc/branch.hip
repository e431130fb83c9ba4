// branch.hip — res_line / res_trafo for every env (mapdn_get_branch_results) and their per-env reduction (mapdn_get_loading_summary):
// what the reference reads from pandapower's result tables after runpp (environments/var_voltage_control/pf_res_plot.py:142-163).
// The arithmetic is branch.hpp's; DESIGN.md §17 holds the layout and the bytes moved.
#include "branch.hpp"
#include "kernels.hpp"

namespace mapdn {

// a wave-uniform record through the constant address space: scalar loads, as k_gather reads its descriptors
__device__ __forceinline__ BranchRec load_rec(const BranchRec* g, int i) {
  typedef const __attribute__((address_space(4))) double* c_f64;
  const c_f64 p = (c_f64)(unsigned long long)(g + i);
  double raw[sizeof(BranchRec) / sizeof(double)];
#pragma unroll
  for (int q = 0; q < (int)(sizeof(BranchRec) / sizeof(double)); ++q) raw[q] = p[q];
  BranchRec r;
  __builtin_memcpy(&r, raw, sizeof(BranchRec));
  return r;
}

// One thread per (env, branch) over both tables.  A workgroup takes 64 envs x BR_TILE branches of ONE table: wave w evaluates branch w
// of the tile with the env on the lane — the branch record is wave-uniform, the voltage reads of the env-state route are 64 consecutive
// doubles of an env-minor row — and every requested column then goes through a [64][BR_TILE + 1] LDS tile so that 16 lanes store
// BR_TILE consecutive doubles (128 bytes) of one env's row of the caller's [B, n] array.
__global__ void __launch_bounds__(64 * BR_TILE) k_branch_results(BranchArgs a) {
  __shared__ double tile[64][BR_TILE + 1];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ty = blockIdx.y, table = ty >= a.line_tiles ? 1 : 0;
  const int b0 = (table ? ty - a.line_tiles : ty) * BR_TILE, nrow = table ? a.n_trafo : a.n_line, base = table ? a.n_line : 0;
  const int e0 = blockIdx.x * 64;
  const size_t er = (size_t)min(e0 + lane, a.B - 1);      // a pad env reads the last env's voltages and stores nothing
  uint32_t mask = 0;
#pragma unroll
  for (int c = 0; c < BC_N; ++c) mask |= (table ? a.out[1][c] : a.out[0][c]) ? (1u << c) : 0u;
  double v[BC_N];
#pragma unroll
  for (int c = 0; c < BC_N; ++c) v[c] = 0.0;
  if (b0 + w < nrow) {                                     // wave-uniform
    const BranchRec r = load_rec(a.rec, base + b0 + w);
    const size_t jf = (size_t)r.f * a.sb + er * a.se, jt = (size_t)r.t * a.sb + er * a.se;
    branch_eval(r, a.vm[jf], a.va[jf] * a.ang, a.vm[jt], a.va[jt] * a.ang, a.sn, mask, v);
  }
  const int j = threadIdx.x & (BR_TILE - 1), r0 = threadIdx.x / BR_TILE;   // r0 = 0 .. 63: one env row of the tile per 16 lanes
  const int e = e0 + r0;
#pragma unroll
  for (int c = 0; c < BC_N; ++c) {
    double* const out = table ? a.out[1][c] : a.out[0][c];
    if (!out) continue;                                    // uniform over the workgroup
    tile[lane][w] = v[c];
    __syncthreads();
    if (e < a.B && b0 + j < nrow) out[(size_t)e * nrow + b0 + j] = tile[r0][j];
    __syncthreads();
  }
}

// max / argmax / count of loading_percent over the rated in-service branches of both tables, from the env's current voltages.  A workgroup
// takes 64 envs; wave w walks branches w, w + LS_WAVES, ... in ascending order, then wave 0 merges the LS_WAVES partials.  max, "lowest
// index that attains it" and an integer count do not depend on the order of a merge, and a branch's loading depends on its env alone:
// the bits are the same in every batch size and launch geometry.
__global__ void __launch_bounds__(64 * LS_WAVES) k_loading_summary(LoadingArgs a) {
  __shared__ double s_max[LS_WAVES][64];
  __shared__ int32_t s_idx[LS_WAVES][64], s_cnt[LS_WAVES][64];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t e = (size_t)blockIdx.x * 64 + lane;        // < Bp: the env-minor rows are padded
  double m = 0.0;
  int32_t idx = -1, cnt = 0;
  for (int b = w; b < a.n_branch; b += LS_WAVES) {
    const BranchRec r = load_rec(a.rec, b);
    if (!r.live || r.rate != r.rate) continue;             // wave-uniform: out of service or unrated
    const size_t jf = (size_t)r.f * a.Bp + e, jt = (size_t)r.t * a.Bp + e;
    double o[BC_N];
    branch_eval(r, a.vm[jf], a.va[jf], a.vm[jt], a.va[jt], a.sn, BM_FLOW, o);
    const double l = o[BC_LOAD];
    if (idx < 0 || l > m) { m = l; idx = b; }
    cnt += l > a.limit ? 1 : 0;
  }
  s_max[w][lane] = m; s_idx[w][lane] = idx; s_cnt[w][lane] = cnt;
  __syncthreads();
  if (w != 0 || e >= (size_t)a.B) return;
  for (int q = 1; q < LS_WAVES; ++q) {
    const double mq = s_max[q][lane];
    const int32_t iq = s_idx[q][lane];
    cnt += s_cnt[q][lane];
    if (iq >= 0 && (idx < 0 || mq > m || (mq == m && iq < idx))) { m = mq; idx = iq; }
  }
  a.max_loading[e] = idx < 0 ? NAN : m;
  a.worst[e] = idx;
  a.n_over[e] = cnt;
}

void launch_branch_results(const BranchArgs& a, int Bp, hipStream_t st) {
  const int tiles = a.line_tiles + a.trafo_tiles;
  if (tiles > 0) hipLaunchKernelGGL(k_branch_results, dim3(Bp / 64, tiles), dim3(64 * BR_TILE), 0, st, a);
}

void launch_loading_summary(const LoadingArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_loading_summary, dim3(a.Bp / 64), dim3(64 * LS_WAVES), 0, st, a);
}

}  // namespace mapdn
