// critic.hip — the learner's critic trunk on rows of 64 as ONE forward and ONE backward launch, gfx950 (MI355X).
//
// Reference: critics/mlp_critic.py:22-36 (fc1 -> LayerNorm -> ReLU -> fc2 -> ReLU -> fc3) as evaluated by models/maddpg.py:35-79 /
// models/iddpg.py:32-58 on [batch x agents] rows and trained by learning_algorithms/ddpg.py:15-39.  What follows the first layer —
//     v = relu( relu(LayerNorm(x)) W2^T + b2 ) . w3 + b3
// — ran as LayerNorm kernel + hipBLASLt GEMM + relu-dot kernel forward and five launches backward, every one of them streaming
// the [rows, 64] activations (2.7 GB at the end-to-end configuration's 10 M rows) through HBM at K = 64.  Here a wavefront owns
// tiles of 16 rows and keeps them in registers from the LayerNorm input to v (forward) and from dv to dx and the parameter
// gradients (backward, which recomputes the forward instead of reading saved activations): HBM sees x (or, for the central
// critic, only the two small operands the row is FORMED from: base[row / n] + per_n[row % n]), dv and the outputs.
//
// All products run on v_mfma_f32_16x16x4_f32 (exact fp32, an fmaf chain: the reference's fp32 modules).  Layouts, for a tile of 16
// rows and lane l = (j = l & 15, g = l >> 4):
//   "A layout"  lane holds row j, features 16 c + 4 g + q (c, q = 0..3): 4 x float4.  This is the MFMA *B* operand of a product
//               whose OUTPUT is transposed, D[i = feature][j = row]: pre^T = W2 xn^T and dxn^T = W2^T dpre^T take the
//               activations as B and the (LDS- or register-resident) weight as A, and their D registers
//               (row j, feature 16 nt + 4 g + r) are again in A layout — the chain x -> xn -> pre -> dpre -> dxn -> dx never
//               leaves the lane's row, and the LayerNorm / dot reductions are 16 in-lane adds + two row swaps
//               (v_permlane16_swap / v_permlane32_swap).
//   "C layout"  lane holds rows 4 g + s, feature 16 nt + j: needed only by dW2 += dpre^T xn (the contraction runs over ROWS),
//               reached through a per-wave 16 x 64 LDS tile.
// dW2 / dgamma / dbeta / db2 / dw3 / db3 (and, for formed rows, dper_n) are accumulated per wavefront over its contiguous range of
// rows, summed across the wavefronts of a workgroup through LDS and across workgroups by a second small launch, both in a fixed
// order: deterministic, no atomics.
//
// Where things live: rowtile.hpp has the lane-level helpers (reductions, LayerNorm statistics, wave_sync); headtile.hpp has the trunk on
// one tile as steps (head_value forward; mm64_lds, dpre_step, dw2_step, ln_backward, formed_handover, head_partials backward).  This file
// has the single head's kernels — how a row is read or formed, what dv is (given, or the fused value loss), where dx goes — the launch
// shapes and the C entry points; critic_twin.hip, critic_cf.hip and critic_shap.hip, included at the end, put the same steps together
// for MATD3, COMA and SQDDPG (k_twin_mse keeps its LayerNorm backward and critic_shap.hip its four MFMA products spelt out, for the
// reasons given there).  critic_attn.hip (MAAC) shares only head_cus and k_head_reduce.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>

#include "../../include/mapdn.h"
#include "rowtile.hpp"
#include "headtile.hpp"

namespace mapdn {

// the lane's row in A layout: x[row][16 c + 4 g ..] or base[row / n] + per_n[row % n] (one f32 add, as the broadcast add would)
template <bool BC>
__device__ __forceinline__ void load_row(const HeadArgs& p, long row, int g, f4 (&xa)[4]) {
  if (BC) {
    const unsigned q = (unsigned)row / (unsigned)p.n, i = (unsigned)row - q * (unsigned)p.n;
    const float* pb = p.x + (size_t)q * 64 + 4 * g;
    const float* pn = p.per_n + (size_t)i * 64 + 4 * g;
#pragma unroll
    for (int c = 0; c < 4; ++c) xa[c] = *(const f4*)(pb + 16 * c) + *(const f4*)(pn + 16 * c);
  } else {
    const float* px = p.x + (size_t)row * 64 + 4 * g;
#pragma unroll
    for (int c = 0; c < 4; ++c) xa[c] = *(const f4*)(px + 16 * c);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// forward: v[row] = relu(relu(LN(x)) W2^T + b2) . w3 + b3.  W2 lives in registers as the A operand (64 VGPRs), 64 MFMAs per tile.
template <bool BC>
__global__ void __launch_bounds__(256)
k_head_fwd(HeadArgs p, float* __restrict__ v, long rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, j = lane & 15;
  f4 wop[4][4];
  load_w2_operand(p.w2, j, g, wop);
  const HeadParams<false> par(p, g);
  const float b3 = p.b3[0];
  const long n_tiles = (rows + 15) >> 4;
  for (long T = (long)blockIdx.x * 4 + wave; T < n_tiles; T += (long)gridDim.x * 4) {
    const long row = T * 16 + j;
    f4 xa[4];
    load_row<BC>(p, row < rows ? row : rows - 1, g, xa);
    const float dot = head_value(xa, p.eps, wop, par);
    if (g == 0 && row < rows) v[row] = dot + b3;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// backward.  MODE 0: dx (or, for formed rows, dbase = sum over the n rows of a group, and dper_n) + every parameter gradient;
//            MODE 1: dx / dbase / dper_n only (the parameters do not require grad);
//            MODE 2: dact[row] = dx[row] . dot_w[row % n] only (the policy update through the central critic: the own-action column
//                    of fc1 — models/maddpg.py:52-58 — is the only path back to the policy);
//            MODE 3: MODE 0 with the value loss fused in (learning_algorithms/ddpg.py:36-38, models/maddpg.py:122-124):
//                    loss = sum_rows w[row] (ret[row] - v[row])^2, w[row] = scale[0] * wrow[row / n] (wrow may be null: 1), and dv is
//                    formed in the kernel as -2 w (ret - v) — the forward launch and its product are not needed at all.
// A wavefront owns a contiguous range of rows (whole groups of n for formed rows: the sum over a group never crosses wavefronts).
// NT threads per workgroup: 256 = one wavefront per SIMD with the whole 512-register file (parameters in registers, the next tile
// prefetched, two staging tiles); 512 = TWO wavefronts per SIMD, each within 256 registers (parameters read from LDS where used, no
// prefetch, one staging tile used twice) — one wavefront's LayerNorm / staging / reduction VALU work then runs under the other's MFMAs.
template <bool BC, int MODE, int NT>
__global__ void __launch_bounds__(NT)
k_head_bwd(HeadArgs p, const float* __restrict__ dv, float* __restrict__ dx, const float* __restrict__ dot_w, float* __restrict__ dact,
           float* __restrict__ partial, int pstride, long rows, const float* __restrict__ wrow, const float* __restrict__ scale) {
  constexpr bool PG = MODE == 0 || MODE == 3;        // parameter gradients wanted
  constexpr int NW = NT / 64, TILES = NT == 512 ? 1 : 2;
  constexpr bool SLIM = NT == 512;
  extern __shared__ float sm[];
  const HeadLds L(sm);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, j = lane & 15;
  float* stage = L.rest + (size_t)wave * TILES * 16 * HS;                                   // TILES 16 x HS tiles per wavefront
  float* accn0 = L.rest + (size_t)NW * TILES * 16 * HS, *accn = accn0 + (size_t)wave * p.n * 64;   // [n][64] per wavefront (BC, MODE != 2)
  L.fill(p, tid, NT);
  if (BC && MODE != 2) for (int i = lane; i < p.n * 64; i += 64) accn[i] = 0.0f;
  const HeadParams<SLIM> par(p, g, L.sP);
  __syncthreads();

  // this wavefront's range of rows [r0, r1)
  const long W = (long)gridDim.x * NW, w = (long)blockIdx.x * NW + wave;
  long r0, r1;
  if (BC) { const long G = rows / p.n; r0 = (G * w / W) * p.n; r1 = (G * (w + 1) / W) * p.n; }
  else { const long Tn = (rows + 15) >> 4; r0 = (Tn * w / W) * 16; r1 = (Tn * (w + 1) / W) * 16; if (r1 > rows) r1 = rows; }

  HeadAcc A;
  float carry = 0.0f;                       // running sum of dx over the rows of the current group (lane = column)
  const float b3 = MODE == 3 ? p.b3[0] : 0.0f, lscale = MODE == 3 ? scale[0] : 0.0f;

  // the rows of the NEXT tile are requested while the current one is in the matrix cores (one wavefront per SIMD: nobody else hides
  // the HBM / L2 latency)
  f4 xnext[4];
  float dvnext = 0.0f;
  if (!SLIM && r0 < r1) {
    const long row = r0 + j;
    load_row<BC>(p, row < r1 ? row : r1 - 1, g, xnext);
    dvnext = row < r1 ? dv[row] : 0.0f;
  }
  for (long row0 = r0; row0 < r1; row0 += 16) {
    const long row = row0 + j;
    const bool valid = row < r1;
    f4 xh[4];
    float dvcur;
    if (SLIM) {
      load_row<BC>(p, valid ? row : r1 - 1, g, xh);
      dvcur = valid ? dv[row] : 0.0f;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) xh[c] = xnext[c];
      dvcur = dvnext;
      if (row0 + 16 < r1) {
        const long rn = row + 16;
        load_row<BC>(p, rn < r1 ? rn : r1 - 1, g, xnext);
        dvnext = rn < r1 ? dv[rn] : 0.0f;
      }
    }
    const float rs = ln_stats(xh, p.eps);
    f4 xn[4], acc[4], dxn[4];
    ln_affine_relu(xh, par, xn);
    mm64_lds(L.sW, lane, xn, acc);           // pre^T = W2 xn^T
    float dvr = dvcur;                       // (MODE 3: dv holds the returns)
    if (MODE == 3) {
      float wgt = lscale;
      if (wrow) { const unsigned rc = (unsigned)(valid ? row : r1 - 1); wgt *= wrow[BC ? rc / (unsigned)p.n : rc]; }
      dvr = mse_dv(acc, par, b3, dvcur, wgt, valid, g, A.aloss);
    }
    dpre_step<PG>(acc, dvr, par, g, A);
    mm64_lds(L.sWT, lane, acc, dxn);         // dxn^T = W2^T dpre^T
    if (PG) dw2_step<SLIM>(stage, j, g, acc, xn, A.accW);
    ln_backward<PG>(xn, xh, rs, par, dxn, A);
    // ---- hand dx over
    if (MODE == 2) {
      const unsigned i = BC ? (unsigned)((valid ? row : r1 - 1) - r0) % (unsigned)p.n : 0u;
      const float d = dx_dot(dxn, dot_w + (size_t)i * 64 + 4 * g);
      if (g == 0 && valid) dact[row] = d;
    } else if (!BC) {
      if (valid) {
        float* px = dx + (size_t)row * 64 + 4 * g;
#pragma unroll
        for (int c = 0; c < 4; ++c) *(f4*)(px + 16 * c) = dxn[c];
      }
    } else {
      wave_release();                        // (the dW2 reads of the staging tile are done)
      formed_handover<SLIM ? 4 : 16>(stage, accn, dx, dxn, carry, p.n, r0, r1, row0, lane, j, g);   // (SLIM: 256 registers, four rows in flight)
    }
  }

  // ---- one partial block per workgroup: [0, HW) the parameter gradients | pad | [HP, HP + n * 64) dper_n
  if (MODE != 2) {
    float* pp = partial + (size_t)blockIdx.x * pstride;
    if (BC) wave_blocks_sum<NT>(accn0, (size_t)p.n * 64, p.n * 64, pp + HP, tid);
    if (PG) head_partials<NT, HP>(sm, pp, A, nullptr, tid);
  }
}

// out[col] = sum over wavefronts of partial[w][col] in a fixed order: four strided sub-sums, then those in order, for lo <= col < hi;
// columns from `written` on are pad that the producer left alone: out[col] becomes zero there without a read of the partials
__global__ void __launch_bounds__(256) k_head_reduce(const float* __restrict__ partial, int nw, int pstride, int lo, int hi, int written,
                                                     float* __restrict__ out) {
  __shared__ float s_acc[4][64];
  const int c = threadIdx.x & 63, grp = threadIdx.x >> 6, col = lo + blockIdx.x * 64 + c;
  float acc = 0.0f;
  if (col < written) for (int i = grp; i < nw; i += 4) acc += partial[(size_t)i * pstride + col];
  s_acc[grp][c] = acc;
  __syncthreads();
  if (grp == 0 && col < hi) out[col] = (s_acc[0][c] + s_acc[1][c]) + (s_acc[2][c] + s_acc[3][c]);
}

}  // namespace mapdn

static int head_cus() {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  return cus;
}
// workgroups of a forward launch (k_head_fwd, k_twin_fwd; k_cf_baseline restates it): four wavefronts, a tile of 16 rows each per step; two per CU at most
static int head_fwd_blocks(int64_t rows) {
  const int64_t tiles = (rows + 15) / 16;
  return (int)std::max<int64_t>(1, std::min<int64_t>((tiles + 3) / 4, (int64_t)head_cus() * 2));
}
// workgroups of the backward launch: one per CU (its wavefronts keep dW2 in registers, the weights in LDS), never more wavefronts
// than units of work (groups of n formed rows / tiles of 16 rows); nw = wavefronts per workgroup (4, or 8 for the 512-thread build)
static int head_bwd_blocks(int64_t rows, int32_t n, bool bc, int nw, int cus = 0) {
  const int64_t units = bc ? rows / n : (rows + 15) / 16;
  return (int)std::max<int64_t>(1, std::min<int64_t>((units + nw - 1) / nw, cus ? cus : head_cus()));
}
static size_t head_bwd_lds(int threads, int32_t n, bool accn) {
  const int nw = threads / 64, tiles = threads == 512 ? 1 : 2;
  return (size_t)2 * 1024 * 16 + 256 * 4 + (size_t)nw * tiles * 16 * mapdn::HS * 4 + (accn ? (size_t)nw * n * 64 * 4 : 0);
}
// 512 threads (two wavefronts per SIMD) when its LDS fits a CU and the batch is big enough to give every wavefront work;
// MAPDN_HEAD_BWD_THREADS = 256 / 512 forces one (A/B measurements)
static int head_bwd_threads(int64_t rows, int32_t n, bool bc, bool accn, int cus = 0) {
  const char* e = getenv("MAPDN_HEAD_BWD_THREADS");
  const bool fits = head_bwd_lds(512, n, accn) <= (size_t)160 * 1024;
  if (e && atoi(e) == 256) return 256;
  if (e && atoi(e) == 512 && fits) return 512;
  const int64_t units = bc ? rows / n : (rows + 15) / 16;
  return fits && units >= (int64_t)(cus ? cus : head_cus()) * 8 ? 512 : 256;
}
static bool head_args_ok(const float* x, const float* per_n, int32_t n, const float* gamma, const float* beta, const float* w2, const float* b2,
                         const float* w3, const float* b3, int64_t rows) {
  if (!x || !gamma || !beta || !w2 || !b2 || !w3 || !b3 || rows < 1 || rows > 0x7fffffff) return false;
  if (per_n && (n < 1 || n > 256 || rows % n)) return false;
  return true;
}

// the kernels' view of a head: rows that are read (per_n == nullptr; n is 1 then) or formed as x[row / n] + per_n[row % n]
static mapdn::HeadArgs head_args(const float* x, const float* per_n, int32_t n, const float* gamma, const float* beta, float eps, const float* w2,
                                 const float* b2, const float* w3, const float* b3) {
  return mapdn::HeadArgs{x, per_n, per_n ? n : 1, gamma, beta, eps, w2, b2, w3, b3};
}

extern "C" int mapdn_critic_head_forward(const float* x, const float* per_n, int32_t n, const float* gamma, const float* beta, float eps,
                                         const float* w2, const float* b2, const float* w3, const float* b3, float* v, int64_t rows,
                                         void* stream) {
  using namespace mapdn;
  if (!head_args_ok(x, per_n, n, gamma, beta, w2, b2, w3, b3, rows) || !v) return MAPDN_E_INVALID;
  const HeadArgs a = head_args(x, per_n, n, gamma, beta, eps, w2, b2, w3, b3);
  const int blocks = head_fwd_blocks(rows);
  if (per_n) hipLaunchKernelGGL(k_head_fwd<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, v, (long)rows);
  else hipLaunchKernelGGL(k_head_fwd<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, v, (long)rows);
  return hipGetLastError() == hipSuccess ? MAPDN_OK : MAPDN_E_HIP;
}

extern "C" int64_t mapdn_critic_head_scratch_floats(int64_t rows, int32_t n, int32_t formed) {
  if (rows < 1 || (formed && (n < 1 || rows % n))) return 0;
  const int64_t blocks = std::max<int64_t>(head_bwd_blocks(rows, n, formed != 0, 4), head_bwd_blocks(rows, n, formed != 0, 8));
  return blocks * (mapdn::HP + (formed ? n * 64 : 0));       // one partial per workgroup (whichever launch shape the backward picks)
}

// the launch head_bwd_launch takes for (rows, n, formed, mode) — host only with cus > 0; cus = 0: the current device's CU count
extern "C" int mapdn_critic_head_backward_geometry(int64_t rows, int32_t n, int32_t formed, int32_t mode, int32_t cus, int32_t* threads,
                                                   int32_t* blocks, int32_t* lds_bytes) {
  if (rows < 1 || rows > 0x7fffffff || mode < 0 || mode > 3 || cus < 0 || (formed && (n < 1 || n > 256 || rows % n))) return MAPDN_E_INVALID;
  const bool bc = formed != 0;
  if (!bc) n = 1;
  const int c = cus ? cus : head_cus();
  const int nt = head_bwd_threads(rows, n, bc, bc && mode != 2, c);
  size_t lds = head_bwd_lds(nt, n, bc && mode != 2);
  if (mode == 0 || mode == 3) lds = std::max(lds, (size_t)(nt / 64) * mapdn::HP * 4);
  if (lds > (size_t)160 * 1024) return MAPDN_E_INVALID;        // (what the launch refuses)
  if (threads) *threads = nt;
  if (blocks) *blocks = head_bwd_blocks(rows, n, bc, nt / 64, c);
  if (lds_bytes) *lds_bytes = (int32_t)lds;
  return MAPDN_OK;
}

template <bool BC, int MODE, int NT>
static int head_bwd_launch_nt(const mapdn::HeadArgs& a, const float* dv, float* dx, const float* dot_w, float* dact, float* scratch, float* grads,
                              int64_t rows, hipStream_t st, const float* wrow, const float* scale) {
  using namespace mapdn;
  constexpr int NW = NT / 64;
  const int blocks = head_bwd_blocks(rows, a.n, BC, NW), nw = blocks;          // one partial per workgroup
  const int pstride = HP + (BC ? a.n * 64 : 0);
  size_t lds = head_bwd_lds(NT, a.n, BC && MODE != 2);
  if (MODE == 0 || MODE == 3) lds = std::max(lds, (size_t)NW * HP * 4);         // the end-of-kernel reduction across wavefronts
  if (lds > (size_t)160 * 1024) return MAPDN_E_INVALID;
  const void* fn = (const void*)k_head_bwd<BC, MODE, NT>;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return MAPDN_E_HIP;
  hipLaunchKernelGGL((k_head_bwd<BC, MODE, NT>), dim3(blocks), dim3(NT), lds, st, a, dv, dx, dot_w, dact, scratch, pstride, (long)rows, wrow, scale);
  if (MODE == 0 || MODE == 3) hipLaunchKernelGGL(k_head_reduce, dim3((HP + 63) / 64), dim3(256), 0, st, scratch, nw, pstride, 0, HP, HW, grads);
  if (BC && MODE != 2) hipLaunchKernelGGL(k_head_reduce, dim3(a.n), dim3(256), 0, st, scratch, nw, pstride, HP, HP + a.n * 64, HP + a.n * 64, grads);
  return hipGetLastError() == hipSuccess ? MAPDN_OK : MAPDN_E_HIP;
}
template <bool BC, int MODE>
static int head_bwd_launch(const mapdn::HeadArgs& a, const float* dv, float* dx, const float* dot_w, float* dact, float* scratch, float* grads,
                           int64_t rows, hipStream_t st, const float* wrow = nullptr, const float* scale = nullptr) {
  if (head_bwd_threads(rows, a.n, BC, BC && MODE != 2) == 512)
    return head_bwd_launch_nt<BC, MODE, 512>(a, dv, dx, dot_w, dact, scratch, grads, rows, st, wrow, scale);
  return head_bwd_launch_nt<BC, MODE, 256>(a, dv, dx, dot_w, dact, scratch, grads, rows, st, wrow, scale);
}

extern "C" int mapdn_critic_head_backward(const float* dv, const float* x, const float* per_n, int32_t n, const float* gamma, const float* beta,
                                          float eps, const float* w2, const float* b2, const float* w3, const float* b3, float* dx, float* grads,
                                          float* scratch, int64_t rows, int32_t param_grads, void* stream) {
  using namespace mapdn;
  if (!head_args_ok(x, per_n, n, gamma, beta, w2, b2, w3, b3, rows) || !dv || !dx || ((param_grads || per_n) && (!grads || !scratch)))
    return MAPDN_E_INVALID;
  const HeadArgs a = head_args(x, per_n, n, gamma, beta, eps, w2, b2, w3, b3);
  hipStream_t st = (hipStream_t)stream;
  if (per_n) return param_grads ? head_bwd_launch<true, 0>(a, dv, dx, nullptr, nullptr, scratch, grads, rows, st)
                                : head_bwd_launch<true, 1>(a, dv, dx, nullptr, nullptr, scratch, grads, rows, st);
  return param_grads ? head_bwd_launch<false, 0>(a, dv, dx, nullptr, nullptr, scratch, grads, rows, st)
                     : head_bwd_launch<false, 1>(a, dv, dx, nullptr, nullptr, scratch, grads, rows, st);
}

extern "C" int mapdn_critic_head_backward_dot(const float* dv, const float* x, const float* per_n, int32_t n, const float* gamma,
                                              const float* beta, float eps, const float* w2, const float* b2, const float* w3, const float* b3,
                                              const float* dot_w, float* dact, int64_t rows, void* stream) {
  using namespace mapdn;
  if (!head_args_ok(x, per_n, n, gamma, beta, w2, b2, w3, b3, rows) || !dv || !dot_w || !dact) return MAPDN_E_INVALID;
  const HeadArgs a = head_args(x, per_n, n, gamma, beta, eps, w2, b2, w3, b3);
  hipStream_t st = (hipStream_t)stream;
  return per_n ? head_bwd_launch<true, 2>(a, dv, nullptr, dot_w, dact, nullptr, nullptr, rows, st)
               : head_bwd_launch<false, 2>(a, dv, nullptr, dot_w, dact, nullptr, nullptr, rows, st);
}

// value loss and every gradient of it in one launch (no forward launch): loss = sum_rows scale[0] wrow[row / n] (ret[row] - v[row])^2
// (wrow may be NULL: weight 1) -> grads[4353]; dx / dbase, grads as mapdn_critic_head_backward with param_grads = 1
extern "C" int mapdn_critic_head_mse(const float* ret, const float* wrow, const float* scale, const float* x, const float* per_n, int32_t n,
                                     const float* gamma, const float* beta, float eps, const float* w2, const float* b2, const float* w3,
                                     const float* b3, float* dx, float* grads, float* scratch, int64_t rows, void* stream) {
  using namespace mapdn;
  if (!head_args_ok(x, per_n, n, gamma, beta, w2, b2, w3, b3, rows) || !ret || !scale || !dx || !grads || !scratch) return MAPDN_E_INVALID;
  const HeadArgs a = head_args(x, per_n, n, gamma, beta, eps, w2, b2, w3, b3);
  hipStream_t st = (hipStream_t)stream;
  return per_n ? head_bwd_launch<true, 3>(a, ret, dx, nullptr, nullptr, scratch, grads, rows, st, wrow, scale)
               : head_bwd_launch<false, 3>(a, ret, dx, nullptr, nullptr, scratch, grads, rows, st, wrow, scale);
}

#include "critic_twin.hip"      // MATD3: both heads of the twin critic on one tile (k_twin_*)
#include "critic_cf.hip"        // COMA: the counterfactual baseline, S sampled heads on one tile (k_cf_*)
#include "critic_attn.hip"      // MAAC: the attention core over the n rows of a sample (k_attn_*)
#include "critic_shap.hip"      // SQDDPG: the Shapley coalition critic, rows formed from a prefix sum over positions (k_shap_*)
