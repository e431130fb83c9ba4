// vjp.hip — mapdn_voltage_vjp: for every candidate that mapdn_evaluate_actions would score, the product of M cotangents
// over the bus voltages (|V| and the angle) with the Jacobian of those voltages by the candidate's actions, by ONE factorisation and M
// adjoint solves per (env, candidate) on the elimination tree.  In the what-if frame (baselines_host.hpp, vjp_run), per candidate:
//   k_whatif_start  ->  the solve (MODE_SOLVE)  ->  k_voltage_vjp  ->  k_whatif_score
// and after the last candidate k_vjp_mask, when the caller asked for vm_pu.  k_voltage_vjp reads the frame's Vout rows, its active set and
// its action rows and writes the workspace of k_action_grad (GradState: fac, lam), grad[e][k][:][:] and va_degree[e][k][:] only, so the
// scoring launch after it sees what it sees in mapdn_evaluate_actions.  The arithmetic is in vjp.hpp.
// Included at the end of kernels.hip (one translation unit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "vjp.hpp"

namespace mapdn {

// Layout: k_action_grad's (grad.hip) — one lane per env, VJP_WG = 64 consecutive envs per one-wave workgroup, every sum of a row in its
// own lane in the order of the plan, no atomics.  The caller's cotangents are env-major, [B][K][M][nbo]: a lane reading its own row would
// touch one 8-byte word per 64-byte line.  So the wave moves them through LDS, VJP_TILE buses of its 64 envs at a time: eight lanes read
// VJP_TILE consecutive doubles of one env's row (one 64-byte line), the tile is stored [env][bus] with one word of padding (9 KiB for both
// cotangents, so that LDS does not bound the waves per SIMD), and lane e then reads row e of the tile.  The tile carries values from
// global memory to the lane that owns the env and nothing else: no value of one env meets a value of another, so a row's bits are those
// of a lane that read its cotangents directly.
constexpr int VJP_WG = 64, VJP_TILE = 8;

__global__ void __launch_bounds__(VJP_WG) k_voltage_vjp(Dev d, GradState s, VjpState v, int k) {
  __shared__ double tile[2][VJP_WG][VJP_TILE + 1];
  const int lane = (int)threadIdx.x, e0 = (int)blockIdx.x * VJP_WG, e = e0 + lane;
  const int n = d.n, ns = d.ns, nbo = d.nbo, M = v.M;
  const size_t Bp = (size_t)d.Bp;
  const bool valid = e < d.B;
  // status 3 or 2, or a solved row whose q_j = lim_j a_j is not finite for some j (k_action_grad's rule): NaN rows
  bool has = valid && s.act[e] != 0 && s.nr_conv[e] != 0;
  if (has)
    for (int j = 0; j < ns; ++j) {
      const size_t o = (size_t)j * Bp + e;
      has = has && isfinite(q_limit(d.cur_pv[o], d.smax[j]) * s.a[o]);
    }
  const size_t ev = valid ? (size_t)e : 0;                       // (a lane past the batch holds pointers of env 0 and never follows them)
  const OpfVec E{d.nrbuf + ((size_t)d.r_vout + VO_E) * Bp + ev, VOF * Bp}, F{d.nrbuf + ((size_t)d.r_vout + VO_F) * Bp + ev, VOF * Bp},
      VM{d.nrbuf + ((size_t)d.r_vout + VO_VM) * Bp + ev, VOF * Bp};
  const OpfVec fac{s.fac + ev, Bp}, lam{s.lam + ev, Bp};
  const size_t row = ev * v.K + k;
  if (valid && v.va_out) {                                       // position n, the slack, holds vroot + 0j (alloc_nrbuf)
    double* __restrict__ va = v.va_out + row * nbo;
    for (int b = 0; b < nbo; ++b) {
      const int p = d.pos_of_obus[b];
      va[b] = has ? vjp_va_degree(E[p], F[p]) : __builtin_nan("");
    }
  }
  if (M == 0) return;                                            // (uniform: no lane waits at a barrier below)
  if (has) vjp_factorise(n, s.par, s.cptr, s.cidx, s.yt, E, F, fac);
  for (int m = 0; m < M; ++m) {
    // c of cotangent m into lam, VJP_TILE buses at a time.  The slack's entries are staged like the others and never read.
    for (int b0 = 0; b0 < nbo; b0 += VJP_TILE) {
      const int t = lane % VJP_TILE, b = b0 + t;
      __syncthreads();                                           // the tile's last readers are done
      for (int r = lane / VJP_TILE; r < VJP_WG; r += VJP_WG / VJP_TILE) {
        const int er = e0 + r;
        if (er < d.B && b < nbo) {
          const size_t o = (((size_t)er * v.K + k) * M + m) * nbo + b;
          tile[0][r][t] = v.cot_vm ? v.cot_vm[o] : 0.0;
          tile[1][r][t] = v.cot_va ? v.cot_va[o] : 0.0;
        }
      }
      __syncthreads();
      if (has) {
        const int tn = min(VJP_TILE, nbo - b0);
        for (int i = 0; i < tn; ++i) {
          const int p = d.pos_of_obus[b0 + i];
          if (p < n) vjp_rhs(p, tile[0][lane][i], tile[1][lane][i], VM[p], lam);
        }
      }
    }
    double* __restrict__ out = v.grad + (row * M + m) * ns;
    if (has) {
      vjp_adjoint(n, s.par, s.cptr, s.cidx, fac, lam);
      for (int j = 0; j < ns; ++j) {
        const size_t o = (size_t)j * Bp + e;
        out[j] = vjp_entry(d.sn, q_limit(d.cur_pv[o], d.smax[j]), d.sgen_scale[j], s.sg_node[j], n, lam);
      }
    } else if (valid) {
      for (int j = 0; j < ns; ++j) out[j] = __builtin_nan("");
    }
  }
}

// After the last candidate: the |V| row of a solved (env, candidate) in which some lim_j a_j is not finite becomes NaN like its grad and
// va_degree rows (the predicate of k_voltage_vjp on the caller's own actions, widened as k_whatif_start widens them).  One thread per
// (env, candidate); every other row keeps the bits k_whatif_score wrote.
template <typename AT>
__global__ void __launch_bounds__(256) k_vjp_mask(Dev d, int K, const AT* __restrict__ actions, const uint8_t* __restrict__ status, double* __restrict__ vm_pu) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)d.B * K) return;
  if (status[i] != WHATIF_SOLVED) return;
  const size_t e = i / (size_t)K, Bp = (size_t)d.Bp;
  bool q_finite = true;
  for (int j = 0; j < d.ns; ++j) q_finite = q_finite && isfinite(q_limit(d.cur_pv[(size_t)j * Bp + e], d.smax[j]) * (double)actions[i * d.ns + j]);
  if (q_finite) return;
  for (int b = 0; b < d.nbo; ++b) vm_pu[i * d.nbo + b] = __builtin_nan("");
}

void launch_voltage_vjp(const Dev& d, const GradState& s, const VjpState& v, int k, hipStream_t st) {
  hipLaunchKernelGGL(k_voltage_vjp, dim3((d.B + VJP_WG - 1) / VJP_WG), dim3(VJP_WG), 0, st, d, s, v, k);
}
void launch_vjp_mask(const Dev& d, int K, const void* actions, int dtype, const uint8_t* status, double* vm_pu, hipStream_t st) {
  const dim3 grid((unsigned)(((size_t)d.B * K + 255) / 256)), block(256);
  if (dtype == MAPDN_F32) hipLaunchKernelGGL(k_vjp_mask<float>, grid, block, 0, st, d, K, (const float*)actions, status, vm_pu);
  else hipLaunchKernelGGL(k_vjp_mask<double>, grid, block, 0, st, d, K, (const double*)actions, status, vm_pu);
}

}  // namespace mapdn
