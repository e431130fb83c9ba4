// grad_sparse.hip — mapdn_action_gradients on a handle that k_nr_sparse solves (mapdn_env_config.grad_meshed = 1): a meshed
// net, or a radial one pinned to the sparse solver.  In the what-if frame (baselines_host.hpp, grad_run), per candidate:
//   k_whatif_start  ->  the solve (MODE_SOLVE)  ->  k_action_grad_sparse  ->  k_whatif_score
// The adjoint system J' lambda = c of grad.hpp is solved by the handle's own elimination program (plan.hpp SparseProg) run on the
// transposed blocks (grad_sparse.hpp): no new symbolic work, no new program.  The kernel reads the frame's Vout rows, its active set and
// its action rows and writes grad[e][k][:] only: no workspace in global memory, every block of an env lives in LDS.
// Included at the end of kernels.hip (one translation unit) like grad.hip, which keeps exactly k_action_grad.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "nr_common.hpp"
#include "grad.hpp"
#include "grad_sparse.hpp"
#include "sparse_prog.hpp"

namespace mapdn {

// Layout: k_nr_sparse's.  One wavefront per workgroup serves L envs with S = 64 / L sub-lanes each (lane = sub * L + env); the blocks
// live in LDS as [slot][env][2x2] behind the [n + 2] voltages, nr_sparse_lds_bytes in all, so every geometry that fits the solver fits
// the gradient.  Control flow is wave-uniform: an env without a gradient (frozen, not converged, a non-finite q) runs the program on
// whatever its own slots hold and differs in the read-out alone.  A stage that reads what other lanes of the wave wrote to LDS waits
// for those writes (gs_handoff: a wait, no barrier — there is one wavefront).  Every sum of an env runs in one lane in an order the
// net fixes (the assembly row, the program, the lines of net.line walked by sub-lane 0), whatever B, K and the env's place are.

template <int L>
__global__ void __launch_bounds__(64)
k_action_grad_sparse(Dev d, GradState g, GradSparseState t, int k) {
  extern __shared__ d2 lds2[];
  constexpr unsigned S = 64u / L;
  const unsigned lane = threadIdx.x, s = lane / L, el = lane % L;
  const unsigned e = blockIdx.x * L + el;                          // < Bp: every per-env array has a row for it
  const int n = d.n, ns = d.ns;
  const size_t Bp = (size_t)d.Bp;
  d2* sV = lds2 + el;                                              // sV[k * L] = (e, f); k = n slack, n + 1 trash
  d2* sB = lds2 + (size_t)(n + 2) * L + 2u * el;                   // block b: sB[b * 2L], sB[b * 2L + 1] = rows (a00 a01), (a10 a11)
  auto blk = [&](unsigned b) { return sB + (size_t)b * (2u * L); };
  const OpfVec E{d.nrbuf + ((size_t)d.r_vout + VO_E) * Bp + e, VOF * Bp}, F{d.nrbuf + ((size_t)d.r_vout + VO_F) * Bp + e, VOF * Bp},
      VM{d.nrbuf + ((size_t)d.r_vout + VO_VM) * Bp + e, VOF * Bp};
  // c -> lambda of the env as grad.hpp's functions index it (entry m at m * L doubles): the voltage area, free once the blocks stand
  const OpfVec lam{(double*)lds2 + el, (size_t)L};
  const GradCfg c = {d.nbo, d.n_line, ns, d.use_line_weight, d.barrier_type, d.voltage_weight, d.q_weight, d.line_weight};
  // rows without a gradient (k_action_grad): status 3 or 2, or a q_j = lim_j a_j that is not finite
  bool has_grad = e < (unsigned)d.B && g.act[e] != 0 && g.nr_conv[e] != 0;
  for (int j = 0; j < ns; ++j) {
    const size_t o = (size_t)j * Bp + e;
    has_grad = has_grad && isfinite(q_limit(d.cur_pv[o], d.smax[j]) * g.a[o]);
  }
  const __amdgpu_buffer_rsrc_t rsO = __builtin_amdgcn_make_buffer_rsrc(const_cast<SpOp*>(d.sp_ops), 0, d.sp_ops_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsZ = __builtin_amdgcn_make_buffer_rsrc(const_cast<GsNz*>(t.nz), 0, t.nz_bytes, 0x00020000);
  const int RPS = t.rows_per_sub, MNZ = t.max_nnz, NPH = d.sp_phases;
  const unsigned voO = s * 16u;                                    // this sub-lane's op of phase p: + p * S * 16
  const unsigned voZ = s * (unsigned)RPS * (unsigned)MNZ * 48u;    // the entries of its assembly rows
  // ---- 1. the converged voltage (the frame's Vout rows, the slack's included); the trash node of the padding entries; the fill slots
  for (unsigned p = s; p < (unsigned)n + 2u; p += S) sV[(size_t)p * L] = p <= (unsigned)n ? d2{E[p], F[p]} : d2{0.0, 0.0};
  for (unsigned q = s; q < (unsigned)d.sp_fill; q += S) {
    d2* f = blk((unsigned)d.sp_fill_slots[q]);
    f[0] = d2{0.0, 0.0}; f[1] = d2{0.0, 0.0};
  }
  gs_handoff();
  // ---- 2. the blocks of J', row by row (sub-lane s owns rows s, s + S, ...): one stream of RPS * MNZ entries per sub-lane, read through
  //      a ring that runs PF entries ahead of the arithmetic, as k_nr_sparse reads its own
  {
    constexpr int PF = 8;
    const int T = RPS * MNZ;
    u32x4 zq0[PF], zq1[PF]; u32x2 zq2[PF];
    auto zload = [&](int tt, u32x4& z0, u32x4& z1, u32x2& z2) {
      const unsigned so = __builtin_amdgcn_readfirstlane((unsigned)min(tt, T - 1) * 48u);
      z0 = __builtin_amdgcn_raw_buffer_load_b128(rsZ, voZ, so, 0);                 // col, slot, Re Y_ij
      z1 = __builtin_amdgcn_raw_buffer_load_b128(rsZ, voZ + 16u, so, 0);           // Im Y_ij, Re Y_ji
      z2 = __builtin_amdgcn_raw_buffer_load_b64(rsZ, voZ + 32u, so, 0);            // Im Y_ji
    };
#pragma unroll
    for (int u = 0; u < PF; ++u) zload(u, zq0[u], zq1[u], zq2[u]);
    int r = 0, q = 0;
    unsigned i = s;
    bool live = i < (unsigned)n;
    d2 vi = sV[(size_t)(live ? i : (unsigned)n + 1u) * L];
    double sr = 0.0, si = 0.0, aii_r = 0.0, aii_i = 0.0;
    for (int t0 = 0; t0 < T; t0 += PF) {
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const int tt = t0 + u;
        if (tt < T) {                            // (uniform; no `break`: the loop must unroll for the ring to stay in registers)
        const u32x4 z0 = zq0[u], z1 = zq1[u]; const u32x2 z2 = zq2[u];
        zload(tt + PF, zq0[u], zq1[u], zq2[u]);
        const double yr = __hiloint2double((int)z0.w, (int)z0.z), yi = __hiloint2double((int)z1.y, (int)z1.x);
        const double ytr = __hiloint2double((int)z1.w, (int)z1.z), yti = __hiloint2double((int)z2.y, (int)z2.x);
        const unsigned col = z0.x;
        const int slot = (int)z0.y;
        const d2 vj = sV[(size_t)col * L];
        double ar, ai;
        gs_a(vi.x, vi.y, yr, yi, vj.x, vj.y, &ar, &ai);                            // A_ij: the row sum S_i and A_ii
        sr += ar; si += ai;
        if (col == i) { aii_r = ar; aii_i = ai; }
        if (slot >= 0) {
          double br, bi;
          gs_a(vj.x, vj.y, ytr, yti, vi.x, vi.y, &br, &bi);                        // A_ji = V_j conj(Y_ji V_i)
          const Opf2x2 m = gs_offdiag_t(br, bi);
          d2* o = blk((unsigned)slot);
          o[0] = d2{m.m00, m.m01}; o[1] = d2{m.m10, m.m11};
        }
        if (++q == MNZ) {                        // (uniform) end of the row: the diagonal block; next row
          if (live) {
            const Opf2x2 m = gs_diag_t(sr, si, aii_r, aii_i);
            d2* dg = blk(i);
            dg[0] = d2{m.m00, m.m01}; dg[1] = d2{m.m10, m.m11};
          }
          q = 0; ++r;
          i = (unsigned)r * S + s;
          live = i < (unsigned)n && r < RPS;
          vi = sV[(size_t)(live ? i : (unsigned)n + 1u) * L];
          sr = si = aii_r = aii_i = 0.0;
        }
        }
      }
    }
  }
  gs_handoff();
  // ---- 3. the right-hand side c (grad.hpp): the barrier term of every node, then the line terms in the order of net.line by ONE
  //      sub-lane of the env — two lines may meet at a node, and its sum must not depend on S —, then c into the slots n + i as [c | 0]
  for (unsigned p = s; p < (unsigned)n; p += S) { lam[(size_t)p * 2] = 0.0; lam[(size_t)p * 2 + 1] = grad_barrier_rhs(c, VM[p]); }
  gs_handoff();
  if (c.use_line_weight && s == 0)
    for (int l = 0; l < d.n_line; ++l) {
      const LineFlow Lf = d.lines[l];
      grad_line_rhs(c, d.sn, Lf.c, Lf.fpos, Lf.tpos, n, E, F, lam);
    }
  gs_handoff();
  for (unsigned p = s; p < (unsigned)n; p += S) {
    d2* rh = blk((unsigned)n + p);
    rh[0] = d2{lam[(size_t)p * 2], 0.0}; rh[1] = d2{lam[(size_t)p * 2 + 1], 0.0};
  }
  gs_handoff();
  // ---- 4. the program (plan.cpp::sparse_program), all phases: sub-lane s executes operation s of every phase for its L envs
  //      (sparse_prog.hpp: the interpreter of k_nr_sparse without its per-env `done` mask)
  sp_run_program<L>(sB, rsO, voO, NPH);
  gs_handoff();
  // ---- 5. the read-out: lambda of the slots n + i where grad_entry indexes it, then entry j = dr/da_j (an sgen on the slack: node == n,
  //      the direct term alone)
  for (unsigned p = s; p < (unsigned)n; p += S) {
    const d2* x = blk((unsigned)n + p);
    lam[(size_t)p * 2] = x[0].x; lam[(size_t)p * 2 + 1] = x[1].x;
  }
  gs_handoff();
  if (e < (unsigned)d.B) {
    double* __restrict__ out = g.grad + ((size_t)e * g.K + k) * ns;
    for (int j = (int)s; j < ns; j += (int)S) {
      const size_t o = (size_t)j * Bp + e;
      out[j] = has_grad ? grad_entry(c, d.sn, q_limit(d.cur_pv[o], d.smax[j]), d.sgen_scale[j], g.a[o], g.sg_node[j], n, lam) : __builtin_nan("");
    }
  }
}

#define SP_FOR_EACH(X) X(16) X(8) X(4) X(2)
int grad_sparse_prepare(int L) {
#define X(l) if (L == l) return hipFuncSetAttribute((const void*)k_action_grad_sparse<l>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess ? 0 : -1;
  SP_FOR_EACH(X)
#undef X
  return -2;
}

void launch_action_grad_sparse(const Dev& d, const GradState& s, const GradSparseState& t, int k, hipStream_t st) {
  const size_t lds = nr_sparse_lds_bytes(d.n, d.sp_blocks, d.sp_lanes);
#define X(l) if (d.sp_lanes == l) { hipLaunchKernelGGL((k_action_grad_sparse<l>), dim3((d.B + l - 1) / l), dim3(64), lds, st, d, s, t, k); return; }
  SP_FOR_EACH(X)
#undef X
}
#undef SP_FOR_EACH

}  // namespace mapdn
