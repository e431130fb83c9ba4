// grad_sparse.hip — mapdn_action_gradients on a handle that k_nr_sparse solves (mapdn_env_config.grad_meshed = 1): a meshed
// net, or a radial one pinned to the sparse solver.  In the what-if frame (baselines_host.hpp, grad_run), per candidate:
//   k_whatif_start  ->  the solve (MODE_SOLVE)  ->  k_action_grad_sparse  ->  k_whatif_score
// The adjoint system J' lambda = c of grad.hpp is solved by the handle's own elimination program (plan.hpp SparseProg) run on the
// transposed blocks (grad_sparse.hpp): no new symbolic work, no new program.  The kernel reads the frame's Vout rows, its active set and
// its action rows and writes grad[e][k][:] only: no workspace in global memory, every block of an env lives in LDS.  The wave frame, the
// assembly ring and the program's interpreter are sparse_prog.hpp's; this file holds what the adjoint stores per entry and per row.
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

// Layout: sparse_prog.hpp's (SpWave).  One wavefront per workgroup serves L envs with S = 64 / L sub-lanes each (lane = sub * L + env); the blocks
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
  const SpWave<L> w(d, lds2);
  const unsigned s = w.s, e = w.e;
  const int n = d.n, ns = d.ns;
  const size_t Bp = (size_t)d.Bp;
  const OpfVec E{d.nrbuf + ((size_t)d.r_vout + VO_E) * Bp + e, VOF * Bp}, F{d.nrbuf + ((size_t)d.r_vout + VO_F) * Bp + e, VOF * Bp},
      VM{d.nrbuf + ((size_t)d.r_vout + VO_VM) * Bp + e, VOF * Bp};
  // c -> lambda of the env as grad.hpp's functions index it (entry m at m * L doubles): the voltage area, free once the blocks stand
  const OpfVec lam{(double*)lds2 + w.el, (size_t)L};
  const GradCfg c = {d.nbo, d.n_line, ns, d.use_line_weight, d.barrier_type, d.voltage_weight, d.q_weight, d.line_weight};
  // rows without a gradient (k_action_grad): status 3 or 2, or a q_j = lim_j a_j that is not finite
  bool has_grad = e < (unsigned)d.B && g.act[e] != 0 && g.nr_conv[e] != 0;
  for (int j = 0; j < ns; ++j) {
    const size_t o = (size_t)j * Bp + e;
    has_grad = has_grad && isfinite(q_limit(d.cur_pv[o], d.smax[j]) * g.a[o]);
  }
  // ---- 1. the converged voltage and the trash node of the padding entries; the fill slots
  sp_load_voltages(w, d);
  sp_zero_fill(w, d);
  gs_handoff();
  // ---- 2. the blocks of J', row by row (sub-lane s owns rows s, s + S, ...), from the transposed stream (GsNz: Y_ij and Y_ji)
  sp_assemble(
      w, sp_stream(t.nz, t.nz_bytes, t.rows_per_sub, t.max_nnz), [](unsigned, bool) {},
      [&](const SpRec<sizeof(GsNz)>& z, unsigned slot, d2 vi, d2 vj, double, double) {
        double br, bi;
        gs_a(vj.x, vj.y, z.ytr(), z.yti(), vi.x, vi.y, &br, &bi);                    // A_ji = V_j conj(Y_ji V_i)
        const Opf2x2 m = gs_offdiag_t(br, bi);
        d2* o = w.blk(slot);
        o[0] = d2{m.m00, m.m01}; o[1] = d2{m.m10, m.m11};
      },
      [&](unsigned i, bool live, d2, double sr, double si, double aii_r, double aii_i) {
        if (live) {
          const Opf2x2 m = gs_diag_t(sr, si, aii_r, aii_i);
          d2* dg = w.blk(i);
          dg[0] = d2{m.m00, m.m01}; dg[1] = d2{m.m10, m.m11};
        }
      });
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
    d2* rh = w.blk((unsigned)n + p);
    rh[0] = d2{lam[(size_t)p * 2], 0.0}; rh[1] = d2{lam[(size_t)p * 2 + 1], 0.0};
  }
  gs_handoff();
  // ---- 4. the program (plan.cpp::sparse_program), all phases: sub-lane s executes operation s of every phase for its L envs
  sp_run_program(w);
  gs_handoff();
  // ---- 5. the read-out: lambda of the slots n + i where grad_entry indexes it, then entry j = dr/da_j (an sgen on the slack: node == n,
  //      the direct term alone)
  for (unsigned p = s; p < (unsigned)n; p += S) {
    const d2* x = w.blk((unsigned)n + p);
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

int grad_sparse_prepare(int L) { return sp_prepare(L, [](auto l) { return k_action_grad_sparse<decltype(l)::value>; }); }

void launch_action_grad_sparse(const Dev& d, const GradState& s, const GradSparseState& t, int k, hipStream_t st) {
  sp_launch(d, d.B, st, [](auto l) { return k_action_grad_sparse<decltype(l)::value>; }, d, s, t, k);
}

}  // namespace mapdn
