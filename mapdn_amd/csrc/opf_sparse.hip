// opf_sparse.hip — the linearisation of the OPF baseline on a handle that k_nr_sparse solves (mapdn_opf_config.meshed = 1):
// a meshed net, or a radial one pinned to the sparse solver.  In the loop of opf.hip, in place of k_opf_linearise:
//   the solve (MODE_SOLVE)  ->  k_opf_sens_sparse (S and dV, by the handle's elimination program)  ->  k_opf_reduce_sparse (M V, loss,
//   violation, W = M dV, g, H)  ->  k_opf_qp  ->  k_opf_update
// with OpfState's workspace in the tree's layouts (no fac), so that k_opf_qp and k_opf_update run as they are.  The arithmetic is in
// opf_sparse.hpp; the wave frame, the assembly ring and the program's interpreter are sparse_prog.hpp's.  Included at the end of
// kernels.hip (one translation unit) like grad_sparse.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "ctlloop.hpp"
#include "nr_common.hpp"
#include "opf_sparse.hpp"
#include "sparse_prog.hpp"

namespace mapdn {

// Layout: sparse_prog.hpp's (SpWave).  One wavefront per workgroup serves L envs with S = 64 / L sub-lanes each (lane =
// sub * L + env); the blocks live in LDS as [slot][env][2x2] behind the [n + 2] voltages, nr_sparse_lds_bytes in all.  Control flow is
// wave-uniform: an env that is not linearised (stopped, or its power flow failed) runs the program on whatever its own slots hold and
// writes nothing.  The program factorises in place, so every PAIR of columns (j, j + 1) assembles the blocks again; the two columns
// ride in the two columns of the right-hand-side blocks, which the block operations never mix.  Hand-offs between the lanes are
// gs_handoff (a wait, no barrier: one wavefront); no atomics.  Every sum of an env runs in one lane in an order the net fixes.
template <int L>
__global__ void __launch_bounds__(64)
k_opf_sens_sparse(Dev d, OpfState o) {
  extern __shared__ d2 lds2[];
  constexpr unsigned S = 64u / L;
  const SpWave<L> w(d, lds2);
  const unsigned s = w.s, e = w.e;
  const int n = d.n, ns = d.ns;
  const size_t Bp = (size_t)d.Bp;
  const OpfVec VM{d.nrbuf + ((size_t)d.r_vout + VO_VM) * Bp + e, VOF * Bp};
  const bool go = e < (unsigned)d.B && o.act[e] != 0 && o.nr_conv[e] != 0;
  const auto nz = sp_stream(d.sp_nz, d.sp_nz_bytes, d.sp_rows_per_sub, d.sp_max_nnz);   // the stream k_nr_sparse assembles from
  // ---- the converged voltage and the trash node of the padding entries
  sp_load_voltages(w, d);
  for (int j = 0; j < ns; j += 2) {                                // (uniform)
    // ---- 1. the fill slots and ALL right-hand-side slots: zero
    gs_handoff();                                                  // (the read-out of the pair before; the voltages)
    sp_zero_fill(w, d);
    for (unsigned p = s; p < (unsigned)n; p += S) {
      d2* rh = w.blk((unsigned)n + p);
      rh[0] = d2{0.0, 0.0}; rh[1] = d2{0.0, 0.0};
    }
    gs_handoff();
    // ---- 2. the blocks of J, row by row (sub-lane s owns rows s, s + S, ...).  (No gen buses here: opf_resolve refuses them.)
    sp_assemble(
        w, nz, [](unsigned, bool) {},
        [&](const SpRec<sizeof(SpNz)>&, unsigned slot, d2, d2, double ar, double ai) {
          const Opf2x2 m = gs_offdiag(ar, ai);
          d2* ob = w.blk(slot);
          ob[0] = d2{m.m00, m.m01}; ob[1] = d2{m.m10, m.m11};
        },
        [&](unsigned i, bool live, d2, double sr, double si, double aii_r, double aii_i) {
          if (live) {
            const Opf2x2 m = gs_diag(sr, si, aii_r, aii_i);
            d2* dg = w.blk(i);
            dg[0] = d2{m.m00, m.m01}; dg[1] = d2{m.m10, m.m11};
          }
        });
    // ---- 3. the two columns: w e_Q of sgen j in column 0 of the slot of its node, of sgen j + 1 in column 1 of the slot of its (an sgen
    //      on the slack, node == n: a zero column; two sgens of one node share a slot).  One sub-lane, after the zeroing above.
    if (s == 0) {
      for (int c = 0; c < 2 && j + c < ns; ++c) {
        const int node = o.sg_node[j + c];
        const size_t oo = (size_t)(j + c) * Bp + e;
        const double wq = q_limit(d.cur_pv[oo], d.smax[j + c]) * d.sgen_scale[j + c] / d.sn;
        if (node < n) {
          d2* rh = w.blk((unsigned)(n + node));
          if (c == 0) rh[1].x = wq; else rh[1].y = wq;
        }
      }
    }
    gs_handoff();
    // ---- 4. the program, all phases
    sp_run_program(w);
    gs_handoff();
    // ---- 5. (dtheta, u) of both columns from the slots n + i: S = u |V| and dV = (u + j dtheta) V, in k_opf_linearise's layouts
    if (go) {
      const size_t xs = (size_t)ns * 2;
      for (unsigned p = s; p < (unsigned)n; p += S) {
        const d2* x = w.blk((unsigned)n + p);
        const d2 th = x[0], u = x[1], v = w.sV[(size_t)p * L];
        const double vm = VM[p];
        o.S[((size_t)p * ns + j) * Bp + e] = u.x * vm;
        double* X0 = o.X + ((size_t)j * 2 + (size_t)p * xs) * Bp + e;
        X0[0] = u.x * v.x - th.x * v.y; X0[Bp] = u.x * v.y + th.x * v.x;
        if (j + 1 < ns) {
          o.S[((size_t)p * ns + j + 1) * Bp + e] = u.y * vm;
          X0[2 * Bp] = u.y * v.x - th.y * v.y; X0[3 * Bp] = u.y * v.y + th.y * v.x;
        }
      }
    }
  }
}

// After k_opf_sens_sparse, in the frame's layout (ctlloop.hpp: DL envs x DS sub-lanes): the sums of k_opf_linearise with M applied row
// by row from the table (opf_sparse.hpp) — M V, the violation and lin; then the loss and per column W = M dV and g; then H, written
// symmetrically.  An env that is not linearised gets lin = 0 and nothing else.
__global__ void __launch_bounds__(DL * DS) k_opf_reduce_sparse(Dev d, OpfState s, OsM m) {
  const int el = (int)threadIdx.x % DL, sl = (int)threadIdx.x / DL;
  const int e = (int)blockIdx.x * DL + el;
  const bool go = e < d.B && s.act[e] != 0 && s.nr_conv[e] != 0;
  const size_t Bp = (size_t)d.Bp;
  const int n = d.n, ns = d.ns;
  const size_t ee = go ? (size_t)e : 0;
  const OpfVec E{d.nrbuf + ((size_t)d.r_vout + VO_E) * Bp + ee, VOF * Bp}, F{d.nrbuf + ((size_t)d.r_vout + VO_F) * Bp + ee, VOF * Bp},
      VM{d.nrbuf + ((size_t)d.r_vout + VO_VM) * Bp + ee, VOF * Bp};
  const OpfVec mv{s.mv + ee, Bp};
  const size_t xs = (size_t)ns * 2;
  if (go) {
    for (int k = sl; k < n; k += DS) os_mv_row(m, k, E, F, mv);
    if (sl == 0) {
      double viol = 0.0;
      for (int k = 0; k < n; ++k) {
        const double v = VM[k];
        viol = fmax(viol, fmax(v - s.v_upper, s.v_lower - v));
      }
      s.viol[e] = viol;
      s.lin[e] = 1;
    }
  } else if (e < d.B && sl == 0) s.lin[e] = 0;
  __syncthreads();
  if (go) {
    if (sl == DS - 1) s.loss[e] = os_loss(m, n, s.loss_slack, E, F, mv);
    for (int j = sl; j < ns; j += DS) {
      const OpfVec x{s.X + (size_t)j * 2 * Bp + ee, Bp}, w{s.W + (size_t)j * 2 * Bp + ee, Bp};
      s.g[(size_t)j * Bp + ee] = os_column(m, n, x, w, mv, xs);
    }
  }
  __syncthreads();
  if (go)
    for (int j = sl; j < ns; j += DS) {
      const OpfVec w{s.W + (size_t)j * 2 * Bp + ee, Bp};
      for (int i = 0; i <= j; ++i) {
        const double h = os_h(n, OpfVec{s.X + (size_t)i * 2 * Bp + ee, Bp}, w, xs);
        s.H[((size_t)i * ns + j) * Bp + ee] = h; s.H[((size_t)j * ns + i) * Bp + ee] = h;
      }
    }
}

int opf_sparse_prepare(int L) { return sp_prepare(L, [](auto l) { return k_opf_sens_sparse<decltype(l)::value>; }); }

void launch_opf_linearise_sparse(const Dev& d, const OpfState& s, const OsM& m, hipStream_t st) {
  sp_launch(d, d.B, st, [](auto l) { return k_opf_sens_sparse<decltype(l)::value>; }, d, s);
  hipLaunchKernelGGL(k_opf_reduce_sparse, dim3((d.B + DL - 1) / DL), dim3(DL * DS), 0, st, d, s, m);
}

}  // namespace mapdn
