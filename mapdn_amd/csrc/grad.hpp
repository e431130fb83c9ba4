// grad.hpp — the arithmetic of mapdn_action_gradients (grad.hip): the gradient of the reward that evaluate_actions
// reports with respect to the candidate's actions, by one adjoint solve on the elimination tree.  Compilable for the HOST as well:
// tests/grad_check.cpp builds this header with g++ (tests/test_action_grad_cpu.py).
//
// At the converged V the power flow is F(x, a) = S_calc(x) - S_spec(a) = 0 in x = (theta_k, u_k = d|V_k| / |V_k|) over the non-slack
// nodes.  Its Jacobian J is the block LU that opf_elim_step (opf.hpp) builds on the tree, J = L U with
//     L: unit diagonal, block (parent, k) = L_k            U: diagonal blocks D_k, block (k, parent) = J_kp
// An action a_j moves only the Q row of sgen j's node, by w_j = lim_j scaling_j / sn_mva, so dx/da_j = J^-1 w_j e_Q and
//     dr/da_j = (dr/da_j)|direct + w_j lambda_(node j, Q),      J' lambda = c,   c = dr/dx.
// J' = U' L':  U' z = c runs leaf -> root,  z_k = D_k^-T (c_k - sum over the children c of J_c,k' z_c)   (canonical child order);
//              L' lambda = z runs root -> leaf,  lambda_k = z_k - L_k' lambda_parent.
// The first sweep visits the nodes in the order of the elimination and reads only what that has left behind for the node, so
// grad_forward_step does both for a node; the second sweep is grad_backward_step.
#pragma once
#include "nrmath.hpp"   // barrier_deriv, sign0
#include "opf.hpp"

namespace mapdn {

// the weights of the reward and the sizes its means run over (whatif.hpp WhatifCfg) and the barrier type
struct GradCfg {
  int n_bus, n_line, n_sgen, use_line_weight, barrier_type;
  double voltage_weight, q_weight, line_weight;
};

// c_k of the barrier term: r has -voltage_weight mean_b barrier(|V_b|), and d|V_k| = |V_k| du_k
OPF_FN double grad_barrier_rhs(const GradCfg& c, double vm) {
  return -(c.voltage_weight / (double)c.n_bus) * barrier_deriv(c.barrier_type, vm) * vm;
}

// d pl / d(theta_f, u_f, theta_t, u_t) of one net.line row, per unit: pl = gff |Vf|^2 + gtt |Vt|^2 + gs wr + bd wi with
// wr + j wi = Vf conj(Vt) (plan.hpp LineFlow, the expression of k_whatif_score).  d/dtheta_f turns W by +j, d/dtheta_t by -j, both u scale it.
OPF_FN void grad_line(const double* lc, double ef, double ff, double et, double ft, double* dthf, double* duf, double* dtht, double* dut) {
  const double gff = lc[0], gtt = lc[1], gs = lc[2], bd = lc[3];
  const double wr = ef * et + ff * ft, wi = ff * et - ef * ft;
  const double cross = gs * wr + bd * wi, turn = bd * wr - gs * wi;
  *dthf = turn; *dtht = -turn;
  *duf = 2.0 * gff * (ef * ef + ff * ff) + cross;
  *dut = 2.0 * gtt * (et * et + ft * ft) + cross;
}

// Node k, leaf -> root: its elimination step (opf.hpp), then z_k into lam[2k], lam[2k + 1], which hold c_k on entry.
OPF_FN void grad_forward_step(int k, int n, const int32_t* par, const int32_t* cptr, const int32_t* cidx, const double* yt, const OpfVec& e,
                              const OpfVec& f, const OpfVec& fac, const OpfVec& lam) {
  double P, Q;
  opf_elim_step(k, n, par, cptr, cidx, yt, e, f, fac, &P, &Q);
  double s0 = 0.0, s1 = 0.0;
  for (int i = cptr[k]; i < cptr[k + 1]; ++i) {
    const int c = cidx[i];
    Opf2x2 J; opf_load4(fac, (size_t)c * OPF_FAC + OF_JKP, &J);
    const double z0 = lam[(size_t)c * 2], z1 = lam[(size_t)c * 2 + 1];
    s0 += J.m00 * z0 + J.m10 * z1; s1 += J.m01 * z0 + J.m11 * z1;
  }
  const double r0 = lam[(size_t)k * 2] - s0, r1 = lam[(size_t)k * 2 + 1] - s1;
  Opf2x2 Di; opf_load4(fac, (size_t)k * OPF_FAC + OF_DINV, &Di);
  lam[(size_t)k * 2] = Di.m00 * r0 + Di.m10 * r1; lam[(size_t)k * 2 + 1] = Di.m01 * r0 + Di.m11 * r1;
}

// Node k, root -> leaf: lambda_k = z_k - L_k' lambda_parent
OPF_FN void grad_backward_step(int k, int p, int n, const OpfVec& fac, const OpfVec& lam) {
  if (p >= n) return;
  Opf2x2 L; opf_load4(fac, (size_t)k * OPF_FAC + OF_L, &L);
  const double x0 = lam[(size_t)p * 2], x1 = lam[(size_t)p * 2 + 1];
  lam[(size_t)k * 2] -= L.m00 * x0 + L.m10 * x1; lam[(size_t)k * 2 + 1] -= L.m01 * x0 + L.m11 * x1;
}

// J' lambda = c in place (lam: c on entry), factorising J at (e, f) on the way
OPF_FN void grad_adjoint(int n, const int32_t* par, const int32_t* cptr, const int32_t* cidx, const double* yt, const OpfVec& e, const OpfVec& f,
                         const OpfVec& fac, const OpfVec& lam) {
  for (int k = 0; k < n; ++k) grad_forward_step(k, n, par, cptr, cidx, yt, e, f, fac, lam);
  for (int k = n - 1; k >= 0; --k) grad_backward_step(k, par[k], n, fac, lam);
}

// The line-loss term of c: r has -line_weight mean_l pl_mw_l.  line l: its constants lc, the positions of its ends (n: the slack, whose
// row Vout keeps too; an out-of-service line has both ends there and zero constants).  Added line by line, in the order of net.line.
OPF_FN void grad_line_rhs(const GradCfg& c, double sn, const double* lc, int fpos, int tpos, int n, const OpfVec& e, const OpfVec& f, const OpfVec& lam) {
  double dthf, duf, dtht, dut;
  grad_line(lc, e[fpos], f[fpos], e[tpos], f[tpos], &dthf, &duf, &dtht, &dut);
  const double s = -(c.line_weight / (double)c.n_line) * sn;
  if (fpos < n) { lam[(size_t)fpos * 2] += s * dthf; lam[(size_t)fpos * 2 + 1] += s * duf; }
  if (tpos < n) { lam[(size_t)tpos * 2] += s * dtht; lam[(size_t)tpos * 2 + 1] += s * dut; }
}

// Entry j of the gradient: the direct term -q_weight mean_j |q_j scaling_j| (q_j = lim_j a_j; sign(0) = 0; absent with line_weight),
// plus w_j lambda_Q of the sgen's node (node >= n: the slack, whose voltage no action moves — the power-flow part is exactly 0)
OPF_FN double grad_entry(const GradCfg& c, double sn, double lim, double scale, double a, int node, int n, const OpfVec& lam) {
  double g = 0.0;
  if (!c.use_line_weight) g = -(c.q_weight / (double)c.n_sgen) * sign0(lim * a * scale) * (lim * scale);
  if (node < n) g += (lim * scale / sn) * lam[(size_t)node * 2 + 1];
  return g;
}

}  // namespace mapdn
