// vjp.hpp — the arithmetic of mapdn_voltage_vjp (vjp.hip): the vector-Jacobian product of the bus voltages that a candidate
// action would commit, by the actions, for cotangents the caller supplies.  Compilable for the HOST as well: tests/vjp_check.cpp builds
// this header with g++ (tests/test_voltage_vjp_cpu.py).
//
// §22's system with another right-hand side.  x = (theta_p, u_p = d|V_p| / |V_p|) over the non-slack nodes, J = L U the block LU of
// opf_elim_step; for one cotangent (cot_vm, cot_va) over the buses
//     c_theta(p) = cot_va[bus(p)] 180 / pi        (va_degree = theta 180 / pi)
//     c_u(p)     = cot_vm[bus(p)] |V_p|           (d|V_p| = |V_p| du_p)
//     J' lambda = c,        grad_j = w_j lambda_(node j, Q),   w_j = lim_j scaling_j / sn_mva.
// There is no direct term: an action reaches the voltages through the power flow alone.  The factors do not depend on c, so J is
// factorised once (vjp_factorise) and every cotangent costs the two transposed sweeps on the stored factors (vjp_adjoint):
//     U' z = c  leaf -> root   (vjp_ut_step: the second half of grad_forward_step, without the elimination before it)
//     L' lambda = z  root -> leaf   (grad_backward_step)
#pragma once
#include "grad.hpp"

namespace mapdn {

#define VJP_DEG_PER_RAD (180.0 / 3.14159265358979323846)

// J = L U at (e, f) into fac, leaf -> root (S_k, which the elimination returns on the way, is not needed)
OPF_FN void vjp_factorise(int n, const int32_t* par, const int32_t* cptr, const int32_t* cidx, const double* yt, const OpfVec& e, const OpfVec& f,
                          const OpfVec& fac) {
  double P, Q;
  for (int k = 0; k < n; ++k) opf_elim_step(k, n, par, cptr, cidx, yt, e, f, fac, &P, &Q);
}

// c of node p from the cotangent entries of its bus
OPF_FN void vjp_rhs(int p, double cot_vm, double cot_va, double vm, const OpfVec& lam) {
  lam[(size_t)p * 2] = cot_va * VJP_DEG_PER_RAD;
  lam[(size_t)p * 2 + 1] = cot_vm * vm;
}

// Node k of U' z = c, leaf -> root, on stored factors: z_k = D_k^-T (c_k - sum over the children c of J_c,k' z_c), canonical child order
OPF_FN void vjp_ut_step(int k, const int32_t* cptr, const int32_t* cidx, const OpfVec& fac, const OpfVec& lam) {
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

// J' lambda = c in place on the factors vjp_factorise left (lam: c on entry)
OPF_FN void vjp_adjoint(int n, const int32_t* par, const int32_t* cptr, const int32_t* cidx, const OpfVec& fac, const OpfVec& lam) {
  for (int k = 0; k < n; ++k) vjp_ut_step(k, cptr, cidx, fac, lam);
  for (int k = n - 1; k >= 0; --k) grad_backward_step(k, par[k], n, fac, lam);
}

// Entry j of the product: w_j lambda_Q of the sgen's node (node >= n: the slack, whose voltage no action moves — exactly 0)
OPF_FN double vjp_entry(double sn, double lim, double scale, int node, int n, const OpfVec& lam) {
  return node < n ? (lim * scale / sn) * lam[(size_t)node * 2 + 1] : 0.0;
}

// res_bus.va_degree of a node from its rectangular voltage
OPF_FN double vjp_va_degree(double e, double f) { return atan2(f, e) * VJP_DEG_PER_RAD; }

}  // namespace mapdn
