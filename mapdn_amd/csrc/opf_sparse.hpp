// opf_sparse.hpp — the arithmetic of the OPF baseline's linearisation on a handle that k_nr_sparse solves (mapdn_opf_config.meshed = 1;
// opf_sparse.hip).  Compilable for the HOST as well: tests/opf_sparse_check.cpp builds this header with g++
// (tests/test_opf_sparse_cpu.py).
//
// The sensitivities of opf.hpp, J X = [w_j e_Q at the node of sgen j], on a net of any topology: the host-compiled block-elimination
// program (plan.hpp SparseProg) solves  B x = b  for the blocks its slots hold, so with the blocks of J itself (grad_sparse.hpp:
// gs_offdiag, gs_diag — what k_nr_sparse assembles) and the columns in the right-hand-side slots it leaves (dtheta, u = d|V| / |V|) there.
// A right-hand-side slot is a 2x2 block of which the power flow uses one column, so one run of the program carries TWO columns.
// Then, as on the tree, S = u |V|, dV = (u + j dtheta) V, and with M = (Ybus + Ybus^H) / 2:  loss = V^H M V,  g_j = 2 Re(dV_j^H M V),
// H_ij = 2 Re(dV_i^H M dV_j).  M is applied row by row from a CSR over the node positions (plan.cpp opf_sparse_table: columns
// ascending, the slack's column apart — dV_slack = 0), every sum in the table's order.
#pragma once
#include "grad_sparse.hpp"   // gs_a, gs_offdiag, gs_diag; opf.hpp: OpfVec, Opf2x2, OPF_FN

namespace mapdn {

// M over the non-slack nodes: row k holds the entries ptr[k] .. ptr[k + 1]: column position (< n) and (Re, Im) M_kj; msv[k] = (Re, Im) of
// M_k,slack V_slack
struct OsM { const int32_t *ptr, *col; const double *val, *msv; };

// (M x)_k over the non-slack columns; x_j = re[j * xs] + j im[j * xs]
OPF_FN void os_m_row(const OsM& m, int k, const OpfVec& re, const OpfVec& im, size_t xs, double* wr, double* wi) {
  double r = 0.0, i = 0.0;
  for (int q = m.ptr[k]; q < m.ptr[k + 1]; ++q) {
    const size_t j = (size_t)m.col[q] * xs;
    const double a = m.val[2 * q], b = m.val[2 * q + 1], xr = re[j], xi = im[j];
    r += a * xr - b * xi; i += a * xi + b * xr;
  }
  *wr = r; *wi = i;
}
// (M V)_k, the slack's column included: into mv[2 k], mv[2 k + 1]
OPF_FN void os_mv_row(const OsM& m, int k, const OpfVec& E, const OpfVec& F, const OpfVec& mv) {
  double r, i;
  os_m_row(m, k, E, F, 1, &r, &i);
  mv[(size_t)k * 2] = r + m.msv[2 * k]; mv[(size_t)k * 2 + 1] = i + m.msv[2 * k + 1];
}
// the loss V^H M V: conj(V_k) (M V)_k over the nodes, + the slack's row (its own term loss_slack and conj(V_slack) M_slack,k V_k, which is
// the conjugate of conj(V_k) M_k,slack V_slack)
OPF_FN double os_loss(const OsM& m, int n, double loss_slack, const OpfVec& E, const OpfVec& F, const OpfVec& mv) {
  double loss = loss_slack;
  for (int k = 0; k < n; ++k)
    loss += E[k] * mv[(size_t)k * 2] + F[k] * mv[(size_t)k * 2 + 1] + (m.msv[2 * k] * E[k] + m.msv[2 * k + 1] * F[k]);
  return loss;
}
// column j: W = M dV into w (the layout of x: node k at [k * xs], [k * xs + 1]); returns g_j = 2 Re(dV^H M V)
OPF_FN double os_column(const OsM& m, int n, const OpfVec& x, const OpfVec& w, const OpfVec& mv, size_t xs) {
  const OpfVec xi{x.p + x.s, x.s};
  double g = 0.0;
  for (int k = 0; k < n; ++k) {
    double wr, wi;
    os_m_row(m, k, x, xi, xs, &wr, &wi);
    w[(size_t)k * xs] = wr; w[(size_t)k * xs + 1] = wi;
    g += x[(size_t)k * xs] * mv[(size_t)k * 2] + x[(size_t)k * xs + 1] * mv[(size_t)k * 2 + 1];
  }
  return 2.0 * g;
}
// H_ij = 2 Re(dV_i^H W_j)
OPF_FN double os_h(int n, const OpfVec& xi, const OpfVec& wj, size_t xs) {
  double h = 0.0;
  for (int k = 0; k < n; ++k) h += xi[(size_t)k * xs] * wj[(size_t)k * xs] + xi[(size_t)k * xs + 1] * wj[(size_t)k * xs + 1];
  return 2.0 * h;
}

}  // namespace mapdn
