// grad_sparse.hpp — the block formulas of k_action_grad_sparse (grad_sparse.hip): mapdn_action_gradients on a handle that
// k_nr_sparse solves.  Compilable for the HOST as well: tests/grad_sparse_check.cpp builds this header with g++
// (tests/test_action_grad_sparse_cpu.py).
//
// The adjoint system of grad.hpp, J' lambda = c, on a net of any topology: the host-compiled block-elimination program (plan.hpp
// SparseProg) solves  B x = b  for whatever blocks its slots hold, and the fill pattern of J is structurally symmetric, so the same
// program on the blocks of J' — slot (i, j) holds (J')_ij = (J_ji)' — with c in the right-hand-side slots leaves lambda there.
// With A_ij = V_i conj(Y_ij V_j) and S_i = sum_j A_ij (k_nr_sparse's assembly; rows (P, Q), columns (theta, u = d|V| / |V|)):
//     J_ij = [[Im A_ij, Re A_ij], [-Re A_ij, Im A_ij]]   (j != i)        J_ii = [[-(Im S_i - Im A_ii), Re S_i + Re A_ii],
//                                                                                [Re S_i - Re A_ii, Im S_i + Im A_ii]]
// so slot (i, j) takes the transpose of the block of A_ji = V_j conj(Y_ji V_i): Y_ji, not Y_ij — Ybus is not symmetric behind a
// phase-shifting transformer — and the diagonal slot the transpose of J_ii.
#pragma once
#include "opf.hpp"   // Opf2x2, OPF_FN

namespace mapdn {

// A = V_a conj(Y V_b)
OPF_FN void gs_a(double ea, double fa, double yr, double yi, double eb, double fb, double* ar, double* ai) {
  const double tr = yr * eb - yi * fb, ti = yr * fb + yi * eb;
  *ar = ea * tr + fa * ti; *ai = fa * tr - ea * ti;
}
// slot (i, j) of J itself, from A_ij, and slot (i, i) from S_i and A_ii: what k_nr_sparse assembles and k_opf_sens_sparse (opf_sparse.hip) as well
OPF_FN Opf2x2 gs_offdiag(double aij_r, double aij_i) { return {aij_i, aij_r, -aij_r, aij_i}; }
OPF_FN Opf2x2 gs_diag(double sr, double si, double aii_r, double aii_i) { return {-(si - aii_i), sr + aii_r, sr - aii_r, si + aii_i}; }
// slot (i, j) of J': (J_ji)' from A_ji
OPF_FN Opf2x2 gs_offdiag_t(double aji_r, double aji_i) { return {aji_i, -aji_r, aji_r, aji_i}; }
// slot (i, i) of J': (J_ii)' from S_i and A_ii
OPF_FN Opf2x2 gs_diag_t(double sr, double si, double aii_r, double aii_i) { return {-(si - aii_i), sr - aii_r, sr + aii_r, si + aii_i}; }

}  // namespace mapdn
