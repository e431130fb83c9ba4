// Host build of csrc/opf_sparse.hpp (with csrc/grad_sparse.hpp's block formulas) for tests/test_opf_sparse_cpu.py: the untransposed
// Jacobian blocks that k_opf_sens_sparse assembles and the M-row sums of k_opf_reduce_sparse, on a dense Ybus by position.
//   in  (float64 stream): n, ns | Y [(n + 1)][(n + 1)][2] by position (position n: the slack) | Re V [n + 1] | Im V [n + 1] |
//                         node of sgen j [ns] (n: the slack) | w_j [ns]
//   out (float64 stream): J [2n][2n], interleaved per node (rows P, Q; columns theta, u) | M V [n][2] | loss | g [ns] | H [ns][ns] |
//                         S [n][ns]
// The sensitivities come from a dense Gaussian elimination with partial pivoting on that J: the program's own elimination is emulated
// in numpy by the test.
#include <cmath>
#include <complex>
#include <cstdio>
#include <map>
#include <vector>

#include "opf_sparse.hpp"

using namespace mapdn;
using cplx = std::complex<double>;

static std::vector<double> read_all(const char* path) {
  std::vector<double> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) return v;
  double x;
  while (std::fread(&x, sizeof(x), 1, f) == 1) v.push_back(x);
  std::fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  const std::vector<double> in = read_all(argv[1]);
  if (in.size() < 2) return 3;
  const int n = (int)in[0], ns = (int)in[1], nb = n + 1;
  size_t o = 2;
  auto Y = [&](int i, int j) { return cplx(in[2 + 2 * ((size_t)i * nb + j)], in[2 + 2 * ((size_t)i * nb + j) + 1]); };
  o += 2 * (size_t)nb * nb;
  std::vector<double> E(in.begin() + o, in.begin() + o + nb), F(in.begin() + o + nb, in.begin() + o + 2 * nb);
  o += 2 * (size_t)nb;
  std::vector<int> node(ns);
  std::vector<double> w(ns);
  for (int j = 0; j < ns; ++j) { node[j] = (int)in[o + j]; w[j] = in[o + ns + j]; }
  if (in.size() != o + 2 * (size_t)ns) return 4;

  // ---- the blocks, as the kernel's assembly row forms them: A_ij over the structural entries of row i in column order
  const int N = 2 * n;
  std::vector<double> J((size_t)N * N, 0.0);
  auto put = [&](int i, int j, const Opf2x2& m) {
    J[(size_t)(2 * i) * N + 2 * j] = m.m00; J[(size_t)(2 * i) * N + 2 * j + 1] = m.m01;
    J[(size_t)(2 * i + 1) * N + 2 * j] = m.m10; J[(size_t)(2 * i + 1) * N + 2 * j + 1] = m.m11;
  };
  for (int i = 0; i < n; ++i) {
    double sr = 0.0, si = 0.0, aii_r = 0.0, aii_i = 0.0;
    for (int j = 0; j < nb; ++j) {
      const cplx y = Y(i, j);
      if (y == cplx(0, 0)) continue;
      double ar, ai;
      gs_a(E[i], F[i], y.real(), y.imag(), E[j], F[j], &ar, &ai);
      sr += ar; si += ai;
      if (j == i) { aii_r = ar; aii_i = ai; }
      else if (j < n) put(i, j, gs_offdiag(ar, ai));
    }
    put(i, i, gs_diag(sr, si, aii_r, aii_i));
  }

  // ---- the rows of M = (Y + Y^H) / 2 (plan.cpp opf_sparse_table's layout): columns ascending, the slack's column apart
  std::vector<int32_t> ptr(1, 0), col;
  std::vector<double> val, msv((size_t)2 * n);
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) {
      const cplx m = 0.5 * (Y(i, j) + std::conj(Y(j, i)));
      if (m != cplx(0, 0)) { col.push_back(j); val.push_back(m.real()); val.push_back(m.imag()); }
    }
    ptr.push_back((int32_t)col.size());
    const cplx ms = 0.5 * (Y(i, n) + std::conj(Y(n, i))) * cplx(E[n], F[n]);
    msv[2 * i] = ms.real(); msv[2 * i + 1] = ms.imag();
  }
  const OsM M{ptr.data(), col.data(), val.data(), msv.data()};
  const double loss_slack = Y(n, n).real() * (E[n] * E[n] + F[n] * F[n]);

  // ---- J X = [w_j e_Q at node(j)]: dense elimination with partial pivoting
  std::vector<double> A = J, X((size_t)N * ns, 0.0);
  for (int j = 0; j < ns; ++j) if (node[j] < n) X[(size_t)(2 * node[j] + 1) * ns + j] = w[j];
  for (int k = 0; k < N; ++k) {
    int p = k;
    for (int r = k + 1; r < N; ++r) if (std::fabs(A[(size_t)r * N + k]) > std::fabs(A[(size_t)p * N + k])) p = r;
    if (p != k) {
      for (int c = 0; c < N; ++c) std::swap(A[(size_t)p * N + c], A[(size_t)k * N + c]);
      for (int c = 0; c < ns; ++c) std::swap(X[(size_t)p * ns + c], X[(size_t)k * ns + c]);
    }
    for (int r = k + 1; r < N; ++r) {
      const double f = A[(size_t)r * N + k] / A[(size_t)k * N + k];
      if (f == 0.0) continue;
      for (int c = k; c < N; ++c) A[(size_t)r * N + c] -= f * A[(size_t)k * N + c];
      for (int c = 0; c < ns; ++c) X[(size_t)r * ns + c] -= f * X[(size_t)k * ns + c];
    }
  }
  for (int k = N - 1; k >= 0; --k)
    for (int c = 0; c < ns; ++c) {
      double x = X[(size_t)k * ns + c];
      for (int q = k + 1; q < N; ++q) x -= A[(size_t)k * N + q] * X[(size_t)q * ns + c];
      X[(size_t)k * ns + c] = x / A[(size_t)k * N + k];
    }

  // ---- S, dV in the kernels' layout (node k, column j at [(k * ns + j) * 2]), then opf_sparse.hpp's sums
  const size_t xs = (size_t)ns * 2;
  std::vector<double> S((size_t)n * ns), dV((size_t)n * xs), W((size_t)n * xs), mv((size_t)2 * n), g(ns), H((size_t)ns * ns);
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < ns; ++j) {
      const double th = X[(size_t)(2 * k) * ns + j], u = X[(size_t)(2 * k + 1) * ns + j];
      S[(size_t)k * ns + j] = u * std::sqrt(E[k] * E[k] + F[k] * F[k]);
      dV[(size_t)k * xs + 2 * j] = u * E[k] - th * F[k]; dV[(size_t)k * xs + 2 * j + 1] = u * F[k] + th * E[k];
    }
  const OpfVec e{E.data(), 1}, f{F.data(), 1}, mvv{mv.data(), 1};
  for (int k = 0; k < n; ++k) os_mv_row(M, k, e, f, mvv);
  const double loss = os_loss(M, n, loss_slack, e, f, mvv);
  for (int j = 0; j < ns; ++j) g[j] = os_column(M, n, OpfVec{dV.data() + 2 * j, 1}, OpfVec{W.data() + 2 * j, 1}, mvv, xs);
  for (int j = 0; j < ns; ++j)
    for (int i = 0; i <= j; ++i) H[(size_t)i * ns + j] = H[(size_t)j * ns + i] = os_h(n, OpfVec{dV.data() + 2 * i, 1}, OpfVec{W.data() + 2 * j, 1}, xs);

  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 5;
  std::fwrite(J.data(), sizeof(double), J.size(), out);
  std::fwrite(mv.data(), sizeof(double), mv.size(), out);
  std::fwrite(&loss, sizeof(double), 1, out);
  std::fwrite(g.data(), sizeof(double), g.size(), out);
  std::fwrite(H.data(), sizeof(double), H.size(), out);
  std::fwrite(S.data(), sizeof(double), S.size(), out);
  std::fclose(out);
  return 0;
}
