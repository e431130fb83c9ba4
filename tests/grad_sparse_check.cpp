// Host build of mapdn_amd/csrc/grad_sparse.hpp and grad.hpp for tests/test_action_grad_sparse_cpu.py: reads a file of doubles, writes a
// file of doubles.  Ybus is dense here, [n + 1][n + 1] by position (position n: the slack), (re, im) interleaved.
//   blocks: 0, n | y[n + 1][n + 1][2] | e[n + 1] | f[n + 1]
//        -> JT[2n][2n] row-major, node-interleaved: block (i, j) is the slot (i, j) of k_action_grad_sparse's assembly — the row sum S_i
//           and A_ii from Y_ij in column order, the off-diagonal block from Y_ji (gs_a, gs_offdiag_t, gs_diag_t)
//   rhs:    1, n, n_line | e[n + 1] | f[n + 1] | vm[n + 1] | n_bus, use_line_weight, barrier_type, voltage_weight, q_weight, line_weight, sn |
//           lines[n_line][6] = fpos, tpos, c[4]
//        -> c[n][2]: the barrier term of every node, then the line terms in the order of net.line (grad_barrier_rhs, grad_line_rhs)
#include <cstdio>
#include <vector>

#include "grad.hpp"
#include "grad_sparse.hpp"

using namespace mapdn;

static std::vector<double> read_all(const char* path) {
  std::vector<double> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  double x;
  while (fread(&x, sizeof(x), 1, f) == 1) v.push_back(x);
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::vector<double> in = read_all(argv[1]);
  if (in.size() < 2) return 3;
  std::vector<double> out;
  size_t o = 0;
  const int mode = (int)in[o++];
  const int n = (int)in[o++];
  const size_t m = (size_t)n + 1;
  if (mode == 0) {
    if (in.size() != 2 + 2 * m * m + 2 * m) return 4;
    const double* y = &in[o]; o += 2 * m * m;
    const double* e = &in[o]; o += m;
    const double* f = &in[o];
    out.assign((size_t)4 * n * n, 0.0);
    auto put = [&](int i, int j, const Opf2x2& b) {
      double* p = &out[((size_t)2 * i) * 2 * n + 2 * j];
      p[0] = b.m00; p[1] = b.m01; p[2 * n] = b.m10; p[2 * n + 1] = b.m11;
    };
    for (int i = 0; i < n; ++i) {
      double sr = 0.0, si = 0.0, aii_r = 0.0, aii_i = 0.0;
      for (size_t j = 0; j < m; ++j) {
        const double* yij = &y[2 * ((size_t)i * m + j)];
        double ar, ai;
        gs_a(e[i], f[i], yij[0], yij[1], e[j], f[j], &ar, &ai);
        sr += ar; si += ai;
        if ((int)j == i) { aii_r = ar; aii_i = ai; }
        if ((int)j != i && j < (size_t)n) {
          const double* yji = &y[2 * (j * m + (size_t)i)];
          double br, bi;
          gs_a(e[j], f[j], yji[0], yji[1], e[i], f[i], &br, &bi);
          put(i, (int)j, gs_offdiag_t(br, bi));
        }
      }
      put(i, i, gs_diag_t(sr, si, aii_r, aii_i));
    }
  } else if (mode == 1) {
    const int n_line = (int)in[o++];
    if (in.size() != 3 + 3 * m + 7 + 6 * (size_t)n_line) return 4;
    const OpfVec e{&in[o], 1}; o += m;
    const OpfVec f{&in[o], 1}; o += m;
    const OpfVec vm{&in[o], 1}; o += m;
    GradCfg c;
    c.n_bus = (int)in[o++]; c.use_line_weight = (int)in[o++]; c.barrier_type = (int)in[o++];
    c.voltage_weight = in[o++]; c.q_weight = in[o++]; c.line_weight = in[o++];
    const double sn = in[o++];
    c.n_line = n_line; c.n_sgen = 1;
    out.assign((size_t)2 * n, 0.0);
    const OpfVec lam{out.data(), 1};
    for (int p = 0; p < n; ++p) { lam[(size_t)p * 2] = 0.0; lam[(size_t)p * 2 + 1] = grad_barrier_rhs(c, vm[p]); }
    if (c.use_line_weight)
      for (int l = 0; l < n_line; ++l) {
        const double* L = &in[o + 6 * (size_t)l];
        grad_line_rhs(c, sn, L + 2, (int)L[0], (int)L[1], n, e, f, lam);
      }
  } else {
    return 5;
  }
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 6;
  fwrite(out.data(), sizeof(double), out.size(), g);
  fclose(g);
  return 0;
}
