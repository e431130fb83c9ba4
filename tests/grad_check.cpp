// Host build of mapdn_amd/csrc/grad.hpp for tests/test_action_grad_cpu.py: reads a file of doubles, writes a file of doubles.
//   adjoint: 0, n, nc | par[n] | cptr[n + 1] | cidx[nc] | yt[n][OPF_YT] | e[n] | f[n] | c[n][2]
//         -> lambda[n][2] of J' lambda = c by the two transposed sweeps (rows (theta, u = d|V| / |V|) per node)
//   barrier: 1, type, m | v[m]  ->  barrier_deriv(type, v)[m]
//   gradient: 2, n, nc, ns, n_line | par | cptr | cidx | yt | e[n + 1] | f[n + 1] | vm[n + 1] (position n: the slack) |
//             n_bus, use_line_weight, barrier_type, voltage_weight, q_weight, line_weight, sn |
//             lines[n_line][6] = fpos, tpos, c[4] | sgens[ns][4] = node, lim, scaling, a
//         -> g[ns]: the right-hand side, the adjoint solve and the read-out in k_action_grad's order
#include <cstdio>
#include <vector>

#include "grad.hpp"

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
  if (in.size() < 3) return 3;
  std::vector<double> out;
  size_t o = 0;
  const int mode = (int)in[o++];
  if (mode == 1) {
    const int type = (int)in[o++], m = (int)in[o++];
    if (in.size() != (size_t)3 + m) return 4;
    for (int i = 0; i < m; ++i) out.push_back(barrier_deriv(type, in[o + i]));
  } else if (mode == 0 || mode == 2) {
    const int n = (int)in[o++], nc = (int)in[o++];
    const int ns = mode == 2 ? (int)in[o++] : 0, n_line = mode == 2 ? (int)in[o++] : 0;
    const size_t tables = (size_t)n + (n + 1) + nc + (size_t)n * OPF_YT;
    if (mode == 0 && in.size() != 3 + tables + 4 * (size_t)n) return 4;
    if (mode == 2 && in.size() != 5 + tables + 3 * (size_t)(n + 1) + 7 + 6 * (size_t)n_line + 4 * (size_t)ns) return 4;
    std::vector<int32_t> par(n), cptr(n + 1), cidx(nc);
    for (int& p : par) p = (int)in[o++];
    for (int& p : cptr) p = (int)in[o++];
    for (int& p : cidx) p = (int)in[o++];
    const double* yt = &in[o]; o += (size_t)n * OPF_YT;
    const size_t nv = mode == 2 ? n + 1 : n;
    const OpfVec e{&in[o], 1}; o += nv;
    const OpfVec f{&in[o], 1}; o += nv;
    std::vector<double> fac((size_t)n * OPF_FAC), lam((size_t)n * 2);
    const OpfVec F{fac.data(), 1}, L{lam.data(), 1};
    if (mode == 0) {
      for (int i = 0; i < 2 * n; ++i) lam[i] = in[o++];
      grad_adjoint(n, par.data(), cptr.data(), cidx.data(), yt, e, f, F, L);
      out = lam;
    } else {
      const double* vm = &in[o]; o += nv;
      GradCfg c;
      c.n_bus = (int)in[o++]; c.use_line_weight = (int)in[o++]; c.barrier_type = (int)in[o++];
      c.voltage_weight = in[o++]; c.q_weight = in[o++]; c.line_weight = in[o++];
      const double sn = in[o++];
      c.n_line = n_line; c.n_sgen = ns;
      for (int p = 0; p < n; ++p) { lam[(size_t)p * 2] = 0.0; lam[(size_t)p * 2 + 1] = grad_barrier_rhs(c, vm[p]); }
      if (c.use_line_weight)
        for (int l = 0; l < n_line; ++l) {
          const double* r = &in[o + 6 * (size_t)l];
          grad_line_rhs(c, sn, r + 2, (int)r[0], (int)r[1], n, e, f, L);
        }
      o += 6 * (size_t)n_line;
      grad_adjoint(n, par.data(), cptr.data(), cidx.data(), yt, e, f, F, L);
      for (int j = 0; j < ns; ++j) {
        const double* r = &in[o + 4 * (size_t)j];
        out.push_back(grad_entry(c, sn, r[1], r[2], r[3], (int)r[0], n, L));
      }
    }
  } else return 5;
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 6;
  fwrite(out.data(), sizeof(double), out.size(), g);
  fclose(g);
  return 0;
}
