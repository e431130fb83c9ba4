// Host build of mapdn_amd/csrc/vjp.hpp for tests/test_voltage_vjp_cpu.py: reads a file of doubles, writes a file of doubles.
//   n, nc, ns, M | par[n] | cptr[n + 1] | cidx[nc] | yt[n][OPF_YT] | e[n] | f[n] | vm[n] | sn |
//   sgens[ns][3] = node, lim, scaling | cot[M][n][2] = cot_vm, cot_va of every node's bus
//   -> g[M][ns]: one factorisation, then per cotangent the right-hand side, the two transposed sweeps on the stored factors and the
//      read-out, in k_voltage_vjp's order;  then va_degree[n]
#include <cstdio>
#include <vector>

#include "vjp.hpp"

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
  if (in.size() < 4) return 3;
  size_t o = 0;
  const int n = (int)in[o++], nc = (int)in[o++], ns = (int)in[o++], M = (int)in[o++];
  if (n < 1 || nc < 0 || ns < 0 || M < 0) return 4;
  const size_t want = 4 + (size_t)n + (n + 1) + nc + (size_t)n * OPF_YT + 3 * (size_t)n + 1 + 3 * (size_t)ns + 2 * (size_t)M * n;
  if (in.size() != want) return 4;
  std::vector<int32_t> par(n), cptr(n + 1), cidx(nc);
  for (int& p : par) p = (int)in[o++];
  for (int& p : cptr) p = (int)in[o++];
  for (int& p : cidx) p = (int)in[o++];
  const double* yt = &in[o]; o += (size_t)n * OPF_YT;
  const OpfVec e{&in[o], 1}; o += n;
  const OpfVec f{&in[o], 1}; o += n;
  const double* vm = &in[o]; o += n;
  const double sn = in[o++];
  const double* sg = &in[o]; o += 3 * (size_t)ns;
  std::vector<double> fac((size_t)n * OPF_FAC), lam((size_t)n * 2), out;
  const OpfVec F{fac.data(), 1}, L{lam.data(), 1};
  vjp_factorise(n, par.data(), cptr.data(), cidx.data(), yt, e, f, F);
  for (int m = 0; m < M; ++m) {
    const double* c = &in[o + 2 * (size_t)m * n];
    for (int p = 0; p < n; ++p) vjp_rhs(p, c[2 * p], c[2 * p + 1], vm[p], L);
    vjp_adjoint(n, par.data(), cptr.data(), cidx.data(), F, L);
    for (int j = 0; j < ns; ++j) out.push_back(vjp_entry(sn, sg[3 * j + 1], sg[3 * j + 2], (int)sg[3 * j], n, L));
  }
  for (int p = 0; p < n; ++p) out.push_back(vjp_va_degree(e[p], f[p]));
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 6;
  fwrite(out.data(), sizeof(double), out.size(), g);
  fclose(g);
  return 0;
}
