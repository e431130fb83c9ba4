// branch_check — mapdn_amd/csrc/branch.hpp compiled for the host (tests/test_branch_cpu.py), the opf_check pattern: a stand-alone program
// that evaluates branch_eval on the records and voltages of a binary file of doubles and writes every column back.
//   in : n_branch, B, n_bus, sn_mva, want (BM_* mask), then per branch 17 doubles  f t live trafo | y[8] | vn_f vn_t | rate | tv_f tv_t,
//        then vm_pu [B][n_bus], va_degree [B][n_bus]
//   out: [B][n_branch][BC_N]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "branch.hpp"

using namespace mapdn;

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: branch_check in.bin out.bin\n"); return 2; }
  std::FILE* fi = std::fopen(argv[1], "rb");
  if (!fi) { std::perror(argv[1]); return 2; }
  std::fseek(fi, 0, SEEK_END);
  const long bytes = std::ftell(fi);
  std::fseek(fi, 0, SEEK_SET);
  std::vector<double> in((size_t)bytes / sizeof(double));
  if (std::fread(in.data(), sizeof(double), in.size(), fi) != in.size()) { std::fprintf(stderr, "short read\n"); return 2; }
  std::fclose(fi);
  if (in.size() < 5) { std::fprintf(stderr, "no header\n"); return 2; }
  const int nbr = (int)in[0], B = (int)in[1], nb = (int)in[2];
  const double sn = in[3];
  const uint32_t want = (uint32_t)in[4];
  const size_t need = 5 + (size_t)17 * nbr + (size_t)2 * B * nb;
  if (nbr < 0 || B < 0 || nb < 1 || in.size() != need) { std::fprintf(stderr, "size mismatch: %zu doubles, expected %zu\n", in.size(), need); return 2; }
  std::vector<BranchRec> rec((size_t)nbr);
  for (int i = 0; i < nbr; ++i) {
    const double* p = &in[5 + (size_t)17 * i];
    BranchRec& r = rec[i];
    r.f = (int32_t)p[0]; r.t = (int32_t)p[1]; r.live = (int32_t)p[2]; r.trafo = (int32_t)p[3];
    for (int q = 0; q < 8; ++q) r.y[q] = p[4 + q];
    r.vn_f = p[12]; r.vn_t = p[13]; r.rate = p[14]; r.tv_f = p[15]; r.tv_t = p[16]; r.parallel = 1.0;
    if (r.f < 0 || r.f >= nb || r.t < 0 || r.t >= nb) { std::fprintf(stderr, "branch %d: bus out of range\n", i); return 2; }
  }
  const double* vm = &in[5 + (size_t)17 * nbr];
  const double* va = vm + (size_t)B * nb;
  const double ang = M_PI / 180.0;                 // the product's conversion: degrees * (pi / 180)
  std::vector<double> out((size_t)B * nbr * BC_N, 0.0);
  for (int e = 0; e < B; ++e)
    for (int i = 0; i < nbr; ++i) {
      const BranchRec& r = rec[i];
      double o[BC_N] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      branch_eval(r, vm[(size_t)e * nb + r.f], va[(size_t)e * nb + r.f] * ang, vm[(size_t)e * nb + r.t], va[(size_t)e * nb + r.t] * ang, sn, want, o);
      for (int c = 0; c < BC_N; ++c) out[((size_t)e * nbr + i) * BC_N + c] = o[c];
    }
  std::FILE* fo = std::fopen(argv[2], "wb");
  if (!fo) { std::perror(argv[2]); return 2; }
  if (std::fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()) { std::fprintf(stderr, "short write\n"); return 2; }
  std::fclose(fo);
  return 0;
}
