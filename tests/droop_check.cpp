// host build of mapdn_amd/csrc/droop.hpp (compiled by tests/test_droop_cpu.py with g++): reads n records of 8 doubles
// (v, va, vb, vc, vd, a, damping, v_last) from argv[1] and writes, per record, f(v), the damped update with target f(v), and one
// term of the ||v - v_last||^2 sum (from 0.25) to argv[2].
#include <cstdio>
#include <vector>
#include "droop.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 3;
  std::vector<double> in;
  double r[8];
  while (fread(r, sizeof(double), 8, fi) == 8) in.insert(in.end(), r, r + 8);
  fclose(fi);
  std::vector<double> out;
  for (size_t i = 0; i + 8 <= in.size(); i += 8) {
    const double* x = &in[i];
    const double f = mapdn::droop_law(x[0], x[1], x[2], x[3], x[4]);
    out.push_back(f);
    out.push_back(mapdn::droop_damped(x[5], f, x[6]));
    out.push_back(mapdn::droop_dv2_add(0.25, x[0], x[7]));
  }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 4;
  fwrite(out.data(), sizeof(double), out.size(), fo);
  fclose(fo);
  return 0;
}
