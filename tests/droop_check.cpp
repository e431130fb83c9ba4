// host build of mapdn_amd/csrc/droop.hpp (compiled by tests/test_droop_cpu.py with g++): reads n records of 12 doubles
// (v, va, vb, vc, vd, a, damping, v_last, f, ratio, smax, lim) from argv[1] and writes, per record, f(v), the damped update with target
// f(v), one term of the ||v - v_last||^2 sum (from 0.25), and droop_target(f, ratio, smax, lim) of the record's own f to argv[2].
#include <cstdio>
#include <vector>
#include "droop.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 3;
  std::vector<double> in;
  double r[12];
  while (fread(r, sizeof(double), 12, fi) == 12) in.insert(in.end(), r, r + 12);
  fclose(fi);
  std::vector<double> out;
  for (size_t i = 0; i + 12 <= in.size(); i += 12) {
    const double* x = &in[i];
    const double f = mapdn::droop_law(x[0], x[1], x[2], x[3], x[4]);
    out.push_back(f);
    out.push_back(mapdn::droop_damped(x[5], f, x[6]));
    out.push_back(mapdn::droop_dv2_add(0.25, x[0], x[7]));
    out.push_back(mapdn::droop_target(x[8], x[9], x[10], x[11]));
  }
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 4;
  fwrite(out.data(), sizeof(double), out.size(), fo);
  fclose(fo);
  return 0;
}
