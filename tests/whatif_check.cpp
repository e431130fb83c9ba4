// host build of mapdn_amd/csrc/whatif.hpp (compiled by tests/test_whatif_cpu.py with g++): reads records from argv[1], each
//   11 doubles: n_bus, n_line, n_sgen, barrier type (MAPDN_BARRIER_*), use_line_weight, voltage_weight, q_weight, line_weight, v_lower,
//               v_upper, solved
//   then vm_pu[n_bus], pl_mw[n_line], res_sgen q[n_sgen] (q x scaling), raw q[n_sgen] (of the candidate)
// forms the ten totals as k_whatif_score forms them (csrc/whatif.hip; here one sequential sum each, the barriers of nr_common.hpp restated
// for the host with nrmath.hpp's bowl_inside) and writes, per record, the reward and the 11 infos of whatif_report to argv[2].
#include <cmath>
#include <cstdio>
#include <vector>
#include "nrmath.hpp"
#include "whatif.hpp"

static double barrier_host(int type, double v) {
  switch (type) {
    case 0: return std::fabs(v - 1.0);
    case 1: return 2.0 * (v - 1.0) * (v - 1.0);
    case 2: { const double a = std::fmax(0.0, v - 1.05), b = std::fmax(0.0, 0.95 - v); return a * a + b * b; }
    case 3: { const double dv = std::fabs(v - 1.0); return dv > 0.05 ? 2.0 * dv - 0.095 : mapdn::bowl_inside(v); }
    default:
      if (std::fabs(v) < 1.0) return std::exp(-1.0 / (1.0 - v * v * v * v));
      if (v > 1.0 && v < 3.0) { const double w = v - 2.0; return std::exp(-1.0 / (1.0 - w * w * w * w)); }
      return 0.0;
  }
}

int main(int argc, char** argv) {
  using namespace mapdn;
  if (argc != 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 3;
  std::vector<double> out;
  double hd[11];
  while (fread(hd, sizeof(double), 11, fi) == 11) {
    const int nb = (int)hd[0], nl = (int)hd[1], ns = (int)hd[2], bt = (int)hd[3];
    if (nb < 1 || nl < 1 || ns < 1) return 5;
    std::vector<double> v((size_t)nb), pl((size_t)nl), qs((size_t)ns), qr((size_t)ns);
    if (fread(v.data(), sizeof(double), v.size(), fi) != v.size() || fread(pl.data(), sizeof(double), pl.size(), fi) != pl.size() ||
        fread(qs.data(), sizeof(double), qs.size(), fi) != qs.size() || fread(qr.data(), sizeof(double), qr.size(), fi) != qr.size())
      return 6;
    const double vlo = hd[8], vhi = hd[9], vref = 0.5 * (vlo + vhi);
    double tot[WT_N] = {0.0};
    for (double x : v) {
      tot[WT_LO] += x < vlo ? 1.0 : 0.0; tot[WT_HI] += x > vhi ? 1.0 : 0.0;
      tot[WT_DEV] += std::fabs(x - vref); tot[WT_VSUM] += x;
      tot[WT_DROP] = std::fmax(tot[WT_DROP], x < vlo ? vlo - x : 0.0);
      tot[WT_RISE] = std::fmax(tot[WT_RISE], x > vhi ? x - vhi : 0.0);
      tot[WT_BAR] += barrier_host(bt, x);
    }
    for (double x : pl) tot[WT_LINE] += x;
    for (double x : qs) tot[WT_Q] += std::fabs(x);
    for (double x : qr) tot[WT_QRAW] += std::fabs(x);
    const WhatifCfg c = {nb, nl, ns, (int)hd[4], hd[5], hd[6], hd[7]};
    double inf[WHATIF_N_INFO];
    out.push_back(whatif_report(tot, c, hd[10] != 0.0, inf));
    out.insert(out.end(), inf, inf + WHATIF_N_INFO);
  }
  fclose(fi);
  FILE* fo = fopen(argv[2], "wb");
  if (!fo) return 4;
  fwrite(out.data(), sizeof(double), out.size(), fo);
  fclose(fo);
  return 0;
}
