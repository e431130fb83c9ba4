// whatif.hpp — the last step of mapdn_evaluate_actions (whatif.hip): the ten totals of an env's statistics -> the reward
// and the MAPDN_N_INFO infos that step() would report (VoltageControl._calc_reward, voltage_control_env.py:574-623, and the unsolvable
// branch of step(), :188-196), as nr_common.hpp::nr_epilogue turns them into a row.  Compilable for the HOST as well:
// tests/test_whatif_cpu.py builds tests/whatif_check.cpp with g++ and holds it to oracle/env_restated.py::_calc_reward.
#pragma once

#ifdef __HIPCC__
#define WHATIF_FN __host__ __device__ __forceinline__
#else
#define WHATIF_FN static inline
#endif

namespace mapdn {

// The totals over every row of res_bus (WT_LO .. WT_BAR), over net.line (WT_LINE) and over the sgens (WT_Q: |q x scaling|, the
// res_sgen.q_mvar of :604-606; WT_QRAW: |q| of the raw table, :189)
enum { WT_LO = 0, WT_HI, WT_DEV, WT_VSUM, WT_DROP, WT_RISE, WT_BAR, WT_LINE, WT_Q, WT_QRAW, WT_N };
enum { WHATIF_N_INFO = 11 };       // MAPDN_N_INFO (include/mapdn.h), column order of INFO_KEYS

// the weights of the reward and the sizes its means run over
struct WhatifCfg {
  int n_bus, n_line, n_sgen;       // rows of res_bus (fused buses included), of net.line, of net.sgen
  int use_line_weight;             // line_weight is given (:612-613), else q_weight (:614-615)
  double voltage_weight, q_weight, line_weight;
};

// solved: the power flow of the candidate converged, tot are the statistics of its solution.  Not solved: tot are those of the
// committed state (:190 restores last_powergrid) except tot[WT_QRAW], the candidate's; the reward loses 200, destroy = 1,
// totally_controllable_ratio = 0 and q_loss = mean |q| of the candidate (:192-196).
WHATIF_FN double whatif_report(const double* tot, const WhatifCfg& c, bool solved, double* inf) {
  const double inv_nb = 1.0 / (double)c.n_bus;                     // all rows of res_bus (:584-589)
  const double out = (tot[WT_LO] + tot[WT_HI]) * inv_nb;
  const double ql = tot[WT_Q] / (double)c.n_sgen, qf = tot[WT_QRAW] / (double)c.n_sgen;
  const double v_loss = tot[WT_BAR] * inv_nb * c.voltage_weight;
  double loss;
  if (c.use_line_weight) loss = tot[WT_LINE] / (double)c.n_line * c.line_weight + v_loss;
  else loss = ql * c.q_weight + v_loss;
  double rew = -loss;
  inf[0] = out; inf[1] = tot[WT_LO] * inv_nb; inf[2] = tot[WT_HI] * inv_nb;
  inf[3] = (out > 1e-3) ? 0.0 : 1.0;
  inf[4] = tot[WT_DEV] * inv_nb; inf[5] = tot[WT_VSUM] * inv_nb; inf[6] = tot[WT_DROP]; inf[7] = tot[WT_RISE];
  inf[8] = tot[WT_LINE]; inf[9] = ql; inf[10] = 0.0;
  if (!solved) { rew -= 200.0; inf[10] = 1.0; inf[3] = 0.0; inf[9] = qf; }
  return rew;
}

}  // namespace mapdn
