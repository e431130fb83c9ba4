// whatif.hip — mapdn_evaluate_actions: what step() would report for K candidate joint actions of every env, from the env's
// current state and without taking the step.  Per candidate, in the control-loop frame of the baselines (ctlloop.hpp):
//   k_whatif_start   the candidate's actions into the frame's env-minor rows, the Sbus rows step() would write for them
//   the solve        the handle's own power-flow kernel in MODE_SOLVE on the frame's active set (baselines_host.hpp, whatif_run)
//   k_whatif_score   _calc_reward (voltage_control_env.py:574-623) and the unsolvable branch of step() (:188-196) on the Vout rows
// What nr_common.hpp::nr_epilogue computes inside the solver for the step it commits, restated here as a wide kernel that commits nothing.
// Included at the end of kernels.hip (one translation unit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "kernels.hpp"
#include "ctlloop.hpp"
#include "nr_common.hpp"   // barrier()
#include "whatif.hpp"

namespace mapdn {

// Layout: ctlloop.hpp (16 consecutive envs x 16 sub-lanes per workgroup).
// Candidate k of every env: a <- actions[e][k][:] widened as the step path widens it (inject.hpp turn_q), then — the barrier: the a of
// every sgen of a bus before its row — the PV-bus rows of the Sbus buffer the next solve reads.  k == 0 also does the start bookkeeping
// (which envs step() would solve: the frame's active set for all K solves) and the several-load-bus rows, which no candidate changes.
template <typename AT>
__global__ void __launch_bounds__(DL * DS) k_whatif_start(Dev d, WhatifState s, const AT* __restrict__ actions, int k) {
  const CtlLane t = ctl_lane(d);
  const size_t S = (size_t)d.Bp;
  const bool run = k == 0 ? ctl_start(d, s, t) : (t.valid && s.act[t.e] != 0);
  if (t.valid) {
    const AT* __restrict__ row = actions + ((size_t)t.e * s.K + k) * d.ns;
    for (int j = t.sl; j < d.ns; j += DS) s.a[(size_t)j * S + t.e] = (double)row[j];
    if (k == 0 && run) ctl_mlo_rows(d, t);
  }
  __syncthreads();
  if (run) for (int jb = t.sl; jb < d.n_sgb; jb += DS) ctl_pv_row(d, t.e, jb, s.a);
}

// the voltage statistics of one row of res_bus, barrier type BT
struct WhatifBus { double lo = 0.0, hi = 0.0, dev = 0.0, sum = 0.0, drop = 0.0, rise = 0.0, bar = 0.0; };
template <int BT>
__device__ __forceinline__ void whatif_bus(WhatifBus& b, double v, double vlo, double vhi, double vref) {
  b.lo += (v < vlo) ? 1.0 : 0.0; b.hi += (v > vhi) ? 1.0 : 0.0;
  b.dev += fabs(v - vref); b.sum += v;
  b.drop = fmax(b.drop, (v < vlo) ? (vlo - v) : 0.0);
  b.rise = fmax(b.rise, (v > vhi) ? (v - vhi) : 0.0);
  b.bar += barrier(BT, v);
}

// After the solve of candidate k: row (e, k) of every output.  Sub-lane s of an env takes the nodes, alias rows, lines and sgens
// s, s + DS, ...; the partials meet in LDS and are totalled in the fixed order of the sub-lanes 0 ... DS - 1 (by sub-lane q for
// quantity q), so that an env's row has the same bits wherever the env sits in the batch and whatever the other candidates are.
//   solved      statistics of the solution in the Vout rows (position n, the slack, holds vroot + 0j: alloc_nrbuf); a fused bus is a row of
//               res_bus too and counts its node again (d.alias_pos)
//   not solved  statistics of the committed tables d.vm / d.pl / d.cur_q, as step() reports them after restoring the last state
//   not run     (step() would not solve the env: ctl_start) status 3, NaN
__global__ void __launch_bounds__(DL * DS) k_whatif_score(Dev d, WhatifState s, int k) {
  __shared__ double s_part[WT_N][DS][DL];
  const CtlLane t = ctl_lane(d);
  const int el = t.el, sl = t.sl, e = t.e;
  const size_t S = (size_t)d.Bp;
  const bool act = t.valid && s.act[e] != 0;
  const bool conv = act && s.nr_conv[e] != 0;
  const double* __restrict__ vout = d.nrbuf + (size_t)d.r_vout * S + e;      // row r of Vout for this env: vout[r * S]
  const double vlo = d.v_lower, vhi = d.v_upper, vref = 0.5 * (vlo + vhi);
  WhatifBus b;
  // the barrier type is hoisted out of the bus loops (one instance per type), as nr_epilogue does it
  auto bus_loops = [&](auto type_tag) {
    constexpr int BT = decltype(type_tag)::value;
    if (conv) {
#pragma unroll 4
      for (int p = sl; p <= d.n; p += DS) whatif_bus<BT>(b, vout[((size_t)VOF * p + VO_VM) * S], vlo, vhi, vref);
      for (int a = sl; a < d.n_alias; a += DS) whatif_bus<BT>(b, vout[((size_t)VOF * d.alias_pos[a] + VO_VM) * S], vlo, vhi, vref);
    } else if (act) {
      for (int r = sl; r < d.nbo; r += DS) whatif_bus<BT>(b, d.vm[(size_t)r * S + e], vlo, vhi, vref);
    }
  };
  switch (d.barrier_type) {
    case MAPDN_BARRIER_L1: bus_loops(std::integral_constant<int, MAPDN_BARRIER_L1>{}); break;
    case MAPDN_BARRIER_L2: bus_loops(std::integral_constant<int, MAPDN_BARRIER_L2>{}); break;
    case MAPDN_BARRIER_COURANT_BELTRAMI: bus_loops(std::integral_constant<int, MAPDN_BARRIER_COURANT_BELTRAMI>{}); break;
    case MAPDN_BARRIER_BOWL: bus_loops(std::integral_constant<int, MAPDN_BARRIER_BOWL>{}); break;
    default: bus_loops(std::integral_constant<int, MAPDN_BARRIER_BUMP>{}); break;
  }
  // res_line.pl_mw = Re(Sf + St) sn from the LineFlow constants (the expression of nr_epilogue), or the committed table
  double line_loss = 0.0;
  if (conv) {
#pragma unroll 2
    for (int l = sl; l < d.n_line; l += DS) {
      const LineFlow L = d.lines[l];
      const double gff = L.c[0], gtt = L.c[1], gs = L.c[2], bd = L.c[3];
      const double* vf = vout + (size_t)VOF * L.fpos * S;
      const double* vt = vout + (size_t)VOF * L.tpos * S;
      const double ef = vf[(size_t)VO_E * S], ff = vf[(size_t)VO_F * S], et = vt[(size_t)VO_E * S], ft = vt[(size_t)VO_F * S];
      const double wr = ef * et + ff * ft, wi = ff * et - ef * ft;
      line_loss += ((gff * (ef * ef + ff * ff) + gtt * (et * et + ft * ft)) + (gs * wr + bd * wi)) * d.sn;
    }
  } else if (act) {
    for (int l = sl; l < d.n_line; l += DS) line_loss += d.pl[(size_t)l * S + e];
  }
  // q of the candidate: clip_q of the step path on the frame's a rows; of a failed solve the committed sgen.q_mvar, and |q| raw
  double q_loss = 0.0, q_raw = 0.0;
  if (act)
    for (int j = sl; j < d.ns; j += DS) {
      const size_t o = (size_t)j * S + e;
      const double q = clip_q(d.cur_pv[o], d.smax[j], s.a[o]);
      q_loss += fabs((conv ? q : d.cur_q[o]) * d.sgen_scale[j]);
      q_raw += fabs(q);
    }
  const double part[WT_N] = {b.lo, b.hi, b.dev, b.sum, b.drop, b.rise, b.bar, line_loss, q_loss, q_raw};
#pragma unroll
  for (int q = 0; q < WT_N; ++q) s_part[q][sl][el] = part[q];
  __syncthreads();
  static_assert(WT_N <= DS, "one sub-lane totals one quantity");
  if (sl < WT_N) {
    double a = s_part[sl][0][el];
#pragma unroll
    for (int w = 1; w < DS; ++w) { const double x = s_part[sl][w][el]; a = (sl == WT_DROP || sl == WT_RISE) ? fmax(a, x) : a + x; }
    s_part[sl][0][el] = a;
  }
  __syncthreads();
  if (!t.valid) return;
  const size_t row = (size_t)e * s.K + k;
  if (s.vm_out) {
    double* vm = s.vm_out + row * d.nbo;
    for (int r = sl; r < d.nbo; r += DS) vm[r] = conv ? d.nrbuf[(size_t)s.vm_row[r] * S + e] : __builtin_nan("");
  }
  if (sl != 0) return;
  // (reward and info are nullptr in mapdn_voltage_vjp's frame, which reports the voltages, the status and the iterations alone)
  double* inf = s.info ? s.info + row * WHATIF_N_INFO : nullptr;
  if (!act) {
    if (s.reward) s.reward[row] = __builtin_nan("");
    if (inf) for (int c = 0; c < WHATIF_N_INFO; ++c) inf[c] = __builtin_nan("");
    s.status_out[row] = CTL_STOPPED;
    if (s.iters_out) s.iters_out[row] = 0;
    return;
  }
  double tot[WT_N], out[WHATIF_N_INFO];
#pragma unroll
  for (int q = 0; q < WT_N; ++q) tot[q] = s_part[q][0][el];
  const WhatifCfg c = {d.nbo, d.n_line, d.ns, d.use_line_weight, d.voltage_weight, d.q_weight, d.line_weight};
  const double reward = whatif_report(tot, c, conv, out);
  if (s.reward) s.reward[row] = reward;
  if (inf) {
#pragma unroll
    for (int i = 0; i < WHATIF_N_INFO; ++i) inf[i] = out[i];
  }
  s.status_out[row] = conv ? WHATIF_SOLVED : WHATIF_PF_FAILED;
  if (s.iters_out) s.iters_out[row] = s.nr_iters[e];
}

void launch_whatif_start(const Dev& d, const WhatifState& s, const void* actions, int dtype, int k, hipStream_t st) {
  const dim3 grid((d.B + DL - 1) / DL), block(DL * DS);
  if (dtype == MAPDN_F32) hipLaunchKernelGGL(k_whatif_start<float>, grid, block, 0, st, d, s, (const float*)actions, k);
  else hipLaunchKernelGGL(k_whatif_start<double>, grid, block, 0, st, d, s, (const double*)actions, k);
}
void launch_whatif_score(const Dev& d, const WhatifState& s, int k, hipStream_t st) {
  hipLaunchKernelGGL(k_whatif_score, dim3((d.B + DL - 1) / DL), dim3(DL * DS), 0, st, d, s, k);
}

}  // namespace mapdn
