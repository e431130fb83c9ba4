// inject.hpp — the bus injection, written once: pandapower build_bus._calc_pq_elements_and_add_on_ppc + makeSbus,
// Sbus[k] = -(sum load - sum sgen) / sn_mva, with the sgen q of _clip_reactive_power (voltage_control_env.py:568-572), and the
// per-env turn of a step() / reset() call.  k_inject, k_inject_sgen (kernels.hip) and the control loops (ctlloop.hpp) call these
// functions; the prologue of k_nr_tree (nr_tree.hpp) keeps a hand-scheduled copy that must match them bit for bit.
// Device-only; kernels.hpp includes this header after Dev: include kernels.hpp, not this file alone.
#pragma once
#include "philox.hpp"     // Philox4x32-10, u53 (host-checkable: tests/test_philox.py)

namespace mapdn {

// One term of a bus's element sum, PD = sum p_mw x scaling (pd2ppc).  k_inject, k_inject_sgen, the prologue of k_nr_tree and the control
// loops (ctlloop.hpp) form the same sums and must land on the same bits, so the fused multiply-add is spelled out here: written as
// `P += p * s` the compiler fused it in some of these loops and not in others.  Scalings of 1 cannot show that (both forms are then
// P + p); a bus with several loads and scalings other than 1 did (tests/test_element_edges_gpu.py).
__device__ __forceinline__ void add_scaled(double& acc, double x, double s) { acc = fma(x, s, acc); }
__device__ __forceinline__ void sub_scaled(double& acc, double x, double s) { acc = fma(-x, s, acc); }
// scheduled injection of the bus at position k as an (re, im) pair from its demand (loads - sgens, MW / MVAr).  A generator on the bus
// (mapdn_netspec.gen_*) is a constant negative demand, Sbus_k = (P_gen - PD_k - j QD_k) / sn_mva: every path that writes an Sbus entry
// comes through here, so they all see it (d.n_gen == 0, a wave-uniform test: the expression of before)
__device__ __forceinline__ double2 sbus_entry(const Dev& d, int k, double P, double Q) {
  if (d.n_gen) P -= d.gen_p_pos[k];
  return make_double2(-P / d.sn, -Q / d.sn);
}
// _clip_reactive_power: the reactive limit of a sgen at active power p, and q = a x limit
__device__ __forceinline__ double q_limit(double p, double sm) { return sqrt(sm * sm - p * p); }
__device__ __forceinline__ double clip_q(double p, double sm, double a) {
  const double lim = q_limit(p, sm);
  return lim * a;
}

// episode start row of reset(): hour, day, interval sampled in the order of voltage_control_env.py:111-113 from the
// env's Philox stream (mapping in oracle/philox.py)
__device__ __forceinline__ int64_t sample_start_row(const Dev& d, int e, uint32_t draw) {
  uint32_t x[4];
  philox4x32_10((uint32_t)(d.env_id_offset + e), draw, STREAM_START, 0u, d.seed_lo, d.seed_hi, x);
  const int64_t hour = (int64_t)(((uint64_t)x[0] * 24u) >> 32);                        // :384
  const int64_t day = (int64_t)(((uint64_t)x[1] * (uint64_t)d.n_start_days) >> 32);    // :398
  const int64_t interval = (int64_t)(((uint64_t)x[2] * (uint64_t)d.per_hour) >> 32);   // :389
  return interval + hour * d.per_hour + day * d.per_day;                                // :445
}
// Box-Muller pair of Philox block b of a stream: the two half-normal noise factors of columns 2b, 2b + 1
__device__ __forceinline__ void noise_pair(const Dev& d, int e, uint32_t draw, int stream, int b, double& n0, double& n1) {
  uint32_t x[4];
  philox4x32_10((uint32_t)(d.env_id_offset + e), draw, (uint32_t)stream, (uint32_t)b, d.seed_lo, d.seed_hi, x);
  const double u1 = (u53(x[0], x[1]) + 0.5) * (1.0 / 9007199254740992.0);
  const double u2 = u53(x[2], x[3]) * (1.0 / 9007199254740992.0);
  const double r = sqrt(-2.0 * log(u1));
  double sn_, cs_;
  sincos(2.0 * M_PI * u2, &sn_, &cs_);
  n0 = fabs(r * cs_); n1 = fabs(r * sn_);
}
// one column of _set_demand_and_pv (:491-513): table value + std/100 * |N(0,1)|; column j of a stream takes the cosine
// (even j) or sine (odd j) branch of the pair of Philox block j >> 1 — the same numbers k_advance produces pairwise
__device__ __forceinline__ double profile_value(const Dev& d, int e, int64_t row, uint32_t draw, int stream, int j, int col0, int add_noise) {
  double v = d.table[(size_t)row * d.ncol + col0 + j];
  if (add_noise) {
    double n0, n1;
    noise_pair(d, e, draw, stream, j >> 1, n0, n1);
    v += d.stdv[col0 + j] * ((j & 1) ? n1 : n0);
  }
  return v;
}
// random initial action of sgen j at a (re)start (:120-122, get_action :337): half (j & 1) of Philox block j >> 1, in [action_low, action_high]
__device__ __forceinline__ double reset_action(const Dev& d, int e, uint32_t draw, int j) {
  uint32_t x[4];
  philox4x32_10((uint32_t)(d.env_id_offset + e), draw, STREAM_ACTION, (uint32_t)(j >> 1), d.seed_lo, d.seed_hi, x);
  const double u = ((j & 1) ? u53(x[2], x[3]) : u53(x[0], x[1])) * (1.0 / 9007199254740992.0);
  return d.action_low + (d.action_high - d.action_low) * u;
}

// ---- the turn of env e in a launch of `mode`.  act: the env takes part (frozen envs keep q_new and Sbus).  ar (auto_reset): an env that
// terminated in an earlier step() starts its next episode in this one (reset(), :96-135, for this env alone) — new start row, first
// profile row of the window ar_row (+ noise), random initial action — element by element by the thread of the element's bus, so that
// every cur_* entry still has exactly one writer.  draw: the env's Philox draw counter of this call.  (MODE_SOLVE: every lane acts.)
struct EnvTurn { bool act, ar; uint32_t draw; int64_t ar_row; };
__device__ __forceinline__ EnvTurn env_turn(const Dev& d, int mode, int e) {
  EnvTurn t = {true, false, 0u, 0};
  if (mode == MODE_SOLVE) return t;
  if (e >= d.B) t.act = false;
  else if (mode == MODE_STEP) {
    const bool dn = d.done[e] != 0;
    t.ar = dn && d.auto_reset;
    t.act = !dn || t.ar;
  } else t.act = d.pending[e] != 0;
  t.draw = mode == MODE_STEP ? d.draw[e] : d.adv_draw[e];
  if (t.ar) t.ar_row = sample_start_row(d, e, t.draw) + 1;   // t = self.steps == 1 (:100, :473)
  return t;
}
// what ONE thread per env (row 0 of the launch) records of the turn
__device__ __forceinline__ void note_turn(const Dev& d, int mode, int e, const EnvTurn& t) {
  if (mode == MODE_SOLVE) return;
  if (t.ar) d.start_row[e] = t.ar_row - 1;
  d.active[e] = t.act ? 1 : 0;
  if (mode == MODE_STEP) {
    d.resetting[e] = t.ar ? 1 : 0;
    // step(): the next profile row is row `steps` (before the increment, :199 vs :202) of the episode window and
    // uses the env's current draw counter; queued here, before the solve (frozen / restarting envs do not advance)
    d.adv_row[e] = (t.act && !t.ar) ? d.start_row[e] + d.steps[e] : -1; d.adv_draw[e] = t.draw;
  }
}

// ---- load part of the injection of the bus at position k: sum p_mw x scaling in the canonical order of its CSR list (ONE thread per bus)
// ... of the element values pl, ql [nl][Bp] (the env's stored loads d.cur_pl / d.cur_ql, or the caller's in MODE_SOLVE)
__device__ __forceinline__ void stored_load_sum(const Dev& d, int k, int e, const double* __restrict__ pl, const double* __restrict__ ql,
                                                double& P, double& Q) {
  P = 0.0; Q = 0.0;
  for (int i = d.load_ptr[k]; i < d.load_ptr[k + 1]; ++i) {
    const int li = d.load_idx[i];
    const size_t o = (size_t)li * d.Bp + e;
    add_scaled(P, pl[o], d.load_scale[li]); add_scaled(Q, ql[o], d.load_scale[li]);
  }
}
// ... of a restarting env: the loads of profile row ar_row (+ noise), which become the env's stored loads
__device__ __forceinline__ void restart_load_sum(const Dev& d, int k, int e, int64_t ar_row, uint32_t draw, int add_noise, double& P, double& Q) {
  P = 0.0; Q = 0.0;
  for (int i = d.load_ptr[k]; i < d.load_ptr[k + 1]; ++i) {
    const int li = d.load_idx[i];
    const size_t o = (size_t)li * d.Bp + e;
    const double p = profile_value(d, e, ar_row, draw, STREAM_LOAD_P, li, d.ns, add_noise);
    const double q = profile_value(d, e, ar_row, draw, STREAM_LOAD_Q, li, d.ns + d.nl, add_noise);
    d.cur_pl[o] = p; d.cur_ql[o] = q;
    add_scaled(P, p, d.load_scale[li]); add_scaled(Q, q, d.load_scale[li]);
  }
}
// ... of PV bus jb (position k) between two steps: k_advance left it in bus_ld unless the bus has several loads
__device__ __forceinline__ void pv_bus_load_sum(const Dev& d, int jb, int k, int e, double& P, double& Q) {
  if (d.load_ptr[k + 1] - d.load_ptr[k] > 1) stored_load_sum(d, k, e, d.cur_pl, d.cur_ql, P, Q);
  else { const double2 v = ((const double2*)d.bus_ld)[(size_t)jb * d.Bp + e]; P = v.x; Q = v.y; }
}

// ---- sgen part: (P, Q) minus p and q x scaling of every sgen on the bus at position k.  p is the stored pv [ns][Bp], or for a restarting
// env that of profile row t.ar_row (stored, with cur_q = 0); q = q_of(j, o, p) of sgen j, element offset o — the caller's rule
template <typename QF>
__device__ __forceinline__ void sub_bus_sgens(const Dev& d, int k, int e, const EnvTurn& t, const double* __restrict__ pv, int add_noise,
                                              QF q_of, double& P, double& Q) {
  for (int i = d.sgen_ptr[k]; i < d.sgen_ptr[k + 1]; ++i) {
    const int j = d.sgen_idx[i];
    const size_t o = (size_t)j * d.Bp + e;
    double p;
    if (t.ar) { p = profile_value(d, e, t.ar_row, t.draw, STREAM_PV, j, 0, add_noise); d.cur_pv[o] = p; d.cur_q[o] = 0.0; }
    else p = pv[o];
    const double q = q_of(j, o, p);
    sub_scaled(P, p, d.sgen_scale[j]); sub_scaled(Q, q, d.sgen_scale[j]);
  }
}
// q of sgen j of an env that takes its turn: the clipped action of step(), at a (re)start the clipped random action or the base net's
// q_mvar = 0 (deepcopy of base_powergrid, :106); actions [B, ns] env-major
template <typename AT>
__device__ __forceinline__ double turn_q(const Dev& d, int mode, const EnvTurn& t, const AT* __restrict__ actions, int e, int j, double p) {
  if (mode == MODE_STEP && !t.ar) return clip_q(p, d.smax[j], (double)actions[(size_t)e * d.ns + j]);
  return d.reset_action ? clip_q(p, d.smax[j], reset_action(d, e, t.draw, j)) : 0.0;
}

}  // namespace mapdn
