// droop.hip — the reference's Volt/VAR droop controller (traditional_control/pf_droop_matpower_all.m:84-162, law :196-231) as a
// batched baseline: per env step, power flow -> |V| at the sgen buses -> droop law -> damped update, until the voltages stop moving.
// The solves are the handle's own power-flow kernels in MODE_SOLVE (baselines_host.hpp, droop_run); this file holds the one kernel
// that runs between them.  Included at the end of kernels.hip (one translation unit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "ctlloop.hpp"
#include "droop.hpp"

namespace mapdn {

// Layout and shared steps: ctlloop.hpp.
// iter == 0: start — a = 0, v_last = 100 (the script restarts from q = 0 every time step, :108), status 3 and a NaN row of voltages for
// envs that step() would not solve, the Sbus of the first solve.  iter = i > 0: after the i-th solve — stop test, damped update, next
// Sbus.  Envs that stop leave the solver's active set (s.act), so the next solves skip them.  The norm is summed by one thread per env
// in sgen order (the terms pass through s.dv2), so that it has the bits of a sequential sum.
__global__ void __launch_bounds__(DL * DS) k_droop_update(Dev d, DroopState s, int iter) {
  __shared__ int s_run[DL];                      // per env lane: 0 stopped, 1 iterating, 2 stops now (record a_sol, |V|)
  const CtlLane t = ctl_lane(d);
  const int el = t.el, sl = t.sl, e = t.e;
  const size_t S = (size_t)d.Bp;
  const double* __restrict__ vout = d.nrbuf;
  if (iter == 0) {
    const bool run = ctl_start(d, s, t);
    if (t.valid) {
      for (int j = sl; j < d.ns; j += DS) { const size_t o = (size_t)j * S + e; s.a[o] = 0.0; s.a_sol[o] = 0.0; s.v_last[o] = 100.0; }
      if (run) ctl_mlo_rows(d, t); else ctl_no_voltages(d, s, t);
    }
    ctl_next_solve(d, s, t, iter, run);
    return;
  }
  const bool act = t.valid && s.act[e] != 0;
  const bool conv_pf = act && s.nr_conv[e] != 0;
  if (conv_pf)
    for (int j = sl; j < d.ns; j += DS) {
      const size_t o = (size_t)j * S + e;
      const double dv = vout[(size_t)s.sg_vrow[j] * S + e] - s.v_last[o];
      s.dv2[o] = dv * dv;
    }
  __syncthreads();
  if (sl == 0) {
    int run = 0;
    if (act) {
      s.iters[e] = iter;
      if (!conv_pf) s.status[e] = DROOP_PF_FAILED;   // the solve failed: stop with the last action whose solve converged (a_sol)
      else {
        double ss = 0.0;
        for (int j = 0; j < d.ns; ++j) ss = droop_dv2_sum(ss, s.dv2[(size_t)j * S + e]);
        const bool conv = sqrt(ss) < s.v_tol;
        if (conv || iter >= s.max_iter) { s.status[e] = conv ? DROOP_CONVERGED : DROOP_MAX_ITER; run = 2; }
        else run = 1;
      }
      s.act[e] = run == 1 ? 1 : 0;
    }
    s_run[el] = run;
  }
  __syncthreads();
  const int run = s_run[el];
  if (act && run == 0) ctl_no_voltages(d, s, t);   // failed solve
  if (run == 2) ctl_record(d, s, t);
  if (run == 1)
    for (int j = sl; j < d.ns; j += DS) {
      const size_t o = (size_t)j * S + e;
      const double v = vout[(size_t)s.sg_vrow[j] * S + e];
      const double a = s.a[o];
      const double p = d.cur_pv[o], sm = d.smax[j];
      const double lim = q_limit(p, sm);
      s.v_last[o] = v;
      s.a_sol[o] = a;
      s.a[o] = droop_damped(a, droop_target(droop_law(v, s.va, s.vb, s.vc, s.vd), s.ratio, sm, lim), s.damping);
    }
  ctl_next_solve(d, s, t, iter, run == 1);
}

void launch_droop_update(const Dev& d, const DroopState& s, int iter, hipStream_t st) {
  hipLaunchKernelGGL(k_droop_update, dim3((d.B + DL - 1) / DL), dim3(DL * DS), 0, st, d, s, iter);
}

}  // namespace mapdn
