// droop.hip — the reference's Volt/VAR droop controller (traditional_control/pf_droop_matpower_all.m:84-162, law :196-231) as a
// batched baseline: per env step, power flow -> |V| at the sgen buses -> droop law -> damped update, until the voltages stop moving.
// The solves are the handle's own power-flow kernels in MODE_SOLVE (capi.hip, mapdn_droop_actions); this file holds the one kernel
// that runs between them.  Included at the end of kernels.hip (one translation unit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "droop.hpp"

namespace mapdn {

// Layout: a workgroup serves DL envs with DS sub-lanes each (thread t: env lane t % DL, sub-lane t / DL); sub-lane s takes the sgens
// j = s, s + DS, ... and the PV buses jb = s, s + DS, ...: DL = 16 consecutive envs keep the env-minor rows coalesced (128 bytes),
// and B / 16 workgroups fill the chip where one thread per env left all but B / 256 CUs idle.
constexpr int DL = 16, DS = 16;

// The PV-bus Sbus entry of bus jb of env e for the actions a (env-minor [ns][Bp]) into the Sbus buffer the next solve reads (d.sb_off):
// the expressions of k_inject_sgen in its order — the load part of the bus (bus_ld, or the sum of the stored loads of a bus with
// several), minus p and q = sqrt(s_max^2 - p^2) a of every sgen on it — so that the droop solve and the step() that applies its
// actions solve the same Sbus.
__device__ __forceinline__ void droop_pv_row(const Dev& d, int e, int jb, const double* __restrict__ a) {
  const int k = d.sgb_pos[jb];
  double P, Q;
  if (d.load_ptr[k + 1] - d.load_ptr[k] > 1) {
    P = 0.0; Q = 0.0;
    for (int i = d.load_ptr[k]; i < d.load_ptr[k + 1]; ++i) {
      const int li = d.load_idx[i];
      P += d.cur_pl[(size_t)li * d.Bp + e] * d.load_scale[li]; Q += d.cur_ql[(size_t)li * d.Bp + e] * d.load_scale[li];
    }
  } else { const double2 v = ((const double2*)d.bus_ld)[(size_t)jb * d.Bp + e]; P = v.x; Q = v.y; }
  for (int i = d.sgen_ptr[k]; i < d.sgen_ptr[k + 1]; ++i) {
    const int j = d.sgen_idx[i];
    const size_t o = (size_t)j * d.Bp + e;
    const double p = d.cur_pv[o];
    const double sm = d.smax[j];
    const double lim = sqrt(sm * sm - p * p);
    const double q = lim * a[o];
    P -= p * d.sgen_scale[j]; Q -= q * d.sgen_scale[j];
  }
  if (k < d.n) ((double2*)((char*)d.nrbuf + d.sb_off))[(size_t)k * d.Bp + e] = make_double2(-P / d.sn, -Q / d.sn);
}

// iter == 0: start — a = 0, v_last = 100 (the script restarts from q = 0 every time step, :108), status 3 for envs that step() would
// not solve (done: terminated, frozen, or waiting for their auto-reset restart), the load-only buses with several loads and the PV
// buses of Sbus for the first solve.  iter = i > 0: after the i-th solve — stop test, damped update, next Sbus.  Envs that stop leave
// the solver's active set (s.act), so the next solves skip them.  Counts the envs still iterating into s.n_active[iter] (the host polls
// it).  The norm is summed by one thread per env in sgen order (the terms pass through s.dv2), so that it has the bits of a sequential sum.
__global__ void __launch_bounds__(DL * DS) k_droop_update(Dev d, DroopState s, int iter) {
  __shared__ int s_run[DL];                      // per env lane: 0 stopped, 1 iterating, 2 stops now (record a_sol, |V|)
  const int el = (int)threadIdx.x % DL, sl = (int)threadIdx.x / DL;
  const int e = (int)blockIdx.x * DL + el;
  const bool valid = e < d.B;
  const size_t S = (size_t)d.Bp;
  const double* __restrict__ vout = d.nrbuf;
  if (iter == 0) {
    const bool run = valid && d.done[e] == 0;
    if (valid) {
      for (int j = sl; j < d.ns; j += DS) { const size_t o = (size_t)j * S + e; s.a[o] = 0.0; s.a_sol[o] = 0.0; s.v_last[o] = 100.0; }
      if (sl == 0) { s.iters[e] = 0; s.status[e] = run ? DROOP_RUNNING : DROOP_STOPPED; s.act[e] = run ? 1 : 0; }
      if (run) {
        for (int i = sl; i < d.n_mlo; i += DS) {   // (k_advance leaves these to the injection of the step)
          const int k = d.mlo_pos[i];
          double P = 0.0, Q = 0.0;
          for (int q = d.load_ptr[k]; q < d.load_ptr[k + 1]; ++q) {
            const int li = d.load_idx[q];
            P += d.cur_pl[(size_t)li * S + e] * d.load_scale[li]; Q += d.cur_ql[(size_t)li * S + e] * d.load_scale[li];
          }
          ((double2*)((char*)d.nrbuf + d.sb_off))[(size_t)k * S + e] = make_double2(-P / d.sn, -Q / d.sn);
        }
      } else if (s.vm_out) {
        for (int b = sl; b < d.nbo; b += DS) s.vm_out[(size_t)e * d.nbo + b] = __builtin_nan("");
      }
    }
    __syncthreads();                               // (a = 0 of every sgen of a bus before its row)
    if (run) for (int jb = sl; jb < d.n_sgb; jb += DS) droop_pv_row(d, e, jb, s.a);
    const unsigned long long m = __ballot(run && sl == 0);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(s.n_active + iter, (int)__popcll(m));
    return;
  }
  const bool act = valid && s.act[e] != 0;
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
  if (act && run == 0 && s.vm_out)                 // failed solve: no voltages
    for (int b = sl; b < d.nbo; b += DS) s.vm_out[(size_t)e * d.nbo + b] = __builtin_nan("");
  if (run == 2) {
    for (int j = sl; j < d.ns; j += DS) s.a_sol[(size_t)j * S + e] = s.a[(size_t)j * S + e];
    if (s.vm_out) for (int b = sl; b < d.nbo; b += DS) s.vm_out[(size_t)e * d.nbo + b] = vout[(size_t)s.vm_row[b] * S + e];
  }
  if (run == 1)
    for (int j = sl; j < d.ns; j += DS) {
      const size_t o = (size_t)j * S + e;
      const double v = vout[(size_t)s.sg_vrow[j] * S + e];
      const double a = s.a[o];
      const double p = d.cur_pv[o], sm = d.smax[j];
      const double lim = sqrt(sm * sm - p * p);
      s.v_last[o] = v;
      s.a_sol[o] = a;
      s.a[o] = droop_damped(a, droop_target(droop_law(v, s.va, s.vb, s.vc, s.vd), s.ratio, sm, lim), s.damping);
    }
  __syncthreads();                                 // (the new a of every sgen of a bus before its row)
  if (run == 1) for (int jb = sl; jb < d.n_sgb; jb += DS) droop_pv_row(d, e, jb, s.a);
  const unsigned long long m = __ballot(run == 1 && sl == 0);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(s.n_active + iter, (int)__popcll(m));
}

void launch_droop_update(const Dev& d, const DroopState& s, int iter, hipStream_t st) {
  hipLaunchKernelGGL(k_droop_update, dim3((d.B + DL - 1) / DL), dim3(DL * DS), 0, st, d, s, iter);
}

}  // namespace mapdn
