// ctlloop.hpp — the frame the traditional baselines share: a control loop around the handle's own power flow,
//   start launch  ->  [ solve (MODE_SOLVE, the loop's own active set)  ->  the baseline's update launch ] ...
// Its state (CtlLoop, the base of DroopState and OpfState), the thread layout of an update kernel and the steps that both update
// kernels take: the Sbus rows the next solve reads, the record of a solved point, the count the host polls.  What a baseline decides —
// its stop test and its law — is in its own kernel (droop.hip, opf.hip); nothing here knows which one calls it.
// kernels.hpp includes this header after Dev (the state structs there derive from CtlLoop): include kernels.hpp, not this file alone.
#pragma once

namespace mapdn {

// Per-env status values that both start launches write (include/mapdn.h; RUNNING only between launches)
enum { CTL_STOPPED = 3, CTL_RUNNING = 255 };

struct CtlLoop {
  int32_t max_iter;
  double *a, *a_sol;                 // [ns][Bp]: the action of the next solve, the action of the last converged solve
  int32_t* iters;                    // [Bp] solves so far
  uint8_t* status;                   // [Bp]
  uint8_t* act;                      // [Bp] the solver's active flags of the loop's solves (Dev::active of those launches)
  const int32_t* nr_iters; const uint8_t* nr_conv;   // [Bp] Dev::iters / conv of those launches
  const int32_t* vm_row;             // [nbo] row of nrbuf that holds |V| of every original bus (Vout, VO_VM)
  int32_t* n_active;                 // [max_iter + 1] envs still iterating after update i
  double* vm_out;                    // [B][nbo] env-major, or nullptr
};

// Layout: a workgroup serves DL envs with DS sub-lanes each (thread t: env lane t % DL, sub-lane t / DL); sub-lane s takes the sgens
// j = s, s + DS, ... and the PV buses jb = s, s + DS, ...: DL = 16 consecutive envs keep the env-minor rows coalesced (128 bytes),
// and B / 16 workgroups fill the chip where one thread per env left all but B / 256 CUs idle.
constexpr int DL = 16, DS = 16;
struct CtlLane { int el, sl, e; bool valid; };     // env lane, sub-lane, env, e < B
__device__ __forceinline__ CtlLane ctl_lane(const Dev& d) {
  const int el = (int)threadIdx.x % DL, sl = (int)threadIdx.x / DL;
  const int e = (int)blockIdx.x * DL + el;
  return {el, sl, e, e < d.B};
}

// The PV-bus Sbus entry of bus jb of env e for the actions a (env-minor [ns][Bp]) into the Sbus buffer the next solve reads (d.sb_off):
// the row k_inject_sgen writes for a stepping env (inject.hpp), with q = sqrt(s_max^2 - p^2) a of every sgen on the bus — so that the
// loop's solve and the step() that applies its actions solve the same Sbus.
__device__ __forceinline__ void ctl_pv_row(const Dev& d, int e, int jb, const double* __restrict__ a) {
  const int k = d.sgb_pos[jb];
  const EnvTurn stepping = {true, false, 0u, 0};
  double P, Q;
  pv_bus_load_sum(d, jb, k, e, P, Q);
  sub_bus_sgens(d, k, e, stepping, d.cur_pv, 0, [&](int j, size_t o, double p) { return clip_q(p, d.smax[j], a[o]); }, P, Q);
  if (k < d.n) ((double2*)((char*)d.nrbuf + d.sb_off))[(size_t)k * d.Bp + e] = sbus_entry(d, k, P, Q);
}

// The Sbus rows of the load-only buses with several loads (k_advance leaves these to the injection of the step)
__device__ __forceinline__ void ctl_mlo_rows(const Dev& d, const CtlLane& t) {
  for (int i = t.sl; i < d.n_mlo; i += DS) {
    const int k = d.mlo_pos[i];
    double P, Q;
    stored_load_sum(d, k, t.e, d.cur_pl, d.cur_ql, P, Q);
    ((double2*)((char*)d.nrbuf + d.sb_off))[(size_t)k * d.Bp + t.e] = sbus_entry(d, k, P, Q);
  }
}

// The start bookkeeping: whether step() would solve the env (not done: neither terminated, frozen, nor waiting for its auto-reset
// restart), no solves so far, status RUNNING or STOPPED, and the env's place in the solver's active set
__device__ __forceinline__ bool ctl_start(const Dev& d, const CtlLoop& s, const CtlLane& t) {
  const bool run = t.valid && d.done[t.e] == 0;
  if (t.valid && t.sl == 0) { s.iters[t.e] = 0; s.status[t.e] = run ? CTL_RUNNING : CTL_STOPPED; s.act[t.e] = run ? 1 : 0; }
  return run;
}

// This solved point is the one the loop would return: a_sol <- a, and |V| of every original bus when the caller asked for it
__device__ __forceinline__ void ctl_record(const Dev& d, const CtlLoop& s, const CtlLane& t) {
  const size_t S = (size_t)d.Bp;
  const double* __restrict__ vout = d.nrbuf;
  for (int j = t.sl; j < d.ns; j += DS) s.a_sol[(size_t)j * S + t.e] = s.a[(size_t)j * S + t.e];
  if (s.vm_out) for (int b = t.sl; b < d.nbo; b += DS) s.vm_out[(size_t)t.e * d.nbo + b] = vout[(size_t)s.vm_row[b] * S + t.e];
}

// No voltages for this env: a row of NaN
__device__ __forceinline__ void ctl_no_voltages(const Dev& d, const CtlLoop& s, const CtlLane& t) {
  if (s.vm_out) for (int b = t.sl; b < d.nbo; b += DS) s.vm_out[(size_t)t.e * d.nbo + b] = __builtin_nan("");
}

// The end of every update launch, for the envs that go on to the next solve (go): their next Sbus for the actions s.a — the barrier
// (the a of every sgen of a bus before its row), then the PV rows — and their number, each env counted once, into s.n_active[iter],
// which the host polls
__device__ __forceinline__ void ctl_next_solve(const Dev& d, const CtlLoop& s, const CtlLane& t, int iter, bool go) {
  __syncthreads();
  if (go) for (int jb = t.sl; jb < d.n_sgb; jb += DS) ctl_pv_row(d, t.e, jb, s.a);
  const unsigned long long m = __ballot(go && t.sl == 0);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(s.n_active + iter, (int)__popcll(m));
}

}  // namespace mapdn
