// opf.hip — the paper's second traditional baseline, optimal power flow (traditional_control/*.m: runopf on the loss objective with
// the PV inverters' reactive power as the controls), as a batched reduced-space SQP: per env and per outer iteration
//   power flow at a  ->  k_opf_linearise (S = d|V|/da, g, the Gauss-Newton H at the converged V)  ->  k_opf_qp (the step d)  ->
//   k_opf_update (stop test, a <- clip(a + t d), the next Sbus).
// The power flows are the handle's own kernels in MODE_SOLVE with the OPF's own active set (baselines_host.hpp, opf_run), in the frame
// the droop loop runs in (ctlloop.hpp).  The arithmetic is in opf.hpp.  Included at the end of kernels.hip (one translation unit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "ctlloop.hpp"
#include "opf.hpp"

namespace mapdn {

// Layout: ctlloop.hpp (DL = 16 consecutive envs with DS = 16 sub-lanes each); sub-lane s takes the columns (sgens) j = s, s + DS, ...
static_assert(OPF_STOPPED == CTL_STOPPED && OPF_RUNNING == CTL_RUNNING, "ctl_start writes the OPF's status values");

// After a solve, for every env whose power flow converged: the block LU of the Jacobian on the tree (sub-lane 0, node by node, the
// children of a node summed in the plan's canonical order: no atomics, the same bits in every run), then per column the forward path
// and the backward sweep, S, dV = (dE, dF), W = M dV and g, and last H_ij = 2 Re(dV_i^H W_j).  M = (Ybus + Ybus^H) / 2 is applied
// branch by branch (node k with its parent and its children) and never formed.  Also the loss V^H M V and the voltage violation.
__global__ void __launch_bounds__(DL * DS) k_opf_linearise(Dev d, OpfState s) {
  const int el = (int)threadIdx.x % DL, sl = (int)threadIdx.x / DL;
  const int e = (int)blockIdx.x * DL + el;
  const bool go = e < d.B && s.act[e] != 0 && s.nr_conv[e] != 0;
  const size_t Bp = (size_t)d.Bp;
  const int n = d.n, ns = d.ns;
  const size_t ee = go ? (size_t)e : 0;
  const OpfVec E{d.nrbuf + ((size_t)d.r_vout + VO_E) * Bp + ee, VOF * Bp}, F{d.nrbuf + ((size_t)d.r_vout + VO_F) * Bp + ee, VOF * Bp},
      VM{d.nrbuf + ((size_t)d.r_vout + VO_VM) * Bp + ee, VOF * Bp};
  const OpfVec fac{s.fac + ee, Bp}, mv{s.mv + ee, Bp};
  if (go) {
    // (M V)_k = g_kk V_k + M_kp V_p + sum over the children of conj(M_c,k) V_c + M_ks V_s
    for (int k = sl; k < n; k += DS) {
      const double* y = s.yt + (size_t)k * OPF_YT;
      double mr = y[OY_KK] * E[k] + y[OY_MSV], mi = y[OY_KK] * F[k] + y[OY_MSV + 1];
      const int p = s.par[k];
      if (p < n) { mr += y[OY_MKP] * E[p] - y[OY_MKP + 1] * F[p]; mi += y[OY_MKP] * F[p] + y[OY_MKP + 1] * E[p]; }
      for (int i = s.cptr[k]; i < s.cptr[k + 1]; ++i) {
        const int c = s.cidx[i];
        const double* yc = s.yt + (size_t)c * OPF_YT;
        mr += yc[OY_MKP] * E[c] + yc[OY_MKP + 1] * F[c]; mi += yc[OY_MKP] * F[c] - yc[OY_MKP + 1] * E[c];
      }
      mv[(size_t)k * 2] = mr; mv[(size_t)k * 2 + 1] = mi;
    }
    if (sl == 0) {
      double viol = 0.0, P, Q;
      for (int k = 0; k < n; ++k) {
        opf_elim_step(k, n, s.par, s.cptr, s.cidx, s.yt, E, F, fac, &P, &Q);
        const double v = VM[k];
        viol = fmax(viol, fmax(v - s.v_upper, s.v_lower - v));
      }
      s.viol[e] = viol;
      s.lin[e] = 1;
    }
  } else if (e < d.B && sl == 0) s.lin[e] = 0;
  __syncthreads();
  if (go) {
    if (sl == DS - 1) {                            // the loss: conj(V_k) (M V)_k over the nodes, + the slack's row
      double loss = s.loss_slack;
      for (int k = 0; k < n; ++k) {
        const double* y = s.yt + (size_t)k * OPF_YT;
        loss += E[k] * mv[(size_t)k * 2] + F[k] * mv[(size_t)k * 2 + 1] + (y[OY_MSV] * E[k] + y[OY_MSV + 1] * F[k]);
      }
      s.loss[e] = loss;
    }
    for (int j = sl; j < ns; j += DS) {
      const size_t xs = (size_t)ns * 2;
      const OpfVec x{s.X + (size_t)j * 2 * Bp + ee, Bp}, w{s.W + (size_t)j * 2 * Bp + ee, Bp};
      const size_t o = (size_t)j * Bp + ee;
      const double p = d.cur_pv[o], sm = d.smax[j];
      const double wj = q_limit(p, sm) * d.sgen_scale[j] / d.sn;
      opf_solve_column(s.sg_node[j], wj, n, s.par, fac, x, xs);
      for (int k = 0; k < n; ++k) {                // S, then dV = (u + j dtheta) V in place of (dtheta, u)
        const double th = x[(size_t)k * xs], u = x[(size_t)k * xs + 1];
        s.S[((size_t)k * ns + j) * Bp + ee] = u * VM[k];
        x[(size_t)k * xs] = u * E[k] - th * F[k]; x[(size_t)k * xs + 1] = u * F[k] + th * E[k];
      }
      double g = 0.0;
      for (int k = 0; k < n; ++k) {                // W = M dV, branch by branch; g = 2 Re(dV^H M V)
        const double* y = s.yt + (size_t)k * OPF_YT;
        const double de = x[(size_t)k * xs], df = x[(size_t)k * xs + 1];
        double wr = y[OY_KK] * de, wi = y[OY_KK] * df;
        const int pk = s.par[k];
        if (pk < n) {
          const double pe = x[(size_t)pk * xs], pf = x[(size_t)pk * xs + 1];
          wr += y[OY_MKP] * pe - y[OY_MKP + 1] * pf; wi += y[OY_MKP] * pf + y[OY_MKP + 1] * pe;
        }
        for (int i = s.cptr[k]; i < s.cptr[k + 1]; ++i) {
          const int c = s.cidx[i];
          const double* yc = s.yt + (size_t)c * OPF_YT;
          const double ce = x[(size_t)c * xs], cf = x[(size_t)c * xs + 1];
          wr += yc[OY_MKP] * ce + yc[OY_MKP + 1] * cf; wi += yc[OY_MKP] * cf - yc[OY_MKP + 1] * ce;
        }
        w[(size_t)k * xs] = wr; w[(size_t)k * xs + 1] = wi;
        g += de * mv[(size_t)k * 2] + df * mv[(size_t)k * 2 + 1];
      }
      s.g[o] = 2.0 * g;
    }
  }
  __syncthreads();
  if (go)
    for (int j = sl; j < ns; j += DS) {
      const size_t xs = (size_t)ns * 2;
      const OpfVec w{s.W + (size_t)j * 2 * Bp + ee, Bp};
      for (int i = 0; i <= j; ++i) {
        const OpfVec x{s.X + (size_t)i * 2 * Bp + ee, Bp};
        double h = 0.0;
        for (int k = 0; k < n; ++k) h += x[(size_t)k * xs] * w[(size_t)k * xs] + x[(size_t)k * xs + 1] * w[(size_t)k * xs + 1];
        h *= 2.0;
        s.H[((size_t)i * ns + j) * Bp + ee] = h; s.H[((size_t)j * ns + i) * Bp + ee] = h;
      }
    }
}

// The QP of the envs that were linearised (opf_qp_solve, opf.hpp), no power flow.  The envs take different numbers of Newton steps,
// so a workgroup barrier would hold sixteen envs to the slowest one's path; instead a team never leaves its wave: a workgroup is one
// wave of OPF_QL consecutive envs with OPF_QS = 16 sub-lanes each (thread t: env lane t % OPF_QL, sub-lane t / OPF_QL).  The sub-lanes
// share the rows of S, H and K; sums and maxima go through a butterfly of lane exchanges, which adds in one fixed order and leaves the
// same bits in every sub-lane; a workgroup-scope fence orders the team's stores to its env-minor workspace before its later loads.
// The multipliers start from those of the env's previous QP (zero at the first, and after a QP that hit its cap).
constexpr int OPF_QL = 4, OPF_QS = 64 / OPF_QL;
struct OpfWaveTeam {                               // (device only: its exchanges have no host meaning)
  int sl;
  __device__ int lane() const { return sl; }
  __device__ int lanes() const { return OPF_QS; }
  __device__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
  __device__ double sum(double x) const {
    for (int m = OPF_QL; m < 64; m <<= 1) x += __shfl_xor(x, m);
    return x;
  }
  __device__ double max(double x) const {
    for (int m = OPF_QL; m < 64; m <<= 1) x = fmax(x, __shfl_xor(x, m));
    return x;
  }
};
__global__ void __launch_bounds__(64) k_opf_qp(Dev d, OpfState s) {
  const int e = (int)blockIdx.x * OPF_QL + (int)threadIdx.x % OPF_QL;
  if (e >= d.B || s.lin[e] == 0) return;
  const OpfWaveTeam tm{(int)threadIdx.x / OPF_QL};
  const size_t Bp = (size_t)d.Bp;
  OpfQp q;
  q.ns = d.ns; q.n = d.n;
  q.g = OpfVec{s.g + e, Bp}; q.H = OpfVec{s.H + e, Bp}; q.S = OpfVec{s.S + e, Bp};
  q.a = OpfVec{s.a + e, Bp}; q.v = OpfVec{d.nrbuf + ((size_t)d.r_vout + VO_VM) * Bp + e, VOF * Bp};
  q.vl = s.v_lower; q.vu = s.v_upper;
  const int warm = s.qp_capped[e] == 0;
  tm.sync();
  const OpfQpOut out = opf_qp_solve(tm, q, OpfVec{s.qd + e, Bp}, OpfVec{s.qy + e, Bp}, OpfVec{s.qw + e, Bp}, warm);
  if (tm.sl == 0) s.qp_capped[e] = (uint8_t)out.capped;
}

// iter == 0: start — a = 0 (or the caller's set-points s.a0, clipped: the probe), status 3 for the envs that step() would not solve,
// a NaN row of voltages for every env, the Sbus of the first solve.
// iter = i > 0: after the i-th solve and its QP, opf_decide (opf.hpp) — the solve failed: halve t (at most max_backtrack times in a
// row) and retry from the last solved a, or stop with status 2 (the |V| of the last solved point stay);  it converged: record a, |V|,
// loss and violation, stop with status 0 when |d|inf < step_tol, the violation is <= v_tol and the QP did not hit its cap, with
// status 1 at max_iter or at the least-violation point of bounds that cannot be met; else a <- clip(a + d).  Then the next Sbus.
__global__ void __launch_bounds__(DL * DS) k_opf_update(Dev d, OpfState s, int iter) {
  __shared__ int s_run[DL];                        // 0 not iterating, 1 next step, 2 stops at this solved point, 3 stops failed, 4 retry
  const CtlLane t = ctl_lane(d);
  const int el = t.el, sl = t.sl, e = t.e;
  const size_t S = (size_t)d.Bp;
  if (iter == 0) {
    const bool run = ctl_start(d, s, t);
    if (t.valid) {
      for (int j = sl; j < d.ns; j += DS) {
        const size_t o = (size_t)j * S + e;
        const double a0 = s.a0 ? opf_trial(s.a0[o], 0.0, 0.0) : 0.0;
        s.a[o] = a0; s.a_sol[o] = a0; s.qd[o] = 0.0;
      }
      for (int r = sl; r < d.ns + d.n; r += DS) s.qy[(size_t)r * S + e] = 0.0;
      if (sl == 0) {
        s.nback[e] = 0; s.t[e] = 1.0; s.lin[e] = 0; s.qp_capped[e] = 0;
        s.loss_out[e] = __builtin_nan(""); s.viol_out[e] = __builtin_nan("");
      }
      ctl_no_voltages(d, s, t);
      if (run) ctl_mlo_rows(d, t);
    }
    ctl_next_solve(d, s, t, iter, run);
    return;
  }
  const bool act = t.valid && s.act[e] != 0;
  if (sl == 0) {
    int run = 0;
    if (act) {
      s.iters[e] = iter;
      const bool solved = s.nr_conv[e] != 0;
      double dn = 0.0, viol = 0.0;
      if (solved) {
        for (int j = 0; j < d.ns; ++j) dn = fmax(dn, fabs(s.qd[(size_t)j * S + e]));
        viol = s.viol[e];
      }
      const OpfDecision dec = opf_decide(iter, solved, s.nback[e], s.t[e], dn, viol, s.viol_out[e], s.qp_capped[e] != 0,
                                         OpfLimits{s.step_tol, s.v_tol, s.max_iter, s.max_backtrack});
      run = dec.run;
      s.nback[e] = dec.nback; s.t[e] = dec.t;
      if (dec.status != OPF_RUNNING) s.status[e] = (uint8_t)dec.status;
      if (solved) { s.loss_out[e] = s.loss[e]; s.viol_out[e] = viol; }
      s.act[e] = (run == 1 || run == 4) ? 1 : 0;
    }
    s_run[el] = run;
  }
  __syncthreads();
  const int run = s_run[el];
  const bool go = run == 1 || run == 4;
  if (run == 1 || run == 2) ctl_record(d, s, t);
  if (go) {
    const double tt = s.t[e];
    for (int j = sl; j < d.ns; j += DS) {
      const size_t o = (size_t)j * S + e;
      s.a[o] = opf_trial(s.a_sol[o], tt, s.qd[o]);
    }
  }
  ctl_next_solve(d, s, t, iter, go);
}

void launch_opf_update(const Dev& d, const OpfState& s, int iter, hipStream_t st) {
  hipLaunchKernelGGL(k_opf_update, dim3((d.B + DL - 1) / DL), dim3(DL * DS), 0, st, d, s, iter);
}
void launch_opf_linearise(const Dev& d, const OpfState& s, hipStream_t st) {
  hipLaunchKernelGGL(k_opf_linearise, dim3((d.B + DL - 1) / DL), dim3(DL * DS), 0, st, d, s);
}
void launch_opf_qp(const Dev& d, const OpfState& s, hipStream_t st) {
  hipLaunchKernelGGL(k_opf_qp, dim3((d.B + OPF_QL - 1) / OPF_QL), dim3(64), 0, st, d, s);
}

}  // namespace mapdn
