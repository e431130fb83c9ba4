// grad.hip — mapdn_action_gradients: d reward / d action of every candidate that mapdn_evaluate_actions would score,
// by one adjoint solve per (env, candidate) on the elimination tree.  In the what-if frame (baselines_host.hpp, grad_run), per candidate:
//   k_whatif_start  ->  the solve (MODE_SOLVE)  ->  k_action_grad  ->  k_whatif_score
// k_action_grad reads the frame's Vout rows, its active set and its action rows and writes its own workspace and grad[e][k][:] only,
// so the scoring launch after it sees what it sees in mapdn_evaluate_actions.  The arithmetic is in grad.hpp.
// Included at the end of kernels.hip (one translation unit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "grad.hpp"

namespace mapdn {

static_assert(MAPDN_BARRIER_L1 == 0 && MAPDN_BARRIER_L2 == 1 && MAPDN_BARRIER_COURANT_BELTRAMI == 2 && MAPDN_BARRIER_BOWL == 3 &&
              MAPDN_BARRIER_BUMP == 4, "nrmath.hpp barrier_deriv switches on these numbers");

// Layout: one lane per env, GRAD_WG = 64 consecutive envs per one-wave workgroup.  An env's work is one chain of dependent 2x2 block
// operations along the tree (the right-hand side, leaf -> root, root -> leaf, the read-out): there is one column per env, so sub-lanes
// would have nothing to share and every hand-off between them would be a barrier on the chain.  A wave costs the same time with 16 or
// 64 lanes at work, so the full wave gives the fewest waves per batch and 512-byte rows of the env-minor workspace; no LDS, no
// barrier, no atomics: every sum runs in its lane, in the order of the plan, whatever B, K and the env's place in the batch are.
constexpr int GRAD_WG = 64;

__global__ void __launch_bounds__(GRAD_WG) k_action_grad(Dev d, GradState s, int k) {
  const int e = (int)blockIdx.x * GRAD_WG + (int)threadIdx.x;
  if (e >= d.B) return;
  const int n = d.n, ns = d.ns;
  const size_t Bp = (size_t)d.Bp;
  double* __restrict__ out = s.grad + ((size_t)e * s.K + k) * ns;
  if (s.act[e] == 0 || s.nr_conv[e] == 0) {            // status 3 or 2: no gradient
    for (int j = 0; j < ns; ++j) out[j] = __builtin_nan("");
    return;
  }
  // A solved row whose q_j = lim_j a_j is not finite for some j (a NaN or infinite action on an sgen of the slack bus, whose injection
  // no solve reads; a NaN lim where p exceeds s_max): its reward is not finite, and sign0(NaN) = 0 would report a stationary point.
  bool q_finite = true;
  for (int j = 0; j < ns; ++j) {
    const size_t o = (size_t)j * Bp + e;
    q_finite = q_finite && isfinite(q_limit(d.cur_pv[o], d.smax[j]) * s.a[o]);
  }
  if (!q_finite) {
    for (int j = 0; j < ns; ++j) out[j] = __builtin_nan("");
    return;
  }
  const OpfVec E{d.nrbuf + ((size_t)d.r_vout + VO_E) * Bp + e, VOF * Bp}, F{d.nrbuf + ((size_t)d.r_vout + VO_F) * Bp + e, VOF * Bp},
      VM{d.nrbuf + ((size_t)d.r_vout + VO_VM) * Bp + e, VOF * Bp};
  const OpfVec fac{s.fac + e, Bp}, lam{s.lam + e, Bp};
  const GradCfg c = {d.nbo, d.n_line, ns, d.use_line_weight, d.barrier_type, d.voltage_weight, d.q_weight, d.line_weight};
  for (int p = 0; p < n; ++p) { lam[(size_t)p * 2] = 0.0; lam[(size_t)p * 2 + 1] = grad_barrier_rhs(c, VM[p]); }
  if (c.use_line_weight)
    for (int l = 0; l < d.n_line; ++l) {
      const LineFlow L = d.lines[l];
      grad_line_rhs(c, d.sn, L.c, L.fpos, L.tpos, n, E, F, lam);
    }
  grad_adjoint(n, s.par, s.cptr, s.cidx, s.yt, E, F, fac, lam);
  for (int j = 0; j < ns; ++j) {
    const size_t o = (size_t)j * Bp + e;
    out[j] = grad_entry(c, d.sn, q_limit(d.cur_pv[o], d.smax[j]), d.sgen_scale[j], s.a[o], s.sg_node[j], n, lam);
  }
}

void launch_action_grad(const Dev& d, const GradState& s, int k, hipStream_t st) {
  hipLaunchKernelGGL(k_action_grad, dim3((d.B + GRAD_WG - 1) / GRAD_WG), dim3(GRAD_WG), 0, st, d, s, k);
}

}  // namespace mapdn
