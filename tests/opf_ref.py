"""CPU restatement (numpy float64) of the OPF baseline on the oracle's power flow: test infrastructure only, independent of the product
code (mapdn_opf_actions, csrc/opf.hpp, csrc/opf.hip).

The problem, per env, on the env's current state (loads and PV of the next step, noise applied):
  minimise   f(a) = sum_k Re(V_k conj((Ybus V)_k))          (the total active loss, p.u.; the script's sum(Pg) - sum(Pd))
  over       a in [-1, 1]^ns,  q_j = sqrt(s_max_j^2 - p_j^2) a_j
  subject to v_lower <= |V_k(a)| <= v_upper at every non-slack bus,   V(a) = runpp_restated.
Here: the objective, its exact sensitivities by dense solves with the oracle's Jacobian (S = d|V|/da, g, the Gauss-Newton H), the
QP routine and the SQP loop restated literally from csrc/opf.hpp / csrc/opf.hip, and a KKT residual of the NONLINEAR problem with
multipliers from a non-negative least squares over the near-active constraints.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from oracle.pp_restated import jacobian, make_ybus, runpp_restated

DEFAULTS = dict(v_lower=0.0, v_upper=0.0, v_tol=5e-6, step_tol=1e-6, max_iter=50, max_backtrack=8)
# the QP routine's constants (csrc/opf.hpp)
QP_RHO, QP_EPS, QP_MAX_OUTER, QP_MAX_NEWTON, QP_RIDGE, QP_SHRINK = 1e4, 1e-10, 60, 60, 1e-8, 0.25
QP_STALL, QP_MAX_STALL = 0.5, 4


def resolve(cfg=None, v_lower=0.95, v_upper=1.05) -> dict:
    """the defaults for every field that is None / 0 / missing (mapdn_opf_config's rule); v_lower / v_upper default to the env's"""
    c = dict(DEFAULTS, v_lower=v_lower, v_upper=v_upper)
    if cfg is not None:
        src = cfg if isinstance(cfg, dict) else {k: getattr(cfg, k, None) for k in DEFAULTS}
        for k, v in src.items():
            if v:
                c[k] = type(DEFAULTS[k])(v)
    return c


def limits(sgen_p, s_max):
    p = np.asarray(sgen_p, dtype=np.float64)
    return np.sqrt(s_max * s_max - p * p)


def loss_pu(ybus, V):
    return float(np.sum((V * np.conj(ybus @ V)).real))


class Lin(NamedTuple):
    S: np.ndarray     # [n_bus, ns]  d|V| / da (slack row 0)
    g: np.ndarray     # [ns]         df / da
    H: np.ndarray     # [ns, ns]     Gauss-Newton Hessian 2 Re(dV^H M dV), M the Hermitian part of Ybus
    dV: np.ndarray    # [n_bus, ns]  dV / da (complex)


def linearise(net, V, lim) -> Lin:
    """exact sensitivities at a converged V: J X = E with E_j = w_j e_{Q, bus(j)}, w_j = lim_j scaling_j / sn (dense solve)"""
    ybus = make_ybus(net)[0]
    nb, ns = net.n_bus, net.n_sgen
    pq = np.setdiff1d(np.arange(nb), [net.ext_grid_bus])
    n = pq.shape[0]
    J = jacobian(ybus, V, pq, pq).toarray()
    E = np.zeros((2 * n, ns))
    where = {int(b): i for i, b in enumerate(pq)}
    w = lim * net.sgen_scaling / net.sn_mva
    for j, b in enumerate(np.asarray(net.sgen_bus)):
        if int(b) in where:
            E[n + where[int(b)], j] = w[j]
    X = np.linalg.solve(J, E)
    dth, dvm = np.zeros((nb, ns)), np.zeros((nb, ns))
    dth[pq], dvm[pq] = X[:n], X[n:]
    vm = np.abs(V)
    dV = (dvm / vm[:, None] + 1j * dth) * V[:, None]
    M = ybus.toarray()
    M = 0.5 * (M + M.conj().T)
    g = 2.0 * (dV.conj().T @ (M @ V)).real
    H = 2.0 * (dV.conj().T @ (M @ dV)).real
    return Lin(dvm, g, 0.5 * (H + H.T), dV)


# ---- the QP of one SQP iteration:  min g'd + d'Hd / 2   s.t.  lo_r <= (A d)_r <= hi_r,  A = [I; S]  (box rows first) ------------------
class QPResult(NamedTuple):
    d: np.ndarray
    y: np.ndarray        # [ns + m] signed multipliers (> 0: upper bound active, < 0: lower)
    kkt: float           # the routine's KKT residual at (d, y)
    newton: int          # Newton steps in all
    capped: bool


def qp_kkt(g, H, A, lo, hi, d, y):
    """opf_qp_kkt (csrc/opf.hpp): (stationarity |g + H d + A'y|inf, violation, complementarity max |y_r| x distance to the bound)"""
    r = g + H @ d + A.T @ y
    c = A @ d
    viol = np.maximum(np.maximum(c - hi, lo - c), 0.0)
    comp = np.where(y > 0, y * np.abs(hi - c), np.where(y < 0, -y * np.abs(c - lo), 0.0))
    return float(np.abs(r).max()), float(viol.max()), float(comp.max())


def qp_solve(g, H, S, lo_box, hi_box, lo_row, hi_row, y0=None, expanded=False) -> QPResult:
    """Augmented Lagrangian on every row of A = [I; S] with a semismooth Newton inner solve, as opf_qp_solve (csrc/opf.hpp):
      phi(d) = g'd + d'Hd / 2 + sum_r psi(c_r),  c = A d,  psi = (rho / 2) dist^2 of (c_r + y_r / rho) to [lo_r, hi_r]
    Newton: (H + rho A_P' A_P + ridge) p = -grad phi over the penalised rows P, backtracking on phi; then y <- the AL multiplier.
    y0: the multipliers of the previous SQP iteration's QP (the loop passes them unless that QP hit its cap).
    Stops on the KKT residual of the QP: stationarity <= eps scale_g, violation <= eps, complementarity <= eps scale_g.
    expanded: the backtracking compares phi along p as opf_qp_solve forms it — the quadratic expanded in t around d, c(t) = c + t A p —
    and not phi recomputed at d + t p.  The two are the same function, but the recomputed one carries the rounding of the whole
    objective, ~1e-16 |phi|, which near the optimum exceeds the decrease the Armijo test asks for: the search then halves t thirty
    times and the QP crawls (case33, a daytime row at a = 0.9 x random: 444 Newton steps and the cap, where the routine and the
    expanded form take 26 and 25).  The kernel tests (tests/test_opf_kernels_gpu.py) compare with expanded=True.  The SQP loop below
    keeps the recomputed form: the iterates stored in tests/golden/opf_golden.npz were made with it."""
    ns = g.shape[0]
    A = np.vstack([np.eye(ns), S])
    lo, hi = np.concatenate([lo_box, lo_row]), np.concatenate([hi_box, hi_row])
    rown = np.maximum((A * A).sum(1), 1e-300)
    hmax = max(float(np.abs(np.diag(H)).max()), 1e-300)
    rho_r = QP_RHO * hmax / rown                     # per row: the penalty curvature of every row is QP_RHO x the largest of H
    gs = max(float(np.abs(g).max()), 1e-300)
    d = np.zeros(ns)
    y = np.zeros(A.shape[0]) if y0 is None else np.array(y0, dtype=np.float64)      # warm start: the multipliers of the last QP
    newton, vi_last, stall = 0, np.inf, 0

    def mult(c, y):
        t = y + rho_r * (c - hi)
        u = y + rho_r * (c - lo)
        return np.where(t > 0, t, np.where(u < 0, u, 0.0))

    def phi(d, y):
        c = A @ d
        z = mult(c, y)
        return float(g @ d + 0.5 * d @ (H @ d) + np.sum((z * z - y * y) / (2.0 * rho_r)))

    for outer in range(QP_MAX_OUTER):
        for _ in range(QP_MAX_NEWTON):
            c = A @ d
            z = mult(c, y)
            grad = g + H @ d + A.T @ z
            if np.abs(grad).max() <= QP_EPS * gs:
                break
            P = z != 0
            K = H + (A[P].T * rho_r[P]) @ A[P]
            K = K + np.eye(ns) * (QP_RIDGE * max(float(np.diag(K).max()), 1e-300))
            p = np.linalg.solve(K, -grad)
            newton += 1
            slope, t = float(grad @ p), 1.0
            if expanded:
                Ap, Hd, Hp = A @ p, H @ d, H @ p
                gd, gp, dHd, dHp, pHp = float(g @ d), float(g @ p), float(d @ Hd), float(p @ Hd), float(p @ Hp)

                def along(tt):
                    zt = mult(c + tt * Ap, y)
                    return gd + tt * gp + 0.5 * (dHd + 2.0 * tt * dHp + tt * tt * pHp) + float(np.sum((zt * zt - y * y) / (2.0 * rho_r)))
            else:
                along = lambda tt: phi(d + tt * p, y)
            f0 = along(0.0)
            for _ in range(30):
                if along(t) <= f0 + 1e-4 * t * slope:
                    break
                t *= 0.5
            d = d + t * p
        c = A @ d
        y = mult(c, y)
        st, vi, co = qp_kkt(g, H, A, lo, hi, d, y)
        if st <= QP_EPS * gs and vi <= QP_EPS and co <= QP_EPS * gs:
            return QPResult(d, y, max(st / gs, vi, co / gs), newton, False)
        if vi > QP_EPS and vi > QP_SHRINK * vi_last:
            # the violation stagnates: rows that share (nearly) one normal keep multipliers that only decay by rho x slack per outer
            # iteration — drop the multiplier of every row that is strictly inside its bound (the AL rebuilds it if it is needed)
            y = np.where(((y > 0) & (c < hi)) | ((y < 0) & (c > lo)), 0.0, y)
        stall = stall + 1 if vi > QP_STALL * vi_last else 0
        if stall >= QP_MAX_STALL:                    # the rows cannot be met inside the box: the least-violation compromise, reported as capped
            break
        vi_last = vi
    return QPResult(d, y, max(st / gs, vi, co / gs), newton, True)


def qp_objective(g, H, d):
    return float(g @ d + 0.5 * d @ (H @ d))


# ---- the SQP loop (csrc/opf.hip: solve -> k_opf_linearise -> k_opf_qp -> k_opf_update) --------------------------------------------------
class OPFResult(NamedTuple):
    actions: np.ndarray
    loss_mw: float
    violation: float
    iterations: int      # power flows solved
    status: int          # 0 converged and feasible, 1 max_iter / QP cap, 2 a power flow failed, 3 not solved
    vm_pu: np.ndarray
    steps: list          # |d|inf of every QP
    trace: list          # the a of every solved power flow


def violation_of(vm, net, v_lower, v_upper):
    v = np.delete(np.asarray(vm), net.ext_grid_bus)
    return float(max(np.max(v - v_upper), np.max(v_lower - v), 0.0))


def opf_ref(net, load_p, load_q, sgen_p, s_max, cfg=None, v_lower=0.95, v_upper=1.05, runpp=runpp_restated, solve=True, qp_log=None, decisions=None):
    c = resolve(cfg, v_lower, v_upper)
    ns = net.n_sgen
    ybus = make_ybus(net)[0]
    nan_vm = np.full(net.n_bus, np.nan)
    if not solve:
        return OPFResult(np.zeros(ns), np.nan, np.nan, 0, 3, nan_vm, [], [])
    p = np.asarray(sgen_p, dtype=np.float64)
    lim = limits(p, s_max)
    nonslack = np.setdiff1d(np.arange(net.n_bus), [net.ext_grid_bus])
    a, a_sol, d, t, nback, y_warm = np.zeros(ns), np.zeros(ns), np.zeros(ns), 1.0, 0, None
    out = (np.nan, np.nan, nan_vm)
    steps, trace = [], []

    def note(**k):                                   # what the loop saw before a decision and the (t, failures in a row) it left
        if decisions is not None:
            decisions.append(k)
    for i in range(1, c["max_iter"] + 1):
        res = runpp(net, load_p, load_q, p, lim * a)
        if not res.converged:
            nback += 1
            if i == 1 or nback > c["max_backtrack"] or i == c["max_iter"]:
                note(iter=i, solved=0, dn=0.0, viol=0.0, prev_viol=out[1], capped=0, t_after=t, nback_after=nback)
                return OPFResult(a_sol, *out[:2], i, 2, out[2], steps, trace)
            t *= 0.5
            note(iter=i, solved=0, dn=0.0, viol=0.0, prev_viol=out[1], capped=0, t_after=t, nback_after=nback)
            a = np.clip(a_sol + t * d, -1.0, 1.0)
            continue
        V = res.V
        vm = np.abs(V)
        viol = violation_of(vm, net, c["v_lower"], c["v_upper"])
        prev = out[1]
        gain = prev - viol                           # NaN at the first solved point
        out = (loss_pu(ybus, V) * net.sn_mva, viol, vm.copy())
        a_sol, t, nback = a.copy(), 1.0, 0
        trace.append(a_sol.copy())
        L = linearise(net, V, lim)
        S = L.S[nonslack]
        q = qp_solve(L.g, L.H, S, -1.0 - a, 1.0 - a, c["v_lower"] - vm[nonslack], c["v_upper"] - vm[nonslack], y_warm)
        y_warm = None if q.capped else q.y
        if qp_log is not None:
            qp_log.append(dict(g=L.g, H=L.H, S=S, v=vm[nonslack], a=a.copy(), d=q.d, y=q.y))
        d = q.d
        dn = float(np.abs(d).max())
        steps.append(dn)
        note(iter=i, solved=1, dn=dn, viol=viol, prev_viol=prev, capped=int(q.capped), t_after=1.0, nback_after=0)
        if not q.capped and dn < c["step_tol"] and viol <= c["v_tol"]:
            return OPFResult(a_sol, *out[:2], i, 0, out[2], steps, trace)
        # a capped QP: the linearised bounds cannot be met inside the box.  With a step below step_tol, or a violation that came down by
        # less than v_tol since the last solved point, this is a least-violation point: stop there, as at max_iter
        if i == c["max_iter"] or (q.capped and (dn < c["step_tol"] or gain < c["v_tol"])):
            return OPFResult(a_sol, *out[:2], i, 1, out[2], steps, trace)
        a = np.clip(a_sol + d, -1.0, 1.0)
    raise AssertionError("unreachable")


# ---- KKT residual of the nonlinear problem -------------------------------------------------------------------------------------------
def kkt_nonlinear(net, load_p, load_q, sgen_p, s_max, a, v_lower=0.95, v_upper=1.05, near=1e-6):
    """(stationarity relative to |grad f|inf, complementarity, violation) at a: the multipliers of the near-active voltage rows and box
    bounds (within `near` of their bound) by non-negative least squares on grad f + sum mu_r n_r = 0, n_r the outward normals."""
    from scipy.optimize import nnls
    p = np.asarray(sgen_p, dtype=np.float64)
    lim = limits(p, s_max)
    res = runpp_restated(net, load_p, load_q, p, lim * a)
    assert res.converged
    L = linearise(net, res.V, lim)
    vm = np.abs(res.V)
    nonslack = np.setdiff1d(np.arange(net.n_bus), [net.ext_grid_bus])
    normals, slack = [], []
    for k in nonslack:
        if v_upper - vm[k] <= near:
            normals.append(L.S[k]); slack.append(v_upper - vm[k])
        if vm[k] - v_lower <= near:
            normals.append(-L.S[k]); slack.append(vm[k] - v_lower)
    for j in range(net.n_sgen):
        e = np.zeros(net.n_sgen); e[j] = 1.0
        if 1.0 - a[j] <= near:
            normals.append(e); slack.append(1.0 - a[j])
        if a[j] + 1.0 <= near:
            normals.append(-e); slack.append(a[j] + 1.0)
    res0 = runpp_restated(net, load_p, load_q, p, lim * 0.0)
    scale = max(float(np.abs(linearise(net, res0.V, lim).g).max()), 1e-300)       # |grad f|inf at a = 0
    if normals:
        N = np.array(normals).T
        cn = np.linalg.norm(N, axis=0)
        mu, _ = nnls(N / cn, -L.g / scale, maxiter=50 * N.shape[1] + 200)
        r = L.g / scale + (N / cn) @ mu
        comp = float(np.max(mu * np.abs(np.array(slack))))
    else:
        r, comp = L.g / scale, 0.0
    return float(np.abs(r).max()), comp, violation_of(vm, net, v_lower, v_upper)
