"""The reference of action_gradients and what tests/test_action_grad_cpu.py and tests/test_action_grad_gpu.py share:
test infrastructure only, independent of the product code.

reward_gradient(): d reward / d action at a converged V, from the definition.  The reward of oracle/env_restated.py::_calc_reward is
written out term by term, its derivative by (theta, |V|) of the non-slack buses is c, the power flow's Jacobian J is
oracle.pp_restated.jacobian, and  J' lambda = c  is numpy.linalg.solve.  An action a_j moves the scheduled Q of its bus by
w_j = lim_j scaling_j / sn_mva, so  g_j = direct_j + w_j lambda_(Q row of the bus)  (0 for a bus that is the slack).
ext=True carries the same evaluation above float64, as tests/opf_kernel_cases.linearise_ext does: numpy.longdouble assembly, the solve
by a float64 LU refined with longdouble residuals (with exact residuals where those stall above the floor: case141); it is the yardstick
for rounding.

The scenario is that of tests/whatif_cases.py (reset, one random step, then candidates {0, random, UNSOLVABLE, random, ...}) on the
nets of tests/opf_kernel_cases.py, tests/element_edge_nets.py and the shipped case33; on the nets of tests/grad_edge_nets.py (B up to 130,
K up to 4) every env starts at a daytime row of its own."""
import functools

import numpy as np
import scipy.linalg as sla

from oracle.env_restated import VoltageControlOracle
from oracle.pp_restated import build_branches, jacobian, make_ybus
from tests import element_edge_nets as N
from tests import grad_edge_nets as EN
from tests import opf_kernel_cases as OK
from tests import whatif_cases as W

LD, CLD = np.longdouble, np.clongdouble
OPF_NETS = ("tiny", "small17", "special")
NETS = OPF_NETS + ("crowded", "one_sgen", "all_pv", "case33")
BARRIER_TYPES = ("l1", "l2", "courant_beltrami", "bowl", "bump")
LINE_ARGS = (("line_weight", 0.7), ("q_weight", None))


# ---- nets and the scenario ---------------------------------------------------------------------------------------------------------------
def make(name):
    """(NetSpec, Profiles, base env args)"""
    if name in EN.NETS:
        return EN.make(name)
    if name in OPF_NETS:
        return (*OK.make(name), W.CASE_ARGS)
    return W.make(name)


def candidates(name, B, K=W.K_MAX):
    """tests/whatif_cases.candidates, also for the nets that module does not know (the same construction)"""
    if name in EN.NETS:
        return EN.candidates(name, B, K)
    if name not in OPF_NETS:
        return W.candidates(name, B, K)
    ns = make(name)[0].n_sgen
    c = np.random.default_rng(23 + sum(map(ord, name))).uniform(-0.8, 0.8, (W.B_MAX, W.K_MAX, ns))
    c[:, 0] = 0.0
    c[:, 2] = W.UNSOLVABLE
    return np.ascontiguousarray(c[:B, :K])


def first_action(name, B):
    if name in EN.NETS:
        return EN.first_action(name, B)
    if name not in OPF_NETS:
        return W.first_action(name, B)
    ns = make(name)[0].n_sgen
    return np.random.default_rng(11 + sum(map(ord, name))).uniform(-0.8, 0.8, (W.B_MAX, ns))[:B]


@functools.lru_cache(maxsize=None)
def reference(name, envs, K, args=()):
    """tests/whatif_cases.reference on make(name) for the env ids `envs` (a tuple; an int B: 0 .. B - 1): (oracles after reset and one
    random step, prediction of their rows of candidates(name, ., K), those candidates [len(envs), K, ns]); cached, read-only"""
    envs = tuple(range(envs)) if isinstance(envs, int) else tuple(envs)
    net, prof, base = make(name)
    cls = N.oracle_class(name) if name in N.NETS else VoltageControlOracle
    os_ = [cls(net, prof, dict(base, **dict(args)), env_id=e, do_reset=False) for e in envs]
    a0 = first_action(name, max(envs) + 1)
    for e, o in zip(envs, os_):
        if name in N.NETS:
            N.first_draw_reset(o)
        elif name in EN.NETS:
            N.first_draw_reset(o, start=EN.start_of(name, e))
        else:
            o.reset()
        _, term, info = o.step(a0[e])
        assert info["destroy"] == 0.0 and not term, (name, e)
    cand = np.ascontiguousarray(candidates(name, max(envs) + 1, K)[list(envs)])
    return os_, W.predict_all(name, os_, cand), cand


def limits(o):
    """lim_j = sqrt(s_max_j^2 - p_j^2) of an oracle env in its current state"""
    return o._clip_reactive_power(np.ones(o.net.n_sgen), o.sgen_p)


def kink_margins(os_, ref, cand):
    """(the smallest distance of a non-slack solved voltage to 0.95, 1.05 and 1.0; the smallest |q_j| that is not a planted zero — an
    all-zero candidate) over the solved rows of a prediction"""
    net = os_[0].net
    pq = np.setdiff1d(np.arange(net.n_bus), [net.ext_grid_bus])
    dv, dq = np.inf, np.inf
    for e, o in enumerate(os_):
        for k in range(cand.shape[1]):
            if not ref["solved"][e, k]:
                continue
            vm = ref["vm"][e, k][pq]
            dv = min(dv, float(min(np.abs(vm - x).min() for x in (0.95, 1.05, 1.0))))
            if np.any(cand[e, k] != 0.0):
                dq = min(dq, float(np.abs(limits(o) * cand[e, k]).min()))
    return dv, dq


# ---- the reward's terms and their derivatives ------------------------------------------------------------------------------------------
def _sign(x):
    return np.sign(x)                                          # sign(0) = 0


def barrier_derivative(kind, v):
    """d barrier / dv of oracle/env_restated.py's five barriers, in the dtype of v; at a kink the branch the forward form takes"""
    v = np.asarray(v)
    T = v.dtype.type
    if kind == "l1":
        return _sign(v - T(1))
    if kind == "l2":
        return T(4) * (v - T(1))
    if kind == "courant_beltrami":
        return T(2) * np.maximum(T(0), v - T(1.05)) - T(2) * np.maximum(T(0), T(0.95) - v)
    if kind == "bowl":                                         # -0.01 N'(v) = 0.01 N(v) (v - 1) / scale^2
        scale = T(0.1)
        normal = T(1) / np.sqrt(T(2) * np.arccos(T(-1)) * scale ** 2) * np.exp(-(v - T(1)) ** 2 / (T(2) * scale ** 2))
        return np.where(np.abs(v - T(1)) > T(0.05), T(2) * _sign(v - T(1)), T(0.01) * normal * (v - T(1)) / scale ** 2)
    assert kind == "bump"
    out = np.zeros_like(v)
    a = np.abs(v) < 1
    b = (~a) & (v > 1) & (v < 3)
    for m, w in ((a, v), (b, v - T(2))):
        t = T(1) - w[m] ** 4
        with np.errstate(all="ignore"):
            out[m] = -T(4) * w[m] ** 3 * np.exp(-T(1) / t) / (t * t)
    return out


def _exact_residual(A, x, b):
    """b - A x of longdouble arrays without a rounding but the last (rationals over the non-zeros of A; a longdouble is the sum of two
    float64 values)"""
    from fractions import Fraction

    def up(v):
        hi = float(v)
        return Fraction(hi) + Fraction(float(v - LD(hi)))
    xs = [up(v) for v in x]
    acc = [up(v) for v in b]
    for i, j in zip(*np.nonzero(A)):
        acc[i] -= up(A[i, j]) * xs[j]
    out = np.zeros(len(acc), LD)
    for i, v in enumerate(acc):
        hi = float(v)
        out[i] = LD(hi) + LD(float(v - Fraction(hi)))
    return out


def reward_gradient(net, args, V, a, lim, ext=False):
    """g [ns] = d reward / d a at the converged V (complex128 [n_bus]) for the actions a and limits lim; args: the env's
    voltage_barrier_type, voltage_weight, q_weight, line_weight.  ext: module docstring.  Returns g in float64 (ext: longdouble)."""
    R, C = (LD, CLD) if ext else (np.float64, np.complex128)
    nb, ns = net.n_bus, net.n_sgen
    pq = np.setdiff1d(np.arange(nb), [net.ext_grid_bus])
    n = pq.shape[0]
    ybus, yf, yt = make_ybus(net)
    Vx = np.asarray(V).astype(C)
    vm = np.abs(Vx)
    # c = d reward / d (theta, |V|) over pq
    c_th, c_vm = np.zeros(nb, R), np.zeros(nb, R)
    c_vm += -(R(args["voltage_weight"]) / R(nb)) * barrier_derivative(args["voltage_barrier_type"], vm)
    if args["line_weight"] is not None:
        f, t, _, _, _, _, is_line = build_branches(net)
        Yf, Yt = yf.toarray().astype(C), yt.toarray().astype(C)
        If, It = Yf @ Vx, Yt @ Vx
        for D, tgt in ((np.diag(C(1j) * Vx), c_th), (np.diag(Vx / vm), c_vm)):
            dS = D[f] * np.conj(If)[:, None] + Vx[f][:, None] * np.conj(Yf @ D) + D[t] * np.conj(It)[:, None] + Vx[t][:, None] * np.conj(Yt @ D)
            tgt += -(R(args["line_weight"]) / R(net.n_line)) * R(net.sn_mva) * dS.real[is_line].sum(axis=0)
    c = np.concatenate([c_th[pq], c_vm[pq]])
    if ext:
        Y = ybus.toarray().astype(C)
        I = Y @ Vx
        Vn = Vx / vm
        dS_dVm = Vx[:, None] * np.conj(Y * Vn[None, :]) + np.diag(np.conj(I) * Vn)
        dS_dVa = C(1j) * Vx[:, None] * np.conj(np.diag(I) - Y * Vx[None, :])
        sub = lambda A: A[np.ix_(pq, pq)]
        J = np.block([[sub(dS_dVa).real, sub(dS_dVm).real], [sub(dS_dVa).imag, sub(dS_dVm).imag]]).astype(LD)
        JT = J.T
        lu = sla.lu_factor(JT.astype(np.float64))
        lam = np.zeros(2 * n, LD)
        last = np.inf
        scale = np.abs(c).max()
        if scale > 0:
            exact = False
            for _ in range(24):
                res = _exact_residual(JT, lam, c) if exact else c - JT @ lam
                dx = sla.lu_solve(lu, res.astype(np.float64)).astype(LD)
                lam = lam + dx
                step = float(np.abs(dx).max() / np.abs(lam).max())
                if step <= 2.0 ** -62:
                    break
                if step > 0.25 * last:
                    # the correction has stopped shrinking.  Above the floor (case141: cond(J) 2^-64 reaches it) the rounding of the
                    # longdouble residual is what holds it up: go on with residuals formed exactly
                    if exact or step <= OK.REFINE_FLOOR:
                        break
                    exact = True
                last = step
            assert step <= OK.REFINE_FLOOR, step
    else:
        J = jacobian(ybus, Vx, pq, pq).toarray()
        lam = np.linalg.solve(J.T, c)
    where = {int(b): i for i, b in enumerate(pq)}
    limR, aR, sc = np.asarray(lim).astype(R), np.asarray(a).astype(R), np.asarray(net.sgen_scaling).astype(R)
    g = np.zeros(ns, R)
    if args["line_weight"] is None:
        g += -(R(args["q_weight"]) / R(ns)) * _sign(limR * aR * sc) * limR * sc
    w = limR * sc / R(net.sn_mva)
    for j, b in enumerate(np.asarray(net.sgen_bus)):
        if int(b) in where:
            g[j] += w[j] * lam[n + where[int(b)]]
    return g


def env_args(o):
    return dict(voltage_barrier_type=o.args["voltage_barrier_type"], voltage_weight=o.voltage_weight, q_weight=o.q_weight, line_weight=o.line_weight)


def rel_inf(x, ref):
    """max |x - ref| relative to |ref|inf (in longdouble); absolute when ref is all zero"""
    ref = np.asarray(ref, LD)
    s = np.abs(ref).max()
    d = np.abs(np.asarray(x, LD) - ref).max()
    return float(d / s) if s > 0 else float(d)


def central_difference(name, o, a, h):
    """[ns] central differences of the oracle's predicted reward (tests/whatif_cases.predict) with step h"""
    g = np.zeros(a.shape[0])
    for j in range(a.shape[0]):
        ap, am = a.copy(), a.copy()
        ap[j] += h
        am[j] -= h
        rp, rm = W.predict(name, o, ap), W.predict(name, o, am)
        assert rp["solved"] and rm["solved"]
        g[j] = (rp["reward"] - rm["reward"]) / (2 * h)
    return g


# ---- the bars of tests/test_action_grad_gpu.py ---------------------------------------------------------------------
# E64: per case the error of the plain float64 reward_gradient against the extended one, relative to the row's largest entry, at the
# oracle's V of the solved rows of the reference envs (B = 33, K = 7; the barrier / line_weight variants B = 5, K = 4), measured on the
# CPU (e64 below; tests/test_action_grad_cpu.py recomputes them).  The kernel's bar is tests/opf_kernel_cases.py's rule: 16 x E64 — its
# block LU takes no pivoting and sums in another order — and never tighter than 64 ulp.
VARIANT_SHAPE = (5, 4)
E64 = {
    ("tiny", ()): 1.08e-14, ("small17", ()): 2.79e-14, ("special", ()): 7.52e-14, ("crowded", ()): 1.51e-14, ("one_sgen", ()): 6.47e-14,
    ("all_pv", ()): 5.72e-15, ("case33", ()): 4.03e-14,
    ("special", (("voltage_barrier_type", "l1"),)): 7.64e-14, ("special", (("voltage_barrier_type", "l2"),)): 5.77e-14,
    ("special", (("voltage_barrier_type", "courant_beltrami"),)): 7.25e-15, ("special", (("voltage_barrier_type", "bump"),)): 3.04e-14,
    ("special", LINE_ARGS): 1.73e-12,
    ("crowded", (("voltage_barrier_type", "l1"),)): 1.88e-14, ("crowded", (("voltage_barrier_type", "l2"),)): 2.41e-14,
    ("crowded", (("voltage_barrier_type", "courant_beltrami"),)): 1.70e-16, ("crowded", (("voltage_barrier_type", "bump"),)): 7.51e-14,
    ("crowded", LINE_ARGS): 1.17e-12,
    # tests/grad_edge_nets.py (B = 130, K = 4; case141 and the line_weight runs B = 65; the reference envs of EN.ref_envs64;
    # tests/test_action_grad_edges_cpu.py recomputes them)
    ("pair", ()): 4.51e-14, ("chain40", ()): 1.42e-13, ("star12", ()): 1.19e-14, ("feeders3", ()): 1.25e-14, ("comb10", ()): 2.21e-14,
    ("ties", ()): 1.24e-14, ("case141", ()): 3.11e-13, ("ties", LINE_ARGS): 9.26e-14, ("feeders3", LINE_ARGS): 9.11e-14,
}


# the nets of tests/grad_edge_nets.py: B = 130 (case141 and the line_weight runs: 65), K = 4, the reference envs of EN.ref_envs64
EDGE_B, EDGE_B_LINE = dict(case141=65), 65


def shape_of(args, name=None):
    if name in EN.NETS:
        return (EDGE_B.get(name, EN.B_MAX) if not args else EDGE_B_LINE, EN.K_MAX)
    return (W.B_MAX, W.K_MAX) if not args else VARIANT_SHAPE


@functools.lru_cache(maxsize=None)
def e64(name, args=()):
    B, K = shape_of(args, name)
    os_, ref, cand = reference(name, B, K, args)
    worst = 0.0
    for e in EN.ref_envs64(B) if name in EN.NETS else OK.ref_envs(B):
        o = os_[e]
        for k in range(K):
            if ref["solved"][e, k]:
                V = ref["rows"][e][k]["r"].V
                g = [reward_gradient(o.net, env_args(o), V, cand[e, k], limits(o), ext=x) for x in (False, True)]
                worst = max(worst, rel_inf(*g))
    return worst


def bar(name, args=()):
    return max(OK.BAR_FACTOR * E64[(name, tuple(args))], OK.BAR_FLOOR)
