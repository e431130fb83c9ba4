"""CPU restatement of the reference's Volt/VAR droop controller (traditional_control/pf_droop_matpower_all.m:84-162, law :196-231) on the
oracle's power flow: test infrastructure only, independent of the product code (mapdn_droop_actions, csrc/droop.hip).

Per env step, on the env's current state (loads and PV of the next step, noise applied):
  a = 0, v_last = 100;  for i = 1 ... max_iter:  solve with q = lim a (lim = sqrt(s_max^2 - p^2), _clip_reactive_power);  v = |V| at
  every sgen's bus;  stop when ||v - v_last||_2 < v_tol;  else v_last = v, a = (1 - damping) a + damping f(v) min(1, ratio s_max / lim).
The output is the action of the last solved power flow.  Status 0 converged, 1 max_iter reached, 2 a power flow failed (the last
action whose power flow converged; 0 if the first failed), 3 not solved.  The arithmetic is spelled in the kernel's order (the norm
as a running sum in sgen order), so that the two agree to the last bit where the power flows do."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from oracle.pp_restated import runpp_restated

DEFAULTS = dict(va=0.95, vb=1.0, vc=1.0, vd=1.05, damping=0.1, max_iter=100, v_tol=1e-4, reactive_ratio=1.0)


def resolve(cfg=None) -> dict:
    """the script's values for every field that is None / 0 / missing (mapdn_droop_config's rule)"""
    c = dict(DEFAULTS)
    if cfg is not None:
        src = cfg if isinstance(cfg, dict) else {k: getattr(cfg, k, None) for k in DEFAULTS}
        for k, v in src.items():
            if v:
                c[k] = type(DEFAULTS[k])(v)
    return c


def law(v, va, vb, vc, vd):
    """f(v), the branches tested in the script's order (elementwise)"""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rise = (v - vb) / (va - vb)
        fall = -(v - vc) / (vd - vc)
    return np.select([v <= va, v > vd, (vb <= v) & (v <= vc), v < vb], [1.0, -1.0, 0.0, rise], fall)


def target(f, ratio, smax, lim):
    with np.errstate(divide="ignore"):
        return f * np.minimum(1.0, ratio * smax / lim)


def damped(a, t, damping):
    return (1.0 - damping) * a + damping * t


def dv_norm(v, v_last):
    s = 0.0
    for x, y in zip(v.tolist(), v_last.tolist()):
        d = x - y
        s = s + d * d
    return float(np.sqrt(s))


class DroopResult(NamedTuple):
    actions: np.ndarray      # [ns]
    iterations: int
    status: int
    vm_pu: np.ndarray        # [nb] of the last solved power flow (NaN: status 2 / 3)
    dists: list              # ||v - v_last||_2 after every solve that converged


def droop_ref(net, load_p, load_q, sgen_p, s_max, cfg=None, runpp=runpp_restated, solve=True) -> DroopResult:
    """one env; solve=False: the env would not be solved (status 3)"""
    c = resolve(cfg)
    ns = net.n_sgen
    nan_vm = np.full(net.n_bus, np.nan)
    a = np.zeros(ns)
    a_sol = np.zeros(ns)
    if not solve:
        return DroopResult(a_sol, 0, 3, nan_vm, [])
    v_last = np.full(ns, 100.0)
    p = np.asarray(sgen_p, dtype=np.float64)
    lim = np.sqrt(s_max * s_max - p * p)
    sb = np.asarray(net.sgen_bus)
    dists = []
    for i in range(1, c["max_iter"] + 1):
        res = runpp(net, load_p, load_q, p, lim * a)
        if not res.converged:
            return DroopResult(a_sol, i, 2, nan_vm, dists)
        v = np.asarray(res.vm_pu)[sb]
        d = dv_norm(v, v_last)
        dists.append(d)
        if d < c["v_tol"] or i == c["max_iter"]:
            return DroopResult(a.copy(), i, 0 if d < c["v_tol"] else 1, np.asarray(res.vm_pu).copy(), dists)
        v_last = v
        a_sol = a.copy()
        a = damped(a, target(law(v, c["va"], c["vb"], c["vc"], c["vd"]), c["reactive_ratio"], s_max, lim), c["damping"])
    raise AssertionError("unreachable")


def droop_ref_oracle(o, cfg=None, runpp=runpp_restated, solve=True) -> DroopResult:
    """droop_ref on the state of an oracle env (oracle.env_restated.VoltageControlOracle)"""
    return droop_ref(o.net, o.load_p, o.load_q, o.sgen_p, o.s_max, cfg, runpp, solve)
