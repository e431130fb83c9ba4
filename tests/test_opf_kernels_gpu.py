"""GPU (-m gpu) tests of the OPF kernels one launch at a time (csrc/opf.hip through VoltageControlBatch.opf_probe -> mapdn_opf_probe): what a
converging SQP loop hides.  k_opf_linearise against the extended-precision form of its definition at the probe's own V
(tests/opf_kernel_cases.linearise_ext) on nets at the edges of its column striping, with a phase shifter, a shunt, sgen scalings, a
four-children junction and an sgen on the slack bus; k_opf_qp's wave teams against the KKT conditions of their own inputs, the
equality-constrained solve on their active set and the numpy restatement, in waves that mix short, long, capped and skipped QPs; every
env's bits against the same env alone, in another lane, workgroup and wave; and k_opf_update's retry and failure branches on states found
by a search on the oracle (tests/golden/make_opf_backtrack.py)."""
import os
import re
import types

import numpy as np
import pytest
import torch

from mapdn_amd.env import VoltageControlBatch
from mapdn_amd.netspec import Profiles
from oracle.pp_restated import make_ybus, runpp_restated
from tests import opf_kernel_cases as K
from tests import opf_ref as R
from tests.baseline_contract import env_state, same, snapshot
from tests.test_opf_gpu import check_point_against_the_oracle, place

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0, voltage_barrier_type="bowl", seed=0)
DEV = "cuda:0"
EPS = np.finfo(np.float64).eps
with open(os.path.join(ROOT, "mapdn_amd", "csrc", "opf.hpp")) as _f:
    QP_EPS = float(re.search(r"#define\s+OPF_QP_EPS\s+(\S+)", _f.read()).group(1))      # the routine's own stop threshold

# ---- the bars of the linearisation: E64 and bar() in tests/opf_kernel_cases.py ----------------------------------------
E64, bar = K.E64, K.bar
# the worst the kernel showed on an MI355X, per case and quantity (for the record: the bars above do not come from it)
GPU_MEASURED = dict(
    tiny=dict(S=9.2e-15, g=5.2e-14, H=1.7e-14, loss=3.0e-13, violation=8.5e-16),
    small15=dict(S=9.7e-15, g=1.4e-13, H=7.5e-15, loss=6.8e-13, violation=6.5e-16),
    small16=dict(S=1.7e-14, g=2.8e-13, H=2.6e-14, loss=2.5e-12, violation=4.8e-15),
    small17=dict(S=2.3e-14, g=7.9e-13, H=3.1e-14, loss=1.5e-12, violation=1.8e-15),
    wide33=dict(S=3.0e-14, g=2.0e-12, H=8.6e-14, loss=4.4e-12, violation=2.2e-15),
    wide48=dict(S=2.5e-14, g=2.8e-13, H=2.3e-14, loss=6.3e-13, violation=1.1e-15),
    wide49=dict(S=3.1e-14, g=5.5e-13, H=7.9e-14, loss=5.7e-12, violation=2.1e-15),
    wide64=dict(S=1.2e-13, g=4.3e-12, H=9.2e-14, loss=5.3e-12, violation=3.0e-15),
    case33=dict(S=2.4e-14, g=6.8e-13, H=3.0e-14, loss=3.0e-12, violation=1.1e-15),
    case141=dict(S=2.1e-13, g=1.5e-12, H=1.7e-13, loss=1.1e-11, violation=2.3e-15),
    special=dict(S=5.9e-14, g=3.6e-12, H=5.9e-14, loss=1.3e-11, violation=2.2e-15),
)
# The kernel's worst multiple of E64: S 2.0 (small15), g 5.3 (tiny), H 6.2 (tiny), loss 11.2 (special), violation 1.1.  The host build of
# opf.hpp with the kernel's sums (HOST_ERR in tests/test_opf_cpu.py, at the oracle's V) is at most 6.0 x E64, on the special net's
# loss 3.6 x: every bar stands at 16 x E64, none had to be reset from the host figure.
CASES = list(K.BATCHES)
# central differences of the oracle's loss, step FD_H: tests/test_opf_cpu.py::test_gradient_against_central_differences finds truncation
# (~0.1 h^2) and the round-off of a power flow converged to 1e-8 MVA (~2e-10 / h) both below 2.2e-7 of |g|inf at h = 1e-3 and sets 1e-6;
# tests/test_opf_cpu.py::test_special_net_carries_what_it_claims holds the restated g of the special net to the same bound
FD_H, FD_BOUND = 1e-3, 1e-6
# the backtracking states: max |a - a of the restated loop| measured on an MI355X over the four "retry" runs (6.7e-10, 4.9e-12, 8.4e-15,
# 1.7e-13; the "mb1" runs return a = 0 on both sides), rounded up; the bound is ten times that, as A_BOUND of tests/test_opf_gpu.py
BT_A_GAP_MEASURED = 7e-10
BT_A_BOUND = 10.0 * BT_A_GAP_MEASURED


# ---- envs and probes ------------------------------------------------------------------------------------------------------------------
def make_env(net, prof, B, args=None, **kw):
    a = dict(ARGS)
    a.update(args or {})
    return VoltageControlBatch(net, prof, a, n_envs=B, device=DEV, obs_dtype=torch.float64, **kw)


def probe(env, a, cfg=None):
    out = env.opf_probe(torch.as_tensor(a, device=DEV), cfg)
    torch.cuda.synchronize()
    return types.SimpleNamespace(**{k: v.cpu().numpy() for k, v in out.items()})


def probe_case(case, cfg=None, order=None, only=None, calls=1):
    """the probe of a case's batch (its envs in `order`, or the single env `only` with env_id_offset), `calls` times"""
    net, prof, rows, a, _ = K.state(case)
    idx = np.arange(len(rows)) if order is None else np.asarray(order)
    if only is not None:
        idx = np.array([only])
    env = make_env(net, prof, len(idx), env_id_offset=0 if only is None else int(only))
    try:
        place(env, prof, rows[idx])
        outs = [probe(env, a[idx], cfg) for _ in range(calls)]
    finally:
        env.close()
    return outs if calls > 1 else outs[0]


_RUNS = {}


def batch(case, band=None):
    """the probe of the case's batch, twice, computed once and shared"""
    if (case, band) not in _RUNS:
        cfg = None if band is None else dict(v_lower=band[0], v_upper=band[1])
        _RUNS[case, band] = probe_case(case, cfg, calls=2)
    return _RUNS[case, band]


FIELDS = ("v", "vm", "S", "g", "H", "loss_mw", "violation", "d", "y", "linearised", "qp_capped")


def same_bits(x, y, ex=slice(None), ey=slice(None), what=""):
    for k in FIELDS:
        assert np.array_equal(getattr(x, k)[ex], getattr(y, k)[ey], equal_nan=True), (what, k)


def by_bus(net, out, e):
    """V [n_bus] and S [n_bus, ns] of env e by bus (the slack: its set-point, a zero row)"""
    V = np.full(net.n_bus, net.ext_grid_vm_pu, np.complex128)
    S = np.zeros((net.n_bus, net.n_sgen))
    V[out.bus_of_node], S[out.bus_of_node] = out.v[e], out.S[e]
    return V, S


# ---- the probe's own contract -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("after_solve", [False, True])
def test_probe_leaves_the_env_untouched(after_solve):
    """opf_actions' contract (tests/test_opf_gpu.py::test_state_untouched_and_step_agrees) for the probe: noisy resets, two random-action
    steps, optionally a mapdn_solve_only that leaves Sbus stale; the probe at random set-points changes no state, no result and not
    the next two steps, and what it returns is what it returns on the twin that was not probed before"""
    B = 24
    net, prof = K.make("special")
    A, T = (make_env(net, prof, B) for _ in range(2))
    try:
        A.reset(); T.reset()
        rng = np.random.default_rng(3)
        for _ in range(2):
            act = torch.as_tensor(rng.uniform(-0.8, 0.8, (B, A.n_sgen)), device=DEV)
            A.step(act); T.step(act)
        if after_solve:
            lp, lq, pv, _ = env_state(A)
            for env in (A, T):
                env.solve(lp * 1.3, lq, pv, np.zeros_like(pv))
        before = snapshot(A)
        sp = rng.uniform(-1.0, 1.0, (B, A.n_sgen))
        out = probe(A, sp)
        assert out.linearised.all()
        same(before, snapshot(A))
        same(before, snapshot(T))
        for _ in range(2):
            act = torch.as_tensor(rng.uniform(-0.8, 0.8, (B, A.n_sgen)), device=DEV)
            r1, t1, i1 = [x.clone() for x in A.step(act)]
            r2, t2, i2 = [x.clone() for x in T.step(act)]
            assert torch.equal(r1, r2) and torch.equal(t1, t2) and torch.equal(i1, i2) and torch.equal(A.get_obs(), T.get_obs())
        if not after_solve:                          # (after the two steps both stand at the same state again)
            same_bits(probe(A, sp), probe(T, sp), what="probed before or not")
    finally:
        A.close(); T.close()
    if after_solve:                                  # the probe solved the env's own loads, not those of solve_only: a fresh twin agrees
        F = make_env(net, prof, B)
        try:
            F.reset()
            rng = np.random.default_rng(3)
            for _ in range(2):
                F.step(torch.as_tensor(rng.uniform(-0.8, 0.8, (B, F.n_sgen)), device=DEV))
            same_bits(out, probe(F, sp), what="after solve_only")
        finally:
            F.close()


# ---- the linearisation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_linearisation_against_the_extended_reference(case):
    """S, g, H, the loss and the violation of k_opf_linearise at the probe's own V against the extended-precision reference at that V.
    Measured on an MI355X: GPU_MEASURED."""
    net, prof, rows, a, smax = K.state(case)
    out, _ = batch(case)
    B = len(rows)
    assert out.linearised.all() and out.v.shape == (B, net.n_bus - 1)
    assert sorted(out.bus_of_node.tolist()) == sorted(set(range(net.n_bus)) - {net.ext_grid_bus})
    for k in ("S", "g", "H", "loss_mw", "violation", "d", "y"):
        assert np.isfinite(getattr(out, k)).all(), k
    assert np.array_equal(out.H, out.H.transpose(0, 2, 1))                  # H == H' bitwise
    assert np.array_equal(out.vm, np.abs(out.v)) or np.abs(out.vm - np.abs(out.v)).max() <= 2 * EPS * np.abs(out.v).max()
    per_env = []
    for e in K.ref_envs(B):
        V, S = by_bus(net, out, e)
        lim = R.limits(prof.pv[rows[e]], smax)
        got = dict(S=S, g=out.g[e], H=out.H[e], loss=K.LD(out.loss_mw[e]) / K.LD(net.sn_mva), violation=out.violation[e])
        per_env.append(K.errors(net, V, lim, got))
    worst = K.worst(per_env)
    print(case, "B", B, "worst", {q: f"{v:.2e}" for q, v in worst.items()}, "bar", {q: f"{bar(case, q):.2e}" for q in K.QUANTITIES})
    for q in K.QUANTITIES:
        assert worst[q] <= bar(case, q), (case, q, worst[q], bar(case, q))


def test_slack_sgen_has_a_zero_column():
    net, _, _, _, _ = K.state("special")
    out, _ = batch("special")
    js = [j for j, b in enumerate(net.sgen_bus) if b == net.ext_grid_bus]
    assert js == [net.n_sgen - 1]
    j = js[0]
    assert (out.S[:, :, j] == 0).all() and (out.g[:, j] == 0).all() and (out.H[:, j, :] == 0).all() and (out.H[:, :, j] == 0).all()
    assert (out.d[:, j] == 0).all()                                         # nothing moves a set-point that moves nothing
    assert (np.abs(out.S[:, :, :j]).max(axis=(1, 2)) > 0).all()


def test_gradient_with_a_phase_shifter_against_central_differences():
    """M = (Ybus + Ybus^H) / 2 keeps g exact when a phase shifter makes Ybus unsymmetric.  Here without M: the
    kernel's g against central differences of the oracle's loss V^H Ybus V in a, on the special net (shift 3 degrees, iron losses)."""
    net, prof, rows, a, smax = K.state("special")
    out, _ = batch("special")
    ybus = make_ybus(net)[0]
    Y = ybus.toarray()
    assert np.abs(Y - Y.T).max() > 1e-3 * np.abs(Y).max()
    eye, worst = np.eye(net.n_sgen), 0.0
    for e in (0, 2, 16):                                                    # a = 0, random with pinned sgens, all pinned
        t = rows[e]
        lim = R.limits(prof.pv[t], smax)
        f = lambda x: R.loss_pu(ybus, runpp_restated(net, prof.load_p[t], prof.load_q[t], prof.pv[t], lim * x).V)
        fd = np.array([(f(a[e] + FD_H * eye[j]) - f(a[e] - FD_H * eye[j])) / (2.0 * FD_H) for j in range(net.n_sgen)])
        worst = max(worst, float(np.abs(fd - out.g[e]).max() / np.abs(fd).max()))
    print("special: g against central differences", worst)
    assert worst <= FD_BOUND, worst


@pytest.mark.parametrize("case", ["tiny", "small17", "wide49", "wide64", "case141", "special"])
def test_every_env_has_the_same_bits_wherever_it_runs(case):
    """across two calls; alone at B = 1 with its env_id_offset; after a permutation that moves every env to another lane, and in the
    larger batches to another workgroup of k_opf_linearise and another wave of k_opf_qp"""
    first, second = batch(case)
    same_bits(first, second, what="second call")
    B = K.BATCHES[case]
    for e in sorted({0, B // 2, B - 1}):
        same_bits(first, probe_case(case, only=e), slice(e, e + 1), slice(0, 1), f"env {e} alone")
    order = np.array([(7 * i + 3) % B for i in range(B)])                   # 7 and B are coprime
    assert sorted(order.tolist()) == list(range(B)) and (order != np.arange(B)).sum() >= B - 3
    same_bits(first, probe_case(case, order=order), order, slice(None), "permuted")


# ---- the QP ---------------------------------------------------------------------------------------------------------------------------
# (case, band): the bands keep the share of capped QPs at or below one env in eight (opf_ref.qp_solve on the oracle's linearisation, on
# the CPU, with the host build of the routine beside it: 0/5, 0/17, 0/5, 0/5, 0/3, 0/33, 0/33, 2/17, 2/17), with voltage rows active in
# most envs (wide64: in a third)
QP_CASES = [("tiny", (0.93, 1.09)), ("small16", None), ("small17", None), ("wide33", None), ("wide48", None), ("wide64", (0.92, 1.10)),
            ("case33", None), ("case141", None), ("special", None)]


def qp_inputs(out, e, a, band):
    ns = a.shape[0]
    g, H, S, v = out.g[e], out.H[e], out.S[e], out.vm[e]
    A = np.vstack([np.eye(ns), S])
    lo, hi = np.concatenate([-1.0 - a, band[0] - v]), np.concatenate([1.0 - a, band[1] - v])
    return g, H, S, A, lo, hi


def bus_sums(net, lim):
    """one row per bus with sgens: sum over its sgens of w_j d_j, the reactive power the step moves at that bus — what H sees of sgens
    that share a bus"""
    w = lim * net.sgen_scaling / net.sn_mva
    buses = sorted(set(int(b) for b in net.sgen_bus) - {int(net.ext_grid_bus)})      # (an sgen on the slack bus moves nothing: its d is free)
    G = np.zeros((len(buses), net.n_sgen))
    for j, b in enumerate(net.sgen_bus):
        if int(b) in buses:
            G[buses.index(int(b)), j] = w[j]
    return G


def check_qp(net, out, e, a, band, lim):
    """the kernel's (d, y) of env e on the kernel's own inputs.  Returns (capped, number of active box rows, of active voltage rows)"""
    ns = a.shape[0]
    g, H, S, A, lo, hi = qp_inputs(out, e, a, band)
    d, y, capped = out.d[e], out.y[e], bool(out.qp_capped[e])
    q = R.qp_solve(g, H, S, lo[:ns], hi[:ns], lo[ns:], hi[ns:], expanded=True)
    assert q.capped == capped, (e, q.capped, capped)
    if capped:
        return True, 0, 0
    gs = max(float(np.abs(g).max()), 1e-300)
    st, vi, co = R.qp_kkt(g, H, A, lo, hi, d, y)
    assert st <= 2.0 * QP_EPS * gs and vi <= 2.0 * QP_EPS and co <= 2.0 * QP_EPS * gs, (e, st / gs, vi, co / gs)
    # the active set as the stop test can see it: a multiplier whose term in the stationarity, |y_r| |a_r|inf, is below the routine's own
    # tolerance eps |g|inf is a zero to it (a row that sits on its bound without pushing: 2.7e-15 in one, 0 in the other)
    seen = lambda yy: np.where(np.abs(yy) * np.abs(A).max(axis=1) > QP_EPS * gs, np.sign(yy), 0.0)
    assert np.array_equal(seen(q.y), seen(y)), (e, np.flatnonzero(seen(q.y) != seen(y)))
    act = y != 0
    m = int(act.sum())
    Kkt = np.block([[H, A[act].T], [A[act], np.zeros((m, m))]])
    rhs = np.concatenate([-g, np.where(y > 0, hi, lo)[act]])
    # what the stop test allows: the stationarity within eps |g|inf; an active row within eps beyond its bound and, by the
    # complementarity, within eps |g|inf / |y_r| inside it
    allowed = np.concatenate([np.full(ns, QP_EPS * gs), np.maximum(QP_EPS, QP_EPS * gs / np.abs(y[act]))])
    sv = np.linalg.svd(Kkt, compute_uv=False)
    if sv[-1] > 1e-10 * sv[0]:
        Kinv, G = np.linalg.inv(Kkt), np.eye(ns)
    else:                              # sgens that share a bus, none of them at its box bound: only the sum of the pair is determined
        Kinv, G = np.linalg.pinv(Kkt, rcond=1e-10), bus_sums(net, lim)
        null = np.linalg.svd(Kkt)[2][sv <= 1e-10 * sv[0]]
        assert np.abs(G @ null[:, :ns].T).max() <= 1e-8 * np.abs(G).max(), e
        assert np.abs(Kkt @ (Kinv @ rhs) - rhs).max() <= 1e-8 * max(np.abs(rhs).max(), 1e-300), e
    ref = (Kinv @ rhs)[:ns]
    bound = 2.0 * np.abs(G @ Kinv[:ns]) @ allowed
    err = np.abs(G @ (d - ref))
    assert (err <= bound + 64.0 * EPS * np.abs(G) @ np.abs(ref)).all(), (e, float((err / bound).max()))
    return False, int(act[:ns].sum()), int(act[ns:].sum())


@pytest.mark.parametrize("case,band", QP_CASES)
def test_qp_against_its_kkt_conditions_and_the_restatement(case, band):
    net, prof, rows, a, smax = K.state(case)
    out, _ = batch(case, band)
    B = len(rows)
    assert out.linearised.all()
    envs = range(B) if net.n_sgen <= 32 else K.ref_envs(B)                  # (the restatement in numpy is slow on the wide nets)
    res = [check_qp(net, out, e, a[e], band or K.V_BAND, R.limits(prof.pv[rows[e]], smax)) for e in envs]
    capped = sum(r[0] for r in res)
    print(case, "B", B, "checked", len(res), "capped", capped, "active box rows", [r[1] for r in res], "voltage rows", [r[2] for r in res])
    assert 8 * int(out.qp_capped.sum()) <= B and 8 * capped <= len(res), (capped, out.qp_capped.tolist())
    assert any(r[2] > 0 for r in res) and (case == "tiny" or any(r[1] > 0 for r in res))


MIXED_ROWS = [100, 260, 700, 740, 280]              # case33 (tests/golden/opf_golden.npz): row 100 has no PV, the others are daytime rows


def mixed_wave(cfg, alone):
    net, prof = K.make("case33")
    rng = np.random.default_rng(5)
    a = np.zeros((5, net.n_sgen))
    a[2] = -1.0
    a[3] = rng.uniform(-0.9, 0.9, net.n_sgen)
    rows = np.array(MIXED_ROWS) % prof.n_rows
    outs = []
    for idx in [np.arange(5)] + ([np.array([e]) for e in range(5)] if alone else []):
        env = make_env(net, prof, len(idx), env_id_offset=int(idx[0]))
        try:
            place(env, prof, rows[idx])
            outs.append(probe(env, a[idx], cfg))
        finally:
            env.close()
    return net, prof, rows, a, outs


def test_a_wave_of_short_and_long_qps():
    """one wave of k_opf_qp (envs 0 .. 3) holds an env with no active row, which leaves after its first Newton step and the one that
    polishes it, an env with several active voltage rows and many steps, and an env pinned at a = -1; env 4 sits in a wave that the
    batch does not fill.  Each has the bits of the env alone."""
    net, prof, rows, a, outs = mixed_wave(None, alone=True)
    full = outs[0]
    assert full.linearised.all()
    for e in range(5):
        same_bits(full, outs[1 + e], slice(e, e + 1), slice(0, 1), f"env {e} alone")
    ns = net.n_sgen
    qs = []
    for e in range(5):
        g, H, S, A, lo, hi = qp_inputs(full, e, a[e], K.V_BAND)
        qs.append(R.qp_solve(g, H, S, lo[:ns], hi[:ns], lo[ns:], hi[ns:], expanded=True))
    print("newton steps", [q.newton for q in qs], "capped", full.qp_capped.tolist(), "active", [int((q.y != 0).sum()) for q in qs])
    assert qs[0].newton <= 2 and not (full.y[0] != 0).any() and not full.qp_capped[0]      # (the ridge leaves a second, polishing step)
    assert (full.y[1, ns:] != 0).sum() >= 2 and qs[1].newton >= 8 and not full.qp_capped[1]
    assert (a[2] == -1).all() and (full.d[2] >= -2.0 * QP_EPS).all()         # pinned: every box row has its bound at d = 0
    for e in range(5):
        assert bool(full.qp_capped[e]) == qs[e].capped


CAP_BAND = (0.9, 1.0005)         # the night env's voltages lie inside it; the first daytime env cannot come down to it with all six sgens at -1


def test_a_wave_of_capped_and_one_step_qps():
    """a capped QP next to a one-step QP in one wave: under CAP_BAND env 0 (night, a = 0) has no active row and leaves after its first
    Newton step and the one that polishes it, while env 1 of the same wave runs into the cap with every box row active (on the CPU, at
    the oracle's V: Newton steps 2 / 19 / 23 / 30 / 17, capped 0 1 0 0 0; the same at upper bounds of 1.0002 and 1.001).  Then the
    band of +-0.1 % that no env meets: every QP of the wave caps.  Each env has the bits of the env alone."""
    net, prof, rows, a, outs = mixed_wave(dict(v_lower=CAP_BAND[0], v_upper=CAP_BAND[1]), alone=True)
    full = outs[0]
    ns = net.n_sgen
    qs = []
    for e in range(5):
        g, H, S, A, lo, hi = qp_inputs(full, e, a[e], CAP_BAND)
        qs.append(R.qp_solve(g, H, S, lo[:ns], hi[:ns], lo[ns:], hi[ns:], expanded=True))
    print("newton steps", [q.newton for q in qs], "capped", full.qp_capped.tolist())
    assert full.linearised.all()
    assert full.qp_capped[:4].any() and not full.qp_capped[:4].all()
    assert not full.qp_capped[0] and (full.y[0] == 0).all() and qs[0].newton <= 2
    assert full.qp_capped[1] and qs[1].newton >= 8
    for e in range(5):
        assert bool(full.qp_capped[e]) == qs[e].capped, e
        same_bits(full, outs[1 + e], slice(e, e + 1), slice(0, 1), f"env {e} alone")
    net, prof, rows, a, outs = mixed_wave(dict(v_lower=0.999, v_upper=1.001), alone=True)
    full = outs[0]
    print("+-0.1 %: capped", full.qp_capped.tolist())
    assert full.linearised.all() and full.qp_capped.all()
    for e in range(5):
        same_bits(full, outs[1 + e], slice(e, e + 1), slice(0, 1), f"env {e} alone")
        g, H, S, A, lo, hi = qp_inputs(full, e, a[e], (0.999, 1.001))
        assert R.qp_solve(g, H, S, lo[:ns], hi[:ns], lo[ns:], hi[ns:], expanded=True).capped, e


def test_skipped_envs_are_reported_and_leave_no_trace():
    """episode_limit has stopped every env: the probe reports not linearised, d and y are the zeros the entry documents; after the
    next reset the same handle gives the bits of a fresh one"""
    net, prof, rows, a, _ = K.state("small17")
    B = len(rows)
    env = make_env(net, prof, B, dict(episode_limit=2))
    try:
        env.reset()
        for _ in range(2):
            _, term, _ = env.step(torch.zeros(B, net.n_sgen, dtype=torch.float64, device=DEV))
        assert bool(term.all())
        out = probe(env, a)
        assert not out.linearised.any() and not out.qp_capped.any() and (out.d == 0).all() and (out.y == 0).all()
        place(env, prof, rows)
        again = probe(env, a)
    finally:
        env.close()
    same_bits(again, batch("small17")[0], what="after the skipped call")


# ---- backtracking and status 2 on honest states -----------------------------------------------------------------------------------------
BACKTRACK = np.load(os.path.join(ROOT, "tests", "golden", "opf_backtrack.npz"))


def backtrack_profiles(i):
    """(net, Profiles whose row 1 holds the i-th stored state, an ordinary daytime row)"""
    G = lambda k: BACKTRACK[f"s{i}_{k}"]
    net, prof0 = K.backtrack_net(int(G("net")))
    assert np.array_equal(prof0.pv[0], G("pv"))
    prof = Profiles(pv=prof0.pv.copy(), load_p=prof0.load_p.copy(), load_q=prof0.load_q.copy(), time_delta_min=prof0.time_delta_min)
    prof.pv[1], prof.load_p[1], prof.load_q[1] = G("pv"), G("load_p"), G("load_q")
    assert np.array_equal(prof.s_max(1.2), prof0.s_max(1.2))
    return net, prof, prof0.start_row(0, 12, 0)


def test_an_env_whose_power_flow_fails_is_skipped_between_its_neighbours():
    """one wave of k_opf_qp and one workgroup of k_opf_linearise mix lin == 0 with linearised envs: the stored state 0 at a = -1, where
    the power flow has no solution (on the oracle too, also with the loads moved by +-1e-3), between ordinary envs.  The probe reports
    the two as not linearised with d = y = 0; the neighbours have the bits they have without them."""
    net, prof, t_ord = backtrack_profiles(0)
    rows = np.array([t_ord, 1, t_ord + 7, 1, t_ord + 11])
    a = np.random.default_rng(11).uniform(-0.5, 0.5, (5, net.n_sgen))
    a[[1, 3]] = -1.0
    smax = prof.s_max(1.2)
    for e in (1, 3):
        assert not runpp_restated(net, prof.load_p[1], prof.load_q[1], prof.pv[1], R.limits(prof.pv[1], smax) * a[e]).converged

    def run(idx):
        env = make_env(net, prof, len(idx), dict(reset_action=False))
        try:
            place(env, prof, rows[idx])
            return probe(env, a[idx])
        finally:
            env.close()
    out, ordinary = run(np.arange(5)), run(np.array([0, 2, 4]))
    assert out.linearised.tolist() == [True, False, True, False, True] and ordinary.linearised.all()
    assert (out.d[[1, 3]] == 0).all() and (out.y[[1, 3]] == 0).all() and not out.qp_capped[[1, 3]].any()
    same_bits(out, ordinary, [0, 2, 4], slice(None), "the neighbours of the failed envs")


@pytest.mark.parametrize("run", ["retry", "mb1"])
@pytest.mark.parametrize("i", range(int(BACKTRACK["n"])))
def test_backtracking_states_take_the_logged_path(i, run):
    """a state of the search (tests/golden/make_opf_backtrack.py: loads near voltage collapse, a band far below the voltages) in a batch
    between ordinary envs.  "retry": power flows fail, the step is halved until one solves, status 1 at max_iter = that iteration;
    "mb1": max_backtrack = 1, status 2 at the second failure in a row, with the last solved set-point (a = 0)."""
    G = lambda k: BACKTRACK[f"s{i}_{k}"]
    net, prof, t_ord = backtrack_profiles(i)
    t_state = 1                                                            # a row of its own for the scaled loads
    cfg = dict(v_lower=float(G("band")[0]), v_upper=float(G("band")[1]))
    cfg.update(dict(max_iter=int(G("max_iter"))) if run == "retry" else dict(max_backtrack=1))
    rows = np.array([t_ord, t_state, t_ord + 7, t_state, t_ord + 11])
    args = dict(reset_action=False)

    def solve(idx):
        env = make_env(net, prof, len(idx), args)
        try:
            place(env, prof, rows[idx])
            return tuple(x.cpu().numpy() for x in env.opf_actions(cfg, vm_pu=True))
        finally:
            env.close()
    out = solve(np.arange(5))
    a, loss, viol, it, st, vm = out
    log = G(run + "_decisions")
    print(i, run, "status", st.tolist(), "iterations", it.tolist(), "logged", int(G(run + "_status")), int(G(run + "_iterations")),
          "solved", log[:, 1].astype(int).tolist())
    assert (log[:-1, 1] == 0).any() if run == "retry" else (log[-2:, 1] == 0).all()      # the log holds what the name says
    print("    max |a - a_log|", float(np.abs(a[[1, 3]] - G(run + "_a")).max()))
    for e in (1, 3):
        assert st[e] == int(G(run + "_status")) == (1 if run == "retry" else 2) and it[e] == int(G(run + "_iterations")) == log.shape[0]
        assert np.abs(a[e] - G(run + "_a")).max() <= BT_A_BOUND, (e, np.abs(a[e] - G(run + "_a")).max())
    check_point_against_the_oracle(net, prof, rows[[1, 3]], tuple(x[[1, 3]] for x in out), cfg["v_lower"], cfg["v_upper"])
    ordinary = solve(np.array([0, 2, 4]))                                   # the same envs without the failing ones between them
    for x, y in zip(out, ordinary):
        assert np.array_equal(x[[0, 2, 4]], y, equal_nan=True)
    assert (ordinary[4] <= 1).all()
