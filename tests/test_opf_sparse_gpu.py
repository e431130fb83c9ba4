"""GPU (-m gpu): the OPF baseline on handles of the sparse solver (mapdn_opf_config.meshed = 1; k_opf_sens_sparse, k_opf_reduce_sparse;
DESIGN.md section 25) — the linearisation through opf_probe against the extended-precision reference at the probe's own V, at every
sp_lanes that fits and batch sizes that leave the last workgroup partly filled; the QP on those inputs; the bits of every env
wherever it runs; the loop against tests/opf_ref.py; the radial cross-check against the tree solver and the stored optima; waves that
mix ordinary, stopped and failing envs; the baselines' contract.  Every condition on the inputs is asserted of the references alone
(tests/test_opf_sparse_cpu.py) before anything is compared.  The bars are tests/opf_sparse_cases.bar (16 x the float64 reference's own
error, never below 64 ulp); what the kernels showed on an MI355X is tabulated in DESIGN.md section 25 (the worst multiple of that error:
11 on pair2x's g, at most 6 elsewhere)."""
import dataclasses
import functools
import types

import numpy as np
import pytest
import torch

from mapdn_amd.baselines import BaselineTester, NoControl, OPFConfig, OPFControl
from mapdn_amd.env import VoltageControlBatch
from tests import meshed_edge_nets as M
from tests import opf_kernel_cases as K
from tests import opf_ref as R
from tests import opf_sparse_cases as OS
from tests import test_opf_gpu as TO
from tests.baseline_contract import check_state_untouched_and_step_agrees, env_state
from tests.test_opf_gpu import place
from tests.test_opf_kernels_gpu import QP_EPS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MESHED = dict(meshed=1)
V_TOL = 5e-6
PROBE_FIELDS = ("v", "vm", "S", "g", "H", "loss_mw", "violation", "d", "y", "linearised", "qp_capped")
# opf_ref.kkt_nonlinear (the larger of stationarity and complementarity) at the returned actions against the residual of the
# reference's own returned point: ten times that, the margin for a stop at step_tol on the other side of the threshold
KKT_FACTOR = 10.0


def make_env(key, B, L=None, scale=1.0, env_id_offset=0, prof=None, tune=True, **args):
    net, p, base = OS.make(key)
    return VoltageControlBatch(net, OS.scaled(p, scale) if prof is None else prof, dict(base, **args), n_envs=B, device=DEV, obs_dtype=torch.float64,
                               tuning=OS.tuning(key, L) if tune else None, env_id_offset=env_id_offset)


def probe(env, a, cfg=MESHED):
    out = env.opf_probe(torch.as_tensor(a, device=DEV), cfg)
    torch.cuda.synchronize()
    return types.SimpleNamespace(**{k: v.cpu().numpy() for k, v in out.items()})


def opf(env, cfg=MESHED):
    out = tuple(x.cpu().numpy() for x in env.opf_actions(cfg, vm_pu=True))
    torch.cuda.synchronize()
    return out


def probe_run(key, L, B, order=None, only=None, calls=1, scale=1.0, cfg=MESHED):
    """the probe of the key's batch of B envs (in `order`, or the single env `only` with its env_id_offset)"""
    prof = OS.make(key)[1]
    idx = np.arange(B) if order is None else np.asarray(order)
    if only is not None:
        idx = np.array([only])
    rows, a = OS.rows_of(prof, B)[idx], OS.setpoints(key, B)[idx]
    env = make_env(key, len(idx), L, scale, env_id_offset=0 if only is None else int(only))
    try:
        assert env.nr_kernel()["solver"] == 1 and (L is None or env.nr_kernel()["L"] == L)
        place(env, OS.scaled(prof, scale), rows)
        outs = [probe(env, a, cfg) for _ in range(calls)]
    finally:
        env.close()
    return outs if calls > 1 else outs[0]


def same_bits(x, y, ex=slice(None), ey=slice(None), what=""):
    for k in PROBE_FIELDS:
        assert np.array_equal(getattr(x, k)[ex], getattr(y, k)[ey], equal_nan=True), (what, k)


def same_run(x, y, ex=slice(None), ey=slice(None), what=""):
    for i, (p, q) in enumerate(zip(x, y)):
        assert np.array_equal(p[ex], q[ey], equal_nan=True), (what, i)


@functools.lru_cache(maxsize=None)
def _errors(key, e, bus, v_bytes, s_bytes, g_bytes, h_bytes, loss, viol):
    net = OS.make(key)[0]
    n, ns = net.n_bus - 1, net.n_sgen
    _, _, pv, smax = OS.inputs(key, e)
    V = np.full(net.n_bus, net.ext_grid_vm_pu, np.complex128)
    S = np.zeros((net.n_bus, ns))
    V[list(bus)], S[list(bus)] = np.frombuffer(v_bytes, np.complex128), np.frombuffer(s_bytes).reshape(n, ns)
    got = dict(S=S, g=np.frombuffer(g_bytes), H=np.frombuffer(h_bytes).reshape(ns, ns), loss=K.LD(loss) / K.LD(net.sn_mva), violation=viol)
    return K.errors(net, V, R.limits(pv, smax), got)


def linearisation_errors(key, out, B):
    """the worst error per quantity of a probe's reference envs against the extended reference at the probe's own V (the reference is a
    function of the env's profile row and of V; cached per env and bit pattern: an env gives the same bits in every batch)"""
    c = np.ascontiguousarray
    bus = tuple(int(b) for b in out.bus_of_node)
    return K.worst([_errors(key, e, bus, c(out.v[e]).tobytes(), c(out.S[e]).tobytes(), c(out.g[e]).tobytes(), c(out.H[e]).tobytes(),
                            float(out.loss_mw[e]), float(out.violation[e])) for e in K.ref_envs(B)])


def check_kkt_of_the_qp(key, out, a, band=OS.V_BAND):
    """d and y of every env against the KKT thresholds tests/test_opf_kernels_gpu.py applies, recomputed in numpy on the kernel's inputs"""
    ns = a.shape[1]
    for e in range(a.shape[0]):
        g, H, S, v = out.g[e], out.H[e], out.S[e], out.vm[e]
        A = np.vstack([np.eye(ns), S])
        lo, hi = np.concatenate([-1.0 - a[e], band[0] - v]), np.concatenate([1.0 - a[e], band[1] - v])
        if out.qp_capped[e]:
            continue
        gs = max(float(np.abs(g).max()), 1e-300)
        st, vi, co = R.qp_kkt(g, H, A, lo, hi, out.d[e], out.y[e])
        assert st <= 2.0 * QP_EPS * gs and vi <= 2.0 * QP_EPS and co <= 2.0 * QP_EPS * gs, (key, e, st / gs, vi, co / gs)


# ---- 5. probe parity ---------------------------------------------------------------------------------------------------------------------
PARITY = [(key, L) for key in OS.NETS for L in OS.fits(key)]


def test_smallest_first():
    """pair2x, one env, one sp_lanes: one node, one sgen, a lone column"""
    out = probe_run("pair2x", 2, 1)
    assert out.linearised.all() and np.isfinite(out.S).all() and np.isfinite(out.H).all()
    worst = linearisation_errors("pair2x", out, 1)
    print("\n[opf sparse gpu] pair2x B=1 sp_lanes=2:", {q: f"{v:.2e}" for q, v in worst.items()})
    for q in K.QUANTITIES:
        assert worst[q] <= OS.bar("pair2x", q), (q, worst[q])


@pytest.mark.parametrize("key,L", PARITY, ids=[f"{k}-{L}" for k, L in PARITY])
def test_probe_against_the_extended_reference(key, L):
    net = OS.make(key)[0]
    ns = net.n_sgen
    slack_sgens = [j for j, b in enumerate(net.sgen_bus) if b == net.ext_grid_bus]
    assert bool(slack_sgens) == (key == "crowded_meshed")
    total = {q: 0.0 for q in K.QUANTITIES}
    for B in OS.BATCHES:
        out = probe_run(key, L, B)
        a = OS.setpoints(key, B)
        assert out.linearised.all() and out.v.shape == (B, net.n_bus - 1)
        others = [b for b in range(net.n_bus) if b != net.ext_grid_bus]
        assert sorted(out.bus_of_node.tolist()) == others and (key in ("pair2x", "tail2x", "case33") or out.bus_of_node.tolist() == others)
        for k in ("S", "g", "H", "loss_mw", "violation", "d", "y"):
            assert np.isfinite(getattr(out, k)).all(), (key, L, B, k)
        assert np.array_equal(out.H, out.H.transpose(0, 2, 1))              # H == H' bitwise
        for j in slack_sgens:
            assert (out.S[:, :, j] == 0).all() and (out.g[:, j] == 0).all() and (out.H[:, j, :] == 0).all() and (out.H[:, :, j] == 0).all()
        worst = linearisation_errors(key, out, B)
        for q in K.QUANTITIES:
            total[q] = max(total[q], worst[q])
            assert worst[q] <= OS.bar(key, q), (key, L, B, q, worst[q], OS.bar(key, q))
        check_kkt_of_the_qp(key, out, a)
    print(f"\n[opf sparse gpu] {key} sp_lanes={L}: gpu", {q: f"{v:.2e}" for q, v in total.items()}, "bar", {q: f"{OS.bar(key, q):.2e}" for q in K.QUANTITIES})


# ---- 6. bits --------------------------------------------------------------------------------------------------------------------------------
def loop_run(key, L, B, order=None, only=None, calls=1, scale=1.0, cfg=MESHED, tune=True):
    prof = OS.make(key)[1]
    idx = np.arange(B) if order is None else np.asarray(order)
    if only is not None:
        idx = np.array([only])
    env = make_env(key, len(idx), L, scale, env_id_offset=0 if only is None else int(only), tune=tune)
    try:
        place(env, OS.scaled(prof, scale), OS.rows_of(prof, B)[idx])
        outs = [opf(env, cfg) for _ in range(calls)]
    finally:
        env.close()
    return outs if calls > 1 else outs[0]


@pytest.mark.parametrize("key", ["tri3", "k9", "grid6", "crowded_meshed", "k9_hv", "case33_meshed"])
def test_every_env_has_the_same_bits_wherever_it_runs(key):
    """across two calls; alone at B = 1 with its env_id_offset; after a permutation of the batch; across every sp_lanes that fits (the
    program's operations and their order per block do not depend on how they are packed into phases: DESIGN.md section 24)"""
    B = 17
    lanes = OS.fits(key)
    first, second = probe_run(key, lanes[0], B, calls=2)
    same_bits(first, second, what="second call")
    run1, run2 = loop_run(key, lanes[0], B, calls=2)
    same_run(run1, run2, what="second call of opf_actions")
    for e in (0, B - 1):
        same_bits(first, probe_run(key, lanes[0], B, only=e), slice(e, e + 1), slice(0, 1), f"env {e} alone")
        same_run(run1, loop_run(key, lanes[0], B, only=e), slice(e, e + 1), slice(0, 1), f"env {e} alone")
    order = np.array([(7 * i + 3) % B for i in range(B)])
    assert sorted(order.tolist()) == list(range(B))
    same_bits(first, probe_run(key, lanes[0], B, order=order), order, slice(None), "permuted")
    same_run(run1, loop_run(key, lanes[0], B, order=order), order, slice(None), "permuted")
    for L in lanes[1:]:
        same_bits(first, probe_run(key, L, B), what=f"sp_lanes {L} against {lanes[0]}")
        same_run(run1, loop_run(key, L, B), what=f"sp_lanes {L} against {lanes[0]}")


def test_the_switch_changes_nothing_on_the_tree_solver():
    B = 17
    prof = OS.make("case33")[1]
    env = make_env("case33", B, tune=False)
    try:
        assert env.nr_kernel()["solver"] == 0
        place(env, prof, OS.rows_of(prof, B))
        a = OS.setpoints("case33", B)
        same_bits(probe(env, a, None), probe(env, a, MESHED), what="probe")
        same_run(opf(env, None), opf(env, OPFConfig(meshed=1)), what="opf_actions")
    finally:
        env.close()


# ---- 7. the loop ----------------------------------------------------------------------------------------------------------------------------
def check_loop(key, out, B, scale, band=OS.V_BAND, envs=None, ref_env=None):
    """status and power-flow count as the reference's on every env; the violation at the returned point by the oracle; the KKT residual
    of the nonlinear problem at the returned actions against that of the reference's own point"""
    net = OS.make(key)[0]
    a, loss, viol, it, st, vm = out
    worst = (0.0, 0.0)
    for e in (range(B) if envs is None else envs):
        re_ = e if ref_env is None else ref_env
        r = OS.reference_run(key, re_, scale, band)
        assert (st[e], it[e]) == (r.status, r.iterations), (key, e, st[e], it[e], r.status, r.iterations)
        res = OS.oracle_voltage(key, re_, a[e], scale)
        v = R.violation_of(res.vm_pu, net, *band)
        assert abs(vm[e] - res.vm_pu).max() < 1e-9 and abs(viol[e] - v) < 1e-9, (key, e)
        if r.status == 0:
            assert v <= V_TOL, (key, e, v)
        if e < 6 and r.status == 0:                          # (the states repeat with period 6)
            mine, ref = (max(OS.kkt_of(key, re_, x, scale, band)[:2]) for x in (a[e], r.actions))
            print(f"[opf sparse gpu] {key} env {e}: kkt residual gpu {mine:.3e} reference {ref:.3e}")
            assert mine <= KKT_FACTOR * ref, (key, e, mine, ref)
            worst = max(worst, (mine, ref))
    return worst


@pytest.mark.parametrize("key", OS.LOOP_NETS)
def test_loop_against_the_restated_sqp(key):
    B = OS.B_MAX
    out = loop_run(key, None, B, scale=OS.LOOP_SCALE)
    worst = check_loop(key, out, B, OS.LOOP_SCALE)
    print(f"\n[opf sparse gpu] {key} x{OS.LOOP_SCALE}: status {out[4].tolist()} power flows {out[3].tolist()} kkt stationarity gpu {worst[0]:.2e} reference {worst[1]:.2e}")


def test_loop_on_the_meshed_feeder():
    B = 19
    out = loop_run("case33_meshed", None, B)
    worst = check_loop("case33_meshed", out, B, 1.0)
    print(f"\n[opf sparse gpu] case33_meshed: status {out[4].tolist()} power flows {out[3].tolist()} kkt stationarity gpu {worst[0]:.2e} reference {worst[1]:.2e}")


@pytest.mark.parametrize("key", list(OS.ACTIVE_BAND))
def test_loop_with_an_active_voltage_row(key):
    band = OS.ACTIVE_BAND[key]
    B = 6
    assert OS.reference_run(key, OS.ACTIVE_ENV, 1.0, band).status == 0 and OS.active_rows(key, OS.ACTIVE_ENV, band) >= 1
    out = loop_run(key, None, B, cfg=dict(meshed=1, v_lower=band[0], v_upper=band[1]))
    worst = check_loop(key, out, B, 1.0, band)
    vm = np.delete(out[5][OS.ACTIVE_ENV], OS.make(key)[0].ext_grid_bus)
    assert (band[1] - vm <= 1e-6).any()                                     # the row sits on its bound on the GPU as well
    print(f"\n[opf sparse gpu] {key} band {band}: power flows {out[3].tolist()} kkt stationarity gpu {worst[0]:.2e} reference {worst[1]:.2e}")


@pytest.mark.parametrize("key", OS.CAPPED_NETS)
def test_loop_stops_at_the_qp_cap_with_status_1(key):
    band, scale = OS.CAPPED_BAND, OS.CAPPED_SCALE
    r = OS.reference_run(key, OS.CAPPED_ENV, scale, band)
    assert r.status == 1
    B = 5
    prof = OS.scaled(OS.make(key)[1], scale)
    env = make_env(key, B, None, scale)
    try:
        place(env, prof, np.full(B, OS.rows_of(prof, OS.B_MAX)[OS.CAPPED_ENV]))
        out = opf(env, dict(meshed=1, v_lower=band[0], v_upper=band[1]))
    finally:
        env.close()
    a, loss, viol, it, st, vm = out
    print(f"\n[opf sparse gpu] {key} capped: status {st.tolist()} power flows {it.tolist()} (reference {r.status}, {r.iterations})")
    check_loop(key, out, B, scale, band, envs=range(B), ref_env=OS.CAPPED_ENV)


# ---- 8. the radial cross-check --------------------------------------------------------------------------------------------------------------
def test_radial_feeder_on_both_solvers_against_the_stored_optima():
    B = TO.BATCH["case33"]
    rows = [TO.ROWS[e % len(TO.ROWS)] for e in range(B)]
    out = {}
    for which, tuning, cfg in (("tree", None, None), ("sparse", dict(nr_solver="sparse"), MESHED)):
        net, prof = TO.make_case("case33", days=3)
        env = VoltageControlBatch(net, prof, dict(TO.ARGS), n_envs=B, device=DEV, obs_dtype=torch.float64, tuning=tuning)
        try:
            assert env.nr_kernel()["solver"] == (0 if tuning is None else 1)
            place(env, prof, rows)
            out[which] = opf(env, cfg)
        finally:
            env.close()
        a, loss, viol, it, st, vm = out[which]
        worst = 0.0
        for e, t in enumerate(rows):
            assert st[e] == 0, (which, e, st[e])
            gold = float(TO.GOLDEN[f"case33_{t}_loss_mw"])
            worst = max(worst, abs(loss[e] - gold) / gold)
            assert np.abs(a[e] - TO.GOLDEN[f"case33_{t}_ref_a"]).max() <= TO.A_BOUND["case33"], (which, e)
        print(f"\n[opf sparse gpu] case33 {which}: loss gap {worst:.2e} (bound {TO.LOSS_GAP_BOUND['case33']:.1e}) power flows {it.tolist()}")
        assert worst <= TO.LOSS_GAP_BOUND["case33"], (which, worst)
        assert float(viol.max()) <= V_TOL + 1e-8
    assert np.array_equal(out["tree"][4], out["sparse"][4]) and np.array_equal(out["tree"][3], out["sparse"][3])


# ---- 9. mixed wavefronts ----------------------------------------------------------------------------------------------------------------------
FROZEN_ENV, FAILING_ENV, FAIL_GAIN = 7, 12, 3000.0


@pytest.mark.parametrize("key", ["tri3", "grid6"])
def test_mixed_wavefronts(key):
    """between ordinary envs: env 7 frozen by an unsolvable step (status 3), env 12 on a row whose loads no power flow carries (status 2,
    predicted by the oracle).  The ordinary envs keep the bits they have in a batch without the two: the same profiles (so the same
    noise), env 7 stepped like the others and env 12 on an ordinary row.  (An episode_limit ends every env of a batch at the same step:
    that stop is test_stopped_by_the_episode_limit.)"""
    net, prof, _ = OS.make(key)
    B = OS.B_MAX
    plain_rows = OS.rows_of(prof, B)
    rows = plain_rows.copy()
    rows[FAILING_ENV] = prof.intervals_per_day // 2 + 40                    # a row of its own: the next one carries the impossible loads
    lp_, lq_ = prof.load_p.copy(), prof.load_q.copy()
    lp_[rows[FAILING_ENV] + 1] *= FAIL_GAIN
    lq_[rows[FAILING_ENV] + 1] *= FAIL_GAIN
    bad = dataclasses.replace(prof, load_p=lp_, load_q=lq_)
    a1 = np.random.default_rng(7).uniform(-0.5, 0.5, (B, net.n_sgen))
    a_frozen = a1.copy()
    a_frozen[FROZEN_ENV] = M.STEP_UNSOLVABLE
    ordinary = [e for e in range(B) if e not in (FROZEN_ENV, FAILING_ENV)]
    runs = {}
    for L in OS.fits(key):
        for which, rr, act in (("mixed", rows, a_frozen), ("plain", plain_rows, a1)):
            env = make_env(key, B, L, prof=bad)
            try:
                place(env, bad, rr)
                env.step(torch.as_tensor(0.5 * a1, device=DEV))             # (the first step draws the noise of the start row again)
                _, term, _ = env.step(torch.as_tensor(act, device=DEV))     # ... and this one moves every env to its next row
                term = term.cpu().numpy()
                assert term.tolist() == [which == "mixed" and e == FROZEN_ENV for e in range(B)]
                lp, lq, pv, smax = env_state(env)
                runs[which, L] = opf(env)
            finally:
                env.close()
            if which == "mixed":
                assert lp[FAILING_ENV].sum() > 0.5 * FAIL_GAIN * prof.load_p[rows[FAILING_ENV] + 1].sum()
                res = OS.runpp_of(key)(net, lp[FAILING_ENV], lq[FAILING_ENV], pv[FAILING_ENV], np.zeros(net.n_sgen))
                assert not res.converged                                    # status 2, by the oracle
        a, loss, viol, it, st, vm = runs["mixed", L]
        assert st[FROZEN_ENV] == 3 and (a[FROZEN_ENV] == 0).all() and it[FROZEN_ENV] == 0
        assert np.isnan(loss[FROZEN_ENV]) and np.isnan(viol[FROZEN_ENV]) and np.isnan(vm[FROZEN_ENV]).all()
        assert st[FAILING_ENV] == 2 and (a[FAILING_ENV] == 0).all() and np.isnan(loss[FAILING_ENV]) and np.isnan(vm[FAILING_ENV]).all()
        assert (st[ordinary] <= 1).all()
        same_run(runs["mixed", L], runs["plain", L], ordinary, ordinary, f"sp_lanes {L}: beside a stopped and a failing env")
        same_run(runs["mixed", L], runs["mixed", OS.fits(key)[0]], what=f"sp_lanes {L}")


@pytest.mark.parametrize("key", ["tri3", "grid6"])
def test_stopped_by_the_episode_limit(key):
    net, prof, _ = OS.make(key)
    B = 5
    for L in OS.fits(key):
        env = make_env(key, B, L, episode_limit=2)
        try:
            env.reset()
            a, loss, viol, it, st, vm = opf(env)
            assert (st <= 1).all() and np.isfinite(loss).all()
            for _ in range(2):
                _, term, _ = env.step(torch.as_tensor(a, device=DEV))
            assert bool(term.all())
            a, loss, viol, it, st, vm = opf(env)
            assert (st == 3).all() and (a == 0).all() and (it == 0).all() and np.isnan(vm).all() and np.isnan(loss).all() and np.isnan(viol).all()
            out = probe(env, np.zeros((B, net.n_sgen)))
            assert not out.linearised.any() and (out.d == 0).all() and (out.y == 0).all()
        finally:
            env.close()


# ---- 10. the contract -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("after_solve", [False, True])
def test_state_untouched_and_step_agrees(after_solve):
    def baseline(env):
        a, loss, viol, it, st, vm = env.opf_actions(MESHED, vm_pu=True)
        print("wheel_rim", after_solve, "status", st.tolist(), "iterations", it.tolist())
        return a, st, vm
    check_state_untouched_and_step_agrees(lambda B: make_env("wheel_rim", B), baseline, after_solve, B=24)


def test_baseline_tester_runs_on_the_meshed_feeder():
    args = types.SimpleNamespace(max_steps=3, action_scale=0.8, action_bias=0.0)
    stats = {}
    for ctrl in (OPFControl(OPFConfig(meshed=1), keep_history=True), NoControl()):
        env = make_env("case33_meshed", 4)
        try:
            stats[ctrl.name] = BaselineTester(args, ctrl, env).batch_run(4)
        finally:
            env.close()
        if ctrl.name == "opf":
            assert all((h[3] <= 1).all() for h in ctrl.history)
    assert stats["opf"].keys() == stats["no_control"].keys()
    assert all(np.isfinite(v).all() for v in stats["opf"].values())
    assert stats["opf"]["mean_test_total_line_loss"][0] <= stats["no_control"]["mean_test_total_line_loss"][0]


def test_refusal_on_a_live_handle_without_the_switch():
    env = make_env("tri3", 3)
    try:
        env.reset()
        with pytest.raises(Exception, match="meshed nets and handles on another solver than the tree solver are not supported"):
            env.opf_actions()
        assert (opf(env)[4] <= 1).all()
    finally:
        env.close()
