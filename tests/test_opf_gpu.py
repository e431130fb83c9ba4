"""GPU (-m gpu) tests of the OPF baseline (VoltageControlBatch.opf_actions -> mapdn_opf_actions, csrc/opf.hip) against the stored optima
(tests/golden/opf_golden.npz: scipy on the oracle's power flow, certified by KKT residuals) and the stored run of the numpy restatement
(tests/opf_ref.py), and of what the call must leave alone: the env's state, its next step(); bits across batch sizes and runs; the
statuses at the edges; BaselineTester's formats."""
import os
import types

import numpy as np
import pytest
import torch

from mapdn_amd.baselines import BaselineTester, DroopControl, OPFConfig, OPFControl
from mapdn_amd.env import VoltageControlBatch
from mapdn_amd.netspec import make_case
from oracle.pp_restated import runpp_restated
from tests import kernel_matrix as km
from tests import opf_ref as R
from tests.baseline_contract import check_state_untouched_and_step_agrees, env_state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "opf_golden.npz"))
ROWS = [int(r) for r in GOLDEN["rows"]]
V_LOWER, V_UPPER = (float(x) for x in GOLDEN["v_bounds"])
ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0, voltage_barrier_type="bowl", seed=0)
DEV = "cuda:0"
V_TOL, STEP_TOL = 5e-6, 1e-6
BATCH = dict(case33=19, case141=17)               # neither a multiple of the 16 envs of a workgroup
# Measured on an MI355X over the 36 envs of the two batches, rounded up: the loss is within a relative
# LOSS_GAP_MEASURED of the stored optimum (2.092e-11 / 8.115e-11), the actions within A_GAP_MEASURED of the restated SQP's (4.33e-13 /
# 3.72e-8).  The bounds are ten times that, per case (the loss bound never looser than 1e-3: the paper's PL column has three
# significant digits).
LOSS_GAP_MEASURED = dict(case33=2.1e-11, case141=8.2e-11)
A_GAP_MEASURED = dict(case33=4.4e-13, case141=3.8e-8)
LOSS_GAP_BOUND = {c: min(10.0 * x, 1e-3) for c, x in LOSS_GAP_MEASURED.items()}
A_BOUND = {c: 10.0 * x for c, x in A_GAP_MEASURED.items()}


def make_env(case, B, args=None, days=3, **kw):
    net, prof = make_case(case, days=days)
    a = dict(ARGS)
    a.update(args or {})
    return VoltageControlBatch(net, prof, a, n_envs=B, device=DEV, obs_dtype=torch.float64, **kw), net, prof


def place(env, prof, rows):
    """a noise-free start whose current state is exactly the profile row rows[e] of every env (manual_reset's kind of start)"""
    rows = np.asarray(rows)
    env.reset(start_rows=torch.tensor(rows), add_noise=False)
    lp = env_state(env)[0]
    off = [k for k in (0, 1, -1, 2) if np.array_equal(lp[0], prof.load_p[rows[0] + k])]
    assert off, "the env's loads are no profile row near its start row"
    if off[0]:
        env.reset(start_rows=torch.tensor(rows - off[0]), add_noise=False)
    lp, lq, pv, smax = env_state(env)
    assert np.array_equal(lp, prof.load_p[rows]) and np.array_equal(lq, prof.load_q[rows]) and np.array_equal(pv, prof.pv[rows])
    assert np.array_equal(smax, prof.s_max(1.2))


def opf(env, cfg=None):
    return tuple(x.cpu().numpy() for x in env.opf_actions(cfg, vm_pu=True))


@pytest.fixture(scope="module")
def runs():
    """per case: the batch on the golden rows, solved twice, and single envs — computed once, shared by the tests below"""
    out = {}
    for case, B in BATCH.items():
        rows = [ROWS[e % len(ROWS)] for e in range(B)]
        env, net, prof = make_env(case, B)
        try:
            place(env, prof, rows)
            first, second = opf(env), opf(env)
        finally:
            env.close()
        singles = {}
        for e in (0, B - 1):
            one, _, _ = make_env(case, 1, env_id_offset=e)
            try:
                place(one, prof, rows[e:e + 1])
                singles[e] = opf(one)
            finally:
                one.close()
        out[case] = types.SimpleNamespace(net=net, prof=prof, rows=rows, first=first, second=second, singles=singles)
    return out


@pytest.mark.parametrize("case", list(BATCH))
def test_golden_agreement(runs, case):
    r = runs[case]
    a, loss, viol, it, st, vm = r.first
    smax = r.prof.s_max(1.2)
    worst_gap, worst_viol = 0.0, 0.0
    for e, t in enumerate(r.rows):
        assert st[e] == 0, (case, e, t, st[e], it[e], viol[e])
        lp, lq, pv = r.prof.load_p[t], r.prof.load_q[t], r.prof.pv[t]
        res = runpp_restated(r.net, lp, lq, pv, R.limits(pv, smax) * a[e])
        assert res.converged
        v = R.violation_of(res.vm_pu, r.net, V_LOWER, V_UPPER)
        worst_viol = max(worst_viol, v)
        assert abs(vm[e] - res.vm_pu).max() < 1e-9 and abs(viol[e] - v) < 1e-9
        gold = float(GOLDEN[f"{case}_{t}_loss_mw"])
        worst_gap = max(worst_gap, abs(loss[e] - gold) / gold)
    print(case, "loss gap", worst_gap, "violation", worst_viol, "iterations", it.tolist())
    assert worst_viol <= V_TOL + 1e-8, worst_viol
    assert worst_gap <= LOSS_GAP_BOUND[case], worst_gap


@pytest.mark.parametrize("case", list(BATCH))
def test_same_iterates_as_the_restated_sqp(runs, case):
    r = runs[case]
    a, loss, viol, it, st, vm = r.first
    worst = 0.0
    for e, t in enumerate(r.rows):
        k = f"{case}_{t}_ref_"
        ref_it, steps = int(GOLDEN[k + "iterations"]), GOLDEN[k + "steps"]
        worst = max(worst, float(np.abs(a[e] - GOLDEN[k + "a"]).max()))
        if it[e] != ref_it:                        # one side stopped a step earlier: its stop test lies at the threshold
            lo = min(int(it[e]), ref_it)
            assert abs(int(it[e]) - ref_it) == 1 and abs(steps[lo - 1] - STEP_TOL) <= A_BOUND[case], (case, e, t, it[e], ref_it, steps)
    print(case, "max |a - a_ref|", worst)
    assert worst <= A_BOUND[case], worst


@pytest.mark.parametrize("case", list(BATCH))
def test_runs_and_batch_sizes_give_the_same_bits(runs, case):
    r = runs[case]
    for x, y in zip(r.first, r.second):
        assert np.array_equal(x, y, equal_nan=True)
    for e, one in r.singles.items():
        for x, y in zip(r.first, one):
            assert np.array_equal(x[e], y[0], equal_nan=True), (case, e)


@pytest.mark.parametrize("case", ["case33", "case141", "case322"])
@pytest.mark.parametrize("after_solve", [False, True])
def test_state_untouched_and_step_agrees(case, after_solve):
    """the droop contract on the radial feeders droop is held to, from the same starts: noisy resets, two random-action steps"""
    net, prof = km.make_net(case)

    def baseline(env):
        a, loss, viol, it, st, vm = env.opf_actions(vm_pu=True)
        print(case, after_solve, "status", st.tolist(), "iterations", it.tolist())
        return a, st, vm
    check_state_untouched_and_step_agrees(lambda B: VoltageControlBatch(net, prof, dict(ARGS), n_envs=B, device=DEV, obs_dtype=torch.float64),
                                          baseline, after_solve, B=24)


def test_stopped_envs_get_status_3():
    for args in (dict(episode_limit=2), dict(episode_limit=2, auto_reset=True)):
        env, _, _ = make_env("case33", 8, args)
        try:
            env.reset()
            a, loss, viol, it, st, vm = opf(env)
            assert (st <= 1).all() and np.isfinite(loss).all()
            _, term, _ = env.step(torch.as_tensor(a, device=DEV))
            assert bool(term.all())                                     # terminated (frozen, or waiting for the auto-reset restart)
            a, loss, viol, it, st, vm = opf(env)
            assert (st == 3).all() and (a == 0).all() and (it == 0).all() and np.isnan(vm).all() and np.isnan(loss).all() and np.isnan(viol).all()
            if args.get("auto_reset"):
                env.step(torch.as_tensor(a, device=DEV))                # the restart
                assert (opf(env)[4] <= 1).all()
        finally:
            env.close()


def test_widest_feeder_runs():
    """case322: 38 sgens, three columns per sub-lane.  Finiteness and statuses only: widths like this one and beyond (33, 48, 49 and 64
    sgens) are held against an extended-precision reference, S, g and H entry by entry, in tests/test_opf_kernels_gpu.py."""
    net, prof = km.make_net("case322")
    env = VoltageControlBatch(net, prof, dict(ARGS), n_envs=16, device=DEV, obs_dtype=torch.float64)
    try:
        assert env.n_sgen == 38
        rows = torch.tensor([prof.start_row(d % (prof.days - 2), 8 + d % 8, 0) for d in range(16)])
        env.reset(start_rows=rows)
        a, loss, viol, it, st, vm = opf(env)
        print("case322 status", st.tolist(), "iterations", it.tolist(), "violation", float(viol.max()))
        assert np.isin(st, (0, 1)).all()
        assert np.isfinite(a).all() and np.isfinite(loss).all() and np.isfinite(viol).all() and np.isfinite(vm).all()
        assert (np.abs(a) <= 1.0).all() and (it >= 1).all() and (viol >= 0.0).all()
        assert (viol[st == 0] <= V_TOL).all()
    finally:
        env.close()


def check_point_against_the_oracle(net, prof, rows, out, v_lower=V_LOWER, v_upper=V_UPPER):
    """a, |V|, loss and violation belong together: the oracle's power flow at the returned a gives the returned rest"""
    a, loss, viol, it, st, vm = out
    smax = prof.s_max(1.2)
    ybus = R.make_ybus(net)[0]
    for e, t in enumerate(rows):
        pv = prof.pv[t]
        res = runpp_restated(net, prof.load_p[t], prof.load_q[t], pv, R.limits(pv, smax) * a[e])
        assert res.converged
        assert abs(vm[e] - res.vm_pu).max() < 1e-9 and abs(viol[e] - R.violation_of(res.vm_pu, net, v_lower, v_upper)) < 1e-9
        ref_loss = R.loss_pu(ybus, res.V) * net.sn_mva
        assert abs(loss[e] - ref_loss) <= 1e-9 * abs(ref_loss) + 1e-12, (e, loss[e], ref_loss)


def test_max_iter_gives_status_1_with_the_last_solved_point():
    rows = [240, 260, 700]
    env, net, prof = make_env("case141", 3)
    try:
        place(env, prof, rows)
        out = opf(env, OPFConfig(max_iter=2))
        a, loss, viol, it, st, vm = out
        assert (st == 1).all() and (it == 2).all()
        check_point_against_the_oracle(net, prof, rows, out)
        smax = prof.s_max(1.2)
        for e, t in enumerate(rows):               # the second solved point of the restated loop
            r = R.opf_ref(net, prof.load_p[t], prof.load_q[t], prof.pv[t], smax, OPFConfig(max_iter=2), V_LOWER, V_UPPER)
            assert r.status == 1 and r.iterations == 2 and np.abs(a[e] - r.actions).max() <= A_BOUND["case141"], (e, t)
            assert (np.abs(a[e]) > 0).any()
    finally:
        env.close()


def test_bounds_out_of_reach_give_status_1_before_max_iter():
    """a band of +-0.1 % that no set-point reaches: every QP reports that its rows cannot be met (the QP cap), and the loop stops with
    status 1 at a least-violation point once the violation stops coming down, as the restated loop does, and long before max_iter"""
    rows = [260, 700]
    cfg = OPFConfig(v_lower=0.999, v_upper=1.001)
    env, net, prof = make_env("case33", 2)
    try:
        place(env, prof, rows)
        out = opf(env, cfg)
        a, loss, viol, it, st, vm = out
        print("unreachable band: iterations", it.tolist(), "violation", viol.tolist())
        assert (st == 1).all() and (it >= 2).all() and (it <= 10).all() and (viol > V_TOL).all()
        check_point_against_the_oracle(net, prof, rows, out, 0.999, 1.001)
        smax = prof.s_max(1.2)
        for e, t in enumerate(rows):
            r = R.opf_ref(net, prof.load_p[t], prof.load_q[t], prof.pv[t], smax, cfg, V_LOWER, V_UPPER)
            assert r.status == 1 and r.iterations == it[e], (e, t, r.iterations, it[e])
            res0 = runpp_restated(net, prof.load_p[t], prof.load_q[t], prof.pv[t], np.zeros(net.n_sgen))
            assert viol[e] < R.violation_of(res0.vm_pu, net, 0.999, 1.001)         # better than doing nothing
    finally:
        env.close()


def test_baseline_tester_formats_equal_the_droop_ones():
    args = types.SimpleNamespace(max_steps=4, action_scale=0.8, action_bias=0.0)

    def run(ctrl):
        env, _, _ = make_env("case33", 2, days=10)
        try:
            t = BaselineTester(args, ctrl, env)
            return t.run(1, 12, 0), t.batch_run(2)
        finally:
            env.close()
    (dr, ds), (orc, os_) = run(DroopControl()), run(OPFControl(keep_history=True))
    assert dr.keys() == orc.keys() and ds.keys() == os_.keys()
    for k in dr:
        assert len(dr[k]) == len(orc[k])
        for x, y in zip(dr[k], orc[k]):
            assert x.shape == y.shape and x.dtype == y.dtype
    for k in ds:
        assert len(os_[k]) == 2 and all(np.isfinite(v) for v in os_[k])
    assert not np.array_equal(dr["pv_reactive"][-1], orc["pv_reactive"][-1])
