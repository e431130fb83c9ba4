"""GPU (-m gpu) tests of the droop baseline (VoltageControlBatch.droop_actions -> mapdn_droop_actions, csrc/droop.hip) against the
numpy restatement of the reference's MATLAB loop (tests/droop_ref.py) on the oracle's power flow, and of what the call must leave
alone: the env's state, its next step(), the counters; bits across k_nr_tree geometries and batch sizes; BaselineTester against the
oracle env driven by droop_ref."""
import functools
import types

import numpy as np
import pytest
import torch

from mapdn_amd.baselines import BaselineTester, DroopConfig, DroopControl, NoControl
from mapdn_amd.env import VoltageControlBatch
from mapdn_amd.tester import PGTester
from oracle.env_restated import INFO_KEYS, VoltageControlOracle
from oracle.pp_restated import runpp_restated
from tests import kernel_matrix as km
from tests.baseline_contract import check_state_untouched_and_step_agrees, env_state
from tests.droop_ref import droop_ref, droop_ref_oracle
from tests.zip_nets import runpp_zip

pytestmark = pytest.mark.gpu

ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0, voltage_barrier_type="bowl", seed=0)
DEV = "cuda:0"
TOL = 1e-9
V_TOL = 1e-4


def runpp_for(key):
    if "_zip" in key:
        return runpp_zip
    if "_hv" in key:
        return functools.partial(runpp_restated, init="dc")
    return runpp_restated


def make_env(key, B, args=None, **kw):
    net, prof = km.make_net(key)
    a = dict(ARGS)
    a.update(args or {})
    return VoltageControlBatch(net, prof, a, n_envs=B, device=DEV, obs_dtype=torch.float64, **kw)


def droop(env, cfg=None):
    a, it, st, vm = env.droop_actions(cfg, vm_pu=True)
    return a.cpu().numpy(), it.cpu().numpy(), st.cpu().numpy(), vm.cpu().numpy()


def check_parity(key, env, cfg=None):
    net, _ = km.make_net(key)
    lp, lq, pv, smax = env_state(env)
    a, it, st, vm = droop(env, cfg)
    runpp = runpp_for(key)
    v_tol = cfg.v_tol if cfg is not None else V_TOL
    worst, compared = 0.0, 0
    for e in range(env.n_envs):
        r = droop_ref(net, lp[e], lq[e], pv[e], smax, cfg, runpp)
        assert st[e] == r.status, (key, e, st[e], r.status, it[e], r.iterations)
        if it[e] != r.iterations:
            k = min(it[e], r.iterations)
            assert abs(int(it[e]) - r.iterations) == 1 and abs(r.dists[k - 1] - v_tol) <= 1e-8, (key, e, it[e], r.iterations)
            continue
        compared += 1
        worst = max(worst, float(np.abs(a[e] - r.actions).max()))
        if r.status in (0, 1):
            worst = max(worst, float(np.abs(vm[e] - r.vm_pu).max()))
        else:
            assert np.isnan(vm[e]).all()
    assert worst < TOL, (key, worst)
    return it, st, compared


@pytest.mark.parametrize("key", ["case33", "case141", "case322", "case33_meshed", "case33_hv", "case33_zip"])
def test_parity_with_the_cpu_reference(key):
    B = 16
    env = make_env(key, B)
    try:
        prof = km.make_net(key)[1]
        env.reset()                                                     # seeded, noisy starts
        it, st, n = check_parity(key, env)
        assert n >= B // 2 and (st <= 1).all() and (it >= 2).all()
        env.step(torch.as_tensor(droop(env)[0], device=DEV))           # one step further: the state after a droop-driven step
        check_parity(key, env)
        rows = [prof.start_row(d % (prof.days - 2), 12, d // (prof.days - 2)) for d in range(B)]             # noon: high PV
        env.reset(start_rows=torch.tensor(rows))
        it2, st2, _ = check_parity(key, env)
        assert (st2 <= 1).all()
        check_parity(key, env, DroopConfig(vb=0.98, vc=1.02, damping=0.3, max_iter=7))    # a deadband; max_iter reached
    finally:
        env.close()


@pytest.mark.parametrize("key", ["case141", "case33_meshed", "case322"])
@pytest.mark.parametrize("after_solve", [False, True])
def test_state_untouched_and_step_agrees(key, after_solve):
    def baseline(env):
        a, it, st, vm = env.droop_actions(vm_pu=True)
        return a, st, vm
    check_state_untouched_and_step_agrees(lambda B: make_env(key, B), baseline, after_solve, B=24)


def test_bits_across_compiled_tree_geometries():
    rows = [r for r in km.ROWS if r.kernel[0] == "tree" and r.net == "case141"]
    assert len(rows) >= 2
    prof = km.make_net("case141")[1]
    starts = torch.tensor([prof.start_row(d % 5, (6 + 3 * d) % 24, 0) for d in range(km.B_ROW)])
    ref = None
    for row in rows:
        env = make_env("case141", row.B, tuning=row.tuning)
        try:
            assert km.kernel_tuple(env.nr_kernel()) == row.kernel
            env.reset(start_rows=starts)
            out = droop(env)
        finally:
            env.close()
        if ref is None:
            ref = out
        else:
            for x, y in zip(ref, out):
                assert np.array_equal(x, y, equal_nan=True), row


def test_one_env_gives_the_bits_of_the_batch():
    prof = km.make_net("case141")[1]
    B = 256
    rng = np.random.default_rng(5)
    starts = torch.tensor(rng.integers(0, prof.n_rows - 300, B))
    big = make_env("case141", B)
    try:
        big.reset(start_rows=starts)
        full = droop(big)
    finally:
        big.close()
    for e in (0, 77, 255):
        one = make_env("case141", 1, env_id_offset=e)
        try:
            one.reset(start_rows=starts[e:e + 1])
            o = droop(one)
        finally:
            one.close()
        for x, y in zip(full, o):
            assert np.array_equal(x[e], y[0], equal_nan=True), e


def test_stopped_envs_get_status_3():
    for args in (dict(episode_limit=2), dict(episode_limit=2, auto_reset=True)):
        env = make_env("case33", 8, args)
        try:
            env.reset()
            a, it, st, vm = droop(env)
            assert (st <= 1).all()
            _, term, _ = env.step(torch.as_tensor(a, device=DEV))
            assert bool(term.all())                                     # terminated (frozen, or waiting for the auto-reset restart)
            a, it, st, vm = droop(env)
            assert (st == 3).all() and (a == 0).all() and (it == 0).all() and np.isnan(vm).all()
            if args.get("auto_reset"):
                env.step(torch.as_tensor(a, device=DEV))                # the restart
                assert (droop(env)[2] <= 1).all()
        finally:
            env.close()


def test_early_exit_bounds_the_solve_launches():
    env = make_env("case141", 64)
    try:
        env.reset()
        env.nr_timing(True)
        env.nr_time_ms()
        _, it, st = env.droop_actions()
        ms, launches = env.nr_time_ms()
        env.nr_timing(False)
        m = int(it.max())
        assert m <= launches <= m + 3, (m, launches)
    finally:
        env.close()


class _ZeroPolicy(torch.nn.Module):
    def __init__(self, n_agents):
        super().__init__()
        self.n_agents = n_agents

    def init_hidden(self, B):
        return None

    def get_actions(self, obs, status, exploration, avail, target, last_hid):
        return torch.zeros(obs.shape[0], self.n_agents, 1, device=obs.device), None, None, None, None


def test_baseline_tester_matches_the_oracle_env():
    B, steps = 8, 24
    env = make_env("case33", B)
    net, prof = km.make_net("case33")
    try:
        tester = BaselineTester(types.SimpleNamespace(max_steps=steps), DroopControl(), env)
        stat = tester.batch_run(B)
    finally:
        env.close()
    oracles = [VoltageControlOracle(net, prof, ARGS, env_id=e, do_reset=False) for e in range(B)]
    infos = []
    for o in oracles:
        o.reset()
        for t in range(steps):
            r = droop_ref_oracle(o)
            _, term, info = o.step(r.actions, add_noise=False)
            infos.append([info[k] for k in INFO_KEYS])
            if term:
                break
    allv = np.array(infos)
    for c, k in enumerate(INFO_KEYS):
        m, s2 = stat["mean_test_" + k]
        assert abs(m - allv[:, c].mean()) < 1e-9 and abs(s2 - 2.0 * allv[:, c].std()) < 1e-9, k


def test_baseline_record_has_the_format_of_pg_tester():
    args = types.SimpleNamespace(max_steps=6, action_scale=0.8, action_bias=0.0)
    def run(make_tester):                                               # a fresh handle each: reset draws its initial action
        env = make_env("case33", 2)                                     # from the handle's draw counter
        try:
            return make_tester(env).run(1, 12, 0)
        finally:
            env.close()
    pg = run(lambda env: PGTester(args, _ZeroPolicy(env.n_agents), env))
    nc = run(lambda env: BaselineTester(args, NoControl(), env))
    dr = run(lambda env: BaselineTester(args, DroopControl(), env))
    assert pg.keys() == nc.keys() == dr.keys()
    for k in pg:
        assert len(pg[k]) == len(nc[k]) == len(dr[k])
        for x, y, z in zip(pg[k], nc[k], dr[k]):
            assert x.shape == y.shape == z.shape and x.dtype == z.dtype
            assert np.array_equal(x, y)                                 # a zero policy is no control
    assert not np.array_equal(nc["pv_reactive"][-1], dr["pv_reactive"][-1])
