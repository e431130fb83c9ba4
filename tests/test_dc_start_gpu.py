"""GPU (-m gpu) tests of the DC-angle start (runpp init="dc", mapdn_env_config.nr_init = 2) on nets with a line above 70 kV, against
oracle.pp_restated.runpp_restated(init="dc"): solve_only on the tree and the sparse solver, the flat start's failure where the DC start
converges, every compiled DC geometry against the automatic one, and an auto-reset episode of VoltageControlBatch replayed on the
oracle env with the DC start."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import oracle.env_restated as env_restated
from mapdn_amd.data import from_pandapower
from mapdn_amd.env import VoltageControlBatch
from mapdn_amd.netspec import Profiles, case33_meshed, make_case
from oracle.env_restated import INFO_KEYS, VoltageControlOracle
from oracle.pp_restated import runpp_restated
from tests.dc_nets import dc_oracle, hv_front
from tests.test_data_ingestion import hv_line_net

pytestmark = pytest.mark.gpu

V_TOL = 1e-9
ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0, voltage_barrier_type="bowl", seed=0)


def hv_line_case():
    """the 150 degree vector-group net of tests/test_data_ingestion.py with a small profile table around its element values"""
    pnet = hv_line_net()
    net = from_pandapower(pnet, hv_init="auto")
    rng = np.random.default_rng(0)
    T = 480 * 3
    f = 0.75 + 0.5 * rng.random((T, 1))
    prof = Profiles(pv=pnet.sgen["p_mw"].to_numpy()[None, :] * rng.uniform(0.0, 1.2, (T, net.n_sgen)),
                    load_p=pnet.load["p_mw"].to_numpy()[None, :] * f, load_q=pnet.load["q_mvar"].to_numpy()[None, :] * f,
                    time_delta_min=3, days=2)
    return net, prof


def case(name):
    if name == "hv_line":
        return hv_line_case()
    if name == "case141_hv":
        net, prof = make_case("case141")
        return hv_front(net, 150.0), prof
    if name == "case33_meshed_hv":
        net, prof = make_case("case33")
        return hv_front(case33_meshed(net, 5), 30.0), prof
    raise KeyError(name)


def inputs(net, prof, B, seed):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, prof.n_rows, B)
    smax = prof.s_max()
    pl, ql, pv = prof.load_p[rows], prof.load_q[rows], prof.pv[rows]
    qs = rng.uniform(-0.8, 0.8, (B, net.n_sgen)) * np.sqrt(np.maximum(smax ** 2 - pv ** 2, 0.0))
    return pl, ql, pv, qs


def solve(net, prof, B, tuning, ins):
    env = VoltageControlBatch(net, prof, ARGS, n_envs=B, device="cuda:0", obs_dtype=torch.float64, tuning=tuning)
    try:
        out = [x.cpu().numpy() for x in env.solve(*ins)]
        return out, env.geometry()
    finally:
        env.close()


@pytest.mark.parametrize("name,solver", [("hv_line", "tree"), ("hv_line", "sparse"), ("case141_hv", "tree"), ("case141_hv", "sparse"),
                                         ("case33_meshed_hv", "auto")])
def test_solve_only_from_the_dc_start_matches_runpp(name, solver):
    net, prof = case(name)
    assert net.va_init == "dc"
    B = 70
    ins = inputs(net, prof, B, 5)
    (vm, va, it, cv), g = solve(net, prof, B, dict(nr_solver=solver), ins)
    assert g["nr_init"] == 2 and g["solver"] == {"tree": 0, "sparse": 1, "auto": 1}[solver]
    assert cv.all()
    worst = 0.0
    for e in range(B):
        r, agrees = dc_oracle(net, *(x[e] for x in ins))
        assert r.converged and agrees(it[e], cv[e]), (e, it[e], r.iterations)
        v = vm[e] * np.exp(1j * np.radians(va[e]))
        worst = max(worst, np.abs(v - r.V).max())
    assert worst <= V_TOL, worst


@pytest.mark.parametrize("name", ["hv_line", "case141_hv"])
def test_the_flat_start_fails_where_the_dc_start_converges(name):
    """the behaviour the feature exists for: with a 150 degree vector group the flat start does not converge (the env would report an
    unsolvable step, -200 and terminate) while runpp — and now the product — solves from the DC angles"""
    net, prof = case(name)
    B = 70
    ins = inputs(net, prof, B, 9)
    (_, _, _, cv_dc), _ = solve(net, prof, B, None, ins)
    (_, _, it_f, cv_f), g = solve(dataclasses.replace(net, va_init="flat"), prof, B, None, ins)
    assert g["nr_init"] == 0
    flat = np.array([runpp_restated(net, *(x[e] for x in ins), init="flat").converged for e in range(B)])
    assert cv_dc.all()
    assert np.array_equal(cv_f, flat)                           # the flat start fails exactly where pandapower's flat start would ...
    assert (~flat).sum() >= B // 2                              # ... which is most of these envs (lightly loaded ones may still converge)


# the DC-start geometries of nr_inst_list.hpp, pinned (waves, lanes, lean, G in LDS)
PINS = [(1, 16, 2, 1), (1, 16, 2, 2), (1, 16, 1, 0), (2, 16, 2, 1), (2, 16, 2, 2), (2, 16, 1, 0), (4, 16, 2, 1), (4, 16, 2, 2),
        (4, 16, 1, 0), (4, 8, 2, 1), (4, 8, 2, 2), (4, 8, 1, 0)]


@pytest.mark.parametrize("name", ["hv_line", "case141_hv"])
def test_every_compiled_dc_geometry_gives_the_bits_of_the_automatic_one(name):
    net, prof = case(name)
    B = 96
    ins = inputs(net, prof, B, 13)
    (vm0, va0, it0, cv0), g0 = solve(net, prof, B, None, ins)
    assert cv0.all() and g0["solver"] == 0
    ran = 0
    for w, l, lean, gl in PINS:
        t = dict(nr_waves=w, nr_lanes=l, nr_lean=lean)
        if gl:
            t["nr_g_lds"] = gl
        try:
            (vm, va, it, cv), g = solve(net, prof, B, t, ins)
        except RuntimeError as ex:                              # a fat layout that does not fit the LDS with this net: nothing to compare
            assert "LDS" in str(ex) or "fit" in str(ex), (t, str(ex))
            continue
        assert (g["waves"], g["lanes"]) == (w, l) and g["nr_init"] == 2
        assert np.array_equal(vm, vm0) and np.array_equal(va, va0) and np.array_equal(it, it0) and np.array_equal(cv, cv0), t
        ran += 1
    assert ran >= 8


def test_auto_reset_episode_from_the_dc_start_matches_the_oracle_env(monkeypatch):
    """VoltageControlBatch on the 150 degree HV net (NetSpec.va_init = "dc" -> nr_init = 2): reset, steps with one unsolvable action and
    auto-reset; rewards, terminated, info, obs and voltages per step against VoltageControlOracle with runpp_restated(init="dc") on every
    env's own load / PV values (the env's loads read back through mapdn_get_loads)"""
    monkeypatch.setattr(env_restated, "runpp_restated", functools.partial(runpp_restated, init="dc"))
    net, prof = hv_line_case()
    B, limit = 3, 6
    args = dict(ARGS, episode_limit=limit, auto_reset=True)
    env = VoltageControlBatch(net, prof, args, n_envs=B, device="cuda:0", obs_dtype=torch.float64)
    assert env.geometry()["nr_init"] == 2
    oracles = [VoltageControlOracle(net, prof, dict(ARGS, episode_limit=limit), env_id=e, do_reset=False) for e in range(B)]
    obs, _ = env.reset()
    for e, o in enumerate(oracles):
        oo, _ = o.reset()
        assert np.abs(np.array(oo) - obs[e].cpu().numpy()).max() < 1e-9
    rng = np.random.default_rng(17)
    pending = [False] * B
    n_term = [0] * B
    for t in range(2 * limit + 3):
        act = rng.uniform(-0.8, 0.8, (B, net.n_sgen))
        if t == 2:
            act[1] = 60.0                                       # env 1: an unsolvable power flow -> terminates early
        lp_before = env.loads()[0].cpu().numpy()
        r, term, info = env.step(torch.as_tensor(act, device="cuda:0"))
        obs = env.get_obs().cpu().numpy()
        vm = env.results(["vm_pu"])["vm_pu"].cpu().numpy()
        mask = env.auto_reset_mask().cpu().numpy()
        for e, o in enumerate(oracles):
            if pending[e]:
                assert mask[e] and r[e].item() == 0.0 and not term[e].item()
                oo, _ = o.reset()
                assert np.abs(np.array(oo) - obs[e]).max() < 1e-9, (t, e)
                pending[e] = False
                continue
            assert not mask[e]
            assert np.abs(lp_before[e] - o.load_p).max() < 1e-12    # the env's own loads, the ones the oracle solves with
            ro, to, io = o.step(act[e])
            assert abs(ro - r[e].item()) < 1e-9 and to == bool(term[e].item()), (t, e, ro, r[e].item())
            assert max(abs(io[k] - info[e, c].item()) for c, k in enumerate(INFO_KEYS)) < 1e-9
            assert np.abs(o.res.vm_pu - vm[e]).max() < V_TOL, (t, e)
            assert np.abs(np.array(o.get_obs()) - obs[e]).max() < 1e-9, (t, e)
            if to:
                pending[e] = True
                n_term[e] += 1
    assert n_term[1] >= 2 and min(n_term) >= 1
    env.close()
