"""GPU (-m gpu) tests of voltage-dependent (ZIP) loads (NetSpec.load_const_z / load_const_i, runpp voltage_depend_loads=True) against
tests/zip_nets.py::runpp_zip: solve_only on the tree and the sparse solver, with the flat and the DC start, every compiled ZIP geometry
against the automatic one, explicit all-zero columns against NULL ones, and episodes of VoltageControlBatch / VoltageControl replayed on
the oracle env with runpp_zip in place of runpp_restated."""
import dataclasses

import numpy as np
import pytest
import torch

import oracle.env_restated as env_restated
from mapdn_amd import _lib
from mapdn_amd.data import from_pandapower
from mapdn_amd.env import VoltageControl, VoltageControlBatch
from mapdn_amd.netspec import case33_meshed, make_case
from oracle.env_restated import INFO_KEYS, VoltageControlOracle
from tests.dc_nets import hv_front
from tests.test_zip_loads_cpu import zip_substation
from tests.zip_nets import runpp_zip, with_zip, zip_oracle

pytestmark = pytest.mark.gpu

V_TOL = 1e-9
ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0, voltage_barrier_type="bowl", seed=0)
FRACTIONS = [(0.3, 0.2), (1.0, 0.0), (0.0, 1.0)]


def base(name):
    if name == "case33_meshed":
        net, prof = make_case("case33")
        return case33_meshed(net, 5), prof
    if name == "case33_vm103":
        net, prof = make_case("case33")
        return dataclasses.replace(net, ext_grid_vm_pu=1.03), prof
    if name.endswith("_hv"):
        net, prof = make_case(name[:-3])
        return hv_front(net, 150.0), prof
    return make_case(name)


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
        return [x.cpu().numpy() for x in env.solve(*ins)], env.geometry()
    finally:
        env.close()


def check_against_oracle(net, ins, out):
    vm, va, it, cv = out
    worst = 0.0
    for e in range(vm.shape[0]):
        r, agrees = zip_oracle(net, *(x[e] for x in ins))
        assert agrees(it[e], cv[e]), (e, it[e], cv[e], r.iterations, r.converged)
        if r.converged:
            v = vm[e] * np.exp(1j * np.radians(va[e]))
            worst = max(worst, np.abs(v - r.V).max())
    assert worst <= V_TOL, worst


@pytest.mark.parametrize("name,solver", [("case33", "tree"), ("case33", "sparse"), ("case141", "tree"), ("case141", "sparse"),
                                         ("case322", "tree"), ("case33_meshed", "auto"), ("case33_vm103", "tree")])
@pytest.mark.parametrize("cz,ci", FRACTIONS)
def test_solve_only_with_zip_loads_matches_runpp(name, solver, cz, ci):
    net, prof = base(name)
    z = with_zip(net, cz, ci)
    B = 48
    ins = inputs(z, prof, B, 5)
    out, g = solve(z, prof, B, dict(nr_solver=solver), ins)
    assert g["solver"] == {"tree": 0, "sparse": 1, "auto": 1}[solver]
    assert out[3].mean() > 0.5                                  # (heavy constant-Z rows may not converge in 10 chord-like
    check_against_oracle(z, ins, out)                           # iterations; the flags are compared with the oracle's)


@pytest.mark.parametrize("name", ["case33_hv", "case141_hv"])
@pytest.mark.parametrize("solver", ["tree", "sparse"])
def test_zip_loads_with_the_dc_start_match_runpp(name, solver):
    net, prof = base(name)
    z = with_zip(net, 0.3, 0.2)
    assert z.va_init == "dc"
    B = 48
    ins = inputs(z, prof, B, 7)
    out, g = solve(z, prof, B, dict(nr_solver=solver), ins)
    assert g["nr_init"] == 2
    assert out[3].mean() > 0.5
    check_against_oracle(z, ins, out)


# the ZIP geometries of nr_inst_list.hpp, pinned (waves, lanes, lean, G in LDS)
PINS = [(1, 16, 2, 1), (1, 16, 1, 0), (2, 16, 1, 0), (4, 16, 2, 2), (4, 16, 1, 0), (4, 8, 2, 2), (4, 8, 1, 0)]


@pytest.mark.parametrize("name", ["case33", "case141", "case141_hv"])
def test_every_compiled_zip_geometry_gives_the_bits_of_the_automatic_one(name):
    net, prof = base(name)
    z = with_zip(net, 0.3, 0.2)
    B = 96
    ins = inputs(z, prof, B, 13)
    out0, g0 = solve(z, prof, B, None, ins)
    assert out0[3].mean() > 0.5 and g0["solver"] == 0
    ran = 0
    for w, l, lean, gl in PINS:
        t = dict(nr_waves=w, nr_lanes=l, nr_lean=lean)
        if gl:
            t["nr_g_lds"] = gl
        try:
            out, g = solve(z, prof, B, t, ins)
        except RuntimeError as ex:                              # a fat layout that does not fit the LDS with this net
            assert "LDS" in str(ex) or "fit" in str(ex), (t, str(ex))
            continue
        assert (g["waves"], g["lanes"]) == (w, l)
        assert all(np.array_equal(a, b) for a, b in zip(out, out0)), t
        ran += 1
    assert ran >= 4


def test_explicit_zero_columns_are_the_constant_power_path(monkeypatch):
    """all-zero load_const_z / _i passed as real arrays (not NULL): bit-identical step outputs over a short episode"""
    net, prof = make_case("case141")
    B = 32

    def run():
        env = VoltageControlBatch(net, prof, ARGS, n_envs=B, device="cuda:0", obs_dtype=torch.float64)
        obs, _ = env.reset()
        outs = [obs.cpu().numpy().copy()]
        rng = np.random.default_rng(3)
        for _ in range(4):
            r, term, info = env.step(torch.as_tensor(rng.uniform(-0.8, 0.8, (B, net.n_sgen)), device="cuda:0"))
            res = env.results()
            outs += [r.cpu().numpy().copy(), term.cpu().numpy().copy(), info.cpu().numpy().copy(), env.get_obs().cpu().numpy().copy()]
            outs += [v.cpu().numpy().copy() for v in res.values()]
        env.close()
        return outs

    a = run()
    orig = _lib.make_cnetspec

    def explicit(n):
        s, keep = orig(n)
        s.load_const_z = _lib._p(n.load_const_z, _lib._pd)
        s.load_const_i = _lib._p(n.load_const_i, _lib._pd)
        return s, keep
    monkeypatch.setattr(_lib, "make_cnetspec", explicit)
    b = run()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def zip_case141():
    net, prof = make_case("case141")
    return with_zip(net, 0.3, 0.2), prof


def test_auto_reset_episode_with_zip_loads_matches_the_oracle_env(monkeypatch):
    """VoltageControlBatch on a net converted with zip_loads="runpp": reset, steps with an unsolvable action and auto-reset; rewards,
    terminated, info, obs, state and res_bus per step against VoltageControlOracle on runpp_zip"""
    monkeypatch.setattr(env_restated, "runpp_restated", runpp_zip)
    net = from_pandapower(zip_substation(), zip_loads="runpp")
    pnet = zip_substation()
    rng = np.random.default_rng(0)
    T = 480 * 3
    f = 0.75 + 0.5 * rng.random((T, 1))
    from mapdn_amd.netspec import Profiles
    prof = Profiles(pv=pnet.sgen["p_mw"].to_numpy()[None, :] * rng.uniform(0.0, 1.2, (T, net.n_sgen)),
                    load_p=pnet.load["p_mw"].to_numpy()[None, :] * f, load_q=pnet.load["q_mvar"].to_numpy()[None, :] * f,
                    time_delta_min=3, days=2)
    B, limit = 3, 6
    args = dict(ARGS, episode_limit=limit, auto_reset=True)
    env = VoltageControlBatch(net, prof, args, n_envs=B, device="cuda:0", obs_dtype=torch.float64)
    oracles = [VoltageControlOracle(net, prof, dict(ARGS, episode_limit=limit), env_id=e, do_reset=False) for e in range(B)]
    obs, _ = env.reset()
    for e, o in enumerate(oracles):
        oo, _ = o.reset()
        assert np.abs(np.array(oo) - obs[e].cpu().numpy()).max() < 1e-9
    pending = [False] * B
    n_term = [0] * B
    arng = np.random.default_rng(17)
    for t in range(2 * limit + 3):
        act = arng.uniform(-0.8, 0.8, (B, net.n_sgen))
        if t == 2:
            act[1] = 60.0                                       # env 1: an unsolvable power flow -> terminates early
        r, term, info = env.step(torch.as_tensor(act, device="cuda:0"))
        obs = env.get_obs().cpu().numpy()
        state = env.get_state().cpu().numpy()
        res = {k: v.cpu().numpy() for k, v in env.results(["vm_pu", "p_mw", "q_mvar"]).items()}
        mask = env.auto_reset_mask().cpu().numpy()
        for e, o in enumerate(oracles):
            if pending[e]:
                assert mask[e] and not term[e].item()
                oo, _ = o.reset()
                assert np.abs(np.array(oo) - obs[e]).max() < 1e-9, (t, e)
                pending[e] = False
                continue
            ro, to, io = o.step(act[e])
            assert abs(ro - r[e].item()) < 1e-9 and to == bool(term[e].item()), (t, e, ro, r[e].item())
            assert max(abs(io[k] - info[e, c].item()) for c, k in enumerate(INFO_KEYS)) < 1e-9
            assert np.abs(o.res.vm_pu - res["vm_pu"][e]).max() < V_TOL, (t, e)
            for k in ("p_mw", "q_mvar"):
                assert np.all(np.abs(o.res[k] - res[k][e]) <= 1e-9 * np.maximum(1.0, np.abs(o.res[k]))), (t, e, k)
            assert np.abs(np.array(o.get_obs()) - obs[e]).max() < 1e-9, (t, e)
            assert np.abs(np.array(o.get_state()) - state[e]).max() < 1e-9, (t, e)
            if to:
                pending[e] = True
                n_term[e] += 1
    assert n_term[1] >= 1
    env.close()


def test_single_env_class_runs_a_zip_step(monkeypatch):
    monkeypatch.setattr(env_restated, "runpp_restated", runpp_zip)
    net, prof = zip_case141()
    kw = dict(ARGS, net=net, profiles=prof)
    env = VoltageControl(kw, device="cuda:0")
    oracle = VoltageControlOracle(net, prof, ARGS, env_id=0, do_reset=False)
    oracle.draw = 1                                             # the constructor's reset consumed draw 0 (voltage_control_env.py:85)
    env.reset()
    oracle.reset()
    act = np.random.default_rng(2).uniform(-0.8, 0.8, net.n_sgen)
    r, term, info = env.step(act)
    ro, to, io = oracle.step(act)
    assert abs(r - ro) < 1e-9 and bool(term) == bool(to)
    assert np.abs(np.asarray(env._get_res_bus_v()) - oracle.res.vm_pu).max() < V_TOL
    assert np.abs(np.asarray(env._get_res_bus_active()) - oracle.res.p_mw).max() < 1e-9
    env.close()


def test_dense_solver_is_refused_by_name():
    net, prof = zip_case141()
    with pytest.raises(RuntimeError, match="dense"):
        VoltageControlBatch(net, prof, ARGS, n_envs=16, device="cuda:0", tuning=dict(nr_solver="dense"))
