"""GPU (-m gpu) tests of generators (net.gen: gen buses, NetSpec.gen_*) against tests/gen_nets.py::runpp_gen: solve() on the tree and the
sparse solver with the flat and the DC start (every compiled GEN kernel: tests/test_kernel_matrix_gpu.py), Q_gen and
the commit of res_bus / res_gen against bars derived from the dot product's error bound, an auto-reset episode with an unsolvable step
replayed on the oracle env, the three injection paths against each other, evaluate_actions / res_line on such a handle, and the
refusals."""
import numpy as np
import pytest
import torch

import oracle.env_restated as env_restated
from mapdn_amd import _lib
from mapdn_amd.data import from_pandapower
from mapdn_amd.env import VoltageControl, VoltageControlBatch
from oracle.env_restated import INFO_KEYS, VoltageControlOracle
from oracle.pp_restated import _cached_ybus, bus_demand
from tests.dc_nets import hv_front
from tests.gen_nets import RADIAL, flat_profiles, gen_case, gen_oracle, gen_substation, inputs, q_bars, runpp_gen, tiny_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V_TOL = 1e-9
ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0, voltage_barrier_type="bowl", seed=0)
_REF = {}                                                       # (net name, seed, B, init) -> the oracle's results, computed once


def make_env(net, prof, B, tuning=None, **args):
    return VoltageControlBatch(net, prof, dict(ARGS, **args), n_envs=B, device=DEV, obs_dtype=torch.float64, tuning=tuning)


def solve(net, prof, B, tuning, ins):
    env = make_env(net, prof, B, tuning)
    try:
        return [x.cpu().numpy() for x in env.solve(*ins)], dict(env.geometry(), kernel=env.nr_kernel())
    finally:
        env.close()


def reference(key, net, ins):
    if key not in _REF:
        _REF[key] = [gen_oracle(net, *(x[e] for x in ins)) for e in range(ins[0].shape[0])]
    return _REF[key]


def check_against_oracle(key, net, ins, out):
    vm, va, it, cv = out
    ref = reference(key, net, ins)
    worst, n_unconv = 0.0, 0
    for e, (r, agrees) in enumerate(ref):
        assert agrees(it[e], cv[e]), (key, e, it[e], cv[e], r.iterations, r.converged)
        n_unconv += not r.converged
        if r.converged:
            v = vm[e] * np.exp(1j * np.radians(va[e]))
            worst = max(worst, np.abs(v - r.V).max())
            assert np.abs(vm[e][net.gen_bus] - net.gen_vm_pu).max() <= V_TOL, (key, e)
    assert worst <= V_TOL, (key, worst)
    return n_unconv


# ---- 1. solve parity ----------------------------------------------------------------------------------------------------------------
CASES = [(n, s) for n in RADIAL for s in ("tree", "sparse")] + [("meshed", "auto")]


@pytest.mark.parametrize("name,solver", CASES)
def test_solve_with_gens_matches_runpp(name, solver):
    net, prof = gen_case(name)
    B = 48
    ins = inputs(net, prof, B, 5)
    out, g = solve(net, prof, B, dict(nr_solver=solver), ins)
    assert g["solver"] == {"tree": 0, "sparse": 1, "auto": 1}[solver]
    n_unconv = check_against_oracle((name, 5, B, "flat"), net, ins, out)
    if name == "far":                                           # a condition on the INPUTS: late and never-converging envs in one wavefront
        assert n_unconv == 13, n_unconv
        its = sorted({r.iterations for r, _ in reference((name, 5, B, "flat"), net, ins) if r.converged})
        assert its[0] >= 5 and its[-1] <= 9, its
    else:
        assert n_unconv == 0, n_unconv
    # what each net probes, as a condition on the inputs: envs of one wavefront that stop at different sweeps
    its = np.array([r.iterations for r, _ in reference((name, 5, B, "flat"), net, ins)])
    want = dict(leaf={3: 11, 4: 37}, mixed={4: 48}, c141={4: 40, 5: 8}).get(name)
    if want:
        assert {int(k): int((its == k).sum()) for k in np.unique(its)} == want


@pytest.mark.parametrize("B", [3, 17, 33])
@pytest.mark.parametrize("solver", ["tree", "sparse"])
def test_solve_on_mixed_at_odd_batch_sizes(B, solver):
    net, prof = gen_case("mixed")
    ins = inputs(net, prof, B, 5)
    out, _ = solve(net, prof, B, dict(nr_solver=solver), ins)
    assert check_against_oracle(("mixed", 5, B, "flat"), net, ins, out) == 0


@pytest.mark.parametrize("n_bus", [2, 3])
@pytest.mark.parametrize("solver", ["tree", "sparse"])
def test_tiny_chains(n_bus, solver):
    net, prof = tiny_case(n_bus)
    B = 48
    ins = inputs(net, prof, B, 1)
    out, _ = solve(net, prof, B, dict(nr_solver=solver), ins)
    assert check_against_oracle((f"tiny{n_bus}", 1, B, "flat"), net, ins, out) == 0 and out[3].all()


# ---- 2. the DC start ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["leaf", "c141"])
@pytest.mark.parametrize("solver", ["tree", "sparse"])
def test_gens_with_the_dc_start_match_runpp(name, solver):
    net, prof = gen_case(name)
    net = hv_front(net, 150.0)
    assert net.va_init == "dc" and net.has_gens
    B = 48
    ins = inputs(net, prof, B, 7)
    out, g = solve(net, prof, B, dict(nr_solver=solver), ins)
    assert g["nr_init"] == 2
    assert check_against_oracle((name + "_hv", 7, B, "dc"), net, ins, out) == 0


# ---- 3. every compiled GEN instantiation: tests/kernel_matrix.py has a row per kernel, tests/test_kernel_matrix_gpu.py holds each to the oracle
def test_a_gen_geometry_that_is_not_compiled_is_refused():
    net, prof = gen_case("mixed")
    with pytest.raises(RuntimeError, match="not compiled in"):
        make_env(net, prof, 16, dict(nr_waves=1, nr_lanes=32))


# ---- 4. Q_gen and the commit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "all", "c141"])
@pytest.mark.parametrize("solver", ["tree", "sparse"])
def test_q_gen_and_the_commit_after_a_step(name, solver):
    """reset plus one step.  The step's solve uses the loads and pv the env holds BEFORE the call (the profile rows advance after the
    commit) and the q the call's actions set, read back afterwards: with them QD and runpp_gen's replay of the step are formed.
    (i) at the kernel's own committed V: res_bus.q = -Im(V conj(Ybus V)) sn and Q_gen = Im(V conj(Ybus V)) sn + QD, i.e.
        res_bus.q + Q_gen = QD, each within 4 (m + 2) 2^-52 sn sum_j |V_k| |Y_kj| |V_j|;
    (ii) against runpp_gen: (i) plus the first-order propagation of the measured voltage difference."""
    check_q_gen_and_the_commit(*gen_case(name), solver, name)


def check_q_gen_and_the_commit(net, prof, solver, name, B=6):
    """the body of the test above on any net with generators"""
    env = make_env(net, prof, B, dict(nr_solver=solver))
    try:
        env.reset()
        lp, lq = (x.cpu().numpy().copy() for x in env.loads())
        pv = env.results(("sgen_p",))["sgen_p"].cpu().numpy().copy()
        act = np.random.default_rng(4).uniform(-0.8, 0.8, (B, net.n_sgen))
        r, term, info = env.step(torch.as_tensor(act, device=DEV))
        assert not term.any()
        res = {k: v.cpu().numpy() for k, v in env.results().items()}
        rg = {k: v.cpu().numpy() for k, v in env.res_gen().items()}
        ybus = _cached_ybus(net)[0]
        gb = net.gen_bus
        sh_q = np.zeros(net.n_bus)
        if net.shunt_bus.shape[0]:
            np.add.at(sh_q, net.shunt_bus, net.shunt_q_mvar)
        for e in range(B):
            x = (lp[e], lq[e], pv[e], res["sgen_q"][e])
            V = res["vm_pu"][e] * np.exp(1j * np.radians(res["va_degree"][e]))
            s = V * np.conj(ybus @ V) * net.sn_mva
            assert np.array_equal(rg["p_mw"][e], net.gen_p_mw * net.gen_scaling)          # exact
            assert np.array_equal(rg["vm_pu"][e], res["vm_pu"][e][gb]) and np.array_equal(rg["va_degree"][e], res["va_degree"][e][gb])
            assert np.abs(res["vm_pu"][e][gb] - net.gen_vm_pu).max() <= V_TOL
            ref = runpp_gen(net, *x)
            assert ref.converged and np.abs(V - ref.V).max() <= V_TOL
            bar_i, prop = q_bars(net, V, ref.V)
            qd = (bus_demand(net, *x)[1] + sh_q * res["vm_pu"][e] ** 2)[gb]
            gap_bus = np.abs(res["q_mvar"][e][gb] + s.imag[gb])
            gap_gen = np.abs(rg["q_mvar"][e] - (s.imag[gb] + qd))
            gap_sum = np.abs(res["q_mvar"][e][gb] + rg["q_mvar"][e] - qd)
            gap_ref = np.abs(rg["q_mvar"][e] - ref.res_gen["q_mvar"])
            print(f"\n[gen commit] {name}/{solver} env {e}: / bar (i): res_bus.q {np.max(gap_bus / bar_i):.3f} Q_gen {np.max(gap_gen / bar_i):.3f} "
                  f"sum {np.max(gap_sum / bar_i):.3f}; Q_gen / bar (ii) {np.max(gap_ref / (bar_i + prop)):.3f}")
            assert np.all(gap_bus <= bar_i) and np.all(gap_gen <= bar_i) and np.all(gap_sum <= bar_i), (e, gap_bus, gap_gen, gap_sum, bar_i)
            assert np.all(gap_ref <= bar_i + prop), (e, gap_ref, bar_i + prop)
            assert np.all(np.abs(res["q_mvar"][e][gb] - ref.q_mvar[gb]) <= bar_i + prop)
            # rule 4 on P: res_bus.p = loads - sgens - P_gen (+ shunt), exact in the inputs up to the roundings of the sum (test_zip bars)
            assert np.all(np.abs(res["p_mw"][e] - ref.p_mw)[gb] <= 1e-9 * np.maximum(1.0, np.abs(ref.p_mw))[gb])
            other = np.setdiff1d(np.arange(net.n_bus), gb)
            for k in ("p_mw", "q_mvar"):
                assert np.all(np.abs(ref[k] - res[k][e])[other] <= 1e-9 * np.maximum(1.0, np.abs(ref[k]))[other]), (e, k)
    finally:
        env.close()


@pytest.mark.parametrize("name", ["mixed", "all", "c141"])
def test_q_gen_against_runpp_gen_on_explicit_inputs(name):
    """manual_reset puts every env on a known profile row without noise: the committed state is runpp_gen's on that row with the reset
    action's q, read back from the env (sgen_q).  Bar (ii) = (i) + the first-order propagation of the measured voltage difference."""
    net, prof = gen_case(name)
    B = 4
    env = make_env(net, prof, B)
    try:
        env.manual_reset(0, 11, 3)
        row = prof.start_row(0, 11, 3) + 1
        res = {k: v.cpu().numpy() for k, v in env.results().items()}
        rg = {k: v.cpu().numpy() for k, v in env.res_gen().items()}
        gb = net.gen_bus
        for e in range(B):
            x = (prof.load_p[row], prof.load_q[row], res["sgen_p"][e], res["sgen_q"][e])
            assert np.array_equal(res["sgen_p"][e], prof.pv[row])
            r = runpp_gen(net, *x)
            assert r.converged
            V = res["vm_pu"][e] * np.exp(1j * np.radians(res["va_degree"][e]))
            assert np.abs(V - r.V).max() <= V_TOL
            bar_i, prop = q_bars(net, V, r.V)
            bar = bar_i + prop
            gap = np.abs(rg["q_mvar"][e] - r.res_gen["q_mvar"])
            print(f"\n[gen commit] {name} env {e}: Q_gen gap / bar (ii) max {np.max(gap / bar):.3f}; gap max {gap.max():.2e}")
            assert np.all(gap <= bar), (e, gap, bar)
            # every other res_bus entry: the bars of tests/test_zip_loads_gpu.py (res_bus.q of a gen bus: bar (ii) without the QD part)
            other = np.setdiff1d(np.arange(net.n_bus), gb)
            for k in ("p_mw", "q_mvar"):
                assert np.all(np.abs(r[k] - res[k][e])[other] <= 1e-9 * np.maximum(1.0, np.abs(r[k]))[other]), (e, k)
            assert np.all(np.abs(r.p_mw - res["p_mw"][e])[gb] <= 1e-9 * np.maximum(1.0, np.abs(r.p_mw))[gb])
            assert np.all(np.abs(r.q_mvar - res["q_mvar"][e])[gb] <= bar_i + prop)
            assert np.abs(r.vm_pu - res["vm_pu"][e]).max() <= V_TOL
    finally:
        env.close()


# ---- 5. an episode ----------------------------------------------------------------------------------------------------------------------
def substation_case():
    pnet = gen_substation()
    net = from_pandapower(pnet, gens="runpp")
    prof = flat_profiles(net, pnet.load["p_mw"].to_numpy(), pnet.load["q_mvar"].to_numpy(), pnet.sgen["p_mw"].to_numpy(), T=480 * 3)
    return net, prof


def test_auto_reset_episode_with_a_gen_matches_the_oracle_env(monkeypatch):
    """VoltageControlBatch on a net converted with gens="runpp": reset, steps with an unsolvable action and auto-reset; rewards,
    terminated, info, obs, state, res_bus and res_gen per step against VoltageControlOracle on runpp_gen"""
    monkeypatch.setattr(env_restated, "runpp_restated", runpp_gen)
    net, prof = substation_case()
    assert net.n_gen == 1 and net.start_vm_pu != net.ext_grid_vm_pu
    B, limit = 3, 6
    env = make_env(net, prof, B, episode_limit=limit, auto_reset=True)
    oracles = [VoltageControlOracle(net, prof, dict(ARGS, episode_limit=limit), env_id=e, do_reset=False) for e in range(B)]
    obs, _ = env.reset()
    for e, o in enumerate(oracles):
        oo, _ = o.reset()
        assert np.abs(np.array(oo) - obs[e].cpu().numpy()).max() < 1e-9
    gb = net.gen_bus
    kind, idx = env.obs_index()
    q_cols = np.isin(kind, (2,)) & np.isin(idx, gb)            # obs entries that are a gen bus's q_mvar
    nb = net.n_bus
    state_q = np.zeros(env.state_size, bool); state_q[nb + gb] = True      # get_state: p [nb] | q [nb] | ...
    pending, n_term = [False] * B, [0] * B
    arng = np.random.default_rng(17)
    for t in range(2 * limit + 3):
        act = arng.uniform(-0.8, 0.8, (B, net.n_sgen))
        if t == 2:
            act[1] = 60.0                                       # env 1: an unsolvable power flow -> terminates early
        before = {k: v.cpu().numpy().copy() for k, v in env.res_gen().items()}
        r, term, info = env.step(torch.as_tensor(act, device=DEV))
        obs = env.get_obs().cpu().numpy()
        state = env.get_state().cpu().numpy()
        res = {k: v.cpu().numpy() for k, v in env.results(["vm_pu", "va_degree", "p_mw", "q_mvar"]).items()}
        rg = {k: v.cpu().numpy() for k, v in env.res_gen().items()}
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
            V = res["vm_pu"][e] * np.exp(1j * np.radians(res["va_degree"][e]))
            bar_i, prop = q_bars(net, V, o.res.V)
            qbar = np.zeros(nb); qbar[gb] = bar_i + prop           # bar (ii), per gen bus
            other = np.setdiff1d(np.arange(nb), gb)
            for k in ("p_mw", "q_mvar"):
                assert np.all(np.abs(o.res[k] - res[k][e])[other] <= 1e-9 * np.maximum(1.0, np.abs(o.res[k]))[other]), (t, e, k)
            assert np.all(np.abs(o.res.p_mw - res["p_mw"][e])[gb] <= 1e-9 * np.maximum(1.0, np.abs(o.res.p_mw))[gb])
            assert np.all(np.abs(o.res.q_mvar - res["q_mvar"][e])[gb] <= qbar[gb]), (t, e, np.abs(o.res.q_mvar - res["q_mvar"][e])[gb], qbar[gb])
            assert np.all(np.abs(o.res.res_gen["q_mvar"] - rg["q_mvar"][e]) <= qbar[gb]), (t, e)
            do, ds = np.abs(np.array(o.get_obs()) - obs[e]), np.abs(np.array(o.get_state()) - state[e])
            assert do[~q_cols].max() < 1e-9 and np.all(do[q_cols] <= qbar[idx[q_cols]]), (t, e, do[q_cols], qbar[idx[q_cols]])
            assert ds[~state_q].max() < 1e-9 and np.all(ds[state_q] <= qbar[gb]), (t, e, ds[state_q], qbar[gb])
            if to:
                pending[e] = True
                n_term[e] += 1
                if t == 2 and e == 1:                           # the rollback: res_gen is the previous committed state's
                    assert all(np.array_equal(before[k][e], rg[k][e]) for k in rg)
    assert n_term[1] >= 1
    env.close()


def test_single_env_class_reports_res_gen(monkeypatch):
    monkeypatch.setattr(env_restated, "runpp_restated", runpp_gen)
    net, prof = gen_case("mixed")
    env = VoltageControl(dict(ARGS, net=net, profiles=prof), device=DEV)
    oracle = VoltageControlOracle(net, prof, ARGS, env_id=0, do_reset=False)
    oracle.draw = 1                                             # the constructor's reset consumed draw 0 (voltage_control_env.py:85)
    env.reset()
    oracle.reset()
    act = np.random.default_rng(2).uniform(-0.8, 0.8, net.n_sgen)
    r, term, info = env.step(act)
    ro, to, io = oracle.step(act)
    assert abs(r - ro) < 1e-9 and bool(term) == bool(to)
    rg = env._get_res_gen()
    assert set(rg) == {"p_mw", "q_mvar", "vm_pu", "va_degree"} and all(v.shape == (1, net.n_gen) for v in rg.values())
    assert np.abs(rg["q_mvar"][0].cpu().numpy() - oracle.res.res_gen["q_mvar"]).max() < 1e-7
    assert np.abs(np.asarray(env._get_res_bus_v()) - oracle.res.vm_pu).max() < V_TOL
    env.close()


# ---- 6. the three injection paths -------------------------------------------------------------------------------------------------------
def snapshot(env):
    out = [env.get_obs().clone(), env.get_state().clone()]
    out += [v.clone() for v in env.results().values()] + [v.clone() for v in env.res_gen().values()]
    return out


def run_pair(net, prof, a, b, n_calls, forced, solve_at):
    B = a.n_envs
    oa, sa = a.reset(); ob, sb = b.reset()
    assert torch.equal(oa, ob) and torch.equal(sa, sb)
    gen = torch.Generator(device=DEV); gen.manual_seed(23)
    rng = np.random.default_rng(2)
    n_restarts = 0
    for t in range(n_calls):
        act = (torch.rand(B, net.n_sgen, device=DEV, generator=gen, dtype=torch.float64) * 2 - 1) * 0.8
        if t == forced:                                         # (with a gen on every bus no q is unsolvable: Q is free everywhere)
            act[11] = 60.0
        if t == solve_at:                                       # a solve on explicit inputs in between: Sbus no longer reflects the stored loads
            ins = inputs(net, prof, B, int(rng.integers(1 << 30)))
            assert all(torch.equal(u, v) for u, v in zip(a.solve(*ins), b.solve(*ins)))
        ra, ta, ia = a.step(act); rb, tb, ib = b.step(act)
        assert torch.equal(ra, rb) and torch.equal(ta, tb) and torch.equal(ia, ib), t
        n_restarts += int(a.auto_reset_mask().sum().item())
        assert all(torch.equal(u, v) for u, v in zip(snapshot(a), snapshot(b))), t
    return n_restarts


def test_the_three_injection_paths_agree_bit_for_bit_with_a_gen_on_every_bus():
    """`all`: a gen on every non-slack bus, sharing buses with the six sgens.  k_inject_sgen + k_advance's stores against the all-bus
    k_inject (inject_full = 1) with auto_reset; the prologue of k_nr_tree (fuse_inject = 1) against k_inject_sgen (fuse_inject = 2)"""
    net, prof = gen_case("all")
    B = 70
    a, b = make_env(net, prof, B, auto_reset=True, episode_limit=4), make_env(net, prof, B, dict(inject_full=1), auto_reset=True, episode_limit=4)
    assert run_pair(net, prof, a, b, 9, forced=1, solve_at=5) >= 2 * B         # every env restarts at the episode limit, twice
    a.close(); b.close()
    a, b = make_env(net, prof, B, dict(fuse_inject=1)), make_env(net, prof, B, dict(fuse_inject=2))
    assert a.geometry()["fuse_inject"] == 1 and b.geometry()["fuse_inject"] == 0
    run_pair(net, prof, a, b, 6, forced=1, solve_at=2)
    a.close(); b.close()


# ---- 7. evaluate_actions, res_line ------------------------------------------------------------------------------------------------------
def test_evaluate_actions_and_res_line_on_a_handle_with_gens():
    from tests import branch_ref
    from tests.test_whatif_gpu import STEP_TOL
    net, prof = gen_case("mixed")
    B, K = 9, 2
    env = make_env(net, prof, B)
    try:
        env.reset()
        cand = np.random.default_rng(8).uniform(-0.8, 0.8, (B, K, net.n_sgen))
        reward, info, st, it = (x.cpu().numpy() for x in env.evaluate_actions(torch.as_tensor(cand, device=DEV)))
        assert (st == 0).all()
        r, term, inf = env.step(torch.as_tensor(cand[:, 1], device=DEV))
        dr, di = np.abs(r.cpu().numpy() - reward[:, 1]), np.abs(inf.cpu().numpy() - info[:, 1])
        print(f"\n[gen whatif] reward {dr.max():.3e} info {di.max():.3e}")
        assert dr.max() <= STEP_TOL and di.max() <= STEP_TOL
        res = {k: v.cpu().numpy() for k, v in env.results(("vm_pu", "va_degree")).items()}
        keys = ("p_from_mw", "q_from_mvar", "p_to_mw", "q_to_mvar", "pl_mw", "ql_mvar", "i_from_ka", "i_to_ka", "i_ka")
        got = {k: v.cpu().numpy() for k, v in env.res_line(keys).items()}
        # tests/branch_ref.py: every column within its bar (16 x e64, never below 64 ulp) of the extended reference at the committed voltages
        err = branch_ref.errors(net, res["vm_pu"], res["va_degree"], got, {})[0]
        bar = branch_ref.bars(net, res["vm_pu"], res["va_degree"])[0]
        for k in keys:
            assert err[k] <= bar[k], (k, err[k], bar[k])
        assert abs(float(got["pl_mw"].sum(1)[0]) - float(env.results(("pl_mw",))["pl_mw"].sum(1)[0])) < 1e-9
        mx, wb, no = env.loading_summary()
        assert mx.shape == (B,)
    finally:
        env.close()


# ---- 8. refusals; explicit empty columns ------------------------------------------------------------------------------------------------
def test_refusals_by_name():
    net, prof = gen_case("mixed")
    with pytest.raises(RuntimeError, match="dense"):
        make_env(net, prof, 16, dict(nr_solver="dense"))
    env = make_env(net, prof, 16)
    try:
        env.reset()
        with pytest.raises(RuntimeError, match="droop_actions: nets with generators"):
            env.droop_actions()
        with pytest.raises(RuntimeError, match="opf_actions: nets with generators"):
            env.opf_actions()
    finally:
        env.close()


def test_explicit_empty_gen_columns_are_the_path_of_before(monkeypatch):
    """n_gen = 0 with real (non-NULL) column pointers and vm_init_pu = the ext_grid set-point: bit-identical outputs over a short episode"""
    from mapdn_amd.netspec import make_case
    net, prof = make_case("case141")
    B = 32

    def run():
        env = make_env(net, prof, B)
        assert env.n_gen == 0
        obs, _ = env.reset()
        outs = [obs.cpu().numpy().copy()]
        rng = np.random.default_rng(3)
        for _ in range(3):
            r, term, info = env.step(torch.as_tensor(rng.uniform(-0.8, 0.8, (B, net.n_sgen)), device=DEV))
            outs += [r.cpu().numpy().copy(), term.cpu().numpy().copy(), info.cpu().numpy().copy(), env.get_obs().cpu().numpy().copy()]
            outs += [v.cpu().numpy().copy() for v in env.results().values()]
        assert all(v.shape == (B, 0) for v in env.res_gen().values())
        k = env.nr_kernel()
        env.close()
        return outs, k
    a, ka = run()
    orig = _lib.make_cnetspec
    dummy_i, dummy_d = np.zeros(1, np.int32), np.ones(1)

    def explicit(n):
        s, keep = orig(n)
        s.gen_bus = _lib._p(dummy_i, _lib._pi)
        s.gen_p_mw = s.gen_vm_pu = s.gen_scaling = _lib._p(dummy_d, _lib._pd)
        s.vm_init_pu = float(n.ext_grid_vm_pu)
        return s, keep
    monkeypatch.setattr(_lib, "make_cnetspec", explicit)
    b, kb = run()
    assert ka == kb and all(np.array_equal(x, y) for x, y in zip(a, b))
