"""GPU (-m gpu): the droop baseline (mapdn_droop_actions: k_droop_update in csrc/droop.hip, ctl_pv_row / ctl_mlo_rows / ctl_next_solve in
csrc/ctlloop.hpp, ctl_drive / droop_run in csrc/baselines_host.hpp) at the edges of its loop, its law and its frame, on the nets and
configs of tests/droop_edge_cases.py; tests/test_droop_edges_cpu.py asserts of the reference alone what these tests rely on.

Bars: actions and |V| to TOL = 1e-9 (the bar of tests/test_droop_gpu.py) against tests/droop_ref.py on the oracle's power flow; status exact;
iterations exact save the documented tie (a count that differs by one with dists[k - 1] within 1e-8 of v_tol).  On `collapse` only the
decidable envs (droop_edge_cases.robust) are compared with the reference; the rest is counted, capped at a quarter of the batch as the
CPU file caps it, and held to what needs no reference (a failed env returns the walk's action of its last solved point and NaN voltages).
Everything that compares two GPU runs is bit for bit.

MEASURED: worst |gpu - reference| per case as seen on an MI355X, with the envs compared and left out; DESIGN.md section 23 has the table.
No bound comes from them."""
import numpy as np
import pytest
import torch

from mapdn_amd.env import VoltageControlBatch
from tests import droop_edge_cases as D
from tests import element_edge_nets as N
from tests.baseline_contract import env_state, same, snapshot
from tests.droop_ref import droop_ref, resolve

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-9
MEASURED = {}
EDGE_NETS = [n for n in D.NETS if n != "collapse"]
CROWDED = [n for n in D.NETS if n.startswith("crowded")]


def make_env(name, B, env_id_offset=0, **args):
    net, prof = D.make(name)
    return VoltageControlBatch(net, prof, dict(D.ARGS, **args), n_envs=B, device=DEV, obs_dtype=torch.float64, env_id_offset=env_id_offset)


def droop(env, cfg=None, vm_pu=True):
    out = env.droop_actions(cfg, vm_pu=vm_pu)
    return tuple(x.cpu().numpy() for x in out)


def same_bits(x, y, where, rows=None):
    for u, v in zip(x, y):
        if rows is not None:
            u, v = u[rows], v[rows]
        assert np.array_equal(u, v, equal_nan=True), where


def note(case, B, worst, compared, left_out=0, failed_compared=0):
    k = (case, B)
    w, c, l, f = MEASURED.get(k, (0.0, 0, 0, 0))
    MEASURED[k] = (max(w, worst), c + compared, l + left_out, f + failed_compared)
    print(f"\n[droop edges] {case} B={B}: worst={worst:.2e} compared={compared} left_out={left_out} status2_compared={failed_compared}")


def compare(case, out, refs, cfg=None, decidable=None):
    """out = (a, it, st, vm) of the GPU against refs[e] (DroopResult); decidable[e] False: the env is counted, not compared"""
    a, it, st, vm = out
    c = resolve(cfg)
    worst, compared, left, failed = 0.0, 0, 0, 0
    for e, r in enumerate(refs):
        w = (case, e, int(st[e]), r.status, int(it[e]), r.iterations)
        if decidable is not None and not decidable[e]:
            left += 1
            assert st[e] in (0, 1, 2) and 1 <= it[e] <= c["max_iter"], w
            if st[e] == 2:                                     # what needs no reference: the walk's action of the last solved point, no voltages
                assert np.isnan(vm[e]).all() and np.array_equal(a[e], np.full(a.shape[1], -(1.0 - 0.5 ** (int(it[e]) - 2)))), w
            else:
                assert np.isfinite(vm[e]).all(), w
            continue
        assert st[e] == r.status, w
        if it[e] != r.iterations:
            k = min(int(it[e]), r.iterations)
            assert abs(int(it[e]) - r.iterations) == 1 and abs(r.dists[k - 1] - c["v_tol"]) <= 1e-8, w
            left += 1
            continue
        compared += 1
        worst = max(worst, float(np.abs(a[e] - r.actions).max()))
        if r.status in (0, 1):
            assert np.isfinite(vm[e]).all(), w
            worst = max(worst, float(np.abs(vm[e] - r.vm_pu).max()))
        else:
            failed += 1
            assert np.isnan(vm[e]).all(), w
    assert worst < TOL, (case, worst)
    return worst, compared, left, failed


def refs_of(name, env, cfg=None, envs=None):
    net, _ = D.make(name)
    lp, lq, pv, smax = env_state(env)
    return [droop_ref(net, lp[e], lq[e], pv[e], smax, cfg, D.runpp_for(name)) for e in (range(env.n_envs) if envs is None else envs)]


def parity(case, name, env, cfg=None):
    out = droop(env, cfg)
    refs = refs_of(name, env, cfg)
    assert all(r.status <= 1 for r in refs), case
    worst, compared, left, _ = compare(case, out, refs, cfg)
    assert left <= 2 and compared >= env.n_envs - 2, (case, left)
    note(case, env.n_envs, worst, compared, left)
    return out


def ext_sgen(net):
    alias = np.asarray(net.bus_alias)
    j = np.flatnonzero(alias[net.sgen_bus] == alias[net.ext_grid_bus])
    assert j.size == 1
    return int(j[0])


# ---- parity on every edge net -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["reset", "stepped", "noon"])
@pytest.mark.parametrize("name", EDGE_NETS)
def test_parity_on_the_edge_nets(name, state):
    """B = 17 (a full workgroup and one lane of a second): after a noisy reset(), after one droop-driven step, at noon rows; the defaults
    and a deadband config whose max_iter is reached"""
    B = D.B_PARITY
    env = make_env(name, B)
    try:
        assert env.nr_kernel()["solver"] == (1 if name == "crowded_meshed" else 0)
        if state == "noon":
            env.reset(start_rows=torch.tensor(D.noon_rows(name, B)))
        else:
            env.reset()
        if state == "stepped":
            a, it, st = env.droop_actions()
            assert (st <= 1).all()
            _, term, _ = env.step(a)
            assert not bool(term.any())
        a, it, st, vm = parity(f"{name}/{state}/defaults", name, env)
        assert (it >= 2).all()
        parity(f"{name}/{state}/deadband", name, env, D.DEADBAND)
        assert env.stats()["reset_failures"] == 0
    finally:
        env.close()


VROOT = 1.0
EXT_CFGS = dict(first_branch=dict(va=VROOT, vb=1.02, vc=1.03, vd=1.05, max_iter=9),       # v == va: +1 by the first branch
                slope_end=dict(va=0.9, vb=0.95, vc=0.97, vd=VROOT, max_iter=9),           # v == vd: the falling slope's end, exactly -1
                deadband=dict(max_iter=9))                                                # vb == v == vc: the closed deadband, 0


@pytest.mark.parametrize("which", list(EXT_CFGS))
@pytest.mark.parametrize("name", CROWDED)
def test_the_ext_grid_sgen_bit_for_bit(name, which):
    """the sgen on the ext_grid bus: no power flow reads its action (k < d.n) and its |V| is the slack's constant row, so its action is
    the damped walk towards f(vroot) min(1, ratio s_max / lim), bit for bit the reference's"""
    net, _ = D.make(name)
    assert net.ext_grid_vm_pu == VROOT
    j = ext_sgen(net)
    cfg = EXT_CFGS[which]
    f = dict(first_branch=1.0, slope_end=-1.0, deadband=0.0)[which]
    B = D.B_PARITY
    env = make_env(name, B)
    try:
        env.reset(start_rows=torch.tensor(D.noon_rows(name, B)))
        out = droop(env, cfg)
        refs = refs_of(name, env, cfg)
        worst, compared, left, _ = compare(f"{name}/ext/{which}", out, refs, cfg)
        a, it, st, vm = out
        n = 0
        for e, r in enumerate(refs):
            assert vm[e, net.ext_grid_bus] == VROOT
            if it[e] == r.iterations:
                n += 1
                assert a[e, j] == r.actions[j] and np.signbit(a[e, j]) == np.signbit(r.actions[j]), (name, which, e, a[e, j], r.actions[j])
                assert (a[e, j] > 0.0) if f > 0 else (a[e, j] < 0.0) if f < 0 else a[e, j] == 0.0
        assert n >= B - 2
        note(f"{name}/ext/{which}", B, worst, compared, left)
    finally:
        env.close()


# ---- collapse -----------------------------------------------------------------------------------------------------------------------
def collapse_env(B=D.B_COLLAPSE, env_id_offset=0, first=0, **args):
    env = make_env("collapse", B, env_id_offset=env_id_offset, **args)
    env.reset(start_rows=torch.tensor(D.night_rows("collapse", D.B_COLLAPSE)[first:first + B]))
    return env


def test_collapse_against_the_reference():
    """status 2 beside 0 and 1 inside one workgroup: statuses, iterations, a_sol and the NaN rows against the reference on the oracle's
    own states (the env's loads agree with them to 1e-12, asserted), with solver timing on: the solve launches stay within the early-exit
    bound"""
    B = D.B_COLLAPSE
    res = D.collapse_reference(B)
    refs, dec = [r for r, _ in res], [d for _, d in res]
    states = D.oracle_states("collapse", B, D.night_rows("collapse", B))
    env = collapse_env()
    try:
        lp, lq, pv, smax = env_state(env)
        for e, s in enumerate(states):
            assert np.abs(lp[e] - s[0]).max() < 1e-11 and np.abs(lq[e] - s[1]).max() < 1e-11 and np.abs(pv[e] - s[2]).max() < 1e-11
            assert np.array_equal(smax, s[3])
        env.nr_timing(True)
        env.nr_time_ms()
        out = droop(env, D.COLLAPSE_CFG)
        _, launches = env.nr_time_ms()
        env.nr_timing(False)
        a, it, st, vm = out
        m = int(it.max())
        assert m <= launches <= m + 3, (m, launches)
        worst, compared, left, failed = compare("collapse", out, refs, D.COLLAPSE_CFG, dec)
        assert failed >= 3 and left <= B // 4, (failed, left)
        assert set(st.tolist()) == {0, 1, 2}
        ok = st <= 1
        assert np.isfinite(vm[ok]).all() and np.isnan(vm[~ok]).all()       # finite exactly on status 0 / 1
        assert (np.abs(a[st == 2]) > 0.0).all() and (it[st == 2] >= 2).all()
        note("collapse", B, worst, compared, left, failed)
    finally:
        env.close()


def test_collapse_leaves_the_state_and_the_step_alone():
    A, T = collapse_env(), collapse_env()
    try:
        before = snapshot(A)
        a, it, st, vm = A.droop_actions(D.COLLAPSE_CFG, vm_pu=True)
        assert set(st.cpu().tolist()) == {0, 1, 2}
        same(before, snapshot(A))
        same(before, snapshot(T))
        r1, t1, i1 = [x.clone() for x in A.step(a)]
        r2, t2, i2 = [x.clone() for x in T.step(a)]
        assert torch.equal(r1, r2) and torch.equal(t1, t2) and torch.equal(i1, i2) and not bool(t1.any())    # a_sol is solvable
        assert torch.equal(A.get_obs(), T.get_obs())
        ok = st <= 1
        committed = A.results(("vm_pu",))["vm_pu"]
        assert float((committed[ok] - vm[ok]).abs().max()) < 1e-12
        same(snapshot(A), snapshot(T))
    finally:
        A.close(); T.close()


# ---- all four statuses in one handle ------------------------------------------------------------------------------------------------
def _stop_env_7(env, twin, acts):
    """step both; `env` gets the unsolvable action at env 7, `twin` a plain one: every other env has the same state in both"""
    bad, plain = acts.clone(), acts.clone()
    bad[N.FORCED_ENV] = N.UNSOLVABLE
    plain[N.FORCED_ENV] = 0.0
    _, t1, _ = env.step(bad)
    _, t2, _ = twin.step(plain)
    t1 = t1.cpu().numpy()
    assert t1[N.FORCED_ENV] and t1.sum() == 1 and not bool(t2.any())


def check_stopped_beside_running(out, ref_out, B):
    a, it, st, vm = out
    e7 = N.FORCED_ENV
    assert st[e7] == 3 and (a[e7] == 0.0).all() and it[e7] == 0 and np.isnan(vm[e7]).all()
    rest = np.arange(B) != e7
    assert (st[rest] <= 2).all() and (it[rest] >= 1).all()
    same_bits(out, ref_out, "beside the stopped env", rest)


def test_a_stopped_env_beside_running_ones_on_crowded():
    """the frozen plan's forced env (element_edge_nets): env 7 terminates on an unsolvable step, its neighbours go on"""
    B = D.B_PARITY
    acts = torch.as_tensor(N.actions("crowded", "frozen", B).astype(np.float64), device=DEV)
    env, twin = make_env("crowded", B), make_env("crowded", B)
    try:
        env.reset(); twin.reset()
        for x in (env, twin):
            x.step(acts[0])
        _stop_env_7(env, twin, acts[1])
        out, ref_out = droop(env), droop(twin)
        check_stopped_beside_running(out, ref_out, B)
        assert (out[2][np.arange(B) != N.FORCED_ENV] <= 1).all()
    finally:
        env.close(); twin.close()


def test_all_four_statuses_in_one_call_on_collapse():
    """one step (no reactive power; env 7 unsolvable) into the night, then the collapse config: 0, 1, 2 and 3 in one call, and every
    env but the stopped one bit-identical to a handle on which env 7 ran"""
    B = D.B_COLLAPSE
    env, twin = collapse_env(), collapse_env()
    try:
        _stop_env_7(env, twin, torch.zeros(B, env.n_sgen, dtype=torch.float64, device=DEV))
        out, ref_out = droop(env, D.COLLAPSE_CFG), droop(twin, D.COLLAPSE_CFG)
        check_stopped_beside_running(out, ref_out, B)
        assert set(out[2].tolist()) == {0, 1, 2, 3}
        g = out[2][:16]
        assert (g == 2).any() and (g <= 1).any() and (g == 3).any()          # all inside the first workgroup
    finally:
        env.close(); twin.close()


# ---- batch edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["crowded", "collapse"])
def test_env_e_has_the_same_bits_in_every_batch(name):
    """B = 1, 15, 16, 17, 33 from the same start rows: t.valid lanes in the last workgroup, the ballot that counts n_active, vm_out rows of
    the last env; and envs 14 .. 18 on a handle of their own (env_id_offset 14), across the workgroup edge of the batch of 33"""
    cfg = D.COLLAPSE_CFG if name == "collapse" else None
    rows = (D.night_rows if name == "collapse" else D.noon_rows)(name, D.B_COLLAPSE)

    def run(B, first=0):
        env = make_env(name, B, env_id_offset=first)
        try:
            env.reset(start_rows=torch.tensor(rows[first:first + B]))
            return droop(env, cfg)
        finally:
            env.close()
    full = run(D.B_COLLAPSE)
    assert set(full[2].tolist()) == ({0, 1, 2} if name == "collapse" else {0})
    for B in D.BATCHES[:-1]:
        out = run(B)
        for x, y in zip(full, out):
            assert x[:B].shape == y.shape and np.array_equal(x[:B], y, equal_nan=True), (name, B)
    edge = run(5, first=14)
    for x, y in zip(full, edge):
        assert np.array_equal(x[14:19], y, equal_nan=True), name


# ---- config and driver edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["crowded", "one_sgen"])
def test_one_solve_and_a_first_solve_that_converges(name):
    """max_iter = 1: every env stops at the first solve with status 1 and the start's action, exactly 0, and |V| of a plain solve at q = 0;
    v_tol = 1e4: the first solve already converges (||v - 100|| < 1e4).  A droop call after the solve() (Sbus stale: ctl_begin rebuilds
    it) has the bits of the call before it."""
    B = D.B_PARITY
    env = make_env(name, B)
    try:
        env.reset()
        lp, lq, pv, _ = env_state(env)
        a, it, st, vm = one = droop(env, dict(max_iter=1))
        assert (st == 1).all() and (it == 1).all() and (a == 0.0).all() and not np.signbit(a).any()
        b = droop(env, dict(v_tol=1e4))
        assert (b[2] == 0).all() and (b[1] == 1).all() and (b[0] == 0.0).all()
        assert np.array_equal(b[3], vm)
        vs, _, _, cv = env.solve(lp, lq, pv, np.zeros_like(pv))
        assert bool(cv.all())
        gap = float(np.abs(vs.cpu().numpy() - vm).max())
        print(f"\n[droop edges] {name}/max_iter=1: |V| against solve(q = 0): {gap:.2e}")
        assert np.array_equal(vs.cpu().numpy(), vm), gap
        same_bits(droop(env, dict(max_iter=1)), one, "after a solve()")
        refs = refs_of(name, env, dict(max_iter=1))
        worst, compared, left, _ = compare(f"{name}/max_iter=1", one, refs, dict(max_iter=1))
        assert compared == B
        note(f"{name}/max_iter=1", B, worst, compared, left)
    finally:
        env.close()


CONFIGS = dict(max_iter_4=dict(max_iter=4), max_iter_5=dict(max_iter=5), damping_1=dict(damping=1.0, max_iter=12),
               deadband_damping_1=dict(vb=0.97, vc=1.01, damping=1.0, max_iter=12), ratio_03=dict(reactive_ratio=0.3),
               ratio_08=dict(reactive_ratio=0.8))


@pytest.mark.parametrize("which", list(CONFIGS))
@pytest.mark.parametrize("name", ["crowded", "one_sgen"])
def test_parity_under_the_config_edges(name, which):
    """both sides of the host's poll (DROOP_POLL = 4), damping = 1 with vb == vc and with a real deadband, reactive_ratio 0.3 (the min binds
    for every sgen) and 0.8 (binds for some sgens of an env, exactly 1 for others: test_droop_edges_cpu.py), at noon rows"""
    B = D.B_PARITY
    env = make_env(name, B)
    try:
        env.reset(start_rows=torch.tensor(D.noon_rows(name, B)))
        a, it, st, vm = parity(f"{name}/{which}", name, env, CONFIGS[which])
        if which.startswith("max_iter"):
            assert (st == 1).all() and (it == CONFIGS[which]["max_iter"]).all()
        if which.startswith("ratio"):
            assert not np.array_equal(a, droop(env)[0])                      # the factor is alive
    finally:
        env.close()


@pytest.mark.parametrize("name", ["crowded", "one_sgen"])
def test_ratio_2_has_the_bits_of_ratio_1(name):
    B = D.B_PARITY
    env = make_env(name, B)
    try:
        env.reset(start_rows=torch.tensor(D.noon_rows(name, B)))
        same_bits(droop(env, dict(reactive_ratio=2.0)), droop(env), name)
        same_bits(droop(env, dict(reactive_ratio=2.0, vb=0.98, vc=1.02)), droop(env, dict(vb=0.98, vc=1.02)), name)
    finally:
        env.close()


# ---- one handle, many calls -----------------------------------------------------------------------------------------------------------
CALLS = [(None, True), (dict(max_iter=3), False), (dict(max_iter=100, reactive_ratio=0.3), True), (None, True)]


@pytest.mark.parametrize("name", ["crowded", "collapse"])
def test_one_handle_many_calls(name):
    """defaults with vm_pu, max_iter = 3 without, max_iter = 100 with reactive_ratio 0.3, defaults again on one handle (s.vm_out null
    after not null and back; the n_active memset covers max_iter + 1 entries of a workspace the longer call before it filled): each call has
    the bits of the same call on a fresh twin, the last those of the first.  On collapse the calls run over the collapse breakpoints."""
    B = D.B_PARITY
    base = dict(D.COLLAPSE_CFG) if name == "collapse" else {}
    calls = [(dict(base, **(cfg or {})), vm) for cfg, vm in CALLS]
    calls[0] = calls[3] = (dict(base), True)

    def fresh():
        if name == "collapse":
            return collapse_env(B)
        env = make_env(name, B)
        env.reset()
        return env
    env = fresh()
    try:
        outs = []
        for cfg, vm in calls:
            outs.append(droop(env, cfg, vm_pu=vm))
            twin = fresh()
            try:
                same_bits(outs[-1], droop(twin, cfg, vm_pu=vm), (name, cfg, vm))
            finally:
                twin.close()
        same_bits(outs[3], outs[0], name)
        assert len(outs[1]) == 3 and (outs[1][1] <= 3).all()
        if name == "collapse":
            assert set(outs[0][2].tolist()) >= {0, 2} and (outs[1][2] >= 1).all() and (outs[1][2] == 2).any()
    finally:
        env.close()
