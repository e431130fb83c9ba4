"""GPU (-m gpu): the env's step path — k_inject, k_inject_sgen, the injection prologue of k_nr_tree, k_reset_begin, k_advance with
commit_bus, k_commit_fused, k_gather, k_to_envminor, k_stats — on the nets of tests/element_edge_nets.py, whose element tables reach the
branches the shipped cases leave idle (DESIGN.md section 18 lists which net reaches which branch).

Against the oracle env every env of every batch is watched at every call; apart from the one forced step per run no step is unsolvable
and no reset takes a second draw (tests/test_element_edges_cpu.py proves that of the oracle alone, element_edge_nets.replay asserts it
again here).  Bounds are the project's own: 1e-9 on reward, info, obs, state and the result tables, 1e-12 on q_loss (test_gpu_parity.py,
test_gpu_shipped_configs.py); the load tables, which are a table value plus std x |N(0, 1)| of the same Philox block on both sides, to
1e-12 (values below 1 MW: 4 500 ulp, where log / sincos / sqrt of the device and of numpy differ by a few).

GPU_MEASURED: the worst gaps to the oracle seen on an MI355X, for the record; no bound comes from them."""
import numpy as np
import pytest
import torch

from mapdn_amd import _lib
from mapdn_amd.env import VoltageControlBatch
from oracle.env_restated import INFO_KEYS
from oracle.pp_restated import residual_inf, runpp_restated
from tests import element_edge_nets as N
from tests.edge_rule import same_newton_count

pytestmark = pytest.mark.gpu

TOL, Q_LOSS_TOL, LOAD_TOL, V_TOL = 1e-9, 1e-12, 1e-12, 1e-9
DEV = "cuda:0"
RESULT_KEYS = ("vm_pu", "va_degree", "p_mw", "q_mvar", "pl_mw", "sgen_p", "sgen_q")
# worst |gpu - oracle| over both plans, all calls and all 21 envs (absolute; MW, MVAr, p.u., degrees)
GPU_MEASURED = {}


def make_env(name, B, tuning=None, env_id_offset=0, obs_dtype=torch.float64, **args):
    net, prof = N.make(name)
    return VoltageControlBatch(net, prof, dict(N.ARGS, **args), n_envs=B, device=DEV, obs_dtype=obs_dtype, tuning=tuning,
                               env_id_offset=env_id_offset)


def snapshot(env):
    """everything the step path leaves behind, as fresh tensors"""
    out = dict(obs=env.get_obs().clone(), state=env.get_state().clone())
    out.update({k: v.clone() for k, v in env.results().items()})
    out["load_p"], out["load_q"] = env.loads()
    return out


def same_bits(a, b, where):
    for k in a:
        assert torch.equal(a[k], b[k]), (where, k)


# ---- against the oracle -------------------------------------------------------------------------------------------------------------
class Gaps(dict):
    def see(self, key, got, ref, tol, where):
        gap = float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max()) if np.size(ref) else 0.0
        self[key] = max(self.get(key, 0.0), gap)
        assert gap <= tol, (where, key, gap)


def watch_state(env, os_, gaps, where):
    """obs, state, results and loads of every env against its oracle's state"""
    net = env.net
    snap = {k: v.cpu().numpy() for k, v in snapshot(env).items()}
    empty = [b for b in N.layout(net)["empty"] if b != net.ext_grid_bus]
    for e, o in enumerate(os_):
        w = (*where, e)
        gaps.see("obs", snap["obs"][e], np.array(o.get_obs()), TOL, w)
        gaps.see("state", snap["state"][e], o.get_state(), TOL, w)
        for k in ("vm_pu", "va_degree", "p_mw", "q_mvar", "pl_mw"):
            gaps.see(k, snap[k][e], o.res[k], TOL, w)
        gaps.see("sgen_p", snap["sgen_p"][e], o.sgen_p, TOL, w)
        gaps.see("sgen_q", snap["sgen_q"][e], o.sgen_q, TOL, w)
        gaps.see("load_p", snap["load_p"][e], o.load_p, LOAD_TOL, w)
        gaps.see("load_q", snap["load_q"][e], o.load_q, LOAD_TOL, w)
        # Sbus by bus: the buses without an element report exactly nothing (the nets have no shunt; the ext_grid bus reports the slack
        # injection); the ext_grid bus and the twins are rows of p_mw / q_mvar like any other and were compared above
        assert (snap["p_mw"][e][empty] == 0.0).all() and (snap["q_mvar"][e][empty] == 0.0).all(), w
    assert snap["p_mw"].shape == (len(os_), net.n_bus) and net.shunt_bus.shape[0] == 0


@pytest.mark.parametrize("plan", list(N.PLANS))
@pytest.mark.parametrize("name", N.NETS)
def test_every_env_against_the_oracle(name, plan):
    """The plans of element_edge_nets.replay — "auto": auto_reset, float64 actions, per-env restarts that run out of step after the forced
    unsolvable step (k_inject_sgen with its restart branch); "frozen": no auto_reset, float32 actions, the forced env frozen, a
    whole-batch reset() in between (the injection in k_nr_tree's prologue; k_inject_sgen on crowded_meshed, which k_nr_sparse solves).

    Measured on an MI355X (worst gap over the nets, plans, calls and envs; GPU_MEASURED per net): see DESIGN.md section 18."""
    p = N.PLANS[plan]
    env = make_env(name, N.B_WATCH, auto_reset=p["auto_reset"])
    assert env.nr_kernel()["solver"] == (1 if name == "crowded_meshed" else 0)
    gaps = Gaps()
    seen = dict(step=0, restart=0, frozen=0)
    for kind, call, x, os_ in N.replay(name, plan):
        if kind == "reset":
            env.reset()
            watch_state(env, os_, gaps, (name, plan, "reset"))
            continue
        act, expect = x
        r, term, info = env.step(torch.as_tensor(act, device=DEV))
        assert act.dtype == p["dtype"]
        r, term, info = r.cpu().numpy(), term.cpu().numpy(), info.cpu().numpy()
        mask = env.auto_reset_mask().cpu().numpy()
        for e, (k, ro, to, io) in enumerate(expect):
            w = (name, plan, call, e)
            seen[k] += 1
            assert bool(mask[e]) == (k == "restart") and bool(term[e]) == to, w
            if k == "step":
                gaps.see("reward", r[e], ro, TOL, w)
                for c, key in enumerate(INFO_KEYS):
                    gaps.see("q_loss" if key == "q_loss" else "info", info[e, c], io[key], Q_LOSS_TOL if key == "q_loss" else TOL, w)
            else:
                assert r[e] == 0.0 and (info[e] == 0.0).all(), w
        watch_state(env, os_, gaps, (name, plan, call))
    assert env.stats()["reset_failures"] == 0
    assert seen["step"] > 0 and (seen["restart"] >= 2 * N.B_WATCH if plan == "auto" else seen["frozen"] == N.B_WATCH + 1)
    GPU_MEASURED[(name, plan)] = dict(gaps)
    print(f"\n[element edges] {name}/{plan}: " + " ".join(f"{k}={v:.1e}" for k, v in sorted(gaps.items())))
    env.close()


# ---- the three injection paths ------------------------------------------------------------------------------------------------------
def run_pair(name, a, b, n_calls, adt, forced, solve_at, reset_at=None):
    """two handles through the same calls; everything they return and hold must have the same bits.  Returns the restarts seen"""
    net, prof = N.make(name)
    B = a.n_envs
    oa, sa = a.reset(); ob, sb = b.reset()
    assert torch.equal(oa, ob) and torch.equal(sa, sb)
    gen = torch.Generator(device=DEV); gen.manual_seed(23)
    rng = np.random.default_rng(2)
    n_restarts = 0
    for t in range(n_calls):
        act = ((torch.rand(B, net.n_sgen, device=DEV, generator=gen, dtype=torch.float64) * 2 - 1) * 0.8).to(adt)
        if t == forced:
            act[11] = N.UNSOLVABLE
        if t == solve_at:                            # a solve on explicit inputs in between: Sbus no longer reflects cur_pl / cur_ql
            rows = rng.integers(0, prof.n_rows, B)
            qs = rng.uniform(-0.3, 0.3, (B, net.n_sgen)) * prof.pv[rows]
            x = a.solve(prof.load_p[rows], prof.load_q[rows], prof.pv[rows], qs)
            y = b.solve(prof.load_p[rows], prof.load_q[rows], prof.pv[rows], qs)
            assert all(torch.equal(u, v) for u, v in zip(x, y))
        if t == reset_at:
            oa, sa = a.reset(); ob, sb = b.reset()
            assert torch.equal(oa, ob) and torch.equal(sa, sb)
        ra, ta, ia = a.step(act); rb, tb, ib = b.step(act)
        assert torch.equal(ra, rb) and torch.equal(ta, tb) and torch.equal(ia, ib), (name, t)
        if t == forced:
            assert bool(ta[11]) and ia[11, 10] == 1.0
        ma = a.auto_reset_mask()
        assert torch.equal(ma, b.auto_reset_mask())
        n_restarts += int(ma.sum().item())
        same_bits(snapshot(a), snapshot(b), (name, t))
    return n_restarts


@pytest.mark.parametrize("name", N.NETS)
def test_pv_bus_injection_equals_all_bus_injection_on_edge_nets(name):
    """k_inject_sgen (PV rows, mlo rows, the restart branch that strides the load-only buses over an env's PV threads) + k_advance's ld_dest
    stores against the all-bus k_inject (inject_full = 1) on handles with auto_reset: per-env restarts after the forced step and at the
    episode limit, and a solve() on explicit inputs in between, which leaves Sbus stale"""
    B = 70
    fast = make_env(name, B, auto_reset=True)
    full = make_env(name, B, tuning=dict(inject_full=1), auto_reset=True)
    n = run_pair(name, fast, full, 11, torch.float64, forced=1, solve_at=5)
    assert n >= 2 * B
    fast.close(); full.close()


@pytest.mark.parametrize("adt", [torch.float64, torch.float32])
@pytest.mark.parametrize("name,geom", [(n, None) for n in N.NETS] + [("crowded", (4, 16)), ("crowded", (1, 32))])
def test_fused_injection_equals_the_injection_launch_on_edge_nets(name, geom, adt):
    """the prologue of k_nr_tree (fuse_inject = 1) against k_inject_sgen as a launch (fuse_inject = 2), no auto_reset: the forced env stays
    frozen, a solve() in between, a whole-batch reset().  crowded with (nr_waves, nr_lanes) pinned: 5 rows x L items on IT x NT = 3 x 64 W
    slots — (4, 16): 80 items, one pass, most threads idle; (1, 32): 160 items, one pass, the third batch a partial tile.
    crowded_meshed runs k_nr_sparse, which has no prologue: there the injection launch is compared with the all-bus k_inject."""
    B = 70
    t0 = dict(nr_waves=geom[0], nr_lanes=geom[1]) if geom else {}
    if name == "crowded_meshed":
        a, b = make_env(name, B, tuning=dict(fuse_inject=2)), make_env(name, B, tuning=dict(inject_full=1))
    else:
        a, b = make_env(name, B, tuning=dict(fuse_inject=1, **t0)), make_env(name, B, tuning=dict(fuse_inject=2, **t0))
        if geom:
            assert (a.nr_kernel()["W"], a.nr_kernel()["L"]) == geom == (b.nr_kernel()["W"], b.nr_kernel()["L"])
    run_pair(name, a, b, 7, adt, forced=1, solve_at=2, reset_at=4)
    a.close(); b.close()


# ---- placement ----------------------------------------------------------------------------------------------------------------------
def episode_start(env, acts, off=0):
    """reset() plus three noisy steps; the snapshots and (reward, terminated, info) after each"""
    env.reset()
    out = [(snapshot(env), None)]
    for t in range(acts.shape[0]):
        r, term, info = env.step(torch.as_tensor(acts[t, off:off + env.n_envs], device=DEV))
        out.append((snapshot(env), (r.clone(), term.clone(), info.clone())))
    return out


def placement_actions(name, B):
    net, _ = N.make(name)
    return np.random.default_rng(B).uniform(-0.8, 0.8, (3, B, net.n_sgen))


@pytest.mark.parametrize("name", N.NETS)
def test_every_env_of_a_batch_equals_the_same_env_alone(name):
    """B = 70 against 70 handles of B = 1 at env_id_offset = e: obs, state, results and loads to the bit; reward and info to rtol = atol =
    1e-13 (the handles choose different launch geometries, whose workers sum the reward's partials in another grouping:
    test_default_launch_matches_oracle_at_full_size)"""
    B = 70
    acts = placement_actions(name, B)
    env = make_env(name, B)
    batch = episode_start(env, acts)
    env.close()
    for e in range(B):
        one = make_env(name, 1, env_id_offset=e)
        alone = episode_start(one, acts, off=e)
        one.close()
        for t, ((sb, ob), (sa, oa)) in enumerate(zip(batch, alone)):
            for k in sb:
                assert torch.equal(sb[k][e], sa[k][0]), (name, e, t, k)
            if ob is not None:
                assert bool(ob[1][e]) == bool(oa[1][0])
                torch.testing.assert_close(ob[0][e], oa[0][0], rtol=1e-13, atol=1e-13)
                torch.testing.assert_close(ob[2][e], oa[2][0], rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("name", ["crowded", "all_pv"])
def test_slices_of_a_512_env_grid_equal_small_handles(name):
    """B = 449 (Bp = 512: k_gather's grid has 8 env tiles, so its XCD remap is on; k_advance, k_inject_sgen and k_stats run two blocks of
    256 envs) against handles of B = 70 at env_id_offset 0, 190 and 379, every env of those slices: obs in float32 and float64, state,
    results, loads.  crowded has 150 obs columns (scalar stores, three column tiles), all_pv 88 (4-column vector stores).
    Once per net the obs is also fetched through mapdn_get_obs into a view that starts one element into a larger buffer — the vector path
    must fall back to scalar stores on the misaligned base — and must equal the aligned fetch, with the elements around it untouched."""
    B, Bs = 449, 70
    acts = placement_actions(name, B)
    big = make_env(name, B)
    n_obs = big.n_agents * big._obs_size1
    assert (n_obs % 4 == 0) == (name == "all_pv")
    smalls = {off: make_env(name, Bs, env_id_offset=off) for off in (0, 190, 379)}
    big.reset()
    for s in smalls.values():
        s.reset()
    for t in range(4):
        if t:
            big.step(torch.as_tensor(acts[t - 1], device=DEV))
        snap = snapshot(big)
        o32 = big.get_obs(torch.float32).clone()
        for dt in (torch.float32, torch.float64):                   # the misaligned view
            buf = torch.full((B * n_obs + 2,), -7.0, dtype=dt, device=DEV)
            with torch.cuda.device(big.device):
                _lib.check(big._lib.mapdn_get_obs(big._h, buf.data_ptr() + buf.element_size(), big._code(dt), big._stream()), big._h)
            want = o32 if dt == torch.float32 else snap["obs"]
            assert torch.equal(buf[1:-1].view(B, big.n_agents, -1), want) and buf[0].item() == -7.0 and buf[-1].item() == -7.0, (name, t, dt)
        for off, s in smalls.items():
            if t:
                s.step(torch.as_tensor(acts[t - 1, off:off + Bs], device=DEV))
            ss = snapshot(s)
            for k in ss:
                assert torch.equal(snap[k][off:off + Bs], ss[k]), (name, t, off, k)
            assert torch.equal(o32[off:off + Bs], s.get_obs(torch.float32)), (name, t, off)
    big.close()
    for s in smalls.values():
        s.close()


# ---- bookkeeping kernels ------------------------------------------------------------------------------------------------------------
def test_reset_with_refused_start_rows_and_stats_beyond_256_envs():
    """reset(start_rows=...) through the C entry (the Python layer refuses such rows up front) at B = 449: k_reset_begin marks the negative
    rows and those with start + episode_limit + 1 >= T bad, k_stats (one block striding 449 envs) counts exactly them, they stay done, and
    the first obs of every good env is the oracle's reset(start=...)"""
    name, B = "crowded", 449
    net, prof = N.make(name)
    rows, bad = N.start_rows_mix(name, B)
    env = make_env(name, B)
    sr = torch.as_tensor(rows, dtype=torch.int64, device=DEV)
    with torch.cuda.device(env.device):
        _lib.check(env._lib.mapdn_reset(env._h, sr.data_ptr(), 1, env.max_reset_tries, env._stream()), env._h)
    env._was_reset = True
    assert env.stats()["reset_failures"] == int(bad.sum())
    assert np.array_equal(env.start_rows().cpu().numpy()[~bad], rows[~bad])
    obs = env.get_obs().cpu().numpy()
    state = env.get_state().cpu().numpy()
    os_ = N.oracles(name, B)
    gaps = Gaps()
    for e, o in enumerate(os_):
        if bad[e]:
            continue
        oo, so = N.first_draw_reset(o, N.row_to_start(prof, rows[e]))
        gaps.see("obs", obs[e], np.array(oo), TOL, e)
        gaps.see("state", state[e], so, TOL, e)
    act = np.random.default_rng(1).uniform(-0.8, 0.8, (B, net.n_sgen))
    r, term, info = env.step(torch.as_tensor(act, device=DEV))
    r, term, info = r.cpu().numpy(), term.cpu().numpy(), info.cpu().numpy()
    assert term[bad].all() and (r[bad] == 0.0).all() and (info[bad] == 0.0).all() and not term[~bad].any()
    iters = []
    for e, o in enumerate(os_):
        if not bad[e]:
            ro, to, io = o.step(act[e])
            assert io["destroy"] == 0.0
            gaps.see("reward", r[e], ro, TOL, e)
            iters.append(o.res.iterations)
    st = env.stats()
    assert st["reset_failures"] == int(bad.sum())
    # the sums of k_stats over the active envs: an env AT the tolerance edge may take one Newton step more or less than the oracle
    # (INTEGRATION.md), which moves the mean by 1 / 398; a sum over the wrong envs would not hide in 0.05
    assert abs(st["mean_nr_iters"] - np.mean(iters)) < 0.05 and abs(st["max_nr_iters"] - max(iters)) <= 1
    print(f"\n[element edges] start rows: " + " ".join(f"{k}={v:.1e}" for k, v in sorted(gaps.items())))
    env.close()


def test_solve_on_explicit_inputs_with_odd_element_counts():
    """solve() on crowded at B = 70: k_to_envminor with nl = 9 and ns = 5 columns (one partial 64-column tile, a partial env tile), then
    the all-bus k_inject in MODE_SOLVE; every env against runpp_restated with V_TOL and the Newton count rule of test_gpu_parity.py"""
    name, B = "crowded", 70
    net, prof = N.make(name)
    env = make_env(name, B)
    pl, ql, pv, qs = N.solve_inputs(name, B)
    vm, va, it, cv = (x.cpu().numpy() for x in env.solve(pl, ql, pv, qs))
    assert cv.all()
    worst = 0.0
    for e in range(B):
        r = runpp_restated(net, pl[e], ql[e], pv[e], qs[e])
        assert r.converged and same_newton_count(net, (pl[e], ql[e], pv[e], qs[e]), it[e], cv[e], r)
        worst = max(worst, np.abs(vm[e] - r.vm_pu).max(), np.abs(va[e] - r.va_degree).max() * np.pi / 180)
        v = vm[e] * np.exp(1j * va[e] * np.pi / 180)
        assert residual_inf(net, v, pl[e], ql[e], pv[e], qs[e]) < 1e-8 / net.sn_mva
    assert worst < V_TOL, worst
    print(f"\n[element edges] solve: worst |dV| = {worst:.1e}")
    env.close()
