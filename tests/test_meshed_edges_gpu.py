"""GPU (-m gpu): the general-topology solvers on the nets of tests/meshed_edge_nets.py (which lists the edge every shape reaches).
  * solve() per shape x solver geometry — k_nr_sparse at every sp_lanes that fits, k_nr_dense on the unvaried shapes, the automatic
    handle (k_nr_tree on the doubled-line feeders) — all 35 envs of the shape's pool against the oracle of its variant: iteration count
    and flag under the agreement rule of tests/edge_rule.py, complex voltage to V_TOL on the envs the oracle converges, the residual
    certificate below 1e-8 / sn_mva; the handle reports the pinned kernel.  The pools mix envs of 2 ... 10 iterations with envs that never
    converge inside every wavefront (tests/test_meshed_edges_cpu.py proves that of the oracle alone).
  * neighbours do not matter: at every sparse sp_lanes the pool reversed, rotated by one env, and envs 0 and 34 (a failing one) alone at
    B = 1 give, env by env, the bits of the first run — an env that finished early or never converges neither moves nor disturbs a lane
    beside it.
  * step() on tri3, wheel_rim and grid6 at sp_lanes 2, the largest sp_lanes that fits and dense, and on tail2x (two line rows on one bus
    pair in res_line and the line-loss term) under k_nr_tree, sp_lanes 2 and dense: the two plans of element_edge_nets.replay against
    the oracle env, with the bounds of tests/test_element_edges_gpu.py.
Results of a (shape, geometry) run and of the oracle are cached and shared between the tests."""
import functools

import numpy as np
import pytest
import torch

from mapdn_amd.env import VoltageControlBatch
from oracle.env_restated import INFO_KEYS
from tests import element_edge_nets as N
from tests import meshed_edge_nets as M
from tests.test_element_edges_gpu import Gaps, Q_LOSS_TOL, TOL, make_env, watch_state
from tests.test_kernel_matrix_gpu import assert_same_solution, oracle_envs

pytestmark = pytest.mark.gpu

V_TOL = 1e-9
DEV = "cuda:0"


def tuning_of(geom):
    """geom: "auto" | "dense" | sp_lanes"""
    return None if geom == "auto" else (dict(nr_solver="dense") if geom == "dense" else dict(nr_solver="sparse", sp_lanes=int(geom)))


def fits(key):
    return [L for L in M.SP_LANES if L not in M.LDS_REFUSED[M.base_of(key)]]


def solve(key, geom, ins):
    """solve() on a fresh handle: ((vm, va, iterations, converged) as numpy, kernel dict, lds_bytes)"""
    net, prof = M.make_net(key)
    env = VoltageControlBatch(net, prof, M.ARGS, n_envs=ins[0].shape[0], device=DEV, obs_dtype=torch.float64, tuning=tuning_of(geom))
    try:
        out = [x.cpu().numpy() for x in env.solve(*ins)]
        return out, env.nr_kernel(), env.geometry()["lds_bytes"]
    finally:
        env.close()


@functools.lru_cache(maxsize=None)
def pool_run(key, geom):
    return solve(key, geom, M.pool(key))


def expected_kernel(key, geom):
    net, _ = M.make_net(key)
    dc, zip_ = M.variant_of(key)
    n = net.n_bus - 1
    if geom == "dense":
        N_ = M.dense_order(n)
        ga = int(N_ > 128)
        return dict(solver=2, W=(1 if N_ <= 64 else 2) if not ga else next(w for w in (3, 4, 5, 6, 8, 11, 13, 16) if 64 * w >= N_), GA=ga)
    if geom == "auto":
        if M.base_of(key) in M.RADIAL:
            return dict(solver=0, DC=dc, ZIP=zip_)
        return dict(solver=1, DC=dc, ZIP=zip_)
    return dict(solver=1, L=int(geom), DC=dc, ZIP=zip_)


def geometries(key):
    if key in M.SOLVE_ONLY:
        return [2, "dense"]
    return fits(key) + (["dense"] if key in M.SHAPES else []) + ["auto"]


SOLVE_CASES = [(k, g) for k in M.POOLED for g in geometries(k)]


@pytest.mark.parametrize("key,geom", SOLVE_CASES, ids=[f"{k}-{g}" for k, g in SOLVE_CASES])
def test_solve_matches_the_oracle(key, geom):
    net, _ = M.make_net(key)
    (vm, va, it, cv), kernel, lds = pool_run(key, geom)
    want = expected_kernel(key, geom)
    assert {k: kernel[k] for k in want} == want, (kernel, want)
    if kernel["solver"] == 1:
        assert kernel["L"] in fits(key) and 0 < lds <= M.CU_LDS
    if kernel["solver"] == 2:                                            # A[N][N + 2] (LDS-resident only) | rhs[N] | dinv[2 N] | V[n + 2] pairs | 10 x threads
        n = net.n_bus - 1
        assert lds == M.dense_lds_bytes(n, M.dense_order(n), kernel["W"], kernel["GA"])
    envs = oracle_envs(M.B_POOL) if key in M.SOLVE_ONLY else list(range(M.B_POOL))
    worst = worst_res = 0.0
    n_failed = 0
    for e in envs:
        r, agrees = M.oracle(key, e)
        assert agrees(it[e], cv[e]), (key, geom, e, int(it[e]), bool(cv[e]), r.iterations, bool(r.converged))
        n_failed += not cv[e]
        if r.converged:
            v = vm[e] * np.exp(1j * np.radians(va[e]))
            worst = max(worst, float(np.abs(v - r.V).max()))
            if cv[e]:
                worst_res = max(worst_res, M.oracle_residual(key, e, v))
    print(f"\n[meshed edges] {key}/{geom}: worst |dV| = {worst:.1e}, worst residual = {worst_res:.1e}, {n_failed} envs not converged")
    assert worst <= V_TOL, (key, geom, worst)
    assert worst_res < 1e-8 / net.sn_mva, (key, geom, worst_res)
    assert n_failed >= 1 and not cv[M.FAILING_ENV]


NEIGHBOUR_CASES = [(k, L) for k in M.POOLED if k not in M.SOLVE_ONLY for L in fits(k)]


@pytest.mark.parametrize("key,L", NEIGHBOUR_CASES, ids=[f"{k}-{L}" for k, L in NEIGHBOUR_CASES])
def test_neighbours_do_not_matter(key, L):
    """the per-lane `done` masking of k_nr_sparse: every env's vm, va, iterations and flag have the bits of the same env in the first
    run, whoever shares its wavefront and wherever its workgroup sits"""
    base, kernel, _ = pool_run(key, L)
    assert kernel["solver"] == 1 and kernel["L"] == L
    ins = M.pool(key)
    B = M.B_POOL
    for what, idx in (("reversed", np.arange(B)[::-1]), ("rotated by one", np.roll(np.arange(B), 1))):
        out, k2, _ = solve(key, L, tuple(np.ascontiguousarray(x[idx]) for x in ins))
        assert k2 == kernel
        assert_same_solution(out, [x[idx] for x in base], f"{key} sp_lanes {L}: pool {what}")
    for e in (0, M.FAILING_ENV):
        out, k2, _ = solve(key, L, tuple(np.ascontiguousarray(x[e:e + 1]) for x in ins))
        assert k2 == kernel
        assert_same_solution(out, [x[e:e + 1] for x in base], f"{key} sp_lanes {L}: env {e} alone")
    assert bool(base[3][0]) and not base[3][M.FAILING_ENV]


# ---- step() -----------------------------------------------------------------------------------------------------------------------------
STEP_CASES = [(k, g) for k in M.STEP_SHAPES for g in sorted({2, max(fits(k))}) + ["dense"]] + [(M.STEP_DOUBLED, g) for g in ("auto", 2, "dense")]


@pytest.mark.parametrize("plan", list(N.PLANS))
@pytest.mark.parametrize("name,geom", STEP_CASES, ids=[f"{k}-{g}" for k, g in STEP_CASES])
def test_step_against_the_oracle_env(name, geom, plan):
    """test_element_edges_gpu.test_every_env_against_the_oracle on a meshed shape under a pinned general solver: the "auto" and "frozen"
    plans (an unsolvable action on env 7, frozen envs, a call that finds every env frozen, a whole-batch reset) — reward, terminated,
    the 11 info values, obs, state and results() of every env at every call"""
    p = N.PLANS[plan]
    env = make_env(name, N.B_WATCH, tuning=tuning_of(geom), auto_reset=p["auto_reset"])
    want = expected_kernel(name, geom)
    kernel = env.nr_kernel()
    assert {k: kernel[k] for k in want} == want, (kernel, want)
    gaps = Gaps()
    seen = dict(step=0, restart=0, frozen=0)
    for kind, call, x, os_ in N.replay(name, plan, unsolvable=M.STEP_UNSOLVABLE):
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
            w = (name, geom, plan, call, e)
            seen[k] += 1
            assert bool(mask[e]) == (k == "restart") and bool(term[e]) == to, w
            if k == "step":
                gaps.see("reward", r[e], ro, TOL, w)
                for c, key in enumerate(INFO_KEYS):
                    gaps.see("q_loss" if key == "q_loss" else "info", info[e, c], io[key], Q_LOSS_TOL if key == "q_loss" else TOL, w)
            else:
                assert r[e] == 0.0 and (info[e] == 0.0).all(), w
        watch_state(env, os_, gaps, (name, geom, plan, call))
    assert env.stats()["reset_failures"] == 0
    assert seen["step"] > 0 and (seen["restart"] >= 2 * N.B_WATCH if plan == "auto" else seen["frozen"] == N.B_WATCH + 1)
    print(f"\n[meshed edges] step {name}/{geom}/{plan}: " + " ".join(f"{k}={v:.1e}" for k, v in sorted(gaps.items())))
    env.close()
