"""GPU (-m gpu): action_gradients on handles of the sparse solver (mapdn_env_config.grad_meshed = 1: k_action_grad_sparse between the solve
and k_whatif_score of the what-if frame).

The reference is tests/grad_ref.py carried above float64, evaluated at the kernel's own |V| with the oracle's angles; the bar is
tests/grad_ref.bar's rule unchanged — 16 x the float64 reference's own error on the case (tests/grad_sparse_cases.E64) and never below
64 ulp, relative to the row's largest entry.  The scenario is that of tests/grad_sparse_cases.py (reset, one random step, candidates
{0, random, UNSOLVABLE, random}); every test asserts the oracle's solved pattern before it compares.

Shapes: nets of 3 to 36 buses at every sp_lanes that fits, B = 1, 5, 17, 35 (ragged for every sp_lanes), K = 1 and 3."""
import copy
import functools

import numpy as np
import pytest
import torch

from mapdn_amd.env import VoltageControlBatch
from tests import grad_ref as G
from tests import grad_sparse_cases as GS
from tests import meshed_edge_nets as M
from tests import opf_kernel_cases as OK
from tests import test_action_grad_edges_gpu as TE
from tests import test_action_grad_gpu as TG
from tests import whatif_cases as W
from tests.baseline_contract import check_state_untouched_and_step_agrees
from tests.test_action_grad_gpu import DEV, evaluate, gradients, same_bits
from tests.test_zip_loads_gpu import V_TOL

pytestmark = pytest.mark.gpu

KERNELS = ["k_action_grad_sparse"]
BATCHES, KS = (1, 5, 17, 35), (1, 3)
PATTERN = np.array([True, True, False, True])


def make_env(key, B, L=None, grad_meshed=1, env_id_offset=0, **args):
    net, prof, base = GS.make(key)
    return VoltageControlBatch(net, prof, dict(base, **args), n_envs=B, device=DEV, obs_dtype=torch.float64,
                               tuning=GS.tuning(key, L, grad_meshed), env_id_offset=env_id_offset)


def scenario(env, key, first=0):
    env.reset()
    a0 = GS.first_action(key, first + env.n_envs)[first:]
    _, term, info = env.step(torch.as_tensor(a0, device=DEV))
    assert env.stats()["reset_failures"] == 0 and not bool(term.any()) and float(info[:, 10].max()) == 0.0


@functools.lru_cache(maxsize=None)
def _ext(key, args, e, k, vm_bytes):
    os_, rows, cand, _ = GS.reference(key, *GS.shape_of(args), args)
    o = os_[e]
    V = np.frombuffer(vm_bytes) * np.exp(1j * np.angle(rows[e][k]["r"].V))
    return G.reward_gradient(o.net, G.env_args(o), V, cand[e, k], G.limits(o), ext=True)


def compare(key, args, got, B, K, where=""):
    """grad rows (e, k) of a call against the extended reference at the kernel's |V| and the oracle's angles; status, |V|, NaN rows"""
    os_, rows, cand, solved = GS.reference(key, *GS.shape_of(args), args)
    assert (solved == PATTERN).all()
    grad, reward, info, st, it, vm = got
    ns = os_[0].net.n_sgen
    assert grad.shape == (B, K, ns) and grad.dtype == np.float64 and st.shape == (B, K) and st.dtype == np.uint8
    worst, bar, at = 0.0, GS.bar(key, args), None
    for e in range(B):
        for k in range(K):
            p, w = rows[e][k], (key, args, where, B, K, e, k)
            assert st[e, k] == (W.SOLVED if p["solved"] else W.PF_FAILED), w
            if not p["solved"]:
                assert np.isnan(grad[e, k]).all() and np.isnan(vm[e, k]).all() and reward[e, k] < -200.0, w
                continue
            assert np.isfinite(grad[e, k]).all() and np.abs(vm[e, k] - p["vm"]).max() <= V_TOL, w
            if e not in OK.ref_envs(B):
                continue
            err = G.rel_inf(grad[e, k], _ext(key, tuple(args), e, k, np.ascontiguousarray(vm[e, k]).tobytes()))
            if err > worst:
                worst, at = err, w
    print(f"\n[grad sparse gpu] {key} {dict(args)} {where} B={B} K={K}: e64 {GS.E64[(key, tuple(args))]:.2e} gpu {worst:.2e} bar {bar:.2e}")
    assert worst <= bar, (at, worst, bar)
    return worst


# ---- parity -------------------------------------------------------------------------------------------------------------------------------
PARITY = [(key, L) for key in GS.PARITY_NETS for L in GS.fits(key)]


@pytest.mark.parametrize("key,L", PARITY, ids=[f"{k}-{L}" for k, L in PARITY])
def test_against_the_extended_reference(key, L):
    """a triangle (n = 2 < S), a doubled line on a pinned radial net, a complete graph, one 25-entry row among 4-entry rows, a fill-heavy
    lattice, an sgen on the ext_grid bus and two on one bus (crowded_meshed), a Ybus that is not symmetric (k9_hv, DC start)"""
    assert W.global_kernels("grad_sparse.hip") == KERNELS
    for B in BATCHES:
        env = make_env(key, B, L)
        try:
            kern = env.nr_kernel()
            assert kern["solver"] == 1 and kern["L"] == L and kern["DC"] == int(key.endswith("_hv"))
            scenario(env, key)
            for K in KS:
                c = GS.candidates(key, B, K)
                compare(key, (), gradients(env, c), B, K, where=f"sp_lanes={L}")
        finally:
            env.close()


@pytest.mark.parametrize("args", GS.VARIANTS, ids=lambda a: str(a[0][1]))
def test_the_other_barriers(args):
    B, K = GS.VARIANT_SHAPE
    env = make_env(GS.VARIANT_NET, B, **dict(args))
    try:
        scenario(env, GS.VARIANT_NET)
        compare(GS.VARIANT_NET, args, gradients(env, GS.candidates(GS.VARIANT_NET, B, K)), B, K)
    finally:
        env.close()


@pytest.mark.parametrize("L", GS.fits(GS.LINE_NET))
def test_line_weight_with_two_lines_on_one_bus_pair(L):
    """tail2x: two net.line rows between one pair of buses add to the same two nodes of c, in the order of net.line at every sp_lanes"""
    B, K = GS.VARIANT_SHAPE
    key, args = GS.LINE_NET, G.LINE_ARGS
    net = GS.make(key)[0]
    pairs = [frozenset(p) for p in zip(net.line_from_bus.tolist(), net.line_to_bus.tolist())]
    assert len(set(pairs)) < len(pairs)
    env = make_env(key, B, L, **dict(args))
    try:
        scenario(env, key)
        compare(key, args, gradients(env, GS.candidates(key, B, K)), B, K, where=f"sp_lanes={L}")
    finally:
        env.close()


def test_radial_cross_check():
    """case33 pinned to the sparse solver with the switch against the default case33 handle (k_action_grad): both within their own bars
    of the extended reference (TG.compare asserts it); their mutual difference is reported"""
    name, B, K = "case33", 17, 4
    os_, ref, cand = G.reference(name, W.B_MAX, W.K_MAX)
    c = np.ascontiguousarray(cand[:B, :K])
    out = {}
    for which, tuning in (("tree", None), ("sparse", dict(nr_solver="sparse", grad_meshed=1))):
        env = TG.make_env(name, B, tuning=tuning)
        try:
            assert env.nr_kernel()["solver"] == (0 if tuning is None else 1)
            TG.scenario(env, name)
            out[which] = gradients(env, c)
            TG.compare(name, (), out[which], os_, ref, c, B, K)
        finally:
            env.close()
    a, b = out["tree"][0], out["sparse"][0]
    ok = np.isfinite(a)
    assert (ok == np.isfinite(b)).all()
    scale = np.abs(a[..., :]).max(axis=-1, keepdims=True)
    diff = float(np.nanmax(np.where(ok, np.abs(a - b) / scale, 0.0)))
    print(f"\n[grad sparse gpu] case33: tree against sparse, mutual difference {diff:.2e} (bar of each {G.bar(name):.2e})")
    assert diff <= 2 * G.bar(name)


def test_the_switch_changes_nothing_on_the_tree_solver():
    name, B, K = "crowded", 17, 4
    cand = G.candidates(name, B, K)
    out = []
    for tuning in (None, dict(grad_meshed=1)):
        env = TG.make_env(name, B, tuning=tuning)
        try:
            assert env.nr_kernel()["solver"] == 0
            TG.scenario(env, name)
            out.append(gradients(env, cand))
        finally:
            env.close()
    same_bits(*out, "grad_meshed = 1 on the tree solver")


# ---- bits -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["wheel_rim", "k9_hv"])
def test_bits(key):
    B, K = 35, 3
    cand = GS.candidates(key, B, K)
    per_lanes = {}
    for L in GS.fits(key):
        env = make_env(key, B, L)
        try:
            scenario(env, key)
            full = gradients(env, cand)
            per_lanes[L] = full
            assert (full[3] == np.where(PATTERN[:K], W.SOLVED, W.PF_FAILED)).all()
            same_bits(full, gradients(env, cand), "two calls")
            same_bits(full[1:], evaluate(env, cand), "reward, info, status, iterations, vm_pu as evaluate_actions")
            for k in range(K):                                # K = 1 gives column k of K = 3
                alone = gradients(env, cand[:, k:k + 1])
                same_bits([a[:, 0] for a in alone], [a[:, k] for a in full], f"K = 1, candidate {k}")
            c32 = cand.astype(np.float32)
            g32 = gradients(env, c32)
            same_bits(g32, gradients(env, c32.astype(np.float64)), "float32")
            assert g32[0].dtype == np.float64
        finally:
            env.close()
        for first_id, n in ((20, 1), (13, 20)):               # an env alone, and a batch that begins at env id 13: other lanes, other workgroups
            other = make_env(key, n, L, env_id_offset=first_id)
            try:
                scenario(other, key, first=first_id)
                got = gradients(other, cand[first_id:first_id + n])
                same_bits(got, [a[first_id:first_id + n] for a in full], f"sp_lanes {L}: env ids from {first_id}, B = {n}")
            finally:
                other.close()
    first = per_lanes[GS.fits(key)[0]]
    for L, got in per_lanes.items():                          # the gradient and |V| across sp_lanes
        same_bits((got[0], got[5]), (first[0], first[5]), f"sp_lanes {L} against {GS.fits(key)[0]}")


# ---- mixed wavefronts -----------------------------------------------------------------------------------------------------------------------
# candidate 0 of env e is FACTORS[e % 8] on every sgen: the oracle's Newton counts of the envs that share a wavefront differ, some never
# converge; env 7 is frozen by an unsolvable step before the call (no auto_reset).  The pools of tests/meshed_edge_nets.py are inputs of
# solve(); the what-if frame works on the env's own state, so the mix is made with the candidates, on the pools' shapes, and asserted of
# the oracle alone before anything is compared.
FACTORS = (0.5, -20.0, -60.0, -120.0, -200.0, 60.0, 200.0, -600.0)
FROZEN_ENV = 7


@functools.lru_cache(maxsize=None)
def mixed_reference(key):
    B = GS.B_MAX
    os_ = [copy.copy(o) for o in GS.reference(key, B, GS.K_MAX)[0]]       # (a shallow copy steps on its own: whatif_cases.predict)
    ns = os_[0].net.n_sgen
    a1 = np.random.default_rng(77).uniform(-0.8, 0.8, (B, ns))
    a1[FROZEN_ENV] = GS.unsolvable(key)
    for e, o in enumerate(os_):
        _, term, info = o.step(a1[e])
        assert bool(term) == (e == FROZEN_ENV) and info["destroy"] == (1.0 if e == FROZEN_ENV else 0.0)
    cand = GS.candidates(key, B, 3).copy()
    cand[:, 0] = np.array(FACTORS)[np.arange(B) % 8][:, None]
    rows = [None if e == FROZEN_ENV else [GS.predict(key, o, cand[e, k]) for k in range(3)] for e, o in enumerate(os_)]
    return os_, a1, cand, rows


@pytest.mark.parametrize("key", ["tri3", "grid6"])
def test_mixed_wavefronts(key):
    os_, a1, cand, rows = mixed_reference(key)
    B, K = cand.shape[:2]
    live = [e for e in range(B) if e != FROZEN_ENV]
    it0 = {e: (rows[e][0]["iterations"], rows[e][0]["solved"]) for e in live}
    head = [e for e in live if e < 16]
    assert len({it0[e][0] for e in head if it0[e][1]}) >= 3 and any(not it0[e][1] for e in head)
    assert it0[0] != it0[1] and it0[2] != it0[3]              # the two envs of a wavefront at sp_lanes 2
    # the bar's e64 on these rows (some sit close to voltage collapse): the float64 reference against the extended one at the oracle's V
    checked = [(e, k) for e in OK.ref_envs(B) + [3, 5, 6] if e != FROZEN_ENV for k in range(K) if rows[e][k]["solved"]]
    e64 = 0.0
    for e, k in checked:
        o, V = os_[e], rows[e][k]["r"].V
        g = [G.reward_gradient(o.net, G.env_args(o), V, cand[e, k], G.limits(o), ext=x) for x in (False, True)]
        e64 = max(e64, G.rel_inf(*g))
    bar = max(OK.BAR_FACTOR * e64, OK.BAR_FLOOR)
    for L in GS.fits(key):
        env = make_env(key, B, L)
        try:
            scenario(env, key)
            _, term, _ = env.step(torch.as_tensor(a1, device=DEV))
            term = term.cpu().numpy()
            assert bool(term[FROZEN_ENV]) and int(term.sum()) == 1
            got = gradients(env, cand)
            same_bits(got[1:], evaluate(env, cand), "reward, info, status, iterations, vm_pu as evaluate_actions")
            grad, st, vm = got[0], got[3], got[5]
            assert (st[FROZEN_ENV] == W.NOT_EVALUATED).all() and np.isnan(grad[FROZEN_ENV]).all()
            for e in live:
                for k in range(K):
                    solved = rows[e][k]["solved"]
                    assert st[e, k] == (W.SOLVED if solved else W.PF_FAILED), (key, L, e, k)
                    assert np.isfinite(grad[e, k]).all() == solved and (solved or np.isnan(grad[e, k]).all()), (key, L, e, k)
            worst, at = 0.0, None
            for e, k in checked:
                o = os_[e]
                V = vm[e, k] * np.exp(1j * np.angle(rows[e][k]["r"].V))
                ext = G.reward_gradient(o.net, G.env_args(o), V, cand[e, k], G.limits(o), ext=True)
                err = G.rel_inf(grad[e, k], ext)
                if err > worst:
                    worst, at = err, (e, k)
            print(f"\n[grad sparse gpu] mixed {key} sp_lanes={L}: e64 {e64:.2e} gpu {worst:.2e} bar {bar:.2e}")
            assert worst <= bar, (key, L, at, worst, bar)
        finally:
            env.close()


@pytest.mark.parametrize("j,on_slack", [(0, False), (2, True)], ids=["ordinary", "slack"])
def test_non_finite_candidates(j, on_slack):
    """tests/test_action_grad_edges_gpu.py's demands, on crowded_meshed under k_action_grad_sparse: an ordinary sgen — status 2 and a NaN
    row; the sgen on the slack bus — status 0 and a NaN row (1e300 keeps lim_j a_j finite: the row keeps its gradient); every other row
    keeps the bits of the clean call"""
    name = "crowded_meshed"
    os_, ref, full = G.reference(name, W.B_MAX, W.K_MAX)
    net = os_[0].net
    assert (int(net.sgen_bus[j]) == int(net.ext_grid_bus)) == on_slack
    cand = np.ascontiguousarray(full[:TE.NF_B, :TE.NF_K])
    env = TG.make_env(name, TE.NF_B, tuning=dict(grad_meshed=1))
    try:
        assert env.nr_kernel()["solver"] == 1
        TG.scenario(env, name)
        clean = gradients(env, TE.poisoned(cand, j, 0.0))
        assert (clean[3] == np.where(W.expected_pattern(TE.NF_K), W.SOLVED, W.PF_FAILED)).all()
        for value in TE.POISON:
            c = TE.poisoned(cand, j, value)
            got = gradients(env, c)
            TE.others_keep_their_bits(got, clean, (name, j, value))
            same_bits(got[1:], evaluate(env, c), "reward, info, status, iterations, vm_pu as evaluate_actions")
            TE.poisoned_rows_follow_the_oracle(name, os_, c, got[1:], on_slack, (name, j, value))
            r = got[0][list(TE.POISONED_ENVS), TE.NF_CAND]
            if on_slack and np.isfinite(value):
                keep = [i for i in range(net.n_sgen) if i != j]
                assert np.isfinite(r).all() and np.array_equal(r[:, keep], clean[0][list(TE.POISONED_ENVS), TE.NF_CAND][:, keep])
                for row, e in zip(r, TE.POISONED_ENVS):
                    lim, s = G.limits(os_[e])[j], net.sgen_scaling[j]
                    want = -os_[e].q_weight / net.n_sgen * lim * s
                    assert abs(row[j] - want) <= 4 * TG.ULP * abs(want), (value, e)
            else:
                assert np.isnan(r).all(), (j, value)
        same_bits(gradients(env, TE.poisoned(cand, j, 0.0)), clean, "the clean call after the poisoned ones")
    finally:
        env.close()


# ---- the contract and the refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("after_solve", [False, True])
def test_state_untouched_and_step_agrees(after_solve):
    key, k0 = "wheel_rim", 1

    def baseline(env):
        cand = torch.as_tensor(GS.candidates(key, env.n_envs, 3), device=DEV)
        g, _, _, st, _, vm = env.action_gradients(cand, vm_pu=True)
        assert (st[:, 2] == W.PF_FAILED).all() and (st[:, k0] == W.SOLVED).any() and bool(torch.isfinite(g[:, k0][st[:, k0] == 0]).all())
        return cand[:, k0].contiguous(), st[:, k0], vm[:, k0]
    check_state_untouched_and_step_agrees(lambda B: make_env(key, B), baseline, after_solve, B=24)


def test_refusals_on_live_handles():
    for key, grad_meshed, word in (("wheel_rim", 0, "meshed"), ("wheel_rim_zip", 1, "ZIP")):
        net, prof = M.make_net(key)
        env = VoltageControlBatch(net, prof, M.ARGS, n_envs=3, device=DEV, obs_dtype=torch.float64, tuning=dict(grad_meshed=grad_meshed))
        try:
            assert env.nr_kernel()["solver"] == 1
            env.reset()
            with pytest.raises(NotImplementedError, match=word):
                env.action_gradients(torch.zeros(3, 2, env.n_sgen, device=DEV))
            env.evaluate_actions(torch.zeros(3, 2, env.n_sgen, device=DEV))      # (which covers these handles)
        finally:
            env.close()
