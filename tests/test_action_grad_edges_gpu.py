"""GPU (-m gpu): action_gradients and evaluate_actions at the edges of their frame (k_action_grad, k_whatif_start, k_whatif_score; DESIGN.md
sections 20 and 22).

  parity       the hand-built nets of tests/grad_edge_nets.py (one node, a 40-bus chain, a star, three trees, a comb, out-of-service /
               parallel / charged net.line rows) at B = 1, 64, 65, 130 — a lane alone, a full wave of k_action_grad's 64-env workgroup, the
               `e >= B` tail of a second one, a third one — and case141 at B = 65; K = 1 and K = 4 on one handle.  The reference and the
               bar are those of tests/test_action_grad_gpu.py (the extended reference at the kernel's |V| and the oracle's angles; 16 x
               E64, never below 64 ulp), on the envs of EN.ref_envs64; statuses and |V| on every env.
  bits         chain40 at B = 130: envs 60 .. 70 against a handle that holds those eleven envs alone, two calls, evaluate_actions.
  non-finite   NaN, +inf, -inf and 1e300 in one entry of candidate 1 of the envs 0, 5, 15, 16 of a batch of 17: the poisoned rows are the
               oracle's (an ordinary sgen: the power flow fails; the sgen on the slack bus: solved, a reward that is not finite), their
               gradient rows are NaN, and every other row of the call — candidates 2 and 3 of the poisoned envs included — keeps the bits
               of the call with 0.0 in that entry.  The loops a non-finite value reaches are bounded by counts (max_it, the static
               sweeps): read in nr_tree.hpp, sparse.hip and dense.hip before this ran.
  call order   droop_actions, opf_actions, opf_probe, evaluate_actions, action_gradients and difference_rewards on one case33 handle, in
               that order, in reverse and after a solve() that leaves Sbus stale, against fresh twin handles."""
import warnings

import numpy as np
import pytest
import torch

from tests import baseline_contract as BC
from tests import grad_edge_nets as EN
from tests import grad_ref as G
from tests import whatif_cases as W
from tests.test_action_grad_gpu import DEV, ULP, evaluate, gradients, make_env, same_bits
from tests.test_action_grad_gpu import scenario as scenario_random
from tests.test_zip_loads_gpu import V_TOL

pytestmark = pytest.mark.gpu

HAND_B = (1, 64, 65, 130)
LINE_B = 65


def scenario(env, name, first=0):
    """the reset at the daytime rows of EN.start_rows and the one random step of G.reference (first: the env id of env 0)"""
    rows = EN.start_rows(name, first + env.n_envs)[first:]
    env.reset(start_rows=torch.as_tensor(rows, dtype=torch.int64))
    a0 = G.first_action(name, first + env.n_envs)[first:]
    _, term, info = env.step(torch.as_tensor(a0, device=DEV))
    assert env.stats()["reset_failures"] == 0 and not bool(term.any()) and float(info[:, 10].max()) == 0.0


def compare64(name, args, got, os_, ref, cand, B, K):
    """tests/test_action_grad_gpu.compare with the reference envs of EN.ref_envs64: status, |V| and NaN rows on every env"""
    grad, reward, info, st, it, vm = got
    ns = os_[0].net.n_sgen
    assert grad.shape == (B, K, ns) and grad.dtype == np.float64 and st.shape == (B, K) and st.dtype == np.uint8
    worst, bar = 0.0, G.bar(name, args)
    for e in range(B):
        for k in range(K):
            p, w = ref["rows"][e][k], (name, args, B, K, e, k)
            assert st[e, k] == (W.SOLVED if p["solved"] else W.PF_FAILED), w
            if not p["solved"]:
                assert np.isnan(grad[e, k]).all() and np.isnan(vm[e, k]).all() and reward[e, k] < -200.0, w
                continue
            assert np.isfinite(grad[e, k]).all() and np.abs(vm[e, k] - p["vm"]).max() <= V_TOL, w
            if e not in EN.ref_envs64(B):
                continue
            o = os_[e]
            V = vm[e, k] * np.exp(1j * np.angle(p["r"].V))
            ext = G.reward_gradient(o.net, G.env_args(o), V, cand[e, k], G.limits(o), ext=True)
            err = G.rel_inf(grad[e, k], ext)
            worst = max(worst, err)
            assert err <= bar, (w, err, bar)
    print(f"\n[grad gpu] {name} {dict(args)} B={B} K={K}: e64 {G.E64[(name, tuple(args))]:.2e} gpu {worst:.2e} bar {bar:.2e}")
    return worst


def parity(name, B, args=()):
    B_ref, K_ref = G.shape_of(args, name)
    os_, ref, cand = G.reference(name, B_ref, K_ref, args)
    assert (ref["solved"] == W.expected_pattern(K_ref)).all()
    env = make_env(name, B, **dict(args))
    try:
        assert env.nr_kernel()["solver"] == 0
        scenario(env, name)
        out = {}
        for K in (1, 4):
            c = np.ascontiguousarray(cand[:B, :K])
            out[K] = gradients(env, c)
            compare64(name, args, out[K], os_, ref, c, B, K)
        same_bits([a[:, 0] for a in out[1]], [a[:, 0] for a in out[4]], "K = 1 gives candidate 0 of K = 4")
        return out[4], os_, cand[:B]
    finally:
        env.close()


# ---- parity -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", HAND_B)
@pytest.mark.parametrize("name", EN.HAND_BUILT)
def test_hand_built_nets_against_the_extended_reference(name, B):
    got, os_, cand = parity(name, B)
    if name == "feeders3":                                        # the sgen on the slack bus: the direct term alone, to the rounding of lim
        grad, net, j = got[0], os_[0].net, 3
        assert int(net.sgen_bus[j]) == int(net.ext_grid_bus) and (grad[:, 0, j] == 0.0).all()
        for e in range(B):
            o = os_[e]
            lim, s = G.limits(o)[j], net.sgen_scaling[j]
            for k in (1, 3):
                want = -o.q_weight / net.n_sgen * np.sign(lim * cand[e, k, j] * s) * lim * s
                assert abs(grad[e, k, j] - want) <= 4 * ULP * abs(want), (e, k, grad[e, k, j], want)


def test_case141_against_the_extended_reference():
    parity("case141", G.EDGE_B["case141"])


@pytest.mark.parametrize("name", ["ties", "feeders3"])
def test_line_weight_on_the_line_table_edges(name):
    """grad_line_rhs over out-of-service rows (both ends at the slack position, zero constants, counted in the mean), a doubled line and
    rows with charging and conductance; three trees under one slack.  No q term: the entry of the slack-bus sgen is exactly zero."""
    got, os_, cand = parity(name, LINE_B, G.LINE_ARGS)
    if name == "feeders3":
        assert (got[0][:, W.expected_pattern(EN.K_MAX)][:, :, 3] == 0.0).all()


# ---- bits across the 64-env edge ----------------------------------------------------------------------------------------------------------
def test_bits_across_the_workgroup_edge():
    name, B, K = "chain40", 130, EN.K_MAX
    first, n = 60, 11
    cand = G.candidates(name, B, K)
    env = make_env(name, B)
    try:
        scenario(env, name)
        full = gradients(env, cand)
        assert (full[3] == np.where(W.expected_pattern(K), W.SOLVED, W.PF_FAILED)).all()
        same_bits(full, gradients(env, cand), "two calls")
        same_bits(full[1:], evaluate(env, cand), "reward, info, status, iterations, vm_pu as evaluate_actions")
    finally:
        env.close()
    other = make_env(name, n, env_id_offset=first)                # envs 60 .. 70: lanes 60 .. 63 and 0 .. 6 there, lanes 0 .. 10 here
    try:
        scenario(other, name, first=first)
        got = gradients(other, cand[first:first + n])
        same_bits(got, [a[first:first + n] for a in full], f"env ids from {first}, B = {n}")
    finally:
        other.close()


# ---- non-finite candidates ----------------------------------------------------------------------------------------------------------------
POISON = (np.nan, np.inf, -np.inf, 1e300)
POISONED_ENVS = (0, 5, 15, 16)
NF_B, NF_K, NF_CAND = 17, 4, 1
TOL = 1e-9                                                        # of tests/test_whatif_gpu.py, on reward and info


def agrees(x, want):
    """x against the oracle's figure: NaN for NaN, the same infinity, else tests/test_whatif_gpu.py's 1e-9 (relative above 1: a q_loss of
    3e299 is no figure an absolute bound applies to)"""
    x, want = np.asarray(x, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    ok = np.where(fin, np.abs(x - np.where(fin, want, 0.0)) <= TOL * np.maximum(1.0, np.abs(np.where(fin, want, 0.0))), False)
    ok = np.where(np.isnan(want), np.isnan(x), ok)
    ok = np.where(np.isinf(want), x == want, ok)
    return bool(ok.all())


def others_keep_their_bits(got, clean, where):
    """every (env, candidate) row but the poisoned ones: bit for bit the call with 0.0 in the poisoned entry"""
    mask = np.ones((NF_B, NF_K), bool)
    mask[list(POISONED_ENVS), NF_CAND] = False
    for i, (a, b) in enumerate(zip(got, clean)):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a[mask], b[mask], equal_nan=True), (where, i)


def poisoned_rows_follow_the_oracle(name, os_, cand, out, solved, where):
    """out = (reward, info, status, iterations, vm_pu) of a call with the poisoned candidates `cand`"""
    reward, info, st, it, vm = out
    for e in POISONED_ENVS:
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")                       # (the oracle's sparse solve on a NaN Jacobian)
            p = W.predict(name, os_[e], cand[e, NF_CAND])
        w = (where, e)
        assert p["solved"] == solved and st[e, NF_CAND] == (W.SOLVED if solved else W.PF_FAILED), w
        assert agrees(reward[e, NF_CAND], p["reward"]) and agrees(info[e, NF_CAND], p["info"]), (w, reward[e, NF_CAND], p["reward"], info[e, NF_CAND], p["info"])
        if solved:
            assert it[e, NF_CAND] == p["iterations"] or W.newton_count_agrees(name, p, it[e, NF_CAND], True), w
            assert np.abs(vm[e, NF_CAND] - p["vm"]).max() <= V_TOL, w
        else:
            assert W.newton_count_agrees(name, p, it[e, NF_CAND], False), (w, it[e, NF_CAND], p["iterations"])
            assert np.isnan(vm[e, NF_CAND]).all() and info[e, NF_CAND, 10] == 1.0 and np.isfinite(reward[e, NF_CAND]), w


def poisoned(cand, j, value):
    c = cand.copy()
    c[list(POISONED_ENVS), NF_CAND, j] = value
    return c


@pytest.mark.parametrize("name,j,on_slack", [("crowded", 0, False), ("crowded", 2, True), ("special", 0, False), ("special", 8, True)],
                         ids=["crowded-ordinary", "crowded-slack", "special-ordinary", "special-slack"])
def test_non_finite_candidates_action_gradients(name, j, on_slack):
    """An ordinary sgen: status 2, the oracle's reward, infos and Newton count, a NaN gradient row and a NaN |V| row.  The sgen on the slack
    bus, whose injection no solve reads: status 0, the oracle's reward and q_loss (NaN, -inf), and — k_action_grad's rule for a row in
    which some lim_j a_j is not finite — a NaN gradient row (sign0(NaN) = 0 would otherwise report a stationary point); 1e300 there leaves
    lim_j a_j finite: the row keeps its gradient, the direct term in entry j and the bits of the clean call in the others."""
    os_, ref, full = G.reference(name, W.B_MAX, W.K_MAX)
    net = os_[0].net
    assert (int(net.sgen_bus[j]) == int(net.ext_grid_bus)) == on_slack
    cand = np.ascontiguousarray(full[:NF_B, :NF_K])
    env = make_env(name, NF_B)
    try:
        scenario_random(env, name)
        clean = gradients(env, poisoned(cand, j, 0.0))
        assert (clean[3] == np.where(W.expected_pattern(NF_K), W.SOLVED, W.PF_FAILED)).all()
        for value in POISON:
            c = poisoned(cand, j, value)
            got = gradients(env, c)
            where = (name, j, value)
            others_keep_their_bits(got, clean, where)
            same_bits(got[1:], evaluate(env, c), "reward, info, status, iterations, vm_pu as evaluate_actions")
            poisoned_rows_follow_the_oracle(name, os_, c, got[1:], on_slack, where)
            rows = got[0][list(POISONED_ENVS), NF_CAND]
            if on_slack and np.isfinite(value):                   # 1e300: q_j = lim_j 1e300 is finite
                keep = [i for i in range(net.n_sgen) if i != j]
                assert np.isfinite(rows).all() and np.array_equal(rows[:, keep], clean[0][list(POISONED_ENVS), NF_CAND][:, keep]), where
                for r, e in zip(rows, POISONED_ENVS):
                    lim, s = G.limits(os_[e])[j], net.sgen_scaling[j]
                    want = -os_[e].q_weight / net.n_sgen * lim * s
                    assert abs(r[j] - want) <= 4 * ULP * abs(want), (where, e)
            else:
                assert np.isnan(rows).all(), where
                if on_slack:
                    rw = got[1][list(POISONED_ENVS), NF_CAND]
                    assert np.isnan(rw).all() if np.isnan(value) else (rw == -np.inf).all(), where
        same_bits(gradients(env, poisoned(cand, j, 0.0)), clean, "the clean call after the poisoned ones")
    finally:
        env.close()


@pytest.mark.parametrize("name,tuning,solver,j,on_slack", [("crowded_meshed", None, 1, 0, False), ("crowded_meshed", None, 1, 2, True),
                                                           ("one_sgen", dict(nr_solver="dense"), 2, 0, False),
                                                           ("crowded_zip", None, 0, 0, False), ("crowded_zip", None, 0, 2, True)],
                         ids=["sparse-ordinary", "sparse-slack", "dense-ordinary", "zip-ordinary", "zip-slack"])
def test_non_finite_candidates_evaluate_actions(name, tuning, solver, j, on_slack):
    """the same on k_nr_sparse, on a handle pinned to k_nr_dense and with ZIP loads on the tree solver"""
    os_, ref = W.reference(name)
    net = os_[0].net
    assert (int(net.sgen_bus[j]) == int(net.ext_grid_bus)) == on_slack
    cand = W.candidates(name, NF_B, NF_K)
    env = make_env(name, NF_B, tuning=tuning)
    try:
        assert env.nr_kernel()["solver"] == solver
        scenario_random(env, name)
        clean = evaluate(env, poisoned(cand, j, 0.0))
        assert (clean[2] == np.where(W.expected_pattern(NF_K), W.SOLVED, W.PF_FAILED)).all()
        for value in POISON:
            c = poisoned(cand, j, value)
            got = evaluate(env, c)
            others_keep_their_bits(got, clean, (name, j, value))
            poisoned_rows_follow_the_oracle(name, os_, c, got, on_slack, (name, j, value))
        same_bits(evaluate(env, poisoned(cand, j, 0.0)), clean, "the clean call after the poisoned ones")
    finally:
        env.close()


# ---- call order ---------------------------------------------------------------------------------------------------------------------------
def _arrays(out):
    vals = out.values() if isinstance(out, dict) else out
    return [v.detach().cpu().numpy() for v in vals]


def test_call_order_on_one_handle():
    """The six calls share one handle's Sbus region and Vout rows, and pairwise the tree tables and the what-if workspace.  On case33 at
    B = 24 after a reset and two random steps: each call's outputs in the order of CALLS, then in reverse, then once more after a solve()
    that leaves Sbus stale — every time the bits of that call made first on a fresh twin handle in the same state; afterwards the handle's
    snapshot is a twin's and one step() on both gives the same bits."""
    name, B = "case33", 24
    cand = torch.as_tensor(W.candidates(name, B, 3), device=DEV)
    a = cand[:, 1].contiguous()
    CALLS = [("droop_actions", lambda env: env.droop_actions(vm_pu=True)), ("opf_actions", lambda env: env.opf_actions(vm_pu=True)),
             ("opf_probe", lambda env: env.opf_probe(a)), ("evaluate_actions", lambda env: env.evaluate_actions(cand, vm_pu=True)),
             ("action_gradients", lambda env: env.action_gradients(cand, vm_pu=True)),
             ("difference_rewards", lambda env: env.difference_rewards(a))]

    def state(env, stale):
        env.reset()
        rng = np.random.default_rng(3)
        for _ in range(2):
            env.step(torch.as_tensor(rng.uniform(-0.8, 0.8, (B, env.n_sgen)), device=DEV))
        if stale:
            lp, lq, pv, _ = BC.env_state(env)
            env.solve(lp * 1.3, lq, pv, np.zeros_like(pv))

    def fresh(stale):
        """the outputs of every call, each as the first call of a fresh twin"""
        out = {}
        for key, call in CALLS:
            twin = make_env(name, B)
            try:
                state(twin, stale)
                got = call(twin)
                torch.cuda.synchronize()
                if key == "opf_probe":                            # (rows that were not linearised are unspecified)
                    assert bool(got["linearised"].all())
                out[key] = _arrays(got)
            finally:
                twin.close()
        return out

    A, T = make_env(name, B), make_env(name, B)
    try:
        state(A, False)
        want = fresh(False)
        for order in (CALLS, CALLS[::-1]):
            for key, call in order:
                same_bits(_arrays(call(A)), want[key], (key, "first" if order is CALLS else "reversed"))
        lp, lq, pv, _ = BC.env_state(A)
        A.solve(lp * 1.3, lq, pv, np.zeros_like(pv))
        want = fresh(True)
        for key, call in CALLS:
            same_bits(_arrays(call(A)), want[key], (key, "after a solve"))
        state(T, True)
        BC.same(BC.snapshot(A), BC.snapshot(T))
        r1, t1, i1 = [x.clone() for x in A.step(a)]
        r2, t2, i2 = [x.clone() for x in T.step(a)]
        assert torch.equal(r1, r2) and torch.equal(t1, t2) and torch.equal(i1, i2) and torch.equal(A.get_obs(), T.get_obs())
    finally:
        A.close(); T.close()
