"""GPU (-m gpu): evaluate_actions (mapdn_evaluate_actions; k_whatif_start, k_whatif_score around the handle's own solver in MODE_SOLVE;
DESIGN.md section 20) — the reward, info, status, Newton count and |V| that step() would report for K candidate actions of every env,
without the step.

The reference is the oracle env (oracle/env_restated.py through tests/whatif_cases.py): a shallow copy of an oracle stepped with the
candidate.  From a reset and one random step the candidates {0, random, UNSOLVABLE, random, ...} come out solved, solved, unsolvable,
solved, ... in every env of every net; every test asserts that pattern of the oracle before it compares, so nothing hides behind
"unsolvable on both sides".  Bounds are the project's own for step(): 1e-9 on reward and info, V_TOL of tests/test_zip_loads_gpu.py on |V|,
status exact, the Newton count exact or one apart at the tolerance edge (tests/edge_rule.py).

Shapes: the six nets of tests/element_edge_nets.py (13 to 19 buses) at B = 1, 5, 17, 33 — a lone env, a partial 16-lane group, one group
plus one env, two groups plus one — and K = 1, 4, 7."""
import numpy as np
import pytest
import torch

from mapdn_amd.env import VoltageControl, VoltageControlBatch
from oracle.env_restated import INFO_KEYS, VoltageControlOracle
from tests import element_edge_nets as N
from tests import whatif_cases as W
from tests.baseline_contract import check_state_untouched_and_step_agrees
from tests.test_zip_loads_gpu import V_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-9
# step() after evaluate_actions against the predicted row: both solve the same Sbus bits, the statistics are summed in different orders
# (the solver's workers there, 16 sub-lanes here).  Measured on an MI355X over the six nets, case33 and case141: the
# largest |difference| is 4.441e-16 (average_voltage, two ulp), of the reward 2.8e-17; the bar is ten times that, and never above 1e-9.
STEP_MEASURED = 4.441e-16
STEP_TOL = min(10 * STEP_MEASURED, 1e-9)
COUNT_INFOS = (0, 1, 2, 10)                                   # the three count-based infos and destroy: exact
assert W.KERNELS == {"k_whatif_start", "k_whatif_score"}      # (tests/test_whatif_cpu.py holds this list to csrc/whatif.hip)


def make_env(name, B, tuning=None, env_id_offset=0, **args):
    net, prof, base = W.make(name)
    return VoltageControlBatch(net, prof, dict(base, **args), n_envs=B, device=DEV, obs_dtype=torch.float64, tuning=tuning,
                               env_id_offset=env_id_offset)


def scenario(env, name, first=0):
    """reset and the one random step of W.reference (first: the env id of env 0)"""
    env.reset()
    a0 = W.first_action(name, first + env.n_envs)[first:]
    _, term, info = env.step(torch.as_tensor(a0, device=DEV))
    assert env.stats()["reset_failures"] == 0 and not bool(term.any()) and float(info[:, 10].max()) == 0.0


def evaluate(env, cand):
    """evaluate_actions(cand, vm_pu=True) as numpy: (reward, info, status, iterations, vm_pu)"""
    out = env.evaluate_actions(torch.as_tensor(cand, device=DEV), vm_pu=True)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


def same_bits(x, y, where=""):
    for i, (a, b) in enumerate(zip(x, y)):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), (where, i)


def assert_pattern(ref, B, K):
    """the oracle alone: solved, solved, unsolvable (reward about -200.1, destroy 1), solved, ..."""
    assert (ref["solved"][:B, :K] == W.expected_pattern(K)).all()
    if K > 2:
        assert (ref["reward"][:B, 2] < -200.0).all() and (ref["reward"][:B, 2] > -201.0).all() and (ref["info"][:B, 2, 10] == 1.0).all()
    assert (ref["info"][:B, :K, 10][:, W.expected_pattern(K)] == 0.0).all()


def compare(name, got, ref, B, K, skip=()):
    """rows (e, k) of a call against the oracle's prediction (its leading B x K rows)"""
    reward, info, st, it, vm = got
    assert reward.shape == (B, K) and info.shape == (B, K, len(INFO_KEYS)) and st.shape == (B, K) and it.shape == (B, K)
    assert st.dtype == np.uint8 and it.dtype == np.int32 and vm.shape[:2] == (B, K)
    worst = dict(reward=0.0, info=0.0, vm=0.0)
    for e in range(B):
        if e in skip:
            assert (st[e] == W.NOT_EVALUATED).all() and (it[e] == 0).all(), e
            assert np.isnan(reward[e]).all() and np.isnan(info[e]).all() and np.isnan(vm[e]).all(), e
            continue
        for k in range(K):
            p, w = ref["rows"][e][k], (name, B, K, e, k)
            assert st[e, k] == (W.SOLVED if p["solved"] else W.PF_FAILED), w
            worst["reward"] = max(worst["reward"], abs(reward[e, k] - p["reward"]))
            worst["info"] = max(worst["info"], float(np.abs(info[e, k] - p["info"]).max()))
            assert abs(reward[e, k] - p["reward"]) <= TOL, (w, reward[e, k], p["reward"])
            assert np.abs(info[e, k] - p["info"]).max() <= TOL, (w, info[e, k] - p["info"])
            if p["solved"]:
                worst["vm"] = max(worst["vm"], float(np.abs(vm[e, k] - p["vm"]).max()))
                assert np.abs(vm[e, k] - p["vm"]).max() <= V_TOL, w
            else:
                assert np.isnan(vm[e, k]).all(), w
            assert W.newton_count_agrees(name, p, it[e, k], st[e, k] == W.SOLVED), (w, it[e, k], p["iterations"])
    print(f"\n[whatif] {name} B={B} K={K}: " + " ".join(f"{k}={v:.1e}" for k, v in worst.items()))
    return worst


# ---- against the oracle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 17, 33])
@pytest.mark.parametrize("name", N.NETS)
def test_against_the_oracle(name, B):
    """k_whatif_start and k_whatif_score on every net of tests/element_edge_nets.py: sgens sharing a bus, an sgen on the ext_grid bus, fused
    twins (alias rows), ZIP loads, a tie line on k_nr_sparse, scalings 0 / < 1 / > 1, odd counts; K = 1, 4, 7 on one handle, one after the
    other — which also shows that a call leaves the state the next call starts from alone"""
    os_, ref = W.reference(name)
    env = make_env(name, B)
    try:
        assert env.nr_kernel()["solver"] == (1 if name == "crowded_meshed" else 0)
        scenario(env, name)
        for K in (1, 4, 7):
            assert_pattern(ref, B, K)
            compare(name, evaluate(env, W.candidates(name, B, K)), ref, B, K)
    finally:
        env.close()


CASE33_ARGS = [(("voltage_barrier_type", b),) for b in ("l1", "l2", "courant_beltrami", "bowl", "bump")] + \
              [(("line_weight", 0.7), ("q_weight", None))]


@pytest.mark.parametrize("args", CASE33_ARGS, ids=lambda a: "-".join(str(v) for _, v in a))
def test_case33_barriers_and_line_weight(args):
    B, K = 17, 3
    os_, ref = W.reference("case33", B, K, args)
    assert_pattern(ref, B, K)
    env = make_env("case33", B, **dict(args))
    try:
        scenario(env, "case33")
        compare("case33", evaluate(env, W.candidates("case33", B, K)), ref, B, K)
    finally:
        env.close()


def test_dense_solver():
    """a small net pinned to k_nr_dense: the handle's own solver, whatever it is"""
    name, B, K = "one_sgen", 5, 4
    os_, ref = W.reference(name)
    assert_pattern(ref, B, K)
    env = make_env(name, B, tuning=dict(nr_solver="dense"))
    try:
        assert env.nr_kernel()["solver"] == 2
        scenario(env, name)
        compare(name, evaluate(env, W.candidates(name, B, K)), ref, B, K)
    finally:
        env.close()


# ---- state untouched and the step agrees ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("after_solve", [False, True])
@pytest.mark.parametrize("name,args", [("case33", {}), ("crowded_meshed", {}), ("crowded", dict(auto_reset=True))],
                         ids=["case33", "crowded_meshed", "crowded-auto_reset"])
def test_state_untouched_and_step_agrees(name, args, after_solve):
    """tests/baseline_contract.py with candidate 1 of {0, random, UNSOLVABLE}: nothing a twin env does not have changes, step() with the
    candidate gives the twin's bits (also after a solve() that leaves Sbus stale), and the committed |V| are the returned ones at 1e-12"""
    k0 = 1

    def baseline(env):
        cand = torch.as_tensor(W.candidates(name, env.n_envs, 3), device=DEV)
        _, _, st, _, vm = env.evaluate_actions(cand, vm_pu=True)
        assert (st[:, 2] == W.PF_FAILED).all() and (st[:, k0] == W.SOLVED).any()
        return cand[:, k0].contiguous(), st[:, k0], vm[:, k0]
    check_state_untouched_and_step_agrees(lambda B: make_env(name, B, **args), baseline, after_solve, B=24)


# ---- the step reports what was predicted ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(N.NETS) + ["case33", "case141"])
def test_step_reports_what_was_predicted(name):
    """evaluate_actions, then step() with candidate 1 — in env 2 with the UNSOLVABLE candidate — against the predicted rows"""
    B, K, e_uns = 17, 3, 2
    os_, ref = W.reference(name) if name in N.NETS else W.reference(name, B, K)
    assert_pattern(ref, B, K)
    assert W.band_margin(dict(vm=ref["vm"][:B, :K], solved=ref["solved"][:B, :K])) > 1e-9   # no count can flip on a rounding
    env = make_env(name, B)
    try:
        scenario(env, name)
        cand = W.candidates(name, B, K)
        reward, info, st, it, vm = evaluate(env, cand)
        pick = np.full(B, 1)
        pick[e_uns] = 2
        rows = np.arange(B)
        r, term, inf = env.step(torch.as_tensor(cand[rows, pick], device=DEV))
        r, term, inf = r.cpu().numpy(), term.cpu().numpy(), inf.cpu().numpy()
        assert (st[rows, pick] == np.where(rows == e_uns, W.PF_FAILED, W.SOLVED)).all()
        assert bool(term[e_uns]) and inf[e_uns, 10] == 1.0 and r[e_uns] < -200.0
        dr, di = np.abs(r - reward[rows, pick]), np.abs(inf - info[rows, pick])
        print(f"\n[whatif step] {name}: reward {dr.max():.3e} info " + " ".join(f"{x:.1e}" for x in di.max(0)))
        assert dr.max() <= STEP_TOL and di.max() <= STEP_TOL, (dr.max(), di.max(0))
        assert (di[:, COUNT_INFOS] == 0.0).all()
        ok = rows != e_uns
        committed = env.results(("vm_pu",))["vm_pu"].cpu().numpy()
        assert np.abs(committed[ok] - vm[rows, pick][ok]).max() < 1e-12
    finally:
        env.close()


# ---- bits -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["crowded", "crowded_meshed"])
def test_bits(name):
    B, K = 33, 7
    cand = W.candidates(name, B, K)
    env = make_env(name, B)
    try:
        scenario(env, name)
        full = evaluate(env, cand)
        assert (full[2] == np.where(W.expected_pattern(K), W.SOLVED, W.PF_FAILED)).all()
        same_bits(full, evaluate(env, cand), "two calls")
        # candidate 1 alone, as the first of 7 and as the last of 7
        alone = evaluate(env, cand[:, 1:2])
        first = evaluate(env, cand[:, [1, 0, 2, 3, 4, 5, 6]])
        last = evaluate(env, cand[:, [0, 6, 2, 3, 4, 5, 1]])
        for x in (alone, first):
            same_bits([a[:, 0] for a in x], [a[:, 1] for a in full], "K = 1 / first of 7")
        same_bits([a[:, 6] for a in last], [a[:, 1] for a in full], "last of 7")
        # the neighbours of the unsolvable candidate, in a call without it
        keep = [0, 1, 3, 4, 5, 6]
        same_bits(evaluate(env, cand[:, keep]), [a[:, keep] for a in full], "without the unsolvable candidate")
        # float32 actions against the float64 call on the same values widened
        c32 = cand.astype(np.float32)
        same_bits(evaluate(env, c32), evaluate(env, c32.astype(np.float64)), "float32")
    finally:
        env.close()
    # an env alone at B = 1, and a batch that begins at env id 13: env id 20 moves from lane 4 of workgroup 1 to lane 7 of workgroup 0
    for first_id, n in ((20, 1), (13, 20)):
        other = make_env(name, n, env_id_offset=first_id)
        try:
            scenario(other, name, first=first_id)
            got = evaluate(other, cand[first_id:first_id + n])
            same_bits(got, [a[first_id:first_id + n] for a in full], f"env ids from {first_id}, B = {n}")
        finally:
            other.close()


# ---- envs that do not run ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["frozen", "auto"])
@pytest.mark.parametrize("name", ["crowded", "all_pv"])
def test_envs_that_step_would_not_solve(name, plan):
    """episode_limit 4, the plans of element_edge_nets.replay up to their forced unsolvable step: env 7 is then frozen ("frozen") or waits for
    its auto-reset restart ("auto") — status 3, NaN rows, 0 iterations —, and the others are held to the oracle as ever"""
    p = N.PLANS[plan]
    env = make_env(name, N.B_WATCH, auto_reset=p["auto_reset"])
    try:
        for kind, call, x, os_ in N.replay(name, plan):
            if kind == "reset":
                env.reset()
                continue
            _, term, _ = env.step(torch.as_tensor(x[0], device=DEV))
            if call == p["forced_call"]:
                break
        term = term.cpu().numpy()
        assert bool(term[N.FORCED_ENV]) and int(term.sum()) == 1
        K = 4
        cand = W.candidates(name, N.B_WATCH, K)
        ref = W.predict_all(name, os_, cand, skip={N.FORCED_ENV})
        live = [e for e in range(N.B_WATCH) if e != N.FORCED_ENV]
        assert (ref["solved"][live] == W.expected_pattern(K)).all()
        got = evaluate(env, cand)
        compare(name, got, ref, N.B_WATCH, K, skip={N.FORCED_ENV})
        same_bits(got, evaluate(env, cand), "two calls")
    finally:
        env.close()


# ---- difference rewards, the drop-in ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B", [("case33", 5), ("one_sgen", 3)])
def test_difference_rewards(name, B):
    os_ = (W.reference(name) if name in N.NETS else W.reference(name, 17, 3))[0][:B]
    a = W.candidates(name, B, 2)[:, 1]
    env = make_env(name, B)
    try:
        scenario(env, name)
        for default in (0.0, 0.3):
            r, diff, st = env.difference_rewards(torch.as_tensor(a, device=DEV), default=default)
            assert r.shape == (B,) and diff.shape == (B, env.n_agents) and st.shape == (B, env.n_agents + 1) and bool((st == 0).all())
            r, diff = r.cpu().numpy(), diff.cpu().numpy()
            for e, o in enumerate(os_):
                r0 = W.predict(name, o, a[e])
                assert r0["solved"] and abs(r[e] - r0["reward"]) <= TOL
                for i in range(env.n_agents):
                    ai = a[e].copy()
                    ai[i] = default
                    ri = W.predict(name, o, ai)
                    assert ri["solved"] and abs(diff[e, i] - (r0["reward"] - ri["reward"])) <= 2e-9, (e, i, default)
    finally:
        env.close()


def test_drop_in():
    """VoltageControl.evaluate_actions at B = 1: the oracle's three rewards and info dicts, then step() goes on as if nothing had been asked"""
    name = "crowded"
    net, prof, base = W.make(name)
    env = VoltageControl(dict(base, net=net, profiles=prof), device=DEV)
    try:
        o = VoltageControlOracle(net, prof, dict(base), env_id=0)
        cand = W.candidates(name, 1, 3)[0]
        rewards, infos, status = env.evaluate_actions(cand)
        assert rewards.shape == (3,) and list(status) == [W.SOLVED, W.SOLVED, W.PF_FAILED] and len(infos) == 3
        for k in range(3):
            p = W.predict(name, o, cand[k])
            assert abs(rewards[k] - p["reward"]) <= TOL and set(infos[k]) == set(INFO_KEYS)
            assert max(abs(infos[k][key] - p["info"][c]) for c, key in enumerate(INFO_KEYS)) <= TOL, k
        r, term, info = env.step(cand[1])
        ro, to, io = o.step(cand[1])
        assert abs(r - ro) <= TOL and term == to and max(abs(info[k] - io[k]) for k in INFO_KEYS) <= TOL
    finally:
        env.close()
