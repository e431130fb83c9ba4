"""GPU (-m gpu): action_gradients (mapdn_action_gradients; k_action_grad between the solve and k_whatif_score of the what-if frame;
DESIGN.md section 22) — d reward / d action of K candidate actions of every env.

The reference is tests/grad_ref.py carried above float64 (longdouble assembly, refined solve), evaluated at the kernel's own |V| with the
oracle's angles; the bar is tests/opf_kernel_cases.py's rule, 16 x the float64 reference's own error on the case and never below 64 ulp,
relative to the row's largest entry.  From a reset and one random step the candidates {0, random, UNSOLVABLE, random, ...} come out
solved, solved, unsolvable, solved, ... in every env of every net; every test asserts that pattern of the oracle before it compares.

Shapes: nets of 9 to 33 buses at B = 1, 5, 17, 33 and K = 1, 4, 7 (a workgroup of k_action_grad is 64 envs: all of them partial)."""
import numpy as np
import pytest
import torch

from mapdn_amd import _lib
from mapdn_amd.env import VoltageControl, VoltageControlBatch
from oracle.pp_restated import runpp_restated
from tests import grad_ref as G
from tests import element_edge_nets as N
from tests import opf_kernel_cases as OK
from tests import whatif_cases as W
from tests.baseline_contract import check_state_untouched_and_step_agrees
from tests.test_zip_loads_gpu import V_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KERNELS = ["k_action_grad"]                                   # every parity test runs it: action_gradients has no other path
ULP = np.finfo(np.float64).eps


def make_env(name, B, tuning=None, env_id_offset=0, **args):
    net, prof, base = G.make(name)
    return VoltageControlBatch(net, prof, dict(base, **args), n_envs=B, device=DEV, obs_dtype=torch.float64, tuning=tuning,
                               env_id_offset=env_id_offset)


def scenario(env, name, first=0):
    """reset and the one random step of G.reference (first: the env id of env 0)"""
    env.reset()
    a0 = G.first_action(name, first + env.n_envs)[first:]
    _, term, info = env.step(torch.as_tensor(a0, device=DEV))
    assert env.stats()["reset_failures"] == 0 and not bool(term.any()) and float(info[:, 10].max()) == 0.0


def gradients(env, cand):
    """action_gradients(cand, vm_pu=True) as numpy: (grad, reward, info, status, iterations, vm_pu)"""
    out = env.action_gradients(torch.as_tensor(cand, device=DEV), vm_pu=True)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


def evaluate(env, cand):
    out = env.evaluate_actions(torch.as_tensor(cand, device=DEV), vm_pu=True)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


def same_bits(x, y, where=""):
    for i, (a, b) in enumerate(zip(x, y)):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (where, i)


def compare(name, args, got, os_, ref, cand, B, K, skip=(), init="flat"):
    """grad rows (e, k) of a call against the extended reference at the kernel's |V| and the oracle's angles (init: of the oracle's power
    flow from that start — two starts end a rounding of the Newton tolerance apart); status, |V| and NaN rows"""
    grad, reward, info, st, it, vm = got
    ns = os_[0].net.n_sgen
    assert grad.shape == (B, K, ns) and grad.dtype == np.float64 and st.shape == (B, K) and st.dtype == np.uint8
    worst = 0.0
    bar = G.bar(name, args)
    for e in range(B):
        if e in skip:
            assert (st[e] == W.NOT_EVALUATED).all() and np.isnan(grad[e]).all() and np.isnan(reward[e]).all(), e
            continue
        for k in range(K):
            p, w = ref["rows"][e][k], (name, args, B, K, e, k)
            assert st[e, k] == (W.SOLVED if p["solved"] else W.PF_FAILED), w
            if not p["solved"]:
                assert np.isnan(grad[e, k]).all() and np.isnan(vm[e, k]).all() and reward[e, k] < -200.0, w
                continue
            assert np.isfinite(grad[e, k]).all() and np.abs(vm[e, k] - p["vm"]).max() <= V_TOL, w
            if e not in OK.ref_envs(B):
                continue
            o = os_[e]
            r = p["r"] if init == "flat" else runpp_restated(o.net, *p["inputs"], init=init)
            assert r.converged
            V = vm[e, k] * np.exp(1j * np.angle(r.V))
            ext = G.reward_gradient(o.net, G.env_args(o), V, cand[e, k], G.limits(o), ext=True)
            err = G.rel_inf(grad[e, k], ext)
            worst = max(worst, err)
            assert err <= bar, (w, err, bar)
    print(f"\n[grad gpu] {name} {dict(args)} B={B} K={K}: e64 {G.E64[(name, tuple(args))]:.2e} gpu {worst:.2e} bar {bar:.2e}")
    return worst


def assert_pattern(ref, B, K):
    assert (ref["solved"][:B, :K] == W.expected_pattern(K)).all()


# ---- parity -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 17, 33])
@pytest.mark.parametrize("name", G.NETS)
def test_against_the_extended_reference(name, B):
    """one sgen, 17 sgens, the transformer / shunt / scalings / four-child junction / slack-bus sgen of `special`, two sgens on one bus
    and an sgen beside a load on the ext_grid bus (`crowded`), a net of PV buses only, the shipped case33; K = 1, 4, 7 on one handle, one
    call after the other"""
    assert W.global_kernels("grad.hip") == KERNELS
    os_, ref, cand = G.reference(name, W.B_MAX, W.K_MAX)
    env = make_env(name, B)
    try:
        assert env.nr_kernel()["solver"] == 0
        scenario(env, name)
        for K in (1, 4, 7):
            assert_pattern(ref, B, K)
            c = np.ascontiguousarray(cand[:B, :K])
            compare(name, (), gradients(env, c), os_, ref, c, B, K)
    finally:
        env.close()


VARIANTS = [(("voltage_barrier_type", b),) for b in G.BARRIER_TYPES if b != "bowl"] + [G.LINE_ARGS]


@pytest.mark.parametrize("args", VARIANTS, ids=lambda a: "-".join(str(v) for _, v in a))
@pytest.mark.parametrize("name", ["crowded", "special"])
def test_barrier_types_and_line_weight(name, args):
    """(bowl is the barrier of every other test)"""
    B, K = G.VARIANT_SHAPE
    os_, ref, cand = G.reference(name, B, K, args)
    assert_pattern(ref, B, K)
    env = make_env(name, B, **dict(args))
    try:
        scenario(env, name)
        got = gradients(env, cand)
        compare(name, args, got, os_, ref, cand, B, K)
        if args == G.LINE_ARGS:                               # no q term: the entry of an sgen on the ext_grid bus is exactly zero
            net = os_[0].net
            slack = [j for j, b in enumerate(net.sgen_bus) if int(b) == int(net.ext_grid_bus)]
            assert slack and (got[0][:, W.expected_pattern(K)][:, :, slack] == 0.0).all()
    finally:
        env.close()


def test_dc_start_is_accepted():
    name, B, K = "tiny", 5, 4
    os_, ref, cand = G.reference(name, W.B_MAX, W.K_MAX)
    env = make_env(name, B, tuning=dict(nr_init="dc"))
    try:
        assert env.geometry()["nr_init"] == 2
        scenario(env, name)
        c = np.ascontiguousarray(cand[:B, :K])
        compare(name, (), gradients(env, c), os_, ref, c, B, K, init="dc")
    finally:
        env.close()


# ---- exact zeros ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,j", [("special", 8), ("crowded", 2)])
def test_slack_bus_sgen_gets_the_direct_term_alone(name, j):
    """the power-flow part of an sgen on the ext_grid bus is exactly zero: its entry is -q_weight sign(q) lim scaling / ns, which is 0 for
    the all-zero candidate and otherwise the oracle's figure to the rounding of lim (a square root of a difference: 4 ulp)"""
    B, K = 5, 4
    os_, ref, cand = G.reference(name, W.B_MAX, W.K_MAX)
    net = os_[0].net
    assert int(net.sgen_bus[j]) == int(net.ext_grid_bus)
    env = make_env(name, B)
    try:
        scenario(env, name)
        c = np.ascontiguousarray(cand[:B, :K])
        grad = gradients(env, c)[0]
        assert (grad[:, 0, j] == 0.0).all()
        for e in range(B):
            o = os_[e]
            lim, s = G.limits(o)[j], net.sgen_scaling[j]
            for k in (1, 3):
                want = -o.q_weight / net.n_sgen * np.sign(lim * c[e, k, j] * s) * lim * s
                assert abs(grad[e, k, j] - want) <= 4 * ULP * abs(want), (e, k, grad[e, k, j], want)
    finally:
        env.close()


# ---- status rows ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["frozen", "auto"])
def test_envs_that_step_would_not_solve(plan):
    """episode_limit 4, the plans of element_edge_nets.replay up to their forced unsolvable step: env 7 is then frozen ("frozen") or waits
    for its auto-reset restart ("auto") — status 3, NaN gradient —, candidate 2 of the others is status 2 with a NaN gradient, and the rest
    is what evaluate_actions reports; in the "frozen" plan one more step ends every episode at the episode limit: every row is status 3"""
    name, p = "crowded", N.PLANS[plan]
    env = make_env(name, N.B_WATCH, auto_reset=p["auto_reset"])
    try:
        steps = N.replay(name, plan)
        for kind, call, x, os_ in steps:
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
        got = gradients(env, cand)
        grad, st = got[0], got[3]
        live = [e for e in range(N.B_WATCH) if e != N.FORCED_ENV]
        assert (ref["solved"][live] == W.expected_pattern(K)).all()
        assert (st[N.FORCED_ENV] == W.NOT_EVALUATED).all() and np.isnan(grad[N.FORCED_ENV]).all()
        assert (st[live, 2] == W.PF_FAILED).all() and np.isnan(grad[live, 2]).all()
        assert (st[live][:, [0, 1, 3]] == W.SOLVED).all() and np.isfinite(grad[live][:, [0, 1, 3]]).all()
        same_bits(got[1:], evaluate(env, cand), "as evaluate_actions")
        for e in live[:3]:                                     # and the live rows are the reference's
            o = os_[e]
            for k in (0, 1, 3):
                V = got[5][e, k] * np.exp(1j * np.angle(ref["rows"][e][k]["r"].V))
                ext = G.reward_gradient(o.net, G.env_args(o), V, cand[e, k], G.limits(o), ext=True)
                assert G.rel_inf(grad[e, k], ext) <= G.bar(name), (e, k)
        if plan == "frozen":
            kind, call, x, os_ = next(steps)
            _, term, _ = env.step(torch.as_tensor(x[0], device=DEV))
            assert bool(term.all())                           # the episode limit
            got = gradients(env, cand)
            assert (got[3] == W.NOT_EVALUATED).all() and np.isnan(got[0]).all() and (got[4] == 0).all()
            same_bits(got[1:], evaluate(env, cand), "as evaluate_actions, every env frozen")
    finally:
        env.close()


# ---- bits -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["crowded", "special"])
def test_bits(name):
    B, K = 33, 7
    cand = G.candidates(name, B, K)
    env = make_env(name, B)
    try:
        scenario(env, name)
        full = gradients(env, cand)
        assert (full[3] == np.where(W.expected_pattern(K), W.SOLVED, W.PF_FAILED)).all()
        same_bits(full, gradients(env, cand), "two calls")
        same_bits(full[1:], evaluate(env, cand), "reward, info, status, iterations, vm_pu as evaluate_actions")
        for k in (1, 2, 6):                                   # K = 1 gives column k of K = 7
            alone = gradients(env, cand[:, k:k + 1])
            same_bits([a[:, 0] for a in alone], [a[:, k] for a in full], f"K = 1, candidate {k}")
        c32 = cand.astype(np.float32)                         # float32 actions: the same values widened
        g32 = gradients(env, c32)
        same_bits(g32, gradients(env, c32.astype(np.float64)), "float32")
        assert g32[0].dtype == np.float64
    finally:
        env.close()
    # an env alone at B = 1, and a batch that begins at env id 13: every env moves to another lane, and its bits move with it
    for first_id, n in ((20, 1), (13, 20)):
        other = make_env(name, n, env_id_offset=first_id)
        try:
            scenario(other, name, first=first_id)
            got = gradients(other, cand[first_id:first_id + n])
            same_bits(got, [a[first_id:first_id + n] for a in full], f"env ids from {first_id}, B = {n}")
        finally:
            other.close()


@pytest.mark.parametrize("after_solve", [False, True])
def test_state_untouched_and_step_agrees(after_solve):
    """tests/baseline_contract.py with candidate 1 of {0, random, UNSOLVABLE}: nothing a twin env does not have changes and step() with the
    candidate gives the twin's bits, also after a solve() that leaves Sbus stale"""
    name, k0 = "case33", 1

    def baseline(env):
        cand = torch.as_tensor(W.candidates(name, env.n_envs, 3), device=DEV)
        g, _, _, st, _, vm = env.action_gradients(cand, vm_pu=True)
        assert (st[:, 2] == W.PF_FAILED).all() and (st[:, k0] == W.SOLVED).any() and bool(torch.isfinite(g[:, k0][st[:, k0] == 0]).all())
        return cand[:, k0].contiguous(), st[:, k0], vm[:, k0]
    check_state_untouched_and_step_agrees(lambda B: make_env(name, B), baseline, after_solve, B=24)


# ---- the C ABI and the refusals on a live handle -----------------------------------------------------------------------------------------
def test_c_abi_refusals_on_a_live_handle():
    name, B, K = "tiny", 5, 2
    env = make_env(name, B)
    try:
        scenario(env, name)
        lib = _lib.load()
        a = torch.as_tensor(G.candidates(name, B, K), device=DEV)
        ns = env.n_sgen
        g = torch.empty(B, K, ns, dtype=torch.float64, device=DEV)
        r = torch.empty(B, K, dtype=torch.float64, device=DEV)
        inf = torch.empty(B, K, 11, dtype=torch.float64, device=DEV)
        st = torch.empty(B, K, dtype=torch.uint8, device=DEV)
        ok = [a.data_ptr(), 1, K, g.data_ptr(), r.data_ptr(), inf.data_ptr(), st.data_ptr(), None, None, None]
        for i, bad, word in ((0, None, "null buffer"), (3, None, "null buffer"), (6, None, "null buffer"), (1, 9, "dtype"), (2, 0, "n_candidates")):
            call = list(ok)
            call[i] = bad
            assert lib.mapdn_action_gradients(env._h, *call) == -1 and word in lib.mapdn_last_error(env._h).decode(), (i, bad)
        assert lib.mapdn_action_gradients(env._h, *ok) == 0    # iterations and vm_pu may be NULL
        torch.cuda.synchronize()
        same_bits((g.cpu().numpy(), r.cpu().numpy()), gradients(env, a.cpu().numpy())[:2], "the C call")
        with pytest.raises(ValueError):
            env.action_gradients(torch.zeros(B, K, ns + 1, device=DEV))
    finally:
        env.close()


@pytest.mark.parametrize("name,tuning,word", [("crowded_meshed", None, "meshed"), ("one_sgen", dict(nr_solver="dense"), "meshed"),
                                              ("crowded_zip", None, "ZIP"), ("crowded_fused", None, "fused")])
def test_python_refusals_on_a_live_handle(name, tuning, word):
    net, prof, base = W.make(name)
    env = VoltageControlBatch(net, prof, dict(base), n_envs=3, device=DEV, obs_dtype=torch.float64, tuning=tuning)
    try:
        env.reset()
        with pytest.raises(NotImplementedError, match=word):
            env.action_gradients(torch.zeros(3, 2, env.n_sgen, device=DEV))
        env.evaluate_actions(torch.zeros(3, 2, env.n_sgen, device=DEV))      # (which covers these handles)
    finally:
        env.close()


# ---- the drop-in ----------------------------------------------------------------------------------------------------------------------------
def test_drop_in():
    """VoltageControl.action_gradients at B = 1 returns row 0 of the batch call"""
    name = "crowded"
    net, prof, base = W.make(name)
    cand = W.candidates(name, 1, 3)
    one = VoltageControl(dict(base, net=net, profiles=prof), device=DEV)
    batch = make_env(name, 1)
    try:
        batch.reset()
        want = gradients(batch, cand)
        g, rewards, infos, status = one.action_gradients(cand[0])
        assert isinstance(g, np.ndarray) and g.shape == (3, net.n_sgen) and rewards.shape == (3,) and len(infos) == 3
        same_bits((g, rewards, status), (want[0][0], want[1][0], want[3][0]), "row 0 of the batch call")
        assert list(status) == [W.SOLVED, W.SOLVED, W.PF_FAILED] and np.isnan(g[2]).all() and np.isfinite(g[:2]).all()
    finally:
        one.close()
        batch.close()
