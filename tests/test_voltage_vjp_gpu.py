"""GPU (-m gpu): voltage_vjp (mapdn_voltage_vjp; k_voltage_vjp between the solve and k_whatif_score of the what-if frame, k_vjp_mask after
the last candidate) — M cotangents over the bus voltages of K candidate actions of every env, times the Jacobian of
those voltages by the actions.  Every call goes through the C ABI with every output between guard zones.

The reference is tests/vjp_ref.py carried above float64, evaluated at the kernel's own |V| with the oracle's angles; the bar is
tests/opf_kernel_cases.py's rule, 16 x the float64 reference's own error on the case and never below 64 ulp, relative to the row's largest
entry.  The scenario is tests/grad_edge_nets.py's: reset, one random step, then the candidates {0, random, UNSOLVABLE}: solved, solved,
unsolvable on every env; the oracle asserts that pattern on the reference envs (0-2, 62-65, 127-129) before anything is compared, and the
kernel's statuses hold it on every env.

Shapes: B = 1, 64, 65, 130 (a lane alone, a full wave of the 64-env workgroup, the tail of a second one, a third one); K = 1 and 3;
M = 0, 1, 2 and 5 (a unit cotangent on one |V|, one on one angle, |V| alone, and two random rows among them)."""
import functools

import numpy as np
import pytest
import torch

from mapdn_amd import _lib
from mapdn_amd.env import VoltageControl, VoltageControlBatch
from oracle.env_restated import VoltageControlOracle
from tests import baseline_contract as BC
from tests import grad_edge_nets as EN
from tests import grad_ref as G
from tests import opf_kernel_cases as OK
from tests import vjp_ref as VR
from tests import whatif_cases as W
from tests.test_action_grad_gpu import DEV, evaluate, make_env, same_bits
from tests.test_sparse_tables_gpu import Guarded
from tests.test_zip_loads_gpu import V_TOL

pytestmark = pytest.mark.gpu

KERNELS = ["k_voltage_vjp", "k_vjp_mask"]                       # the parity tests run both: every call asks for vm_pu
NETS = ("pair", "chain40", "star12", "feeders3", "ties", "tiny", "case33")
BATCHES = (1, 64, 65, 130)
B_MAX, K, M = 130, 3, 5
REF_ENVS = (0, 1, 2, 62, 63, 64, 65, 127, 128, 129)
VA_TOL = 1e-9 * 180.0 / np.pi                                   # 1e-9 rad, in degrees
PATTERN = np.array([W.SOLVED, W.SOLVED, W.PF_FAILED], np.uint8)


# ---- the scenario ---------------------------------------------------------------------------------------------------------------------------
def first_action(name):
    if name in EN.NETS:
        return EN.first_action(name, B_MAX)
    ns = G.make(name)[0].n_sgen
    return np.random.default_rng(11 + sum(map(ord, name))).uniform(-0.8, 0.8, (B_MAX, ns))


@functools.lru_cache(maxsize=None)
def candidates(name):
    """[B_MAX, K, ns]: {0, random, UNSOLVABLE} of every env"""
    if name in EN.NETS:
        return EN.candidates(name, B_MAX, K)
    ns = G.make(name)[0].n_sgen
    c = np.random.default_rng(23 + sum(map(ord, name))).uniform(-0.8, 0.8, (B_MAX, K, ns))
    c[:, 0] = 0.0
    c[:, 2] = W.UNSOLVABLE
    return c


@functools.lru_cache(maxsize=None)
def cots(name):
    """(cot_vm, cot_va) [B_MAX, K, M, n_bus]: row 0 random in both, row 1 a unit cotangent on the last non-slack bus's |V|, row 2 on the
    first non-slack bus's angle, row 3 |V| alone (cot_va zero), row 4 random in both"""
    net = G.make(name)[0]
    nb = net.n_bus
    pq = np.setdiff1d(np.arange(nb), [net.ext_grid_bus])
    rng = np.random.default_rng(97 + sum(map(ord, name)))
    cvm, cva = rng.uniform(-1.0, 1.0, (B_MAX, K, M, nb)), rng.uniform(-1.0, 1.0, (B_MAX, K, M, nb)) / 60.0
    cvm[:, :, 1:3], cva[:, :, 1:4] = 0.0, 0.0
    cvm[:, :, 1, pq[-1]] = 1.0
    cva[:, :, 2, pq[0]] = 1.0
    return cvm, cva


@functools.lru_cache(maxsize=None)
def oracle_rows(name):
    """{env id: (oracle env after the reset and the random step, [K] predictions)} of the reference envs; the pattern is asserted here, from
    the oracle alone"""
    if name in EN.NETS:
        os_, ref, cand = G.reference(name, REF_ENVS, K)
        assert np.array_equal(cand, candidates(name)[list(REF_ENVS)])
        rows = {e: (os_[i], ref["rows"][i]) for i, e in enumerate(REF_ENVS)}
    else:
        net, prof, base = G.make(name)
        a0, cand, rows = first_action(name), candidates(name), {}
        for e in REF_ENVS:
            o = VoltageControlOracle(net, prof, dict(base), env_id=e, do_reset=False)
            o.reset()
            _, term, info = o.step(a0[e])
            assert info["destroy"] == 0.0 and not term, (name, e)
            rows[e] = (o, [W.predict(name, o, cand[e, k]) for k in range(K)])
    for e, (o, row) in rows.items():
        assert [p["solved"] for p in row] == [True, True, False], (name, e)
    return rows


def scenario(env, name, first=0):
    B = env.n_envs
    if name in EN.NETS:
        env.reset(start_rows=torch.as_tensor(EN.start_rows(name, first + B)[first:], dtype=torch.int64))
    else:
        env.reset()
    _, term, info = env.step(torch.as_tensor(first_action(name)[first:first + B], device=DEV))
    assert env.stats()["reset_failures"] == 0 and not bool(term.any()) and float(info[:, 10].max()) == 0.0


# ---- the call -------------------------------------------------------------------------------------------------------------------------------
def vjp(env, cand, cvm=None, cva=None, m=None):
    """mapdn_voltage_vjp with every output between guard zones: (grad [B, K, M, ns] or None, vm_pu, va_degree, status, iterations).
    m: the number of cotangents when both are None (0: the voltages alone)"""
    a = torch.as_tensor(cand, device=DEV).contiguous()
    B, Kc, ns = a.shape
    assert (B, ns) == (env.n_envs, env.n_sgen)
    c = [None if x is None else torch.as_tensor(x, dtype=torch.float64, device=DEV).contiguous() for x in (cvm, cva)]
    Mc = m if m is not None else next(x for x in c if x is not None).shape[2]
    for x in c:
        assert x is None or x.shape == (B, Kc, Mc, env.n_bus)
    out = [Guarded((B, Kc, Mc, ns)) if Mc else None, Guarded((B, Kc, env.n_bus)), Guarded((B, Kc, env.n_bus)), Guarded((B, Kc), torch.uint8),
           Guarded((B, Kc), torch.int32)]
    with torch.cuda.device(env.device):
        _lib.check(env._lib.mapdn_voltage_vjp(env._h, a.data_ptr(), env._code(a.dtype), Kc, Mc, *[None if x is None else x.data_ptr() for x in c],
                                              *[None if g is None else g.ptr for g in out], env._stream()), env._h)
    torch.cuda.synchronize()
    got = tuple(None if g is None else g.get() for g in out)
    for i, x in enumerate(got):
        assert x is None or (x != out[i].sent).all(), ("an entry that was not written", i)
    return got


@functools.lru_cache(maxsize=None)
def _row_errors(name, e, k, vm_bytes, grad_bytes):
    """(error of the kernel's M rows, error of the float64 reference's) against the extended reference at the kernel's |V| and the
    oracle's angles, relative to each row's largest entry; cached on the bits, which an env keeps whatever B is"""
    o, row = oracle_rows(name)[e]
    net, lim = o.net, G.limits(o)
    V = np.frombuffer(vm_bytes) * np.exp(1j * np.angle(row[k]["r"].V))
    grad = np.frombuffer(grad_bytes).reshape(M, net.n_sgen)
    cvm, cva = cots(name)
    ext, f64 = VR.Adjoint(net, V, ext=True), VR.Adjoint(net, V)
    err = e64 = 0.0
    for m in range(M):
        want = VR.voltage_vjp(net, V, lim, cvm[e, k, m], cva[e, k, m], ext=True, adjoint=ext)
        err = max(err, G.rel_inf(grad[m], want))
        e64 = max(e64, G.rel_inf(VR.voltage_vjp(net, V, lim, cvm[e, k, m], cva[e, k, m], adjoint=f64), want))
    return err, e64


def compare(name, got, cand, B, first=0):
    """the rows of a K = 3, M = 5 call: statuses and NaN rows on every env, |V| and the angles against the oracle and the gradient against
    the extended reference on the reference envs.  Only the planted unsolvable candidate is left out, and counted."""
    grad, vm, va, st, it = got
    net = G.make(name)[0]
    assert grad.shape == (B, K, M, net.n_sgen) and grad.dtype == np.float64 and st.dtype == np.uint8 and it.dtype == np.int32
    assert (st == PATTERN).all(), (name, B)
    assert np.isnan(grad[:, 2]).all() and np.isnan(vm[:, 2]).all() and np.isnan(va[:, 2]).all()
    assert np.isfinite(grad[:, :2]).all() and np.isfinite(vm[:, :2]).all() and np.isfinite(va[:, :2]).all()
    assert int((st != W.SOLVED).sum()) == B                       # the rows left out: the planted candidate of every env, nothing else
    assert (va[:, :2, int(net.ext_grid_bus)] == 0.0).all()
    rows, errs, e64s = oracle_rows(name), [], []
    for e in [e for e in REF_ENVS if first <= e < first + B]:
        for k in (0, 1):
            Vo = rows[e][1][k]["r"].V
            i = e - first
            assert np.abs(vm[i, k] - np.abs(Vo)).max() <= V_TOL and np.abs(va[i, k] - np.degrees(np.angle(Vo))).max() <= VA_TOL, (name, e, k)
            err, e64 = _row_errors(name, e, k, vm[i, k].tobytes(), grad[i, k].tobytes())
            errs.append(err); e64s.append(e64)
    bar = max(OK.BAR_FACTOR * max(e64s), OK.BAR_FLOOR)
    print(f"\n[vjp gpu] {name} B={B}: e64 {max(e64s):.2e} gpu {max(errs):.2e} bar {bar:.2e}")
    assert max(errs) <= bar, (name, B, max(errs), bar)


# ---- parity -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", NETS)
def test_nets_against_the_extended_reference(name, B):
    """one node, a 40-bus chain, a star, three trees with an sgen on the slack bus, the line-table edges, `tiny` and the shipped case33;
    K = 3 with M = 5, then K = 3 with M = 1, K = 1 with M = 5, K = 1 with M = 2 and M = 0 on the same handle: every smaller call has the
    bits of its rows of the first"""
    assert W.global_kernels("vjp.hip") == KERNELS
    cand = np.ascontiguousarray(candidates(name)[:B])
    cvm, cva = (np.ascontiguousarray(x[:B]) for x in cots(name))
    env = make_env(name, B)
    try:
        assert env.nr_kernel()["solver"] == 0
        scenario(env, name)
        full = vjp(env, cand, cvm, cva)
        compare(name, full, cand, B)
        ev = evaluate(env, cand)                                  # (reward, info, status, iterations, vm_pu)
        same_bits((full[1], full[3], full[4]), (ev[4], ev[2], ev[3]), "vm_pu, status, iterations as evaluate_actions")
        one = vjp(env, cand, cvm[:, :, 3:4], cva[:, :, 3:4])
        same_bits(one, (full[0][:, :, 3:4],) + full[1:], "row 3 of M = 5 against M = 1 with that cotangent alone")
        col = vjp(env, cand[:, 1:2], cvm[:, 1:2], cva[:, 1:2])
        same_bits(col, [x[:, 1:2] for x in full], "K = 1 against column 1 of K = 3")
        two = vjp(env, cand[:, :1], cvm[:, :1, :2], cva[:, :1, :2])
        same_bits(two, (full[0][:, :1, :2],) + tuple(x[:, :1] for x in full[1:]), "K = 1, M = 2")
        none = vjp(env, cand, m=0)
        assert none[0] is None
        same_bits(none[1:], full[1:], "M = 0: the voltages alone")
        if name == "feeders3":                                    # the sgen on the slack bus: exactly 0, in every cotangent
            net = G.make(name)[0]
            assert int(net.sgen_bus[3]) == int(net.ext_grid_bus) and (full[0][:, :2, :, 3] == 0.0).all()
    finally:
        env.close()


# ---- bits -------------------------------------------------------------------------------------------------------------------------------
def test_bits():
    name, B = "chain40", 130
    cand, (cvm, cva) = candidates(name), cots(name)
    net = G.make(name)[0]
    env = make_env(name, B)
    try:
        scenario(env, name)
        full = vjp(env, cand, cvm, cva)
        same_bits(full, vjp(env, cand, cvm, cva), "two calls")
        c32 = cand.astype(np.float32)                             # float32 actions: the same values widened
        same_bits(vjp(env, c32, cvm, cva), vjp(env, c32.astype(np.float64), cvm, cva), "float32")
        vm_only = vjp(env, cand, cvm, None)
        same_bits(vm_only, vjp(env, cand, cvm, np.zeros_like(cva)), "cot_va = NULL against zeros")
        same_bits(vjp(env, cand, None, cva), vjp(env, cand, np.zeros_like(cvm), cva), "cot_vm = NULL against zeros")
        p_vm, p_va = cvm.copy(), cva.copy()                       # a NaN in the slack bus's entries never reaches the result
        p_vm[..., int(net.ext_grid_bus)], p_va[..., int(net.ext_grid_bus)] = np.nan, np.nan
        same_bits(vjp(env, cand, p_vm, p_va), full, "NaN in the slack-bus cotangent entries")
    finally:
        env.close()
    # an env alone at B = 1, and a batch that begins at env id 13 and crosses the 64-env edge: every env moves to another lane
    for first, n in ((20, 1), (13, 60)):
        other = make_env(name, n, env_id_offset=first)
        try:
            scenario(other, name, first=first)
            got = vjp(other, cand[first:first + n], cvm[first:first + n], cva[first:first + n])
            same_bits(got, [x[first:first + n] for x in full], f"env ids from {first}, B = {n}")
        finally:
            other.close()


# ---- NaN rows ---------------------------------------------------------------------------------------------------------------------------------
def test_frozen_batch_is_status_3():
    """episode_limit 2: after two steps every episode has ended and no env would be solved by step(): status 3, NaN, 0 iterations"""
    name, B = "tiny", 5
    env = make_env(name, B, episode_limit=2)
    try:
        env.reset()
        for _ in range(2):
            _, term, _ = env.step(torch.zeros(B, env.n_sgen, dtype=torch.float64, device=DEV))
        assert bool(term.all())
        cand, (cvm, cva) = candidates(name)[:B], cots(name)
        grad, vm, va, st, it = vjp(env, cand, cvm[:B], cva[:B])
        assert (st == W.NOT_EVALUATED).all() and (it == 0).all() and np.isnan(grad).all() and np.isnan(vm).all() and np.isnan(va).all()
        ev = evaluate(env, cand)
        same_bits((vm, st, it), (ev[4], ev[2], ev[3]), "as evaluate_actions, every env frozen")
    finally:
        env.close()


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_non_finite_action_on_the_slack_bus_sgen(value):
    """feeders3's fourth sgen sits on the ext_grid bus: no solve reads its injection, so the row solves (status 0), and k_action_grad's
    rule makes it NaN in grad, vm_pu and va_degree; every other row keeps the bits of the call with 0.0 in that entry"""
    name, B, j, envs = "feeders3", 65, 3, [0, 5, 63, 64]
    cand, (cvm, cva) = candidates(name)[:B].copy(), cots(name)
    env = make_env(name, B)
    try:
        scenario(env, name)
        cand[envs, 1, j] = 0.0
        clean = vjp(env, cand, cvm[:B], cva[:B])
        cand[envs, 1, j] = value
        got = vjp(env, cand, cvm[:B], cva[:B])
        assert (got[3] == PATTERN).all()
        mask = np.ones((B, K), bool)
        mask[envs, 1] = False
        for a, b in zip(got, clean):
            assert np.array_equal(a[mask], b[mask], equal_nan=True)
        assert all(np.isnan(x[envs, 1]).all() for x in got[:3]) and np.isfinite(clean[0][envs, 1]).all()
        same_bits((got[3], got[4]), (clean[3], clean[4]), "status and iterations")
    finally:
        env.close()


# ---- the contract -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["voltage_vjp", "backward"])
def test_state_untouched_and_step_agrees(how):
    """tests/baseline_contract.py with candidate 1 of {0, random, UNSOLVABLE}, after voltage_vjp and after a backward() through
    differentiable_voltages"""
    name, k0 = "case33", 1

    def baseline(env):
        cand = torch.as_tensor(W.candidates(name, env.n_envs, 3), device=DEV)
        if how == "voltage_vjp":
            g, vm, va, st, it = env.voltage_vjp(cand, cot_vm=torch.ones(env.n_envs, 3, env.n_bus, dtype=torch.float64, device=DEV))
        else:
            a = cand.clone().requires_grad_(True)
            vm, va, st = env.differentiable_voltages(a)
            ok = (st == 0)
            (vm[ok].sum() + va[ok].sum()).backward()
            g = a.grad
        assert (st[:, 2] == W.PF_FAILED).all() and (st[:, k0] == W.SOLVED).any() and bool(torch.isfinite(g[:, k0][st[:, k0] == 0]).all())
        return cand[:, k0].contiguous(), st[:, k0], vm[:, k0].detach()
    BC.check_state_untouched_and_step_agrees(lambda B: make_env(name, B), baseline, False, B=24)


# ---- against action_gradients -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("barrier", G.BARRIER_TYPES)
def test_barrier_cotangent_plus_the_direct_term_is_action_gradients(barrier):
    """cot_vm = -voltage_weight / n_bus barrier'(|V|) in float64 from the returned vm_pu, cot_va = 0: voltage_vjp plus the direct term of the
    reward is action_gradients' row, within the sum of the two kernels' bars (tests/grad_ref.bar of the case, twice)"""
    name = "crowded"
    args = () if barrier == "bowl" else (("voltage_barrier_type", barrier),)
    B, Kc = G.VARIANT_SHAPE
    os_, ref, cand = G.reference(name, B, Kc, args)
    env = make_env(name, B, **dict(args))
    try:
        from tests.test_action_grad_gpu import scenario as scenario_random
        scenario_random(env, name)
        ag = env.action_gradients(torch.as_tensor(cand, device=DEV))[0].cpu().numpy()
        vm = vjp(env, cand, m=0)[1]
        cot = np.stack([[VR.barrier_cotangent(os_[e], np.nan_to_num(vm[e, k], nan=1.0)) for k in range(Kc)] for e in range(B)])[:, :, None]
        grad, _, _, st, _ = vjp(env, cand, cot, None)
        bar, n = 2 * G.bar(name, args), 0
        for e in range(B):
            for k in range(Kc):
                if st[e, k] != W.SOLVED:
                    assert np.isnan(ag[e, k]).all() and np.isnan(grad[e, k]).all()
                    continue
                got = grad[e, k, 0] + VR.direct_term(os_[e], cand[e, k], G.limits(os_[e]))
                scale = max(np.abs(ag[e, k]).max(), np.abs(grad[e, k, 0]).max())          # each bar is relative to its own row's largest entry
                assert np.abs(got - ag[e, k]).max() <= bar * scale, (barrier, e, k)
                n += 1
        assert n == B * int(W.expected_pattern(Kc).sum())
    finally:
        env.close()


# ---- autograd -------------------------------------------------------------------------------------------------------------------------------
def loss_of(vm, va):
    return torch.relu(vm - 1.03).pow(2).sum() + 1e-3 * va.pow(2).sum()


def test_autograd():
    name, B = "tiny", 5
    cand = torch.as_tensor(candidates(name)[:B], device=DEV)
    env = make_env(name, B)
    try:
        scenario(env, name)
        a = cand.clone().requires_grad_(True)
        vm, va, st = env.differentiable_voltages(a)
        assert vm.grad_fn is not None and va.grad_fn is not None and not st.requires_grad
        solved = (st == 0)
        assert np.array_equal(st.cpu().numpy(), np.tile(PATTERN, (B, 1)))
        loss_of(vm[solved], va[solved]).backward()
        # the cotangents torch computed, by hand: d loss / d vm and d loss / d va (zero on the rows the loss leaves out)
        vm0, va0, _, _ = env.solve_actions(cand)
        same_bits((vm0.cpu().numpy(), va0.cpu().numpy()), (vm.detach().cpu().numpy(), va.detach().cpu().numpy()), "forward is solve_actions")
        lv, la = vm0.clone().requires_grad_(True), va0.clone().requires_grad_(True)
        loss_of(lv[solved], la[solved]).backward()
        want = env.voltage_vjp(cand, cot_vm=lv.grad, cot_va=la.grad)[0]
        want = torch.where(solved.unsqueeze(-1), want, torch.zeros_like(want))
        assert torch.equal(a.grad, want) and bool((a.grad[:, 2] == 0.0).all()) and bool(a.grad[:, :2].abs().max() > 0)
        # float32 actions get a float32 gradient of the same values
        a32 = cand.float().requires_grad_(True)
        vm32, va32, st32 = env.differentiable_voltages(a32)
        loss_of(vm32[st32 == 0], va32[st32 == 0]).backward()
        assert a32.grad.dtype == torch.float32 and a32.grad.shape == a32.shape and bool(torch.isfinite(a32.grad).all())
        # a step between forward and backward: the state has moved
        b = cand.clone().requires_grad_(True)
        vm, va, st = env.differentiable_voltages(b)
        env.step(cand[:, 1].contiguous())
        with pytest.raises(RuntimeError, match="state has moved"):
            loss_of(vm[st == 0], va[st == 0]).backward()
    finally:
        env.close()


# ---- the Jacobian ---------------------------------------------------------------------------------------------------------------------------
def test_voltage_jacobian():
    name, B = "tiny", 5
    net = G.make(name)[0]
    nb, ns = net.n_bus, net.n_sgen
    cand = candidates(name)[:B, :2]
    env = make_env(name, B)
    try:
        scenario(env, name)
        jac = env.voltage_jacobian(torch.as_tensor(cand, device=DEV)).cpu().numpy()
        assert jac.shape == (B, 2, nb, ns)
        for b in range(nb):                                       # nb calls with one unit cotangent each
            unit = np.zeros((B, 2, 1, nb))
            unit[..., b] = 1.0
            assert np.array_equal(vjp(env, cand, unit, None)[0][:, :, 0], jac[:, :, b]), b
        some = env.voltage_jacobian(torch.as_tensor(cand, device=DEV), buses=[nb - 1, 1]).cpu().numpy()
        assert np.array_equal(some, jac[:, :, [nb - 1, 1]])
        assert (jac[:, :, int(net.ext_grid_bus)] == 0.0).all()
        # ... and the columns of J^-1 of the reference at the kernel's |V| and the oracle's angles
        vm = vjp(env, cand, m=0)[1]
        errs, e64s = [], []
        for e in (0, 1, 2):
            o, row = oracle_rows(name)[e]
            for k in (0, 1):
                V = vm[e, k] * np.exp(1j * np.angle(row[k]["r"].V))
                ext, f64 = VR.Adjoint(net, V, ext=True), VR.Adjoint(net, V)
                for b in range(nb):
                    want = VR.voltage_vjp(net, V, G.limits(o), np.eye(nb)[b], None, ext=True, adjoint=ext)
                    if b == int(net.ext_grid_bus):
                        assert (want == 0).all()
                        continue
                    errs.append(G.rel_inf(jac[e, k, b], want))
                    e64s.append(G.rel_inf(VR.voltage_vjp(net, V, G.limits(o), np.eye(nb)[b], None, adjoint=f64), want))
        bar = max(OK.BAR_FACTOR * max(e64s), OK.BAR_FLOOR)
        print(f"\n[vjp gpu] jacobian {name}: e64 {max(e64s):.2e} gpu {max(errs):.2e} bar {bar:.2e}")
        assert max(errs) <= bar
    finally:
        env.close()


# ---- the C ABI and the refusals on a live handle -----------------------------------------------------------------------------------------
def test_c_abi_refusals_on_a_live_handle():
    name, B = "tiny", 5
    env = make_env(name, B)
    try:
        scenario(env, name)
        lib = _lib.load()
        a = torch.as_tensor(candidates(name)[:B, :2], device=DEV).contiguous()
        cot = torch.ones(B, 2, 2, env.n_bus, dtype=torch.float64, device=DEV)
        g = torch.empty(B, 2, 2, env.n_sgen, dtype=torch.float64, device=DEV)
        st = torch.empty(B, 2, dtype=torch.uint8, device=DEV)
        ok = [a.data_ptr(), 1, 2, 2, cot.data_ptr(), None, g.data_ptr(), None, None, st.data_ptr(), None, None]
        for change, word in (({2: 0}, "n_candidates"), ({2: 1025}, "n_candidates"), ({3: -1}, "n_cotangents"), ({3: 1025}, "n_cotangents"),
                             ({4: None}, "cot_vm or cot_va"), ({3: 0}, "grad must be NULL"), ({6: None}, "grad must be NULL"), ({1: 9}, "dtype"),
                             ({0: None}, "null buffer"), ({9: None}, "null buffer")):
            call = list(ok)
            for i, v in change.items():
                call[i] = v
            assert lib.mapdn_voltage_vjp(env._h, *call) == -1 and word in lib.mapdn_last_error(env._h).decode(), change
        assert lib.mapdn_voltage_vjp(env._h, *ok) == 0           # vm_pu, va_degree and iterations may be NULL
        torch.cuda.synchronize()
        assert torch.equal(g, env.voltage_vjp(a, cot_vm=cot)[0])
        for bad in (dict(actions=torch.zeros(B, 2, env.n_sgen + 1)), dict(actions=a, cot_vm=torch.zeros(B, 2, 2, env.n_bus + 1)),
                    dict(actions=a, cot_vm=torch.zeros(B, 3, env.n_bus)), dict(actions=a), dict(actions=a, cot_vm=cot, cot_va=cot[:, :, :1])):
            with pytest.raises(ValueError):
                env.voltage_vjp(**bad)
        squeezed = env.voltage_vjp(a, cot_vm=cot[:, :, 0])[0]
        assert squeezed.shape == (B, 2, env.n_sgen) and torch.equal(squeezed, g[:, :, 0])
    finally:
        env.close()


@pytest.mark.parametrize("name,tuning,word", [("crowded_meshed", None, "sparse solver"), ("crowded_meshed", dict(grad_meshed=1), "sparse solver"),
                                              ("one_sgen", dict(nr_solver="dense"), "dense solver"), ("crowded_zip", None, "ZIP"),
                                              ("crowded_fused", None, "fused")])
def test_python_refusals_on_a_live_handle(name, tuning, word):
    net, prof, base = W.make(name)
    env = VoltageControlBatch(net, prof, dict(base), n_envs=3, device=DEV, obs_dtype=torch.float64, tuning=tuning)
    try:
        env.reset()
        a = torch.zeros(3, 2, env.n_sgen, device=DEV)
        for call in (lambda: env.voltage_vjp(a, cot_vm=torch.zeros(3, 2, env.n_bus, device=DEV)), lambda: env.solve_actions(a),
                     lambda: env.voltage_jacobian(a), lambda: env.differentiable_voltages(a)):
            with pytest.raises(NotImplementedError, match=word):
                call()
        env.evaluate_actions(a)                                   # (which covers these handles)
    finally:
        env.close()


# ---- the drop-in ----------------------------------------------------------------------------------------------------------------------------
def test_drop_in():
    """VoltageControl.voltage_vjp and .solve_actions at B = 1 return row 0 of the batch call"""
    name = "crowded"
    net, prof, base = W.make(name)
    cand = W.candidates(name, 1, 3)
    cot = np.random.default_rng(5).uniform(-1, 1, (1, 3, 2, net.n_bus))
    one = VoltageControl(dict(base, net=net, profiles=prof), device=DEV)
    batch = make_env(name, 1)
    try:
        batch.reset()
        want = vjp(batch, cand, cot, None)
        got = one.voltage_vjp(cand[0], cot_vm=cot[0])
        assert all(isinstance(x, np.ndarray) for x in got) and got[0].shape == (3, 2, net.n_sgen)
        same_bits(got, [x[0] for x in want], "row 0 of the batch call")
        same_bits(one.solve_actions(cand[0]), [x[0] for x in want[1:]], "solve_actions")
        assert list(got[3]) == [W.SOLVED, W.SOLVED, W.PF_FAILED] and np.isnan(got[0][2]).all() and np.isfinite(got[0][:2]).all()
    finally:
        one.close()
        batch.close()
