"""CPU tests of the PPO kernel matrix (tests/ppo_kernel_matrix.py): the rows cover the kernel set parsed from csrc/ppo.hip — a kernel added
without a row fails here —, the launch sites are the ones the rows were built for, the entries refuse bad arguments on the host before
anything is launched, the two float64 restatements of the GAE agree, and the float32 PyTorch fallback is measured against the float64
restatements over every row: that measurement is what the kernels' bars are four times of."""
import re

import pytest
import torch

from mapdn_amd import _lib
from mapdn_amd import learner as L
from tests import ppo_kernel_matrix as pm


def test_the_rows_cover_the_compiled_set_exactly():
    ck = pm.compiled_kernels()
    assert set(ck) == pm.KERNELS
    assert sorted(ck) == sorted(list(pm.KERNELS) + ["k_ppo_loss_finish"])          # the finishing pass: launched by both losses, nothing twice otherwise
    have = {k for r in pm.GAE_ROWS + pm.LOSS_ROWS for k in r.kernels}
    assert have == set(ck), (sorted(set(ck) - have), sorted(have - set(ck)))
    labels = [r.label for r in pm.GAE_ROWS + pm.LOSS_ROWS]
    assert len(set(labels)) == len(labels)
    assert [r.label for r in pm.gae_rows(304) + pm.loss_rows(304)] == labels
    assert {(r.rows, r.n, r.S) for r in pm.GAE_ROWS} >= {(1, 1, 1), (9, 3, 1), (240, 3, 1), (7, 3, 16), (37, 38, 8)}
    for cus in (pm.CUS, 304, 64):
        big = [r for r in pm.gae_rows(cus) if r.label == "big"][0]
        over = big.S * big.n - pm.capacity(cus)
        assert 0 < over < 8 and over % 2 == 1 and big.rows % big.S and big.rows > 2 * big.S        # past one turn of the grid by a small odd number; ragged
        shapes = {r.rows * r.n for r in pm.loss_rows(cus)}
        assert shapes == {1, 63, 65, 27 * 38, pm.capacity(cus) + 1}
    assert (37 * 38) % 64 and (8 * 38) % 64
    print(f"[ppo kernel matrix] compiled: {len(set(ck))} kernels; {len(pm.GAE_ROWS)} GAE rows, {len(pm.LOSS_ROWS)} loss rows x {len(pm.VALID_MODES)} weightings")


def test_a_kernel_without_a_row_is_caught():
    """copies of the source with one more kernel: a new k_ppo_* kernel with a launch site, a templated one, a name that is no kernel"""
    real = pm._src
    site = "  hipLaunchKernelGGL(k_ppo_gae, dim3(blocks)"
    assert site in real()
    extra_kernel = "__global__ void k_ppo_extra(float* x) { x[0] = 0.0f; }\n"
    cases = ((lambda s: extra_kernel + s.replace(site, "  hipLaunchKernelGGL(k_ppo_extra, dim3(1), dim3(64), 0, st, adv); " + site.strip(), 1), "set"),
             (lambda s: s.replace(site, site.replace("(k_ppo_gae,", "((k_ppo_gae<1>),"), 1), "raise"),
             (lambda s: s + "\nstatic int k_ppo_orphan = 0;\n", "raise"))
    for edit, how in cases:
        pm._src = lambda name="ppo.hip", _e=edit: _e(real(name))
        try:
            if how == "raise":
                with pytest.raises(AssertionError):
                    pm.compiled_kernels()
            else:
                assert set(pm.compiled_kernels()) - pm.KERNELS == {"k_ppo_extra"}       # the exact-cover test then fails
        finally:
            pm._src = real


def test_the_launch_sites():
    """256 threads, no dynamic LDS, workgroups = min(ceil(units / 256), 8 per CU): the grid the "big" rows were built for; the loss
    kernels leave one partial per workgroup, the finishing pass is ONE workgroup"""
    src = pm._src()
    assert f"PPO_NT = {pm.THREADS}" in src and f"PPO_BLOCKS_PER_CU = {pm.BLOCKS_PER_CU}" in src
    launches = re.findall(r"hipLaunchKernelGGL\((k_ppo_\w+),\s*dim3\((\w+)\),\s*dim3\((\w+)\),\s*(\d+),", src)
    assert sorted(launches) == sorted([("k_ppo_gae", "blocks", "PPO_NT", "0"), ("k_ppo_policy_loss", "blocks", "PPO_NT", "0"),
                                       ("k_ppo_value_loss", "blocks", "PPO_NT", "0"), ("k_ppo_loss_finish", "1", "PPO_NT", "0"),
                                       ("k_ppo_loss_finish", "1", "PPO_NT", "0")])
    assert re.search(r"std::min<int64_t>\(\(units \+ PPO_NT - 1\) / PPO_NT, \(int64_t\)\(cus \? cus : ppo_cus\(\)\) \* PPO_BLOCKS_PER_CU\)", src)
    assert src.count("__launch_bounds__(PPO_NT)") == 4
    assert not re.search(r"atomic", src), "the loss sums are deterministic: no atomics"
    assert src.count("#pragma clang fp contract(off)") == 4
    lib = _lib.load()
    assert lib.mapdn_ppo_loss_blocks(0) == 0 and lib.mapdn_ppo_loss_blocks(-5) == 0
    assert lib.mapdn_ppo_loss_blocks(1) == 1 and lib.mapdn_ppo_loss_blocks(256) == 1 and lib.mapdn_ppo_loss_blocks(257) == 2


@pytest.mark.parametrize("row", pm.GAE_ROWS + pm.LOSS_ROWS, ids=[r.label for r in pm.GAE_ROWS + pm.LOSS_ROWS])
def test_every_row_names_an_exported_entry(row):
    assert hasattr(_lib.load(), row.entry) and row.entry in _lib.EXPORTS
    assert row.rows >= 1 and row.n >= 1 and row.rows * row.n <= L.PPO_MAX_ELEMS


def test_invalid_arguments_are_refused_on_the_host():
    """n, rows or stride below 1, too many elements, a missing pointer: MAPDN_E_INVALID before any launch (the pointers are never read)"""
    lib = _lib.load()
    buf = torch.zeros(64)
    p = buf.data_ptr()

    def gae(rows=9, n=3, S=1, ptrs=(p,) * 6):
        return lib.mapdn_ppo_gae(*ptrs, rows, n, S, 0.99, 0.95, None)

    def pol(rows=9, n=3, eps=0.6, ptrs=(p,) * 8, outs=(p, p, p)):
        return lib.mapdn_ppo_policy_loss(*ptrs, eps, *outs, rows, n, None)

    def val(rows=9, n=3, eps=0.6, ptrs=(p,) * 7, outs=(p, p, p)):
        return lib.mapdn_ppo_value_loss(*ptrs, 0.99, eps, 2.0, *outs, rows, n, None)

    def without(k, count):
        return tuple(None if i == k else p for i in range(count))
    codes = [gae(rows=0), gae(rows=-1), gae(n=0), gae(n=-2), gae(S=0), gae(S=-3), gae(rows=2 ** 40, n=2)] + [gae(ptrs=without(k, 6)) for k in range(6)]
    codes += [pol(rows=0), pol(n=0), pol(eps=-0.1), pol(eps=float("nan")), pol(rows=2 ** 40, n=2)] + [pol(ptrs=without(k, 8)) for k in (0, 1, 2, 4, 5, 7)]
    codes += [pol(outs=without(k, 3)) for k in range(3)]
    codes += [val(rows=0), val(n=0), val(eps=-0.1), val(rows=2 ** 40, n=2)] + [val(ptrs=without(k, 7)) for k in (0, 1, 2, 3, 4, 6)]
    codes += [val(outs=without(k, 3)) for k in range(3)]
    assert codes == [-1] * len(codes), codes             # MAPDN_E_INVALID (include/mapdn.h); avail and valid may be NULL: not in the list


def test_the_learner_predicate(monkeypatch):
    import types
    ok = types.SimpleNamespace(is_cuda=True, dtype=torch.float32, dim=lambda: 2, numel=lambda: 12)
    assert L.ppo_fused_ok(ok, ok, None)
    assert not L.ppo_fused_ok(ok, types.SimpleNamespace(is_cuda=False, dtype=torch.float32))
    assert not L.ppo_fused_ok(ok, types.SimpleNamespace(is_cuda=True, dtype=torch.float64))
    assert not L.ppo_fused_ok(types.SimpleNamespace(is_cuda=True, dtype=torch.float32, dim=lambda: 2, numel=lambda: L.PPO_MAX_ELEMS + 1))
    assert not L.ppo_fused_ok(types.SimpleNamespace(is_cuda=True, dtype=torch.float32, dim=lambda: 2, numel=lambda: 0))
    assert not L.ppo_fused_ok(torch.zeros(3, 2))                       # the CPU: the vectorised PyTorch route
    monkeypatch.setenv("MAPDN_FUSED_PPO", "0")
    assert not L.ppo_fused_ok(ok, ok)


@pytest.mark.parametrize("row", [r for r in pm.GAE_ROWS if r.rows <= 2000], ids=lambda r: r.label)
def test_the_two_float64_restatements_of_the_gae_agree(row):
    """the reference's loop over the rows (per-chain carry) and the padded [T, S, n] form the big row is compared against"""
    inp = pm.gae_inputs(row, 100 + row.rows)
    a, b = pm.gae_rowloop64(inp, row.S), pm.gae_padded64(inp, row.S)
    assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max()))
    if row.rows >= 4:
        combos = {(int(d), int(s)) for d, s in zip(inp["done"], inp["last_step"])}
        assert combos == {(0, 0), (0, 1), (1, 0), (1, 1)}
    if row.S > row.rows:                                                       # chains of one row: the advantage is the delta
        mask = torch.where(inp["last_step"] != 0, 1 - inp["done"], torch.ones_like(inp["done"])).double().unsqueeze(1)
        assert torch.equal(a, inp["reward"].double() + pm.GAMMA * inp["next_value"].double() * mask - inp["value"].double())


def fallback_errors():
    """{quantity: largest rel_err of the float32 PyTorch fallback against the float64 restatement over all rows and weightings}"""
    worst = dict.fromkeys(pm.MEASURED, 0.0)

    def note(k, e):
        worst[k] = max(worst[k], e)
    for i, row in enumerate(pm.GAE_ROWS):
        inp = pm.gae_inputs(row, 100 + i)
        got = L.ppo_gae_torch(inp["reward"], inp["value"], inp["next_value"], inp["done"], inp["last_step"], row.S, pm.GAMMA, pm.LAMBDA)
        note("gae", pm.rel_err(got, pm.gae_padded64(inp, row.S)))
    for i, row in enumerate(pm.LOSS_ROWS):
        for j, mode in enumerate(pm.VALID_MODES):
            valid = pm.valid_of(mode, row.rows, torch.Generator().manual_seed(1000 + 10 * i + j))
            if row.kind == "policy":
                inp = pm.policy_inputs(row, 200 + i)
                for eps, exact in ((pm.EPS_CLIP, False), (0.0, True)):
                    mean = inp["mean"].clone().requires_grad_(True)
                    sh = (row.rows, row.n, 1)
                    loss = L.ppo_policy_loss_torch(mean.view(sh), inp["action"].view(sh), inp["log_std"].view(sh), inp["avail"].view(sh),
                                                   inp["old"].view(sh), inp["adv"], valid, eps)
                    (grad,) = torch.autograd.grad(loss, mean)
                    rl, rg, scale = pm.policy_ref64(inp, valid, eps, exact)
                    note("policy_loss", pm.rel_err(loss.detach(), rl, scale)); note("policy_grad", pm.rel_err(grad, rg))
            else:
                inp = pm.value_inputs(row, 300 + i)
                v = inp["v"].clone().requires_grad_(True)
                loss = L.ppo_value_loss_torch(v, inp["v_old"], inp["reward"], inp["v_next"], inp["done"], valid, pm.GAMMA, pm.EPS_EXACT, pm.COEF)
                (grad,) = torch.autograd.grad(loss, v)
                rl, rg, scale = pm.value_ref64(inp, valid)
                note("value_loss", pm.rel_err(loss.detach(), rl, scale)); note("value_grad", pm.rel_err(grad, rg))
    return worst


def test_the_float32_fallback_defines_the_bars():
    """the deviation of the float32 PyTorch route from the float64 restatements over every row: the figures in ppo_kernel_matrix.MEASURED
    are this measurement (to within the half that another CPU's exp / log may move a largest error), the kernels' bars are four times them"""
    worst = fallback_errors()
    for k, e in worst.items():
        print(f"[ppo kernel matrix] float32 fallback, {k}: {e:.3e} (recorded {pm.MEASURED[k]:.3e}, kernel bar {pm.BAR[k]:.3e})")
    for k, e in worst.items():
        assert 0.5 * pm.MEASURED[k] <= e <= 1.5 * pm.MEASURED[k], (k, e, pm.MEASURED[k])
        assert pm.BAR[k] == 4.0 * pm.MEASURED[k] and pm.BAR[k] < 1e-4                      # far below what a logic error moves (~0.1)


def test_a_wrong_mask_or_tie_rule_is_far_above_the_bars():
    """the sensitivity the bars rely on: cutting the chain at a timeout row, or dropping torch.min's half-gradient at a tie, moves the
    float64 result by orders of magnitude more than any bar"""
    row = pm.GAE_ROWS[2]
    inp = pm.gae_inputs(row, 102)
    ref = pm.gae_padded64(inp, row.S)
    wrong = dict(inp, done=torch.maximum(inp["done"], inp["last_step"]))          # "a timeout cuts the chain"
    assert pm.rel_err(pm.gae_padded64(wrong, row.S), ref) > 1e-2
    prow = [r for r in pm.LOSS_ROWS if r.label == "policy-n38"][0]
    pin = pm.policy_inputs(prow, 203)
    _, g_tie, _ = pm.policy_ref64(pin, None, 0.0, True)
    _, g_off, _ = pm.policy_ref64(pin, None, 0.0, False)                          # rho a rounding off the bounds: the clamp blocks the gradient
    assert pm.rel_err(g_off, g_tie) > 1e-2
