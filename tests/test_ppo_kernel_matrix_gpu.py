"""Every row of the PPO kernel matrix (tests/ppo_kernel_matrix.py) on the GPU, through the C ABI, against the float64 restatements written
there (the GAE as the reference's recurrence on rows padded to whole steps; the losses as the PyTorch expressions with float64 autograd).

Bars: ppo_kernel_matrix.BAR — four times the deviation of the float32 PyTorch fallback from the same restatements over the same rows,
measured on the CPU (see that module's docstring for the figures and the error measure).  Every loss row runs with `valid` absent, all
ones, mixed and all zeros (exactly 0 then, not NaN), the policy rows also with eps_clip = 0 (rho == 1 on both clip bounds).  Every output
has guard floats on both sides and is pre-filled with a sentinel; two launches on the same input must agree bit for bit.  The measured
figures are printed as "[ppo matrix] ..." lines."""
import pytest
import torch

from mapdn_amd import _lib
from tests import ppo_kernel_matrix as pm

pytestmark = pytest.mark.gpu
SENT, G = -7777.25, 256


def _dev():
    return torch.device("cuda:0")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _guarded(count, dev):
    buf = torch.full((2 * G + count,), SENT, dtype=torch.float32, device=dev)
    return buf, buf[G:G + count]


def _intact(buf, count):
    return bool((buf[:G] == SENT).all()) and bool((buf[G + count:] == SENT).all())


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _run_gae(row, inp):
    lib, dev = _lib.load(), inp["reward"].device
    buf, adv = _guarded(row.rows * row.n, dev)
    rc = lib.mapdn_ppo_gae(inp["reward"].data_ptr(), inp["value"].data_ptr(), inp["next_value"].data_ptr(), inp["done"].data_ptr(),
                           inp["last_step"].data_ptr(), adv.data_ptr(), row.rows, row.n, row.S, pm.GAMMA, pm.LAMBDA, _stream(dev))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _intact(buf, row.rows * row.n) and not bool((adv == SENT).any())
    return adv.view(row.rows, row.n)


@pytest.mark.parametrize("i", range(len(pm.GAE_ROWS)), ids=[r.label for r in pm.GAE_ROWS])
def test_gae_against_float64(i):
    row, dev = pm.gae_rows(_cus())[i], _dev()
    inp = pm.gae_inputs(row, 100 + i, dev)
    a, b = _run_gae(row, inp), _run_gae(row, inp)
    assert torch.equal(a, b)
    ref = pm.gae_padded64(inp, row.S)
    err = pm.rel_err(a, ref)
    print(f"[ppo matrix] gae {row.label} rows={row.rows} n={row.n} S={row.S}: err {err:.3e} bar {pm.BAR['gae']:.3e}")
    assert err <= pm.BAR["gae"], (row, err)
    if row.S == 1 and row.rows > 4:            # (the stride matters: the same rows as chains of stride 2 are other numbers)
        assert pm.rel_err(pm.gae_padded64(inp, 2), ref) > 1e-2


def _run_loss(row, inp, valid, eps):
    lib, dev = _lib.load(), inp["done"].device if row.kind == "value" else inp["adv"].device
    rows, n = row.rows, row.n
    with torch.cuda.device(dev):
        nb = lib.mapdn_ppo_loss_blocks(rows * n)
    assert nb == min((rows * n + pm.THREADS - 1) // pm.THREADS, _cus() * pm.BLOCKS_PER_CU)
    (lb, loss), (gb, grad), (pb, partial) = _guarded(1, dev), _guarded(rows * n, dev), _guarded(nb, dev)
    if valid is None:
        scale = torch.full((1,), 1.0 / (rows * n), device=dev)
    else:
        scale = (1.0 / (valid.sum().clamp(min=1.0) * n)).reshape(1)
    if row.kind == "policy":
        rc = lib.mapdn_ppo_policy_loss(inp["action"].data_ptr(), inp["mean"].data_ptr(), inp["log_std"].data_ptr(), inp["avail"].data_ptr(),
                                       inp["old"].data_ptr(), inp["adv"].data_ptr(), _ptr(valid), scale.data_ptr(), eps, loss.data_ptr(),
                                       grad.data_ptr(), partial.data_ptr(), rows, n, _stream(dev))
    else:
        rc = lib.mapdn_ppo_value_loss(inp["v"].data_ptr(), inp["v_old"].data_ptr(), inp["reward"].data_ptr(), inp["v_next"].data_ptr(),
                                      inp["done"].data_ptr(), _ptr(valid), scale.data_ptr(), pm.GAMMA, eps, pm.COEF, loss.data_ptr(),
                                      grad.data_ptr(), partial.data_ptr(), rows, n, _stream(dev))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _intact(lb, 1) and _intact(gb, rows * n) and _intact(pb, nb)
    assert not bool((grad == SENT).any()) and not bool((loss == SENT).any()) and not bool((partial == SENT).any())
    return loss[0].clone(), grad.view(rows, n).clone()


@pytest.mark.parametrize("i", range(len(pm.LOSS_ROWS)), ids=[r.label for r in pm.LOSS_ROWS])
def test_loss_and_gradient_against_float64(i):
    row, dev = pm.loss_rows(_cus())[i], _dev()
    policy = row.kind == "policy"
    inp = pm.policy_inputs(row, 200 + i, dev) if policy else pm.value_inputs(row, 300 + i, dev)
    for j, mode in enumerate(pm.VALID_MODES):
        valid = pm.valid_of(mode, row.rows, torch.Generator().manual_seed(1000 + 10 * i + j))
        valid = valid.to(dev) if valid is not None else None
        for eps, exact in (((pm.EPS_CLIP, False), (0.0, True)) if policy else ((pm.EPS_EXACT, False),)):
            (l1, g1), (l2, g2) = _run_loss(row, inp, valid, eps), _run_loss(row, inp, valid, eps)
            assert torch.equal(l1, l2) and torch.equal(g1, g2)                       # deterministic: the same bits again
            rl, rg, scale = pm.policy_ref64(inp, valid, eps, exact) if policy else pm.value_ref64(inp, valid)
            el, eg = pm.rel_err(l1, rl, scale), pm.rel_err(g1, rg)
            bl, bg = pm.BAR[row.kind + "_loss"], pm.BAR[row.kind + "_grad"]
            print(f"[ppo matrix] {row.label} rows={row.rows} n={row.n} valid={mode} eps={eps}: loss err {el:.3e} bar {bl:.3e}; grad err {eg:.3e} bar {bg:.3e}")
            assert torch.isfinite(l1) and bool(torch.isfinite(g1).all())
            assert el <= bl and eg <= bg, (row, mode, eps, el, eg)
            if mode == "zeros":
                assert float(l1) == 0.0 and float(g1.abs().max()) == 0.0


def test_invalid_arguments_launch_nothing():
    """bad rows, n, stride or eps_clip: the error code, and the output buffers keep their sentinel"""
    lib, dev = _lib.load(), _dev()
    row = pm.GAE_ROWS[1]
    inp = pm.gae_inputs(row, 5, dev)
    buf, adv = _guarded(row.rows * row.n, dev)
    p = [inp[k].data_ptr() for k in ("reward", "value", "next_value", "done", "last_step")]
    for rows, n, S in ((0, 3, 1), (9, 0, 1), (9, 3, 0), (9, 3, -1), (2 ** 40, 2, 1)):
        assert lib.mapdn_ppo_gae(*p, adv.data_ptr(), rows, n, S, pm.GAMMA, pm.LAMBDA, _stream(dev)) == -1, (rows, n, S)
    scale = torch.ones(1, device=dev)
    for rows, n, eps in ((0, 3, 0.6), (9, 0, 0.6), (9, 3, -0.5)):
        assert lib.mapdn_ppo_value_loss(p[0], p[1], p[2], p[0], p[3], None, scale.data_ptr(), pm.GAMMA, eps, pm.COEF, adv.data_ptr(), adv.data_ptr(),
                                        adv.data_ptr(), rows, n, _stream(dev)) == -1
        assert lib.mapdn_ppo_policy_loss(p[0], p[1], p[2], None, p[0], p[1], None, scale.data_ptr(), eps, adv.data_ptr(), adv.data_ptr(), adv.data_ptr(),
                                         rows, n, _stream(dev)) == -1
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())
