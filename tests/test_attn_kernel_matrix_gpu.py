"""Every row of the attention-core kernel matrix (tests/attn_kernel_matrix.py) on the GPU, through the C ABI, forward and backward,
against the literal per-head, per-agent loop (learner.attention_loop_reference) in float64 under autograd.

Bars are not fixed numbers: for each row and quantity the batched PyTorch float32 route (learner.attention_core_torch on the same
device) is measured against the same float64 values, and the kernel's bar is 4 x that error — another order of summation and the
device's exp —, with a floor of 1e-6 of the quantity's largest magnitude.  The floor stands for one f32 rounding per summed term, so for
sums it grows with the square root of the number of terms: B (n - 1) for logit_sq[i][h], n - 1 for the rows of dsel and dkey (which carry
logit_sq's gradient, 2 logit dlogit_sq, summed over the other agents).  Measured errors and bars are printed as "[attn matrix] ..." lines.
Every output sits between guard rows pre-filled with a sentinel, and two launches must agree bit for bit."""
import math

import pytest
import torch

from mapdn_amd import _lib
from mapdn_amd import learner
from tests import attn_kernel_matrix as am

pytestmark = pytest.mark.gpu
SENT, G = -7777.25, 4
IDX = list(range(len(am.ROWS)))


def _dev():
    return torch.device("cuda:0")


def _row(i):
    return am.rows_for(torch.cuda.get_device_properties(0).multi_processor_count)[i]


def _guarded(shape, dev):
    n = math.prod(shape)
    buf = torch.full((2 * G * 64 + n,), SENT, dtype=torch.float32, device=dev)
    return buf, buf[G * 64:G * 64 + n].view(shape)


def _intact(buf, n):
    return bool((buf[:G * 64] == SENT).all()) and bool((buf[G * 64 + n:] == SENT).all())


def _inputs(row, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    B, n, H = row.shape["B"], row.shape["n"], row.shape["H"]
    sel, key, val = (0.5 * torch.randn(B, n, 64, generator=g) for _ in range(3))
    if row.special == "diag":
        key = 50.0 * sel / sel.square().sum(-1, keepdim=True)                 # sel_i . key_i = 50: the own key would take all the weight
    if row.special == "hot":
        sel, key = 6.0 * sel, 6.0 * key
        logits = torch.einsum("bic,bjc->bij", sel.double(), key.double()) / math.sqrt(64 // H)
        off = logits.masked_fill(torch.eye(n, dtype=torch.bool), 0.0).abs().max()
        sel = (sel.double() * (100.0 / off)).float()                          # the largest scaled logit between two agents is +-100
    w_out, w_sq = torch.randn(B, n, 64, generator=g), 1e-3 * torch.randn(n, H, generator=g) / (B * (n - 1))
    return tuple(t.to(dev).contiguous() for t in (sel, key, val, w_out, w_sq))


def _with_grads(fn, sel, key, val, w_out, w_sq, H):
    ops = [t.detach().clone().requires_grad_(True) for t in (sel, key, val)]
    out, lsq = fn(*ops, H)
    return dict(zip(("out", "lsq", "dsel", "dkey", "dval"), (out.detach(), lsq.detach()) + torch.autograd.grad((out * w_out).sum() + (lsq * w_sq).sum(), ops)))


def _kernel(sel, key, val, w_out, w_sq, H):
    lib, dev = _lib.load(), sel.device
    B, n = sel.shape[:2]
    st = torch.cuda.current_stream(dev).cuda_stream
    bufs = {k: _guarded((B, n, 64), dev) for k in ("out", "dsel", "dkey", "dval")}
    bufs["lsq"] = _guarded((n, H), dev)
    sb, scratch = _guarded((lib.mapdn_attention_scratch_floats(B, n, H),), dev)
    assert lib.mapdn_attention_forward(sel.data_ptr(), key.data_ptr(), val.data_ptr(), B, n, H, bufs["out"][1].data_ptr(), bufs["lsq"][1].data_ptr(),
                                       scratch.data_ptr(), st) == 0
    assert lib.mapdn_attention_backward(w_out.data_ptr(), w_sq.data_ptr(), sel.data_ptr(), key.data_ptr(), val.data_ptr(), B, n, H,
                                        bufs["dsel"][1].data_ptr(), bufs["dkey"][1].data_ptr(), bufs["dval"][1].data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert _intact(sb, scratch.numel()) and not bool((scratch == SENT).any())
    for k, (buf, view) in bufs.items():
        assert _intact(buf, view.numel()), k
        assert not bool((view == SENT).any()), k
    return {k: v for k, (_, v) in bufs.items()}


@pytest.mark.parametrize("i", IDX, ids=[am.ROWS[i].label for i in IDX])
def test_attention_core_against_float64(i):
    row, dev = _row(i), _dev()
    B, n, H = row.shape["B"], row.shape["n"], row.shape["H"]
    sel, key, val, w_out, w_sq = _inputs(row, 17 * i + 3, dev)
    got, again = _kernel(sel, key, val, w_out, w_sq, H), _kernel(sel, key, val, w_out, w_sq, H)
    for k in got:
        assert torch.equal(got[k], again[k]), k                                # deterministic: the same bits again
    ref = _with_grads(learner.attention_loop_reference, sel.double(), key.double(), val.double(), w_out.double(), w_sq.double(), H)
    t32 = _with_grads(learner.attention_core_torch, sel, key, val, w_out, w_sq, H)
    terms = dict(out=1, dval=1, lsq=B * (n - 1), dsel=n - 1, dkey=n - 1)
    failed = []
    for k in ("out", "lsq", "dsel", "dkey", "dval"):
        assert bool(torch.isfinite(ref[k]).all()) and bool(torch.isfinite(got[k]).all()), k
        scale = float(ref[k].abs().max())
        e_torch, e_kernel = float((t32[k].double() - ref[k]).abs().max()), float((got[k].double() - ref[k]).abs().max())
        bar = max(4.0 * e_torch, 1e-6 * scale * math.sqrt(terms[k]))
        print(f"[attn matrix] {row.label} B={B} n={n} H={H} {k}: scale {scale:.3e} torch-f32 err {e_torch:.3e} kernel err {e_kernel:.3e} bar {bar:.3e}")
        if not e_kernel <= bar:
            failed.append((k, e_kernel, bar))
    assert not failed, failed
    if row.label == "n2":                                                      # one other agent: its value row, bit for bit
        assert torch.equal(got["out"][:, 0], val[:, 1]) and torch.equal(got["out"][:, 1], val[:, 0])
        zero = _kernel(sel, key, val, w_out, torch.zeros_like(w_sq), H)        # ... and the logits matter through the regulariser alone
        assert not bool(zero["dsel"].any()) and not bool(zero["dkey"].any())
        assert bool(got["dsel"].any()) and bool(got["dkey"].any())
    if row.special == "diag":                                                  # the own key really would have dominated
        own = torch.einsum("bic,bic->bi", sel, key)
        assert float((own - 50.0).abs().max()) < 1e-3
    if row.special == "hot":
        scaled = torch.einsum("bic,bjc->bij", sel.double(), key.double()) / math.sqrt(64 // H)
        assert float(scaled.masked_fill(torch.eye(n, dtype=torch.bool, device=dev), 0.0).abs().max()) >= 99.9


def test_the_autograd_function_is_the_kernels():
    """learner.attention_core on a CUDA float32 batch takes _AttentionCore and returns what the C ABI returns; MAPDN_FUSED_ATTN=0 does not"""
    row, dev = _row(2), _dev()
    sel, key, val, w_out, w_sq = _inputs(row, 5, dev)
    H = row.shape["H"]
    want = _kernel(sel, key, val, w_out, w_sq, H)
    before = learner._AttentionCore.launches
    got = _with_grads(learner.attention_core, sel, key, val, w_out, w_sq, H)
    assert learner._AttentionCore.launches == before + 1
    for k in want:
        assert torch.equal(got[k], want[k]), k
