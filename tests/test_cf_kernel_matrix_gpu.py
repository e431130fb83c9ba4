"""Every row of the counterfactual-baseline kernel matrix (tests/cf_kernel_matrix.py) on the GPU, through the C ABI, against the PyTorch
MLPCritic deep-copied to float64 and evaluated S times on x + delta[s] * act_col[row % n] (and once on x for v0).  The float64 input of
a sampled row is the kernel's own f32 value of it — one fused multiply-add, i.e. the exact product and sum rounded once —, as _reference
in tests/test_twin_kernel_matrix_gpu.py takes the kernel's f32 sums.

Bars: baseline and v0 2e-6 of their scale, the bar tests/test_learner_kernel_matrix_gpu.py (_check_head) holds v to: a mean of values
each within the bar is within it.  delta is drawn at the real scale: a standard-normal draw minus a tanh'd action.  Each row runs with
v0 given and with v0 NULL; every output has guard rows on both sides and is pre-filled with a sentinel, and two launches must agree bit
for bit.  The measured figures are printed as "[cf matrix] ..." lines."""
import copy

import pytest
import torch

from mapdn_amd import _lib
from mapdn_amd.learner import MLPCritic, make_alg_args
from tests import cf_kernel_matrix as cm

pytestmark = pytest.mark.gpu
SENT, G = -7777.25, 4
HEAD_PARAMS = ("layernorm.weight", "layernorm.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias")
IDX = list(range(len(cm.ROWS)))


def _dev():
    return torch.device("cuda:0")


def _row(i):
    return cm.rows_for(torch.cuda.get_device_properties(0).multi_processor_count)[i]


def _guarded(n, dev):
    buf = torch.full((2 * G * 64 + n,), SENT, dtype=torch.float32, device=dev)
    return buf, buf[G * 64:G * 64 + n]


def _intact(buf, n):
    return bool((buf[:G * 64] == SENT).all()) and bool((buf[G * 64 + n:] == SENT).all())


def _critic(dev, seed):
    torch.manual_seed(seed)
    cr = MLPCritic(7, 1, make_alg_args(3, 5, 1))
    with torch.no_grad():
        cr.layernorm.weight.copy_(1.0 + 0.3 * torch.randn(64)); cr.layernorm.bias.copy_(0.2 * torch.randn(64))
        cr.fc2.weight.copy_(0.2 * torch.randn(64, 64)); cr.fc2.bias.copy_(0.1 * torch.randn(64))
        cr.fc3.weight.copy_(0.3 * torch.randn(1, 64)); cr.fc3.bias.copy_(0.1 * torch.randn(1))
    return cr.to(dev)


def _head64(cr64, x):
    return cr64.fc3(torch.relu(cr64.fc2(torch.relu(cr64.layernorm(x))))).reshape(-1)


def _inputs(shape, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    n, rows, S = shape["n"], shape["rows"], shape["S"]
    taken = torch.tanh(torch.randn(rows, generator=g))
    return dict(x=(1.2 * torch.randn(rows, 64, generator=g)).to(dev), col=(0.5 * torch.randn(n, 64, generator=g)).to(dev),
                delta=(torch.randn(S, rows, generator=g) - taken).to(dev), n=n, rows=rows, S=S)


def _reference(cr, inp):
    """(baseline, v0) in float64; a sampled row enters as the f32 number the kernel forms: fma(delta, col, x) = the exact product and sum
    (float64 holds both exactly enough: 24 + 24 bits of product, one rounding of the sum far below f32's) rounded to f32"""
    cr64 = copy.deepcopy(cr).double()
    rows, n, S = inp["rows"], inp["n"], inp["S"]
    x64 = inp["x"].double()
    colr = inp["col"].double()[torch.arange(rows, device=x64.device) % n]              # [rows, 64]
    with torch.no_grad():
        total = torch.zeros(rows, dtype=torch.float64, device=x64.device)
        for s in range(S):
            xs = (x64 + inp["delta"][s].double().unsqueeze(1) * colr).float().double()
            total += _head64(cr64, xs)
        return total / S, _head64(cr64, x64)


def _run(cr, inp, with_v0):
    lib, dev, rows = _lib.load(), inp["x"].device, inp["rows"]
    prm = [dict(cr.named_parameters())[k].detach().contiguous().reshape(-1) for k in HEAD_PARAMS]
    pp = [t.data_ptr() for t in prm]
    (bb, base), (vb, v0) = _guarded(rows, dev), _guarded(rows, dev)
    rc = lib.mapdn_critic_head_counterfactual(inp["x"].data_ptr(), inp["n"], inp["col"].data_ptr(), inp["delta"].data_ptr(), inp["S"], pp[0], pp[1],
                                              float(cr.layernorm.eps), pp[2], pp[3], pp[4], pp[5], base.data_ptr(), v0.data_ptr() if with_v0 else None,
                                              rows, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _intact(bb, rows) and _intact(vb, rows)
    if not with_v0:
        assert bool((v0 == SENT).all()), "v0 was NULL and its would-be buffer was written"
    assert not bool((base == SENT).any()) and (not with_v0 or not bool((v0 == SENT).any()))
    return base, (v0 if with_v0 else None)


@pytest.mark.parametrize("with_v0", [True, False], ids=["v0", "nov0"])
@pytest.mark.parametrize("i", IDX, ids=[cm.ROWS[i].label for i in IDX])
def test_cf_baseline_against_float64(i, with_v0):
    row, dev = _row(i), _dev()
    cr = _critic(dev, i)
    inp = _inputs(row.shape, 31 * i + 7, dev)
    (base, v0), (base2, v02) = _run(cr, inp, with_v0), _run(cr, inp, with_v0)
    assert torch.equal(base, base2) and (not with_v0 or torch.equal(v0, v02))          # deterministic: the same bits again
    ref_b, ref_v = _reference(cr, inp)
    for name, got, ref in (("baseline", base, ref_b),) + ((("v0", v0, ref_v),) if with_v0 else ()):
        err, scale = float((got.double() - ref).abs().max()), max(1.0, float(ref.abs().max()))
        print(f"[cf matrix] {row.label} n={row.shape['n']} rows={row.shape['rows']} S={row.shape['S']} {name}: err {err:.3e} bar {2e-6 * scale:.3e}")
        assert err <= 2e-6 * scale, (name, err, 2e-6 * scale)
    assert float((ref_b - ref_v).abs().max()) > 1e-2            # (the samples do move the value: the baseline is not v0 by another name)


def test_cf_v0_is_the_single_head_forward():
    """v0 is head(x): the same tile arithmetic as mapdn_critic_head_forward on rows that are read — bit for bit"""
    lib, dev = _lib.load(), _dev()
    row = _row(2)
    cr = _critic(dev, 2)
    inp = _inputs(row.shape, 99, dev)
    _, v0 = _run(cr, inp, True)
    prm = [dict(cr.named_parameters())[k].detach().contiguous().reshape(-1) for k in HEAD_PARAMS]
    pp = [t.data_ptr() for t in prm]
    v = torch.empty(inp["rows"], device=dev)
    assert lib.mapdn_critic_head_forward(inp["x"].data_ptr(), None, 1, pp[0], pp[1], float(cr.layernorm.eps), pp[2], pp[3], pp[4], pp[5], v.data_ptr(),
                                         inp["rows"], torch.cuda.current_stream(dev).cuda_stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(v, v0)


def test_invalid_shapes_launch_nothing():
    """bad S, n or rows: the error code, and the output buffer keeps its sentinel"""
    lib, dev = _lib.load(), _dev()
    cr = _critic(dev, 0)
    inp = _inputs(dict(n=6, rows=30, S=10), 5, dev)
    prm = [dict(cr.named_parameters())[k].detach().contiguous().reshape(-1) for k in HEAD_PARAMS]
    pp = [t.data_ptr() for t in prm]
    buf, base = _guarded(30, dev)
    for n, S, rows in ((6, 0, 30), (6, cm.S_MAX + 1, 30), (0, 10, 30), (6, 10, 0), (6, 10, 2 ** 31)):
        rc = lib.mapdn_critic_head_counterfactual(inp["x"].data_ptr(), n, inp["col"].data_ptr(), inp["delta"].data_ptr(), S, pp[0], pp[1], 1e-5, pp[2], pp[3],
                                                  pp[4], pp[5], base.data_ptr(), None, rows, torch.cuda.current_stream(dev).cuda_stream)
        assert rc == -1, (n, S, rows, rc)
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())
