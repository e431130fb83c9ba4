"""Every row of the twin-critic kernel matrix (tests/twin_kernel_matrix.py) on the GPU, through the C ABI, against autograd through the
PyTorch MLPCritic deep-copied to float64 and evaluated twice: on x = base[b] + per_n[i] (flag 0) and on x + flag_col (flag 1).

Bars: those tests/test_learner_kernel_matrix_gpu.py holds the single head to (_check_head) — values (v1, v2, and vmin: the minimum of two
values each within the bar is within it, whichever head wins) 2e-6 of their scale, the loss 3e-6, every gradient of the fused loss 2e-4
of that gradient's maximum; d flag_col additionally 3e-7 sqrt(rows) x 4 of its scale (the bar of dper_n with rows in the place of nb).
No bar was widened for the two-head sums.  Inputs are moved off the ReLU kinks of BOTH heads, decided by the float64 modules alone.
Every output has guard rows on both sides, scratch and grads are filled with NaN before the launch, and two launches must agree bit
for bit.  The measured figures are printed as "[twin matrix] ..." lines."""
import copy

import pytest
import torch

from mapdn_amd import _lib
from mapdn_amd.learner import MLPCritic, make_alg_args
from tests import twin_kernel_matrix as tm

pytestmark = pytest.mark.gpu
SENT, G, KINK = -7777.25, 4, 2e-5
HEAD_PARAMS = ("layernorm.weight", "layernorm.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias")
GRAD_SLICES = ((4096, 4160), (4160, 4224), (0, 4096), (4224, 4288), (4288, 4352), (4352, 4353))      # of grads, in HEAD_PARAMS order
MSE_IDX = [i for i, r in enumerate(tm.ROWS) if r.kernel[0] == "twin_mse"]
FWD_IDX = [i for i, r in enumerate(tm.ROWS) if r.kernel[0] == "twin_fwd"]


def _dev():
    return torch.device("cuda:0")


def _row(i):
    return tm.rows_for(torch.cuda.get_device_properties(0).multi_processor_count)[i]


def _guarded(n, dev):
    buf = torch.full((2 * G * 64 + n,), SENT, dtype=torch.float32, device=dev)
    return buf, buf[G * 64:G * 64 + n]


def _intact(buf, n):
    return bool((buf[:G * 64] == SENT).all()) and bool((buf[G * 64 + n:] == SENT).all())


def _err(a, ref):
    return float((a.double() - ref.double()).abs().max())


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
    nb, n = shape["nb"], shape["n"]
    return dict(x=(1.2 * torch.randn(nb, 64, generator=g)).to(dev), pern=(0.8 * torch.randn(n, 64, generator=g)).to(dev),
                flag=(0.7 * torch.randn(64, generator=g)).to(dev), n=n, nb=nb, rows=nb * n, ret=torch.randn(nb * n, generator=g).to(dev),
                wrow=(torch.rand(nb, generator=g) < 0.7).float().to(dev))


def _off_the_kinks(cr, inp, seed):
    """as tests/test_learner_kernel_matrix_gpu.py: groups with a pre-activation of EITHER head within KINK of 0 (float64 modules) are redrawn"""
    cr64 = copy.deepcopy(cr).double()
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    for _ in range(80):
        x = (inp["x"].unsqueeze(1) + inp["pern"].unsqueeze(0)).reshape(-1, 64)
        bad = torch.zeros(inp["nb"], dtype=torch.bool, device=x.device)
        with torch.no_grad():
            for xx in (x, x + inp["flag"]):
                y = cr64.layernorm(xx.double())
                pre = cr64.fc2(torch.relu(y))
                bad |= ((y.abs() < KINK) | (pre.abs() < KINK)).any(-1).view(inp["nb"], inp["n"]).any(-1)
        k = int(bad.sum())
        if not k:
            return inp
        inp["x"][bad] = (1.2 * torch.randn(k, 64, generator=g)).to(inp["x"].device)
    raise AssertionError("could not move the rows off the ReLU kinks")


def _ptrs(cr):
    prm = [dict(cr.named_parameters())[k].detach().contiguous().reshape(-1) for k in HEAD_PARAMS]
    return prm, [t.data_ptr() for t in prm]


def _reference(cr, inp):
    """float64 leaves; the VALUE of a row is the kernel's f32 sums (one add for the first head, one more for the second)"""
    cr64 = copy.deepcopy(cr).double()
    prm64 = [dict(cr64.named_parameters())[k] for k in HEAD_PARAMS]
    rows = inp["rows"]
    base, pern, flag = (inp[k].double().requires_grad_(True) for k in ("x", "pern", "flag"))
    x32 = (inp["x"].unsqueeze(1) + inp["pern"].unsqueeze(0)).reshape(rows, 64)
    e1 = (base.unsqueeze(1) + pern.unsqueeze(0)).reshape(rows, 64)
    x1 = e1 + (x32.double() - e1).detach()
    e2 = e1 + flag
    x2 = e2 + ((x32 + inp["flag"]).double() - e2).detach()
    return _head64(cr64, x1), _head64(cr64, x2), [base, pern, flag] + prm64


def _run_fwd(cr, inp, outputs):
    lib, dev, rows = _lib.load(), inp["x"].device, inp["rows"]
    keep, pp = _ptrs(cr)
    bufs = {k: _guarded(rows, dev) for k in outputs}
    ptr = [bufs[k][1].data_ptr() if k in bufs else None for k in ("v1", "v2", "vmin")]
    rc = lib.mapdn_critic_twin_forward(inp["x"].data_ptr(), inp["pern"].data_ptr(), inp["n"], inp["flag"].data_ptr(), pp[0], pp[1], float(cr.layernorm.eps),
                                       pp[2], pp[3], pp[4], pp[5], ptr[0], ptr[1], ptr[2], rows, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert _intact(buf, rows), k
    return {k: v for k, (_, v) in bufs.items()}


def _run_mse(cr, inp, weighted):
    lib, dev = _lib.load(), inp["x"].device
    rows, n, nb = inp["rows"], inp["n"], inp["nb"]
    keep, pp = _ptrs(cr)
    ng, ns = tm.TP + n * 64, max(1, lib.mapdn_critic_twin_scratch_floats(rows, n))
    (gb, grads), (sb, scratch), (xb, dbase) = _guarded(ng, dev), _guarded(ns, dev), _guarded(nb * 64, dev)
    grads.fill_(float("nan")); scratch.fill_(float("nan"))
    wr = inp["wrow"] if weighted else None
    scale = (1.0 / (wr.sum().clamp(min=1.0) * n)).reshape(1) if weighted else torch.full((1,), 1.0 / rows, device=dev)
    rc = lib.mapdn_critic_twin_mse(inp["ret"].data_ptr(), wr.data_ptr() if weighted else None, scale.data_ptr(), inp["x"].data_ptr(), inp["pern"].data_ptr(), n,
                                   inp["flag"].data_ptr(), pp[0], pp[1], float(cr.layernorm.eps), pp[2], pp[3], pp[4], pp[5], dbase.data_ptr(), grads.data_ptr(),
                                   scratch.data_ptr(), rows, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _intact(xb, nb * 64) and _intact(gb, ng) and _intact(sb, ns)
    return dict(dbase=dbase.view(nb, 64), grads=grads, scratch=scratch, scale=scale)


def _check_pads(out, inp, blocks):
    """the pad rule of include/mapdn.h: pad elements of grads are zero, pad columns of scratch are neither read nor written, every
    documented element is finite, nothing beyond blocks x stride of scratch is touched"""
    n, grads, scratch = inp["n"], out["grads"], out["scratch"]
    assert bool(torch.isfinite(grads[:tm.HW]).all()) and bool((grads[tm.HW:tm.HP] == 0).all()) and bool(torch.isfinite(grads[tm.HP:]).all())
    stride = tm.TP + n * 64
    part = scratch[:blocks * stride].view(blocks, stride)
    assert bool(part[:, tm.HW:tm.HP].isnan().all()), "a pad column of scratch was written"
    assert bool(torch.isfinite(part[:, :tm.HW]).all()) and bool(torch.isfinite(part[:, tm.HP:]).all())
    assert bool(scratch[blocks * stride:].isnan().all())


@pytest.mark.parametrize("i", FWD_IDX, ids=[tm.ROWS[i].label for i in FWD_IDX])
def test_twin_forward_against_float64(i):
    row, dev = _row(i), _dev()
    cr = _critic(dev, i)
    inp = _inputs(row.shape, 31 * i + 7, dev)
    out, again = _run_fwd(cr, inp, row.opts["outputs"]), _run_fwd(cr, inp, row.opts["outputs"])
    with torch.no_grad():
        r1, r2, _ = _reference(cr, inp)
    ref = dict(v1=r1, v2=r2, vmin=torch.minimum(r1, r2))
    assert set(out) == set(row.opts["outputs"])
    for k, v in out.items():
        assert torch.equal(v, again[k]), k
        err, scale = _err(v, ref[k]), max(1.0, float(ref[k].abs().max()))
        print(f"[twin matrix] {row.label} {k}: err {err:.3e} bar {2e-6 * scale:.3e}")
        assert err <= 2e-6 * scale, (k, err, 2e-6 * scale)
    if "vmin" in out and "v1" in out and "v2" in out:
        assert torch.equal(out["vmin"], torch.minimum(out["v1"], out["v2"]))


@pytest.mark.parametrize("i", MSE_IDX, ids=[tm.ROWS[i].label for i in MSE_IDX])
def test_twin_mse_against_float64(i):
    row, dev = _row(i), _dev()
    assert tm.reported_kernel(row, cus=0) == row.kernel                  # asked of this device, before the launch
    cr = _critic(dev, i)
    inp = _off_the_kinks(cr, _inputs(row.shape, 31 * i + 7, dev), i)
    rows, n, nb, weighted = inp["rows"], inp["n"], inp["nb"], row.opts["wrow"]
    blocks = _lib.critic_twin_geometry(rows, n, 0)[1]
    out, again = _run_mse(cr, inp, weighted), _run_mse(cr, inp, weighted)
    for k in ("dbase", "grads"):
        assert torch.equal(out[k], again[k]), k                          # deterministic: a second launch gives the same bits
    _check_pads(out, inp, blocks)
    r1, r2, leaves = _reference(cr, inp)
    w = (inp["wrow"].double().repeat_interleave(n) if weighted else torch.ones(rows, dtype=torch.float64, device=dev)) * out["scale"].double()
    ret = inp["ret"].double()
    loss = (w * 0.5 * ((ret - r1) ** 2 + (ret - r2) ** 2)).sum()
    want = torch.autograd.grad(loss, leaves)
    got_loss = float(out["grads"][4353])
    loss = loss.detach()
    assert abs(got_loss - float(loss)) <= 3e-6 * max(1.0, abs(float(loss))), ("loss", got_loss, float(loss))
    g = out["grads"]
    got = [out["dbase"], g[tm.TP:].view(n, 64), g[tm.HP:tm.TP]] + [g[lo:hi] for lo, hi in GRAD_SLICES]
    names = ("dbase", "dper_n", "dflag") + HEAD_PARAMS
    for name, a, b in zip(names, got, want):
        err, ref_max = _err(a.reshape(-1), b.reshape(-1)), float(b.abs().max())
        print(f"[twin matrix] {row.label} {name}: err {err:.3e} of max {ref_max:.3e} = {err / max(ref_max, 1e-300):.2e} (bar 2e-4)")
        assert err <= 2e-4 * ref_max, (name, err, ref_max)
    assert _err(g[tm.HP:tm.TP], want[2]) <= 3e-7 * max(1.0, rows ** 0.5) * 4 * max(1.0, float(want[2].abs().max()))


def test_twin_mse_agrees_with_two_single_head_launches():
    """the same loss and gradients as mapdn_critic_head_mse on per_n and on per_n + flag_col, halved and summed (f32 against f32: the
    value of a row differs by the order of the two adds, hence a bar and not bit equality)"""
    lib, dev = _lib.load(), _dev()
    cr = _critic(dev, 5)
    inp = _off_the_kinks(cr, _inputs(dict(nb=4099, n=38), 77, dev), 77)
    rows, n, nb = inp["rows"], inp["n"], inp["nb"]
    out = _run_mse(cr, inp, True)
    keep, pp = _ptrs(cr)
    tot_dx, tot_g = torch.zeros(nb, 64, device=dev), torch.zeros(tm.HP + n * 64, device=dev)
    half = out["scale"] * 0.5
    for pern in (inp["pern"], (inp["pern"] + inp["flag"]).contiguous()):
        dx, grads = torch.empty(nb, 64, device=dev), torch.empty(tm.HP + n * 64, device=dev)
        scratch = torch.empty(lib.mapdn_critic_head_scratch_floats(rows, n, 1), device=dev)
        assert lib.mapdn_critic_head_mse(inp["ret"].data_ptr(), inp["wrow"].data_ptr(), half.data_ptr(), inp["x"].data_ptr(), pern.data_ptr(), n, pp[0], pp[1],
                                         float(cr.layernorm.eps), pp[2], pp[3], pp[4], pp[5], dx.data_ptr(), grads.data_ptr(), scratch.data_ptr(), rows,
                                         torch.cuda.current_stream(dev).cuda_stream) == 0
        tot_dx += dx; tot_g += grads
    torch.cuda.synchronize()
    g = out["grads"]
    for name, a, b in (("dbase", out["dbase"], tot_dx), ("head", g[:tm.HW], tot_g[:tm.HW]), ("dper_n", g[tm.TP:], tot_g[tm.HP:])):
        assert _err(a, b) <= 2e-4 * float(b.abs().max()), (name, _err(a, b), float(b.abs().max()))
