"""Every row of the Shapley coalition-critic kernel matrix (tests/shap_kernel_matrix.py) on the GPU, through the C ABI, forward and both
backward modes, against the literal construction of models/sqddpg.py (shap_kernel_matrix.literal_critic_input, then fc1 -> LayerNorm ->
ReLU -> fc2 -> ReLU -> fc3) in float64 under autograd.

Bars are not fixed numbers: for each row and quantity the factored PyTorch float32 route (learner.shapley_first_layer + the same trunk on
the same device) is measured against the same float64 values, and the kernel's bar is 4 x that error — another order of summation —,
with a floor of 1e-6 of the quantity's largest magnitude.  The floor stands for one f32 rounding per summed term, so for sums it grows
with the square root of the number of terms: S for phi and dact, S n for dbase, b S for the rows of d id_cols, b S n for those of d act_cols
(suffix sums over up to n rows of every group) and for the trunk's parameter gradients.  Measured errors and bars are printed as
"[shap matrix] ..." lines.  Every output sits between guard rows pre-filled with a sentinel, and two launches must agree bit for bit."""
import math

import pytest
import torch
import torch.nn.functional as F

from mapdn_amd import _lib
from mapdn_amd import learner
from tests import shap_kernel_matrix as sm

pytestmark = pytest.mark.gpu
SENT, G = -7777.25, 4
IDX = list(range(len(sm.ROWS)))
PRM = ("gamma", "beta", "w2", "b2", "w3", "b3")


def _dev():
    return torch.device("cuda:0")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _row(i):
    return sm.rows_for(_cus())[i]


def _guarded(shape, dev):
    n = math.prod(shape)
    buf = torch.full((2 * G * 64 + n,), SENT, dtype=torch.float32, device=dev)
    return buf, buf[G * 64:G * 64 + n].view(shape)


def _intact(buf, n):
    return bool((buf[:G * 64] == SENT).all()) and bool((buf[G * 64 + n:] == SENT).all())


def _inputs(row, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    b, n, S = row.shape["b"], row.shape["n"], row.shape["S"]
    r = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    t = dict(base=r(b, 64), id_cols=0.3 * r(n, 64), act_cols=0.3 * r(n, 64), act=torch.tanh(r(b, n)), gamma=1.0 + 0.1 * r(64), beta=0.1 * r(64),
             w2=0.15 * r(64, 64), b2=0.1 * r(64), w3=0.15 * r(64), b3=0.1 * r(1), dv=r(b, S, n))
    pos = learner.sample_coalition_positions(b * S, n, "cpu", generator=g).view(b, S, n)
    if row.special == "ident":
        pos = torch.arange(n).expand(b, S, n).contiguous()
    if row.special == "reversed":
        pos = torch.arange(n - 1, -1, -1).expand(b, S, n).contiguous()
    if row.special == "zero-act":
        t["act"] = torch.zeros(b, n)
    if row.special == "hot":
        t["act"] = 100.0 * t["act"]
    t = {k: v.to(dev).contiguous() for k, v in t.items()}
    t["pos"] = pos.to(torch.int32).to(dev).contiguous()
    return t


def _trunk(x, t):
    h = F.relu(F.layer_norm(x, (64,), t["gamma"], t["beta"], 1e-5))
    return F.relu(F.linear(h, t["w2"], t["b2"])) @ t["w3"] + t["b3"]


def _outputs(v, leaves, t, S):
    """forward values and every gradient of sum(v dv) as a dict of detached tensors"""
    grads = torch.autograd.grad((v * t["dv"]).sum(), [leaves[k] for k in ("base", "id_cols", "act_cols", "act") + PRM])
    out = dict(zip(("dbase", "did", "dactc", "dact") + tuple("d" + k for k in PRM), grads))
    out["v"], out["phi"] = v.detach(), v.detach().mean(dim=1)
    return out


def _literal64(t):
    """the reference's input rows through fc1 = [I | act_cols^T | id_cols^T] (the observation block is the identity on base: base IS the
    observation term), then the trunk, in float64"""
    d = {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in t.items()}
    b, S, n = t["pos"].shape
    inp = sm.literal_critic_input(d["base"], d["act"], t["pos"])
    w1 = torch.cat((torch.eye(64, dtype=torch.float64, device=inp.device), d["act_cols"].t(), d["id_cols"].t()), dim=1)
    return _outputs(_trunk(inp @ w1.t(), d).view(b, S, n), d, d, S)


def _factored32(t):
    d = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in t.items()}
    b, S, n = t["pos"].shape
    x = learner.shapley_first_layer(d["base"], d["id_cols"], d["act_cols"], d["act"], t["pos"])
    return _outputs(_trunk(x, d).view(b, S, n), d, d, S)


def _kernel(t):
    lib, dev = _lib.load(), t["base"].device
    b, S, n = t["pos"].shape
    st = torch.cuda.current_stream(dev).cuda_stream
    shapes = dict(v=(b, S, n), phi=(b, n), dbase=(b, 64), grads=(4416 + 2 * n * 64,), dact=(b, n), dact_only=(b, n))
    bufs = {k: _guarded(s, dev) for k, s in shapes.items()}
    sb, scratch = _guarded((lib.mapdn_critic_shapley_scratch_floats(b, S, n),), dev)
    p = lambda k: t[k].data_ptr()                        # noqa: E731
    o = lambda k: bufs[k][1].data_ptr()                  # noqa: E731
    ops = (p("base"), p("id_cols"), p("act_cols"), p("act"), p("pos"), b, S, n, p("gamma"), p("beta"), 1e-5, p("w2"), p("b2"), p("w3"), p("b3"))
    assert lib.mapdn_critic_shapley_forward(*ops, o("v"), o("phi"), st) == 0
    assert lib.mapdn_critic_shapley_backward(p("dv"), *ops, o("dbase"), o("grads"), scratch.data_ptr(), o("dact"), 1, st) == 0
    assert lib.mapdn_critic_shapley_backward(p("dv"), *ops, None, None, None, o("dact_only"), 0, st) == 0
    torch.cuda.synchronize()
    assert _intact(sb, scratch.numel())
    for k, (buf, view) in bufs.items():
        assert _intact(buf, view.numel()), k
        assert not bool((view == SENT).any()), k
    gr = bufs["grads"][1]
    assert not bool(gr[4354:4416].any())                 # the pad of the trunk's block is zeroed by the reduce
    out = {k: bufs[k][1] for k in ("v", "phi", "dbase", "dact", "dact_only")}
    out.update(dw2=gr[:4096].view(64, 64), dgamma=gr[4096:4160], dbeta=gr[4160:4224], db2=gr[4224:4288], dw3=gr[4288:4352], db3=gr[4352:4353],
               did=gr[4416:4416 + n * 64].view(n, 64), dactc=gr[4416 + n * 64:].view(n, 64))
    return out


@pytest.mark.parametrize("i", IDX, ids=[sm.ROWS[i].label for i in IDX])
def test_shapley_critic_against_float64(i):
    row, dev = _row(i), _dev()
    b, n, S = row.shape["b"], row.shape["n"], row.shape["S"]
    cpu_row = sm.ROWS[i]
    for mode, k in ((1, cpu_row.kernels()[1]), (2, cpu_row.kernels()[2])):               # the instantiation the row stands for is the one it reaches
        assert sm.geometry(b, S, n, mode, _cus())[1] == k[2], (row.label, mode)
    t = _inputs(row, 13 * i + 5, dev)
    got, again = _kernel(t), _kernel(t)
    for k in got:
        assert torch.equal(got[k], again[k]), k                                # deterministic: the same bits again
    ref, t32 = _literal64(t), _factored32(t)
    rows = b * S * n
    terms = dict(v=1, phi=S, dact=S, dact_only=S, dbase=S * n, did=b * S, dactc=rows, dw2=rows, dgamma=rows, dbeta=rows, db2=rows, dw3=rows, db3=rows)
    failed = []
    for k in terms:
        rk = "dact" if k == "dact_only" else k
        want = ref[rk].view(got[k].shape)
        assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(got[k]).all()), k
        scale = float(want.abs().max())
        e_torch = float((t32[rk].view(got[k].shape).double() - want).abs().max())
        e_kernel = float((got[k].double() - want).abs().max())
        bar = max(4.0 * e_torch, 1e-6 * scale * math.sqrt(terms[k]))
        print(f"[shap matrix] {row.label} b={b} n={n} S={S} {k}: scale {scale:.3e} torch-f32 err {e_torch:.3e} kernel err {e_kernel:.3e} bar {bar:.3e}")
        if not e_kernel <= bar:
            failed.append((k, e_kernel, bar))
    assert not failed, failed
    if row.special == "zero-act":                                              # P = 0: the central critic's formed rows base[b] + id_cols[i]
        lib = _lib.load()
        hv = torch.empty(b, n, dtype=torch.float32, device=dev)
        assert lib.mapdn_critic_head_forward(t["base"].data_ptr(), t["id_cols"].data_ptr(), n, t["gamma"].data_ptr(), t["beta"].data_ptr(), 1e-5,
                                             t["w2"].data_ptr(), t["b2"].data_ptr(), t["w3"].data_ptr(), t["b3"].data_ptr(), hv.data_ptr(), b * n,
                                             torch.cuda.current_stream(dev).cuda_stream) == 0
        torch.cuda.synchronize()
        diff = float((got["v"] - hv.view(b, 1, n)).abs().max())
        print(f"[shap matrix] zero-act against mapdn_critic_head_forward: max difference {diff:.3e}")
        assert diff <= 2.0 ** -22 * float(hv.abs().max())                      # to fp32 rounding (the same operations: in fact the same bits)
        assert not bool(got["dactc"].any())                                    # d act_cols carries the action as a factor
    if row.special == "hot":
        assert float(t["act"].abs().max()) > 50.0


def test_a_pos_in_pinned_host_memory_is_checked_and_then_read():
    """the permutation check is host-side when the tensor is on the host: a pinned pos with a repeated position is MAPDN_E_INVALID without a
    launch (the outputs keep their sentinel); a pinned permutation gives what the device tensor gives"""
    row, dev = _row(3), _dev()
    t = _inputs(row, 3, dev)
    want = _kernel(t)
    pinned = t["pos"].cpu().pin_memory()
    same = _kernel(dict(t, pos=pinned))
    for k in want:
        assert torch.equal(want[k], same[k]), k
    bad = pinned.clone().pin_memory()
    bad[1, 0, 0] = bad[1, 0, 1]
    lib = _lib.load()
    b, S, n = bad.shape
    buf, v = _guarded((b, S, n), dev)
    p = lambda k: t[k].data_ptr()                        # noqa: E731
    ops = (p("base"), p("id_cols"), p("act_cols"), p("act"), bad.data_ptr(), b, S, n, p("gamma"), p("beta"), 1e-5, p("w2"), p("b2"), p("w3"), p("b3"))
    assert lib.mapdn_critic_shapley_forward(*ops, v.data_ptr(), None, None) == -1
    assert lib.mapdn_critic_shapley_backward(p("dv"), *ops, None, None, None, v.data_ptr(), 0, None) == -1
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())


def test_the_autograd_function_is_the_kernels(monkeypatch):
    """SQDDPGNet.marginal_contribution on a CUDA float32 batch with the default critic takes _ShapleyCritic and returns what the C ABI
    returns for the operands it forms; MAPDN_FUSED_SHAP=0 does not take it"""
    dev = _dev()
    n, o, b, S = 5, 6, 9, 3
    torch.manual_seed(1)
    net = learner.SQDDPGNet(learner.make_alg_args(n, o, 1, alg="sqddpg", sample_size=S)).to(dev)
    obs, act = torch.randn(b, n, o, device=dev), torch.tanh(torch.randn(b, n, 1, device=dev)).requires_grad_(True)
    pos = net.sample_coalitions(b, dev)
    before = learner._ShapleyCritic.launches
    v = net.marginal_contribution(obs, act, pos)
    assert learner._ShapleyCritic.launches == before + 1 and v.shape == (b, S, n, 1)
    cr = net.value_dicts[0]
    w = cr.fc1.weight.detach()
    t = dict(base=F.linear(obs.reshape(b, -1), w[:, :n * o], cr.fc1.bias.detach()), id_cols=w[:, n * o + n:].t().contiguous(),
             act_cols=w[:, n * o:n * o + n].t().contiguous(), act=act.detach().reshape(b, n).contiguous(), pos=pos.to(torch.int32).contiguous(),
             gamma=cr.layernorm.weight.detach(), beta=cr.layernorm.bias.detach(), w2=cr.fc2.weight.detach(), b2=cr.fc2.bias.detach(),
             w3=cr.fc3.weight.detach().reshape(64).contiguous(), b3=cr.fc3.bias.detach(), dv=torch.randn(b, S, n, device=dev))
    want = _kernel(t)
    assert torch.equal(v.detach().view(b, S, n), want["v"])
    grads = torch.autograd.grad((v.view(b, S, n) * t["dv"]).sum(), [act, cr.fc2.weight, cr.fc1.weight])
    assert torch.equal(grads[0].view(b, n), want["dact"]) and torch.equal(grads[1], want["dw2"])
    assert torch.equal(grads[2][:, n * o:n * o + n].t(), want["dactc"]) and torch.equal(grads[2][:, n * o + n:].t(), want["did"])
    monkeypatch.setenv("MAPDN_FUSED_SHAP", "0")
    v0 = net.marginal_contribution(obs, act, pos)
    assert learner._ShapleyCritic.launches == before + 1
    assert float((v0 - v).abs().max()) <= 1e-5 * max(1.0, float(v.abs().max()))
