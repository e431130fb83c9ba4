"""The learner's building blocks on tall batches (millions of rows of 64): LayerNorm + ReLU and ReLU + one-output layer as HIP launches
(csrc/policy.hip), and the weight gradient of a tall linear layer split over row blocks (_TallLinear, _splitk_dw).  Each *_ok / route
function says when its kernel applies; the PyTorch modules remain otherwise."""

import os
from typing import Dict

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._hip import buffer, launch


class _LayerNorm64(torch.autograd.Function):
    """LayerNorm over 64 features with the ReLU that follows it in both reference modules fused in (agents/rnn_agent.py:16-21,
    critics/mlp_critic.py:22-27), forward and backward as hand-written HIP kernels (libmapdn_hip.so: mapdn_layernorm64_*): at the
    reference's update intensity a batch is millions of rows of 64, where the stock kernels run at an eighth of the HBM rate."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, relu):
        x2 = x.reshape(-1, 64).contiguous()
        w, b = weight.detach().contiguous(), bias.detach().contiguous()
        rows = x2.shape[0]
        y = torch.empty_like(x2)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        launch("mapdn_layernorm64_forward", x.device, x2, w, b, y, mean, rstd, rows, float(eps), int(relu))
        ctx.save_for_backward(x2, w, b, mean, rstd)
        ctx.relu, ctx.shape = bool(relu), x.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, w, b, mean, rstd = ctx.saved_tensors
        rows = x2.shape[0]
        dy2 = dy.reshape(-1, 64).contiguous()
        dx = torch.empty_like(x2)
        dw, db = torch.empty_like(w), torch.empty_like(b)
        partial = buffer("mapdn_layernorm64_backward_blocks", x2.device, rows, per=128)
        launch("mapdn_layernorm64_backward", x2.device, dy2, x2, w, b, mean, rstd, dx, dw, db, partial, rows, int(ctx.relu))
        return dx.view(ctx.shape), dw, db, None, None


class _TallLinear(torch.autograd.Function):
    """y = x W^T + b for x of MILLIONS of rows and a small weight (the 64 -> 64 and 64 -> 1 layers of the critic / agent trunks on a
    batch of 32 x 8192 transitions x 38 agents = 10 M rows).  Forward and dX are ordinary GEMMs; the WEIGHT gradient dW = dy^T x is a
    [out, in] product with the 10 M rows as its reduction dimension — the BLAS back end runs it on two workgroups (8.4 ms and 5.6 ms
    per call, the two largest GEMM entries of profiles/e2e/r04_e2e_reference_kernel_stats.txt, against 1.3 ms for the forward).  Here
    the rows are cut into blocks whose partial products are one batched GEMM, then summed (split-K by hand): same sum, other order."""

    BLOCK_ROWS = 16384

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return F.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = dy @ weight
        if ctx.needs_input_grad[1]:
            rows = x.shape[0]
            dw = _splitk_dw(dy.reshape(rows, -1).contiguous(), x.reshape(rows, -1).contiguous(),      # (a permuted upstream gradient is not viewable)
                            blk=_TallLinear.BLOCK_ROWS)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy.reshape(-1, dy.shape[-1]).sum(0)
        return dx, dw, db


def tall_linear(lin: nn.Linear, x: torch.Tensor) -> torch.Tensor:
    """lin(x); with the hand-split weight gradient when x is a tall 2-D batch on the GPU (>= 2^18 rows, <= 128 features each way)"""
    if x.dim() == 2 and _tall_ok(x, x.shape[0], lin.weight):
        return _TallLinear.apply(x, lin.weight, lin.bias)
    return lin(x)


def tall_linear_w(x: torch.Tensor, weight: torch.Tensor, bias=None) -> torch.Tensor:
    """x W^T (+ b) for a weight given as a tensor (a column slice of a larger layer): _TallLinear on a tall GPU batch under autograd.
    The central critic's observation block (K = n * obs = 2204-3116 inputs, 2^18 rows of reduction) included: its weight gradient as 16
    batched products + a sum is 0.3 ms faster per update than the back end's single GEMM (round 6, same-box A/B: value update 0.216 ->
    0.205 s per episode); MAPDN_TALL_LINEAR_WIDE=0 keeps the stock backward for weights wider than 128 inputs."""
    if x.dim() == 2 and _tall_ok(x, x.shape[0], weight, wide=os.environ.get("MAPDN_TALL_LINEAR_WIDE", "1") != "0"):
        return _TallLinear.apply(x, weight, bias)
    return F.linear(x, weight, bias)


def _tall_ok(x: torch.Tensor, rows: int, weight: torch.Tensor, wide: bool = False) -> bool:
    return (x.is_cuda and rows >= (1 << 18) and weight.shape[0] <= 256 and (weight.shape[1] <= 128 or wide) and torch.is_grad_enabled()
            and weight.requires_grad and os.environ.get("MAPDN_TALL_LINEAR", "1") != "0")


_GRU_FUSED_OK: Dict[str, bool] = {}


def _gru_fused_ok(device) -> bool:
    """one-time self-check of the route gru_cell_tall takes (input / hidden projections as _TallLinear, then ATen's fused GRU cell on
    the pre-computed gates) against nn.GRUCell, values and gradients; any exception or mismatch disables the route for the process"""
    key = str(device)
    if key not in _GRU_FUSED_OK:
        ok = False
        try:
            g = torch.Generator(device="cpu").manual_seed(1)
            with torch.random.fork_rng(devices=[]):          # nn.GRUCell's initialisation draws from the GLOBAL generator: leave the caller's stream alone
                cell = nn.GRUCell(8, 8).to(device)
            x = torch.randn(32, 8, generator=g).to(device).requires_grad_(True)
            h = torch.randn(32, 8, generator=g).to(device).requires_grad_(True)
            ref = cell(x, h)
            gr = torch.autograd.grad(ref.square().sum(), [x, h, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh])
            out = torch.ops.aten._thnn_fused_gru_cell(_TallLinear.apply(x, cell.weight_ih, None), _TallLinear.apply(h, cell.weight_hh, None),
                                                      h, cell.bias_ih, cell.bias_hh)[0]
            go = torch.autograd.grad(out.square().sum(), [x, h, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh])
            ok = bool(torch.allclose(out, ref, rtol=1e-5, atol=1e-6)) and all(bool(torch.allclose(a, b, rtol=1e-4, atol=1e-5)) for a, b in zip(go, gr))
        except Exception:                      # noqa: BLE001 — an ATen signature change must not break training: the stock cell is used
            ok = False
        _GRU_FUSED_OK[key] = ok
    return _GRU_FUSED_OK[key]


def gru_cell_tall(rnn: nn.GRUCell, x: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
    """rnn(x, h); on a tall GPU batch under autograd the two projections go through _TallLinear (their weight gradients are products
    with millions of rows of reduction) and ATen's fused cell does the gate arithmetic, as inside nn.GRUCell"""
    if x.dim() == 2 and _tall_ok(x, x.shape[0], rnn.weight_ih) and rnn.bias and _gru_fused_ok(x.device):
        ig = _TallLinear.apply(x, rnn.weight_ih, None)
        hg = _TallLinear.apply(h, rnn.weight_hh, None)
        return torch.ops.aten._thnn_fused_gru_cell(ig, hg, h, rnn.bias_ih, rnn.bias_hh)[0]
    return rnn(x, h)


class _LayerNorm64BC(torch.autograd.Function):
    """relu(LayerNorm(base[b] + per_n[i])) for every (b, i), rows ordered (b, i), WITHOUT materialising the [b, n, 64] sum — the central
    critic's first layer (DDPGNet._value_central) is exactly such a sum: W_obs·obs_all + bias per batch element plus the agent's id
    column.  HIP kernels mapdn_layernorm64_bc_* (csrc/policy.hip): the row is formed in registers (one f32 add, as PyTorch's broadcast
    add would), forward and backward; the backward hands back dx per formed row, reduced here over the agents / over the batch."""

    @staticmethod
    def forward(ctx, base, per_n, weight, bias, eps, relu):
        b2, p2 = base.contiguous(), per_n.contiguous()
        w, bb = weight.detach().contiguous(), bias.detach().contiguous()
        nb, n = b2.shape[0], p2.shape[0]
        rows = nb * n
        y = torch.empty(rows, 64, dtype=torch.float32, device=base.device)
        mean = torch.empty(rows, dtype=torch.float32, device=base.device)
        rstd = torch.empty_like(mean)
        launch("mapdn_layernorm64_bc_forward", base.device, b2, p2, n, w, bb, y, mean, rstd, rows, float(eps), int(relu))
        ctx.save_for_backward(b2, p2, w, bb, mean, rstd)
        ctx.relu = bool(relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        b2, p2, w, bb, mean, rstd = ctx.saved_tensors
        nb, n = b2.shape[0], p2.shape[0]
        rows = nb * n
        dy2 = dy.reshape(rows, 64).contiguous()
        dx = torch.empty_like(dy2)
        dw, db = torch.empty_like(w), torch.empty_like(bb)
        partial = buffer("mapdn_layernorm64_backward_blocks", b2.device, rows, per=128)
        launch("mapdn_layernorm64_bc_backward", b2.device, dy2, b2, p2, n, w, bb, mean, rstd, dx, dw, db, partial, rows, int(ctx.relu))
        dx3 = dx.view(nb, n, 64)
        dbase = dx3.sum(1) if ctx.needs_input_grad[0] else None
        dpern = dx3.sum(0) if ctx.needs_input_grad[1] else None
        return dbase, dpern, dw, db, None, None


class _ReluDot64(torch.autograd.Function):
    """v = relu(pre) @ w^T + b for pre [rows, 64], w [1, 64]: the critic's activation after fc2 and its one-output fc3 as one pass
    over the pre-activation (mapdn_relu_dot64_*, csrc/policy.hip); relu(pre) is never materialised, forward or backward."""

    @staticmethod
    def forward(ctx, pre, weight, bias):
        p2 = pre.contiguous()
        w = weight.detach().reshape(64).contiguous()
        rows = p2.shape[0]
        v = torch.empty(rows, 1, dtype=torch.float32, device=pre.device)
        launch("mapdn_relu_dot64_forward", pre.device, p2, w, 0.0, v, rows)
        ctx.save_for_backward(p2, w)
        return v + bias.detach()          # (the bias stays a device tensor: no host read of a parameter inside the training loop)

    @staticmethod
    def backward(ctx, dv):
        p2, w = ctx.saved_tensors
        rows = p2.shape[0]
        dv2 = dv.reshape(rows).contiguous()
        dpre = torch.empty_like(p2)
        dw, db = torch.empty(64, dtype=torch.float32, device=p2.device), torch.empty(64, dtype=torch.float32, device=p2.device)
        partial = buffer("mapdn_layernorm64_backward_blocks", p2.device, rows, per=128)
        launch("mapdn_relu_dot64_backward", p2.device, dv2, p2, w, dpre, dw, db, partial, rows)
        return dpre, dw.view(1, 64), db[:1].clone()


def relu_dot64_ok(act, fc3: nn.Linear, pre: torch.Tensor) -> bool:
    return (pre.is_cuda and pre.dtype == torch.float32 and pre.dim() == 2 and pre.shape[1] == 64 and pre.shape[0] >= 64 * 1024 and act is F.relu
            and fc3.out_features == 1 and fc3.bias is not None and os.environ.get("MAPDN_FUSED_RELU_DOT", "1") != "0")


def layernorm_act_bc(ln: nn.LayerNorm, act, base: torch.Tensor, per_n: torch.Tensor):
    """act(LayerNorm(base.unsqueeze(1) + per_n.unsqueeze(0))).reshape(b * n, 64) through the broadcast-input kernels, or None when the
    case is not theirs (the caller then forms the sum and takes layernorm_act)"""
    if (base.is_cuda and base.dtype == torch.float32 and per_n.dtype == torch.float32 and base.dim() == 2 and per_n.dim() == 2
            and base.shape[-1] == 64 and per_n.shape[-1] == 64 and act is F.relu and ln.elementwise_affine and ln.bias is not None
            and ln.weight.dtype == torch.float32 and base.shape[0] * per_n.shape[0] >= 1024
            and os.environ.get("MAPDN_FUSED_LN", "1") != "0" and os.environ.get("MAPDN_FUSED_LN_BC", "1") != "0"):
        return _LayerNorm64BC.apply(base, per_n, ln.weight, ln.bias, ln.eps, True)
    return None


def layernorm_act(ln: nn.LayerNorm, act, x: torch.Tensor) -> torch.Tensor:
    """act(LayerNorm(x)): one HIP launch each way for the reference's default shape (64 features, ReLU, fp32, on the GPU), the
    PyTorch modules otherwise (MAPDN_FUSED_LN=0 forces them)."""
    if (x.is_cuda and x.dtype == torch.float32 and x.shape[-1] == 64 and act is F.relu and ln.elementwise_affine and ln.bias is not None
            and ln.weight.dtype == torch.float32 and x.numel() >= 64 * 1024 and os.environ.get("MAPDN_FUSED_LN", "1") != "0"):
        return _LayerNorm64.apply(x, ln.weight, ln.bias, ln.eps, True)
    return act(ln(x))


def _splitk_dw(dy2: torch.Tensor, x2: torch.Tensor, blk: int = 16384) -> torch.Tensor:
    """dy2^T x2 ([out, in]) for [rows, out] x [rows, in] with millions of rows: the rows cut into blocks whose partial products are one
    batched GEMM, then summed (_TallLinear.backward's weight gradient).  dy2 may be a column slice of a wider tensor."""
    rows = x2.shape[0]
    full = rows // blk * blk
    dw = None
    if full:
        a = dy2[:full].unflatten(0, (-1, blk)).transpose(1, 2)
        dw = torch.bmm(a, x2[:full].unflatten(0, (-1, blk))).sum(0)
    if full < rows:
        rest = dy2[full:].t() @ x2[full:]
        dw = rest if dw is None else dw + rest
    return dw
