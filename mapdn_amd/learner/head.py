"""Everything of the reference's default critic behind its first layer (critics/mlp_critic.py:22-36: LayerNorm -> ReLU -> fc2 64 -> 64 ->
ReLU -> fc3 -> 1) as HIP launches: the head (csrc/critic.hip), its value loss in one launch, MATD3's twin (csrc/critic_twin.hip: ONE
critic valued twice, matd3.py:35-86) and COMA's counterfactual baseline (csrc/critic_cf.hip, coma.py:139-151).  The head's six parameters
and its gradient block are described ONCE here — head_params / head_pack / head_abi and HEAD_GRADS / head_param_grads — for every wrapper
that launches a head kernel (the coalition critic of sqddpg.py included)."""

import os
from typing import Optional

import torch
import torch.nn.functional as F

from ._hip import buffer, launch


def head_params(cr: "MLPCritic"):
    """the head's seven arguments of every wrapper's .apply, in their order"""
    ln = cr.layernorm
    return ln.weight, ln.bias, ln.eps, cr.fc2.weight, cr.fc2.bias, cr.fc3.weight, cr.fc3.bias


def head_pack(ln_w, ln_b, w2, b2, w3, b3):
    """the six parameter tensors as the kernels read them (detached, contiguous, fc3 flat), in the order of the C ABI"""
    return tuple(t.detach().contiguous() for t in (ln_w, ln_b, w2, b2, w3.reshape(64), b3.reshape(1)))


def head_abi(prm, eps):
    """head_pack's tuple as launch arguments: the C ABI has eps between ln_b and w2"""
    return (*prm[:2], float(eps), *prm[2:])


def _head_abi_of(cr: "MLPCritic"):
    ln_w, ln_b, eps, w2, b2, w3, b3 = head_params(cr)
    return head_abi(head_pack(ln_w, ln_b, w2, b2, w3, b3), eps)


# The gradient block of the head kernels (include/mapdn.h, mapdn_critic_head_backward; csrc/rowtile.hpp HP / HW), in floats:
# dW2 [0, 4096) | dgamma [4096, 4160) | dbeta [4160, 4224) | db2 [4224, 4288) | dw3 [4288, 4352) | db3 4352 | loss 4353 | zero pad to 4416,
# then the tails: dper_n [n][64] (formed rows); the twin: d flag_col [4416, 4480), then dper_n; the coalition critic: d id_cols, d act_cols.
HEAD_GRADS, HEAD_LOSS, TWIN_GRADS = 4416, 4353, 4480


def head_param_grads(gs: torch.Tensor):
    """views of a gradient block (scaled by the incoming gradient or not) as the seven .apply slots of head_params: (dgamma, dbeta, None
    for eps, dW2, db2, dw3, db3)"""
    return gs[4096:4160], gs[4160:4224], None, gs[:4096].view(64, 64), gs[4224:4288], gs[4288:4352].view(1, 64), gs[4352:4353]


def head_dper_n(gs: torch.Tensor, n: int) -> torch.Tensor:
    return gs[HEAD_GRADS:].view(n, 64)


def twin_tails(gs: torch.Tensor, n: int):
    """(dper_n [n, 64], d flag_col [64]) behind the head's block (mapdn_critic_twin_mse)"""
    return gs[TWIN_GRADS:].view(n, 64), gs[HEAD_GRADS:TWIN_GRADS]


def shapley_tails(gs: torch.Tensor, n: int):
    """(d id_cols [n, 64], d act_cols [n, 64]) behind the head's block (mapdn_critic_shapley_backward)"""
    return gs[HEAD_GRADS:HEAD_GRADS + n * 64].view(n, 64), gs[HEAD_GRADS + n * 64:].view(n, 64)


def default_critic_fp32(cr: "MLPCritic") -> bool:
    """is `cr` the reference's default critic — LayerNorm with weight and bias, ReLU, fc2 64 -> 64 and fc3 -> 1 with biases — in fp32?"""
    return (cr.use_ln and cr.act is F.relu and cr.layernorm.elementwise_affine and cr.layernorm.bias is not None and cr.fc2.in_features == 64
            and cr.fc2.out_features == 64 and cr.fc2.bias is not None and cr.fc3.out_features == 1 and cr.fc3.bias is not None
            and cr.fc2.weight.dtype == torch.float32)


def _head_forward(ctx, x2, pn, prm, eps):
    """the forward launch of _CriticHead and _CriticHeadOwnAction on their (contiguous) operands: v [rows, 1]; ctx gets eps, n and rows"""
    ctx.eps, ctx.n = float(eps), pn.shape[0] if pn is not None else 1
    ctx.rows = x2.shape[0] * ctx.n
    v = torch.empty(ctx.rows, 1, dtype=torch.float32, device=x2.device)
    launch("mapdn_critic_head_forward", x2.device, x2, pn, ctx.n, *head_abi(prm, eps), v, ctx.rows)
    return v


class _CriticHead(torch.autograd.Function):
    """v = relu(relu(LayerNorm(x)) W2^T + b2) . w3 + b3 on rows of 64 — everything of the critic behind its first layer
    (critics/mlp_critic.py:22-36) — as ONE HIP launch forward and one backward (libmapdn_hip.so: mapdn_critic_head_*, csrc/critic.hip:
    fp32 MFMA, the 16-row tile stays in registers from the LayerNorm input to v / from dv to dx and the parameter gradients; the backward
    recomputes the forward, so nothing but the inputs is saved).  x is read ([rows, 64], per_n None) or formed as base[b] + per_n[i]
    (rows ordered (b, i): the central critic); the backward then returns dbase / dper_n already summed over the agents / the batch."""

    @staticmethod
    def forward(ctx, x, per_n, ln_w, ln_b, eps, w2, b2, w3, b3):
        x2 = x.contiguous()
        pn = per_n.contiguous() if per_n is not None else None
        prm = head_pack(ln_w, ln_b, w2, b2, w3, b3)
        ctx.save_for_backward(x2, pn, *prm)
        return _head_forward(ctx, x2, pn, prm, eps)

    @staticmethod
    def backward(ctx, dv):
        x2, pn, *prm = ctx.saved_tensors
        rows, n, formed = ctx.rows, ctx.n, pn is not None
        need = ctx.needs_input_grad
        param_grads = bool(need[2] or need[3] or need[5] or need[6] or need[7] or need[8])
        dv2 = dv.reshape(rows).contiguous()
        dx = torch.empty_like(x2)
        dev = x2.device
        grads = torch.empty(HEAD_GRADS + (n * 64 if formed else 0), dtype=torch.float32, device=dev)
        scratch = buffer("mapdn_critic_head_scratch_floats", dev, rows, n, int(formed), at_least=1)
        launch("mapdn_critic_head_backward", dev, dv2, x2, pn, n, *head_abi(prm, ctx.eps), dx, grads, scratch, rows, int(param_grads))
        dpn = head_dper_n(grads, n) if formed and need[1] else None
        return (dx, dpn) + (head_param_grads(grads) if param_grads else (None,) * 7)


class _CriticHeadOwnAction(torch.autograd.Function):
    """The central critic's value as a function of every agent's OWN action only (models/maddpg.py:52-58: the other agents' actions
    enter detached): forward = _CriticHead on base[b] + id_column[i] (the own-action term (a - a.detach()) W_act[:, i] is zero in
    value), backward = d loss / d act[b, i] = dx[b, i, :] . W_act[:, i] straight from the kernel (mapdn_critic_head_backward_dot);
    no [b, n, 64] tensor exists in either direction and the critic's parameters receive no gradient — the policy optimiser does not
    own them (utilities/trainer.py:26-27, 73-98)."""

    @staticmethod
    def forward(ctx, act, base, per_n, dot_w, ln_w, ln_b, eps, w2, b2, w3, b3):
        x2, pn, dw = base.detach().contiguous(), per_n.detach().contiguous(), dot_w.detach().contiguous()
        prm = head_pack(ln_w, ln_b, w2, b2, w3, b3)
        ctx.save_for_backward(x2, pn, dw, *prm)
        ctx.act_shape = act.shape
        return _head_forward(ctx, x2, pn, prm, eps)

    @staticmethod
    def backward(ctx, dv):
        x2, pn, dw, *prm = ctx.saved_tensors
        rows, n, dev = ctx.rows, ctx.n, x2.device
        dv2 = dv.reshape(rows).contiguous()
        dact = torch.empty(rows, dtype=torch.float32, device=dev)
        launch("mapdn_critic_head_backward_dot", dev, dv2, x2, pn, n, *head_abi(prm, ctx.eps), dw, dact, rows)
        return (dact.view(ctx.act_shape),) + (None,) * 10


class _CriticHeadMSE(torch.autograd.Function):
    """The value loss of the DDPG family (learning_algorithms/ddpg.py:36-38 == models/maddpg.py:122-124),
        loss = sum_rows w[row] (returns[row] - v[row])^2,    w[row] = scale * wrow[row / n]   (wrow None: 1),
    with v the critic head of _CriticHead — as ONE launch that produces the loss AND every gradient of it (mapdn_critic_head_mse):
    d loss / d v = -2 w (returns - v) is known per row the moment v is, so the separate forward launch (a fifth 64 x 64 product over
    all rows) disappears.  backward only scales the stored gradients by the incoming one (1 for `loss.backward()`)."""

    @staticmethod
    def forward(ctx, x, per_n, ln_w, ln_b, eps, w2, b2, w3, b3, returns, wrow, scale):
        x2 = x.detach().contiguous()
        pn = per_n.detach().contiguous() if per_n is not None else None
        n = pn.shape[0] if pn is not None else 1
        rows, formed, dev = x2.shape[0] * n, pn is not None, x2.device
        prm = head_pack(ln_w, ln_b, w2, b2, w3, b3)
        ret = returns.detach().reshape(rows).contiguous().float()
        wr = wrow.detach().contiguous().float() if wrow is not None else None
        sc = scale.detach().reshape(1).contiguous().float()
        dx = torch.empty_like(x2)
        grads = torch.empty(HEAD_GRADS + (n * 64 if formed else 0), dtype=torch.float32, device=dev)
        scratch = buffer("mapdn_critic_head_scratch_floats", dev, rows, n, int(formed), at_least=1)
        launch("mapdn_critic_head_mse", dev, ret, wr, sc, x2, pn, n, *head_abi(prm, eps), dx, grads, scratch, rows)
        ctx.save_for_backward(dx, grads)
        ctx.n, ctx.formed = n, formed
        return grads[HEAD_LOSS].clone()

    @staticmethod
    def backward(ctx, g):
        dx, grads = ctx.saved_tensors
        n, need = ctx.n, ctx.needs_input_grad
        gs = grads * g
        return (dx * g if need[0] else None, head_dper_n(gs, n) if ctx.formed and need[1] else None) + head_param_grads(gs) + (None, None, None)


class _CriticTwinMSE(torch.autograd.Function):
    """MATD3's value loss (models/matd3.py:143-150) on the twin of the central critic,
        loss = sum_rows w[row] 1/2 [(returns - v1)^2 + (returns - v2)^2],   w[row] = scale * wrow[row / n]   (wrow None: 1),
    v1 / v2 = the critic head on base[b] + per_n[i] / on the same + flag_col — ONE launch for the loss and every gradient of it
    (mapdn_critic_twin_mse, csrc/critic_twin.hip): dbase, dper_n and the head's parameter gradients arrive summed over both heads,
    d flag_col is the second head's dx summed over all rows.  NOT the default route: at config 5's 10 M rows it takes 6.6 ms where two
    mapdn_critic_head_mse launches take 5.9; DDPGNet.value_mse takes it under MAPDN_TWIN_MSE_KERNEL=1."""
    launches = 0           # how often the kernel was reached (tests count through the wrapper)

    @staticmethod
    def forward(ctx, base, per_n, flag, ln_w, ln_b, eps, w2, b2, w3, b3, returns, wrow, scale):
        x2, pn, fl = base.detach().contiguous(), per_n.detach().contiguous(), flag.detach().contiguous()
        n = pn.shape[0]
        rows, dev = x2.shape[0] * n, x2.device
        prm = head_pack(ln_w, ln_b, w2, b2, w3, b3)
        ret = returns.detach().reshape(rows).contiguous().float()
        wr = wrow.detach().contiguous().float() if wrow is not None else None
        sc = scale.detach().reshape(1).contiguous().float()
        dbase = torch.empty_like(x2)
        grads = torch.empty(TWIN_GRADS + n * 64, dtype=torch.float32, device=dev)
        scratch = buffer("mapdn_critic_twin_scratch_floats", dev, rows, n, at_least=1)
        launch("mapdn_critic_twin_mse", dev, ret, wr, sc, x2, pn, n, fl, *head_abi(prm, eps), dbase, grads, scratch, rows)
        _CriticTwinMSE.launches += 1
        ctx.save_for_backward(dbase, grads)
        ctx.n = n
        return grads[HEAD_LOSS].clone()

    @staticmethod
    def backward(ctx, g):
        dbase, grads = ctx.saved_tensors
        n, need = ctx.n, ctx.needs_input_grad
        gs = grads * g
        dpn, dflag = twin_tails(gs, n)
        return (dbase * g if need[0] else None, dpn if need[1] else None, dflag if need[2] else None) + head_param_grads(gs) + (None, None, None)


def critic_twin_forward(cr: "MLPCritic", base: torch.Tensor, per_n: torch.Tensor, flag: torch.Tensor, want=("v1", "v2")):
    """the twin head without autograd (target values, evaluation): {name: [b * n, 1]} for the names in `want` out of v1, v2, vmin —
    one mapdn_critic_twin_forward launch"""
    x2, pn, fl = base.detach().contiguous(), per_n.detach().contiguous(), flag.detach().contiguous()
    n = pn.shape[0]
    rows, dev = x2.shape[0] * n, x2.device
    out = {k: torch.empty(rows, 1, dtype=torch.float32, device=dev) for k in want}
    launch("mapdn_critic_twin_forward", dev, x2, pn, n, fl, *_head_abi_of(cr), out.get("v1"), out.get("v2"), out.get("vmin"), rows)
    critic_twin_forward.launches += 1
    return out


critic_twin_forward.launches = 0


class twin_pair_mse:
    """how often MATD3's value loss took the pair of single-head loss launches (tests count the routes)"""
    launches = 0


HEAD_MAX_FORMED_N = 88      # formed rows keep one [n][64] LDS accumulator per wavefront: n <= 88 fits the 160 KB of a CU with four of them


def critic_head_ok(cr: "MLPCritic", x: torch.Tensor, rows: int, formed_n: int = 0) -> bool:
    """the one-launch critic head covers the reference's default critic (LayerNorm, ReLU, hidden size 64, one output) in fp32 on the GPU
    (formed_n: the number of agents when the rows are formed as base[b] + per_n[i])"""
    return (formed_n <= HEAD_MAX_FORMED_N and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[-1] == 64 and rows >= 1024 and rows < 2 ** 31
            and default_critic_fp32(cr) and os.environ.get("MAPDN_FUSED_HEAD", "1") != "0")


def critic_twin_ok(cr: "MLPCritic", base: torch.Tensor, rows: int, n: int) -> bool:
    """the one-launch twin head (csrc/critic_twin.hip) covers what critic_head_ok covers for formed rows — the default critic in fp32 on
    the GPU, enough rows, n <= 88 —; MAPDN_FUSED_TWIN=0 switches it off (the PyTorch route and the single-head kernels remain).  It gates
    the forward launch (target min, value()) and both fused forms of the value loss; of those the default is two mapdn_critic_head_mse
    launches, MAPDN_TWIN_MSE_KERNEL=1 takes mapdn_critic_twin_mse (one launch, 12 % slower at 10 M rows: DESIGN section 11)"""
    return critic_head_ok(cr, base, rows, n) and n >= 1 and os.environ.get("MAPDN_FUSED_TWIN", "1") != "0"


def critic_cf_ok(cr: "MLPCritic", x: torch.Tensor, rows: int, act_dim: int) -> bool:
    """the one-launch counterfactual baseline (csrc/critic_cf.hip) covers what critic_head_ok covers for rows that are read — the default
    critic in fp32 on the GPU, enough rows — with one action per agent; MAPDN_FUSED_CF=0 switches it off (the PyTorch loop over the samples
    remains)"""
    return act_dim == 1 and critic_head_ok(cr, x, rows) and os.environ.get("MAPDN_FUSED_CF", "1") != "0"


def critic_counterfactual(cr: "MLPCritic", x: torch.Tensor, act_col: torch.Tensor, delta: torch.Tensor, want_v0: bool = True):
    """(baseline [rows], v0 [rows] or None) without autograd: baseline = mean over s of the head on x + delta[s] * act_col[row % n], v0 = the
    head on x — one mapdn_critic_head_counterfactual launch.  x [rows, 64], act_col [n, 64], delta [S, rows]."""
    x2, col, dl = x.detach().contiguous(), act_col.detach().contiguous(), delta.detach().contiguous()
    rows, dev = x2.shape[0], x2.device
    if dl.dim() != 2 or dl.shape[1] != rows or col.dim() != 2 or col.shape[1] != 64 or dl.dtype != torch.float32 or col.dtype != torch.float32:
        raise ValueError("critic_counterfactual: x [rows, 64], act_col [n, 64], delta [S, rows], float32")
    baseline = torch.empty(rows, dtype=torch.float32, device=dev)
    v0 = torch.empty(rows, dtype=torch.float32, device=dev) if want_v0 else None
    launch("mapdn_critic_head_counterfactual", dev, x2, col.shape[0], col, dl, dl.shape[0], *_head_abi_of(cr), baseline, v0, rows)
    critic_counterfactual.launches += 1
    return baseline, v0


critic_counterfactual.launches = 0           # how often the kernel was reached (tests count the routes)


def critic_head(cr: "MLPCritic", x: torch.Tensor, per_n: Optional[torch.Tensor] = None) -> torch.Tensor:
    return _CriticHead.apply(x, per_n, *head_params(cr))
