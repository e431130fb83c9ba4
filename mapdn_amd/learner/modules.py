"""The reference's network modules with its parameter names (agents/rnn_agent.py, agents/rnn_agent_gaussian.py, critics/mlp_critic.py), so
that a reference `model.pt` loads with strict=True and vice versa; their trunks take the HIP routes of ops.py / head.py where those
apply.  _PolicyTrunk is the shared recurrent agent for the policy update as two HIP launches (csrc/policy.hip, csrc/policy_bwd.hip)."""

import torch
import torch.nn as nn

from ._hip import buffer, launch
from .args import _activation
from .head import critic_head, critic_head_ok
from .ops import _ReluDot64, _splitk_dw, gru_cell_tall, layernorm_act, relu_dot64_ok, tall_linear


class RNNAgent(nn.Module):
    """fc1 -> LayerNorm -> act -> GRUCell -> fc2 (agents/rnn_agent.py:5-32)."""

    def __init__(self, input_shape: int, args):
        super().__init__()
        self.hid_size = args.hid_size
        self.fc1 = nn.Linear(input_shape, args.hid_size)
        if args.layernorm:
            self.layernorm = nn.LayerNorm(args.hid_size)
        self.rnn = nn.GRUCell(args.hid_size, args.hid_size)
        self.fc2 = nn.Linear(args.hid_size, args.action_dim)
        self.use_ln = bool(args.layernorm)
        self.act = _activation(args.hid_activation)

    def trunk(self, x: torch.Tensor, hidden: torch.Tensor):
        """x: pre-activation of fc1, [rows, hid]"""
        x = layernorm_act(self.layernorm, self.act, x) if self.use_ln else self.act(x)
        h = gru_cell_tall(self.rnn, x, hidden.reshape(-1, self.hid_size))
        return tall_linear(self.fc2, h), h

    def forward(self, inputs, hidden):
        a, h = self.trunk(self.fc1(inputs), hidden)
        return a, None, h


class MLPCritic(nn.Module):
    """fc1 -> LayerNorm -> act -> fc2 -> act -> fc3 (critics/mlp_critic.py:7-36)."""

    def __init__(self, input_shape: int, output_shape: int, args):
        super().__init__()
        self.fc1 = nn.Linear(input_shape, args.hid_size)
        if args.layernorm:
            self.layernorm = nn.LayerNorm(args.hid_size)
        self.fc2 = nn.Linear(args.hid_size, args.hid_size)
        self.fc3 = nn.Linear(args.hid_size, output_shape)
        self.use_ln = bool(args.layernorm)
        self.act = _activation(args.hid_activation)

    def trunk(self, x: torch.Tensor):
        if critic_head_ok(self, x, x.shape[0]):
            return critic_head(self, x), None                      # (no caller uses the hidden activation)
        x = layernorm_act(self.layernorm, self.act, x) if self.use_ln else self.act(x)
        return self.head(x)

    def head(self, x: torch.Tensor):
        """what follows the first layer's LayerNorm + activation: fc2 -> act -> fc3"""
        pre = tall_linear(self.fc2, x)
        if relu_dot64_ok(self.act, self.fc3, pre):
            return _ReluDot64.apply(pre, self.fc3.weight, self.fc3.bias), None      # (no caller uses the hidden activation)
        h = self.act(pre)
        return tall_linear(self.fc3, h), h

    def forward(self, inputs, hidden=None):
        return self.trunk(self.fc1(inputs))


class GaussianRNNAgent(nn.Module):
    """fc1 -> LayerNorm -> act -> GRUCell -> (mean, log_std) with log_std squashed by tanh into [LOG_STD_MIN, LOG_STD_MAX]
    (agents/rnn_agent_gaussian.py:6-41).  PyTorch modules (the fused LayerNorm of RNNAgent where it applies): the one-launch policy
    kernels have a single output head and are not extended to two."""

    def __init__(self, input_shape: int, args):
        super().__init__()
        self.hid_size = args.hid_size
        self.fc1 = nn.Linear(input_shape, args.hid_size)
        if args.layernorm:
            self.layernorm = nn.LayerNorm(args.hid_size)
        self.rnn = nn.GRUCell(args.hid_size, args.hid_size)
        self.mean = nn.Linear(args.hid_size, args.action_dim)
        self.log_std = nn.Linear(args.hid_size, args.action_dim)
        self.use_ln = bool(args.layernorm)
        self.act = _activation(args.hid_activation)
        self.lo, self.hi = float(args.LOG_STD_MIN), float(args.LOG_STD_MAX)

    def trunk(self, x: torch.Tensor, hidden: torch.Tensor):
        """x: pre-activation of fc1, [rows, hid]"""
        x = layernorm_act(self.layernorm, self.act, x) if self.use_ln else self.act(x)
        h = gru_cell_tall(self.rnn, x, hidden.reshape(-1, self.hid_size))
        log_std = self.lo + 0.5 * (self.hi - self.lo) * (torch.tanh(tall_linear(self.log_std, h)) + 1)
        return tall_linear(self.mean, h), log_std, h

    def forward(self, inputs, hidden):
        return self.trunk(self.fc1(inputs), hidden)


class _PolicyTrunk(torch.autograd.Function):
    """means = fc2(GRUCell(relu(LayerNorm(fc1(obs) + id column)), last_hid)) of the shared recurrent agent (agents/rnn_agent.py:5-32) for the
    policy UPDATE (models/maddpg.py:103-125: only the means carry gradient — the loss does not read the new hidden state), forward and
    backward as HIP launches: mapdn_policy_forward_train (the rollout's one-launch forward; keeps x1 = the LayerNorm input) and
    mapdn_policy_backward (csrc/policy_bwd.hip: recomputes the trunk, writes d gate pre-activations / xn / dx1 and the small gradients).
    What is left for the BLAS back end are the three K = rows weight-gradient products, run block-wise (_splitk_dw).  The PyTorch route
    moved ~100 GB per update through the projections, ATen's fused cell and its workspace."""

    @staticmethod
    def forward(ctx, obs2, hid2, n_agents, ids, eps, w1, b1, lnw, lnb, w_ih, w_hh, b_ih, b_hh, w2, b2):
        obs2, hid2 = obs2.contiguous(), hid2.contiguous()
        rows, o = obs2.shape
        prm = tuple(t.detach().contiguous() for t in (w1, b1, lnw, lnb, w_ih, w_hh, b_ih, b_hh, w2, b2))
        means = torch.empty(rows, dtype=torch.float32, device=obs2.device)
        x1 = torch.empty(rows, 64, dtype=torch.float32, device=obs2.device)
        launch("mapdn_policy_forward_train", obs2.device, obs2, hid2, *prm, means, None, x1, rows, int(n_agents), o, int(ids), float(eps))
        ctx.save_for_backward(obs2, hid2, x1, *prm)
        ctx.n_agents, ctx.ids, ctx.eps = int(n_agents), int(ids), float(eps)
        return means

    @staticmethod
    def backward(ctx, dmeans):
        obs2, hid2, x1, w1, b1, lnw, lnb, w_ih, w_hh, b_ih, b_hh, w2, b2 = ctx.saved_tensors
        rows, o = obs2.shape
        n, dev = ctx.n_agents, obs2.device
        dm = dmeans.reshape(rows).contiguous()
        dx1 = torch.empty_like(x1)
        xn = torch.empty_like(x1)
        dg = torch.empty(rows, 256, dtype=torch.float32, device=dev)
        small = torch.empty(512, dtype=torch.float32, device=dev)
        scratch = buffer("mapdn_policy_backward_scratch_floats", dev, rows, at_least=1)
        launch("mapdn_policy_backward", dev, dm, x1, hid2, lnw, lnb, ctx.eps, w_ih, w_hh, b_ih, b_hh, w2, dx1, dg, xn, small, scratch, rows)
        dw_ih = _splitk_dw(dg[:, :192], xn)
        dw_hh = torch.cat((_splitk_dw(dg[:, :128], hid2), _splitk_dw(dg[:, 192:], hid2)), 0)
        db_ih = small[:192].clone()
        db_hh = torch.cat((small[:128], small[192:256]))
        dw1 = torch.empty_like(w1)
        dw1[:, :o] = _splitk_dw(dx1, obs2)
        per_agent = dx1.view(-1, n, 64).sum(0)                   # [n, 64]: sum over the batch for every agent
        if ctx.ids:
            dw1[:, o:] = per_agent.t()
        db1 = per_agent.sum(0)
        return (None, None, None, None, None, dw1, db1, small[256:320], small[320:384], dw_ih, dw_hh, db_ih, db_hh, small[384:448].view(1, 64),
                small[448:449])
