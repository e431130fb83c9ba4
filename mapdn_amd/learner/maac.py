"""MAAC (models/maac.py, critics/maac_critic.py, agents/rnn_agent_gaussian.py): Gaussian recurrent agents and ONE attention critic whose
attention over the other agents is one HIP launch each way (csrc/critic_attn.hip); reached through make_alg_args(..., alg="maac")."""

import math
import os
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._hip import buffer, launch
from .args import Batch, _maac_args_ok
from .ddpg import DDPGNet
from .modules import GaussianRNNAgent


def attention_loop_reference(sel: torch.Tensor, key: torch.Tensor, val: torch.Tensor, H: int):
    """critics/maac_critic.py:120-136 restated literally: per head and per agent, the keys / values of the OTHER agents stacked and
    permuted to [b, d, n - 1], softmax over the last dimension.  (out [b, n, hid], logit_sq [n, H] = the sum of the squared unscaled
    logits.)  What the batched route and the kernels are tested against; never on a training path."""
    b, n, hid = sel.shape
    d = hid // H
    outs, lsq = [[] for _ in range(n)], sel.new_zeros(n, H)
    for h in range(H):
        cols = slice(h * d, (h + 1) * d)
        for i in range(n):
            keys = [key[:, j, cols] for j in range(n) if j != i]
            values = [val[:, j, cols] for j in range(n) if j != i]
            logits = torch.matmul(sel[:, i, cols].reshape(b, 1, -1), torch.stack(keys).permute(1, 2, 0))          # [b, 1, n - 1]
            weights = F.softmax(logits / math.sqrt(d), dim=2)
            outs[i].append((torch.stack(values).permute(1, 2, 0) * weights).sum(dim=2))
            lsq[i, h] = (logits ** 2).sum()
    return torch.stack([torch.cat(o, 1) for o in outs], 1), lsq


def attention_core_torch(sel: torch.Tensor, key: torch.Tensor, val: torch.Tensor, H: int):
    """the same as ONE masked softmax over [b, H, n, n] (the diagonal — an agent's own key — masked out): two batched products, no loop
    over heads or agents.  The CPU route, and the GPU route where the kernels do not apply."""
    b, n, hid = sel.shape
    d = hid // H
    q, k, v = (t.reshape(b, n, H, d).transpose(1, 2) for t in (sel, key, val))                 # [b, H, n, d]
    logits = q @ k.transpose(-1, -2)                                                           # [b, H, n, n]
    own = torch.eye(n, dtype=torch.bool, device=sel.device)
    p = F.softmax((logits / math.sqrt(d)).masked_fill(own, float("-inf")), dim=-1)
    out = (p @ v).transpose(1, 2).reshape(b, n, hid)
    return out, logits.masked_fill(own, 0.0).square().sum(dim=(0, 3)).t()                      # [n, H]


class _AttentionCore(torch.autograd.Function):
    """(out, logit_sq) of attention_core_torch as one HIP launch forward and one backward (libmapdn_hip.so: mapdn_attention_*,
    csrc/critic_attn.hip): a workgroup holds one sample's three [n, 64] operands and its [H, n, n] scores in LDS; the backward recomputes
    the probabilities, so only the operands are saved."""
    launches = 0           # how often the forward kernel was reached (tests count the routes)

    @staticmethod
    def forward(ctx, sel, key, val, H):
        s, k, v = sel.contiguous(), key.contiguous(), val.contiguous()
        B, n, dev = s.shape[0], s.shape[1], s.device
        out = torch.empty_like(s)
        lsq = torch.empty(n, H, dtype=torch.float32, device=dev)
        scratch = buffer("mapdn_attention_scratch_floats", dev, B, n, H, at_least=1)
        launch("mapdn_attention_forward", dev, s, k, v, B, n, H, out, lsq, scratch)
        _AttentionCore.launches += 1
        ctx.save_for_backward(s, k, v)
        ctx.H = H
        return out, lsq

    @staticmethod
    def backward(ctx, dout, dlsq):
        s, k, v = ctx.saved_tensors
        B, n, dev = s.shape[0], s.shape[1], s.device
        do, dl = dout.contiguous(), dlsq.contiguous()
        ds, dk, dv = torch.empty_like(s), torch.empty_like(s), torch.empty_like(s)
        launch("mapdn_attention_backward", dev, do, dl, s, k, v, B, n, ctx.H, ds, dk, dv)
        return ds, dk, dv, None


ATTN_MAX_N = 48            # csrc/critic_attn.hip AT_MAX_N (mapdn_attention_max_agents()): one sample's operands and scores must fit a CU's LDS


def attention_ok(sel: torch.Tensor, H: int) -> bool:
    """the attention kernels cover fp32 on the GPU, hidden size 64, 2 <= n <= ATTN_MAX_N agents, 1 / 2 / 4 heads; MAPDN_FUSED_ATTN=0
    switches them off (the batched PyTorch route remains)"""
    return (sel.is_cuda and sel.dtype == torch.float32 and sel.dim() == 3 and sel.shape[-1] == 64 and 2 <= sel.shape[1] <= ATTN_MAX_N
            and H in (1, 2, 4) and sel.shape[0] >= 1 and sel.shape[0] * sel.shape[1] * 64 < 2 ** 31 and os.environ.get("MAPDN_FUSED_ATTN", "1") != "0")


def attention_core(sel: torch.Tensor, key: torch.Tensor, val: torch.Tensor, H: int):
    if attention_ok(sel, H) and key.dtype == torch.float32 and val.dtype == torch.float32:
        return _AttentionCore.apply(sel, key, val, H)
    return attention_core_torch(sel, key, val, H)


def _named_sequential(**mods) -> nn.Sequential:
    seq = nn.Sequential()
    for k, m in mods.items():
        if m is not None:
            seq.add_module(k, m)
    return seq


class AttentionCritic(nn.Module):
    """critics/maac_critic.py:8-161 for continuous actions, with the reference's module tree (critic_encoders.{i}.enc_fc1,
    critics.{i}.critic_fc1 / critic_fc2, biases.{i}.bias_fc1 / bias_fc2, state_encoders.{i}.s_enc_fc1, key_extractors.{h},
    selector_extractors.{h}, value_extractors.{h}.0; enc_bn / s_enc_bn under norm_in), so that its state_dict is the reference's.
    forward: [b, n, o], [b, n, a] -> (q - bias [b, n], regulariser [n]).  The per-agent encoders, critics and biases run batched over
    their stacked parameters; the attention over the other agents is attention_core (HIP kernels, or one masked softmax)."""

    def __init__(self, args):
        super().__init__()
        self.hidden_dim, self.attend_heads, self.nagents = args.hid_size, int(args.attend_heads), args.agent_num
        assert self.hidden_dim % self.attend_heads == 0
        sdim, adim, hid = args.obs_size, args.action_dim, args.hid_size
        bn = (lambda k: nn.BatchNorm1d(k, affine=False)) if args.norm_in else (lambda k: None)
        self.norm_in = bool(args.norm_in)
        self.critic_encoders, self.critics, self.biases, self.state_encoders = nn.ModuleList(), nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        for _ in range(self.nagents):
            self.critic_encoders.append(_named_sequential(enc_bn=bn(sdim + adim), enc_fc1=nn.Linear(sdim + adim, hid), enc_nl=nn.LeakyReLU()))
            self.critics.append(_named_sequential(critic_fc1=nn.Linear(2 * hid, hid), critic_nl=nn.LeakyReLU(), critic_fc2=nn.Linear(hid, 1)))
            self.biases.append(_named_sequential(bias_fc1=nn.Linear(hid, hid), bias_nl=nn.LeakyReLU(), bias_fc2=nn.Linear(hid, 1)))
            self.state_encoders.append(_named_sequential(s_enc_bn=bn(sdim), s_enc_fc1=nn.Linear(sdim, hid), s_enc_nl=nn.LeakyReLU()))
        d = hid // self.attend_heads
        self.key_extractors, self.selector_extractors, self.value_extractors = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        for _ in range(self.attend_heads):
            self.key_extractors.append(nn.Linear(hid, d, bias=False))
            self.selector_extractors.append(nn.Linear(hid, d, bias=False))
            self.value_extractors.append(nn.Sequential(nn.Linear(hid, d), nn.LeakyReLU()))

    @staticmethod
    def _per_agent(x: torch.Tensor, layers) -> torch.Tensor:
        """layers[i](x[:, i]) for every agent i as one batched product over the stacked weights: [b, n, in] -> [b, n, out]"""
        w = torch.stack([m.weight for m in layers])                                        # [n, out, in]
        return torch.einsum("bni,noi->bno", x, w) + torch.stack([m.bias for m in layers])

    def forward(self, obs: torch.Tensor, act: torch.Tensor):
        b, n, H = obs.shape[0], self.nagents, self.attend_heads
        sa = torch.cat((obs, act), dim=-1)
        s_in = obs
        if self.norm_in:                                                                    # plain per-agent BatchNorm1d(affine=False) modules
            sa = torch.stack([enc.enc_bn(sa[:, i]) for i, enc in enumerate(self.critic_encoders)], 1)
            s_in = torch.stack([enc.s_enc_bn(obs[:, i]) for i, enc in enumerate(self.state_encoders)], 1)
        sa_enc = F.leaky_relu(self._per_agent(sa, [e.enc_fc1 for e in self.critic_encoders]))          # [b, n, hid]
        s_enc = F.leaky_relu(self._per_agent(s_in, [e.s_enc_fc1 for e in self.state_encoders]))
        # head h's extractor fills columns h d .. (h + 1) d: the H extractors of a kind are one [hid, hid] product
        key = F.linear(sa_enc, torch.cat([m.weight for m in self.key_extractors], 0))
        val = F.leaky_relu(F.linear(sa_enc, torch.cat([m[0].weight for m in self.value_extractors], 0),
                                    torch.cat([m[0].bias for m in self.value_extractors], 0)))
        sel = F.linear(s_enc, torch.cat([m.weight for m in self.selector_extractors], 0))
        other, logit_sq = attention_core(sel, key, val, H)                                  # [b, n, hid], [n, H]
        x = F.leaky_relu(self._per_agent(torch.cat((sa_enc, other), -1), [c.critic_fc1 for c in self.critics]))
        q = self._per_agent(x, [c.critic_fc2 for c in self.critics]).squeeze(-1)            # [b, n]
        y = F.leaky_relu(self._per_agent(s_enc, [c.bias_fc1 for c in self.biases]))
        bias = self._per_agent(y, [c.bias_fc2 for c in self.biases]).squeeze(-1)
        reg = 1e-3 * logit_sq.sum(1) / float(b * (n - 1))                                   # 1e-3 sum over heads of mean(logit^2): maac_critic.py:156-157
        return q - bias, reg


class MAACNet(DDPGNet):
    """`MAAC(Model)` (models/maac.py:10-121): Gaussian recurrent agents, ONE attention critic for all agents, the soft actor-critic loss.
    Target handling, reward BatchNorm, initialisation and the Gaussian branch of select_action are DDPGNet's.  Off-policy: the replay ring
    is kept between update rounds (models/model.py:53-56 clears it for COMA, IAC, IPPO and MAPPO only)."""
    ALGS = ("maac",)

    def __init__(self, args, alg: str = "maac", target_net: Optional["MAACNet"] = None):
        ids = self._begin(args, alg, _maac_args_ok)
        self.batchnorm = nn.BatchNorm1d(self.n_)                   # rewards AND advantages (maac.py:18, 112-113; model.py:317-318)
        self.__dict__["_adv_batchnorm"] = self.batchnorm
        self.value_dicts = nn.ModuleList([AttentionCritic(args)])                                          # maac.py:40-41
        self.policy_dicts = nn.ModuleList([GaussianRNNAgent(self.obs_dim + ids, args) for _ in range(1 if args.shared_params else self.n_)])
        self._finish(target_net)

    def policy(self, obs: torch.Tensor, last_hid: torch.Tensor, means_grad_only: bool = False):
        """models/model.py:101-139 with gaussian_policy: obs [b, n, o], last_hid [b, n, h] -> means, log_stds [b, n, a], hiddens [b, n, h]"""
        b, n, o = obs.shape[0], self.n_, self.obs_dim
        if self.args.shared_params:
            ag = self.policy_dicts[0]
            m, ls, h = ag.trunk(self._shared_agent_first_layer(ag, obs).reshape(b * n, -1), last_hid)
            return m.view(b, n, -1), ls.view(b, n, -1), h.view(b, n, -1)
        ms, lss, hs = [], [], []
        for i, ag in enumerate(self.policy_dicts):
            w = ag.fc1.weight
            x = F.linear(obs[:, i], w[:, :o], ag.fc1.bias)
            if self.args.agent_id:
                x = x + w[:, o + i]
            m, ls, h = ag.trunk(x, last_hid[:, i])
            ms.append(m); lss.append(ls); hs.append(h)
        return torch.stack(ms, 1), torch.stack(lss, 1), torch.stack(hs, 1)

    def value(self, obs: torch.Tensor, act: torch.Tensor, own_action_only: bool = False) -> torch.Tensor:
        """maac.py:47-66: [b + 1, n] — rows 0 .. b - 1 the values, row b the per-agent attention regulariser"""
        q, reg = self.value_dicts[0](obs, act)
        return torch.cat((q, reg.unsqueeze(0)), 0)

    def get_actions(self, state, status, exploration, actions_avail, target=False, last_hid=None, means_grad_only=False, clip=False, noise=None):
        """maac.py:68-92: DDPGNet.get_actions with the log-probability masked and summed over the action dimension: [b, n]"""
        actions, restore, log_prob, out, hid = super().get_actions(state, status, exploration, actions_avail, target, last_hid, means_grad_only, clip, noise)
        if log_prob is not None:
            log_prob = ((1.0 - (actions_avail == 0).to(log_prob.dtype)) * log_prob).sum(dim=-1)
        return actions, restore, log_prob, out, hid

    def get_loss(self, batch: Batch, want=("policy", "value")):
        """maac.py:94-121.  Two draws per call, in the reference's order: the actions at `state` from the behaviour policy, then the next
        actions at `next_state` from the target policy; batch["noise"] / batch["next_noise"] [bs, n, 1] replace them.  A loss not in
        `want` is None; of its forward passes only those are kept that change state the reference's call changes (the draws, and the
        running statistics of `batchnorm` / the norm_in BatchNorms, which see every value() call while training)."""
        n, a = self.n_, self.args
        state, actions, next_state, avail, last_hid, hid, rewards, done, valid, wmean = self._unpack(batch)
        bs = state.shape[0]
        want_p, want_v = "policy" in want, "value" in want
        stats = self.training and (a.norm_in or a.normalize_advantages)      # value() calls that move running statistics cannot be skipped
        _, actions_pol, log_prob, action_out, _ = self.get_actions(state, "train", True, avail, False, last_hid, noise=batch.get("noise"))
        if want_v or (stats and a.norm_in):
            with torch.no_grad():
                _, next_actions, _, _, _ = self.get_actions(next_state, "train", True, avail, True, hid, noise=batch.get("next_noise"))
        elif batch.get("next_noise") is None:
            torch.randn_like(actions_pol)                                    # the call's second draw, so that the generator goes the reference's way
        policy_loss = value_loss = None
        values_pol = None
        if want_p or stats:
            with torch.set_grad_enabled(want_p and torch.is_grad_enabled()):
                values_pol = self.value(state, actions_pol)[:bs]             # (every agent's action carries gradient: maac.py:99 detaches nothing)
        if want_v or want_p:
            with torch.set_grad_enabled(want_v and torch.is_grad_enabled()):
                compose = self.value(state, actions.detach())
            values, attn_reg = compose[:bs], compose[bs]
        if want_v or (stats and a.norm_in):
            with torch.no_grad():
                net = self.target_net if a.target else self
                next_values = net.value(next_state, next_actions)[:bs].view(-1, n)
        if values_pol is not None:
            advantages = values_pol
            if a.normalize_advantages:
                advantages = self._adv_batchnorm.to(advantages.device)(advantages)
        if want_p:
            if a.soft:
                pl = log_prob / a.reward_scale - advantages
            else:
                pl = -advantages.detach() * log_prob
            policy_loss = wmean(pl + attn_reg)                               # the regulariser goes to the POLICY loss only (maac.py:118)
        if want_v:
            returns = rewards + a.gamma * (1 - done) * next_values - a.soft * log_prob / a.reward_scale       # log_prob NOT detached (maac.py:109)
            value_loss = wmean((returns - values).pow(2))
        return policy_loss, value_loss, (action_out if want_p else None)
