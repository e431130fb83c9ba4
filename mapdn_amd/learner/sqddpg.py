"""SQDDPG (models/sqddpg.py): the deterministic agents with a critic valued on sampled coalition orders, whose b x sample_size x n rows are
formed inside the kernels of csrc/critic_shap.hip from a prefix sum over positions; reached through make_alg_args(..., alg="sqddpg")."""

import ctypes
import functools
import os
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._hip import buffer, entry, launch
from .args import Batch, _sqddpg_args_ok
from .ddpg import DDPGNet
from .head import HEAD_GRADS, default_critic_fp32, head_abi, head_pack, head_param_grads, head_params, shapley_tails
from .modules import MLPCritic, RNNAgent
from .ops import tall_linear_w


def sample_coalition_positions(rows: int, n: int, device, generator=None) -> torch.Tensor:
    """sqddpg.py:38-40: ONE th.multinomial of shape [rows, n] on float64 uniform weights, without replacement -> pos [rows, n] int64,
    pos[r, i] = the position of agent i in row r's random order"""
    w = torch.full((rows, n), 1.0 / n, dtype=torch.float64, device=device)
    return torch.multinomial(w, n, replacement=False, generator=generator)


def shapley_first_layer(base: torch.Tensor, id_cols: Optional[torch.Tensor], act_cols: torch.Tensor, act: torch.Tensor, pos: torch.Tensor,
                        who: Optional[int] = None) -> torch.Tensor:
    """The first layer of the coalition critic's rows (sqddpg.py:65-93) in factored form.  base [b, h] = W_obs obs_all + b1, id_cols [n, h]
    or None, act_cols [n, h] (W_act transposed: row p is the column of action SLOT p), act [b, n], pos [b, S, n] integer.  With
    gc = argsort(pos) the agent at each position, slot p holds the action of agent gc[p]; row (b, s, i) keeps the slots up to its own
    position pos_i and zeroes the rest:
        x[b, s, i] = base[b] + id_cols[i] + P[b, s, pos_i],   P[b, s, p] = sum_{q <= p} act[b, gc[q]] act_cols[q]   (one cumsum + one gather)
    Only the own slot carries a gradient back to the action (sqddpg.py:77): P is built from the detached actions and a zero-valued
    (act_i - act_i.detach()) act_cols[pos_i] restores that path.  who: agent i's rows only ([b, S, h]; id_cols is then that agent's [h])."""
    b, S, n = pos.shape
    h = base.shape[-1]
    pos = pos.long()
    gc = pos.argsort(dim=-1)
    a_slot = act.detach().unsqueeze(1).expand(b, S, n).gather(2, gc)                  # [b, S, n]: the action in slot p
    P = (a_slot.unsqueeze(-1) * act_cols).cumsum(dim=2)                               # [b, S, n, h]
    if who is None:
        x = P.gather(2, pos.unsqueeze(-1).expand(b, S, n, h)) + base.view(b, 1, 1, h)
        if id_cols is not None:
            x = x + id_cols
        if act.requires_grad:
            x = x + (act - act.detach()).view(b, 1, n, 1) * act_cols[pos]
        return x
    pw = pos[:, :, who]
    x = P.gather(2, pw.view(b, S, 1, 1).expand(b, S, 1, h)).squeeze(2) + base.view(b, 1, h)
    if id_cols is not None:
        x = x + id_cols
    if act.requires_grad:
        x = x + (act[:, who] - act[:, who].detach()).view(b, 1, 1) * act_cols[pw]
    return x


class _ShapleyCritic(torch.autograd.Function):
    """v[b, s, i] of the coalition critic behind its first layer as HIP launches (libmapdn_hip.so: mapdn_critic_shapley_*, csrc/critic_shap.hip):
    the rows x[b, s, i] = base[b] + id_cols[i] + P[b, s, pos_i] are formed in the kernel from the prefix sum over positions, so that neither
    the reference's [b S n, (o + 1) n + n] input nor a [b S n, 64] activation exists.  The backward recomputes the forward; when only the
    action needs a gradient (the policy update) it returns d act alone and skips every parameter partial."""
    launches = 0

    @staticmethod
    def forward(ctx, act, base, id_cols, act_cols, pos32, ln_w, ln_b, eps, w2, b2, w3, b3):
        b, S, n = pos32.shape
        ops = tuple(t.detach().contiguous() for t in (base, id_cols, act_cols, act.reshape(b, n)))
        prm = head_pack(ln_w, ln_b, w2, b2, w3, b3)
        v = torch.empty(b, S, n, dtype=torch.float32, device=base.device)
        launch("mapdn_critic_shapley_forward", base.device, *ops, pos32, b, S, n, *head_abi(prm, eps), v, None)
        _ShapleyCritic.launches += 1
        ctx.save_for_backward(pos32, *ops, *prm)
        ctx.eps, ctx.act_shape = float(eps), act.shape
        return v

    @staticmethod
    def backward(ctx, dv):
        pos32, base, idc, actc, act, *prm = ctx.saved_tensors
        b, S, n = pos32.shape
        need, dev = ctx.needs_input_grad, base.device
        param_grads = any(need[i] for i in (1, 2, 3, 5, 6, 8, 9, 10, 11))
        dv2 = dv.reshape(b, S, n).contiguous()
        dact = torch.empty(b, n, dtype=torch.float32, device=dev) if need[0] else None
        dbase = grads = scratch = None
        if param_grads:
            dbase = torch.empty_like(base)
            grads = torch.empty(HEAD_GRADS + 2 * n * 64, dtype=torch.float32, device=dev)
            scratch = buffer("mapdn_critic_shapley_scratch_floats", dev, b, S, n, at_least=1)
        launch("mapdn_critic_shapley_backward", dev, dv2, base, idc, actc, act, pos32, b, S, n, *head_abi(prm, ctx.eps), dbase, grads, scratch, dact,
               int(param_grads))
        da = dact.view(ctx.act_shape) if dact is not None else None
        if not param_grads:
            return (da,) + (None,) * 11
        return (da, dbase, *shapley_tails(grads, n), None, *head_param_grads(grads))


@functools.lru_cache(maxsize=None)
def shapley_max_agents() -> int:
    """the largest n the coalition kernels admit (their per-wavefront LDS holds one group's prefix and two [n][64] accumulators)"""
    m = ctypes.c_int32(0)
    entry("mapdn_critic_shapley_geometry")(1, 1, 1, 0, 1, None, None, None, None, ctypes.byref(m))
    return int(m.value)


def shapley_ok(cr: "MLPCritic", base: torch.Tensor, n: int, S: int) -> bool:
    """the coalition kernels cover the reference's default critic (LayerNorm, ReLU, hidden size 64, one output) in fp32 on the GPU for
    n <= shapley_max_agents() and fewer than 2^31 rows; MAPDN_FUSED_SHAP=0 switches them off (the factored PyTorch form remains)"""
    return (base.is_cuda and base.dtype == torch.float32 and base.dim() == 2 and base.shape[-1] == 64 and default_critic_fp32(cr)
            and os.environ.get("MAPDN_FUSED_SHAP", "1") != "0" and base.shape[0] >= 1 and base.shape[0] * S * n < 2 ** 31 - 1
            and n <= shapley_max_agents())


class SQDDPGNet(DDPGNet):
    """`SQDDPG(Model)` (models/sqddpg.py:10-160): the deterministic recurrent agents, target handling and reward BatchNorm are DDPGNet's; the
    critic is valued on sampled coalitions — per sample `sample_size` random orders of the agents, per order and agent one row that
    sees the actions of the agents before it and its own — and the mean over the orders is the agent's approximate Shapley value.
    Off-policy: the replay ring is kept between update rounds."""
    ALGS = ("sqddpg",)

    def __init__(self, args, alg: str = "sqddpg", target_net: Optional["SQDDPGNet"] = None):
        ids = self._begin(args, alg, _sqddpg_args_ok)
        self.sample_size = int(args.sample_size)
        n, o, a = self.n_, self.obs_dim, self.act_dim
        self.batchnorm = nn.BatchNorm1d(n)                         # rewards (model.py:317-318) AND advantages (sqddpg.py:19, 155-156)
        self.__dict__["_adv_batchnorm"] = self.batchnorm
        copies = 1 if args.shared_params else n
        self.value_dicts = nn.ModuleList([MLPCritic((o + a) * n + ids, 1, args) for _ in range(copies)])       # sqddpg.py:22-31: ids AFTER the actions
        self.policy_dicts = nn.ModuleList([RNNAgent(o + ids, args) for _ in range(copies)])
        self._finish(target_net)

    def sample_coalitions(self, batch_size: int, device) -> torch.Tensor:
        """pos [b, S, n] int64 from one multinomial draw of shape [b S, n] (sqddpg.py:37-40)"""
        return sample_coalition_positions(batch_size * self.sample_size, self.n_, device).view(batch_size, self.sample_size, self.n_)

    def marginal_contribution(self, obs: torch.Tensor, act: torch.Tensor, pos: Optional[torch.Tensor] = None,
                              own_action_only: bool = False) -> torch.Tensor:
        """sqddpg.py:65-106: obs [b, n, o], act [b, n, 1] -> [b, S, n, 1]; pos [b, S, n] replaces the draw.  Routes: (a) the coalition
        kernels where shapley_ok; (b) the factored PyTorch form (shapley_first_layer: cumsum + gather), also the CPU path; (c) without
        shared parameters the same factored form per agent critic.  own_action_only: the caller differentiates with respect to `act`
        alone (the policy loss): the first layer's operands enter detached, and route (a) then skips every parameter gradient."""
        b, n, o = obs.shape[0], self.n_, self.obs_dim
        if pos is None:
            pos = self.sample_coalitions(b, obs.device)
        S, ids = pos.shape[1], self.id_dim
        obs_all, act2 = obs.reshape(b, n * o), act.reshape(b, n)
        if self.args.shared_params:
            cr = self.value_dicts[0]
            w, b1 = (cr.fc1.weight.detach(), cr.fc1.bias.detach()) if own_action_only else (cr.fc1.weight, cr.fc1.bias)
            base = tall_linear_w(obs_all, w[:, :n * o], b1)
            act_cols = w[:, n * o:n * o + n].t()
            id_cols = w[:, n * o + n:].t() if ids else None
            if ids and shapley_ok(cr, base, n, S):
                prm = head_params(cr)
                if own_action_only:
                    prm = tuple(t.detach() if torch.is_tensor(t) else t for t in prm)
                v = _ShapleyCritic.apply(act2, base, id_cols, act_cols, pos.to(torch.int32).contiguous(), *prm)
                return v.view(b, S, n, 1)
            x = shapley_first_layer(base, id_cols, act_cols, act2, pos)
            v, _ = cr.trunk(x.reshape(b * S * n, -1))
            return v.view(b, S, n, 1)
        vs = []
        for i, cr in enumerate(self.value_dicts):
            w, b1 = (cr.fc1.weight.detach(), cr.fc1.bias.detach()) if own_action_only else (cr.fc1.weight, cr.fc1.bias)
            base = F.linear(obs_all, w[:, :n * o], b1)
            x = shapley_first_layer(base, w[:, n * o + n + i] if ids else None, w[:, n * o:n * o + n].t(), act2, pos, who=i)
            vs.append(cr.trunk(x.reshape(b * S, -1))[0].view(b, S, 1))
        return torch.stack(vs, 2)

    def value(self, obs: torch.Tensor, act: torch.Tensor, own_action_only: bool = False) -> torch.Tensor:
        """sqddpg.py:108-109: the marginal contributions of a fresh draw, [b, S, n, 1]"""
        return self.marginal_contribution(obs, act)

    def get_loss(self, batch: Batch, want=("policy", "value")):
        """sqddpg.py:133-160.  Three coalition draws per call, in the reference's order: for the policy actions at `state`, for the replay
        actions at `state`, for the next actions at `next_state` (on the target net).  batch["coalitions"] (three pos [bs, S, n]) replaces
        them.  A loss not in `want` is None and its forward passes are skipped, but its draw is still made, so that the generator goes the
        reference's way (and `batchnorm`, under normalize_advantages, still sees the advantages while training).  The rewards pass
        `batchnorm` under reward_normalisation as for every algorithm (model.py:317-318); sqddpg.py adds nothing of its own."""
        n, a = self.n_, self.args
        state, actions, next_state, avail, last_hid, hid, rewards, done, valid, wmean = self._unpack(batch)
        bs = state.shape[0]
        want_p, want_v = "policy" in want, "value" in want
        given = batch.get("coalitions")
        draw = (lambda k: given[k].view(bs, -1, n)) if given is not None else (lambda k: self.sample_coalitions(bs, state.device))
        stats = self.training and a.normalize_advantages             # `batchnorm` sees the advantages in every call of the reference
        policy_loss = value_loss = action_out = None
        pos_pol = draw(0)
        if want_p or stats:
            with torch.set_grad_enabled(want_p and torch.is_grad_enabled()):
                _, actions_pol, _, action_out, _ = self.get_actions(state, "train", False, avail, False, last_hid, means_grad_only=True)
                advantages = self.marginal_contribution(state, actions_pol, pos_pol, own_action_only=True).mean(dim=1).view(-1, n)
                if a.normalize_advantages:
                    advantages = self._adv_batchnorm.to(advantages.device)(advantages)
            if want_p:
                policy_loss = wmean(-advantages)
        pos_val, pos_next = draw(1), draw(2)
        if want_v:
            with torch.no_grad():
                _, next_actions, _, _, _ = self.get_actions(next_state, "train", False, avail, not a.double_q, hid, means_grad_only=True)
                net = self.target_net if a.target else self
                next_sum = net.marginal_contribution(next_state, next_actions, pos_next).mean(dim=1).view(-1, n).sum(dim=-1, keepdim=True)
                returns = rewards + a.gamma * (1 - done) * next_sum.expand(bs, n)
            value_sum = self.marginal_contribution(state, actions.detach(), pos_val).mean(dim=1).view(-1, n).sum(dim=-1, keepdim=True)
            value_loss = wmean((returns - value_sum.expand(bs, n)).pow(2))
        return policy_loss, value_loss, (action_out if want_p else None)
