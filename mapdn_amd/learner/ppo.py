"""MAPPO / IPPO (models/mappo.py, models/ippo.py, learning_algorithms/ppo.py): the deterministic agents with a state-value critic,
generalised advantage estimation and the clipped surrogate / clipped value losses; the GAE recurrence over strided chains and both
losses with their gradients are the launches of csrc/ppo.hip.  Reached through make_alg_args(..., alg="mappo" | "ippo").  Two quirks of
the reference are kept and stated at PPONet."""

import math
import os
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._hip import buffer, launch
from .args import Batch, _ppo_args_ok
from .ddpg import DDPGNet, _wmean
from .head import critic_head, critic_head_ok
from .modules import MLPCritic, RNNAgent
from .ops import tall_linear_w


_LOG_SQRT_2PI = math.log(math.sqrt(2 * math.pi))
PPO_MAX_ELEMS = 1 << 40                    # csrc/capi.hip ppo_shape_ok: rows * n at most


def ppo_fused_ok(*tensors) -> bool:
    """the PPO kernels (csrc/ppo.hip: the strided GAE, the two clipped losses) cover fp32 tensors on the GPU with at most 2^40 elements;
    MAPDN_FUSED_PPO=0 switches them off (the vectorised PyTorch forms below remain, which are also the CPU route).  tensors: every tensor
    the launch would read (None for an optional one that is absent); the first is a per-agent [rows, n] one."""
    return (os.environ.get("MAPDN_FUSED_PPO", "1") != "0" and all(t is None or (t.is_cuda and t.dtype == torch.float32) for t in tensors)
            and tensors[0].dim() == 2 and 1 <= tensors[0].numel() <= PPO_MAX_ELEMS)


def ppo_gae_torch(reward, value, next_value, done, last_step, stride: int, gamma: float, lambda_: float) -> torch.Tensor:
    """ppo.py:46-54 over chains of `stride`: row i's successor is row i + stride.  reward / value / next_value [rows, n], done / last_step
    [rows] -> advantages [rows, n].  A loop over the ceil(rows / stride) chain STEPS on [stride, n] slices (newest first), never over
    rows; stride 1 is the reference's loop, operation for operation."""
    rows = reward.shape[0]
    S = int(stride)
    mask = torch.where(last_step != 0, 1.0 - done, torch.ones_like(done)).unsqueeze(-1)          # ppo.py:48-51
    delta = reward + gamma * next_value * mask - value                                            # ppo.py:52
    adv = torch.empty_like(delta)
    last = torch.zeros_like(delta[:min(S, rows)])
    for t in reversed(range(-(-rows // S))):
        lo, hi = t * S, min((t + 1) * S, rows)
        new = delta[lo:hi] + gamma * lambda_ * last[:hi - lo] * mask[lo:hi]                       # ppo.py:53
        adv[lo:hi] = new
        last = new if hi - lo == last.shape[0] else torch.cat((new, last[hi - lo:]))             # (the ragged end: the other chains start one step later)
    return adv


def ppo_gae(reward, value, next_value, done, last_step, stride: int, gamma: float, lambda_: float) -> torch.Tensor:
    """the advantages of ppo_gae_torch, without autograd: ONE launch (mapdn_ppo_gae) where ppo_fused_ok, the chain-step loop otherwise"""
    if stride < 1:
        raise ValueError(f"GAE chain stride {stride} must be at least 1")
    r, v, nv, d, ls = (t.detach() for t in (reward, value, next_value, done, last_step))
    if not ppo_fused_ok(r, v, nv, d, ls):
        with torch.no_grad():
            return ppo_gae_torch(r, v, nv, d, ls, stride, gamma, lambda_)
    r, v, nv, d, ls = (t.contiguous() for t in (r, v, nv, d, ls))
    rows, n = r.shape
    adv = torch.empty_like(r)
    launch("mapdn_ppo_gae", r.device, r, v, nv, d, ls, adv, rows, n, int(stride), float(gamma), float(lambda_))
    ppo_gae.launches += 1
    return adv


ppo_gae.launches = 0            # how often the kernel was reached (tests count the routes)


def _ppo_weights(valid: Optional[torch.Tensor], like: torch.Tensor):
    """(valid as f32 [rows] or None, scale [1] = 1 / (the divisor of DDPGNet.get_loss's wmean)) for a per-agent tensor [rows, n]"""
    rows, n = like.shape
    if valid is None:
        return None, like.new_full((1,), 1.0 / (rows * n))
    vf = valid.float().view(-1).contiguous()
    return vf, (1.0 / (vf.sum().clamp(min=1.0) * n)).reshape(1)


def _ppo_loss_launch(ctx, cls, name: str, wrt: torch.Tensor, first: torch.Tensor, *rest) -> torch.Tensor:
    """what both loss wrappers do around their entry call lib.<name>(first, *rest, loss, d loss / d wrt, partial, rows, n): the gradient is kept
    for backward, which scales it by the incoming one (1 for `loss.backward()`)"""
    (rows, n), dev = first.shape, first.device
    loss, grad = torch.empty(1, dtype=torch.float32, device=dev), torch.empty_like(first)
    launch(name, dev, first, *rest, loss, grad, buffer("mapdn_ppo_loss_blocks", dev, rows * n), rows, n)
    cls.launches += 1
    ctx.save_for_backward(grad)
    ctx.shape = wrt.shape
    return loss[0].clone()


class _PPOPolicyLoss(torch.autograd.Function):
    """-wmean(min(rho A, clamp(rho, 1 -/+ eps) A)) of ppo.py:39, 62-64 and its gradient with respect to the policy means as ONE entry
    call (mapdn_ppo_policy_loss: the streaming launch + the fixed-order pass over its per-workgroup partial sums).  backward scales the
    stored gradient by the incoming one (1 for `loss.backward()`).  The log-std of the non-Gaussian agent is a constant: no gradient."""
    launches = 0

    @staticmethod
    def forward(ctx, means, actions, log_stds, avail, old_log_prob, adv, valid, scale, eps_clip):
        rows, n = adv.shape
        mu, ac, ls, ol, ad = (t.detach().reshape(rows, n).contiguous() for t in (means, actions, log_stds, old_log_prob, adv))
        av = avail.detach().reshape(rows, n).contiguous() if avail is not None else None
        return _ppo_loss_launch(ctx, _PPOPolicyLoss, "mapdn_ppo_policy_loss", means, ac, mu, ls, av, ol, ad, valid, scale, float(eps_clip))

    @staticmethod
    def backward(ctx, g):
        (dmean,) = ctx.saved_tensors
        return ((dmean * g).view(ctx.shape),) + (None,) * 8


class _PPOValueLoss(torch.autograd.Function):
    """coef wmean(max((V - R)^2, (V_clip - R)^2)) of ppo.py:56, 67-70 and its gradient with respect to V as ONE entry call
    (mapdn_ppo_value_loss), R = r + gamma (1 - done) V(next) formed inside; backward scales the stored gradient by the incoming one"""
    launches = 0

    @staticmethod
    def forward(ctx, values, old_values, reward, next_values, done, valid, scale, gamma, eps_clip, coef):
        rows, n = old_values.shape
        v, vo, r, vn = (t.detach().reshape(rows, n).contiguous() for t in (values, old_values, reward, next_values))
        d = done.detach().reshape(rows).contiguous()
        return _ppo_loss_launch(ctx, _PPOValueLoss, "mapdn_ppo_value_loss", values, v, vo, r, vn, d, valid, scale, float(gamma), float(eps_clip),
                                float(coef))

    @staticmethod
    def backward(ctx, g):
        (dv,) = ctx.saved_tensors
        return ((dv * g).view(ctx.shape),) + (None,) * 9


def ppo_policy_loss_torch(means, actions, log_stds, avail, old_log_prob, adv, valid, eps_clip: float) -> torch.Tensor:
    """ppo.py:30-33, 39, 62-64 as written (Normal(means, stds).log_prob of utilities/util.py:44-46 spelled out); [bs, n, 1] tensors, adv
    [bs, n]; the means of the loss weighted by `valid` as in DDPGNet.get_loss"""
    std = log_stds.exp()
    log_prob = -((actions - means) ** 2) / (2 * std ** 2) - std.log() - _LOG_SQRT_2PI
    mask = 1.0 if avail is None else 1.0 - (avail == 0).to(log_prob.dtype)
    log_prob, old = (mask * log_prob).sum(dim=-1), (mask * old_log_prob).sum(dim=-1)
    ratios = torch.exp(log_prob - old.detach())
    adv = adv.detach()
    return -_wmean(valid)(torch.min(ratios * adv, torch.clamp(ratios, 1 - eps_clip, 1 + eps_clip) * adv))


def ppo_value_loss_torch(values, old_values, reward, next_values, done, valid, gamma: float, eps_clip: float, coef: float) -> torch.Tensor:
    """ppo.py:56, 67-70 as written; [bs, n] tensors, done [bs]"""
    returns = reward + gamma * (1 - done.view(-1, 1)) * next_values.detach()
    clipped = old_values + torch.clamp(values - old_values, -eps_clip, eps_clip)
    return coef * _wmean(valid)(torch.max((values - returns).pow(2), (clipped - returns).pow(2)))


def ppo_policy_loss(means, actions, log_stds, avail, old_log_prob, adv, valid, eps_clip: float) -> torch.Tensor:
    if not (ppo_fused_ok(adv, means, actions, log_stds, avail, old_log_prob) and means.shape[-1] == 1 and not log_stds.requires_grad):
        return ppo_policy_loss_torch(means, actions, log_stds, avail, old_log_prob, adv, valid, eps_clip)
    vf, scale = _ppo_weights(valid, adv)
    return _PPOPolicyLoss.apply(means, actions, log_stds, avail, old_log_prob, adv, vf, scale, eps_clip)


def ppo_value_loss(values, old_values, reward, next_values, done, valid, gamma: float, eps_clip: float, coef: float) -> torch.Tensor:
    if not ppo_fused_ok(old_values, values, reward, next_values, done):
        return ppo_value_loss_torch(values, old_values, reward, next_values, done, valid, gamma, eps_clip, coef)
    vf, scale = _ppo_weights(valid, old_values)
    return _PPOValueLoss.apply(values, old_values, reward, next_values, done, vf, scale, gamma, eps_clip, coef)


class PPONet(DDPGNet):
    """`MAPPO(Model)` (models/mappo.py:11) and `IPPO(Model)` (models/ippo.py:10) with the loss of `PPO` (learning_algorithms/ppo.py): the
    deterministic recurrent agents (their fixed std makes them a Gaussian policy for the ratio), target handling and reward BatchNorm
    are DDPGNet's; the critic is a state value V(s) — MAPPO's on [all obs | id], IPPO's on [own obs | id].  On-policy: PGTrainer empties
    the replay ring after every update round (models/model.py:53-56), stores log_prob / value / next_value with every transition, and
    sets `gae_stride` to its env count.

    Two quirks of the reference are kept.  (1) The GAE mask (ppo.py:48-51) is 1 - done on a last_step row and 1 on every other row, so
    a timeout (last_step without done) does not cut the chain, nor does a done without last_step.  (2) Model.unpack_data
    (models/model.py:309) fills old_log_prob_a from batch.action, so the reference's ratio is exp(log_prob_new - action):
    args.ppo_old_log_prob="reference" (the default; not a reference key) does the same, "stored" takes the log-probability recorded at
    rollout time (batch["log_prob"]).  The target net is built, updated and saved, and never read by the loss (ppo.py:16).

    Chain stride.  get_loss(batch, want, stride) treats row i + stride as row i's successor (default: the attribute `gae_stride`, 1
    unless the trainer set it; 1 is the reference's row-by-row walk, literally).  The replay ring holds rows in (step, env) order and
    every insertion adds one row per env, so with stride = the env count each residue class of a sampled window is one env's time
    series wherever the window starts.  A window shorter than the stride gives chains of one row (advantage = delta): on-policy
    training wants batch_size to be a multiple of the env count."""
    ALGS = ("mappo", "ippo")

    def __init__(self, args, alg: str = "mappo", target_net: Optional["PPONet"] = None):
        ids = self._begin(args, alg, _ppo_args_ok)
        n, o = self.n_, self.obs_dim
        self.batchnorm = nn.BatchNorm1d(n)                         # rewards only (model.py:317-318)
        # advantages: PPO.batchnorm (ppo.py:11, 58-59) lives on a plain object — not part of the state_dict, never switched to eval
        self.__dict__["_adv_batchnorm"] = nn.BatchNorm1d(n)
        self.__dict__["gae_stride"] = 1
        copies = 1 if args.shared_params else n
        critic_in = (n * o if alg == "mappo" else o) + ids         # mappo.py:21-26, ippo.py:20-25: a V(s), no action columns
        self.value_dicts = nn.ModuleList([MLPCritic(critic_in, 1, args) for _ in range(copies)])
        self.policy_dicts = nn.ModuleList([RNNAgent(o + ids, args) for _ in range(copies)])
        self._finish(target_net)

    def value(self, obs: torch.Tensor, act: Optional[torch.Tensor] = None, own_action_only: bool = False) -> torch.Tensor:
        """obs [b, n, o] -> V [b, n, 1]; `act` is ignored (mappo.py:36-65, ippo.py:35-59).  MAPPO's [b, n, n o] input is never built: the
        first layer is W_obs·obs_all + b1 once per sample plus the agent's id column, and with the default critic on the GPU everything
        behind it is the one-launch head on rows formed as base[b] + per_n[i]."""
        b, n, o, ids = obs.shape[0], self.n_, self.obs_dim, self.id_dim
        if self.alg == "ippo":
            if self.args.shared_params:
                cr = self.value_dicts[0]
                w = cr.fc1.weight
                x = tall_linear_w(obs.reshape(b * n, o), w[:, :o], cr.fc1.bias)
                if ids:
                    x = (x.view(b, n, -1) + w[:, o:].t().unsqueeze(0)).reshape(b * n, -1)
                return cr.trunk(x)[0].view(b, n, 1)
            return torch.stack([cr.trunk(F.linear(obs[:, i], cr.fc1.weight[:, :o], cr.fc1.bias) + (cr.fc1.weight[:, o + i] if ids else 0.0))[0]
                                for i, cr in enumerate(self.value_dicts)], 1)
        obs_all = obs.reshape(b, n * o)
        if self.args.shared_params:
            cr = self.value_dicts[0]
            w = cr.fc1.weight
            base = tall_linear_w(obs_all, w[:, :n * o], cr.fc1.bias)                         # [b, h]: once per sample
            if ids:
                per_n = w[:, n * o:].t()                                                    # [n, h]: the id columns
                if critic_head_ok(cr, base, b * n, n):
                    return critic_head(cr, base, per_n).view(b, n, 1)
                x = base.unsqueeze(1) + per_n.unsqueeze(0)
            else:
                x = base.unsqueeze(1).expand(b, n, -1)
            return cr.trunk(x.reshape(b * n, -1))[0].view(b, n, 1)
        return torch.stack([cr.trunk(F.linear(obs_all, cr.fc1.weight[:, :n * o], cr.fc1.bias) + (cr.fc1.weight[:, n * o + i] if ids else 0.0))[0]
                            for i, cr in enumerate(self.value_dicts)], 1)

    @torch.no_grad()
    def advantages(self, batch: Batch, rewards: torch.Tensor, stride: Optional[int] = None) -> torch.Tensor:
        """GAE on the STORED value / next_value (ppo.py:46-54) over chains of `stride`, through PPO.batchnorm with normalize_advantages
        (ppo.py:58-59; the union of the ranks' batches under data-parallel training): [bs, n], no gradient"""
        n, a = self.n_, self.args
        S = int(self.__dict__.get("gae_stride", 1) if stride is None else stride)
        adv = ppo_gae(rewards, batch["value"].float().view(-1, n), batch["next_value"].float().view(-1, n), batch["done"].float().view(-1),
                      batch["last_step"].float().view(-1), S, a.gamma, a.lambda_)
        if a.normalize_advantages:
            adv = self._union_batchnorm(self._adv_batchnorm.to(adv.device), adv)
        return adv.detach()

    def get_loss(self, batch: Batch, want=("policy", "value"), stride: Optional[int] = None):
        """ppo.py:16-71.  batch: the fields of DDPGNet.get_loss plus last_step [bs, 1], value / next_value [bs, n, 1] (what the behaviour
        critic gave at rollout time) and, for ppo_old_log_prob="stored", log_prob [bs, n, 1].  stride: the GAE chain stride (see the
        class).  The returns use FRESH behaviour-net values of next_state, the advantages the STORED ones; the target net is not read.
        No random number is drawn.  Returns (policy_loss, value_loss, (means, log_stds)); a loss not in `want` is None and its forward
        passes are skipped (the reward BatchNorm sees the rewards in every call, as the reference's does)."""
        n, a = self.n_, self.args
        rewards = self.normalise_reward(batch["reward"].float())
        valid = batch.get("valid")
        policy_loss = value_loss = action_out = None
        if "policy" in want:
            actions, avail = batch["action"], batch["action_avail"]
            means, log_stds, _ = self.policy(batch["state"], batch["last_hid"], means_grad_only=True)
            action_out = (means, log_stds)
            adv = self.advantages(batch, rewards.detach(), stride)
            old = actions if a.ppo_old_log_prob == "reference" else batch["log_prob"].float()       # models/model.py:309
            policy_loss = ppo_policy_loss(means, actions, log_stds, avail, old, adv, valid, a.eps_clip)
        if "value" in want:
            values = self.value(batch["state"]).view(-1, n)
            with torch.no_grad():
                next_values = self.value(batch["next_state"]).view(-1, n)                           # ppo.py:41, 56: the behaviour net, now
            value_loss = ppo_value_loss(values, batch["value"].float().view(-1, n), rewards.detach(), next_values, batch["done"].float().view(-1),
                                        valid, a.gamma, a.eps_clip, a.value_loss_coef)
        return policy_loss, value_loss, action_out
