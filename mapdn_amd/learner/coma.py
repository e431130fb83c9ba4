"""COMA (models/coma.py).  The counterfactual baseline (coma.py:139-151: the critic valued sample_size more times with one agent's action
redrawn) is one HIP launch over the first layer's output (head.critic_counterfactual), a sampled row being the taken row plus a rank-1 term."""

import math
from typing import Optional

import torch
import torch.nn.functional as F

from .args import Batch
from .ddpg import DDPGNet
from .head import critic_cf_ok, critic_counterfactual
from .ops import tall_linear_w


class COMANet(DDPGNet):
    """`COMA(Model)` (models/coma.py:11): the policy, target handling, reward BatchNorm and value half of the loss are DDPGNet's; the
    critic input, the counterfactual baseline and the policy loss are its own.  On-policy: PGTrainer empties the replay ring after every
    update round (models/model.py:53-56)."""
    ALGS = ("coma",)

    def __init__(self, args, alg: str = "coma", target_net: Optional["COMANet"] = None):
        if alg in self.ALGS and int(args.sample_size) < 2:
            # coma.py:44 tells the sampled actions [S b, n, n a] from taken ones [b, n, a] by the batch dimension: equal at S == 1
            raise ValueError(f"sample_size must be at least 2 for COMA (got {args.sample_size})")
        super().__init__(args, alg, target_net)

    def _coma_first_layer(self, cr, obs, act, who=None):
        """first layer of COMA's critic on [all obs (n o) | own obs (o) | ids (n) | joint action (n a)] (coma.py:24, 53-80) as
        W_all·obs_all + b1 + W_act·act_all (per batch element) + W_own·obs[b, i] + id column (per agent): [b, n, h] for who None, [b, h]
        for agent `who`; never built at input width.  Every action carries gradient (coma.py has no detach in value())."""
        b, n, o, a, ids = obs.shape[0], self.n_, self.obs_dim, self.act_dim, self.id_dim
        w = cr.fc1.weight
        na = (n + 1) * o + ids
        base = tall_linear_w(obs.reshape(b, n * o), w[:, :n * o], cr.fc1.bias) + tall_linear_w(act.reshape(b, n * a), w[:, na:na + n * a])      # [b, h]
        if who is not None:
            x = base + F.linear(obs[:, who], w[:, n * o:(n + 1) * o])
            return x + w[:, (n + 1) * o + who] if ids else x
        x = tall_linear_w(obs.reshape(b * n, o), w[:, n * o:(n + 1) * o]).view(b, n, -1) + base.unsqueeze(1)
        if ids:
            x = x + w[:, (n + 1) * o:na].t().unsqueeze(0)
        return x

    def _value_coma(self, obs, act):
        """coma.py:43-104 on taken actions (obs and act of the same batch size): [b, n, 1]"""
        b, n = obs.shape[0], self.n_
        if self.args.shared_params:
            cr = self.value_dicts[0]
            return cr.trunk(self._coma_first_layer(cr, obs, act).reshape(b * n, -1))[0].view(b, n, 1)
        return torch.stack([cr.trunk(self._coma_first_layer(cr, obs, act, i))[0] for i, cr in enumerate(self.value_dicts)], 1)

    def sampled_actions(self, means: torch.Tensor, log_stds: torch.Tensor, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """coma.py:139-143: th.normal(means, std) for sample_size repeats of the batch, [S, b, n, a] — ONE draw per get_loss call, taken as
        means + std * randn (the same numbers from the same generator state; tests/golden/make_coma_golden.py asserts it), or with
        `noise` [S, b, n, a] in the place of randn"""
        S = int(self.args.sample_size)
        eps = torch.randn((S,) + tuple(means.shape), dtype=means.dtype, device=means.device) if noise is None else noise.to(means.dtype).view((S,) + tuple(means.shape))
        return means.detach().unsqueeze(0) + log_stds.detach().exp().unsqueeze(0) * eps

    @torch.no_grad()
    def counterfactual(self, obs: torch.Tensor, act: torch.Tensor, sampled: torch.Tensor):
        """(baselines [b, n], values [b, n]) of coma.py:144-152: baselines[b, i] = mean over s of Q_i(obs, act with agent i's action
        replaced by sampled[s, b, i]); values = Q(obs, act).  The critic's first layer is linear in the actions, so the replaced input
        is the taken one plus (sampled - act)[b, i] · W_act[:, i]: the [S b, n, (n + 1) o + n + n a] input of the reference is never
        built.  The default critic on the GPU with one action per agent: ONE launch for all samples and the values
        (critic_counterfactual); otherwise a loop over the samples through the PyTorch modules."""
        b, n, o, a, ids = obs.shape[0], self.n_, self.obs_dim, self.act_dim, self.id_dim
        na = (n + 1) * o + ids
        S = sampled.shape[0]
        delta = sampled - act.unsqueeze(0)                                           # [S, b, n, a]
        if self.args.shared_params:
            cr = self.value_dicts[0]
            x = self._coma_first_layer(cr, obs, act).reshape(b * n, -1)
            w_act = cr.fc1.weight[:, na:na + n * a]
            if critic_cf_ok(cr, x, b * n, a):
                base, v0 = critic_counterfactual(cr, x, w_act.t(), delta.reshape(S, b * n))
                return base.view(b, n), v0.view(b, n)
            own_col = w_act.reshape(-1, n, a)                                        # [h, n, a]: agent i's own action columns
            values = cr.trunk(x)[0].view(b, n)
            total = torch.zeros_like(values)
            for s in range(S):
                total += cr.trunk(x + torch.einsum("bna,hna->bnh", delta[s], own_col).reshape(b * n, -1))[0].view(b, n)
            return total / S, values
        xs = [self._coma_first_layer(cr, obs, act, i) for i, cr in enumerate(self.value_dicts)]
        values = torch.stack([cr.trunk(x)[0] for x, cr in zip(xs, self.value_dicts)], 1).view(b, n)
        total = torch.zeros_like(values)
        for s in range(S):
            total += torch.stack([cr.trunk(x + F.linear(delta[s][:, i], cr.fc1.weight[:, na + i * a:na + (i + 1) * a]))[0]
                                  for i, (x, cr) in enumerate(zip(xs, self.value_dicts))], 1).view(b, n)
        return total / S, values

    def _coma_policy_loss(self, batch: Batch, wmean, want_loss: bool):
        """coma.py:131-152, 181-190: policy_loss = -mean(advantages * log_prob), advantages = (Q(s, a) - baseline).detach() (through
        `batchnorm` with normalize_advantages), log_prob of the STORED action under N(mean, std), masked by the available actions.
        The sample_size draws are taken in every call, as the reference does (coma.py:143 runs for the value update too);
        batch["cf_noise"] [S, bs, n, a] replaces the standard-normal draw.  want_loss False (a value update): only what the call
        changes besides the loss is done — the draw, and with normalize_advantages the running statistics of `batchnorm`."""
        n = self.n_
        state, actions, avail = batch["state"], batch["action"], batch["action_avail"]
        if not want_loss and not (self.args.normalize_advantages and self.batchnorm.training):
            if batch.get("cf_noise") is None:                    # the call's one draw, so that the generator goes the reference's way
                torch.randn((int(self.args.sample_size),) + tuple(actions.shape), dtype=torch.float32, device=actions.device)
            return None, None
        with torch.set_grad_enabled(want_loss and torch.is_grad_enabled()):
            means, log_stds, _ = self.policy(state, batch["last_hid"], means_grad_only=True)
        sampled = self.sampled_actions(means, log_stds, batch.get("cf_noise"))
        baselines, values = self.counterfactual(state, actions, sampled)
        advantages = (values - baselines).detach()
        if self.args.normalize_advantages:
            advantages = self._adv_batchnorm.to(advantages.device)(advantages)
        if not want_loss:
            return None, None
        std = log_stds.exp()
        log_prob = -((actions - means) ** 2) / (2 * std ** 2) - log_stds - math.log(math.sqrt(2 * math.pi))      # util.py:44-46
        log_prob = ((1.0 - (avail == 0).to(log_prob.dtype)) * log_prob).sum(-1).view(-1, n)
        return wmean(-advantages * log_prob), (means, log_stds)
