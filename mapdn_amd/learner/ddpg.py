"""MADDPG / IDDPG / MATD3 (models/maddpg.py, models/iddpg.py, models/matd3.py, learning_algorithms/ddpg.py, models/model.py) — and the base
class of every other net.  Tensors in, tensors out: a batch is a dict of device tensors straight from `mapdn_amd.replay`.  The central
MADDPG critic never materialises the reference's [batch, n, n·obs] input (maddpg.py:41-66): its first layer is (shared observation
term) + (agent-id column) + (joint-action term), with the "other agents' actions are detached" rule (maddpg.py:52-58) kept by a
zero-valued, gradient-carrying own-action term.  MATD3's twin (matd3.py:35-86: ONE critic valued twice, one more input column that is 0
or 1) is that first layer and the same plus the last column of fc1.weight, both heads in one HIP launch."""

import math
import os
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._hip import entry, launch
from .args import Batch
from .head import (_CriticHeadMSE, _CriticHeadOwnAction, _CriticTwinMSE, critic_head, critic_head_ok, critic_twin_forward, critic_twin_ok,
                   head_params, twin_pair_mse)
from .modules import MLPCritic, RNNAgent, _PolicyTrunk
from .ops import _TallLinear, _tall_ok, layernorm_act_bc, tall_linear_w


def _wmean(valid):
    """the mean over (batch, agent) of a [bs, n] tensor, weighted by `valid` [bs] when given (1 everywhere = the reference's plain mean)"""
    return (lambda t: t.mean()) if valid is None else \
        (lambda t: (t * valid.float().view(-1, 1)).sum() / (valid.float().sum().clamp(min=1.0) * t.shape[1]))


class DDPGNet(nn.Module):
    """`MADDPG(Model)` (models/maddpg.py:10), `IDDPG(Model)` (models/iddpg.py:9), `MATD3(Model)` (models/matd3.py:10): behaviour net
    holding its target net, the per-agent reward BatchNorm (models/model.py:26) and the DDPG loss.  `COMA(Model)` is the subclass COMANet."""

    ALGS = ("maddpg", "iddpg", "matd3")         # the algorithms this class is; COMANet (coma.py) is "coma"; net_class(alg) picks the class

    def __init__(self, args, alg: str = "maddpg", target_net: Optional["DDPGNet"] = None):
        ids = self._begin(args, alg)
        n, o, a = self.n_, self.obs_dim, self.act_dim
        self.batchnorm = nn.BatchNorm1d(n)
        # advantage normalisation: MADDPG re-uses `batchnorm` (maddpg.py:17,120); IDDPG's lives in its DDPG
        # helper object, which is not an nn.Module — so it is NOT part of the state_dict (ddpg.py:10,34)
        # (MATD3's is `batchnorm` too: matd3.py:18,146-147; COMA's as well: coma.py:19,183-184)
        self.__dict__["_adv_batchnorm"] = self.batchnorm if alg in ("maddpg", "matd3", "coma") else nn.BatchNorm1d(n)
        critic_in = {"maddpg": (o + a) * n + ids, "iddpg": o + a + ids, "matd3": (o + a) * n + ids + 1,
                     "coma": (n + 1) * o + n * a + ids}[alg]       # maddpg.py:20-24, iddpg.py:19-23, matd3.py:20-25, coma.py:21-27
        copies = 1 if args.shared_params else n
        self.value_dicts = nn.ModuleList([MLPCritic(critic_in, 1, args) for _ in range(copies)])
        self.policy_dicts = nn.ModuleList([RNNAgent(o + ids, args) for _ in range(copies)])   # model.py:141-164
        self._finish(target_net)

    def _begin(self, args, alg: str, args_ok=None) -> int:
        """what every net class starts from; returns the width of the agent-id block of the first layers"""
        nn.Module.__init__(self)
        if alg not in self.ALGS:
            raise KeyError(alg)                                    # models/model_registry.py:14-25
        if args_ok is not None:
            args_ok(args)
        self.args, self.alg = args, alg
        self.n_, self.obs_dim, self.act_dim, self.hid_dim = args.agent_num, args.obs_size, args.action_dim, args.hid_size
        self._fused_fits = None                   # does the one-launch HIP policy forward have a launch shape for this obs width?
        return self.id_dim

    @property
    def id_dim(self) -> int:
        """the width of the one-hot agent-id block of the first layers"""
        return self.n_ if self.args.agent_id else 0

    def _finish(self, target_net):
        self.apply(self._init_weights)
        if target_net is not None:
            self.target_net = target_net
            self.reload_params_to_target()

    # ---- initialisation / target handling (models/model.py:28-48,169-177) ----------------------
    def _init_weights(self, m):
        if type(m) == nn.Linear:
            if self.args.init_type == "normal":
                nn.init.normal_(m.weight, 0.0, self.args.init_std)
            elif self.args.init_type == "orthogonal":
                nn.init.orthogonal_(m.weight, gain=nn.init.calculate_gain(self.args.hid_activation))

    def reload_params_to_target(self):
        self.target_net.policy_dicts.load_state_dict(self.policy_dicts.state_dict())
        self.target_net.value_dicts.load_state_dict(self.value_dicts.state_dict())

    @torch.no_grad()
    def update_target(self):
        """soft update over every state_dict entry of the policy and value nets (model.py:34-48)"""
        lr = self.args.target_lr
        for mine, theirs in ((self.policy_dicts, self.target_net.policy_dicts), (self.value_dicts, self.target_net.value_dicts)):
            src = mine.state_dict()
            for name, param in theirs.state_dict().items():
                param.copy_((1 - lr) * param + lr * src[name])

    def init_hidden(self, batch: int = 1):
        return self.policy_dicts[0].fc1.weight.new_zeros(batch, self.n_, self.hid_dim)    # rnn_agent.py:22-24

    # ---- policy (models/model.py:101-139) --------------------------------------------------------
    def _fused_policy_ok(self, obs: torch.Tensor, last_hid: torch.Tensor) -> bool:
        """the one-launch HIP forward (libmapdn_hip.so: mapdn_policy_forward) covers the reference's default agent — shared
        parameters, LayerNorm, ReLU, hidden size 64, one action — for inference on the GPU in fp32"""
        return (not torch.is_grad_enabled() and self._default_agent_fp32(obs, last_hid) and os.environ.get("MAPDN_FUSED_POLICY", "1") != "0"
                and self._fits())

    def _default_agent_fp32(self, obs: torch.Tensor, last_hid: torch.Tensor) -> bool:
        a = self.args
        return (obs.is_cuda and obs.dtype == torch.float32 and last_hid.dtype == torch.float32 and a.shared_params and a.layernorm
                and a.hid_activation == "relu" and self.hid_dim == 64 and self.act_dim == 1)

    def _fits(self) -> bool:
        if self._fused_fits is None:              # the parameter set + activations of one tile must fit a CU's LDS (wide observations,
            # e.g. history > 1 on the 322-bus net, do not): those keep the PyTorch modules
            self._fused_fits = bool(entry("mapdn_policy_forward_fits")(self.obs_dim, self.id_dim))
        return self._fused_fits

    def _fused_policy(self, obs: torch.Tensor, last_hid: torch.Tensor, need_hidden: bool = True):
        ag = self.policy_dicts[0]
        b, n, o = obs.shape[0], self.n_, self.obs_dim
        obs_c, hid_c = obs.contiguous(), last_hid.contiguous()
        means = torch.empty(b, n, 1, dtype=torch.float32, device=obs.device)
        hid = torch.empty(b, n, self.hid_dim, dtype=torch.float32, device=obs.device) if need_hidden else None
        prm = tuple(t.detach().contiguous() for t in (ag.fc1.weight, ag.fc1.bias, ag.layernorm.weight, ag.layernorm.bias, ag.rnn.weight_ih,
                                                      ag.rnn.weight_hh, ag.rnn.bias_ih, ag.rnn.bias_hh, ag.fc2.weight, ag.fc2.bias))
        launch("mapdn_policy_forward", obs.device, obs_c, hid_c, *prm, means, hid, b * n, n, o, self.id_dim, float(ag.layernorm.eps))
        return means, torch.full_like(means, math.log(self.args.fixed_policy_std)), hid

    def _fused_policy_train_ok(self, obs: torch.Tensor, last_hid: torch.Tensor) -> bool:
        return (torch.is_grad_enabled() and self._default_agent_fp32(obs, last_hid) and not last_hid.requires_grad and not obs.requires_grad
                and obs.shape[0] * self.n_ >= 4096 and os.environ.get("MAPDN_FUSED_POLICY_TRAIN", "1") != "0" and self._fits())

    def policy(self, obs: torch.Tensor, last_hid: torch.Tensor, means_grad_only: bool = False):
        """obs [b, n, o], last_hid [b, n, h] -> means [b, n, a], log_stds, hiddens [b, n, h].  means_grad_only: the caller differentiates the
        means alone (the policy loss; the new hidden state is then not returned) — the HIP forward / backward pair of _PolicyTrunk."""
        b, n, o = obs.shape[0], self.n_, self.obs_dim
        if self._fused_policy_ok(obs, last_hid):
            return self._fused_policy(obs, last_hid, need_hidden=not means_grad_only)
        if means_grad_only and self._fused_policy_train_ok(obs, last_hid):
            ag = self.policy_dicts[0]
            means = _PolicyTrunk.apply(obs.reshape(b * n, o), last_hid.reshape(b * n, -1), n, self.id_dim, ag.layernorm.eps,
                                       ag.fc1.weight, ag.fc1.bias, ag.layernorm.weight, ag.layernorm.bias, ag.rnn.weight_ih, ag.rnn.weight_hh,
                                       ag.rnn.bias_ih, ag.rnn.bias_hh, ag.fc2.weight, ag.fc2.bias).view(b, n, 1)
            return means, torch.full_like(means, math.log(self.args.fixed_policy_std)), None
        if self.args.shared_params:
            ag = self.policy_dicts[0]
            means, hid = ag.trunk(self._shared_agent_first_layer(ag, obs).reshape(b * n, -1), last_hid)
            means, hid = means.view(b, n, -1), hid.view(b, n, -1)
            log_stds = torch.full_like(means, math.log(self.args.fixed_policy_std))       # model.py:119-120
        else:
            ms, hs = [], []
            for i, ag in enumerate(self.policy_dicts):
                w = ag.fc1.weight
                x = F.linear(obs[:, i], w[:, :o], ag.fc1.bias)
                if self.args.agent_id:
                    x = x + w[:, o + i]
                m, h = ag.trunk(x, last_hid[:, i])
                ms.append(m); hs.append(h)
            means, hid = torch.stack(ms, 1), torch.stack(hs, 1)
            log_stds = torch.zeros_like(means)                            # model.py:134-135
        return means, log_stds, hid

    def _shared_agent_first_layer(self, ag, obs: torch.Tensor) -> torch.Tensor:
        """fc1 of the shared agent on [obs | one-hot id] as W_obs obs + b1 + id column: [b, n, h]"""
        b, n, o = obs.shape[0], self.n_, self.obs_dim
        w = ag.fc1.weight
        if _tall_ok(obs, b * n, w):                                  # (the policy update on a replay batch: weight gradient over b * n rows)
            x = _TallLinear.apply(obs.reshape(b * n, o), w[:, :o], ag.fc1.bias).view(b, n, -1)
        else:
            x = F.linear(obs, w[:, :o], ag.fc1.bias)                 # observation columns
        if self.args.agent_id:
            x = x + w[:, o:].t().unsqueeze(0)                        # one-hot id i selects column o + i
        return x

    # ---- critics ---------------------------------------------------------------------------------
    def value(self, obs: torch.Tensor, act: torch.Tensor, own_action_only: bool = False) -> torch.Tensor:
        """obs [b, n, o], act [b, n, a] -> [b, n, 1].  own_action_only: the caller differentiates with respect to `act` alone (the policy
        loss): the central critic may then skip the gradients of its own parameters, which the policy optimiser never reads."""
        if self.alg == "iddpg":
            return self._value_independent(obs, act)
        if self.alg == "coma":
            return self._value_coma(obs, act)
        if self.alg == "matd3" and not own_action_only:            # matd3.py:86: [2b, n, 1] = values1 over values2
            return torch.cat(self._value_twin(obs, act), 0)
        return self._value_central(obs, act, own_action_only)      # (MATD3's policy loss reads the first head only — flag column times 0)

    def _independent_first_layer(self, cr, obs, act):
        """IDDPG's shared critic, first layer on [obs_i | id_i | act_i] (iddpg.py:32-58) as  W_obs obs + id column + W_act act, [b, n, h];
        on a tall GPU batch the observation product takes _TallLinear (its weight gradient is a [h, o] product with b * n rows of
        reduction, which the BLAS back end runs on two workgroups)"""
        b, n, o, ids = obs.shape[0], self.n_, self.obs_dim, self.id_dim
        w = cr.fc1.weight
        if _tall_ok(obs, b * n, w):
            x = _TallLinear.apply(obs.reshape(b * n, o), w[:, :o], cr.fc1.bias)
            if self.act_dim == 1:        # a one-column product is an outer product: one fused multiply-add pass instead of a GEMM + an add
                x = torch.addcmul(x, act.reshape(b * n, 1), w[:, o + ids:].t()).view(b, n, -1)
            else:
                x = (x + _TallLinear.apply(act.reshape(b * n, -1), w[:, o + ids:], None)).view(b, n, -1)
        else:
            x = F.linear(obs, w[:, :o], cr.fc1.bias) + F.linear(act, w[:, o + ids:])
        if ids:
            x = x + w[:, o:o + n].t().unsqueeze(0)
        return x

    def _value_independent(self, obs, act):
        """IDDPG (iddpg.py:32-58): critic input [obs_i | id_i | act_i]"""
        b, n, o, ids = obs.shape[0], self.n_, self.obs_dim, self.id_dim

        def first_layer(cr, ob, ac, who):
            w = cr.fc1.weight
            x = F.linear(ob, w[:, :o], cr.fc1.bias) + F.linear(ac, w[:, o + ids:])
            if ids:
                x = x + (w[:, o:o + n].t().unsqueeze(0) if who is None else w[:, o + who])
            return x

        if self.args.shared_params:
            cr = self.value_dicts[0]
            v, _ = cr.trunk(self._independent_first_layer(cr, obs, act).reshape(b * n, -1))
            return v.view(b, n, -1)
        return torch.stack([cr.trunk(first_layer(cr, obs[:, i], act[:, i], i))[0] for i, cr in enumerate(self.value_dicts)], 1)

    def _central_first_layer(self, cr, obs_all, act_all, own, who, obs_term=None):
        """first layer of a central critic (maddpg.py:35-79, matd3.py:35-69 with the flag column at 0) = W_obs·obs_all + b1 + W_id[:, i]
        + W_act·act_all, where the joint action enters detached and agent i's own (act_i - act_i.detach()) — zero in value — restores
        its gradient path; [b, n, h] for who None, [b, h] for agent `who`.  obs_term: W_obs·obs_all + b1 when the caller holds it."""
        b, n, o, a, ids = obs_all.shape[0], self.n_, self.obs_dim, self.act_dim, self.id_dim
        w = cr.fc1.weight
        w_act = w[:, n * o + ids:n * o + ids + n * a]
        base = (F.linear(obs_all, w[:, :n * o], cr.fc1.bias) if obs_term is None else obs_term) + F.linear(act_all.detach(), w_act)      # [b, h]
        if who is None:                                              # all agents at once: [b, n, h]
            x = base.unsqueeze(1)
            if ids:
                x = x + w[:, n * o:n * o + n].t().unsqueeze(0)
            else:
                x = x.expand(b, n, -1)
            if own is not None:
                x = x + torch.einsum("bna,hna->bnh", own, w_act.reshape(-1, n, a))
            return x
        x = base + w[:, n * o + who] if ids else base
        if own is not None:
            x = x + F.linear(own[:, who], w_act[:, who * a:(who + 1) * a])
        return x

    def _value_central(self, obs, act, own_action_only=False):
        """MADDPG (maddpg.py:35-79): agent i's critic sees [all obs | id_i | all actions] and only its OWN
        action carries gradient.  First layer = W_obs·obs_all + W_id[:, i] + W_act·act_all, where the joint
        action enters detached and agent i's own (act_i - act_i.detach()) — zero in value — restores its
        gradient path; no [b, n, n·o] tensor is ever built."""
        b, n, o, a, ids = obs.shape[0], self.n_, self.obs_dim, self.act_dim, self.id_dim
        obs_all, act_all = obs.reshape(b, n * o), act.reshape(b, n * a)
        own = (act - act.detach()) if act.requires_grad else None
        na = n * o + ids + n * a                                         # end of the action columns (MATD3: the flag column follows)

        def first_layer(cr, who):
            return self._central_first_layer(cr, obs_all, act_all, own, who)

        if self.args.shared_params:
            cr = self.value_dicts[0]
            if ids and cr.use_ln and own is not None and a == 1 and own_action_only and critic_head_ok(cr, obs_all.new_empty(0, 64), b * n, n):
                # the policy update (maddpg.py:52-58, 103-125): value = the head on base[b] + id_column[i] (the own-action term is zero in
                # value), gradient = d/d act[b, i] only, from the kernel; the critic's own parameters are not differentiated
                w = cr.fc1.weight.detach()
                with torch.no_grad():
                    base = F.linear(obs_all, w[:, :n * o], cr.fc1.bias.detach()) + F.linear(act_all.detach(), w[:, n * o + ids:na])
                v = _CriticHeadOwnAction.apply(act, base, w[:, n * o:n * o + n].t(), w[:, n * o + ids:na].t(), *head_params(cr))
                return v.view(b, n, 1)
            if ids and own is None and cr.use_ln:
                # no gradient path through the actions (value loss, target values): the first layer's output is base[b] + id_column[i] —
                # LayerNorm + ReLU straight from the two small operands, the [b, n, h] sum is never written
                w = cr.fc1.weight
                base = tall_linear_w(obs_all, w[:, :n * o], cr.fc1.bias) + tall_linear_w(act_all.detach(), w[:, n * o + ids:na])
                if critic_head_ok(cr, base, b * n, n):
                    return critic_head(cr, base, w[:, n * o:n * o + n].t()).view(b, n, 1)
                xn = layernorm_act_bc(cr.layernorm, cr.act, base, w[:, n * o:n * o + n].t())
                if xn is not None:
                    return cr.head(xn)[0].view(b, n, 1)
            v, _ = cr.trunk(first_layer(cr, None).reshape(b * n, -1))
            return v.view(b, n, 1)
        return torch.stack([cr.trunk(first_layer(cr, i))[0] for i, cr in enumerate(self.value_dicts)], 1)

    def _value_twin(self, obs, act, want="both", obs_term=None):
        """MATD3 (matd3.py:35-86): the central critic valued twice, its input one column wider — 0 for values1, 1 for values2 —, i.e.
        first layer = that of _value_central, and the same + fc1.weight[:, -1].  Returns (values1, values2), each [b, n, 1], or with
        want="min" their minimum (matd3.py:141-142).  obs_term [b, h]: W_obs·obs_all + b1 of the shared critic when the caller holds it
        (PGTrainer caches it per update round).  Without a gradient path the default critic on the GPU takes ONE launch for both heads."""
        b, n, o, a, ids = obs.shape[0], self.n_, self.obs_dim, self.act_dim, self.id_dim
        obs_all, act_all = obs.reshape(b, n * o), act.reshape(b, n * a)
        own = (act - act.detach()) if act.requires_grad else None
        out = (lambda v1, v2: torch.minimum(v1, v2)) if want == "min" else (lambda v1, v2: (v1, v2))
        if self.args.shared_params:
            cr = self.value_dicts[0]
            w = cr.fc1.weight
            flag = w[:, -1]
            if ids and own is None and cr.use_ln:
                w_act = w[:, n * o + ids:n * o + ids + n * a]
                base = (tall_linear_w(obs_all, w[:, :n * o], cr.fc1.bias) if obs_term is None else obs_term) + tall_linear_w(act_all.detach(), w_act)
                per_n = w[:, n * o:n * o + n].t()
                if not (torch.is_grad_enabled() and (base.requires_grad or w.requires_grad)) and critic_twin_ok(cr, base, b * n, n):
                    if want == "min":
                        return critic_twin_forward(cr, base, per_n, flag, ("vmin",))["vmin"].view(b, n, 1)
                    r = critic_twin_forward(cr, base, per_n, flag, ("v1", "v2"))
                    return r["v1"].view(b, n, 1), r["v2"].view(b, n, 1)
                if critic_head_ok(cr, base, b * n, n):
                    return out(critic_head(cr, base, per_n).view(b, n, 1), critic_head(cr, base, per_n + flag).view(b, n, 1))
            x = self._central_first_layer(cr, obs_all, act_all, own, None, obs_term)
            return out(cr.trunk(x.reshape(b * n, -1))[0].view(b, n, 1), cr.trunk((x + flag).reshape(b * n, -1))[0].view(b, n, 1))
        xs = [self._central_first_layer(cr, obs_all, act_all, own, i) for i, cr in enumerate(self.value_dicts)]
        return out(torch.stack([cr.trunk(x)[0] for x, cr in zip(xs, self.value_dicts)], 1),
                   torch.stack([cr.trunk(x + cr.fc1.weight[:, -1])[0] for x, cr in zip(xs, self.value_dicts)], 1))

    def value_mse(self, obs, act, returns, valid=None):
        """mean over (batch, agent) of (returns - Q(obs, act))^2 — the value loss of maddpg.py:122-124 / ddpg.py:36-38 — weighted by
        `valid` [b] when given (1 everywhere = the reference).  With the default critic on the GPU the loss and its gradients come out of
        ONE head launch (_CriticHeadMSE); otherwise value() + the plain expression."""
        b, n, o = obs.shape[0], self.n_, self.obs_dim
        a, ids = self.args, self.id_dim
        if (a.shared_params and torch.is_grad_enabled() and not act.requires_grad and obs.is_cuda
                and os.environ.get("MAPDN_FUSED_MSE", "1") != "0"):
            cr = self.value_dicts[0]
            w = cr.fc1.weight
            x = per_n = None
            if self.alg in ("maddpg", "matd3") and ids and cr.use_ln:
                x = tall_linear_w(obs.reshape(b, n * o), w[:, :n * o], cr.fc1.bias) \
                    + tall_linear_w(act.reshape(b, n * self.act_dim), w[:, n * o + ids:n * o + ids + n * self.act_dim])
                per_n = w[:, n * o:n * o + n].t()
            elif self.alg == "iddpg":
                x = self._independent_first_layer(cr, obs, act).reshape(b * n, -1)
            elif self.alg == "coma" and cr.use_ln:                 # coma.py:179-180: the same loss on rows that are read, as IDDPG's
                x = self._coma_first_layer(cr, obs, act).reshape(b * n, -1)
            twin = self.alg == "matd3"
            if x is not None and (critic_twin_ok(cr, x, b * n, n) if twin else critic_head_ok(cr, x, b * n, n if per_n is not None else 0)):
                if valid is None:
                    scale, wrow = x.new_full((1,), 1.0 / (b * n)), None
                else:
                    vf = valid.float().view(-1)
                    scale = (1.0 / (vf.sum().clamp(min=1.0) * n)).reshape(1)
                    wrow = vf if per_n is not None else vf.repeat_interleave(n)
                if twin and os.environ.get("MAPDN_TWIN_MSE_KERNEL", "0") == "1":      # both heads in ONE launch: measured slower than the pair below
                    return _CriticTwinMSE.apply(x, per_n, w[:, -1], *head_params(cr), returns, wrow, scale)
                if twin:
                    # matd3.py:143-150, both heads against the same returns: two single-head loss launches, on per_n and on per_n + w_flag,
                    # each with half the weight; autograd sums the two dbase and hands the second dper_n's column sum to w_flag
                    twin_pair_mse.launches += 1
                    head = (*head_params(cr), returns, wrow, 0.5 * scale)
                    return _CriticHeadMSE.apply(x, per_n, *head) + _CriticHeadMSE.apply(x, per_n + w[:, -1], *head)
                return _CriticHeadMSE.apply(x, per_n, *head_params(cr), returns, wrow, scale)
        wm = _wmean(valid)
        if self.alg == "matd3":                          # matd3.py:143-150
            v1, v2 = self._value_twin(obs, act)
            return 0.5 * (wm((returns - v1.view(-1, n)).pow(2)) + wm((returns - v2.view(-1, n)).pow(2)))
        values = self.value(obs, act).view(-1, n)
        return wm((returns - values).pow(2))

    # ---- action selection (maddpg.py:81-101 == iddpg.py:60-80; utilities/util.py:52-98) ----------
    def get_actions(self, state, status, exploration, actions_avail, target=False, last_hid=None, means_grad_only=False, clip=False, noise=None):
        net = self.target_net if (target and self.args.target) else self
        means, log_stds, hiddens = net.policy(state, last_hid, means_grad_only)
        if means.size(-1) > 1:                                   # maddpg.py:85-87 (action_dim > 1 sums over agents)
            means_, log_stds_ = means.sum(dim=1, keepdim=True), log_stds.sum(dim=1, keepdim=True)
        else:
            means_, log_stds_ = means, log_stds
        actions, log_prob = self._select_action(means_, log_stds_, status, exploration, clip, noise)
        restore_mask = 1.0 - (actions_avail == 0).to(actions.dtype)
        return actions, restore_mask * actions, log_prob, (means, log_stds), hiddens

    def _select_action(self, mean, log_std, status, exploration, clip=False, noise=None):
        """utilities/util.py:52-87.  clip (matd3.py:119-124 passes True for the next actions) is read ONLY without action_enforcebound: the
        bounded branch ignores it (util.py:58-66), as the reference does.  noise: the standard-normal draw to use instead of drawing."""
        a = self.args
        draw = (lambda: torch.randn_like(mean)) if noise is None else (lambda: noise.to(mean.dtype).view_as(mean))
        if status == "train":
            if not exploration:
                return mean, None
            std = log_std.exp()
            if a.action_enforcebound:                            # util.py:57-66
                x_t = mean + std * draw()                        # Normal(mean, std).rsample()
                y_t = torch.tanh(x_t)
                log_prob = -((x_t - mean) ** 2) / (2 * std ** 2) - log_std - math.log(math.sqrt(2 * math.pi))
                return y_t, log_prob - torch.log(1 - y_t.pow(2) + 1e-6)
            x_t = std * draw()                                   # util.py:67-76
            log_prob = -(x_t ** 2) / (2 * std ** 2) - log_std - math.log(math.sqrt(2 * math.pi))
            if clip:
                return mean + torch.clamp(x_t, min=-a.clip_c, max=a.clip_c), log_prob
            return mean + x_t, log_prob
        if status == "test":                                     # util.py:80-87
            return (torch.tanh(mean) if a.action_enforcebound else mean), None
        raise ValueError(status)

    # ---- loss (models/maddpg.py:103-125 == learning_algorithms/ddpg.py:15-39) ----------------------
    def normalise_reward(self, reward: torch.Tensor) -> torch.Tensor:
        """model.py:316-317: BatchNorm1d over the batch, per agent.  Data-parallel ranks (PGTrainer sets `_dp_all_reduce`) normalise with
        the statistics of the UNION of their batches — one small all-reduce of (count, sum, sum of squares) — so that an N-rank update
        equals the one-rank update on the concatenated batch and the running statistics stay identical on every replica."""
        if not self.args.reward_normalisation:
            return reward
        return self._union_batchnorm(self.batchnorm, reward)

    def _union_batchnorm(self, bn: nn.BatchNorm1d, reward: torch.Tensor) -> torch.Tensor:
        """bn(x) for x [batch, n]; in training mode under data-parallel training with the statistics of the union of the ranks' batches
        (see normalise_reward).  MAPPO / IPPO's advantage BatchNorm goes through it as well."""
        red = self.__dict__.get("_dp_all_reduce")
        if red is None or not bn.training:
            return bn(reward)
        x = reward.double()
        st = torch.cat((x.new_full((1,), float(x.shape[0])), x.sum(0), (x * x).sum(0)))
        red(st)
        cnt, n = st[0], x.shape[1]
        mean = st[1:1 + n] / cnt
        var = (st[1 + n:] / cnt - mean * mean).clamp(min=0.0)                      # biased, as BatchNorm normalises with
        with torch.no_grad():
            m = bn.momentum if bn.momentum is not None else 0.1
            bn.running_mean.mul_(1 - m).add_(m * mean.to(bn.running_mean.dtype))
            bn.running_var.mul_(1 - m).add_(m * (var * cnt / (cnt - 1).clamp(min=1.0)).to(bn.running_var.dtype))
            bn.num_batches_tracked += 1
        y = (reward - mean.to(reward.dtype)) * torch.rsqrt(var.to(reward.dtype) + bn.eps)
        return y * bn.weight + bn.bias

    def smoothed_actions(self, means: torch.Tensor, avail: torch.Tensor, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """MATD3's next actions from the next-state policy means (matd3.py:119-124: exploration=True, clip=True — see _select_action for
        what clip does), with the restore mask of get_actions; one [bs, n, 1] draw unless `noise` is given"""
        assert means.size(-1) == 1, "one action per agent (get_actions sums wider means and log_stds over the agents: not built here)"
        log_std = torch.full_like(means, math.log(self.args.fixed_policy_std)) if self.args.shared_params else torch.zeros_like(means)
        actions, _ = self._select_action(means, log_std, "train", True, True, noise)
        return (1.0 - (avail == 0).to(actions.dtype)) * actions

    def _matd3_next_values(self, batch: Batch) -> torch.Tensor:
        """min(Q1', Q2') of the target critic at the smoothed next actions (matd3.py:119-142).  The noise is drawn anew in every call, after
        the noise-free policy forward; batch["next_noise"] [bs, n, 1] replaces the draw.  PGTrainer hands over what does not change within
        an update round: the policy means (next_mean_cached) and the target critic's observation term (next_obs_term_cached)."""
        pol = self if self.args.double_q else (self.target_net if self.args.target else self)
        means = batch["next_mean_cached"] if "next_mean_cached" in batch else pol.policy(batch["next_state"], batch["hid"], True)[0]
        next_actions = self.smoothed_actions(means, batch["action_avail"], batch.get("next_noise"))
        return self.target_net._value_twin(batch["next_state"], next_actions, "min", batch.get("next_obs_term_cached"))

    def _unpack(self, batch: Batch):
        """what every get_loss starts from: the `unpack_data` tensors (model.py:304-319) with the rewards through `batchnorm` (model.py:316-317),
        done as [bs, 1] floats, `valid` or None and the mean it weights"""
        valid = batch.get("valid")
        return (batch["state"], batch["action"], batch["next_state"], batch["action_avail"], batch["last_hid"], batch["hid"],
                self.normalise_reward(batch["reward"].float()), batch["done"].float().view(-1, 1), valid, _wmean(valid))

    def get_loss(self, batch: Batch, want=("policy", "value")):
        """batch: state/next_state [bs, n, o], action/action_avail [bs, n, a], reward [bs, n], done [bs, 1],
        last_hid/hid [bs, n, h] float32 (the `unpack_data` tensors, model.py:304-319); optional `valid`
        [bs] weights the means (1 everywhere = the reference); MATD3: optional `next_noise` [bs, n, 1] (see _matd3_next_values); COMA:
        optional `cf_noise` [S, bs, n, a] (see _coma_policy_loss; its loss is coma.py:128-191, the value half shared with the others).  Returns (policy_loss, value_loss,
        (means, log_stds)); a loss not in `want` is None and its forward passes are skipped."""
        n = self.n_
        state, actions, next_state, avail, last_hid, hid, rewards, done, valid, wmean = self._unpack(batch)
        policy_loss = value_loss = action_out = None
        if self.alg == "coma":
            policy_loss, action_out = self._coma_policy_loss(batch, wmean, "policy" in want)
        elif "policy" in want:
            _, actions_pol, _, action_out, _ = self.get_actions(state, "train", False, avail, False, last_hid, means_grad_only=True)
            advantages = self.value(state, actions_pol, own_action_only=True).view(-1, n)
            if self.args.normalize_advantages:
                advantages = self._adv_batchnorm.to(advantages.device)(advantages)
            policy_loss = wmean(-advantages)
        elif self.alg == "matd3" and self.args.normalize_advantages and self.batchnorm.training:
            # the reference evaluates BOTH losses in every get_loss call (matd3.py:113-151), so with normalize_advantages its `batchnorm`
            # — part of the state_dict — sees the advantages in the value updates too: keep its running statistics the reference's
            with torch.no_grad():
                _, a_pol, _, _, _ = self.get_actions(state, "train", False, avail, False, last_hid, means_grad_only=True)
                self._adv_batchnorm.to(a_pol.device)(self.value(state, a_pol, own_action_only=True).view(-1, n))
        if "value" in want:
            with torch.no_grad():
                if self.alg == "matd3":
                    next_values = self._matd3_next_values(batch).view(-1, n)
                elif "next_value_cached" in batch:                 # PGTrainer precomputed both for the whole replay ring (same values)
                    next_values = batch["next_value_cached"].view(-1, n)
                else:
                    if "next_action_cached" in batch:
                        next_actions = batch["next_action_cached"]
                    else:
                        _, next_actions, _, _, _ = self.get_actions(next_state, "train", False, avail,
                                                                    not self.args.double_q, hid)
                    next_values = self.target_net.value(next_state, next_actions).view(-1, n)
                returns = rewards + self.args.gamma * (1 - done) * next_values
            value_loss = self.value_mse(state, actions, returns, valid)
        return policy_loss, value_loss, action_out
