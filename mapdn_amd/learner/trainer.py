"""`PGTrainer` (utilities/trainer.py) with the rollout / update schedule of models/model.py for a batch of envs; data-parallel ranks
average gradients through one flat RCCL all-reduce per update."""

import math
import os
from typing import Optional

import torch
import torch.nn.functional as F

from ..replay import TransReplayBuffer
from ._hip import launch
from .args import Batch
from .coma import COMANet
from .ddpg import DDPGNet
from .maac import MAACNet
from .ppo import PPONet
from .sqddpg import SQDDPGNet


def net_class(alg: str):
    """the module class of an algorithm name (models/model_registry.py:14-25); KeyError for a name that is not built"""
    for c in (DDPGNet, COMANet, MAACNet, SQDDPGNet, PPONet):
        if alg in c.ALGS:
            return c
    raise KeyError(alg)


def normal_entropy(log_stds: torch.Tensor) -> torch.Tensor:
    """Normal(mean, std).entropy().mean() (utilities/util.py:37-38)"""
    return (0.5 + 0.5 * math.log(2 * math.pi) + log_stds).mean()


class PGTrainer:
    """`PGTrainer` (utilities/trainer.py:9-108) + the rollout/update schedule of `Model.train_process`,
    `transition_update` and `evaluation` (models/model.py:39-70,197-302) for a batch of B envs.

    One `run()` is one episode of every env.  `steps` counts batched steps, so with B == 1 the update
    schedule is the reference's; with B envs each update still draws `batch_size` transitions (a
    contiguous window of the (step, env)-ordered replay, see mapdn_amd/replay.py).  With
    torch.distributed initialised, gradients are averaged over ranks (one flat all-reduce per
    update) before clipping, so every rank applies the same step to identical replicas."""

    def __init__(self, args, alg: str, env, device=None, data_parallel: Optional[bool] = None):
        self.args, self.env = args, env
        self.device = torch.device(device if device is not None else getattr(env, "device", "cpu"))
        Net = net_class(alg)
        target = Net(args, alg).to(self.device) if args.target else None
        self.behaviour_net = Net(args, alg, target).to(self.device)
        self.replay_buffer = TransReplayBuffer(int(args.replay_buffer_size), device=self.device, window=int(args.batch_size))   # windows are views
        rms = dict(alpha=0.99, eps=1e-5)                                                   # trainer.py:26-27
        self.policy_optimizer = torch.optim.RMSprop(self.behaviour_net.policy_dicts.parameters(), lr=args.policy_lrate, **rms)
        self.value_optimizer = torch.optim.RMSprop(self.behaviour_net.value_dicts.parameters(), lr=args.value_lrate, **rms)
        self.steps = 0
        self.episodes = 0
        self.entr = args.entr
        import torch.distributed as dist
        self._dist = dist if (data_parallel if data_parallel is not None else (dist.is_available() and dist.is_initialized())) else None
        self.collectives = {"broadcast": 0, "all_reduce_grads": 0, "all_reduce_flag": 0, "all_reduce_reward_stats": 0}   # issued so far
        if self._dist is not None:
            def _bn_reduce(t):
                self._collective(self._dist.all_reduce, t)
                self.collectives["all_reduce_reward_stats"] += 1
            self.behaviour_net.__dict__["_dp_all_reduce"] = _bn_reduce
        self.on_policy = alg in ("coma", "mappo", "ippo")         # models/model.py:53-56: the ring is emptied after every update round
        self.ppo = isinstance(self.behaviour_net, PPONet)
        if self.ppo and env is not None:
            # rows enter the ring in (step, env) order, n_envs per insertion: row i + n_envs is the same env one step later, wherever a
            # sampled window starts — the GAE chain stride (PPONet)
            self.behaviour_net.__dict__["gae_stride"] = int(env.n_envs)
        if self._dist is not None:                               # identical replicas to start from
            for t in self.behaviour_net.state_dict().values():
                self._collective(self._dist.broadcast, t, src=0)
                self.collectives["broadcast"] += 1

    def _collective(self, fn, t: torch.Tensor, **kw):
        """fn(t, **kw) in place.  RCCL ("nccl") takes the device tensor as it is; any other backend (gloo: the CPU / one-GPU pre-flight of
        the N-rank path) gets a host copy and the result is written back."""
        if t.is_cuda and self._dist.get_backend() != "nccl":
            h = t.detach().cpu()
            fn(h, **kw)
            t.copy_(h)
        else:
            fn(t, **kw)

    # ---- one optimiser step (trainer.py:73-98) ---------------------------------------------------
    def _all_reduce_grads(self, params):
        if self._dist is None:
            return
        grads = [p.grad for p in params if p.grad is not None]
        flat = torch.cat([g.reshape(-1) for g in grads])
        self._collective(self._dist.all_reduce, flat)
        self.collectives["all_reduce_grads"] += 1
        flat /= self._dist.get_world_size()
        off = 0
        for g in grads:
            g.copy_(flat[off:off + g.numel()].view_as(g)); off += g.numel()

    def replica_fingerprint(self) -> torch.Tensor:
        """[2] float64: (sum of every state_dict value, sum of their bit patterns read as integers) — equal on every rank exactly when the
        replicas are (bit-)identical, which data-parallel training must keep them (same broadcast start, same averaged gradients, same
        optimiser arithmetic).  replicas_identical() gathers and compares it."""
        tot, bits = torch.zeros((), dtype=torch.float64, device=self.device), torch.zeros((), dtype=torch.float64, device=self.device)
        for v in self.behaviour_net.state_dict().values():
            if v.dtype == torch.float32:
                tot += v.double().sum(); bits += v.contiguous().view(torch.int32).double().sum()
            else:
                tot += v.double().sum(); bits += v.double().sum()
        return torch.stack((tot, bits))

    def replicas_identical(self) -> bool:
        if self._dist is None:
            return True
        fp = self.replica_fingerprint()
        world = self._dist.get_world_size()
        mine = fp if self._dist.get_backend() == "nccl" else fp.cpu()
        out = [torch.empty_like(mine) for _ in range(world)]
        self._dist.all_gather(out, mine)
        return all(torch.equal(o, out[0]) for o in out)

    def _apply(self, optimizer, loss, stat, key):
        optimizer.zero_grad()
        loss.backward()
        params = optimizer.param_groups[0]["params"]
        self._all_reduce_grads(params)
        norm = torch.nn.utils.clip_grad_norm_(params, self.args.grad_clip_eps)          # util.py:161-163
        optimizer.step()
        stat[f"mean_train_{key}_grad_norm"] = norm
        stat[f"mean_train_{key}_loss"] = loss.detach()

    def value_transition_process(self, stat, batch: Batch):
        _, value_loss, _ = self.behaviour_net.get_loss(batch, want=("value",))
        self._apply(self.value_optimizer, value_loss, stat, "value")

    def policy_transition_process(self, stat, batch: Batch):
        policy_loss, _, (means, log_stds) = self.behaviour_net.get_loss(batch, want=("policy",))
        stat["mean_train_policy_loss_raw"] = policy_loss.detach()
        if self.entr > 0:                                        # trainer.py:39-49
            entropy = normal_entropy(log_stds)
            policy_loss = policy_loss - self.entr * entropy
            stat["mean_train_entropy"] = entropy.detach()
        self._apply(self.policy_optimizer, policy_loss, stat, "policy")

    # ---- optional per-phase device timing of an episode (examples/train_ddpg.py --phases): CUDA events on the current stream around
    # replay insertion, batch sampling, the value / policy updates and the target update; the rollout is the rest of the episode
    profile_phases = False

    class _Phase:
        def __init__(self, trainer, name):
            self.t, self.name = trainer, name

        def __enter__(self):
            if self.t.profile_phases and self.t.device.type == "cuda":
                self.a = torch.cuda.Event(enable_timing=True); self.b = torch.cuda.Event(enable_timing=True)
                self.a.record()
            return self

        def __exit__(self, *exc):
            if self.t.profile_phases and self.t.device.type == "cuda":
                self.b.record()
                self.t._phase_events.append((self.name, self.a, self.b))

    def _phase(self, name):
        if not hasattr(self, "_phase_events"):
            self._phase_events = []
        return PGTrainer._Phase(self, name)

    def phase_seconds(self):
        """{phase: seconds} accumulated since the last call (synchronises); empty unless profile_phases"""
        out = {}
        ev = getattr(self, "_phase_events", [])
        if ev:
            torch.cuda.synchronize(self.device)
            for name, a, b in ev:
                out[name] = out.get(name, 0.0) + a.elapsed_time(b) * 1e-3
            ev.clear()
        return out

    def value_replay_process(self, stat):
        with self._phase("sample"):
            batch = self.replay_buffer.get_batch(self.args.batch_size)
        with self._phase("value_update"):
            self.value_transition_process(stat, batch)

    def policy_replay_process(self, stat):
        with self._phase("sample"):
            batch = self.replay_buffer.get_batch(self.args.batch_size)
        with self._phase("policy_update"):
            self.policy_transition_process(stat, batch)

    def _cache_targets(self) -> bool:
        """The value loss needs pi(next_state) and Q_target(next_state, pi(next_state)) of every sampled transition (maddpg.py:103-125).
        The value epochs of one update round (models/model.py:46-49: ten of them) train the behaviour CRITIC only: neither the policy
        that produces those actions nor the target critic that values them changes between the epochs, and their windows overlap
        heavily (32 of the ring's 64 steps each).  Both are therefore computed ONCE for the whole ring, in chunks of one batch — the
        same kernels on the same inputs as the per-epoch passes, same values — and handed out with the sampled windows as two more
        (temporary) fields of the replay store.  Only when that is the cheaper order: a ring longer than the transitions the round's
        value epochs sample (the reference's own defaults: a 5000-transition ring against 10 x 32) keeps the per-epoch passes.
        MAPDN_CACHE_NEXT_ACTIONS=0 disables it.
        MATD3's target is NOT constant over the round: it values tanh(mean + std·eps) with eps drawn anew in every get_loss call
        (matd3.py:119-142), so no action and no value is cached — one draw would otherwise serve every epoch that samples the transition.
        Cached is what is deterministic: the next-state policy MEANS and, for the shared critic, the target's observation term
        W_obs·next_obs_all + b1 ([ring, h]; the K = n·o product is the expensive part of the target's first layer).  The smoothed action,
        the K = n action term and the twin head are formed per epoch (DDPGNet._matd3_next_values)."""
        rb, net, a = self.replay_buffer, self.behaviour_net, self.args
        if not isinstance(rb, TransReplayBuffer) or os.environ.get("MAPDN_CACHE_NEXT_ACTIONS", "1") == "0" or len(rb) == 0:
            return False
        if net.alg == "maac":              # MAAC's target values the next actions DRAWN in every get_loss call (maac.py:98-102): nothing is cached
            return False
        if net.alg == "sqddpg":            # SQDDPG's target is valued on coalitions DRAWN in every get_loss call (sqddpg.py:145): nothing is cached
            return False
        if self.ppo:                       # MAPPO / IPPO read no target net and no next action (ppo.py:16-71): nothing to cache
            return False
        st = rb.store
        if not all(k in st for k in ("next_state", "action_avail", "hid", "action")):
            return False
        n_ring = rb.size if len(rb) == rb.size else len(rb)      # (the ring fills from position 0: a partly filled ring is [0, len))
        if n_ring > int(a.value_update_epochs) * int(a.batch_size):
            return False
        if net.alg == "matd3":
            return self._cache_matd3(n_ring)
        cache = torch.empty_like(st["action"])
        values = torch.empty(st["action"].shape[0], net.n_, dtype=torch.float32, device=cache.device) if a.target else None
        chunk = max(int(a.batch_size), 1)
        with torch.no_grad():
            for lo in range(0, n_ring, chunk):
                hi = min(lo + chunk, n_ring)
                _, na, _, _, _ = net.get_actions(st["next_state"][lo:hi], "train", False, st["action_avail"][lo:hi], not a.double_q, st["hid"][lo:hi],
                                                 means_grad_only=True)          # (only the actions are read: the new hidden state is not stored)
                cache[lo:hi] = na
                if values is not None:
                    values[lo:hi] = net.target_net.value(st["next_state"][lo:hi], na).view(-1, net.n_)
            if rb.window:
                m = min(rb.window, n_ring)
                cache[rb.size:rb.size + m] = cache[:m]
                if values is not None:
                    values[rb.size:rb.size + m] = values[:m]
        st["next_action_cached"] = cache
        if values is not None:
            st["next_value_cached"] = values
        return True

    def _cache_matd3(self, n_ring: int) -> bool:
        rb, net, a = self.replay_buffer, self.behaviour_net, self.args
        st = rb.store
        pol = net if a.double_q else (net.target_net if a.target else net)
        tgt = net.target_net
        means = torch.empty_like(st["action"])
        cr = tgt.value_dicts[0]
        term = torch.empty(st["action"].shape[0], cr.fc1.out_features, dtype=cr.fc1.weight.dtype, device=means.device) if a.shared_params else None
        chunk, no = max(int(a.batch_size), 1), net.n_ * net.obs_dim
        with torch.no_grad():
            for lo in range(0, n_ring, chunk):
                hi = min(lo + chunk, n_ring)
                means[lo:hi] = pol.policy(st["next_state"][lo:hi], st["hid"][lo:hi], True)[0]
                if term is not None:
                    term[lo:hi] = F.linear(st["next_state"][lo:hi].reshape(hi - lo, no), cr.fc1.weight[:, :no], cr.fc1.bias)
            if rb.window:
                m = min(rb.window, n_ring)
                means[rb.size:rb.size + m] = means[:m]
                if term is not None:
                    term[rb.size:rb.size + m] = term[:m]
        st["next_mean_cached"] = means
        if term is not None:
            st["next_obs_term_cached"] = term
        return True

    def transition_update(self, trans: Batch, stat):
        """models/model.py:39-70 with replay=True, mixer=False"""
        a = self.args
        with self._phase("replay_insert"):
            self.replay_buffer.add_experience(trans)
        if self.steps > a.replay_warmup and len(self.replay_buffer) >= a.batch_size and self.steps % a.behaviour_update_freq == 0:
            cached = a.value_update_epochs > 1 and self._cache_targets()
            try:
                for _ in range(a.value_update_epochs):
                    self.value_replay_process(stat)
            finally:
                if cached:
                    for k in ("next_action_cached", "next_value_cached", "next_mean_cached", "next_obs_term_cached"):
                        self.replay_buffer.store.pop(k, None)
            for _ in range(a.policy_update_epochs):
                self.policy_replay_process(stat)
            if self.on_policy:                                   # COMA, MAPPO, IPPO: the ring is emptied after every update round (model.py:53-56)
                self.replay_buffer.clear()
        if a.target and self.steps % a.target_update_freq == 0:
            with self._phase("target_update"):
                self.behaviour_net.update_target()

    # ---- rollouts (models/model.py:197-302): episodes run through the package's one rollout loop (rollout.BatchedRollout) ----
    def _episode(self, stat, train: bool):
        env, net, a = self.env, self.behaviour_net, self.args
        B, dv = env.n_envs, self.device
        prefix = "mean_train_" if train else "mean_test_"
        avail = env.get_avail_actions().to(dv)

        # (MAPPO / IPPO store the log-probability of the taken action, which the one-launch exploration sample does not produce)
        fused_explore = (train and self.device.type == "cuda" and a.action_dim == 1 and a.continuous and not a.gaussian_policy and not self.ppo
                         and os.environ.get("MAPDN_FUSED_ROLLOUT", "1") != "0")
        if fused_explore:
            # std = exp(log_std) with log_std = log(fixed_policy_std) (model.py:119-120, util.py:56), rounded as the f32 tensors are
            std = float(torch.tensor(math.log(a.fixed_policy_std), dtype=torch.float32).exp()) if a.shared_params else 1.0

        def policy(obs, last_hid):
            if fused_explore:
                # get_actions(status="train", exploration=True) without the log-probability nobody reads in this loop (maddpg.py:81-101,
                # util.py:52-76) and with translate_action (util.py:123-132) in the same launch: mapdn_explore_actions draws nothing itself —
                # eps is torch.randn_like(means), the same draw from the same generator as Normal(mean, std).rsample()
                means, _, hid = net.policy(obs, last_hid)
                means = means.contiguous()
                eps = torch.randn_like(means)
                action, action_pol, actual = torch.empty_like(means), torch.empty_like(means), torch.empty_like(means)
                av = avail.expand_as(means).contiguous() if avail.shape != means.shape else avail.contiguous()
                launch("mapdn_explore_actions", dv, means, eps, av, std, int(bool(a.action_enforcebound)), float(a.action_scale), float(a.action_bias),
                       action, action_pol, actual, means.numel())
                return action, hid, dict(action_pol=action_pol, last_hid=last_hid, hid=hid, actual=actual)
            if train:
                action, action_pol, log_prob, _, hid = net.get_actions(obs, "train", True, avail, False, last_hid)
            else:
                action, action_pol, log_prob, _, hid = net.get_actions(obs, "test", False, avail, False, last_hid)
            return action, hid, dict(action_pol=action_pol, last_hid=last_hid, hid=hid, log_prob=log_prob)

        def on_step(t, obs, action, reward, done, info, next_obs, alive, aux):
            action_pol, last_hid, hid = aux["action_pol"], aux["last_hid"], aux["hid"]
            trans = dict(state=obs, action=action_pol, reward=reward.float().unsqueeze(-1).expand(B, net.n_).contiguous(),
                         next_state=next_obs, done=done.view(B, 1).float(),
                         last_step=(done | (t == a.max_steps - 1)).view(B, 1).float(), action_avail=avail,
                         last_hid=last_hid, hid=hid, valid=alive.clone())
            if self.ppo:                                        # models/model.py:212-222: what the behaviour net gave BEFORE this step's update
                with torch.no_grad():
                    trans.update(log_prob=aux["log_prob"], value=net.value(obs), next_value=net.value(next_obs))
            self.transition_update(trans, stat)
            self.steps += 1

        def agree(flag):                                        # data-parallel ranks must agree on the early exit: `steps` drives
            if self._dist is None:                              # the update schedule and every update is a collective
                return flag
            if self._dist.get_backend() != "nccl":
                flag = flag.cpu()
            self._dist.all_reduce(flag, op=self._dist.ReduceOp.MAX)
            self.collectives["all_reduce_flag"] += 1
            return flag

        from ..rollout import BatchedRollout
        ro = BatchedRollout(env, policy, a.max_steps, on_step=on_step if train else None, store_window=False, all_alive_reduce=agree,
                            action_scale=a.action_scale, action_bias=a.action_bias)
        _, ep = ro.run(prefix=prefix, hidden=net.init_hidden(B))
        for k, v in ep.items():
            stat[k] = v if train else stat.get(k, 0.0) + v

    def train_process(self, stat):
        self._episode(stat, train=True)
        self.episodes += 1
        for k, v in list(stat.items()):
            if torch.is_tensor(v):
                stat[k] = float(v)

    def evaluation(self, stat):
        """num_eval_episodes episodes in total, B at a time (model.py:265-302)"""
        rounds = max(1, -(-self.args.num_eval_episodes // self.env.n_envs))
        test = {}
        for _ in range(rounds):
            self._episode(test, train=False)
        stat.update({k: v / rounds for k, v in test.items()})

    def run(self, stat, episode: int):
        """trainer.py:110-113"""
        self.train_process(stat)
        if episode % self.args.eval_freq == self.args.eval_freq - 1 or episode == 0:
            self.evaluation(stat)

    def save(self, path):
        torch.save({"model_state_dict": self.behaviour_net.state_dict()}, path)          # train.py:119

    def load(self, path):
        self.behaviour_net.load_state_dict(torch.load(path, map_location=self.device)["model_state_dict"])
