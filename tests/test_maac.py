"""MAAC learner (mapdn_amd/learner/maac.py) against fixtures produced by the reference's own code
(tests/golden/make_maac_golden.py): forward passes, value() with its regulariser row, d value / d action, both losses, the stats and every
entry of the state_dict after one value step, one policy step and one soft target update, strict state_dict round trip — with the bars
tests/test_coma.py holds the same quantities to.  The reference draws twice inside get_loss; the fixtures carry the seed set before each
call and the two standard-normal tensors it yields, which the learner takes as batch["noise"] / batch["next_noise"] (and, on the CPU, must
also DRAW itself from that seed, twice per call).  Then the refusals and the registry, the batched attention route against a literal
restatement of the reference's per-head, per-agent loop in float64, and the trainer on a CPU stand-in env: the ring is kept."""
import os

import numpy as np
import pytest
import torch

from mapdn_amd import learner
from mapdn_amd.learner import COMANet, DDPGNet, MAACNet, PGTrainer, make_alg_args, net_class

HERE = os.path.dirname(__file__)
VARIANTS = {
    "maac_shared": dict(),
    "maac_separate": dict(shared_params=False, agent_id=False, hid_activation="tanh"),
    "maac_heads4": dict(attend_heads=4),
    "maac_norm_in": dict(norm_in=True),
    "maac_nosoft": dict(soft=False),
    "maac_advnorm": dict(normalize_advantages=True),
}
RTOL, ATOL = 2e-5, 2e-6                      # tests/test_coma.py's


def _load(name, device="cpu"):
    z = np.load(os.path.join(HERE, "golden", f"learner_{name}.npz"))
    n, o = z["batch/state"].shape[1:]
    h = z["batch/hid"].shape[-1]
    args = make_alg_args(n, o, 1, alg="maac", hid_size=h, **VARIANTS[name])
    trainer = PGTrainer(args, "maac", env=None, device=device, data_parallel=False)
    init = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("init/")}
    trainer.behaviour_net.load_state_dict(init, strict=True)          # names/shapes == reference model.pt
    batch = {k[6:]: torch.from_numpy(z[k]).float().to(device) for k in z.files if k.startswith("batch/")}
    return z, args, trainer, batch


def _with_noise(z, b, call, device):
    return dict(b, noise=torch.from_numpy(z["noise/" + call]).to(device), next_noise=torch.from_numpy(z["next_noise/" + call]).to(device))


def _close(a, b, what, rtol=RTOL, atol=ATOL):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    assert np.allclose(a, b, rtol=rtol, atol=atol), (what, np.abs(a - b).max())


def check_forward_and_losses(name, device, rtol=RTOL, atol=ATOL):
    import functools
    _close = functools.partial(globals()["_close"], rtol=rtol, atol=atol)
    z, args, tr, b = _load(name, device)
    net = tr.behaviour_net
    bs, n = b["state"].shape[:2]
    assert z["noise/loss"].shape == (bs, n, 1) and z["next_noise/loss"].shape == (bs, n, 1)
    net.eval()
    means, log_stds, hid = net.policy(b["state"], b["last_hid"])
    _close(means, z["out/means"], "means"); _close(log_stds, z["out/log_stds"], "log_stds"); _close(hid, z["out/hiddens"], "hid")
    assert float(log_stds.detach().min()) >= args.LOG_STD_MIN and float(log_stds.detach().max()) <= args.LOG_STD_MAX and float(log_stds.detach().std()) > 0
    v = net.value(b["state"], b["action"])
    assert v.shape == (bs + 1, n)                        # row bs: the attention regulariser per agent
    _close(v, z["out/value_eval"], "value (eval mode)")
    a, _, lp, _, _ = net.get_actions(b["state"], "test", False, b["action_avail"], False, b["last_hid"])
    assert lp is None
    _close(a, z["out/test_action"], "test action")
    _close(a, np.tanh(z["out/means"]), "test action = tanh(mean)")
    net.train()
    if "out/value" in z.files:
        _close(net.value(b["state"], b["action"]), z["out/value"], "value")
        act = b["action"].clone().requires_grad_(True)
        net.value(b["state"], act)[:bs].sum().backward()
        _close(act.grad, z["out/dvalue_daction"], "d value / d action (the whole joint action carries gradient)")
        net.zero_grad()
    state0 = {k: t.clone() for k, t in net.state_dict().items()}
    pl, vl, (m2, ls2) = net.get_loss(_with_noise(z, b, "loss", device))
    _close(pl, z["out/policy_loss"], "policy loss"); _close(vl, z["out/value_loss"], "value loss")
    if device == "cpu":                                  # the learner's OWN draws from the recorded seed are the reference's, two per call
        for want in (("policy", "value"), ("value",), ("policy",)):
            net.load_state_dict(state0)
            torch.manual_seed(int(z["seed/loss"]))
            torch.randn(bs, n, 1); torch.randn(bs, n, 1)
            after_two_draws = torch.get_rng_state()
            torch.manual_seed(int(z["seed/loss"]))
            pl2, vl2, _ = net.get_loss(b, want=want)
            if "policy" in want:
                _close(pl2, z["out/policy_loss"], f"policy loss, actions drawn from the recorded seed, want={want}")
            if "value" in want:
                _close(vl2, z["out/value_loss"], f"value loss, actions drawn from the recorded seed, want={want}")
            assert torch.equal(torch.get_rng_state(), after_two_draws), want
        pl3, _, _ = net.get_loss(b, want=("policy",))    # ... and the next call draws anew
        assert abs(float(pl3.detach()) - float(z["out/policy_loss"])) > 1e-7
    only_v = net.get_loss(_with_noise(z, b, "loss", device), want=("value",))
    assert only_v[0] is None and only_v[2] is None


def check_update_steps(name, device, rtol=RTOL, atol=ATOL, move_rtol=2e-3, move_atol=2e-6):
    import functools
    _close = functools.partial(globals()["_close"], rtol=rtol, atol=atol)
    z, args, tr, b = _load(name, device)
    net = tr.behaviour_net
    net.get_loss(_with_noise(z, b, "loss", device))      # the generator's loss probe also moved the BatchNorm statistics
    stat = {}
    tr.value_transition_process(stat, _with_noise(z, b, "value", device))
    tr.policy_transition_process(stat, _with_noise(z, b, "policy", device))
    net.update_target()
    for k in ("value_grad_norm", "value_loss", "entropy", "policy_grad_norm", "policy_loss"):
        _close(stat["mean_train_" + k], z["stat/mean_train_" + k], k)
    final = net.state_dict()
    ref_keys = sorted(k[6:] for k in z.files if k.startswith("final/"))
    assert sorted(final) == ref_keys
    for k in ref_keys:
        if k.endswith("num_batches_tracked"):
            assert int(final[k]) == int(z["final/" + k]), k
        else:
            init = z["init/" + k]                        # parameters moved by lr 1e-4 RMSprop steps: compare the MOVE, not just the value
            assert np.allclose(final[k].cpu().numpy() - init, z["final/" + k] - init, rtol=move_rtol, atol=move_atol), k


@pytest.mark.parametrize("name", list(VARIANTS))
def test_forward_and_losses_match_reference(name):
    check_forward_and_losses(name, "cpu")


@pytest.mark.parametrize("name", list(VARIANTS))
def test_update_steps_match_reference(name):
    check_update_steps(name, "cpu")


def test_state_dict_layout_and_round_trip(tmp_path):
    """the reference's names: one AttentionCritic for all agents under value_dicts.0, mean / log_std heads in the agent"""
    z, args, tr, b = _load("maac_shared")
    sd = tr.behaviour_net.state_dict()
    n, o = b["state"].shape[1:]
    h = args.hid_size
    assert sd["value_dicts.0.critic_encoders.2.enc_fc1.weight"].shape == (h, o + 1) and sd["value_dicts.0.state_encoders.0.s_enc_fc1.weight"].shape == (h, o)
    assert sd["value_dicts.0.critics.1.critic_fc1.weight"].shape == (h, 2 * h) and sd["value_dicts.0.biases.1.bias_fc2.weight"].shape == (1, h)
    assert sd["value_dicts.0.key_extractors.0.weight"].shape == (h, h) and sd["value_dicts.0.value_extractors.0.0.bias"].shape == (h,)
    assert "value_dicts.0.selector_extractors.0.bias" not in sd and "value_dicts.0.key_extractors.0.bias" not in sd
    assert sd["policy_dicts.0.mean.weight"].shape == (1, h) and sd["policy_dicts.0.log_std.bias"].shape == (1,) and "policy_dicts.0.fc2.weight" not in sd
    assert "batchnorm.running_mean" in sd and "target_net.value_dicts.0.critics.0.critic_fc2.bias" in sd
    assert sorted(sd) == sorted(k[6:] for k in z.files if k.startswith("final/"))
    h4 = _load("maac_heads4")[2].behaviour_net.state_dict()
    assert h4["value_dicts.0.key_extractors.3.weight"].shape == (h // 4, h) and h4["value_dicts.0.value_extractors.3.0.weight"].shape == (h // 4, h)
    ni = _load("maac_norm_in")[2].behaviour_net.state_dict()
    assert ni["value_dicts.0.critic_encoders.0.enc_bn.running_mean"].shape == (o + 1,) and ni["value_dicts.0.state_encoders.2.s_enc_bn.running_var"].shape == (o,)
    assert "value_dicts.0.critic_encoders.0.enc_bn.weight" not in ni                    # affine=False
    sep = _load("maac_separate")[2].behaviour_net.state_dict()
    assert "policy_dicts.2.log_std.weight" in sep and "value_dicts.1.critics.0.critic_fc1.weight" not in sep       # one critic either way
    p = tmp_path / "model.pt"
    tr.save(p)
    tr2 = PGTrainer(args, "maac", env=None, device="cpu", data_parallel=False)
    tr2.load(p)
    for k, v in sd.items():
        assert torch.equal(v, tr2.behaviour_net.state_dict()[k])
    ref_named = {k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("final/")}      # ... and a reference-named dict the other way
    tr2.behaviour_net.load_state_dict(ref_named, strict=True)
    with pytest.raises(RuntimeError):
        PGTrainer(make_alg_args(n, o, 1, hid_size=h), "maddpg", env=None, device="cpu", data_parallel=False).behaviour_net.load_state_dict(sd, strict=True)


def test_arguments_and_registry():
    assert net_class("maac") is MAACNet and net_class("coma") is COMANet and net_class("maddpg") is DDPGNet
    a = make_alg_args(3, 7, alg="maac")
    assert a.gaussian_policy is True and a.attend_heads == 1 and a.norm_in is False and a.soft is True and a.reward_scale == 100 and a.action_enforcebound
    d = make_alg_args(3, 7)
    assert d.gaussian_policy is False and (d.attend_heads, d.norm_in, d.soft, d.reward_scale) == (1, False, True, 100)
    for kw in (dict(), dict(alg="maddpg"), dict(alg="coma")):           # the Gaussian head passes on the MAAC route alone
        with pytest.raises(NotImplementedError):
            make_alg_args(3, 7, gaussian_policy=True, **kw)
    for kw, name in ((dict(continuous=False), "continuous"), (dict(agent_type="mlp"), "agent_type"), (dict(action_dim=2), "action_dim")):
        with pytest.raises(NotImplementedError, match=name):
            make_alg_args(3, 7, alg="maac", **kw)
    with pytest.raises(ValueError, match="agent_num"):
        make_alg_args(1, 7, alg="maac")
    with pytest.raises(ValueError, match="attend_heads"):
        make_alg_args(3, 7, alg="maac", attend_heads=3)
    with pytest.raises(KeyError):
        make_alg_args(3, 7, alg="maac", heads=2)
    for bad in (lambda: net_class("iac"), lambda: DDPGNet(a, "maac"), lambda: COMANet(a, "maac"), lambda: MAACNet(a, "maddpg")):
        with pytest.raises(KeyError):
            bad()
    with pytest.raises(NotImplementedError, match="gaussian_policy"):   # args made for another algorithm do not build a MAAC net
        MAACNet(make_alg_args(3, 7), "maac")


@pytest.mark.parametrize("b,n,hid,H", [(5, 2, 8, 1), (1, 3, 8, 4), (7, 6, 64, 2), (3, 38, 64, 4)])
def test_batched_route_equals_the_literal_loop(b, n, hid, H):
    """one masked softmax over [b, H, n, n] against the per-head, per-agent stack / permute / softmax / sum chain, float64, values and
    gradients: 1e-12 of the scale"""
    g = torch.Generator().manual_seed(b * 100 + n)
    ops = [torch.randn(b, n, hid, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(3)]
    w_out, w_sq = torch.randn(b, n, hid, generator=g, dtype=torch.float64), torch.randn(n, H, generator=g, dtype=torch.float64)
    res = []
    for fn in (learner.attention_loop_reference, learner.attention_core_torch):
        out, lsq = fn(*ops, H)
        assert out.shape == (b, n, hid) and lsq.shape == (n, H)
        res.append((out, lsq) + torch.autograd.grad((out * w_out).sum() + (lsq * w_sq).sum(), ops))
    for x, y in zip(*res):
        assert float((x - y).detach().abs().max()) <= 1e-12 * max(1.0, float(x.detach().abs().max()))
    assert not learner.attention_ok(ops[0], H)           # float64 on the CPU is the batched route's


def test_value_is_the_reference_loop_through_the_modules():
    """value() through attention_core against the same critic evaluated agent by agent with the literal loop in its place"""
    z, args, tr, b = _load("maac_heads4")
    net = tr.behaviour_net.double()
    obs, act = b["state"].double(), b["action"].double()
    want = net.value(obs, act)
    real = learner.maac.attention_core                   # (patched in the module AttentionCritic.forward looks it up in)
    learner.maac.attention_core = learner.attention_loop_reference
    try:
        got = net.value(obs, act)
    finally:
        learner.maac.attention_core = real
    assert float((got - want).abs().max()) <= 1e-12


def test_valid_mask():
    z, args, tr, b = _load("maac_shared")
    net = tr.behaviour_net
    bn = _with_noise(z, b, "loss", "cpu")
    p0, v0, _ = net.get_loss(bn)
    p1, v1, _ = net.get_loss(dict(bn, valid=torch.ones(b["state"].shape[0], dtype=torch.bool)))
    assert torch.allclose(p0, p1) and torch.allclose(v0, v1)
    half = torch.tensor([1, 1, 0, 0], dtype=torch.bool)
    ph, vh, _ = net.get_loss(dict(bn, valid=half))
    assert torch.isfinite(vh) and not torch.allclose(vh, v1) and torch.isfinite(ph) and not torch.allclose(ph, p1)


class _ToyEnv:
    """stand-in with the VoltageControlBatch surface (the real one needs a GPU): reward = -|a - target|"""

    def __init__(self, B, n, o, device="cpu", episode_limit=12):
        self.n_envs, self.n_agents, self.obs_size, self.device, self.episode_limit = B, n, o, torch.device(device), episode_limit
        self.g = torch.Generator().manual_seed(0)

    def reset(self):
        self.t = 0
        self.o = torch.randn(self.n_envs, self.n_agents, self.obs_size, generator=self.g)
        return self.o, None

    def get_avail_actions(self):
        return torch.ones(self.n_envs, self.n_agents, 1)

    def get_obs(self):
        return self.o

    def step(self, a):
        self.t += 1
        r = -(a - 0.3 * self.o[..., 0]).abs().mean(1).double()
        self.o = torch.randn(self.n_envs, self.n_agents, self.obs_size, generator=self.g)
        done = torch.full((self.n_envs,), self.t >= self.episode_limit, dtype=torch.bool)
        return r, done, torch.zeros(self.n_envs, 11, dtype=torch.float64)


TOY = dict(hid_size=16, max_steps=12, batch_size=8, replay_buffer_size=16, behaviour_update_freq=4, target_update_freq=6, value_update_epochs=3,
           num_eval_episodes=4, attend_heads=2)


def test_trainer_episode_keeps_the_ring_and_caches_nothing(tmp_path):
    """models/model.py:53-56: MAAC is off-policy, its buffer is not cleared; its targets depend on a draw, so no *_cached field exists
    while the value epochs run"""
    torch.manual_seed(0); np.random.seed(0)
    env = _ToyEnv(4, 3, 5)
    args = make_alg_args(3, 5, 1, alg="maac", **TOY)
    tr = PGTrainer(args, "maac", env, device="cpu", data_parallel=False)
    seen, vrp = [], tr.value_replay_process

    def value_spy(stat):
        seen.append((len(tr.replay_buffer), sorted(k for k in tr.replay_buffer.store if k.endswith("_cached"))))
        return vrp(stat)
    tr.value_replay_process = value_spy
    before = {k: v.clone() for k, v in tr.behaviour_net.state_dict().items()}
    stat = {}
    tr.run(stat, 0)
    assert tr.steps == 12 and tr.episodes == 1
    assert len(seen) == 2 * 3 and all(c == [] for _, c in seen)
    assert len(tr.replay_buffer) == 16                   # the ring is full and was never emptied
    assert {"mean_train_reward", "mean_test_reward", "mean_train_value_loss", "mean_train_policy_loss", "mean_train_entropy"} <= set(stat)
    assert all(isinstance(v, float) and np.isfinite(v) for v in stat.values())
    after = tr.behaviour_net.state_dict()
    for prefix in ("value_dicts", "policy_dicts", "target_net.value_dicts"):
        assert any(not torch.equal(before[k], after[k]) for k in before if k.startswith(prefix)), prefix
    p = tmp_path / "model.pt"
    tr.save(p)
    tr2 = PGTrainer(args, "maac", env, device="cpu", data_parallel=False)
    tr2.load(p)
    for k, v in after.items():
        assert torch.equal(v, tr2.behaviour_net.state_dict()[k])
