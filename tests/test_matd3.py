"""MATD3 learner (mapdn_amd/learner/ddpg.py, alg="matd3") against fixtures produced by the reference's own code
(tests/golden/make_matd3_golden.py): forward passes (value() is [2b, n, 1]), both losses, every entry of the state_dict after two value
steps, one policy step and one soft target update, strict state_dict round trip — with the bars tests/test_learner.py holds the other
two algorithms to.  The reference draws the target-smoothing noise inside get_loss; the fixtures carry the seed set before each call and
the tensor it yields, which the learner takes as batch["next_noise"] (and, on the CPU, must also DRAW itself from that seed).
Then the trainer on a CPU stand-in env, and the per-round cache of what is deterministic in MATD3's target."""
import os

import numpy as np
import pytest
import torch

from mapdn_amd.learner import DDPGNet, PGTrainer, make_alg_args

HERE = os.path.dirname(__file__)
VARIANTS = {
    "matd3_shared": dict(),
    "matd3_separate": dict(shared_params=False, agent_id=False, hid_activation="tanh"),
    "matd3_clamp": dict(action_enforcebound=False, clip_c=0.5),
    "matd3_target_policy": dict(double_q=False),
    "matd3_noln": dict(layernorm=False, reward_normalisation=False, normalize_advantages=True),
    "matd3_advnorm": dict(normalize_advantages=True),
}
RTOL, ATOL = 2e-5, 2e-6


def _load(name, device="cpu"):
    z = np.load(os.path.join(HERE, "golden", f"learner_{name}.npz"))
    n, o = z["batch/state"].shape[1:]
    h = z["batch/hid"].shape[-1]
    args = make_alg_args(n, o, 1, hid_size=h, **VARIANTS[name])
    trainer = PGTrainer(args, "matd3", env=None, device=device, data_parallel=False)
    init = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("init/")}
    trainer.behaviour_net.load_state_dict(init, strict=True)          # names/shapes == reference model.pt
    batch = {k[6:]: torch.from_numpy(z[k]).float().to(device) for k in z.files if k.startswith("batch/")}
    return z, args, trainer, batch


def _with_noise(z, b, call, device):
    return dict(b, next_noise=torch.from_numpy(z["noise/" + call]).to(device))


def _close(a, b, what, rtol=RTOL, atol=ATOL):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    assert np.allclose(a, b, rtol=rtol, atol=atol), (what, np.abs(a - b).max())


def _check_forward_and_losses(name, device, rtol=RTOL, atol=ATOL):
    import functools
    _close = functools.partial(globals()["_close"], rtol=rtol, atol=atol)
    z, args, tr, b = _load(name, device)
    net = tr.behaviour_net
    bs, n = b["state"].shape[:2]
    means, log_stds, hid = net.policy(b["state"], b["last_hid"])
    _close(means, z["out/means"], "means"); _close(log_stds, z["out/log_stds"], "log_stds"); _close(hid, z["out/hiddens"], "hid")
    v = net.value(b["state"], b["action"])
    assert v.shape == (2 * bs, n, 1)
    _close(v, z["out/value"], "value (values1 over values2)")
    a, _, lp, _, _ = net.get_actions(b["state"], "test", False, b["action_avail"], False, b["last_hid"])
    assert lp is None
    _close(a, z["out/test_action"], "test action")
    a, _, _, _, _ = net.get_actions(b["state"], "train", False, b["action_avail"], True, b["last_hid"])
    _close(a, z["out/target_mean_action"], "target policy")
    act = b["action"].clone().requires_grad_(True)
    net.value(b["state"], act).sum().backward()
    _close(act.grad, z["out/dvalue_daction"], "d value / d action (own-action gradient rule, both heads)")
    net.zero_grad()
    state0 = {k: t.clone() for k, t in net.state_dict().items()}
    pl, vl, _ = net.get_loss(_with_noise(z, b, "loss", device))
    _close(pl, z["out/policy_loss"], "policy loss"); _close(vl, z["out/value_loss"], "value loss")
    if device == "cpu":                                  # the learner's OWN draw from the recorded seed is the reference's
        net.load_state_dict(state0)
        torch.manual_seed(int(z["seed/loss"]))
        _, vl2, _ = net.get_loss(b)
        _close(vl2, z["out/value_loss"], "value loss, noise drawn from the recorded seed")
        _, vl3, _ = net.get_loss(b, want=("value",))    # ... and the next call draws anew
        assert abs(float(vl3.detach()) - float(vl2.detach())) > 1e-6
    only_v = net.get_loss(b, want=("value",))
    assert only_v[0] is None and only_v[2] is None


def _check_update_steps(name, device, rtol=RTOL, atol=ATOL, move_rtol=2e-3, move_atol=2e-6):
    import functools
    _close = functools.partial(globals()["_close"], rtol=rtol, atol=atol)
    z, args, tr, b = _load(name, device)
    net = tr.behaviour_net
    net.get_loss(_with_noise(z, b, "loss", device))      # the generator's loss probe also moved the BatchNorm statistics
    stat = {}
    tr.value_transition_process(stat, _with_noise(z, b, "value0", device))
    tr.value_transition_process(stat, _with_noise(z, b, "value1", device))
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
    _check_forward_and_losses(name, "cpu")


@pytest.mark.parametrize("name", list(VARIANTS))
def test_update_steps_match_reference(name):
    _check_update_steps(name, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VARIANTS))
def test_forward_and_losses_match_reference_on_gpu(name):
    _check_forward_and_losses(name, "cuda:0", rtol=1e-4, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VARIANTS))
def test_update_steps_match_reference_on_gpu(name):
    _check_update_steps(name, "cuda:0", rtol=1e-4, atol=1e-5, move_rtol=1e-2, move_atol=1e-5)


def test_state_dict_layout_and_round_trip(tmp_path):
    """the twin is ONE critic with one more input column (matd3.py:20-29): 46 entries with shared parameters, 118 without (n = 3)"""
    z, args, tr, b = _load("matd3_shared")
    sd = tr.behaviour_net.state_dict()
    n, o = b["state"].shape[1:]
    assert len(sd) == 46 and sd["value_dicts.0.fc1.weight"].shape == (args.hid_size, (o + 1) * n + n + 1)
    assert sd["target_net.value_dicts.0.fc1.weight"].shape == sd["value_dicts.0.fc1.weight"].shape and "batchnorm.running_mean" in sd
    assert len(_load("matd3_separate")[2].behaviour_net.state_dict()) == 118
    p = tmp_path / "model.pt"
    tr.save(p)
    tr2 = PGTrainer(args, "matd3", env=None, device="cpu", data_parallel=False)
    tr2.load(p)
    for k, v in sd.items():
        assert torch.equal(v, tr2.behaviour_net.state_dict()[k])
    with pytest.raises(RuntimeError):                     # a MADDPG critic is one column narrower: not interchangeable
        PGTrainer(args, "maddpg", env=None, device="cpu", data_parallel=False).behaviour_net.load_state_dict(sd, strict=True)


def test_valid_mask_clip_rule_and_unknown_algorithm():
    z, args, tr, b = _load("matd3_shared")
    net = tr.behaviour_net
    bn = _with_noise(z, b, "loss", "cpu")
    p0, v0, _ = net.get_loss(bn)
    p1, v1, _ = net.get_loss(dict(bn, valid=torch.ones(b["state"].shape[0], dtype=torch.bool)))
    assert torch.allclose(p0, p1) and torch.allclose(v0, v1)
    half = torch.tensor([1, 1, 1, 0, 0, 0], dtype=torch.bool)
    _, vh, _ = net.get_loss(dict(bn, valid=half), want=("value",))
    assert torch.isfinite(vh) and not torch.allclose(vh, v1)
    with pytest.raises(KeyError):
        DDPGNet(args, "coma")
    with pytest.raises(KeyError):
        PGTrainer(args, "td3", env=None, device="cpu", data_parallel=False)
    # utilities/util.py:57-76: `clip` is read only without action_enforcebound
    mean, ls, eps = torch.zeros(4, 3, 1), torch.zeros(4, 3, 1), torch.full((4, 3, 1), 3.0)
    a_bound, _ = net._select_action(mean, ls, "train", True, clip=True, noise=eps)
    assert torch.allclose(a_bound, torch.tanh(eps))
    netc = _load("matd3_clamp")[2].behaviour_net
    a_clip, _ = netc._select_action(mean, ls, "train", True, clip=True, noise=eps)
    a_free, _ = netc._select_action(mean, ls, "train", True, clip=False, noise=eps)
    assert torch.allclose(a_clip, torch.full_like(eps, 0.5)) and torch.allclose(a_free, eps)


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
           num_eval_episodes=4)


def test_trainer_episode_and_checkpoint(tmp_path):
    torch.manual_seed(0); np.random.seed(0)
    env = _ToyEnv(4, 3, 5)
    args = make_alg_args(3, 5, 1, **TOY)
    tr = PGTrainer(args, "matd3", env, device="cpu", data_parallel=False)
    before = {k: v.clone() for k, v in tr.behaviour_net.state_dict().items()}
    stat = {}
    tr.run(stat, 0)
    assert tr.steps == 12 and tr.episodes == 1
    assert {"mean_train_reward", "mean_test_reward", "mean_train_value_loss", "mean_train_policy_loss"} <= set(stat)
    assert all(isinstance(v, float) and np.isfinite(v) for v in stat.values())
    after = tr.behaviour_net.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before if k.startswith("value_dicts"))
    assert any(not torch.equal(before[k], after[k]) for k in before if k.startswith("target_net.value_dicts"))
    assert not any(k.endswith("_cached") for k in tr.replay_buffer.store)           # the round's cache does not outlive the round
    p = tmp_path / "model.pt"
    tr.save(p)
    tr2 = PGTrainer(args, "matd3", env, device="cpu", data_parallel=False)
    tr2.load(p)
    for k, v in after.items():
        assert torch.equal(v, tr2.behaviour_net.state_dict()[k])


# ---- the per-round cache: deterministic parts only ---------------------------------------------------------------------------------
def _round(monkeypatch, cache_on, fixed_noise, **over):
    """one episode of the toy env; returns (final state_dict, [per value epoch: (window fields seen, noise used)])"""
    monkeypatch.setenv("MAPDN_CACHE_NEXT_ACTIONS", "1" if cache_on else "0")
    torch.manual_seed(0); np.random.seed(0)
    env = _ToyEnv(4, 3, 5)
    args = make_alg_args(3, 5, 1, **dict(TOY, **over))
    tr = PGTrainer(args, "matd3", env, device="cpu", data_parallel=False)
    net, seen = tr.behaviour_net, []
    sample = tr.replay_buffer.get_batch
    g = torch.Generator().manual_seed(5)
    calls = [0]

    def get_batch(bs):                                   # the same windows and (when fixed) the same noise per call on both code paths
        np.random.seed(1000 + calls[0]); calls[0] += 1
        b = dict(sample(bs))
        if fixed_noise:
            b["next_noise"] = torch.randn(bs, 3, 1, generator=g)
        return b
    monkeypatch.setattr(tr.replay_buffer, "get_batch", get_batch)
    smooth = net.smoothed_actions

    def spy(means, avail, noise=None):
        out = smooth(means, avail, noise)
        seen.append((means.clone(), out.clone()))
        return out
    monkeypatch.setattr(net, "smoothed_actions", spy)
    cached_keys = []
    vtp = tr.value_transition_process

    def vspy(stat, batch):
        cached_keys.append(sorted(k for k in batch if k.endswith("_cached")))
        return vtp(stat, batch)
    monkeypatch.setattr(tr, "value_transition_process", vspy)
    tr.train_process({})
    return {k: v.clone() for k, v in net.state_dict().items()}, seen, cached_keys


@pytest.mark.parametrize("over", [dict(), dict(double_q=False), dict(shared_params=False)], ids=["default", "target_policy", "separate"])
def test_round_cache_equals_per_epoch_passes(monkeypatch, over):
    on, _, keys_on = _round(monkeypatch, True, True, **over)
    off, _, keys_off = _round(monkeypatch, False, True, **over)
    want = ["next_mean_cached"] + (["next_obs_term_cached"] if over.get("shared_params", True) else [])
    assert keys_on and all(k == want for k in keys_on) and all(k == [] for k in keys_off)
    assert not any("value" in k or "action" in k for ks in keys_on for k in ks)      # nothing that depends on the noise is cached
    init = PGTrainer(make_alg_args(3, 5, 1, **dict(TOY, **over)), "matd3", None, device="cpu", data_parallel=False).behaviour_net.state_dict()
    for k in on:
        if k.endswith("num_batches_tracked"):
            assert int(on[k]) == int(off[k])
        else:
            assert np.allclose(on[k].numpy(), off[k].numpy(), rtol=2e-3, atol=2e-6), k
    assert set(init) == set(on)


def test_cached_round_draws_fresh_noise_every_epoch(monkeypatch):
    """ring of 16 transitions, windows of 8, three value epochs per round: epochs share transitions; with the cache on their means are
    the cached ones (equal for a shared transition) but the smoothed actions differ — every epoch has its own draw"""
    _, seen, keys = _round(monkeypatch, True, False)
    assert keys and all("next_mean_cached" in k for k in keys)
    pairs = 0
    for i in range(len(seen)):
        for j in range(i + 1, len(seen)):
            (m1, a1), (m2, a2) = seen[i], seen[j]
            same = (m1.unsqueeze(1) == m2.unsqueeze(0)).flatten(2).all(-1)            # [bs, bs]: the same transition's means
            for r, c in same.nonzero().tolist():
                pairs += 1
                assert not torch.equal(a1[r], a2[c])
    assert pairs > 0
