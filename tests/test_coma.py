"""COMA learner (mapdn_amd/learner/coma.py) against fixtures produced by the reference's own code
(tests/golden/make_coma_golden.py): forward passes, value(), d value / d action, both losses, the stats and every entry of the state_dict
after two value steps, one policy step and one soft target update, strict state_dict round trip — with the bars tests/test_matd3.py holds
the same quantities to.  The reference draws the counterfactual actions inside get_loss; the fixtures carry the seed set before each call
and the standard-normal tensor it yields, which the learner takes as batch["cf_noise"] (and, on the CPU, must also DRAW itself from that
seed, once per call).  Then the counterfactual route against explicit value() calls on the merged actions, and the trainer on a CPU
stand-in env: the ring is emptied after every update round."""
import os

import numpy as np
import pytest
import torch

from mapdn_amd.learner import COMANet, DDPGNet, PGTrainer, make_alg_args, net_class

HERE = os.path.dirname(__file__)
VARIANTS = {
    "coma_shared": dict(),
    "coma_separate": dict(shared_params=False, agent_id=False, hid_activation="tanh"),
    "coma_target_policy": dict(double_q=False),
    "coma_advnorm": dict(normalize_advantages=True),
    "coma_noln": dict(layernorm=False, reward_normalisation=False),
    "coma_s2": dict(sample_size=2),
}
RTOL, ATOL = 2e-5, 2e-6                      # tests/test_matd3.py's


def _load(name, device="cpu"):
    z = np.load(os.path.join(HERE, "golden", f"learner_{name}.npz"))
    n, o = z["batch/state"].shape[1:]
    h = z["batch/hid"].shape[-1]
    args = make_alg_args(n, o, 1, hid_size=h, **VARIANTS[name])
    trainer = PGTrainer(args, "coma", env=None, device=device, data_parallel=False)
    init = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("init/")}
    trainer.behaviour_net.load_state_dict(init, strict=True)          # names/shapes == reference model.pt
    batch = {k[6:]: torch.from_numpy(z[k]).float().to(device) for k in z.files if k.startswith("batch/")}
    return z, args, trainer, batch


def _with_noise(z, b, call, device):
    return dict(b, cf_noise=torch.from_numpy(z["noise/" + call]).to(device))


def _close(a, b, what, rtol=RTOL, atol=ATOL):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    assert np.allclose(a, b, rtol=rtol, atol=atol), (what, np.abs(a - b).max())


def check_forward_and_losses(name, device, rtol=RTOL, atol=ATOL):
    import functools
    _close = functools.partial(globals()["_close"], rtol=rtol, atol=atol)
    z, args, tr, b = _load(name, device)
    net = tr.behaviour_net
    bs, n = b["state"].shape[:2]
    assert z["noise/loss"].shape == (args.sample_size, bs, n, 1)
    means, log_stds, hid = net.policy(b["state"], b["last_hid"])
    _close(means, z["out/means"], "means"); _close(log_stds, z["out/log_stds"], "log_stds"); _close(hid, z["out/hiddens"], "hid")
    v = net.value(b["state"], b["action"])
    assert v.shape == (bs, n, 1)
    _close(v, z["out/value"], "value")
    a, _, lp, _, _ = net.get_actions(b["state"], "test", False, b["action_avail"], False, b["last_hid"])
    assert lp is None
    _close(a, z["out/test_action"], "test action")
    a, _, _, _, _ = net.get_actions(b["state"], "train", False, b["action_avail"], True, b["last_hid"])
    _close(a, z["out/target_mean_action"], "target policy")
    act = b["action"].clone().requires_grad_(True)
    net.value(b["state"], act).sum().backward()
    _close(act.grad, z["out/dvalue_daction"], "d value / d action (the whole joint action carries gradient)")
    net.zero_grad()
    state0 = {k: t.clone() for k, t in net.state_dict().items()}
    pl, vl, _ = net.get_loss(_with_noise(z, b, "loss", device))
    _close(pl, z["out/policy_loss"], "policy loss"); _close(vl, z["out/value_loss"], "value loss")
    if device == "cpu":                                  # the learner's OWN draw from the recorded seed is the reference's, once per call
        net.load_state_dict(state0)
        torch.manual_seed(int(z["seed/loss"]))
        torch.randn(z["noise/loss"].shape)
        after_one_draw = torch.get_rng_state()
        torch.manual_seed(int(z["seed/loss"]))
        pl2, _, _ = net.get_loss(b)
        _close(pl2, z["out/policy_loss"], "policy loss, actions drawn from the recorded seed")
        assert torch.equal(torch.get_rng_state(), after_one_draw)
        pl3, _, _ = net.get_loss(b, want=("policy",))    # ... and the next call draws anew
        assert abs(float(pl3.detach()) - float(pl2.detach())) > 1e-7
        torch.manual_seed(int(z["seed/loss"]))
        net.get_loss(b, want=("value",))                 # the value update draws too (coma.py:143 runs in every get_loss)
        assert torch.equal(torch.get_rng_state(), after_one_draw)
    only_v = net.get_loss(b, want=("value",))
    assert only_v[0] is None and only_v[2] is None


def check_update_steps(name, device, rtol=RTOL, atol=ATOL, move_rtol=2e-3, move_atol=2e-6):
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
    check_forward_and_losses(name, "cpu")


@pytest.mark.parametrize("name", list(VARIANTS))
def test_update_steps_match_reference(name):
    check_update_steps(name, "cpu")


def test_state_dict_layout_and_round_trip(tmp_path):
    """critic input [all obs | own obs | ids | joint action] (coma.py:24): 46 entries with shared parameters, 118 without (n = 3)"""
    z, args, tr, b = _load("coma_shared")
    sd = tr.behaviour_net.state_dict()
    n, o = b["state"].shape[1:]
    assert len(sd) == 46 and sd["value_dicts.0.fc1.weight"].shape == (args.hid_size, (n + 1) * o + n + n)
    assert sd["target_net.value_dicts.0.fc1.weight"].shape == sd["value_dicts.0.fc1.weight"].shape and "batchnorm.running_mean" in sd
    sep = _load("coma_separate")[2].behaviour_net.state_dict()
    assert len(sep) == 118 and sep["value_dicts.2.fc1.weight"].shape == (args.hid_size, (n + 1) * o + n)
    assert sorted(sd) == sorted(k[6:] for k in z.files if k.startswith("final/"))
    p = tmp_path / "model.pt"
    tr.save(p)
    tr2 = PGTrainer(args, "coma", env=None, device="cpu", data_parallel=False)
    tr2.load(p)
    for k, v in sd.items():
        assert torch.equal(v, tr2.behaviour_net.state_dict()[k])
    with pytest.raises(RuntimeError):                     # a MADDPG critic is one observation narrower: not interchangeable
        PGTrainer(args, "maddpg", env=None, device="cpu", data_parallel=False).behaviour_net.load_state_dict(sd, strict=True)


def test_sample_size_below_two_is_refused_by_name():
    """coma.py:44 tells sampled from taken actions by the batch dimension, which is the same at sample_size 1"""
    for s in (1, 0):
        with pytest.raises(ValueError, match="sample_size"):
            COMANet(make_alg_args(3, 5, 1, sample_size=s), "coma")
        with pytest.raises(ValueError, match="sample_size"):
            PGTrainer(make_alg_args(3, 5, 1, sample_size=s), "coma", env=None, device="cpu", data_parallel=False)
    assert COMANet(make_alg_args(3, 5, 1, sample_size=2)).alg == "coma"
    DDPGNet(make_alg_args(3, 5, 1, sample_size=1), "maddpg")        # read by COMA alone
    assert net_class("coma") is COMANet and net_class("matd3") is DDPGNet
    for bad in (lambda: net_class("iac"), lambda: COMANet(make_alg_args(3, 5, 1), "maddpg"), lambda: DDPGNet(make_alg_args(3, 5, 1), "coma")):
        with pytest.raises(KeyError):                                # each class is its own algorithms only; the registry picks
            bad()


def test_valid_mask():
    z, args, tr, b = _load("coma_shared")
    net = tr.behaviour_net
    bn = _with_noise(z, b, "loss", "cpu")
    p0, v0, _ = net.get_loss(bn)
    p1, v1, _ = net.get_loss(dict(bn, valid=torch.ones(b["state"].shape[0], dtype=torch.bool)))
    assert torch.allclose(p0, p1) and torch.allclose(v0, v1)
    half = torch.tensor([1, 1, 1, 0, 0, 0], dtype=torch.bool)
    ph, vh, _ = net.get_loss(dict(bn, valid=half))
    assert torch.isfinite(vh) and not torch.allclose(vh, v1) and torch.isfinite(ph) and not torch.allclose(ph, p1)


@pytest.mark.parametrize("name", ["coma_shared", "coma_separate", "coma_noln"])
def test_counterfactual_route_equals_explicit_value_calls(name):
    """the PyTorch baseline route (taken row + rank-1 term per sample) against S value() calls on the merged actions of coma.py:144-149:
    for every agent i the joint action with agent i's entry replaced by the draw.  float32 against float32 in another order of
    summation: 1e-5 of the values' scale."""
    z, args, tr, b = _load(name)
    net = tr.behaviour_net
    bs, n = b["state"].shape[:2]
    S = args.sample_size
    g = torch.Generator().manual_seed(3)
    sampled = torch.randn(S, bs, n, 1, generator=g)
    baselines, values = net.counterfactual(b["state"], b["action"], sampled)
    assert baselines.shape == (bs, n) and values.shape == (bs, n)
    with torch.no_grad():
        want_v = net.value(b["state"], b["action"]).view(bs, n)
        want_b = torch.zeros(bs, n)
        for s in range(S):
            for i in range(n):
                merged = b["action"].clone()
                merged[:, i] = sampled[s, :, i]
                want_b[:, i] += net.value(b["state"], merged)[:, i, 0]
        want_b /= S
    scale = max(1.0, float(want_v.abs().max()))
    assert float((values - want_v).abs().max()) <= 1e-5 * scale
    assert float((baselines - want_b).abs().max()) <= 1e-5 * scale
    assert float((baselines - values).abs().max()) > 1e-3           # (the draws do move the critic)


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
           num_eval_episodes=4, sample_size=3)


@pytest.mark.parametrize("alg", ["coma", "maddpg"])
def test_the_ring_is_emptied_after_an_update_round_and_not_before(alg):
    """models/model.py:53-56: COMA's buffer is cleared after the round's value and policy epochs; MADDPG's is not"""
    torch.manual_seed(0); np.random.seed(0)
    env = _ToyEnv(4, 3, 5)
    tr = PGTrainer(make_alg_args(3, 5, 1, **TOY), alg, env, device="cpu", data_parallel=False)
    seen = []                                            # (step, ring length when the round's policy update sampled, ring length after the step)
    ppp, tu = tr.policy_replay_process, tr.transition_update
    at_policy = []

    def policy_spy(stat):
        at_policy.append(len(tr.replay_buffer))
        return ppp(stat)

    def update_spy(trans, stat):
        before = len(at_policy)
        tu(trans, stat)
        seen.append((tr.steps, at_policy[-1] if len(at_policy) > before else None, len(tr.replay_buffer)))
    tr.policy_replay_process, tr.transition_update = policy_spy, update_spy
    tr.train_process({})
    rounds = [s for s in seen if s[1] is not None]
    assert [s[0] for s in rounds] == [4, 8]              # steps 4 and 8 (step 0 is not past the warm-up; 12 is not reached)
    for step, at_pol, after in rounds:
        assert at_pol >= 8                                # not emptied before the round's last update
        assert after == (0 if alg == "coma" else at_pol)
    if alg == "coma":
        assert [s[2] for s in seen if s[0] in (5, 9, 11)] == [4, 4, 12]      # refills from empty, 4 envs per step
        assert not any(k.endswith("_cached") for k in tr.replay_buffer.store)


def test_trainer_episode_and_checkpoint(tmp_path):
    torch.manual_seed(0); np.random.seed(0)
    env = _ToyEnv(4, 3, 5)
    args = make_alg_args(3, 5, 1, **TOY)
    tr = PGTrainer(args, "coma", env, device="cpu", data_parallel=False)
    before = {k: v.clone() for k, v in tr.behaviour_net.state_dict().items()}
    stat = {}
    tr.run(stat, 0)
    assert tr.steps == 12 and tr.episodes == 1
    assert {"mean_train_reward", "mean_test_reward", "mean_train_value_loss", "mean_train_policy_loss", "mean_train_entropy"} <= set(stat)
    assert all(isinstance(v, float) and np.isfinite(v) for v in stat.values())
    after = tr.behaviour_net.state_dict()
    for prefix in ("value_dicts", "policy_dicts", "target_net.value_dicts"):
        assert any(not torch.equal(before[k], after[k]) for k in before if k.startswith(prefix)), prefix
    p = tmp_path / "model.pt"
    tr.save(p)
    tr2 = PGTrainer(args, "coma", env, device="cpu", data_parallel=False)
    tr2.load(p)
    for k, v in after.items():
        assert torch.equal(v, tr2.behaviour_net.state_dict()[k])
