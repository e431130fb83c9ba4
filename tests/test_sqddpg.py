"""SQDDPG learner (mapdn_amd/learner/sqddpg.py) against fixtures produced by the reference's own code
(tests/golden/make_sqddpg_golden.py): forward passes, value(), d value / d action, both losses, the stats and every entry of the state_dict
after two value steps, one policy step and one soft target update, strict state_dict round trip — with the bars tests/test_coma.py holds
the same quantities to.  The reference draws its coalition orders inside every marginal_contribution call; the fixtures carry the seed
set before each call and the position tensors it yields, which the learner takes as batch["coalitions"] (and, on the CPU, must also
DRAW itself from that seed, three times per get_loss call).  Then the factored first layer against a literal restatement of the
reference's five-dimensional expand / gather / mask in float64, the own-slot-only action gradient, the argument refusals, and the
trainer on a CPU stand-in env: the ring is kept and no target is cached."""
import os

import numpy as np
import pytest
import torch

from mapdn_amd.learner import DDPGNet, PGTrainer, SQDDPGNet, make_alg_args, net_class, sample_coalition_positions
from tests.shap_kernel_matrix import literal_critic_input as _literal

HERE = os.path.dirname(__file__)
VARIANTS = {
    "sqddpg_shared": dict(),
    "sqddpg_separate": dict(shared_params=False, agent_id=False, hid_activation="tanh"),
    "sqddpg_target_policy": dict(double_q=False),
    "sqddpg_advnorm": dict(normalize_advantages=True),
    "sqddpg_noln": dict(layernorm=False),
    "sqddpg_s1": dict(sample_size=1),
    "sqddpg_s3": dict(sample_size=3),
}
RTOL, ATOL = 2e-5, 2e-6                      # tests/test_coma.py's


def _load(name, device="cpu"):
    z = np.load(os.path.join(HERE, "golden", f"learner_{name}.npz"))
    n, o = z["batch/state"].shape[1:]
    h = z["batch/hid"].shape[-1]
    args = make_alg_args(n, o, 1, alg="sqddpg", hid_size=h, **VARIANTS[name])
    trainer = PGTrainer(args, "sqddpg", env=None, device=device, data_parallel=False)
    init = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("init/")}
    trainer.behaviour_net.load_state_dict(init, strict=True)          # names/shapes == reference model.pt
    batch = {k[6:]: torch.from_numpy(z[k]).float().to(device) for k in z.files if k.startswith("batch/")}
    return z, args, trainer, batch


def _with_pos(z, b, call, device):
    return dict(b, coalitions=torch.from_numpy(z["pos/" + call]).to(device))


def _close(a, b, what, rtol=RTOL, atol=ATOL):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    assert np.allclose(a, b, rtol=rtol, atol=atol), (what, np.abs(a - b).max())


def _three_draws(z, call):
    """the generator state after the three [bs * S, n] multinomial draws of a get_loss call from the recorded seed"""
    _, bs, S, n = z["pos/" + call].shape
    torch.manual_seed(int(z["seed/" + call]))
    for k in range(3):
        assert np.array_equal(sample_coalition_positions(bs * S, n, "cpu").view(bs, S, n).numpy(), z["pos/" + call][k])
    return torch.get_rng_state()


def check_forward_and_losses(name, device, rtol=RTOL, atol=ATOL):
    import functools
    _close = functools.partial(globals()["_close"], rtol=rtol, atol=atol)
    z, args, tr, b = _load(name, device)
    net = tr.behaviour_net
    bs, n = b["state"].shape[:2]
    S = args.sample_size
    assert z["pos/loss"].shape == (3, bs, S, n) and z["pos/value"].shape == (1, bs, S, n)
    means, log_stds, hid = net.policy(b["state"], b["last_hid"])
    _close(means, z["out/means"], "means"); _close(log_stds, z["out/log_stds"], "log_stds"); _close(hid, z["out/hiddens"], "hid")
    pos = torch.from_numpy(z["pos/value"][0]).to(device)
    act = b["action"].clone().requires_grad_(True)
    v = net.marginal_contribution(b["state"], act, pos)
    assert v.shape == (bs, S, n, 1)
    _close(v, z["out/value"], "value")
    v.sum().backward()
    _close(act.grad, z["out/dvalue_daction"], "d value / d action (the own slot only)")
    net.zero_grad()
    a, _, lp, _, _ = net.get_actions(b["state"], "test", False, b["action_avail"], False, b["last_hid"])
    assert lp is None
    _close(a, z["out/test_action"], "test action")
    a, _, _, _, _ = net.get_actions(b["state"], "train", False, b["action_avail"], True, b["last_hid"])
    _close(a, z["out/target_mean_action"], "target policy")
    state0 = {k: t.clone() for k, t in net.state_dict().items()}
    pl, vl, _ = net.get_loss(_with_pos(z, b, "loss", device))
    _close(pl, z["out/policy_loss"], "policy loss"); _close(vl, z["out/value_loss"], "value loss")
    if device == "cpu":                                  # the learner's OWN draws from the recorded seed are the reference's, three per call
        net.load_state_dict(state0)
        torch.manual_seed(int(z["seed/value"]))
        _close(net.value(b["state"], b["action"]), z["out/value"], "value(), coalitions drawn from the recorded seed")
        after = _three_draws(z, "loss")
        torch.manual_seed(int(z["seed/loss"]))
        pl2, vl2, _ = net.get_loss(b)
        _close(pl2, z["out/policy_loss"], "policy loss, coalitions drawn from the recorded seed")
        _close(vl2, z["out/value_loss"], "value loss, coalitions drawn from the recorded seed")
        assert torch.equal(torch.get_rng_state(), after)
        for want in (("value",), ("policy",)):           # a skipped forward pass still makes its draw
            torch.manual_seed(int(z["seed/loss"]))
            net.get_loss(b, want=want)
            assert torch.equal(torch.get_rng_state(), after), want
    only_v = net.get_loss(b, want=("value",))
    assert only_v[0] is None and only_v[2] is None
    only_p = net.get_loss(b, want=("policy",))
    assert only_p[1] is None and only_p[0] is not None


def check_update_steps(name, device, rtol=RTOL, atol=ATOL, move_rtol=2e-3, move_atol=2e-6):
    import functools
    _close = functools.partial(globals()["_close"], rtol=rtol, atol=atol)
    z, args, tr, b = _load(name, device)
    net = tr.behaviour_net
    net.get_loss(_with_pos(z, b, "loss", device))        # the generator's loss probe also moved the BatchNorm statistics
    stat = {}
    tr.value_transition_process(stat, _with_pos(z, b, "value0", device))
    tr.value_transition_process(stat, _with_pos(z, b, "value1", device))
    tr.policy_transition_process(stat, _with_pos(z, b, "policy", device))
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
    """critic input [all obs | joint action | ids] (sqddpg.py:22-26, 83-90): 46 entries with shared parameters, 118 without (n = 3).  Both
    directions: the reference's state_dict loads here with strict=True (_load), and what is saved here has exactly the reference's keys and
    shapes (the fixture's final/ entries are the reference's own state_dict), so that it loads there with strict=True."""
    z, args, tr, b = _load("sqddpg_shared")
    sd = tr.behaviour_net.state_dict()
    n, o = b["state"].shape[1:]
    assert len(sd) == 46 and sd["value_dicts.0.fc1.weight"].shape == (args.hid_size, (o + 1) * n + n)
    assert sd["target_net.value_dicts.0.fc1.weight"].shape == sd["value_dicts.0.fc1.weight"].shape and "batchnorm.running_mean" in sd
    zs = np.load(os.path.join(HERE, "golden", "learner_sqddpg_separate.npz"))
    sep = _load("sqddpg_separate")[2].behaviour_net.state_dict()
    assert len(sep) == 118 and sep["value_dicts.2.fc1.weight"].shape == (args.hid_size, (o + 1) * n)
    for mine, ref in ((sd, z), (sep, zs)):
        assert {k: tuple(v.shape) for k, v in mine.items()} == {k[6:]: ref[k].shape for k in ref.files if k.startswith("final/")}
    p = tmp_path / "model.pt"
    tr.save(p)
    tr2 = PGTrainer(args, "sqddpg", env=None, device="cpu", data_parallel=False)
    tr2.load(p)
    for k, v in sd.items():
        assert torch.equal(v, tr2.behaviour_net.state_dict()[k])
    # MADDPG's critic has the same width but the id block BEFORE the actions: the classes are told apart by the registry, not by shape
    assert net_class("sqddpg") is SQDDPGNet and net_class("maddpg") is DDPGNet


def test_arguments_and_registry():
    a = make_alg_args(3, 5, 1, alg="sqddpg")
    assert a.sample_size == 10 and a.action_enforcebound is True and a.gaussian_policy is False
    assert make_alg_args(3, 5, 1, alg="sqddpg", sample_size=4).sample_size == 4
    assert SQDDPGNet(a).alg == "sqddpg" and SQDDPGNet(a).sample_size == 10
    for over, word in ((dict(continuous=False), "continuous=False"), (dict(mixer=True), "mixer"), (dict(episodic=True), "episodic"),
                       (dict(gaussian_policy=True), "gaussian_policy=True")):
        with pytest.raises(NotImplementedError, match=word):
            make_alg_args(3, 5, 1, alg="sqddpg", **over)
    with pytest.raises(NotImplementedError, match="action_dim"):
        make_alg_args(3, 5, 2, alg="sqddpg")
    bad = make_alg_args(3, 5, 1)
    bad.action_dim = 2
    with pytest.raises(NotImplementedError, match="action_dim"):       # the class checks too, whatever assembled the namespace
        SQDDPGNet(bad)
    with pytest.raises(ValueError, match="sample_size"):
        make_alg_args(3, 5, 1, alg="sqddpg", sample_size=0)
    for wrong in (lambda: SQDDPGNet(a, "maddpg"), lambda: DDPGNet(a, "sqddpg"), lambda: net_class("facmaddpg")):
        with pytest.raises(KeyError):
            wrong()


# ---- the factored first layer against the reference's construction, restated literally ------------------------------------------------
def literal_critic_input(obs, act, pos):
    """tests/shap_kernel_matrix.py's literal construction for obs [b, n, o], act [b, n, 1]"""
    return _literal(obs.reshape(obs.shape[0], -1), act.reshape(act.shape[0], -1), pos)


def _net64(n, o, **over):
    torch.manual_seed(5)
    args = make_alg_args(n, o, 1, alg="sqddpg", hid_size=8, **over)
    net = SQDDPGNet(args).double()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return net


@pytest.mark.parametrize("b,n,S", [(2, 1, 1), (3, 2, 1), (4, 5, 3), (2, 17, 2)])
def test_factored_route_equals_the_literal_construction(b, n, S):
    o = 4
    net = _net64(n, o, sample_size=S)
    g = torch.Generator().manual_seed(b * 100 + n)
    obs, act = torch.randn(b, n, o, generator=g, dtype=torch.float64), torch.randn(b, n, 1, generator=g, dtype=torch.float64)
    pos = sample_coalition_positions(b * S, n, "cpu", generator=g).view(b, S, n)
    cr = net.value_dicts[0]
    a1, a2 = act.clone().requires_grad_(True), act.clone().requires_grad_(True)
    got = net.marginal_contribution(obs, a1, pos)
    want = cr(literal_critic_input(obs, a2, pos).reshape(b * S * n, -1))[0].view(b, S, n, 1)
    assert got.shape == want.shape and float((got - want).detach().abs().max()) <= 1e-12
    wts = torch.randn(b, S, n, 1, generator=g, dtype=torch.float64)
    params = list(cr.parameters())
    g_got = torch.autograd.grad((got * wts).sum(), [a1] + params)
    g_want = torch.autograd.grad((want * wts).sum(), [a2] + params)
    for x, y in zip(g_got, g_want):
        assert float((x - y).abs().max()) <= 1e-12 * max(1.0, float(y.abs().max()))


def test_factored_route_per_agent_critics_equal_the_literal_construction():
    b, n, S, o = 3, 4, 2, 3
    net = _net64(n, o, sample_size=S, shared_params=False, agent_id=False, hid_activation="tanh")
    g = torch.Generator().manual_seed(9)
    obs, act = torch.randn(b, n, o, generator=g, dtype=torch.float64), torch.randn(b, n, 1, generator=g, dtype=torch.float64)
    pos = sample_coalition_positions(b * S, n, "cpu", generator=g).view(b, S, n)
    got = net.marginal_contribution(obs, act, pos)
    inp = literal_critic_input(obs, act, pos)[..., :-n]                # (no id block)
    want = torch.stack([cr(inp[:, :, i].reshape(b * S, -1))[0].view(b, S, 1) for i, cr in enumerate(net.value_dicts)], 2)
    assert float((got - want).detach().abs().max()) <= 1e-12


def test_only_the_own_slot_carries_the_action_gradient():
    """sqddpg.py:73-77: row (b, s, i) sees the actions before it detached: d v[b, s, i] / d act[b, j] = 0 for j != i, and for j = i it is
    dx . W_act[:, pos_i] — the column of the SLOT, not of the agent"""
    b, n, S, o = 2, 4, 3, 3
    net = _net64(n, o, sample_size=S)
    g = torch.Generator().manual_seed(2)
    obs, act = torch.randn(b, n, o, generator=g, dtype=torch.float64), torch.randn(b, n, 1, generator=g, dtype=torch.float64)
    pos = sample_coalition_positions(b * S, n, "cpu", generator=g).view(b, S, n)
    for i in range(n):
        a = act.clone().requires_grad_(True)
        net.marginal_contribution(obs, a, pos)[:, :, i].sum().backward()
        grad = a.grad.view(b, n)
        others = [j for j in range(n) if j != i]
        assert float(grad[:, others].abs().max()) == 0.0 and float(grad[:, i].abs().min()) > 0.0
    # the value does depend on the agents before: moving the FIRST agent of an order moves the rows behind it
    first = int(pos[0, 0].argmin())
    moved = act.clone(); moved[0, first] += 1.0
    d = (net.marginal_contribution(obs, moved, pos) - net.marginal_contribution(obs, act, pos))[0, 0].abs().view(n)
    assert float(d.min()) > 0.0
    # own_action_only: same values, same action gradient, no critic gradient
    a = act.clone().requires_grad_(True)
    v = net.marginal_contribution(obs, a, pos, own_action_only=True)
    a2 = act.clone().requires_grad_(True)
    v2 = net.marginal_contribution(obs, a2, pos)
    assert torch.equal(v, v2)
    v.sum().backward(); v2.sum().backward()
    assert torch.allclose(a.grad, a2.grad, rtol=0, atol=1e-14)


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


def test_trainer_episode_keeps_the_ring_and_caches_nothing(tmp_path):
    """off-policy (models/model.py:53-56 clears the buffer for the on-policy algorithms only), and the value target depends on coalitions
    drawn in every get_loss call: nothing of it can be computed once per round"""
    torch.manual_seed(0); np.random.seed(0)
    env = _ToyEnv(4, 3, 5)
    args = make_alg_args(3, 5, 1, alg="sqddpg", **TOY)
    tr = PGTrainer(args, "sqddpg", env, device="cpu", data_parallel=False)
    before = {k: v.clone() for k, v in tr.behaviour_net.state_dict().items()}
    cached, seen_keys = [], set()
    ct, vrp = tr._cache_targets, tr.value_replay_process

    def cache_spy():
        cached.append(ct())
        return cached[-1]

    def value_spy(stat):
        seen_keys.update(tr.replay_buffer.store)
        return vrp(stat)
    tr._cache_targets, tr.value_replay_process = cache_spy, value_spy
    stat = {}
    tr.run(stat, 0)
    assert tr.steps == 12 and tr.episodes == 1
    assert cached and not any(cached) and not any(k.endswith("_cached") for k in seen_keys)
    assert len(tr.replay_buffer) == 16                    # the ring is full (4 envs x 12 steps into 16 places) and was never emptied
    assert {"mean_train_reward", "mean_test_reward", "mean_train_value_loss", "mean_train_policy_loss", "mean_train_entropy"} <= set(stat)
    assert all(isinstance(v, float) and np.isfinite(v) for v in stat.values())
    after = tr.behaviour_net.state_dict()
    for prefix in ("value_dicts", "policy_dicts", "target_net.value_dicts"):
        assert any(not torch.equal(before[k], after[k]) for k in before if k.startswith(prefix)), prefix
    p = tmp_path / "model.pt"
    tr.save(p)
    tr2 = PGTrainer(args, "sqddpg", env, device="cpu", data_parallel=False)
    tr2.load(p)
    for k, v in after.items():
        assert torch.equal(v, tr2.behaviour_net.state_dict()[k])
