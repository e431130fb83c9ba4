"""MAPPO / IPPO learners (mapdn_amd/learner/ppo.py) against fixtures produced by the reference's own code
(tests/golden/make_ppo_golden.py): forward passes, value(), both losses, the stats and every entry of the state_dict after two value steps,
one policy step and one soft target update, strict state_dict round trip — with the bars tests/test_coma.py holds the same quantities to
(tests/test_matd3.py's).  Then what is this project's own: the refusals, ppo_old_log_prob="stored" against a hand-written ratio, the GAE
chain stride (B interleaved series at stride B == each series alone at stride 1), the union statistics of the advantage BatchNorm under
data-parallel training, and the trainer on a CPU stand-in env: the three new transition fields, the emptied ring, and MADDPG's
transitions unchanged."""
import os

import numpy as np
import pytest
import torch

from mapdn_amd import learner as L
from mapdn_amd.learner import DDPGNet, PGTrainer, PPONet, make_alg_args, net_class
from tests.test_coma import TOY, _ToyEnv

HERE = os.path.dirname(__file__)
VARIANTS = {
    "shared": dict(),
    "separate": dict(shared_params=False, agent_id=False, hid_activation="tanh"),
    "plain": dict(normalize_advantages=False, layernorm=False, reward_normalisation=False),
    "target_policy": dict(double_q=False),
}
NAMES = [f"{alg}_{v}" for alg in ("mappo", "ippo") for v in VARIANTS]
RTOL, ATOL = 2e-5, 2e-6                      # tests/test_coma.py's, from tests/test_matd3.py


def _load(name, device="cpu", **over):
    alg, variant = name.split("_", 1)
    z = np.load(os.path.join(HERE, "golden", f"learner_{name}.npz"))
    n, o = z["batch/state"].shape[1:]
    h = z["batch/hid"].shape[-1]
    args = make_alg_args(n, o, 1, alg=alg, hid_size=h, **dict(VARIANTS[variant], **over))
    trainer = PGTrainer(args, alg, env=None, device=device, data_parallel=False)
    init = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("init/")}
    trainer.behaviour_net.load_state_dict(init, strict=True)          # names/shapes == reference model.pt
    batch = {k[6:]: torch.from_numpy(z[k]).float().to(device) for k in z.files if k.startswith("batch/")}
    batch["log_prob"] = batch.pop("log_prob_a")                       # the reference's Transition field name
    return z, args, trainer, batch


def _close(a, b, what, rtol=RTOL, atol=ATOL):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    assert np.allclose(a, b, rtol=rtol, atol=atol), (what, np.abs(a - b).max())


def check_forward_and_losses(name, device, rtol=RTOL, atol=ATOL):
    import functools
    _close = functools.partial(globals()["_close"], rtol=rtol, atol=atol)
    z, args, tr, b = _load(name, device)
    net = tr.behaviour_net
    bs, n = b["state"].shape[:2]
    done, last = z["batch/done"].reshape(-1), z["batch/last_step"].reshape(-1)
    combos = {(int(d), int(s)) for d, s in zip(done, last)}
    assert combos == {(0, 0), (0, 1), (1, 0), (1, 1)} and last[-1] == 1 and (done[:-1] * last[:-1]).sum() == 1      # the batch the issue asks for
    means, log_stds, hid = net.policy(b["state"], b["last_hid"])
    _close(means, z["out/means"], "means"); _close(log_stds, z["out/log_stds"], "log_stds"); _close(hid, z["out/hiddens"], "hid")
    v = net.value(b["state"], b["action"])
    assert v.shape == (bs, n, 1)
    _close(v, z["out/value"], "value")
    _close(net.value(b["next_state"]), z["out/next_value"], "value(next_state), no action given")
    a, _, lp, _, _ = net.get_actions(b["state"], "test", False, b["action_avail"], False, b["last_hid"])
    assert lp is None
    _close(a, z["out/test_action"], "test action")
    a, _, _, _, _ = net.get_actions(b["state"], "train", False, b["action_avail"], True, b["last_hid"])
    _close(a, z["out/target_mean_action"], "target policy")
    before = torch.get_rng_state()
    pl, vl, (m2, ls2) = net.get_loss(b)
    assert torch.equal(torch.get_rng_state(), before), "get_loss drew a random number"
    _close(pl, z["out/policy_loss"], "policy loss"); _close(vl, z["out/value_loss"], "value loss")
    _close(m2, z["out/means"], "action_out means")
    only_v = net.get_loss(b, want=("value",))
    assert only_v[0] is None and only_v[2] is None and only_v[1] is not None
    only_p = net.get_loss(b, want=("policy",))
    assert only_p[1] is None and only_p[0] is not None


def check_update_steps(name, device, rtol=RTOL, atol=ATOL, move_rtol=2e-3, move_atol=2e-6):
    import functools
    _close = functools.partial(globals()["_close"], rtol=rtol, atol=atol)
    z, args, tr, b = _load(name, device)
    net = tr.behaviour_net
    net.get_loss(b)                                      # the generator's loss probe also moved the BatchNorm statistics
    stat = {}
    tr.value_transition_process(stat, b)
    tr.value_transition_process(stat, b)
    tr.policy_transition_process(stat, b)
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


@pytest.mark.parametrize("name", NAMES)
def test_forward_and_losses_match_reference(name):
    check_forward_and_losses(name, "cpu")


@pytest.mark.parametrize("name", NAMES)
def test_update_steps_match_reference(name):
    check_update_steps(name, "cpu")


def test_registry_and_merged_arguments():
    assert net_class("mappo") is PPONet and net_class("ippo") is PPONet and net_class("maddpg") is DDPGNet
    for bad in ("iac", "facmaddpg"):
        with pytest.raises(KeyError):
            net_class(bad)
    with pytest.raises(KeyError):
        PPONet(make_alg_args(3, 5, 1, alg="mappo"), "maddpg")
    with pytest.raises(KeyError):
        DDPGNet(make_alg_args(3, 5, 1), "mappo")
    for alg in ("mappo", "ippo"):
        a = make_alg_args(3, 5, 1, alg=alg)
        got = {k: getattr(a, k) for k in ("policy_update_epochs", "value_update_epochs", "lambda_", "eps_clip", "value_loss_coef", "normalize_advantages",
                                          "behaviour_update_freq", "target_update_freq", "ppo_old_log_prob")}
        assert got == dict(policy_update_epochs=10, value_update_epochs=10, lambda_=0.95, eps_clip=0.6, value_loss_coef=2.0, normalize_advantages=True,
                           behaviour_update_freq=240, target_update_freq=480, ppo_old_log_prob="reference")
        assert make_alg_args(3, 5, 1, alg=alg, eps_clip=0.2, lambda_=0.9).eps_clip == 0.2            # overrides come last (train.py:60-62)
    d = make_alg_args(3, 5, 1)                                       # the other algorithms' merged values are what they were
    assert (d.policy_update_epochs, d.behaviour_update_freq, d.target_update_freq, d.normalize_advantages) == (1, 60, 120, False)
    with pytest.raises(KeyError):
        make_alg_args(3, 5, 1, alg="mappo", clip_range=0.2)


@pytest.mark.parametrize("alg", ["mappo", "ippo"])
@pytest.mark.parametrize("over,exc,match", [
    (dict(continuous=False), NotImplementedError, "continuous"), (dict(gaussian_policy=True), NotImplementedError, "gaussian_policy"),
    (dict(action_dim=2), NotImplementedError, "action_dim"), (dict(mixer=True), NotImplementedError, "mixer"),
    (dict(episodic=True), NotImplementedError, "episodic"), (dict(agent_type="mlp"), NotImplementedError, "agent_type"),
    (dict(ppo_old_log_prob="new"), ValueError, "ppo_old_log_prob")])
def test_each_refusal_names_its_argument(alg, over, exc, match):
    rest = dict(over)
    with pytest.raises(exc, match=match):
        make_alg_args(3, 5, rest.pop("action_dim", 1), alg=alg, **rest)
    args = make_alg_args(3, 5, 1, alg=alg)
    (key, value), = over.items()
    setattr(args, key, value)
    with pytest.raises(exc, match=match):                             # the class refuses as well, however its args were made
        PPONet(args, alg)


@pytest.mark.parametrize("name", ["mappo_shared", "ippo_separate"])
def test_state_dict_layout_and_round_trip(name, tmp_path):
    """V(s) critics: MAPPO's first layer is n o (+ n) wide, IPPO's o (+ n); PPO.batchnorm (the advantages') is no part of the state_dict"""
    z, args, tr, b = _load(name)
    net = tr.behaviour_net
    sd = net.state_dict()
    n, o = b["state"].shape[1:]
    ids = n if args.agent_id else 0
    assert sd["value_dicts.0.fc1.weight"].shape == (args.hid_size, (n * o if net.alg == "mappo" else o) + ids)
    assert sd["target_net.value_dicts.0.fc1.weight"].shape == sd["value_dicts.0.fc1.weight"].shape
    assert len(sd) == (46 if args.shared_params else 118)
    assert sorted(sd) == sorted(k[6:] for k in z.files if k.startswith("final/"))
    assert [k for k in sd if "batchnorm" in k] == ["batchnorm.weight", "batchnorm.bias", "batchnorm.running_mean", "batchnorm.running_var",
                                                   "batchnorm.num_batches_tracked", "target_net.batchnorm.weight", "target_net.batchnorm.bias",
                                                   "target_net.batchnorm.running_mean", "target_net.batchnorm.running_var",
                                                   "target_net.batchnorm.num_batches_tracked"]
    adv_bn = net.__dict__["_adv_batchnorm"]
    assert adv_bn is not net.batchnorm and adv_bn.training
    net.eval()
    assert adv_bn.training and not net.batchnorm.training           # a plain object's module: never switched to eval (ppo.py:11)
    net.train()
    p = tmp_path / "model.pt"
    tr.save(p)
    tr2 = PGTrainer(args, net.alg, env=None, device="cpu", data_parallel=False)
    tr2.load(p)                                                       # strict
    for k, v in sd.items():
        assert torch.equal(v, tr2.behaviour_net.state_dict()[k])
    other = "ippo" if net.alg == "mappo" else "mappo"
    with pytest.raises(RuntimeError):                                 # the two critics differ in width: not interchangeable
        PGTrainer(make_alg_args(n, o, 1, alg=other, hid_size=args.hid_size, **VARIANTS[name.split("_", 1)[1]]), other, env=None, device="cpu",
                  data_parallel=False).behaviour_net.load_state_dict(sd, strict=True)


def test_stored_old_log_prob_differs_and_equals_a_hand_written_ratio():
    z, args, tr, b = _load("mappo_shared", ppo_old_log_prob="stored")
    net = tr.behaviour_net
    ref_net = _load("mappo_shared")[2].behaviour_net
    pl_stored = net.get_loss(b, want=("policy",))[0]
    pl_ref = ref_net.get_loss(b, want=("policy",))[0]
    _close(pl_ref, z["out/policy_loss"], "the default is the reference's ratio")
    assert abs(float(pl_stored) - float(pl_ref)) > 1e-3
    with torch.no_grad():
        fresh = _load("mappo_shared", ppo_old_log_prob="stored")[2].behaviour_net
        means, log_stds, _ = fresh.policy(b["state"], b["last_hid"])
        lp = torch.distributions.Normal(means, log_stds.exp()).log_prob(b["action"])
        mask = 1.0 - (b["action_avail"] == 0).float()
        ratio = torch.exp((mask * lp).sum(-1) - (mask * b["log_prob"]).sum(-1))
        adv = fresh.advantages(b, fresh.batchnorm(b["reward"]))
        want = -torch.min(ratio * adv, torch.clamp(ratio, 1 - 0.6, 1 + 0.6) * adv).mean()
    _close(pl_stored, float(want), "policy loss with the stored log-probability")
    with pytest.raises(KeyError):                                     # "stored" needs the field; the default never reads it
        net.get_loss({k: v for k, v in b.items() if k != "log_prob"}, want=("policy",))
    ref_net.get_loss({k: v for k, v in b.items() if k != "log_prob"}, want=("policy",))


def test_valid_mask():
    z, args, tr, b = _load("ippo_shared")
    net = tr.behaviour_net
    p0, v0, _ = net.get_loss(b)
    p1, v1, _ = net.get_loss(dict(b, valid=torch.ones(b["state"].shape[0], dtype=torch.bool)))
    assert torch.allclose(p0, p1) and torch.allclose(v0, v1)
    half = torch.tensor([1, 1, 1, 1, 0, 0, 0, 0, 0], dtype=torch.bool)
    ph, vh, _ = net.get_loss(dict(b, valid=half))
    assert torch.isfinite(vh) and not torch.allclose(vh, v1) and torch.isfinite(ph) and not torch.allclose(ph, p1)
    pz, vz, _ = net.get_loss(dict(b, valid=torch.zeros(9, dtype=torch.bool)))
    assert float(pz) == 0.0 and float(vz) == 0.0


def _series(B, T, n, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    done = (torch.rand(T, B, generator=g) < 0.2).float()
    last = (torch.rand(T, B, generator=g) < 0.3).float()
    return dict(reward=r(T, B, n), value=r(T, B, n), next_value=r(T, B, n), done=done, last_step=last)


@pytest.mark.parametrize("B,T,lo,hi", [(4, 6, 0, 24), (4, 6, 2, 24), (4, 6, 0, 21), (5, 7, 3, 31), (3, 5, 4, 6)],
                         ids=["whole", "mid-step-start", "ragged-end", "both", "shorter-than-two-steps"])
def test_stride_property(B, T, lo, hi):
    """B envs' series interleaved in (step, env) order and evaluated at S = B give, per env, the advantages of that env's series alone
    at S = 1 — for a window that starts in the middle of a step and one that ends in the middle of one too"""
    n = 3
    s = _series(B, T, n, 7 * B + T)
    flat = {k: v.reshape((T * B,) + v.shape[2:])[lo:hi] for k, v in s.items()}           # rows (t, env), a window of them
    got = L.ppo_gae_torch(flat["reward"], flat["value"], flat["next_value"], flat["done"], flat["last_step"], B, 0.99, 0.95)
    assert got.shape == (hi - lo, n)
    seen = 0
    for e in range(B):
        rows = [i for i in range(lo, hi) if i % B == e]                                    # env e's rows of the window, oldest first
        if not rows:
            continue
        t = [i // B for i in rows]
        alone = L.ppo_gae_torch(s["reward"][t, e], s["value"][t, e], s["next_value"][t, e], s["done"][t, e], s["last_step"][t, e], 1, 0.99, 0.95)
        assert torch.equal(got[[i - lo for i in rows]], alone), e
        seen += len(rows)
    assert seen == hi - lo
    ref = torch.zeros(hi - lo, n)                       # S = 1 on the alone series is the reference's loop, literally (ppo.py:46-54)
    for e in range(B):
        last_adv = 0
        for i in reversed([i for i in range(lo, hi) if i % B == e]):
            t = i // B
            mask = 1.0 - s["done"][t, e] if s["last_step"][t, e] else 1.0
            deltas = s["reward"][t, e] + 0.99 * s["next_value"][t, e] * mask - s["value"][t, e]
            last_adv = deltas + 0.99 * 0.95 * last_adv * mask
            ref[i - lo] = last_adv
    assert torch.equal(got, ref)
    if hi - lo <= B:                                     # a window shorter than the stride: chains of one row, the advantage is the delta
        mask = torch.where(flat["last_step"] != 0, 1 - flat["done"], torch.ones_like(flat["done"])).unsqueeze(1)
        assert torch.equal(got, flat["reward"] + 0.99 * flat["next_value"] * mask - flat["value"])
    with pytest.raises(ValueError):
        L.ppo_gae(flat["reward"], flat["value"], flat["next_value"], flat["done"], flat["last_step"], 0, 0.99, 0.95)


def test_the_stride_reaches_get_loss_by_argument_and_by_attribute():
    z, args, tr, b = _load("mappo_plain")
    net = tr.behaviour_net
    assert net.gae_stride == 1 and "gae_stride" not in net.state_dict()
    p1 = float(net.get_loss(b, want=("policy",))[0])
    p3 = float(net.get_loss(b, want=("policy",), stride=3)[0])
    assert abs(p1 - p3) > 1e-4
    net.__dict__["gae_stride"] = 3
    assert float(net.get_loss(b, want=("policy",))[0]) == p3 and float(net.get_loss(b, want=("policy",), stride=1)[0]) == p1
    env = _ToyEnv(4, 3, 5)
    assert PGTrainer(make_alg_args(3, 5, 1, alg="ippo", **TOY), "ippo", env, device="cpu", data_parallel=False).behaviour_net.gae_stride == 4


def test_union_statistics_equal_batchnorm_on_the_concatenation():
    """the helper normalise_reward and the advantage BatchNorm share: with the ranks' (count, sum, sum of squares) added by the
    all-reduce, a rank's output and running statistics are those of BatchNorm1d on the concatenated batch"""
    torch.manual_seed(3)
    n = 3
    mine, theirs = 2.0 * torch.randn(9, n) + 1.0, 0.5 * torch.randn(7, n) - 2.0
    net = PPONet(make_alg_args(n, 5, 1, alg="mappo"), "mappo")
    calls = []

    def fake_all_reduce(st):
        x = theirs.double()
        st += torch.cat((x.new_full((1,), float(x.shape[0])), x.sum(0), (x * x).sum(0)))
        calls.append(1)
    net.__dict__["_dp_all_reduce"] = fake_all_reduce
    for bn_of in (lambda: net.__dict__["_adv_batchnorm"], lambda: net.batchnorm):
        want_bn = torch.nn.BatchNorm1d(n)
        want = want_bn(torch.cat((mine, theirs)))[:9]
        bn = bn_of()
        got = net._union_batchnorm(bn, mine)
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)
        assert torch.allclose(bn.running_mean, want_bn.running_mean, rtol=1e-5, atol=1e-7)
        assert torch.allclose(bn.running_var, want_bn.running_var, rtol=1e-5, atol=1e-7) and int(bn.num_batches_tracked) == 1
    assert len(calls) == 2
    assert torch.allclose(net.normalise_reward(mine), torch.nn.BatchNorm1d(n)(torch.cat((mine, theirs)))[:9], rtol=1e-5, atol=1e-6)     # rewards: as before
    # ... and get_loss sends the advantages through it: one all-reduce for the rewards, one for the advantages
    z, args, tr, b = _load("mappo_shared")
    tr.behaviour_net.__dict__["_dp_all_reduce"] = lambda st: calls.append(2)
    del calls[:]
    tr.behaviour_net.get_loss(b, want=("policy",))
    assert calls == [2, 2]
    del calls[:]
    tr.behaviour_net.get_loss(b, want=("value",))
    assert calls == [2]


def _run_toy(alg, seed=0):
    torch.manual_seed(seed); np.random.seed(seed)
    env = _ToyEnv(4, 3, 5)
    over = dict(TOY, policy_update_epochs=2) if alg in ("mappo", "ippo") else TOY
    tr = PGTrainer(make_alg_args(3, 5, 1, alg=alg if alg in ("mappo", "ippo") else None, **over), alg, env, device="cpu", data_parallel=False)
    seen, recomputed = [], []
    tu = tr.transition_update

    def spy(trans, stat):
        net = tr.behaviour_net
        if tr.ppo:                                        # with the parameters as they are BEFORE this step's update
            with torch.no_grad():
                means, log_stds, _ = net.policy(trans["state"], trans["last_hid"])
                y = trans["action"]
                x = torch.atanh(y.clamp(-1 + 1e-7, 1 - 1e-7))
                lp = torch.distributions.Normal(means, log_stds.exp()).log_prob(x) - torch.log(1 - y.pow(2) + 1e-6)       # util.py:57-66
                recomputed.append(dict(value=net.value(trans["state"]), next_value=net.value(trans["next_state"]), log_prob=lp))
        seen.append({k: v.clone() for k, v in trans.items()})
        tu(trans, stat)
        seen[-1]["ring_after"] = len(tr.replay_buffer)
    tr.transition_update = spy
    stat = {}
    tr.train_process(stat)
    return tr, seen, recomputed, stat


@pytest.mark.parametrize("alg", ["mappo", "ippo"])
def test_trainer_stores_the_three_fields_and_empties_the_ring(alg):
    tr, seen, recomputed, stat = _run_toy(alg)
    assert tr.steps == 12 and len(seen) == 12 and tr.on_policy and tr.ppo
    for trans, want in zip(seen, recomputed):
        for k in ("log_prob", "value", "next_value"):
            assert trans[k].shape == (4, 3, 1) and trans[k].dtype == torch.float32 and not trans[k].requires_grad
        assert torch.equal(trans["value"], want["value"]) and torch.equal(trans["next_value"], want["next_value"])
        assert torch.allclose(trans["log_prob"], want["log_prob"], rtol=1e-3, atol=1e-3)
    assert {"log_prob", "value", "next_value"} <= set(tr.replay_buffer.store)
    assert [s["ring_after"] for s in seen] == [4, 8, 12, 16, 0, 4, 8, 12, 0, 4, 8, 12]           # rounds at steps 4 and 8 empty the ring (model.py:53-56)
    assert not any(k.endswith("_cached") for k in tr.replay_buffer.store) and not tr._cache_targets()
    assert all(isinstance(v, float) and np.isfinite(v) for v in stat.values())
    assert {"mean_train_value_loss", "mean_train_policy_loss", "mean_train_entropy"} <= set(stat)


def test_maddpg_transitions_are_unchanged():
    tr, seen, _, _ = _run_toy("maddpg")
    assert not tr.ppo and not tr.on_policy
    want = {"state", "action", "reward", "next_state", "done", "last_step", "action_avail", "last_hid", "hid", "valid"}
    assert all(set(s) - {"ring_after"} == want for s in seen) and set(tr.replay_buffer.store) == want
    assert PGTrainer(make_alg_args(3, 5, 1, **TOY), "coma", _ToyEnv(4, 3, 5), device="cpu", data_parallel=False).on_policy


def test_trainer_checkpoint_round_trip(tmp_path):
    tr, _, _, _ = _run_toy("mappo")
    p = tmp_path / "model.pt"
    tr.save(p)
    ck = torch.load(p)["model_state_dict"]
    assert not any("adv" in k for k in ck)
    tr2 = PGTrainer(tr.args, "mappo", _ToyEnv(4, 3, 5), device="cpu", data_parallel=False)
    tr2.load(p)
    for k, v in tr.behaviour_net.state_dict().items():
        assert torch.equal(v, tr2.behaviour_net.state_dict()[k])
