"""MAPPO / IPPO on the GPU: the reference fixtures of tests/test_ppo.py on cuda:0 through the fused route (the GAE and both losses from
csrc/ppo.hip) at the GPU bars tests/test_coma_gpu.py holds COMA's to; get_loss on one mid-size batch (4 steps x 16 envs, 6 agents, chain
stride 16) through the kernels against MAPDN_FUSED_PPO=0 — both losses and every parameter gradient, within the on/off bar of
tests/test_coma_gpu.py (rtol 2e-3, atol 2e-6: the two routes differ by expf / logf and the order of the loss sum only) —; and a
two-episode trainer run on the 33-bus env that reaches the kernels, stores the three new fields, empties the ring after its update round
and gives the same bits when run again from the same seeds."""
import numpy as np
import pytest
import torch

from mapdn_amd import learner
from mapdn_amd.learner import PGTrainer, PPONet, make_alg_args
from tests import test_ppo as tp

pytestmark = pytest.mark.gpu


def _counts():
    return learner.ppo_gae.launches, learner._PPOPolicyLoss.launches, learner._PPOValueLoss.launches


@pytest.mark.parametrize("name", tp.NAMES)
def test_forward_and_losses_match_reference_on_gpu(name, monkeypatch):
    monkeypatch.delenv("MAPDN_FUSED_PPO", raising=False)
    c0 = _counts()
    tp.check_forward_and_losses(name, "cuda:0", rtol=1e-4, atol=1e-5)
    c1 = _counts()
    assert all(b > a for a, b in zip(c0, c1)), (c0, c1)               # the fused route: every kernel was reached


@pytest.mark.parametrize("name", tp.NAMES)
def test_update_steps_match_reference_on_gpu(name, monkeypatch):
    monkeypatch.delenv("MAPDN_FUSED_PPO", raising=False)
    tp.check_update_steps(name, "cuda:0", rtol=1e-4, atol=1e-5, move_rtol=1e-2, move_atol=1e-5)


def _net_and_batch(alg, n=6, o=20, steps=4, envs=16, seed=0, **over):
    dev = "cuda:0"
    torch.manual_seed(seed)
    bs = steps * envs
    args = make_alg_args(n, o, 1, alg=alg, **over)
    net = PPONet(args, alg, PPONet(args, alg)).to(dev)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.1 * torch.randn_like(p))
    r = lambda *s: torch.randn(*s, device=dev)      # noqa: E731
    avail = torch.ones(bs, n, 1, device=dev)
    avail[5, 2] = 0.0
    done = (torch.rand(bs, 1, device=dev) < 0.2).float()
    last = torch.maximum((torch.rand(bs, 1, device=dev) < 0.2).float(), torch.cat((torch.zeros(bs - envs, 1, device=dev), torch.ones(envs, 1, device=dev))))
    batch = dict(state=r(bs, n, o), action=torch.tanh(r(bs, n, 1)), reward=r(bs, 1).expand(bs, n).contiguous(), next_state=r(bs, n, o), done=done,
                 last_step=last, action_avail=avail, last_hid=0.3 * r(bs, n, 64), hid=0.3 * r(bs, n, 64), log_prob=-1.0 + 0.5 * r(bs, n, 1),
                 value=r(bs, n, 1), next_value=r(bs, n, 1), valid=torch.rand(bs, device=dev) < 0.8)
    return net, batch


def _losses_and_grads(net, batch, stride):
    net.zero_grad()
    state = {k: v.clone() for k, v in net.batchnorm.state_dict().items()}
    pl, vl, _ = net.get_loss(batch, stride=stride)
    (pl + vl).backward()
    net.batchnorm.load_state_dict(state)
    grads = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None and not k.startswith("target_net")}
    return float(pl.detach()), float(vl.detach()), grads


@pytest.mark.parametrize("alg,over", [("mappo", dict()), ("ippo", dict()), ("mappo", dict(ppo_old_log_prob="stored", normalize_advantages=False))],
                         ids=["mappo", "ippo", "mappo-stored"])
def test_get_loss_through_the_kernels_against_the_pytorch_route(monkeypatch, alg, over):
    net, batch = _net_and_batch(alg, **over)
    monkeypatch.delenv("MAPDN_FUSED_PPO", raising=False)
    c0 = _counts()
    pl, vl, grads = _losses_and_grads(net, batch, 16)
    assert _counts() == tuple(c + 1 for c in c0)
    monkeypatch.setenv("MAPDN_FUSED_PPO", "0")
    pl_ref, vl_ref, grads_ref = _losses_and_grads(net, batch, 16)
    assert _counts() == tuple(c + 1 for c in c0)
    print(f"[ppo gpu] {alg} policy loss kernels {pl:.8e} torch {pl_ref:.8e}; value loss kernels {vl:.8f} torch {vl_ref:.8f}")
    assert np.allclose(pl, pl_ref, rtol=2e-3, atol=2e-6) and np.allclose(vl, vl_ref, rtol=2e-3, atol=2e-6)
    assert set(grads) == set(grads_ref)
    assert any(k.startswith("policy_dicts") and float(g.abs().max()) > 0 for k, g in grads_ref.items())
    assert any(k.startswith("value_dicts") and float(g.abs().max()) > 0 for k, g in grads_ref.items())
    for k, g in grads.items():
        err = float((g - grads_ref[k]).abs().max())
        print(f"[ppo gpu] d {k}: err {err:.3e} of max {float(grads_ref[k].abs().max()):.3e}")
        assert np.allclose(g.cpu().numpy(), grads_ref[k].cpu().numpy(), rtol=2e-3, atol=2e-6), (k, err)
    pl_s1, _, _ = _losses_and_grads(net, batch, 1)                     # (the stride matters on this batch)
    assert abs(pl_s1 - pl_ref) > 1e-5


def _train_two_episodes(alg="mappo", envs=8, max_steps=12):
    from mapdn_amd.env import VoltageControlBatch
    from mapdn_amd.netspec import make_case
    dev = torch.device("cuda:0")
    torch.manual_seed(1); np.random.seed(1)
    net, prof = make_case("case33")
    env = VoltageControlBatch(net, prof, dict(episode_limit=max_steps, action_scale=0.8, action_bias=0.0, voltage_barrier_type="bowl", seed=0),
                              n_envs=envs, device=dev, copy=True)
    try:
        args = make_alg_args(env.n_agents, env.obs_size, env.n_actions, 0.8, 0.0, alg=alg, max_steps=max_steps, behaviour_update_freq=max_steps,
                             batch_size=32, num_eval_episodes=envs)
        tr = PGTrainer(args, alg, env, device=dev)
        ring, stats = [], []
        tu = tr.transition_update

        def spy(trans, stat):
            assert {"log_prob", "value", "next_value"} <= set(trans) and all(trans[k].shape == (envs, env.n_agents, 1) for k in ("log_prob", "value", "next_value"))
            tu(trans, stat)
            ring.append(len(tr.replay_buffer))
        tr.transition_update = spy
        for _ in range(2):
            stat = {}
            tr.train_process(stat)
            stats.append(stat)
        torch.cuda.synchronize()
        return tr, ring, stats, {k: v.clone() for k, v in tr.behaviour_net.state_dict().items()}
    finally:
        env.close()


def test_two_episode_trainer_run_is_finite_clears_the_ring_and_repeats_bit_for_bit(monkeypatch):
    monkeypatch.delenv("MAPDN_FUSED_PPO", raising=False)
    c0 = _counts()
    tr, ring, stats, sd = _train_two_episodes()
    assert tr.behaviour_net.gae_stride == 8 and tr.steps == 24
    # one update round, at step 12 (the first step of the second episode): the ring held 13 steps x 8 envs, and is empty after it
    assert ring == [8 * (t + 1) for t in range(12)] + [0] + [8 * (t + 1) for t in range(11)], ring
    assert {"log_prob", "value", "next_value"} <= set(tr.replay_buffer.store)
    c1 = _counts()
    assert c1[0] >= c0[0] + 10 and c1[1] >= c0[1] + 10 and c1[2] >= c0[2] + 10             # ten policy and ten value epochs through the kernels
    for k in ("mean_train_value_loss", "mean_train_policy_loss", "mean_train_reward"):
        assert np.isfinite(stats[1][k]), (k, stats[1])
    assert all(bool(torch.isfinite(v).all()) for v in sd.values() if v.is_floating_point())
    tr2, ring2, stats2, sd2 = _train_two_episodes()
    assert ring2 == ring and stats2 == stats
    for k, v in sd.items():
        assert torch.equal(v, sd2[k]), k
