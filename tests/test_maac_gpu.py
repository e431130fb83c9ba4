"""MAAC on the GPU: the reference fixtures of tests/test_maac.py on cuda:0 at the GPU bars tests/test_coma_gpu.py holds COMA's to (their
hidden size is 8, so the attention takes the batched PyTorch route on the device); the fused route — hidden size 64, 38 agents, 1 and 4
heads — against the same batch and the same start with MAPDN_FUSED_ATTN=0: losses, stats and the state_dict after one value step, one
policy step and one target update within the on/off bars of tests/test_coma_gpu.py, with the launch counter showing which route ran; and
three end-to-end episodes on the 33-bus net."""
import numpy as np
import pytest
import torch

from mapdn_amd import learner
from mapdn_amd.learner import PGTrainer, make_alg_args
from tests import test_maac as tm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(tm.VARIANTS))
def test_forward_and_losses_match_reference_on_gpu(name):
    tm.check_forward_and_losses(name, "cuda:0", rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("name", list(tm.VARIANTS))
def test_update_steps_match_reference_on_gpu(name):
    tm.check_update_steps(name, "cuda:0", rtol=1e-4, atol=1e-5, move_rtol=1e-2, move_atol=1e-5)


def _trainer_and_batch(H, n=38, o=82, bs=64, seed=0, **over):
    dev = "cuda:0"
    torch.manual_seed(seed)
    args = make_alg_args(n, o, 1, alg="maac", attend_heads=H, **over)
    tr = PGTrainer(args, "maac", env=None, device=dev, data_parallel=False)
    with torch.no_grad():
        for p in tr.behaviour_net.parameters():
            p.add_(0.1 * torch.randn_like(p))
    r = lambda *s: torch.randn(*s, device=dev)      # noqa: E731
    batch = dict(state=r(bs, n, o), action=torch.tanh(r(bs, n, 1)), reward=r(bs, 1).expand(bs, n).contiguous(), next_state=r(bs, n, o),
                 done=(torch.rand(bs, 1, device=dev) < 0.2).float(), action_avail=torch.ones(bs, n, 1, device=dev), last_hid=0.3 * r(bs, n, 64),
                 hid=0.3 * r(bs, n, 64), noise=r(bs, n, 1), next_noise=r(bs, n, 1))
    return tr, batch


def _one_round(tr, batch, init):
    net = tr.behaviour_net
    net.load_state_dict(init)
    tr.policy_optimizer.state.clear(); tr.value_optimizer.state.clear()
    pl, vl, _ = net.get_loss(batch)
    stat = {}
    tr.value_transition_process(stat, batch)
    tr.policy_transition_process(stat, batch)
    net.update_target()
    return float(pl.detach()), float(vl.detach()), {k: float(v) for k, v in stat.items()}, {k: v.clone() for k, v in net.state_dict().items()}


@pytest.mark.parametrize("H,over", [(1, dict()), (4, dict()), (2, dict(normalize_advantages=True, soft=False))], ids=["h1", "h4", "h2-advnorm-nosoft"])
def test_fused_route_against_the_batched_route(monkeypatch, H, over):
    tr, batch = _trainer_and_batch(H, **over)
    init = {k: v.clone() for k, v in tr.behaviour_net.state_dict().items()}
    monkeypatch.delenv("MAPDN_FUSED_ATTN", raising=False)
    c0 = learner._AttentionCore.launches
    pl, vl, stat, final = _one_round(tr, batch, init)
    fused_calls = learner._AttentionCore.launches - c0
    assert fused_calls >= 3 + 2 + 2                      # get_loss: three value() calls; a value step and a policy step: at least two each
    monkeypatch.setenv("MAPDN_FUSED_ATTN", "0")
    pl_ref, vl_ref, stat_ref, final_ref = _one_round(tr, batch, init)
    assert learner._AttentionCore.launches == c0 + fused_calls
    print(f"[maac gpu] H={H} policy loss fused {pl:.8e} batched {pl_ref:.8e}; value loss fused {vl:.8f} batched {vl_ref:.8f}; {fused_calls} fused forwards")
    assert np.isfinite(pl_ref) and np.isfinite(vl_ref)
    assert np.allclose(pl, pl_ref, rtol=2e-3, atol=2e-6) and np.allclose(vl, vl_ref, rtol=2e-3, atol=2e-6)
    for k, v in stat_ref.items():
        assert np.allclose(stat[k], v, rtol=2e-3, atol=2e-6), (k, stat[k], v)
    moved = 0
    for k, v in final_ref.items():
        if k.endswith("num_batches_tracked"):
            assert int(final[k]) == int(v), k
            continue
        a, b, i = final[k].cpu().numpy(), v.cpu().numpy(), init[k].cpu().numpy()
        moved += int(np.abs(b - i).max() > 0)
        assert np.allclose(a - i, b - i, rtol=1e-2, atol=1e-5), (k, np.abs(a - b).max())
    assert moved > 20


def test_end_to_end_episodes():
    """three episodes of 240 steps on the 33-bus net (6 agents), an update round every 60 steps: the fused attention is reached, the losses
    are finite and the ring is kept between the rounds"""
    from mapdn_amd import e2e
    c0 = learner._AttentionCore.launches
    lines = e2e.run(case="case33", envs=64, alg="maac", episodes=3)
    assert len(lines) == 3 and lines[0]["alg"] == "maac"
    for line in lines:
        for k in ("mean_train_reward", "mean_train_value_loss", "mean_train_policy_loss", "env_steps_per_s"):
            assert np.isfinite(line[k]), (k, line)
    assert lines[-1]["replay_transitions"] >= 60 * 64, lines[-1]
    assert learner._AttentionCore.launches > c0
