"""SQDDPG on the GPU: the reference fixtures of tests/test_sqddpg.py on cuda:0 at the GPU bars tests/test_coma_gpu.py holds COMA's to (their
hidden size is 8, so the coalition critic takes the factored PyTorch route on the device); the fused route — hidden size 64, 3 and 38
agents, 1 and 10 coalition draws, 64 samples — against the same batch, the same coalitions and the same start with MAPDN_FUSED_SHAP=0:
losses, stats and the state_dict after one value step, one policy step and one target update, with the launch counter showing which
route ran; and three end-to-end episodes on the 33-bus net.

The on/off bars.  Both routes are float32 in different orders of summation; the kernel matrix holds the fused route's gradients to 4 x the
factored route's own error, i.e. the two differ by a few 1e-6 of a gradient's scale times the square root of the summed terms
(b S n <= 24 320 rows: about 1e-3 relative at the worst).  Losses and stats: rtol 2e-3, atol 2e-6.  Parameters: the first RMSprop step
is lr g / (0.1 |g| + 1e-5), at most 10 lr = 1e-3 whatever the gradient's size, so a relative gradient difference d moves it by at most
1e-3 d where the gradient is large and by 10 |dg| where it is tiny: the MOVE is compared at rtol 1e-2 with atol 1e-5 (1 % of the step) —
the bars tests/test_maac_gpu.py and tests/test_coma_gpu.py hold the same comparison to."""
import numpy as np
import pytest
import torch

from mapdn_amd import learner
from mapdn_amd.learner import PGTrainer, make_alg_args
from tests import test_sqddpg as ts

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(ts.VARIANTS))
def test_forward_and_losses_match_reference_on_gpu(name):
    ts.check_forward_and_losses(name, "cuda:0", rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("name", list(ts.VARIANTS))
def test_update_steps_match_reference_on_gpu(name):
    ts.check_update_steps(name, "cuda:0", rtol=1e-4, atol=1e-5, move_rtol=1e-2, move_atol=1e-5)


def _trainer_and_batch(n, S, o=12, bs=64, seed=0, **over):
    dev = "cuda:0"
    torch.manual_seed(seed)
    args = make_alg_args(n, o, 1, alg="sqddpg", sample_size=S, **over)
    tr = PGTrainer(args, "sqddpg", env=None, device=dev, data_parallel=False)
    with torch.no_grad():
        for p in tr.behaviour_net.parameters():
            p.add_(0.1 * torch.randn_like(p))
    r = lambda *s: torch.randn(*s, device=dev)      # noqa: E731
    net = tr.behaviour_net
    batch = dict(state=r(bs, n, o), action=torch.tanh(r(bs, n, 1)), reward=r(bs, 1).expand(bs, n).contiguous(), next_state=r(bs, n, o),
                 done=(torch.rand(bs, 1, device=dev) < 0.2).float(), action_avail=torch.ones(bs, n, 1, device=dev), last_hid=0.3 * r(bs, n, 64),
                 hid=0.3 * r(bs, n, 64), coalitions=torch.stack([net.sample_coalitions(bs, dev) for _ in range(3)]))
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


@pytest.mark.parametrize("n,S,over", [(3, 1, dict()), (3, 10, dict()), (38, 1, dict()), (38, 10, dict()), (3, 10, dict(normalize_advantages=True, double_q=False))],
                         ids=["n3-s1", "n3-s10", "n38-s1", "n38-s10", "n3-s10-advnorm-target-policy"])
def test_fused_route_against_the_factored_route(monkeypatch, n, S, over):
    tr, batch = _trainer_and_batch(n, S, **over)
    init = {k: v.clone() for k, v in tr.behaviour_net.state_dict().items()}
    monkeypatch.delenv("MAPDN_FUSED_SHAP", raising=False)
    c0 = learner._ShapleyCritic.launches
    pl, vl, stat, final = _one_round(tr, batch, init)
    fused_calls = learner._ShapleyCritic.launches - c0
    assert fused_calls == 3 + 2 + 1 + (1 if over.get("normalize_advantages") else 0)      # get_loss: three; a value step: two; a policy step: one (+ the
    monkeypatch.setenv("MAPDN_FUSED_SHAP", "0")                                           # advantages that `batchnorm` sees in the value step)
    pl_ref, vl_ref, stat_ref, final_ref = _one_round(tr, batch, init)
    assert learner._ShapleyCritic.launches == c0 + fused_calls
    print(f"[sqddpg gpu] n={n} S={S} policy loss fused {pl:.8e} factored {pl_ref:.8e}; value loss fused {vl:.8f} factored {vl_ref:.8f}; {fused_calls} fused forwards")
    assert np.isfinite(pl_ref) and np.isfinite(vl_ref)
    assert np.allclose(pl, pl_ref, rtol=2e-3, atol=2e-6) and np.allclose(vl, vl_ref, rtol=2e-3, atol=2e-6)
    for k, v in stat_ref.items():
        print(f"[sqddpg gpu] n={n} S={S} {k}: fused {stat[k]:.8e} factored {v:.8e}")
        assert np.allclose(stat[k], v, rtol=2e-3, atol=2e-6), (k, stat[k], v)
    moved, worst = 0, 0.0
    for k, v in final_ref.items():
        if k.endswith("num_batches_tracked"):
            assert int(final[k]) == int(v), k
            continue
        a, b, i = final[k].cpu().numpy(), v.cpu().numpy(), init[k].cpu().numpy()
        moved += int(np.abs(b - i).max() > 0)
        worst = max(worst, float(np.abs(a - b).max()))
        assert np.allclose(a - i, b - i, rtol=1e-2, atol=1e-5), (k, np.abs(a - b).max())
    print(f"[sqddpg gpu] n={n} S={S} largest parameter difference after the round {worst:.3e}; {moved} entries moved")
    assert moved > 20


def test_end_to_end_episodes():
    """three episodes of 240 steps on the 33-bus net (6 agents) at 64 envs, an update round every 60 steps: the coalition kernels are
    reached, the losses and every parameter are finite and the ring is kept between the rounds"""
    from mapdn_amd import e2e
    c0 = learner._ShapleyCritic.launches
    seen = {}
    init = PGTrainer.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        seen["trainer"] = self
    PGTrainer.__init__ = spy
    try:
        lines = e2e.run(case="case33", envs=64, alg="sqddpg", episodes=3)
    finally:
        PGTrainer.__init__ = init
    assert len(lines) == 3 and lines[0]["alg"] == "sqddpg"
    for line in lines:
        for k in ("mean_train_reward", "mean_train_value_loss", "mean_train_policy_loss", "env_steps_per_s"):
            assert np.isfinite(line[k]), (k, line)
    assert lines[-1]["replay_transitions"] >= 60 * 64, lines[-1]
    assert learner._ShapleyCritic.launches > c0
    tr = seen["trainer"]
    assert len(tr.replay_buffer) > 0
    assert all(bool(torch.isfinite(v).all()) for v in tr.behaviour_net.state_dict().values() if v.is_floating_point())
