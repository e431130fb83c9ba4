"""MATD3 on the GPU through its fused routes: get_loss on a tall batch with fixed smoothing noise — the default (mapdn_critic_twin_forward
for the target's min, two mapdn_critic_head_mse launches for the loss) and MAPDN_TWIN_MSE_KERNEL=1 (mapdn_critic_twin_mse, one launch) —
against the route without them (MAPDN_FUSED_TWIN=0: the single-head kernels under autograd / PyTorch), within the bars tests/test_critic_head.py holds the single
head's fused loss to (loss 3e-6 of max(1, |loss|), every parameter gradient 2e-4 of its maximum); and one end-to-end episode that reaches both
default launches, counted through the wrappers."""
import numpy as np
import pytest
import torch

from mapdn_amd import learner
from mapdn_amd.learner import DDPGNet, make_alg_args

pytestmark = pytest.mark.gpu


def _net_and_batch(n=38, o=20, bs=512, seed=0):
    dev = "cuda:0"
    torch.manual_seed(seed)
    args = make_alg_args(n, o, 1)
    net = DDPGNet(args, "matd3", DDPGNet(args, "matd3")).to(dev)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.1 * torch.randn_like(p))
    r = lambda *s: torch.randn(*s, device=dev)      # noqa: E731
    batch = dict(state=r(bs, n, o), action=torch.tanh(r(bs, n, 1)), reward=r(bs, 1).expand(bs, n).contiguous(), next_state=r(bs, n, o),
                 done=(torch.rand(bs, 1, device=dev) < 0.2).float(), action_avail=torch.ones(bs, n, 1, device=dev), last_hid=0.3 * r(bs, n, 64),
                 hid=0.3 * r(bs, n, 64), next_noise=r(bs, n, 1), valid=torch.rand(bs, device=dev) < 0.8)
    return net, batch


def _value_grads(net, batch):
    net.zero_grad()
    state = {k: v.clone() for k, v in net.batchnorm.state_dict().items()}
    _, vl, _ = net.get_loss(batch, want=("value",))
    vl.backward()
    net.batchnorm.load_state_dict(state)
    return float(vl.detach()), {k: p.grad.clone() for k, p in net.value_dicts.named_parameters()}


def _counts():
    return learner.critic_twin_forward.launches, learner.twin_pair_mse.launches, learner._CriticTwinMSE.launches


@pytest.mark.parametrize("kernel", ["pair", "twin_mse"])
@pytest.mark.parametrize("masked", [False, True])
def test_get_loss_through_the_twin_kernels(monkeypatch, masked, kernel):
    net, batch = _net_and_batch()
    if not masked:
        batch.pop("valid")
    monkeypatch.delenv("MAPDN_FUSED_TWIN", raising=False)
    monkeypatch.delenv("MAPDN_TWIN_MSE_KERNEL", raising=False)
    if kernel == "twin_mse":
        monkeypatch.setenv("MAPDN_TWIN_MSE_KERNEL", "1")
    f0, p0, m0 = _counts()
    loss, grads = _value_grads(net, batch)
    after = (f0 + 1, p0 + (kernel == "pair"), m0 + (kernel == "twin_mse"))                # target min + the loss route asked for
    assert _counts() == after
    monkeypatch.setenv("MAPDN_FUSED_TWIN", "0")
    loss_ref, grads_ref = _value_grads(net, batch)
    assert _counts() == after
    print(f"[matd3 gpu] value loss twin {loss:.8f} reference route {loss_ref:.8f}")
    assert abs(loss - loss_ref) <= 3e-6 * max(1.0, abs(loss_ref))
    assert set(grads) == set(grads_ref)
    for k, g in grads.items():
        err, mx = float((g - grads_ref[k]).abs().max()), float(grads_ref[k].abs().max())
        print(f"[matd3 gpu] d {k}: err {err:.3e} of max {mx:.3e}")
        assert err <= 2e-4 * mx, (k, err, mx)
    with torch.no_grad():                                    # value(): [2b, n, 1] from one forward launch == the other route
        monkeypatch.delenv("MAPDN_FUSED_TWIN")
        f0 = f0 + 1
        v = net.value(batch["state"], batch["action"])
        monkeypatch.setenv("MAPDN_FUSED_TWIN", "0")
        v_ref = net.value(batch["state"], batch["action"])
    assert v.shape == (2 * batch["state"].shape[0], 38, 1) and learner.critic_twin_forward.launches == f0 + 1
    assert float((v - v_ref).abs().max()) <= 2e-6 * max(1.0, float(v_ref.abs().max()))


def test_end_to_end_episode_reaches_the_twin_kernels(monkeypatch):
    from mapdn_amd import e2e
    monkeypatch.delenv("MAPDN_FUSED_TWIN", raising=False)
    monkeypatch.delenv("MAPDN_TWIN_MSE_KERNEL", raising=False)
    f0, p0, m0 = _counts()
    lines = e2e.run(case="case33", envs=64, alg="matd3", episodes=1)
    assert len(lines) == 1 and lines[0]["alg"] == "matd3"
    for k in ("mean_train_reward", "mean_train_value_loss", "mean_train_policy_loss", "env_steps_per_s"):
        assert np.isfinite(lines[0][k]), (k, lines[0])
    f1, p1, m1 = _counts()
    assert f1 > f0 and p1 > p0 and m1 == m0          # the twin forward for the target, the pair of head-loss launches for the loss
