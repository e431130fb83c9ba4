#!/usr/bin/env python
"""The PPO launches of csrc/ppo.hip (mapdn_ppo_gae, mapdn_ppo_policy_loss, mapdn_ppo_value_loss through learner.ppo_gae /
ppo_policy_loss / ppo_value_loss) against the vectorised PyTorch forms (MAPDN_FUSED_PPO=0) at a training batch: 32 steps x `envs` envs
(chain stride = envs) x n agents, each launch's time against its compulsory traffic.  The GAE reads five [rows, n] f32 tensors and writes
one (done / last_step [rows] are counted too); the policy loss reads six and writes one, the value loss reads four and writes one; a loss is
timed forward + backward (the backward scales the stored gradient).  Device events around each side, one process, 3 warm-up rounds, the
two sides alternating; the median of 9 repetitions is the figure.
    python tools/ppo_kernel_timing.py [out.txt] [envs] [agents]
With a file name the lines are written there as well (DESIGN section 15 names what is to be recorded)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mapdn_amd import learner  # noqa: E402

dev = torch.device("cuda:0")
ENVS = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
N = int(sys.argv[3]) if len(sys.argv) > 3 else 22
STEPS, REPS = 32, 9
rows = STEPS * ENVS


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


torch.manual_seed(0)
r = lambda *s: torch.randn(*s, device=dev)      # noqa: E731
reward, value, next_value, adv0 = r(rows, N), r(rows, N), r(rows, N), r(rows, N)
done, last = (torch.rand(rows, device=dev) < 0.05).float(), (torch.rand(rows, device=dev) < 0.1).float()
valid = torch.rand(rows, device=dev) < 0.9
action, old = torch.tanh(r(rows, N, 1)), -1.0 + 0.5 * r(rows, N, 1)
log_std, avail = torch.zeros(rows, N, 1, device=dev), torch.ones(rows, N, 1, device=dev)
mean = (0.5 * r(rows, N, 1)).requires_grad_(True)
v = r(rows, N).requires_grad_(True)


def gae():
    return learner.ppo_gae(reward, value, next_value, done, last, ENVS, 0.99, 0.95)


def policy():
    loss = learner.ppo_policy_loss(mean, action, log_std, avail, old, adv0, valid, 0.6)
    return loss, torch.autograd.grad(loss, mean)[0]


def value_loss():
    loss = learner.ppo_value_loss(v, value, reward, next_value, done, valid, 0.99, 0.6, 2.0)
    return loss, torch.autograd.grad(loss, v)[0]


work = {"gae": (gae, (6 * rows * N + 2 * rows) * 4), "policy loss + gradient": (policy, (7 * rows * N + rows) * 4),
        "value loss + gradient": (value_loss, (5 * rows * N + 2 * rows) * 4)}
times = {(k, route): [] for k in work for route in ("kernels", "PyTorch")}
results = {}
for rep in range(3 + REPS):
    for k, (fn, _) in work.items():
        for route in ("kernels", "PyTorch"):
            os.environ["MAPDN_FUSED_PPO"] = "1" if route == "kernels" else "0"
            t = timed(fn)
            if rep >= 3:
                times[(k, route)].append(t)
            results[(k, route)] = fn()
os.environ.pop("MAPDN_FUSED_PPO", None)
props = torch.cuda.get_device_properties(0)
out = [f"PPO launches (csrc/ppo.hip) against the vectorised PyTorch forms; rows = {STEPS} steps x {ENVS} envs = {rows}, n = {N} agents, chain stride {ENVS}; "
       f"{torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs)",
       f"device events around each side, one process, 3 warm-up rounds, {REPS} alternating repetitions"]
for (k, route), t in times.items():
    t = sorted(t)
    med = statistics.median(t)
    out.append(f"{k + ', ' + route:<40s} median {med:9.3f} ms   min {t[0]:9.3f}   max {t[-1]:9.3f}   compulsory {work[k][1] / 1e6:8.1f} MB -> {work[k][1] / med / 1e6:8.1f} GB/s")
a, b = results[("gae", "kernels")], results[("gae", "PyTorch")]
out.append(f"check: gae max diff {float((a - b).abs().max()):.2e} of {float(b.abs().max()):.2e}")
for k in ("policy loss + gradient", "value loss + gradient"):
    (la, ga), (lb, gb) = results[(k, "kernels")], results[(k, "PyTorch")]
    out.append(f"check: {k}: loss {float(la):.8e} / {float(lb):.8e}; gradient max diff {float((ga - gb).abs().max()):.2e} of {float(gb.abs().max()):.2e}")
print("\n".join(out))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(out) + "\n")
