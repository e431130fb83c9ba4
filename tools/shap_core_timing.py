#!/usr/bin/env python
"""SQDDPG's coalition critic as HIP launches (mapdn_critic_shapley_forward / _backward, csrc/critic_shap.hip, through
learner._ShapleyCritic) against the factored PyTorch route (learner.shapley_first_layer: cumsum + gather, then the critic's trunk, which
on the GPU is the one-launch critic head on the materialised [b S n, 64] rows) at n = 38 agents and S = 10 coalition draws.  The batch is
the largest power of two at which the PyTorch route's forward + backward still fits the card: tried from 2^18 samples downwards, the
first that does not run out of memory is used for both routes and stated in the output.  Timed per direction: the forward alone (no
graph), and the backward alone (the gradient of sum(v * w) with respect to base, the id / action columns, the trunk's parameters and the
actions, on a graph built outside the timed window).  Device events around each side, one process, 3 warm-up rounds, the two sides
alternating; the median of 9 repetitions is the figure.
    python tools/shap_core_timing.py [out.txt] [largest log2 of the batch to try]
profiles/shap_core_timing.txt is its record; DESIGN section 14 quotes it."""
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mapdn_amd import learner  # noqa: E402

dev = torch.device("cuda:0")
n, S, REPS = 38, 10, 9
TOP = int(sys.argv[2]) if len(sys.argv) > 2 else 18


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def line(name, t):
    t = sorted(t)
    return f"{name:<34s} median {statistics.median(t):9.3f} ms   min {t[0]:9.3f}   max {t[-1]:9.3f}"


torch.manual_seed(0)
cr = learner.MLPCritic(64, 1, learner.make_alg_args(n, 8, 1, alg="sqddpg")).to(dev)      # only its trunk is used
ln = cr.layernorm
cols = [(0.3 * torch.randn(n, 64, device=dev)).requires_grad_(True) for _ in range(2)]


def operands(b):
    base = torch.randn(b, 64, device=dev).requires_grad_(True)
    act = torch.tanh(torch.randn(b, n, device=dev)).requires_grad_(True)
    pos = learner.sample_coalition_positions(b * S, n, dev).view(b, S, n)
    return base, act, pos, pos.to(torch.int32).contiguous(), torch.randn(b, S, n, device=dev)


def fused(base, act, pos, pos32, w):
    return learner._ShapleyCritic.apply(act, base, cols[0], cols[1], pos32, ln.weight, ln.bias, ln.eps, cr.fc2.weight, cr.fc2.bias, cr.fc3.weight, cr.fc3.bias)


def factored(base, act, pos, pos32, w):
    x = learner.shapley_first_layer(base, cols[0], cols[1], act, pos)
    return cr.trunk(x.reshape(-1, 64))[0].view(pos.shape)


def leaves(ops):
    return [ops[0], ops[1], cols[0], cols[1], ln.weight, ln.bias, cr.fc2.weight, cr.fc2.bias, cr.fc3.weight, cr.fc3.bias]


b, ops = None, None
for lg in range(TOP, 5, -1):
    try:
        ops = operands(1 << lg)
        torch.autograd.grad((factored(*ops) * ops[4]).sum(), leaves(ops))
        torch.cuda.synchronize()
        b = 1 << lg
        break
    except torch.OutOfMemoryError:
        ops = None
        torch.cuda.empty_cache()
assert b is not None
props = torch.cuda.get_device_properties(0)
out = [f"coalition critic: fused HIP launches against the factored PyTorch route; n = {n}, S = {S}, batch {b} = 2^{b.bit_length() - 1} samples "
       f"({b * S * n} rows; the largest power of two <= 2^{TOP} at which the PyTorch route's forward + backward fits {props.total_memory / 2 ** 30:.0f} GiB); "
       f"{torch.cuda.get_device_name(0)} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs, clock {getattr(props, 'clock_rate', 0) / 1e3:.0f} MHz max)",
       f"device events around each side, one process, 3 warm-up rounds, {REPS} alternating repetitions"]
routes = {"fused": fused, "factored PyTorch": factored}
for _ in range(3):
    for r in routes.values():
        torch.autograd.grad((r(*ops) * ops[4]).sum(), leaves(ops))
torch.cuda.synchronize()
tf, tb = {r: [] for r in routes}, {r: [] for r in routes}
for _ in range(REPS):
    for name, r in routes.items():
        with torch.no_grad():
            tf[name].append(timed(lambda: r(*ops)))
    for name, r in routes.items():
        loss = (r(*ops) * ops[4]).sum()
        torch.cuda.synchronize()
        tb[name].append(timed(lambda: torch.autograd.grad(loss, leaves(ops))))
        del loss
for name in routes:
    out.append(line(f"forward, {name}", tf[name]))
for name in routes:
    out.append(line(f"backward, {name}", tb[name]))
mf, mb = {k: statistics.median(v) for k, v in tf.items()}, {k: statistics.median(v) for k, v in tb.items()}
out.append(f"fused / factored: forward {mf['fused'] / mf['factored PyTorch']:.3f}, backward {mb['fused'] / mb['factored PyTorch']:.3f} (the bar: below 1 in both)")
with torch.no_grad():
    vf, vt = fused(*ops), factored(*ops)
gf = torch.autograd.grad((fused(*ops) * ops[4]).sum(), leaves(ops))
gt = torch.autograd.grad((factored(*ops) * ops[4]).sum(), leaves(ops))
out.append(f"check: v max diff {float((vf - vt).abs().max()):.2e} of {float(vt.abs().max()):.2e}; gradients, largest diff relative to the gradient's largest entry "
           f"{max(float((a - c).abs().max() / c.abs().max()) for a, c in zip(gf, gt)):.2e}")
print("\n".join(out))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(out) + "\n")
