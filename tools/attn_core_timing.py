#!/usr/bin/env python
"""MAAC's attention core as HIP launches (mapdn_attention_forward / _backward, csrc/critic_attn.hip, through learner._AttentionCore)
against the batched PyTorch route (learner.attention_core_torch: one masked softmax over [b, H, n, n]) at the end-to-end update batch:
32 x 8192 samples x 38 agents x 64, H = 1 and 4.  Timed per direction: the forward alone (no graph), and the backward alone (the
gradient of sum(out * w) + sum(logit_sq * w_sq) with respect to the three operands, on a graph built outside the timed window).
Device events around each side, one process, 3 warm-up rounds, the two sides alternating; the median of 15 repetitions is the figure.
    python tools/attn_core_timing.py [out.txt] [samples]
profiles/attn_core_timing.txt is its record; DESIGN section 13 quotes it."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mapdn_amd import learner  # noqa: E402

dev = torch.device("cuda:0")
B, n = (int(sys.argv[2]) if len(sys.argv) > 2 else 32 * 8192), 38
REPS = 15


def operands(seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return [(0.5 * torch.randn(B, n, 64, device=dev, generator=g)).requires_grad_(True) for _ in range(3)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def line(name, t):
    t = sorted(t)
    return f"{name:<46s} median {statistics.median(t):8.3f} ms   min {t[0]:8.3f}   max {t[-1]:8.3f}   p10-p90 {t[len(t) // 10]:8.3f}-{t[-1 - len(t) // 10]:8.3f}"


out = [f"attention core: fused HIP launches against the batched PyTorch route; {B} samples x {n} agents x 64; "
       f"{torch.cuda.get_device_name(0)} ({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs)",
       f"device events around each side, one process, 3 warm-up rounds, {REPS} alternating repetitions"]
for H in (1, 4):
    ops = operands(H)
    w_out = torch.randn(B, n, 64, device=dev)
    w_sq = torch.randn(n, H, device=dev) / (B * (n - 1))
    routes = {"fused": lambda: learner._AttentionCore.apply(*ops, H), "batched PyTorch": lambda: learner.attention_core_torch(*ops, H)}

    def fwd(route):
        with torch.no_grad():
            routes[route]()

    def graph(route):
        o, l = routes[route]()
        return (o * w_out).sum() + (l * w_sq).sum()

    def bwd_time(route):
        loss = graph(route)
        torch.cuda.synchronize()
        return timed(lambda: torch.autograd.grad(loss, ops))

    for _ in range(3):
        for r in routes:
            fwd(r); torch.autograd.grad(graph(r), ops)
    torch.cuda.synchronize()
    tf, tb = {r: [] for r in routes}, {r: [] for r in routes}
    for _ in range(REPS):
        for r in routes:
            tf[r].append(timed(lambda: fwd(r)))
        for r in routes:
            tb[r].append(bwd_time(r))
    for r in routes:
        out.append(line(f"H = {H} forward, {r}", tf[r]))
    for r in routes:
        out.append(line(f"H = {H} backward, {r}", tb[r]))
    with torch.no_grad():
        (of, lf), (ot, lt) = routes["fused"](), routes["batched PyTorch"]()
    gf, gt = torch.autograd.grad(graph("fused"), ops), torch.autograd.grad(graph("batched PyTorch"), ops)
    out.append(f"H = {H} check: out max diff {float((of - ot).abs().max()):.2e} of {float(ot.abs().max()):.2e}; logit_sq rel diff "
               f"{float(((lf - lt).abs() / lt.abs()).max()):.2e}; gradients max diff {max(float((a - b).abs().max()) for a, b in zip(gf, gt)):.2e} "
               f"of {max(float(b.abs().max()) for b in gt):.2e}")
    del ops, w_out, of, ot, gf, gt
    torch.cuda.empty_cache()
print("\n".join(out))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(out) + "\n")
