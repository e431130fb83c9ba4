#!/usr/bin/env python
"""COMA's counterfactual baseline as one launch (mapdn_critic_head_counterfactual, csrc/critic_cf.hip) against what the kernels without
it can do, at config 5's update batch (32 x 8192 transitions x 38 agents, about 10 M critic rows of 64) with sample_size S = 10:
S x (form x_s = x + delta[s] * act_col as one addcmul into a reused buffer, mapdn_critic_head_forward on it, add to the running sum)
plus the division by S — and, for the variant that also returns v0 = head(x), one more mapdn_critic_head_forward on x.
Device events around each side, one process, warmed up, the two sides alternating; the median of 25 repetitions is the figure.
    python tools/cf_baseline_timing.py [out.txt]
profiles/cf_baseline_timing.txt is its record; DESIGN section 12 quotes it."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mapdn_amd import _lib  # noqa: E402

lib = _lib.load()
dev = torch.device("cuda:0")
nb, n, S = 32 * 8192, 38, 10
rows = nb * n
g = torch.Generator().manual_seed(0)
r = lambda *s, k=1.0: (k * torch.randn(*s, generator=g)).to(dev)      # noqa: E731
x = torch.empty(rows, 64, device=dev)
for lo in range(0, rows, 1 << 20):                                    # (drawn on the host in pieces)
    x[lo:lo + (1 << 20)] = r(min(1 << 20, rows - lo), 64, k=1.2)
col = r(n, 64, k=0.5)
delta = (torch.randn(S, rows, device=dev) - torch.tanh(torch.randn(rows, device=dev))).contiguous()
gam, bet, w2, b2, w3, b3 = 1 + r(64, k=0.3), r(64, k=0.2), r(64, 64, k=0.2), r(64, k=0.1), r(64, k=0.3), r(1, k=0.1)
st = torch.cuda.current_stream(dev).cuda_stream
P = [t.data_ptr() for t in (gam, bet, w2, b2, w3, b3)]
eps = 1e-5
base_k, v0_k, base_l, v0_l, v, xs = tuple(torch.empty(rows, device=dev) for _ in range(5)) + (torch.empty(rows, 64, device=dev),)
x3, xs3, col3, d4 = x.view(nb, n, 64), xs.view(nb, n, 64), col.view(1, n, 64), delta.view(S, nb, n, 1)


def kernel(with_v0):
    assert lib.mapdn_critic_head_counterfactual(x.data_ptr(), n, col.data_ptr(), delta.data_ptr(), S, P[0], P[1], eps, P[2], P[3], P[4], P[5],
                                                base_k.data_ptr(), v0_k.data_ptr() if with_v0 else None, rows, st) == 0


def forward(src, out):
    assert lib.mapdn_critic_head_forward(src.data_ptr(), None, 1, P[0], P[1], eps, P[2], P[3], P[4], P[5], out.data_ptr(), rows, st) == 0


def loop(with_v0):
    base_l.zero_()
    for s in range(S):
        torch.addcmul(x3, d4[s], col3, out=xs3)
        forward(xs, v)
        base_l.add_(v)
    base_l.div_(S)
    if with_v0:
        forward(x, v0_l)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def ab(fa, fb, reps=25):
    for _ in range(3):
        fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(fa)); tb.append(timed(fb))
    return ta, tb


def line(name, t):
    t = sorted(t)
    return f"{name:<58s} median {statistics.median(t):7.3f} ms   min {t[0]:7.3f}   max {t[-1]:7.3f}   p10-p90 {t[len(t) // 10]:7.3f}-{t[-1 - len(t) // 10]:7.3f}"


out = [f"counterfactual baseline: one launch against S x (form, head forward) + mean; {rows} rows (nb = {nb}, n = {n}), S = {S}; "
       f"{torch.cuda.get_device_name(0)} ({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs)",
       "device events around each side, one process, 3 warm-up rounds, 25 alternating repetitions"]
ta, tb = ab(lambda: kernel(False), lambda: loop(False))
out += [line("mapdn_critic_head_counterfactual (baseline only)", ta), line("S x (addcmul, mapdn_critic_head_forward, add) + div", tb)]
ta, tb = ab(lambda: kernel(True), lambda: loop(True))
out += [line("mapdn_critic_head_counterfactual (baseline + v0)", ta), line("the loop + mapdn_critic_head_forward(x)", tb)]
torch.cuda.synchronize()
out.append(f"check: baseline max diff {float((base_k - base_l).abs().max()):.2e} of {float(base_l.abs().max()):.2e}; v0 max diff {float((v0_k - v0_l).abs().max()):.2e}")
print("\n".join(out))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(out) + "\n")
