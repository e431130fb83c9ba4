#!/usr/bin/env python
"""The twin critic launches (csrc/critic_twin.hip) against the pairs of single-head launches they stand for, at config 5's shape
(nb = 32 x 8192 batch elements, n = 38 agents, about 10 M formed rows): mapdn_critic_twin_mse against two mapdn_critic_head_mse (the
second on per_n + flag_col, each with half the weight), mapdn_critic_twin_forward(vmin) against two mapdn_critic_head_forward plus the
elementwise minimum.  Device events around each side, one process, warmed up, the two sides alternating.
    python tools/twin_head_timing.py [out.txt]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/twin_head_timing.py      (kernel statistics, in a run of its own)
profiles/twin_head_timing.txt and profiles/twin_head_kernel_stats.txt are its records; DESIGN section 11 quotes them."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mapdn_amd import _lib  # noqa: E402

lib = _lib.load()
dev = torch.device("cuda:0")
nb, n = 32 * 8192, 38
rows = nb * n
g = torch.Generator().manual_seed(0)
r = lambda *s, k=1.0: (k * torch.randn(*s, generator=g)).to(dev)      # noqa: E731
base, pern, flag, ret = r(nb, 64, k=1.2), r(n, 64, k=0.8), r(64, k=0.7), r(rows)
pern2 = (pern + flag).contiguous()
gam, bet, w2, b2, w3, b3 = 1 + r(64, k=0.3), r(64, k=0.2), r(64, 64, k=0.2), r(64, k=0.1), r(64, k=0.3), r(1, k=0.1)
wrow = (torch.rand(nb, generator=g) < 0.9).float().to(dev)
scale = (1.0 / (wrow.sum() * n)).reshape(1)
half = scale * 0.5
st = torch.cuda.current_stream(dev).cuda_stream
P = [t.data_ptr() for t in (gam, bet, w2, b2, w3, b3)]
eps = 1e-5
dbase, dx1, dx2 = (torch.empty(nb, 64, device=dev) for _ in range(3))
gt = torch.empty(4480 + n * 64, device=dev)
g1, g2 = (torch.empty(4416 + n * 64, device=dev) for _ in range(2))
st_t = torch.empty(lib.mapdn_critic_twin_scratch_floats(rows, n), device=dev)
s1 = torch.empty(lib.mapdn_critic_head_scratch_floats(rows, n, 1), device=dev)
v1, v2, vm, vm2 = (torch.empty(rows, device=dev) for _ in range(4))


def twin_mse():
    assert lib.mapdn_critic_twin_mse(ret.data_ptr(), wrow.data_ptr(), scale.data_ptr(), base.data_ptr(), pern.data_ptr(), n, flag.data_ptr(), P[0], P[1], eps,
                                     P[2], P[3], P[4], P[5], dbase.data_ptr(), gt.data_ptr(), st_t.data_ptr(), rows, st) == 0


def pair_mse():
    for pn, dx, gg in ((pern, dx1, g1), (pern2, dx2, g2)):
        assert lib.mapdn_critic_head_mse(ret.data_ptr(), wrow.data_ptr(), half.data_ptr(), base.data_ptr(), pn.data_ptr(), n, P[0], P[1], eps, P[2], P[3], P[4],
                                         P[5], dx.data_ptr(), gg.data_ptr(), s1.data_ptr(), rows, st) == 0


def twin_fwd():
    assert lib.mapdn_critic_twin_forward(base.data_ptr(), pern.data_ptr(), n, flag.data_ptr(), P[0], P[1], eps, P[2], P[3], P[4], P[5], None, None, vm.data_ptr(),
                                         rows, st) == 0


def pair_fwd():
    for pn, v in ((pern, v1), (pern2, v2)):
        assert lib.mapdn_critic_head_forward(base.data_ptr(), pn.data_ptr(), n, P[0], P[1], eps, P[2], P[3], P[4], P[5], v.data_ptr(), rows, st) == 0
    torch.minimum(v1, v2, out=vm2)


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
    return f"{name:<44s} median {statistics.median(t):7.3f} ms   min {t[0]:7.3f}   max {t[-1]:7.3f}   p10-p90 {t[len(t) // 10]:7.3f}-{t[-1 - len(t) // 10]:7.3f}"


out = [f"twin critic head against the pair of single-head launches; nb = {nb}, n = {n} ({rows} formed rows); {torch.cuda.get_device_name(0)} ({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs)",
       "device events around each side, one process, 3 warm-up rounds, 25 alternating repetitions"]
ta, tb = ab(twin_mse, pair_mse)
out += [line("mapdn_critic_twin_mse (k_twin_mse)", ta), line("2 x mapdn_critic_head_mse (library's choice)", tb)]
ta, tb = ab(twin_fwd, pair_fwd)
out += [line("mapdn_critic_twin_forward (vmin only)", ta), line("2 x mapdn_critic_head_forward + minimum", tb)]
torch.cuda.synchronize()
out.append(f"check: loss twin {float(gt[4353]):.7f} pair {float(g1[4353] + g2[4353]):.7f}; vmin max diff {float((vm - vm2).abs().max()):.2e}; "
           f"dbase max diff {float((dbase - dx1 - dx2).abs().max()):.2e} of {float(dbase.abs().max()):.2e}")
print("\n".join(out))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(out) + "\n")
