"""The three kernels of csrc/rollout.hip (k_explore, k_rollout_stats, k_copy_segments) through the C ABI at their edges, and the two Python
routes that launch them (TransReplayBuffer._copy_in_one_launch, BatchedRollout.run), against plain references.

Conventions of tests/test_learner_kernel_matrix_gpu.py: every output sits between sentinel guards (256 floats / 64 doubles / 64 bytes on
either side), inputs are seeded on the CPU, a second launch gives the same bits.

Bars.
k_explore: bit-identical to the PyTorch f32 chain on the device (NaN at the same places; a NaN mean gives a NaN `actual`); and `actual`
    against the float64 definition bias - scale + (clip(tanh(x64), -1, 1) + 1) scale: the stock chain's own error against it on the
    same finite inputs is measured, the kernel may have 2 x that, floored at 2^-22 (2 + |bias| + 2 scale) — six f32 roundings of values
    of at most that magnitude.  Printed as "[rollout glue] explore ...".
k_rollout_stats: against exactly rounded host sums (math.fsum).  The kernel's tree is ceil(B / 1024) serial adds per thread, 5 shuffle
    levels, 32 serial adds over the groups and the add into `sums`, so per column
        |error| <= (ceil(B / 1024) + 5 + 32 + 1) 2^-53 sum_live |x| + 2^-53 |result|;
    the live count is exact, alive_out is exact, with no live env `sums` keeps its bits.
k_copy_segments: bytes."""
import ctypes as C
import functools
import math

import pytest
import torch

from mapdn_amd import _lib
from mapdn_amd.rollout import translate_action
from tests import rollout_glue_cases as rc

pytestmark = pytest.mark.gpu
OK, INVALID = rc.MAPDN_OK, rc.MAPDN_E_INVALID
SENT = -7777.25                 # guard floats / doubles
SENT_B = 0xA5                   # guard bytes
GF, GD, GB = 256, 64, 64        # guard elements on either side: floats, doubles, bytes


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream(_dev()).cuda_stream


def _sync():
    torch.cuda.synchronize()


def _guarded(n, dtype, g, sent):
    buf = torch.full((2 * g + n,), sent, dtype=dtype, device=_dev())
    return buf, buf[g:g + n]


def _intact(buf, n, g, sent):
    return bool((buf[:g] == sent).all()) and bool((buf[g + n:] == sent).all())


def _bits(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def _same_with_nan(a, b):
    """torch.equal where a NaN equals a NaN"""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.where(a.isnan(), torch.zeros_like(a), a), torch.where(b.isnan(), torch.zeros_like(b), b))


# ================================================================================================================================
# k_explore
# ================================================================================================================================
PLANT = [0.0, 1e-40, 1e-8, 0.5, 1.0, 5.0, 9.0, 10.0, 20.0, 88.0, 1e30, float("inf")]
PLANT_AT = [3 + 10 * k for k in range(2 * len(PLANT) + 1)]         # 3 .. 243: below the smallest planted size, 255
STRIDE_N = 4096 * 256 + 257                                           # the launch is capped at 4096 x 256 threads: the stride loop turns


def _launch_explore(mean, eps, avail, stdv, bound, scale, bias, action, pol, actual, n):
    p = lambda t: t.data_ptr() if t is not None else None            # noqa: E731
    return _lib.load().mapdn_explore_actions(p(mean), p(eps), p(avail), stdv, int(bound), scale, bias, p(action), p(pol), p(actual), n, _stream())


@functools.lru_cache(maxsize=None)
def _explore_inputs(n):
    """(mean, eps, avail) on the CPU: means 1.5 randn, eps randn, avail zero at a tenth of the positions.  From 255 elements on, the
    values of PLANT with both signs and a NaN sit at PLANT_AT with eps = 0 there; avail is zero at +inf and at the NaN, one elsewhere"""
    g = torch.Generator(device="cpu").manual_seed(7 + n % 1009)
    mean, eps = 1.5 * torch.randn(n, generator=g), torch.randn(n, generator=g)
    avail = (torch.rand(n, generator=g) >= 0.1).float()
    if n >= 255:
        vals = [s * v for v in PLANT for s in (1.0, -1.0)] + [float("nan")]
        at = torch.tensor(PLANT_AT)
        mean[at] = torch.tensor(vals, dtype=torch.float64).float()
        eps[at] = 0.0
        avail[at] = 1.0
        avail[PLANT_AT[vals.index(float("inf"))]] = 0.0
        avail[PLANT_AT[-1]] = 0.0
        assert bool(mean[PLANT_AT[-1]].isnan()) and float(mean[PLANT_AT[2]]) == float(torch.tensor(1e-40).float()) != 0.0
    return mean, eps, avail


def _chain(mean, eps, avail, stdv, bound, scale, bias):
    """utilities/util.py:57-66, maddpg.py:92-93, utilities/util.py:123-132 as PyTorch runs them, one f32 operation after the other"""
    x = mean + stdv * eps
    a = torch.tanh(x) if bound else x
    pol = (1.0 - (avail == 0).to(a.dtype)) * a if avail is not None else a
    return a, pol, translate_action(a, scale, bias)


@pytest.mark.parametrize("with_avail", [True, False], ids=["avail+pol", "null"])
@pytest.mark.parametrize("scale,bias,bound,std", [(0.8, 0.0, 1, 1.0), (0.5, 0.25, 1, 0.7), (0.8, 0.1, 0, 1.0)])
@pytest.mark.parametrize("n", [1, 255, 256, 257, STRIDE_N])
def test_explore_against_the_chain_and_float64(n, scale, bias, bound, std, with_avail):
    dev = _dev()
    mean, eps, avail = (t.to(dev) for t in _explore_inputs(n))
    keep = [t.clone() for t in (mean, eps, avail)]
    av = avail if with_avail else None
    stdv = float(torch.tensor(std, dtype=torch.float32))

    def launch():
        bufs = [_guarded(n, torch.float32, GF, SENT) for _ in range(3)]
        pol = bufs[1][1] if with_avail else None
        assert _launch_explore(mean, eps, av, stdv, bound, scale, bias, bufs[0][1], pol, bufs[2][1], n) == OK
        _sync()
        for (buf, _), name in zip(bufs, ("action", "action_pol", "actual")):
            assert _intact(buf, n, GF, SENT), f"{name}: a store outside [0, n)"
        if not with_avail:
            assert bool((bufs[1][0] == SENT).all()), "action_pol is NULL: nothing to write"
        return bufs[0][1], pol, bufs[2][1]
    act, pol, actual = launch()
    again = launch()
    assert torch.equal(_bits(act), _bits(again[0])) and torch.equal(_bits(actual), _bits(again[2]))
    assert pol is None or torch.equal(_bits(pol), _bits(again[1]))
    for t, k in zip((mean, eps, avail), keep):
        assert torch.equal(_bits(t), _bits(k)), "an input changed"
    # the PyTorch f32 chain on the device
    want = _chain(mean, eps, av, stdv, bound, scale, bias)
    assert _same_with_nan(act, want[0]), "action"
    assert pol is None or _same_with_nan(pol, want[1]), "action_pol"
    assert _same_with_nan(actual, want[2]), "actual"
    if n >= 255:
        at = PLANT_AT[-1]
        assert bool(actual[at].isnan()) and bool(act[at].isnan()) and (pol is None or bool(pol[at].isnan())), "a NaN mean must stay NaN"
        assert int(actual.isnan().sum()) == 1
    else:
        assert not bool(actual.isnan().any())
    # the float64 definition, on the host
    m64, e64 = (t.double() for t in _explore_inputs(n)[:2])
    x64 = m64 + float(stdv) * e64
    fin = torch.isfinite(x64)
    y64 = torch.tanh(x64) if bound else x64
    d64 = (bias - scale) + (torch.clamp(y64, -1.0, 1.0) + 1.0) * scale
    e_stock = float((want[2].cpu().double() - d64)[fin].abs().max())
    e_kernel = float((actual.cpu().double() - d64)[fin].abs().max())
    bar = max(2.0 * e_stock, 2.0 ** -22 * (2.0 + abs(bias) + 2.0 * scale))
    print(f"[rollout glue] explore n={n} scale={scale} bias={bias} bound={bound} std={std} {'avail' if with_avail else 'null'}: "
          f"actual against float64: stock f32 chain {e_stock:.2e} kernel {e_kernel:.2e} bar {bar:.2e}")
    assert e_kernel <= bar, (e_kernel, bar, e_stock)


# ================================================================================================================================
# k_rollout_stats
# ================================================================================================================================
def _launch_stats(info, reward, alive_ptr, done, out_ptr, sums, B):
    return _lib.load().mapdn_rollout_stats(info.data_ptr(), reward.data_ptr(), alive_ptr, done.data_ptr(), out_ptr, sums.data_ptr(), B, _stream())


@functools.lru_cache(maxsize=None)
def _stats_inputs(B, data):
    """on the CPU: info [B, 11], reward [B] f64 and the two uniform draws the masks are cut from.  "cancel": +-1e8 (1 + rand), the sign
    alternating from env to env, plus randn — the sum is ~1e4 times smaller than the sum of magnitudes"""
    g = torch.Generator(device="cpu").manual_seed(100 * B + len(data))
    info, reward = torch.randn(B, 11, generator=g, dtype=torch.float64), torch.randn(B, generator=g, dtype=torch.float64)
    if data == "cancel":
        sign = (1.0 - 2.0 * (torch.arange(B) % 2)).double()
        info = sign.unsqueeze(-1) * 1e8 * (1.0 + torch.rand(B, 11, generator=g, dtype=torch.float64)) + info
        reward = sign * 1e8 * (1.0 + torch.rand(B, generator=g, dtype=torch.float64)) + reward
    return info, reward, torch.rand(B, generator=g), torch.rand(B, generator=g)


@pytest.mark.parametrize("data", ["randn", "cancel"])
@pytest.mark.parametrize("aliased", [False, True], ids=["separate", "aliased"])
@pytest.mark.parametrize("mask", ["alive", "dead", "random"])
@pytest.mark.parametrize("B", [1, 31, 32, 33, 1023, 1024, 1025, 2049, 5000])
def test_rollout_stats_against_exact_sums(B, mask, aliased, data):
    dev = _dev()
    info_h, reward_h, r1, r2 = _stats_inputs(B, data)
    alive_h = {"alive": torch.ones(B, dtype=torch.bool), "dead": torch.zeros(B, dtype=torch.bool), "random": r1 > 0.3}[mask]
    done_h = r2 > 0.8
    info, reward, done = info_h.to(dev), reward_h.to(dev), done_h.to(torch.uint8).to(dev)
    start_h = torch.arange(13, dtype=torch.float64) * 0.5

    def launch():
        sb, sums = _guarded(13, torch.float64, GD, SENT)
        sums.copy_(start_h)
        ab, alive = _guarded(B, torch.uint8, GB, SENT_B)
        alive.copy_(alive_h.to(torch.uint8))
        ob, out = (ab, alive) if aliased else _guarded(B, torch.uint8, GB, SENT_B)
        assert _launch_stats(info, reward, alive.data_ptr(), done, out.data_ptr(), sums, B) == OK
        _sync()
        assert _intact(sb, 13, GD, SENT), "sums: a store outside its 13 doubles"
        assert _intact(ob, B, GB, SENT_B) and _intact(ab, B, GB, SENT_B), "alive_out: a store outside [0, B)"
        if not aliased:
            assert torch.equal(alive.cpu(), alive_h.to(torch.uint8)), "alive changed although alive_out is another buffer"
        return sums.cpu(), out.cpu()
    sums, out = launch()
    sums2, out2 = launch()
    assert torch.equal(_bits(sums), _bits(sums2)) and torch.equal(out, out2), "a second launch from the same start gives other bits"
    assert torch.equal(_bits(info), _bits(info_h.to(dev))) and torch.equal(_bits(reward), _bits(reward_h.to(dev))) and torch.equal(done.cpu(), done_h.to(torch.uint8))
    assert torch.equal(out, (alive_h & ~done_h).to(torch.uint8))
    live = int(alive_h.sum())
    assert float(sums[12]) == float(start_h[12]) + live
    if live == 0:
        assert torch.equal(_bits(sums), _bits(start_h)), "no live env: sums keeps its bits"
    depth = -(-B // 1024) + 5 + 32 + 1
    cols = [info_h[:, k] for k in range(11)] + [reward_h]
    for k, col in enumerate(cols):
        vals = col[alive_h].tolist()
        got, start = float(sums[k]), float(start_h[k])
        err = abs(math.fsum(vals + [start, -got]))                   # |exact result - got|, rounded once
        bar = depth * 2.0 ** -53 * math.fsum(abs(v) for v in vals) + 2.0 ** -53 * abs(math.fsum(vals + [start]))
        assert err <= bar, (k, err, bar, got)


# ================================================================================================================================
# k_copy_segments, through the C ABI
# ================================================================================================================================
def _launch_copy(src, dst, nbytes, n=None, stream=None):
    """src / dst: lists of addresses (None: a NULL entry); the arrays are as long as the lists, n may claim otherwise"""
    a, b, c = (C.c_void_p * len(src))(*src), (C.c_void_p * len(dst))(*dst), (C.c_int64 * len(nbytes))(*nbytes)
    return _lib.load().mapdn_copy_segments(a, b, c, len(nbytes) if n is None else n, _stream() if stream is None else stream)


class _Segments:
    """sources: random bytes, back to back in one buffer (+ 64 spare bytes).  Destinations: one sentinel-filled buffer, every segment
    with 64 guard bytes before and after it (gap = 0: back to back, as a ring and its mirror are, guards at the two ends only)"""

    def __init__(self, lengths, seed, gap=GB):
        dev = _dev()
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.lengths = list(lengths)
        total = sum(self.lengths)
        self.src_h = torch.randint(0, 256, (total + 64,), dtype=torch.uint8, generator=g)
        self.src = self.src_h.to(dev)
        self.s_off, self.d_off = [], []
        s, d = 0, GB
        for ln in self.lengths:
            self.s_off.append(s)
            self.d_off.append(d)
            s, d = s + ln, d + ln + gap
        d = d - gap + GB
        self.want_h = torch.full((d,), SENT_B, dtype=torch.uint8)
        self.dst = torch.full((d,), SENT_B, dtype=torch.uint8, device=dev)
        for ln, so, do in zip(self.lengths, self.s_off, self.d_off):
            self.want_h[do:do + ln] = self.src_h[so:so + ln]
        assert self.src.data_ptr() % 16 == 0 and self.dst.data_ptr() % 16 == 0
        self.sp = [self.src.data_ptr() + o for o in self.s_off]
        self.dp = [self.dst.data_ptr() + o for o in self.d_off]

    def check_copied(self):
        _sync()
        assert torch.equal(self.dst.cpu(), self.want_h), "a destination differs from its source, or a guard byte was written"
        assert torch.equal(self.src.cpu(), self.src_h), "a source changed"

    def check_untouched(self):
        _sync()
        assert bool((self.dst == SENT_B).all()), "a refused (or empty) call wrote to a destination"
        assert torch.equal(self.src.cpu(), self.src_h)


CYCLE = [0, 16, 32, 4080, 4096, 4112, (1 << 20) + 16]
STRIDE_BYTES = (2048 * 256 + 257) * 16                                # the launch is capped at 2048 x 256 threads per segment


def test_copy_48_segments_with_the_stride_loop_turning():
    lengths = [CYCLE[i % len(CYCLE)] for i in range(48)]
    lengths[29] = STRIDE_BYTES                                        # between a 0-byte and a 32-byte neighbour
    assert lengths[28] == 0 and lengths[30] == 32 and all(v in lengths for v in CYCLE)
    s = _Segments(lengths, seed=48)
    assert _launch_copy(s.sp, s.dp, s.lengths) == OK
    s.check_copied()


@pytest.mark.parametrize("nbytes", [16, 4112, 256 * 16, 257 * 16, STRIDE_BYTES])
def test_copy_one_segment_alone(nbytes):
    s = _Segments([nbytes], seed=nbytes % 1000)
    assert _launch_copy(s.sp, s.dp, s.lengths) == OK
    s.check_copied()


def test_copy_into_adjacent_destinations():
    s = _Segments([4112, 16, 0, 2 * 256 * 16 + 32, 4096], seed=5, gap=0)
    assert s.dp[1] == s.dp[0] + 4112 and s.dp[2] == s.dp[3]
    assert _launch_copy(s.sp, s.dp, s.lengths) == OK
    s.check_copied()


def test_copy_on_a_side_stream():
    s = _Segments([4096, 0, (1 << 20) + 16, 32], seed=6)
    side = torch.cuda.Stream(device=_dev())
    side.wait_stream(torch.cuda.current_stream(_dev()))               # the buffers were filled on the current stream
    assert _launch_copy(s.sp, s.dp, s.lengths, stream=side.cuda_stream) == OK
    torch.cuda.current_stream(_dev()).wait_stream(side)
    assert torch.equal(s.dst, s.want_h.to(_dev()))                    # read on the current stream, behind the wait
    s.check_copied()


def test_copy_refusals_write_nothing():
    s = _Segments([16] * 49 + [64], seed=7)                           # room for every call below, were it not refused
    sp, dp, ln = s.sp[:4], s.dp[:4], [16, 16, 16, 16]
    calls = dict(
        segments_49=(s.sp[:49], s.dp[:49], s.lengths[:49], None),
        segments_0=(sp, dp, ln, 0),
        src_plus_4=([sp[0], sp[1] + 4, sp[2], sp[3]], dp, ln, None),
        dst_plus_4=(sp, [dp[0], dp[1], dp[2] + 4, dp[3]], ln, None),
        nbytes_24=(sp, dp, [16, 16, 16, 24], None),
        nbytes_minus_16=(sp, dp, [-16, 16, 16, 16], None),
        null_src=([sp[0], None, sp[2], sp[3]], dp, ln, None),
        null_dst=(sp, [dp[0], dp[1], dp[2], None], ln, None),
    )
    for name, (a, b, c, n) in calls.items():
        assert _launch_copy(a, b, c, n) == INVALID, name
        s.check_untouched()
    assert _launch_copy(s.sp[:48], s.dp[:48], [0] * 48) == OK        # nothing to copy
    assert _launch_copy(sp[:1], dp[:1], [0]) == OK
    s.check_untouched()
    assert _launch_copy(s.sp[:48], s.dp[:48], s.lengths[:48]) == OK  # and the largest count that is taken
    _sync()
    want = torch.full_like(s.want_h, SENT_B)
    for i in range(48):
        want[s.d_off[i]:s.d_off[i] + 16] = s.src_h[s.s_off[i]:s.s_off[i] + 16]
    assert torch.equal(s.dst.cpu(), want)


# ================================================================================================================================
# the replay ring's route to k_copy_segments
# ================================================================================================================================
def _replay_routes(monkeypatch, batches, size, window, expect):
    """the same insertions with MAPDN_FUSED_ROLLOUT 0 / 1 (and the copy on a side stream or not): the whole stores and len() are equal,
    and _copy_in_one_launch answered `expect` (one bool per insertion) on the fused route"""
    from mapdn_amd.replay import TransReplayBuffer
    dev = _dev()
    answers = []
    orig = TransReplayBuffer._copy_in_one_launch

    def spy(self, pieces):
        r = orig(self, pieces)
        answers.append(r)
        return r
    monkeypatch.setattr(TransReplayBuffer, "_copy_in_one_launch", spy)

    def run(fused, asyn):
        monkeypatch.setenv("MAPDN_FUSED_ROLLOUT", fused)
        monkeypatch.setenv("MAPDN_REPLAY_ASYNC", asyn)
        del answers[:]
        rb = TransReplayBuffer(size, device=dev, window=window)
        for tr in batches:
            rb.add_experience({k: v.to(dev) for k, v in tr.items()})
        store = {k: v.clone() for k, v in rb.store.items()}
        _sync()
        return store, len(rb), list(answers)
    base, n_base, ans = run("0", "1")
    assert ans == [False] * len(batches)
    for k, v in base.items():
        assert v.shape[0] == size + window and torch.equal(v[size:], v[:window]), k     # every slot was written; the mirror repeats the ring
    for asyn in ("1", "0"):
        got, n_got, ans = run("1", asyn)
        assert ans == expect, (asyn, ans)
        assert n_got == n_base
        for k in base:
            assert torch.equal(_bits(got[k]), _bits(base[k])), (asyn, k)


def test_replay_pieces_beyond_the_launch_cap(monkeypatch):
    """(a) a `state` of more than 8 MiB per piece: the stride loop of k_copy_segments turns; the ring is 2.5 batches long with a mirror
    of one batch, so of the five insertions one wraps (ring, wrap-around, mirror pieces)"""
    B = 1024
    g = torch.Generator(device="cpu").manual_seed(21)
    batches = [dict(state=torch.randn(B, 38, 58, generator=g), done=(torch.rand(B, 1, generator=g) > 0.5).float()) for _ in range(5)]
    assert batches[0]["state"].numel() * 4 > 2048 * 256 * 16
    _replay_routes(monkeypatch, batches, size=5 * B // 2, window=B, expect=[True] * 5)


def test_replay_a_field_that_is_not_16_byte_granular(monkeypatch):
    """(b) 100 transitions with a bool field: 100 bytes — every insertion takes the copy_ loop, the contents are the same"""
    B = 100
    g = torch.Generator(device="cpu").manual_seed(22)
    batches = [dict(state=torch.randn(B, 6, 26, generator=g), valid=torch.rand(B, generator=g) > 0.5) for _ in range(5)]
    _replay_routes(monkeypatch, batches, size=250, window=B, expect=[False] * 5)


def test_replay_a_wrap_at_an_odd_row_count(monkeypatch):
    """(c) a ring of 5 x 64 + 33 rows with a [B, 1] f32 field: the sixth insertion wraps after 33 rows = 132 bytes — refused there only"""
    B = 64
    g = torch.Generator(device="cpu").manual_seed(23)
    batches = [dict(state=torch.randn(B, 6, 26, generator=g), done=(torch.rand(B, 1, generator=g) > 0.5).float()) for _ in range(6)]
    _replay_routes(monkeypatch, batches, size=5 * B + 33, window=0, expect=[True] * 5 + [False])


def test_replay_more_than_48_pieces(monkeypatch):
    """(d) 13 fields, the mirror as long as the ring: the wrapping insertion has 4 pieces per field (ring, wrap-around and the mirror of
    each) = 52 — refused; the others have 26"""
    B = 64
    g = torch.Generator(device="cpu").manual_seed(24)
    batches = [{f"f{i:02d}": torch.randn(B, 1 + i, generator=g) for i in range(13)} for _ in range(8)]
    _replay_routes(monkeypatch, batches, size=5 * B + 32, window=5 * B + 32, expect=[True] * 5 + [False] + [True] * 2)


# ================================================================================================================================
# BatchedRollout on a scripted env
# ================================================================================================================================
@pytest.mark.parametrize("max_steps", [48, 64])
def test_batched_rollout_on_the_scripted_env(max_steps, monkeypatch):
    """envs end at steps spread over 3 .. 37: the fused bookkeeping (k_rollout_stats, alive / alive_next swapped every step) and the
    PyTorch one against the float64 host means of the script; on_step sees the script's mask before the step on both routes; both stop
    at t = 47, the first t % 16 == 15 with no env alive — the last step of a 48-step episode, an early exit from a 64-step one"""
    script = rc.make_script()
    lib = _lib.load()
    calls = []
    orig = lib.mapdn_rollout_stats

    def counted(*a):
        calls.append(a[6])
        return orig(*a)
    monkeypatch.setattr(lib, "mapdn_rollout_stats", counted)
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("MAPDN_FUSED_ROLLOUT", flag)
        del calls[:]
        out[flag] = rc.run_scripted(script, _dev(), max_steps)
        assert calls == ([rc.N_ENVS] * rc.script_steps(max_steps) if flag == "1" else []), (flag, calls)
        rc.check_scripted(script, max_steps, *out[flag])
    assert out["1"][2] == out["0"][2] and out["1"][3] == out["0"][3]
    assert all(torch.equal(a, b) for a, b in zip(out["1"][1], out["0"][1]))
