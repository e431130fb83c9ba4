"""The part of the rollout glue (csrc/rollout.hip, mapdn_amd/rollout.py, mapdn_amd/replay.py) that needs no GPU: the refusals the three
entry points make before any HIP call, the replay ring's plain route, BatchedRollout on a scripted env against the float64 host reference
(tests/rollout_glue_cases.py — the same reference the GPU test holds the fused route to), and the list of kernels rollout.hip defines."""
import ctypes as C

import pytest
import torch

from tests import rollout_glue_cases as rc

OK, INVALID = rc.MAPDN_OK, rc.MAPDN_E_INVALID
SENT = 0xA5


def test_the_kernels_of_rollout_hip_are_the_tested_three():
    """a fourth __global__ function in rollout.hip needs its own tests in tests/test_rollout_glue_gpu.py (and its name here)"""
    names = rc.global_kernels()
    assert len(names) == len(set(names)), names
    assert set(names) == rc.KERNELS, names


def test_a_fourth_kernel_is_caught(monkeypatch):
    extra = rc._read() + "\n__global__ void __launch_bounds__(64)\nk_fourth(float* x) { x[0] = 0.0f; }\n" \
        "// __global__ void k_in_a_comment(int)\n/* __global__ void k_in_a_block_comment(int) */\n"
    monkeypatch.setattr(rc, "_read", lambda name="rollout.hip": extra)
    assert set(rc.global_kernels()) == rc.KERNELS | {"k_fourth"}


def _host(nbytes=4096):
    """a 64-byte aligned host address inside a sentinel-filled buffer: stands in for a device pointer, never dereferenced"""
    buf = (C.c_ubyte * (nbytes + 64))(*([SENT] * (nbytes + 64)))
    return buf, (C.addressof(buf) + 63) & ~63


def test_explore_actions_refuses_before_any_launch(lib):
    buf, p = _host()

    def call(mean=p, eps=p, avail=p, action=p, pol=p, actual=p, n=7):
        return lib.mapdn_explore_actions(mean, eps, avail, 1.0, 1, 0.8, 0.0, action, pol, actual, n, None)
    for k in ("mean", "eps", "action", "actual"):
        assert call(**{k: None}) == INVALID, k
    for n in (0, -1, -2 ** 40):
        assert call(n=n) == INVALID, n
    assert call(avail=None, pol=None, n=0) == INVALID
    assert bytes(buf) == bytes([SENT]) * len(buf)


def test_rollout_stats_refuses_before_any_launch(lib):
    buf, p = _host()
    names = ("info", "reward", "alive", "done", "alive_out", "sums")

    def call(n_envs=5, **kw):
        return lib.mapdn_rollout_stats(*[kw.get(k, p) for k in names], n_envs, None)
    for k in names:
        assert call(**{k: None}) == INVALID, k
    for n in (0, -1, -2 ** 31):
        assert call(n_envs=n) == INVALID, n
    assert bytes(buf) == bytes([SENT]) * len(buf)


def _segs(src, dst, nbytes):
    n = len(nbytes)
    return (C.c_void_p * len(src))(*src), (C.c_void_p * len(dst))(*dst), (C.c_int64 * n)(*nbytes)


def test_copy_segments_refuses_before_any_launch(lib):
    sbuf, s = _host()
    dbuf, d = _host()

    def call(src, dst, nbytes, n=None):
        a, b, c = _segs(src, dst, nbytes)
        return lib.mapdn_copy_segments(a, b, c, len(nbytes) if n is None else n, None)
    good = ([s, s + 256], [d, d + 256], [64, 32])
    a, b, c = _segs(*good)
    assert lib.mapdn_copy_segments(None, b, c, 2, None) == INVALID
    assert lib.mapdn_copy_segments(a, None, c, 2, None) == INVALID
    assert lib.mapdn_copy_segments(a, b, None, 2, None) == INVALID
    assert call(*good, n=0) == INVALID and call(*good, n=-1) == INVALID
    assert call([s + 16 * i for i in range(49)], [d + 16 * i for i in range(49)], [16] * 49) == INVALID
    assert call([s + 4, s + 256], good[1], good[2]) == INVALID                 # a misaligned source
    assert call(good[0], [d, d + 260], good[2]) == INVALID                      # a misaligned destination
    assert call(good[0], good[1], [64, 24]) == INVALID                          # not a multiple of 16
    assert call(good[0], good[1], [-16, 32]) == INVALID
    assert call([s, None], good[1], good[2]) == INVALID and call(good[0], [None, d], good[2]) == INVALID
    assert call([s, None], good[1], [64, 0]) == INVALID                         # also behind a length of 0
    # nothing to copy: MAPDN_OK without a launch (there is no device here to launch on)
    assert call(good[0], good[1], [0, 0]) == OK
    assert call([s + 16 * i for i in range(48)], [d + 16 * i for i in range(48)], [0] * 48) == OK
    assert bytes(dbuf) == bytes([SENT]) * len(dbuf) and bytes(sbuf) == bytes([SENT]) * len(sbuf)


@pytest.mark.parametrize("flag", ["1", "0"])
def test_the_replay_ring_on_the_cpu_takes_the_plain_route(flag, monkeypatch):
    """CPU tensors: _copy_in_one_launch declines whatever MAPDN_FUSED_ROLLOUT says, and add_experience fills the ring as a list with
    pop(0) would (utilities/replay_buffer.py:25-29), the mirror repeating the first `window` ring positions"""
    from mapdn_amd.replay import TransReplayBuffer
    monkeypatch.setenv("MAPDN_FUSED_ROLLOUT", flag)
    answers = []
    orig = TransReplayBuffer._copy_in_one_launch

    def spy(self, pieces):
        r = orig(self, pieces)
        answers.append(r)
        return r
    monkeypatch.setattr(TransReplayBuffer, "_copy_in_one_launch", spy)
    B, size, window = 64, 5 * 64 + 33, 100
    rb = TransReplayBuffer(size, device="cpu", window=window)
    g = torch.Generator(device="cpu").manual_seed(2)
    fifo = []
    for t in range(9):
        tr = dict(state=torch.randn(B, 6, 26, generator=g), done=(torch.rand(B, 1, generator=g) > 0.5).float(), valid=torch.rand(B, generator=g) > 0.5)
        rb.add_experience(tr)
        fifo += [{k: v[e] for k, v in tr.items()} for e in range(B)]
        fifo = fifo[-size:]
        assert len(rb) == len(fifo)
    assert answers == [False] * 9
    for i in (0, 1, len(fifo) // 2, len(fifo) - 1):
        got = rb.get_single(i)
        assert all(torch.equal(got[k], fifo[i][k]) for k in got), i
    for k, v in rb.store.items():
        assert v.shape[0] == size + window and torch.equal(v[size:], v[:window]), k
    whole = rb.get_batch(len(fifo), start=0)
    for k, v in whole.items():
        assert torch.equal(v, torch.stack([f[k] for f in fifo])), k


@pytest.mark.parametrize("max_steps", [48, 64])
def test_batched_rollout_on_the_scripted_env_cpu(max_steps):
    """the unfused bookkeeping on device="cpu" against the float64 host means over the live (step, env) pairs of the script; the `alive`
    handed to on_step is the script's mask before the step; the loop stops at the first t % 16 == 15 with no env alive (48 steps)"""
    script = rc.make_script()
    rc.check_scripted(script, max_steps, *rc.run_scripted(script, "cpu", max_steps))
