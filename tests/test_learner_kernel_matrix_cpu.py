"""CPU tests of the learner kernel matrix (tests/learner_kernel_matrix.py): the rows cover the compiled set parsed from the sources — an
instantiation added without a row fails here —, every row's kernel is the one the library's host-only geometry queries report
(mapdn_policy_forward_geometry, mapdn_critic_head_backward_geometry: the functions the launchers call), and the boundaries of both
choosers are where the launchers' LDS arithmetic puts them."""
import os
import types

import pytest
import torch

from mapdn_amd import _lib
from mapdn_amd.learner import HEAD_MAX_FORMED_N, DDPGNet, MLPCritic, critic_head_ok, make_alg_args
from tests import learner_kernel_matrix as lm


def uncovered(compiled, rows):
    """compiled kernels without a row, and row kernels that are not compiled"""
    have = {lm.compiled_of(r.kernel) for r in rows}
    return sorted(set(compiled) - have), sorted(have - set(compiled))


def test_the_compiled_set_parses():
    ck = lm.compiled_kernels()
    assert len(set(ck)) == len(ck), sorted(k for k in set(ck) if ck.count(k) > 1)         # a kernel listed twice in the sources shows
    assert {k for k in ck if k[0].startswith("policy_fwd")} == {(f, p) for f in ("policy_fwd", "policy_fwd2") for p in (512, 256)}
    assert {k for k in ck if k[0] == "head_bwd"} == {("head_bwd", bc, m, nt) for bc in (0, 1) for m in (0, 1, 2, 3) for nt in (256, 512)}
    assert {k for k in ck if k[0].startswith("ln64")} == {("ln64_" + d, r, bc) for d in ("fwd", "bwd") for r in (0, 1) for bc in (0, 1)}
    assert {("head_fwd", 0), ("head_fwd", 1), ("policy_bwd",), ("relu_dot64_fwd",), ("relu_dot64_bwd",)} <= set(ck)
    print(f"[learner kernel matrix] compiled: {len(ck)} kernels; {len(lm.ROWS)} rows")


def test_the_rows_cover_the_compiled_set_exactly():
    missing, extra = uncovered(lm.compiled_kernels(), lm.ROWS)
    assert not missing, f"compiled learner kernels without a row in tests/learner_kernel_matrix.py: {missing}"
    assert not extra, f"rows for kernels that are not compiled: {extra}"
    labels = [r.label for r in lm.ROWS]
    assert len(set(labels)) == len(labels)
    # the policy forward's run-time cells: every form x threads x ids_lds x parity
    cells = {r.kernel for r in lm.ROWS if r.kernel[0].startswith("policy_fwd")}
    assert cells == {(f, p, il, odd) for f in ("policy_fwd", "policy_fwd2") for p in (512, 256) for il in (0, 1) for odd in (0, 1)}
    assert [r.label for r in lm.rows_for(304)] == labels                                # the same rows on a device with another CU count


def test_an_instantiation_without_a_row_is_caught():
    """the coverage check above on copies of the sources with one more instantiation: a third thread count of k_head_bwd, a third
    workgroup size of k_policy_fwd2, a kernel listed twice"""
    real = lm._src
    cases = (
        ("critic.hip", "    return head_bwd_launch_nt<BC, MODE, 512>(", "    if (false) return head_bwd_launch_nt<BC, MODE, 128>(a, dv, dx, dot_w, dact, "
         "scratch, grads, rows, st, wrow, scale);\n    return head_bwd_launch_nt<BC, MODE, 512>(", [("head_bwd", bc, m, 128) for bc in (0, 1) for m in (0, 1, 2, 3)]),
        ("policy.hip", "MAPDN_POLICY_LAUNCH(k_policy_fwd2, 512);", "MAPDN_POLICY_LAUNCH(k_policy_fwd2, 512); MAPDN_POLICY_LAUNCH(k_policy_fwd2, 128);",
         [("policy_fwd2", 128)]),
    )
    for fname, old, new, want in cases:
        def patched(name, _f=fname, _o=old, _n=new):
            s = real(name)
            if name == _f:
                assert _o in s, _o
                s = s.replace(_o, _n, 1)
            return s
        lm._src = patched
        try:
            compiled = lm.compiled_kernels()
        finally:
            lm._src = real
        assert uncovered(compiled, lm.ROWS) == (sorted(want), []), fname
    lm._src = lambda name: real(name).replace("MAPDN_POLICY_LAUNCH(k_policy_fwd, 256);", "MAPDN_POLICY_LAUNCH(k_policy_fwd, 256); MAPDN_POLICY_LAUNCH(k_policy_fwd, 256);", 1)
    try:
        twice = lm.compiled_kernels()
    finally:
        lm._src = real
    assert twice.count(("policy_fwd", 256)) == 2


@pytest.mark.parametrize("row", lm.ROWS, ids=[r.label for r in lm.ROWS])
def test_every_row_reports_its_kernel(row):
    """with cus = 256, under the row's switches, in a private copy of the environment's two switches (restored afterwards)"""
    assert lm.reported_kernel(row, cus=lm.CUS) == row.kernel, row
    assert hasattr(_lib.load(), row.entry)


def test_the_policy_forward_fits_up_to_width_176():
    lib = _lib.load()
    for (pt, il, odd), widths in lm.POLICY_WIDTHS.items():
        for o, ids in widths:
            g = _lib.policy_forward_geometry(o, ids)
            assert g is not None and g[:2] == (pt, il) and o % 2 == odd, (o, ids, g)
            assert 0 < g[2] <= lm.LDS_MAX and lib.mapdn_policy_forward_fits(o, ids) == 1
    assert _lib.policy_forward_geometry(176, 38) == (256, 0, 163328) and _lib.policy_forward_geometry(176, 0)[:2] == (256, 1)
    for o, ids in lm.POLICY_REFUSED:
        assert _lib.policy_forward_geometry(o, ids) is None and lib.mapdn_policy_forward_fits(o, ids) == 0, (o, ids)
    for o in range(1, 260):                                  # the reported LDS never exceeds a CU's 160 KB, the two exports agree
        for ids in (0, 6, 22, 38):
            g = _lib.policy_forward_geometry(o, ids)
            assert (g is not None) == bool(lib.mapdn_policy_forward_fits(o, ids)) == (o <= 176), (o, ids)
            assert g is None or (g[0] in (256, 512) and g[2] <= lm.LDS_MAX and (g[1] == 1 or ids > 0))
    assert lib.mapdn_policy_forward_geometry(0, 0, None, None, None) == 0 and lib.mapdn_policy_forward_geometry(58, 22, None, None, None) == 1


def test_the_learner_keeps_the_pytorch_route_beyond_the_last_width_that_fits():
    """DDPGNet._fused_policy_ok asks mapdn_policy_forward_fits: true at 176 + 38, false at 177 + 38 and 192 + 0.  The decision reads
    only the device and dtype of its arguments, which stand-ins provide here"""
    f32 = types.SimpleNamespace(is_cuda=True, dtype=torch.float32)
    for n, o, ids, want in ((38, 176, True, True), (38, 177, True, False), (5, 192, False, False), (5, 176, False, True)):
        net = DDPGNet(make_alg_args(n, o, 1, agent_id=ids), "maddpg")
        with torch.no_grad():
            assert net._fused_policy_ok(f32, f32) is want, (n, o, ids)
        with torch.enable_grad():
            assert net._fused_policy_ok(f32, f32) is False                                # (inference only)
    # and a net that does not fit computes its policy with the modules (here on the CPU)
    net = DDPGNet(make_alg_args(3, 192, 1, agent_id=False), "maddpg")
    with torch.no_grad():
        means, _, hid = net.policy(torch.randn(2, 3, 192), torch.zeros(2, 3, 64))
    assert means.shape == (2, 3, 1) and hid.shape == (2, 3, 64)


def _g(rows, n, formed, mode, monkeypatch, force=None, cus=lm.CUS):
    if force is None:
        monkeypatch.delenv("MAPDN_HEAD_BWD_THREADS", raising=False)
    else:
        monkeypatch.setenv("MAPDN_HEAD_BWD_THREADS", str(force))
    return _lib.critic_head_backward_geometry(rows, n, formed, mode, cus)


def test_head_backward_geometry(monkeypatch):
    # forcing 512 where its LDS does not fit falls to 256: formed rows with n = 50 keep 8 x [50][64] accumulators (MODE 2 keeps none)
    assert _g(50 * 4000, 50, True, 0, monkeypatch, 512)[0] == 256 and _g(50 * 4000, 50, True, 1, monkeypatch, 512)[0] == 256
    assert _g(50 * 4000, 50, True, 2, monkeypatch, 512)[0] == 512 and _g(38 * 4000, 38, True, 0, monkeypatch, 512)[0] == 512
    assert _g(50 * 4000, 50, True, 0, monkeypatch)[0] == 256 and _g(38 * 4000, 38, True, 0, monkeypatch)[0] == 512
    assert _g(38 * 4000, 38, True, 0, monkeypatch, 256)[0] == 256
    # n = 88 fits at 256 threads within 160 KB; the learner refuses the head from 89 agents on, the library from the first n whose LDS
    # does not fit
    t, b, lds = _g(88 * 64, 88, True, 0, monkeypatch)
    assert t == 256 and lds <= lm.LDS_MAX
    cr = MLPCritic(7, 1, make_alg_args(3, 5, 1))
    x = types.SimpleNamespace(is_cuda=True, dtype=torch.float32, dim=lambda: 2, shape=(64, 64))
    assert HEAD_MAX_FORMED_N == 88 and critic_head_ok(cr, x, 64 * 88, 88) and not critic_head_ok(cr, x, 64 * 89, 89)
    fits = [n for n in range(1, 257) if _g(n * 64, n, True, 0, monkeypatch) is not None]
    assert fits == list(range(1, fits[-1] + 1)) and fits[-1] >= HEAD_MAX_FORMED_N
    assert all(_g(n * 64, n, True, 0, monkeypatch)[2] <= lm.LDS_MAX for n in fits)
    # bad arguments
    assert _g(0, 1, False, 0, monkeypatch) is None and _g(20, 7, True, 0, monkeypatch) is None and _g(64, 1, False, 4, monkeypatch) is None
    # blocks: one workgroup per CU at most, never more wavefronts than units of work
    assert _g(40, 1, False, 0, monkeypatch, 256)[1] == 1 and _g(40, 1, False, 0, monkeypatch, 512)[1] == 1
    assert _g(lm.big_rows(lm.CUS), 1, False, 0, monkeypatch, 512)[1] == lm.CUS and _g(lm.big_rows(77), 1, False, 0, monkeypatch, 512, cus=77)[1] == 77


@pytest.mark.parametrize("row", [r for r in lm.ROWS if r.kernel[0] == "head_bwd"], ids=lambda r: r.label)
def test_head_scratch_covers_both_thread_counts(row, monkeypatch):
    """mapdn_critic_head_scratch_floats (which asks the current device, or assumes 256 CUs without one) >= blocks x (HP + n 64) of the
    launch at either thread count"""
    lib = _lib.load()
    formed, n, rows = "nb" in row.shape, row.shape.get("n", 1), lm.total_rows(row.shape)
    have = lib.mapdn_critic_head_scratch_floats(rows, n, int(formed))
    for force in (256, 512):
        g = _g(rows, n, formed, row.kernel[2], monkeypatch, force)
        assert g is not None and have >= g[1] * (lm.HP + (n * 64 if formed else 0)), (row, force, g, have)
