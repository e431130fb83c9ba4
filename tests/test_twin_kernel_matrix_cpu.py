"""CPU tests of the twin-critic kernel matrix (tests/twin_kernel_matrix.py): the rows cover the compiled set parsed from
csrc/critic_twin.hip — an instantiation added without a row fails here —, the host-only geometry query (mapdn_critic_twin_geometry, the
function the launcher calls) reports each row's kernel, its limits are where the LDS arithmetic puts them, and the learner's predicate
agrees with them."""
import types

import pytest
import torch

from mapdn_amd import _lib
from mapdn_amd.learner import MLPCritic, critic_twin_ok, make_alg_args
from tests import learner_kernel_matrix as lm
from tests import twin_kernel_matrix as tm


def test_the_rows_cover_the_compiled_set_exactly():
    ck = tm.compiled_kernels()
    assert len(set(ck)) == len(ck), ck
    assert set(ck) == {("twin_fwd",), ("twin_mse",)}
    have = {r.kernel for r in tm.ROWS}
    assert have == set(ck), (sorted(set(ck) - have), sorted(have - set(ck)))
    labels = [r.label for r in tm.ROWS]
    assert len(set(labels)) == len(labels) and [r.label for r in tm.rows_for(304)] == labels
    assert {r.shape["n"] for r in tm.ROWS if r.kernel[0] == "twin_mse"} == {1, 6, 38, 88}
    assert {r.opts["outputs"] for r in tm.ROWS if r.kernel[0] == "twin_fwd"} >= {("v1",), ("v2",), ("vmin",), ("v1", "v2", "vmin")}
    print(f"[twin kernel matrix] compiled: {len(ck)} kernels; {len(tm.ROWS)} rows")


def test_an_instantiation_without_a_row_is_caught():
    """copies of the source with one more kernel: a third k_twin_* name, a templated one, a kernel launched from two sites"""
    real = tm._src
    site = "  hipLaunchKernelGGL(k_twin_mse, dim3(blocks)"
    assert site in real()
    for new, caught in ((site.replace("k_twin_mse", "k_twin_mse2"), True), (site.replace("(k_twin_mse,", "((k_twin_mse<512>),"), True), (site, False)):
        tm._src = lambda name="critic_twin.hip", _n=new: real(name).replace(site, _n + "; " + site.strip(), 1)
        try:
            if caught:
                with pytest.raises(AssertionError):
                    tm.compiled_kernels()
            else:
                assert tm.compiled_kernels().count(("twin_mse",)) == 2             # listed twice: the exact-cover test's duplicate check fails
        finally:
            tm._src = real


def test_the_single_head_matrix_is_unchanged_by_the_include():
    """critic.hip compiles critic_twin.hip inside it; the single-head launch sites parsed from critic.hip's own text are the same set"""
    assert {k for k in lm.head_kernels() if k[0] == "head_bwd"} == {("head_bwd", bc, m, nt) for bc in (0, 1) for m in (0, 1, 2, 3) for nt in (256, 512)}
    assert "k_twin" not in lm._src("critic.hip").replace('#include "critic_twin.hip"', "")


@pytest.mark.parametrize("row", tm.ROWS, ids=[r.label for r in tm.ROWS])
def test_every_row_reports_its_kernel(row):
    assert tm.reported_kernel(row, cus=tm.CUS) == row.kernel, row
    assert hasattr(_lib.load(), row.entry)


def test_twin_geometry_and_scratch():
    lib = _lib.load()
    fits = [n for n in range(1, 257) if _lib.critic_twin_geometry(n * 64, n, tm.CUS) is not None]
    assert fits == list(range(1, fits[-1] + 1)) and fits[-1] >= tm.MAX_N
    assert all(_lib.critic_twin_geometry(n * 64, n, tm.CUS)[2] <= tm.LDS_MAX for n in fits)
    # the LDS of the launch covers the end-of-kernel reduction: 4 wavefronts x TP floats
    assert _lib.critic_twin_geometry(64, 1, tm.CUS)[2] >= 4 * tm.TP * 4
    # bad arguments: rows not a multiple of n, no rows, no agents
    assert _lib.critic_twin_geometry(20, 7, tm.CUS) is None and _lib.critic_twin_geometry(0, 1, tm.CUS) is None
    assert _lib.critic_twin_geometry(64, 0, tm.CUS) is None and lib.mapdn_critic_twin_scratch_floats(20, 7) == 0
    # blocks: one workgroup per CU at most, never more wavefronts than groups; scratch = blocks x (TP + n 64)
    assert _lib.critic_twin_geometry(3 * 6, 6, tm.CUS)[1] == 1
    assert _lib.critic_twin_geometry(tm.big_groups(tm.CUS, 256) * 6, 6, tm.CUS)[1] == tm.CUS
    assert _lib.critic_twin_geometry(tm.big_groups(77, 256) * 6, 6, 77)[1] == 77
    for row in tm.ROWS:
        if row.kernel[0] == "twin_mse":
            nb, n = row.shape["nb"], row.shape["n"]
            assert lib.mapdn_critic_twin_scratch_floats(nb * n, n) >= _lib.critic_twin_geometry(nb * n, n, tm.CUS)[1] * (tm.TP + n * 64)


def test_the_learner_predicate(monkeypatch):
    cr = MLPCritic(7, 1, make_alg_args(3, 5, 1))
    x = types.SimpleNamespace(is_cuda=True, dtype=torch.float32, dim=lambda: 2, shape=(64, 64))
    assert critic_twin_ok(cr, x, 64 * 88, 88) and not critic_twin_ok(cr, x, 64 * 89, 89) and not critic_twin_ok(cr, x, 512, 8)
    assert not critic_twin_ok(cr, types.SimpleNamespace(is_cuda=False, dtype=torch.float32, dim=lambda: 2, shape=(64, 64)), 64 * 88, 88)
    assert not critic_twin_ok(MLPCritic(7, 1, make_alg_args(3, 5, 1, hid_activation="tanh")), x, 64 * 88, 88)
    monkeypatch.setenv("MAPDN_FUSED_TWIN", "0")
    assert not critic_twin_ok(cr, x, 64 * 88, 88)
