"""CPU tests of the counterfactual-baseline kernel matrix (tests/cf_kernel_matrix.py): the rows cover the compiled set parsed from
csrc/critic_cf.hip — an instantiation added without a row fails here —, the one launch site is the one the rows were built for, the
entry refuses bad S, n and rows on the host before anything is launched, and the learner's predicate agrees with the kernel's limits."""
import re
import types

import pytest
import torch

from mapdn_amd import _lib
from mapdn_amd.learner import MLPCritic, critic_cf_ok, make_alg_args
from tests import cf_kernel_matrix as cm
from tests import learner_kernel_matrix as lm


def test_the_rows_cover_the_compiled_set_exactly():
    ck = cm.compiled_kernels()
    assert len(set(ck)) == len(ck), ck
    assert set(ck) == {("cf_baseline",)}
    have = {r.kernel for r in cm.ROWS}
    assert have == set(ck), (sorted(set(ck) - have), sorted(have - set(ck)))
    labels = [r.label for r in cm.ROWS]
    assert len(set(labels)) == len(labels) and [r.label for r in cm.rows_for(304)] == labels
    assert {(r.shape["n"], r.shape["S"]) for r in cm.ROWS} >= {(1, 1), (6, 10), (38, 10), (38, 2), (6, cm.S_MAX)}
    assert any(r.shape["rows"] % 16 for r in cm.ROWS) and any(r.shape["rows"] < 4 * 16 for r in cm.ROWS)
    big = [r for r in cm.ROWS if r.label == "big"][0]
    assert (big.shape["rows"] + 15) // 16 > cm.CUS * 2 * 4 + 11
    print(f"[cf kernel matrix] compiled: {len(ck)} kernels; {len(cm.ROWS)} rows")


def test_an_instantiation_without_a_row_is_caught():
    """copies of the source with one more kernel: a second k_cf_* name, a templated one, a kernel launched from two sites"""
    real = cm._src
    site = "  hipLaunchKernelGGL(k_cf_baseline, dim3(blocks)"
    assert site in real()
    for new, caught in ((site.replace("k_cf_baseline", "k_cf_baseline2"), True), (site.replace("(k_cf_baseline,", "((k_cf_baseline<true>),"), True),
                        (site, False)):
        cm._src = lambda name="critic_cf.hip", _n=new: real(name).replace(site, _n + "; " + site.strip(), 1)
        try:
            if caught:
                with pytest.raises(AssertionError):
                    cm.compiled_kernels()
            else:
                assert cm.compiled_kernels().count(("cf_baseline",)) == 2          # listed twice: the exact-cover test's duplicate check fails
        finally:
            cm._src = real


def test_the_one_launch_site():
    """no chooser: 256 threads (four wavefronts, one 16-row tile each per turn), no dynamic LDS, workgroups = min(ceil(tiles / 4), 2 per CU)
    — the grid the rows' "idle" and "big" shapes were built for"""
    src = cm._src()
    launch = re.findall(r"hipLaunchKernelGGL\(k_cf_baseline,\s*dim3\((\w+)\),\s*dim3\((\d+)\),\s*(\d+),", src)
    assert launch == [("blocks", "256", "0")]
    assert "__launch_bounds__(256)" in src
    assert re.search(r"blocks = \(int\)std::max<int64_t>\(1, std::min<int64_t>\(\(tiles \+ 3\) / 4, \(int64_t\)head_cus\(\) \* 2\)\)", src)
    assert re.search(r"T = \(long\)blockIdx\.x \* 4 \+ wave; T < n_tiles; T \+= \(long\)gridDim\.x \* 4", src)


def test_the_other_learner_matrices_are_unchanged_by_the_include():
    """critic.hip compiles critic_cf.hip inside it; the single-head launch sites parsed from critic.hip's own text are the same set"""
    assert {k for k in lm.head_kernels() if k[0] == "head_bwd"} == {("head_bwd", bc, m, nt) for bc in (0, 1) for m in (0, 1, 2, 3) for nt in (256, 512)}
    assert "k_cf" not in lm._src("critic.hip").replace('#include "critic_cf.hip"', "")


@pytest.mark.parametrize("row", cm.ROWS, ids=[r.label for r in cm.ROWS])
def test_every_row_names_an_exported_entry(row):
    assert hasattr(_lib.load(), row.entry) and row.entry in _lib.EXPORTS
    assert 1 <= row.shape["S"] <= cm.S_MAX and row.shape["n"] >= 1 and 1 <= row.shape["rows"] < 2 ** 31


def test_invalid_shapes_are_refused_on_the_host():
    """bad S, n, rows or a missing pointer: MAPDN_E_INVALID before any launch (no GPU is needed to be told so; the pointers are never read)"""
    lib = _lib.load()
    buf = torch.zeros(64 * 64)
    p = buf.data_ptr()

    def call(n=6, S=10, rows=30, x=p, col=p, delta=p, out=p):
        return lib.mapdn_critic_head_counterfactual(x, n, col, delta, S, p, p, 1e-5, p, p, p, p, out, None, rows, None)
    codes = [call(S=0), call(S=-1), call(S=cm.S_MAX + 1), call(n=0), call(n=-3), call(rows=0), call(rows=-16), call(rows=2 ** 31),
             call(x=None), call(col=None), call(delta=None), call(out=None)]
    assert codes == [-1] * len(codes), codes             # MAPDN_E_INVALID (include/mapdn.h)


def test_the_learner_predicate(monkeypatch):
    cr = MLPCritic(7, 1, make_alg_args(3, 5, 1))
    x = types.SimpleNamespace(is_cuda=True, dtype=torch.float32, dim=lambda: 2, shape=(4096, 64))
    assert critic_cf_ok(cr, x, 4096, 1) and not critic_cf_ok(cr, x, 4096, 2) and not critic_cf_ok(cr, x, 512, 1)
    assert not critic_cf_ok(cr, types.SimpleNamespace(is_cuda=False, dtype=torch.float32, dim=lambda: 2, shape=(4096, 64)), 4096, 1)
    assert not critic_cf_ok(MLPCritic(7, 1, make_alg_args(3, 5, 1, hid_activation="tanh")), x, 4096, 1)
    assert not critic_cf_ok(MLPCritic(7, 1, make_alg_args(3, 5, 1, layernorm=False)), x, 4096, 1)
    monkeypatch.setenv("MAPDN_FUSED_CF", "0")
    assert not critic_cf_ok(cr, x, 4096, 1)
