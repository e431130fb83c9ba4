"""CPU tests of the attention-core kernel matrix (tests/attn_kernel_matrix.py): the rows cover the compiled set parsed from
csrc/critic_attn.hip — a kernel added without a row fails here —, the launch sites are the ones the rows were built for, both entries
refuse bad shapes and pointers on the host before anything is launched, and the learner's predicate agrees with the kernel's limit."""
import re
import types

import pytest
import torch

from mapdn_amd import _lib
from mapdn_amd import learner
from tests import attn_kernel_matrix as am


def test_the_rows_cover_the_compiled_set_exactly():
    ck = am.compiled_kernels()
    assert len(set(ck)) == len(ck), ck
    assert set(ck) == {("attn_fwd",), ("attn_bwd",)}
    have = {k for r in am.ROWS for k in r.kernels}
    assert have == set(ck), (sorted(set(ck) - have), sorted(have - set(ck)))
    labels = [r.label for r in am.ROWS]
    assert len(set(labels)) == len(labels) and [r.label for r in am.rows_for(304)] == labels
    assert {(r.shape["B"], r.shape["n"], r.shape["H"]) for r in am.ROWS} >= {(5, 2, 1), (1, 3, 4), (67, 17, 2), (27, 38, 1), (27, 38, 4), (5, 6, 1)}
    assert {r.special for r in am.ROWS} == {"", "diag", "hot"}
    big = [r for r in am.ROWS if r.label == "big"][0]
    assert big.shape["B"] > am.CUS * am.BLOCKS_PER_CU and big.shape["n"] == 38 and big.shape["H"] == 1
    assert all(2 <= r.shape["n"] <= am.max_agents() and r.shape["H"] in (1, 2, 4) for r in am.ROWS)


def test_a_kernel_without_a_row_is_caught():
    real = am._src
    site = "  hipLaunchKernelGGL(k_attn_fwd, dim3(blocks)"
    assert site in real()
    for new, caught in ((site.replace("k_attn_fwd", "k_attn_fwd2"), True), (site.replace("(k_attn_fwd,", "((k_attn_fwd<true>),"), True), (site, False)):
        am._src = lambda name="critic_attn.hip", _n=new: real(name).replace(site, _n + "; " + site.strip(), 1)
        try:
            if caught:
                with pytest.raises(AssertionError):
                    am.compiled_kernels()
            else:
                assert am.compiled_kernels().count(("attn_fwd",)) == 2          # listed twice: the exact-cover test's duplicate check fails
        finally:
            am._src = real


def test_the_launch_sites():
    """256 threads, min(B, 4 per CU) workgroups, one sample per workgroup and turn, dynamic LDS = operands + two score arrays; the sum of
    logit_sq over the workgroups is k_head_reduce on a partial stride of exactly n H (no pad to zero)"""
    src = am._src()
    assert re.findall(r"hipLaunchKernelGGL\(k_attn_fwd,\s*dim3\((\w+)\),\s*dim3\((\w+)\),\s*(\w+),", src) == [("blocks", "AT_NT", "lds")]
    assert re.findall(r"hipLaunchKernelGGL\(k_attn_bwd,\s*dim3\(([\w()]+)\),\s*dim3\((\w+)\),\s*(\w+),", src) == [("attn_blocks(B)", "AT_NT", "lds")]
    assert "constexpr int AT_NT = 256;" in src and src.count("__launch_bounds__(AT_NT)") == 2
    assert re.search(r"std::min<int64_t>\(B, \(int64_t\)head_cus\(\) \* 4\)", src)
    assert src.count("for (int s = blockIdx.x; s < B; s += gridDim.x)") == 2
    assert re.search(r"hipLaunchKernelGGL\(k_head_reduce, dim3\(\(R \+ 63\) / 64\), dim3\(256\), 0, \(hipStream_t\)stream, \(const float\*\)scratch, blocks, R, 0, R, R, logit_sq\)", src)
    assert "atomic" not in src.lower().replace("no atomics", "")


@pytest.mark.parametrize("name", ["mapdn_attention_forward", "mapdn_attention_backward", "mapdn_attention_scratch_floats", "mapdn_attention_max_agents"])
def test_the_entries_are_exported(name):
    assert hasattr(_lib.load(), name) and name in _lib.EXPORTS


def test_invalid_shapes_are_refused_on_the_host():
    """a null or misaligned pointer, B < 1, n < 2, n above the limit, H not in {1, 2, 4}: MAPDN_E_INVALID before any launch (no GPU is
    needed to be told so; the pointers are never read)"""
    lib = _lib.load()
    buf = torch.zeros(64 * 64)
    p = buf.data_ptr()
    assert p % 16 == 0
    N = lib.mapdn_attention_max_agents()

    def fwd(B=5, n=6, H=1, sel=p, key=p, val=p, out=p, lsq=p, scratch=p):
        return lib.mapdn_attention_forward(sel, key, val, B, n, H, out, lsq, scratch, None)

    def bwd(B=5, n=6, H=1, dout=p, dlsq=p, sel=p, key=p, val=p, dsel=p, dkey=p, dval=p):
        return lib.mapdn_attention_backward(dout, dlsq, sel, key, val, B, n, H, dsel, dkey, dval, None)
    shapes = [dict(B=0), dict(B=-3), dict(n=1), dict(n=0), dict(n=-2), dict(n=N + 1), dict(H=0), dict(H=3), dict(H=8), dict(H=-1), dict(B=2 ** 31 // (6 * 64) + 1)]
    codes = [fwd(**s) for s in shapes] + [fwd(**{k: None}) for k in ("sel", "key", "val", "out", "lsq", "scratch")] + [fwd(sel=p + 4), fwd(out=p + 8)]
    assert codes == [-1] * len(codes), codes             # MAPDN_E_INVALID (include/mapdn.h)
    codes = [bwd(**s) for s in shapes] + [bwd(**{k: None}) for k in ("dout", "dlsq", "sel", "key", "val", "dsel", "dkey", "dval")] + [bwd(dout=p + 4)]
    assert codes == [-1] * len(codes), codes
    assert lib.mapdn_attention_scratch_floats(0, 6, 1) == 0 and lib.mapdn_attention_scratch_floats(5, 6, 3) == 0
    assert lib.mapdn_attention_scratch_floats(5, 6, 2) == 5 * 6 * 2          # one partial per workgroup, min(B, 4 per CU) workgroups


def test_the_learner_predicate(monkeypatch):
    N = am.max_agents()
    assert learner.ATTN_MAX_N == N == _lib.load().mapdn_attention_max_agents()

    def t(B=8, n=6, hid=64, cuda=True, dtype=torch.float32):
        return types.SimpleNamespace(is_cuda=cuda, dtype=dtype, dim=lambda: 3, shape=(B, n, hid))
    assert all(learner.attention_ok(t(), H) for H in (1, 2, 4)) and learner.attention_ok(t(n=2), 1) and learner.attention_ok(t(n=N), 4)
    assert not learner.attention_ok(t(n=N + 1), 1) and not learner.attention_ok(t(n=1), 1)
    assert not learner.attention_ok(t(hid=32), 1) and not learner.attention_ok(t(hid=128), 1)
    assert not learner.attention_ok(t(), 8) and not learner.attention_ok(t(), 3)
    assert not learner.attention_ok(t(cuda=False), 1) and not learner.attention_ok(t(dtype=torch.float64), 1)
    assert not learner.attention_ok(t(B=2 ** 31 // (6 * 64) + 1), 1)
    monkeypatch.setenv("MAPDN_FUSED_ATTN", "0")
    assert not learner.attention_ok(t(), 1)
