"""CPU tests of the Shapley coalition-critic kernel matrix (tests/shap_kernel_matrix.py): the rows cover the compiled set parsed from
csrc/critic_shap.hip — a kernel or instantiation added without a row fails here —, the launch sites are the ones the rows were built
for, every entry refuses bad shapes and pointers on the host before anything is launched, the geometry function reports the LDS budget
and the largest n, and the learner's predicate agrees with the kernel's limit."""
import re
import types

import pytest
import torch
import torch.nn.functional as F

from mapdn_amd import _lib
from mapdn_amd import learner
from tests import shap_kernel_matrix as sm


def test_the_rows_cover_the_compiled_set_exactly():
    ck = sm.compiled_kernels()
    assert len(set(ck)) == len(ck), ck
    assert set(ck) == {("shap_fwd",), ("shap_bwd", True, 256), ("shap_bwd", True, 192), ("shap_bwd", True, 128), ("shap_bwd", False, 256)}
    have = {k for r in sm.ROWS for k in r.kernels()}
    assert have == set(ck), (sorted(set(ck) - have), sorted(have - set(ck)))
    labels = [r.label for r in sm.ROWS]
    assert len(set(labels)) == len(labels) and [r.label for r in sm.rows_for(304)] == labels
    N = sm.max_agents()
    assert {(r.shape["b"], r.shape["n"], r.shape["S"]) for r in sm.ROWS} >= {(5, 1, 1), (5, 2, 1), (1, 3, 3), (7, 17, 2), (3, 38, 10), (2, N, 1)}
    assert {r.special for r in sm.ROWS} == {"", "ident", "reversed", "zero-act", "hot"}
    big = [r for r in sm.ROWS if r.label == "big"][0]
    assert big.shape["b"] == 4 * 4 * sm.CUS + 11 and big.shape["n"] == 3 and big.shape["S"] == 2
    code, threads, blocks, lds, budget, _ = sm.geometry(big.shape["b"], 2, 3, 0)
    assert code == 0 and blocks == 2 * sm.CUS and big.shape["b"] > blocks * 4          # every forward wavefront owns more than one sample
    assert sm.geometry(big.shape["b"], 2, 3, 1)[2] == sm.CUS                            # the reduce sums one partial per CU
    assert all(1 <= r.shape["n"] <= N for r in sm.ROWS)


def test_a_kernel_without_a_row_is_caught():
    real = sm._src
    site = "    return shap_bwd_launch<true, 128>(a, q, dv, dbase, dact, scratch, grads, st);"
    assert site in real()
    for new, caught in ((site.replace("128", "64"), "row"), ("  hipLaunchKernelGGL(k_shap_fwd2, dim3(1), dim3(256), 0, st);", "parse"), (site, "dup")):
        sm._src = lambda name="critic_shap.hip", _n=new: real(name).replace(site, _n + "\n" + site, 1)
        try:
            if caught == "parse":
                with pytest.raises(AssertionError):
                    sm.compiled_kernels()
            elif caught == "row":
                assert ("shap_bwd", True, 64) in sm.compiled_kernels()                  # ... which no row reaches: the exact-cover test fails
                assert ("shap_bwd", True, 64) not in {k for r in sm.ROWS for k in r.kernels()}
            else:
                assert sm.compiled_kernels().count(("shap_bwd", True, 128)) == 2        # listed twice: the duplicate check fails
        finally:
            sm._src = real


def test_the_launch_sites():
    """forward: 256 threads, min(ceil(b / 4), 2 per CU) workgroups; backward: NT threads, min(ceil(b / (NT / 64)), 1 per CU) workgroups; both
    split the SAMPLES over the wavefronts (dbase, dact and phi have one writer); the partials are reduced by k_head_reduce: the trunk's
    HP block with its pad zeroed, then the 2 n 64 column partials; no atomics anywhere"""
    src = sm._src()
    assert re.findall(r"hipLaunchKernelGGL\(k_shap_fwd,\s*dim3\(([\w(), ]+?)\),\s*dim3\((\w+)\),\s*(\w+),", src) == [("shap_blocks(b, 4, 2)", "256", "lds")]
    assert re.findall(r"hipLaunchKernelGGL\(\(k_shap_bwd<PG, NT>\),\s*dim3\((\w+)\),\s*dim3\((\w+)\),\s*(\w+),", src) == [("blocks", "NT", "lds")]
    assert "const int blocks = shap_blocks(q.b, NT / 64, 1), pstride = HP + 2 * a.n * 64;" in src
    assert src.count("(q.b * w / W) * q.S, g1 = (q.b * (w + 1) / W) * q.S") == 2
    assert "hipLaunchKernelGGL(k_head_reduce, dim3((HP + 63) / 64), dim3(256), 0, st, (const float*)scratch, blocks, pstride, 0, HP, HW, grads);" in src
    assert "hipLaunchKernelGGL(k_head_reduce, dim3(2 * a.n), dim3(256), 0, st, (const float*)scratch, blocks, pstride, HP, pstride, pstride, grads);" in src
    assert "atomic" not in src.lower().replace("no atomics", "").replace("__atomic_release", "").replace("__atomic_acquire", "")
    assert src.count("__builtin_amdgcn_mfma_f32_16x16x4f32") == 4 and "ln_stats(" in src and "relu_nan(" in src


@pytest.mark.parametrize("name", ["mapdn_critic_shapley_forward", "mapdn_critic_shapley_backward", "mapdn_critic_shapley_scratch_floats",
                                  "mapdn_critic_shapley_geometry"])
def test_the_entries_are_exported(name):
    assert hasattr(_lib.load(), name) and name in _lib.EXPORTS


def test_the_geometry_function():
    code, threads, blocks, lds, budget, N = sm.geometry(1, 1, 1, 0)
    assert code == 0 and budget == 160 * 1024 and 38 <= N < 256
    for n, nt in ((1, 256), (17, 256), (38, 192), (N, 128)):
        for mode, want in ((0, 256), (1, nt), (2, 256)):
            code, threads, blocks, lds, _, _ = sm.geometry(9, 2, n, mode)
            assert code == 0 and threads == want and 0 < lds <= budget, (n, mode, threads, lds)
    assert sm.geometry(9, 2, N + 1, 1)[0] == -1 and sm.geometry(9, 2, N + 1, 1)[4:] == (budget, N)      # still reports budget and limit
    assert sm.geometry(9, 2, 3, 3)[0] == -1 and sm.geometry(9, 2, 3, 0, -1)[0] == -1
    assert sm.geometry(3, 1, 3, 0)[2] == 1 and sm.geometry(3, 1, 3, 1)[2] == 1           # never more workgroups than ceil(b / wavefronts)


def test_invalid_arguments_are_refused_on_the_host():
    """a null or misaligned pointer, b < 1, S < 1, n < 1, n above the limit, 2^31 rows or more: MAPDN_E_INVALID before any launch (no GPU is
    needed to be told so; the pointers are never read by these checks).  A pos in plain host memory is refused whatever it holds — a row
    that is not a permutation here."""
    lib = _lib.load()
    buf = torch.zeros(64 * 64)
    p = buf.data_ptr()
    assert p % 16 == 0
    N = sm.max_agents()
    pos = torch.zeros(5 * 2 * 6, dtype=torch.int32).data_ptr()             # every position 0: no permutation

    def fwd(b=5, S=2, n=6, base=p, idc=p, actc=p, act=p, pos=pos, gamma=p, beta=p, w2=p, b2=p, w3=p, b3=p, v=p, phi=p):
        return lib.mapdn_critic_shapley_forward(base, idc, actc, act, pos, b, S, n, gamma, beta, 1e-5, w2, b2, w3, b3, v, phi, None)

    def bwd(b=5, S=2, n=6, dv=p, base=p, idc=p, actc=p, act=p, pos=pos, gamma=p, beta=p, w2=p, b2=p, w3=p, b3=p, dbase=p, grads=p, scratch=p,
            dact=p, pg=1):
        return lib.mapdn_critic_shapley_backward(dv, base, idc, actc, act, pos, b, S, n, gamma, beta, 1e-5, w2, b2, w3, b3, dbase, grads, scratch, dact,
                                                 pg, None)
    shapes = [dict(b=0), dict(b=-3), dict(S=0), dict(S=-1), dict(n=0), dict(n=-2), dict(n=N + 1), dict(b=2 ** 31 // 12 + 1), dict(b=2 ** 40)]
    ptrs = ("base", "idc", "actc", "act", "pos", "gamma", "beta", "w2", "b2", "w3", "b3")
    codes = ([fwd(**s) for s in shapes] + [fwd(**{k: None}) for k in ptrs + ("v",)] + [fwd(base=p + 4), fwd(idc=p + 8), fwd(actc=p + 4), fwd(w2=p + 4),
             fwd(act=p + 2), fwd(pos=pos + 1), fwd(v=p + 1), fwd(phi=p + 2)] + [fwd(), fwd(phi=None)])
    assert codes == [-1] * len(codes), codes             # MAPDN_E_INVALID (include/mapdn.h)
    codes = ([bwd(**s) for s in shapes] + [bwd(**{k: None}) for k in ptrs + ("dv", "dbase", "grads", "scratch")] + [bwd(dact=None, pg=0)]
             + [bwd(dbase=p + 4), bwd(dv=p + 2), bwd(dact=p + 1), bwd(base=p + 8)] + [bwd(), bwd(pg=0), bwd(dact=None)])
    assert codes == [-1] * len(codes), codes
    assert lib.mapdn_critic_shapley_scratch_floats(0, 2, 6) == 0 and lib.mapdn_critic_shapley_scratch_floats(5, 2, N + 1) == 0
    assert lib.mapdn_critic_shapley_scratch_floats(5, 0, 6) == 0
    cu1 = lib.mapdn_critic_shapley_scratch_floats(1, 2, 6)
    assert cu1 == 4416 + 2 * 6 * 64                      # one sample: one workgroup's partial [HP | n 64 | n 64]


def test_the_learner_predicate(monkeypatch):
    N = sm.max_agents()
    assert learner.shapley_max_agents() == N
    cr = types.SimpleNamespace(use_ln=True, act=F.relu, layernorm=torch.nn.LayerNorm(64), fc2=torch.nn.Linear(64, 64), fc3=torch.nn.Linear(64, 1))

    def t(b=8, hid=64, cuda=True, dtype=torch.float32):
        return types.SimpleNamespace(is_cuda=cuda, dtype=dtype, dim=lambda: 2, shape=(b, hid))
    assert learner.shapley_ok(cr, t(), 3, 10) and learner.shapley_ok(cr, t(b=1), 1, 1) and learner.shapley_ok(cr, t(), N, 10)
    assert not learner.shapley_ok(cr, t(), N + 1, 10)
    assert not learner.shapley_ok(cr, t(hid=32), 3, 10) and not learner.shapley_ok(cr, t(cuda=False), 3, 10)
    assert not learner.shapley_ok(cr, t(dtype=torch.float64), 3, 10) and not learner.shapley_ok(cr, t(b=2 ** 31 // 30 + 1), 3, 10)
    tanh = types.SimpleNamespace(**dict(vars(cr), act=torch.tanh))
    noln = types.SimpleNamespace(**dict(vars(cr), use_ln=False))
    assert not learner.shapley_ok(tanh, t(), 3, 10) and not learner.shapley_ok(noln, t(), 3, 10)
    monkeypatch.setenv("MAPDN_FUSED_SHAP", "0")
    assert not learner.shapley_ok(cr, t(), 3, 10)
