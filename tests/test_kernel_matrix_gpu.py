"""GPU (-m gpu) tests of every compiled power-flow kernel (tests/kernel_matrix.py), one row each:
  * solve_only at a ragged batch: the handle runs the row's kernel; k_nr_tree rows give the bits (vm, va, iterations, converged) of the
    automatic-geometry handle of the same net and variant (canonical child order); every row matches the oracle of its variant
    (runpp_restated, dc_oracle, zip_oracle) on 8 envs to 1e-9 p.u., with iteration counts under the agreement rule;
  * B = 1 for one row per variant (whole workgroups of padding): the bits of the ragged run's first env;
  * case322 at B = 8192, (4, 16, F, F, 2), inputs tiled from the B = 70 run: every env has the bits of its small-run twin;
  * step mode on a fat case141 layout, with the res_line constants, step records and flat-start constants out of LDS and automatic:
    bit-identical episodes, with the PV-bus injection fused and as its own launch.
Handles are made one at a time and closed; inputs, automatic-handle results and oracle results are cached per net."""
import functools
import zlib

import numpy as np
import pytest
import torch

from mapdn_amd.env import VoltageControlBatch
from oracle.pp_restated import runpp_restated
from tests import kernel_matrix as km
from tests.dc_nets import dc_oracle
from tests.edge_rule import same_newton_count
from tests.zip_nets import zip_oracle

pytestmark = pytest.mark.gpu

V_TOL = 1e-9
N_ORACLE = 8


def _row_id(r):
    return f"{r.net}-" + "-".join(str(x) for x in r.kernel)


@functools.lru_cache(maxsize=None)
def pool(key):
    """seeded inputs (p_load, q_load, p_sgen, q_sgen) of B_ROW envs of a net: profile rows and random reactive set-points"""
    net, prof = km.make_net(key)
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    rows = rng.integers(0, prof.n_rows, km.B_ROW)
    smax = prof.s_max()
    pv = prof.pv[rows]
    qs = rng.uniform(-0.8, 0.8, (km.B_ROW, net.n_sgen)) * np.sqrt(np.maximum(smax ** 2 - pv ** 2, 0.0))
    return prof.load_p[rows], prof.load_q[rows], pv, qs


def oracle_envs(B):
    """the envs checked against the oracle: the first, the last and seeded ones between"""
    mid = np.random.default_rng(B).choice(np.arange(1, B - 1), size=min(N_ORACLE - 2, max(B - 2, 0)), replace=False)
    return sorted({0, B - 1, *mid.tolist()})


@functools.lru_cache(maxsize=None)
def oracle(key, e):
    """(result, agreement rule of the iteration count) of env e of the pool, by the oracle of the net's variant"""
    net, _ = km.make_net(key)
    ins = [x[e] for x in pool(key)]
    dc, zip_ = km.variant_of(key)
    if zip_:
        return zip_oracle(net, *ins)
    if dc:
        return dc_oracle(net, *ins)
    r = runpp_restated(net, *ins)
    return r, lambda it, conv: same_newton_count(net, ins, it, conv, r)


def run(key, B, tuning, ins=None):
    """solve_only on a fresh handle: (vm, va, iterations, converged) as numpy, and the kernel the handle reports"""
    net, prof = km.make_net(key)
    if ins is None:
        ins = [x[:B] for x in pool(key)]
    env = VoltageControlBatch(net, prof, km.ARGS, n_envs=B, device="cuda:0", obs_dtype=torch.float64, tuning=tuning)
    try:
        out = [x.cpu().numpy() for x in env.solve(*ins)]
        return out, km.kernel_tuple(env.nr_kernel())
    finally:
        env.close()


@functools.lru_cache(maxsize=None)
def automatic(key, B):
    return run(key, B, None)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.uint8) == b.view(np.uint8)).all())


def assert_same_solution(out, ref, what):
    for name, x, y in zip(("vm", "va", "iterations", "converged"), out, ref):
        if not same_bits(x, y):
            bad = np.nonzero((x != y).reshape(x.shape[0], -1).any(axis=1))[0]
            raise AssertionError(f"{what}: {name} differs in {len(bad)} envs, first {bad[:8].tolist()}")


def check_oracle(key, out, envs):
    vm, va, it, cv = out
    worst = 0.0
    for i, e in enumerate(envs):
        r, agrees = oracle(key, e)
        assert agrees(it[i], cv[i]), (key, e, int(it[i]), bool(cv[i]), r.iterations, r.converged)
        if r.converged:
            v = vm[i] * np.exp(1j * np.radians(va[i]))
            worst = max(worst, float(np.abs(v - r.V).max()))
    assert worst <= V_TOL, (key, worst)


@pytest.mark.parametrize("row", km.ROWS, ids=_row_id)
def test_every_compiled_kernel_matches_the_oracle(row):
    out, kernel = run(row.net, row.B, row.tuning)
    assert kernel == row.kernel, (kernel, row)
    assert out[3].mean() >= 0.5, f"{row.net}: only {out[3].mean():.0%} of the envs converge; change the inputs, not the bar"
    envs = oracle_envs(row.B)
    check_oracle(row.net, [x[envs] for x in out], envs)
    if row.kernel[0] == "tree":                                  # (bits are not compared across k_nr_sparse's L: another program)
        ref, ref_kernel = automatic(row.net, row.B)
        assert ref_kernel[0] == "tree" and ref_kernel[6:] == row.kernel[6:], ref_kernel
        assert_same_solution(out, ref, f"{row.kernel} vs the automatic {ref_kernel}")


# one row per (solver, DC, ZIP): B = 1 leaves all but one lane group of the first workgroup, and every further workgroup, as padding
B1_ROWS = list({(r.kernel[0], *km.variant_of(r.net)): r for r in reversed(km.ROWS)}.values())


@pytest.mark.parametrize("row", B1_ROWS, ids=_row_id)
def test_one_env_gives_the_bits_of_the_ragged_batch(row):
    one, kernel = run(row.net, 1, row.tuning)
    assert kernel == row.kernel, (kernel, row)
    many, _ = run(row.net, row.B, row.tuning)
    assert_same_solution(one, [x[:1] for x in many], f"{row.kernel}: B = 1 vs B = {row.B}")
    check_oracle(row.net, one, [0])


@pytest.mark.parametrize("suffix", ["", "_hv", "_zip", "_hv_zip"])
def test_position_invariance_beyond_one_round_of_workgroups(suffix):
    """case322 at B = 8192 runs the 16-envs-per-workgroup layout (4, 16, F, F, 2) over several rounds of workgroups; its inputs are the
    B = 70 pool tiled, and every env gives the bits of the env of the small automatic run with the same inputs"""
    key = "case322" + suffix
    dc, zip_ = km.variant_of(key)
    small, small_kernel = automatic(key, km.B_ROW)
    B = 8192
    idx = np.arange(B) % km.B_ROW
    big, kernel = run(key, B, None, [x[idx] for x in pool(key)])
    assert kernel == ("tree", 4, 16, 0, 0, 2, dc, zip_), kernel
    assert small_kernel != kernel
    assert_same_solution(big, [x[idx] for x in small], f"{kernel} at B = {B} vs {small_kernel} at B = {km.B_ROW}")


STEP_ARGS = dict(km.ARGS, seed=11)


def episode(key, B, tuning, n_steps=6):
    net, prof = km.make_net(key)
    env = VoltageControlBatch(net, prof, STEP_ARGS, n_envs=B, device="cuda:0", obs_dtype=torch.float64, tuning=tuning)
    try:
        g = env.geometry()
        rng = np.random.default_rng(5)
        obs, _ = env.reset()
        trace = [obs.clone()]
        for _ in range(n_steps):
            act = torch.as_tensor(rng.uniform(-0.8, 0.8, (B, net.n_sgen)), device="cuda:0")
            r, term, info = env.step(act)
            trace += [r.clone(), term.clone(), info.clone(), env.get_obs().clone()]
            trace += [v.clone() for v in env.results().values()]
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in trace], g
    finally:
        env.close()


@pytest.mark.parametrize("fuse", [1, 2], ids=["fused_inject", "separate_inject"])
@pytest.mark.parametrize("suffix", ["", "_hv", "_zip", "_hv_zip"])
def test_step_mode_without_lds_residents_gives_the_automatic_bits(suffix, fuse):
    """step() is the only caller of the fused res_line epilogue, whose constants come from LDS (nr_line_lds) or from global memory:
    a 6-step episode on a fat (4, 16) case141 layout with the line constants, step records and flat-start constants pinned out of LDS
    gives the bits of the automatic layout (all of them resident) — reward, terminated, info, obs and every result"""
    key = "case141" + suffix
    B = 40
    base = dict(nr_waves=4, nr_lanes=16, nr_lean=2, fuse_inject=fuse)
    off = dict(base, nr_line_lds=2, nr_rec_lds=2, nr_flat_lds=2)
    if "_zip" in suffix:
        off["nr_h_lds"] = 2                                      # (the ZIP list has no h-resident body without the residents)
    a, ga = episode(key, B, base)
    b, gb = episode(key, B, off)
    assert (ga["line_lds"], ga["rec_lds"], ga["flat_lds"]) == (1, 1, 1), ga
    assert (gb["line_lds"], gb["rec_lds"], gb["flat_lds"]) == (0, 0, 0), gb
    assert ga["fuse_inject"] == gb["fuse_inject"] == (1 if fuse == 1 else 0)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert same_bits(x, y), f"{key} fuse_inject={fuse}: trace item {i} differs"
