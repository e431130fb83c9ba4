"""GPU (-m gpu) tests of every compiled power-flow kernel (tests/kernel_matrix.py), one row each:
  * solve_only at a ragged batch: the handle runs the row's kernel; k_nr_tree rows give the bits (vm, va, iterations, converged) of the
    automatic-geometry handle of the same net and variant (canonical child order); every row matches the oracle of its variant
    (runpp_restated, dc_oracle, zip_oracle, gen_oracle) on 8 envs to 1e-9 p.u., with iteration counts under the agreement rule; rows
    with generators also converge on every env and hold every gen bus at its set-point;
  * B = 1 for one row per variant (whole workgroups of padding): the bits of the ragged run's first env;
  * case322 at B = 8192, (4, 16, F, F, 2), inputs tiled from the B = 70 run: every env has the bits of its small-run twin;
  * step mode on a fat case141 layout, with the res_line constants, step records and flat-start constants out of LDS and automatic:
    bit-identical episodes, with the PV-bus injection fused and as its own launch;
  * nets with generators: the mismatch pass against the mismatch-only sweep with an env that never converges, Q_gen and the commit at
    the 322-bus size, and the start-only form (no gen bus, a start other than the ext_grid set-point).
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
from tests.gen_nets import gen_oracle, with_gens
from tests.zip_nets import zip_oracle

pytestmark = pytest.mark.gpu

V_TOL = 1e-9
N_ORACLE = 8


def pool_rule(key, B, seed):
    """seeded inputs (p_load, q_load, p_sgen, q_sgen) of B envs of a net: profile rows and random reactive set-points"""
    net, prof = km.make_net(key)
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, prof.n_rows, B)
    smax = prof.s_max()
    pv = prof.pv[rows]
    qs = rng.uniform(-0.8, 0.8, (B, net.n_sgen)) * np.sqrt(np.maximum(smax ** 2 - pv ** 2, 0.0))
    return prof.load_p[rows], prof.load_q[rows], pv, qs


@functools.lru_cache(maxsize=None)
def pool(key):
    """the inputs of the rows of a net: pool_rule for B_ROW envs, seeded by the key"""
    return pool_rule(key, km.B_ROW, zlib.crc32(key.encode()))


def oracle_envs(B):
    """the envs checked against the oracle: the first, the last and seeded ones between"""
    mid = np.random.default_rng(B).choice(np.arange(1, B - 1), size=min(N_ORACLE - 2, max(B - 2, 0)), replace=False)
    return sorted({0, B - 1, *mid.tolist()})


@functools.lru_cache(maxsize=None)
def oracle(key, e):
    """(result, agreement rule of the iteration count) of env e of the pool, by the oracle of the net's variant"""
    net, _ = km.make_net(key)
    ins = [x[e] for x in pool(key)]
    dc, zip_, gen = km.variant_of(key)
    if gen:
        return gen_oracle(net, *ins)                             # (both starts, through net.va_init)
    if zip_:
        return zip_oracle(net, *ins)
    if dc:
        return dc_oracle(net, *ins)
    r = runpp_restated(net, *ins)
    return r, lambda it, conv: same_newton_count(net, ins, it, conv, r)


def run(key, B, tuning, ins=None):
    """solve_only on a fresh handle: (vm, va, iterations, converged) as numpy, and the kernel the handle reports (printed before it
    runs)"""
    if ins is None:
        ins = [x[:B] for x in pool(key)]
    return run_net(*km.make_net(key), B, tuning, ins, key)


def run_net(net, prof, B, tuning, ins, what):
    env = VoltageControlBatch(net, prof, km.ARGS, n_envs=B, device="cuda:0", obs_dtype=torch.float64, tuning=tuning)
    try:
        kernel = km.kernel_tuple(env.nr_kernel())
        print(f"\n[kernel matrix] {what} B = {B}: {kernel}")
        out = [x.cpu().numpy() for x in env.solve(*ins)]
        return out, kernel
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


def check_oracle(key, out, envs, ref=None):
    """the rows `envs` of a solve against the oracle (`ref(e)`: another one than the key's); the worst |V - V_oracle|"""
    vm, va, it, cv = out
    worst = 0.0
    for i, e in enumerate(envs):
        r, agrees = ref(e) if ref else oracle(key, e)
        assert agrees(it[i], cv[i]), (key, e, int(it[i]), bool(cv[i]), r.iterations, r.converged)
        if r.converged:
            v = vm[i] * np.exp(1j * np.radians(va[i]))
            worst = max(worst, float(np.abs(v - r.V).max()))
    print(f"[kernel matrix] {key}: worst |V - V_oracle| = {worst:.3e} over envs {list(envs)}")
    assert worst <= V_TOL, (key, worst)
    return worst


@pytest.mark.parametrize("row", km.ROWS, ids=km.row_id)
def test_every_compiled_kernel_matches_the_oracle(row):
    out, kernel = run(row.net, row.B, row.tuning)
    assert kernel == row.kernel, (kernel, row)
    assert out[3].mean() >= 0.5, f"{row.net}: only {out[3].mean():.0%} of the envs converge; change the inputs, not the bar"
    envs = oracle_envs(row.B)
    check_oracle(row.net, [x[envs] for x in out], envs)
    if row.kernel[0] != "dense" and row.kernel[-1]:              # generators: the inputs are such that the oracle converges on every env
        net, _ = km.make_net(row.net)
        assert out[3].all(), f"{row.net}: envs {np.nonzero(~out[3].astype(bool))[0].tolist()} do not converge"
        gap = float(np.abs(out[0][:, net.gen_bus] - net.gen_vm_pu).max())
        assert gap <= V_TOL, (row.net, gap)
    if row.kernel[0] == "tree":                                  # (bits are not compared across k_nr_sparse's L: another program)
        ref, ref_kernel = automatic(row.net, row.B)
        assert ref_kernel[0] == "tree" and ref_kernel[6:] == row.kernel[6:], ref_kernel
        assert_same_solution(out, ref, f"{row.kernel} vs the automatic {ref_kernel}")


# one row per (solver, DC, ZIP, GEN): B = 1 leaves all but one lane group of the first workgroup, and every further workgroup, as padding
B1_ROWS = list({(r.kernel[0], *km.variant_of(r.net)): r for r in reversed(km.ROWS)}.values())


@pytest.mark.parametrize("row", B1_ROWS, ids=km.row_id)
def test_one_env_gives_the_bits_of_the_ragged_batch(row):
    one, kernel = run(row.net, 1, row.tuning)
    assert kernel == row.kernel, (kernel, row)
    many, _ = run(row.net, row.B, row.tuning)
    assert_same_solution(one, [x[:1] for x in many], f"{row.kernel}: B = 1 vs B = {row.B}")
    check_oracle(row.net, one, [0])


@pytest.mark.parametrize("suffix", ["", "_hv", "_zip", "_hv_zip", "_gen", "_hv_gen"])
def test_position_invariance_beyond_one_round_of_workgroups(suffix):
    """case322 at B = 8192 runs the 16-envs-per-workgroup layout (4, 16, F, F, 2) over several rounds of workgroups; its inputs are the
    B = 70 pool tiled, and every env gives the bits of the env of the small automatic run with the same inputs"""
    key = "case322" + suffix
    small, small_kernel = automatic(key, km.B_ROW)
    B = 8192
    idx = np.arange(B) % km.B_ROW
    big, kernel = run(key, B, None, [x[idx] for x in pool(key)])
    assert kernel == ("tree", 4, 16, 0, 0, 2, *km.variant_of(key)), kernel
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
            if net.n_gen:                                        # the commit of Q_gen
                trace += [v.clone() for v in env.res_gen().values()]
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in trace], g
    finally:
        env.close()


@pytest.mark.parametrize("fuse", [1, 2], ids=["fused_inject", "separate_inject"])
@pytest.mark.parametrize("suffix", ["", "_hv", "_zip", "_hv_zip", "_gen", "_hv_gen"])
def test_step_mode_without_lds_residents_gives_the_automatic_bits(suffix, fuse):
    """step() is the only caller of the fused res_line epilogue, whose constants come from LDS (nr_line_lds) or from global memory:
    a 6-step episode on a fat (4, 16) case141 layout with the line constants, step records and flat-start constants pinned out of LDS
    gives the bits of the automatic layout (all of them resident) — reward, terminated, info, obs and every result, with generators
    every res_gen column too (the commit of Q_gen)"""
    key = "case141" + suffix
    B = 40
    base = dict(nr_waves=4, nr_lanes=16, nr_lean=2, fuse_inject=fuse)
    off = dict(base, nr_line_lds=2, nr_rec_lds=2, nr_flat_lds=2)
    if "_zip" in suffix or "_gen" in suffix:
        off["nr_h_lds"] = 2                                      # (the ZIP and GEN lists have no h-resident body without the residents)
    a, ga = episode(key, B, base)
    b, gb = episode(key, B, off)
    assert (ga["line_lds"], ga["rec_lds"], ga["flat_lds"]) == (1, 1, 1), ga
    assert (gb["line_lds"], gb["rec_lds"], gb["flat_lds"]) == (0, 0, 0), gb
    assert ga["fuse_inject"] == gb["fuse_inject"] == (1 if fuse == 1 else 0)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert same_bits(x, y), f"{key} fuse_inject={fuse}: trace item {i} differs"


# ---- nets with generators ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["case33_gen", "case141_gen", "case322_gen"])
def test_mismatch_pass_equals_mismatch_sweep_with_generators(key):
    """tests/test_gpu_parity.py::test_mismatch_pass_equals_mismatch_sweep on nets with generators: the pass reads the gen flag from its
    own records (MM_GEN), the sweep from the step records (S_GEN); both drop Fq of a gen node before the verdict, so iterations, flags
    and voltages are bit-identical — also with the predictor forced to 'always'.  Env 11 carries 30 times its loads: the oracle does
    not converge on it (a condition on the inputs)"""
    B = 96
    net, prof = km.make_net(key)
    pl, ql, pv, qs = pool_rule(key, B, 8)
    pl = pl.copy()
    pl[11] *= 30.0
    out = {}
    for tag, mm, always in (("sweep", 2, False), ("pass", 1, False), ("sweep_always", 2, True), ("pass_always", 1, True)):
        tuning = dict(nr_mm_pass=mm)
        if always:
            tuning.update(nr_check_dx=1e30, nr_check_quad=1e-300)
        env = VoltageControlBatch(net, prof, km.ARGS, n_envs=B, device="cuda:0", obs_dtype=torch.float64, tuning=tuning)
        try:
            assert env.geometry()["mm_pass"] == (1 if mm == 1 else 0) and env.nr_kernel()["GEN"] == 1
            out[tag] = [x.cpu().numpy() for x in env.solve(pl, ql, pv, qs)]
        finally:
            env.close()
    vm0, va0, it0, cv0 = out["sweep"]
    r, agrees = gen_oracle(net, pl[11], ql[11], pv[11], qs[11])
    assert not r.converged and agrees(it0[11], cv0[11])
    assert not cv0[11] and it0[11] == 10 and cv0[[0, 1, 50]].all()
    ok = cv0.astype(bool)
    for tag in ("pass", "sweep_always", "pass_always"):
        vm, va, it, cv = out[tag]
        assert np.array_equal(it, it0) and np.array_equal(cv, cv0), tag
        assert same_bits(vm[ok], vm0[ok]) and same_bits(va[ok], va0[ok]), tag


@pytest.mark.parametrize("solver", ["tree", "sparse"])
def test_q_gen_and_the_commit_at_the_322_bus_size(solver):
    """tests/test_gen_gpu.py::test_q_gen_and_the_commit_after_a_step on case322_gen, with its bars (tests/gen_nets.py::q_bars): the hub
    gen's Ybus row has six terms, and one gen sits beside the slack, where Q_gen is large and sensitive to the voltage"""
    from tests.test_gen_gpu import check_q_gen_and_the_commit
    net, prof = km.make_net("case322_gen")
    check_q_gen_and_the_commit(net, prof, solver, "case322_gen")


@pytest.mark.parametrize("base,solver", [("case141", "tree"), ("case141", "sparse"), ("case33_meshed", "sparse")])
def test_the_start_only_form_matches_the_oracle(base, solver):
    """a net without a gen bus whose PQ buses start at 1.02 p.u. (what out-of-service gen rows leave behind) runs the GEN form of its
    kernel with no flag set"""
    net, prof = km.make_net(base)
    net = with_gens(net, [], vm_init_pu=1.02)
    assert net.n_gen == 0
    ins = pool(base)
    out, kernel = run_net(net, prof, km.B_ROW, dict(nr_solver=solver), ins, f"{base} from 1.02 p.u.")
    assert kernel[0] == solver and kernel[-2:] == (0, 1), kernel
    envs = oracle_envs(km.B_ROW)
    check_oracle(f"{base} from 1.02 p.u.", [x[envs] for x in out], envs, lambda e: gen_oracle(net, *(x[e] for x in ins)))
