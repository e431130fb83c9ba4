"""CPU: action_gradients on handles of the sparse solver (mapdn_env_config.grad_meshed = 1; csrc/grad_sparse.hpp, csrc/grad_sparse.hip;
DESIGN.md section 24) without a GPU —
  1. the transposition: the exported elimination program, executed in numpy on the transposed blocks of the oracle's Jacobian for every
     S that fits, against numpy.linalg.solve(J.T, c); the kernel's block formulas restated in numpy give those blocks, and on k9_hv (a
     150 degree vector-group shift: Ybus is not symmetric) they do NOT when Y_ij stands in for Y_ji;
  2. csrc/grad_sparse.hpp and csrc/grad.hpp built for the host (tests/grad_sparse_check.cpp): the assembly's blocks against the
     transpose of meshed_edge_nets.program_jacobian, the right-hand side against the reference's c;
  3. the reference tests/grad_ref.py against central differences of the oracle's predicted reward on meshed nets, on rows that keep
     clear of every kink;
  4. host-only handles: the switch, what it lets through and what stays refused, by name;
  5. the E64 constants of the GPU bars."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from mapdn_amd import _lib
from mapdn_amd.netspec import add_fused_buses, case33_meshed, make_case
from oracle.env_restated import BARRIER_IDS
from tests import grad_ref as G
from tests import grad_sparse_cases as GS
from tests import kernel_matrix as km
from tests import meshed_edge_nets as M
from tests import whatif_cases as W
from tests.test_action_grad_cpu import line_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 4
# 1. the worst error of the emulated program on transposed blocks against numpy.linalg.solve(J.T, c), relative to |lambda|inf, over
# PROGRAM_NETS x every S that fits, measured on the CPU (k9_hv at S = 32); the bound is ten times that
PROGRAM_MEASURED = 3.70e-14
PROGRAM_TOL = 10 * PROGRAM_MEASURED
# 3. env ids whose solved rows keep clear of the kinks (searched on the CPU with the oracle alone; test_kink_condition asserts it) and
# the worst disagreement between the reference and a central difference of the oracle's predicted reward, relative to the row's
# |g|inf, over every row at H and H / 2 (wheel_rim); the bound is ten times that
CPU_ENVS = dict(crowded_meshed=(0, 1, 2), tri3=(0, 1, 2), wheel_rim=(0, 1, 2))
V_MARGIN, Q_MARGIN = 1e-4, 1e-6
H = 2e-4
CD_MEASURED = 4.595e-8
CD_TOL = 10 * CD_MEASURED
HOST_TOL = 1e-12                                              # as tests/grad_check.cpp's transposed solve
# 2. the right-hand side is checked at the pool env with the nominal loads (load scale 1).  At env 0 (load scale 0.02) the net is all
# but unloaded: the line term of c is then the difference of numbers |g| |V|^2 ~ 650 p.u. that are 4e3 times larger than |c|inf, and
# float64 itself leaves 1.1e-12 of |c|inf there on k9_hv (measured against the longdouble c), whatever the code.
RHS_ENV = 2
assert M.LOAD_SCALES[RHS_ENV] == 1.0


# ---- 1. the transposition -----------------------------------------------------------------------------------------------------------------
PROGRAM_CASES = [(key, 64 // L) for key in GS.PROGRAM_NETS for L in GS.fits(key)]


@pytest.mark.parametrize("key,S", PROGRAM_CASES, ids=[f"{k}-S{s}" for k, s in PROGRAM_CASES])
def test_program_on_transposed_blocks_solves_the_adjoint_system(key, S):
    net = GS.make(key)[0]
    V = GS.converged_pool_voltage(key)
    n, pos, dims, ops, slots = GS.host_program(key, S)
    J = M.program_jacobian(net, pos, V)
    c = np.random.default_rng(5 + n + S).uniform(-1.0, 1.0, 2 * n)
    got = M.emulate_program(n, S, dims, ops, slots, np.ascontiguousarray(J.T), c)
    want = np.linalg.solve(J.T, c)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"\n[grad sparse] {key} S={S}: transposed program, relative error {err:.2e} (bound {PROGRAM_TOL:.1e})")
    assert err <= PROGRAM_TOL, (key, S, err)


@pytest.mark.parametrize("key", GS.PROGRAM_NETS)
def test_block_formulas_give_the_transpose_and_need_y_ji(key):
    """slot (i, j) = (J_ji)' from A_ji = V_j conj(Y_ji V_i), in numpy: the transpose of the oracle's Jacobian; with Y_ij in place of
    Y_ji the same only where Ybus is symmetric — not on k9_hv"""
    net = GS.make(key)[0]
    V = GS.converged_pool_voltage(key)
    n, pos, *_ = GS.host_program(key, 64 // GS.fits(key)[0])
    J = M.program_jacobian(net, pos, V)
    Yp, Vp = GS.ybus_by_position(net, pos), V[np.array(pos)]
    scale = np.abs(J).max()
    assert np.abs(GS.transposed_blocks_from_ybus(Yp, Vp) - J.T).max() <= HOST_TOL * scale
    asym = np.abs(Yp - Yp.T).max()
    wrong = np.abs(GS.transposed_blocks_from_ybus(Yp, Vp, swap=True) - J.T).max()
    if key == "k9_hv":
        assert asym > 1.0 and wrong > 1e-3 * scale, (asym, wrong)        # Ybus is not symmetric, and the blocks show it
    else:
        assert asym == 0.0


# ---- 2. csrc/grad_sparse.hpp and csrc/grad.hpp on the host -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("grad_sparse")
    exe = str(d / "grad_sparse_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "mapdn_amd", "csrc"),
                        os.path.join(ROOT, "tests", "grad_sparse_check.cpp"), "-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(rec):
        fi, fo = str(d / "in.bin"), str(d / "out.bin")
        np.ascontiguousarray(rec, dtype=np.float64).tofile(fi)
        p = subprocess.run([exe, fi, fo], capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stderr)
        return np.fromfile(fo, dtype=np.float64)
    return run


@pytest.mark.parametrize("key", ["tri3", "k9_hv"])
def test_host_blocks_against_the_transposed_jacobian(host_check, key):
    net = GS.make(key)[0]
    V = GS.converged_pool_voltage(key)
    n, pos, *_ = GS.host_program(key, 4)
    J = M.program_jacobian(net, pos, V)
    Yp, Vp = GS.ybus_by_position(net, pos), V[np.array(pos)]
    y = np.stack([Yp.real, Yp.imag], axis=-1)
    got = host_check(np.concatenate([[0, n], y.ravel(), Vp.real, Vp.imag])).reshape(2 * n, 2 * n)
    err = float(np.abs(got - J.T).max() / np.abs(J).max())
    print(f"\n[grad sparse host] {key}: blocks of J', relative error {err:.2e}")
    assert err <= HOST_TOL, (key, err)
    if key == "k9_hv":
        assert np.abs(Yp - Yp.T).max() > 1.0


@pytest.mark.parametrize("args", [(("voltage_barrier_type", b),) for b in G.BARRIER_TYPES] + [G.LINE_ARGS], ids=lambda a: str(a[0][1]))
@pytest.mark.parametrize("key", ["tri3", "k9_hv"])
def test_host_right_hand_side_against_the_reference(host_check, key, args):
    net = GS.make(key)[0]
    V = GS.converged_pool_voltage(key, RHS_ENV)
    n, pos, *_ = GS.host_program(key, 4)
    cfg = dict(voltage_barrier_type="bowl", voltage_weight=1.0, q_weight=0.1, line_weight=None)
    cfg.update(dict(args))
    Vp = V[np.array(pos)]
    lines = line_records(net, pos[:n])
    head = [net.n_bus, int(cfg["line_weight"] is not None), BARRIER_IDS[cfg["voltage_barrier_type"]], cfg["voltage_weight"],
            cfg["q_weight"] or 0.0, cfg["line_weight"] or 0.0, net.sn_mva]
    got = host_check(np.concatenate([[1, n, lines.shape[0]], Vp.real, Vp.imag, np.abs(Vp), head, lines.ravel()])).reshape(n, 2)
    c_th, c_vm = GS.reference_c(net, cfg, V, ext=True)                # (in longdouble: the float64 form loses 1e-12 itself on k9_hv's lines)
    p = np.array(pos[:n])
    want = np.stack([c_th[p], c_vm[p] * np.abs(V[p].astype(G.CLD))], axis=1)     # the kernel's unknowns are (theta, u = d|V| / |V|)
    scale = np.abs(want).max()
    err = float(np.abs(got - want).max() / scale) if scale > 0 else float(np.abs(got).max())
    print(f"\n[grad sparse host] {key} {dict(args)}: right-hand side, relative error {err:.2e}")
    assert err <= HOST_TOL, (key, args, err)


# ---- 3. the reference against central differences on meshed nets ----------------------------------------------------------------------------
@pytest.mark.parametrize("key", GS.CD_NETS)
def test_kink_condition(key):
    os_, rows, cand, solved = GS.reference(key, CPU_ENVS[key], K)
    assert (solved == W.expected_pattern(K)).all()
    dv, dq = GS.kink_margins(os_, rows, cand)
    assert dv >= V_MARGIN and dq >= Q_MARGIN, (key, dv, dq)
    assert (cand[:, 0] == 0.0).all()


@pytest.mark.parametrize("key", GS.CD_NETS)
def test_reference_against_central_differences(key):
    os_, rows, cand, solved = GS.reference(key, CPU_ENVS[key], K)
    worst = 0.0
    for i, o in enumerate(os_):
        for k in range(K):
            if solved[i, k]:
                g = G.reward_gradient(o.net, G.env_args(o), rows[i][k]["r"].V, cand[i, k], G.limits(o))
                for h in (H, H / 2):
                    worst = max(worst, G.rel_inf(GS.central_difference(key, o, cand[i, k], h), g))
    print(f"\n[grad sparse cd] {key}: worst relative disagreement {worst:.3e} (bound {CD_TOL:.1e})")
    assert worst <= CD_TOL, (key, worst)


# ---- 4. the C ABI on host-only handles ---------------------------------------------------------------------------------------------------
ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0)
OLD_MESHED_TEXT = "action_gradients: meshed nets and handles on another solver than the tree solver are not supported"


def host_handle(lib, net, tuning=None):
    cn, keep = _lib.make_cnetspec(net)
    cc = _lib.make_cconfig(ARGS, tuning=tuning)
    h = C.c_void_p()
    rc = lib.mapdn_create(C.byref(cn), C.byref(cc), 4, -1, C.byref(h))
    return rc, h, keep


def call(lib, h):
    one = C.c_void_p(1)
    rc = lib.mapdn_action_gradients(h, one, 1, 1, one, one, one, one, None, None, None)
    return rc, lib.mapdn_last_error(h).decode()


def test_field_in_header_struct_and_make_cconfig(lib):
    hdr = open(os.path.join(ROOT, "include", "mapdn.h")).read()
    body = hdr[hdr.index("typedef struct mapdn_env_config"):hdr.index("} mapdn_env_config;")]
    fields = re.findall(r"^\s*(?:int32_t|double|uint64_t|int64_t)\s+([\w, ]+);", body, flags=re.M)
    names = [n.strip() for f in fields for n in f.split(",")]
    assert names[-2:] == ["xcd_map", "grad_meshed"]
    assert [f[0] for f in _lib.CEnvConfig._fields_][-2:] == ["xcd_map", "grad_meshed"] and _lib.CEnvConfig._fields_[-1][1] is C.c_int32
    assert "grad_meshed" in _lib.TUNING_INT and "MAPDN_GRAD_MESHED" in hdr
    assert _lib.make_cconfig(ARGS).grad_meshed == 0 and _lib.make_cconfig(ARGS, tuning=dict(grad_meshed=1)).grad_meshed == 1


def test_kernel_lists():
    assert W.global_kernels("grad_sparse.hip") == ["k_action_grad_sparse"]
    assert W.global_kernels("grad.hip") == ["k_action_grad"]
    assert W.global_kernels("sparse.hip") == ["k_nr_sparse"]


def test_meshed_handle_with_the_switch_stops_at_the_host_only_refusal(lib):
    net = case33_meshed(make_case("case33")[0], 5)
    for tuning, want_rc, text in ((None, -1, OLD_MESHED_TEXT), (dict(grad_meshed=0), -1, OLD_MESHED_TEXT), (dict(grad_meshed=1), -4, "host-only")):
        rc, h, keep = host_handle(lib, net, tuning)
        assert rc == 0
        try:
            assert _lib.nr_kernel(h)["solver"] == 1
            got, msg = call(lib, h)
            assert got == want_rc and (msg == text if want_rc == -1 else text in msg), (tuning, got, msg)
        finally:
            lib.mapdn_destroy(h)


def test_radial_handles_with_the_switch(lib):
    """a radial net pinned to the sparse solver answers with the switch and is refused without; on the tree solver the switch changes
    nothing; nr_init = 2 is accepted on the sparse solver as on the tree"""
    net = make_case("case33")[0]
    for tuning, want_rc in ((dict(nr_solver="sparse"), -1), (dict(nr_solver="sparse", grad_meshed=1), -4), (dict(grad_meshed=1), -4),
                            (dict(nr_solver="sparse", grad_meshed=1, nr_init="dc"), -4)):
        rc, h, keep = host_handle(lib, net, tuning)
        assert rc == 0
        try:
            got, msg = call(lib, h)
            assert got == want_rc, (tuning, got, msg)
            if want_rc == -1:
                assert msg == OLD_MESHED_TEXT
        finally:
            lib.mapdn_destroy(h)


@pytest.mark.parametrize("which,word", [("dense", "dense"), ("zip", "ZIP"), ("gen", "generators"), ("gen_start", "start"), ("fused", "fused")])
def test_still_refused_with_the_switch(lib, which, word):
    net = case33_meshed(make_case("case33")[0], 5)
    tuning = dict(grad_meshed=1)
    if which == "dense":
        tuning["nr_solver"] = "dense"
    elif which == "zip":
        net = km.make_net("case33_zip")[0]
        tuning["nr_solver"] = "sparse"
    elif which == "gen":
        net = dataclasses.replace(net, gen_bus=np.array([3], np.int32), gen_p_mw=np.array([0.1]), gen_vm_pu=np.array([1.0]), gen_scaling=np.array([1.0]))
    elif which == "gen_start":
        net = dataclasses.replace(net, vm_init_pu=net.ext_grid_vm_pu + 0.01)
    else:
        net = add_fused_buses(make_case("case33")[0], [3, 7])
        tuning["nr_solver"] = "sparse"
    rc, h, keep = host_handle(lib, net, tuning)
    assert rc == 0, lib.mapdn_last_error(None)
    try:
        assert _lib.nr_kernel(h)["solver"] == (2 if which == "dense" else 1)
        got, msg = call(lib, h)
        assert got == -1 and msg.startswith("action_gradients:") and word in msg and "not supported" in msg, (which, got, msg)
    finally:
        lib.mapdn_destroy(h)


def test_other_values_of_the_switch_are_refused_at_create(lib):
    net = make_case("case33")[0]
    for v in (2, -1):
        rc, h, keep = host_handle(lib, net, dict(grad_meshed=v))
        assert rc == -1 and "grad_meshed" in lib.mapdn_last_error(None).decode(), (v, rc)


# ---- 5. the E64 constants of the GPU bars ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,args", list(GS.E64), ids=[n + "".join("-" + str(v) for _, v in a) for n, a in GS.E64])
def test_e64_constants_are_what_the_float64_reference_gives(key, args):
    got = GS.e64(key, args)
    print(f"\n[grad sparse e64] {key} {dict(args)}: {got:.2e} (constant {GS.E64[(key, args)]:.2e})")
    assert 0.5 * GS.E64[(key, args)] <= got <= 2.0 * GS.E64[(key, args)], (key, args, got)
