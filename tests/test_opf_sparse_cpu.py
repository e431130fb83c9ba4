"""CPU: the OPF baseline on handles of the sparse solver (mapdn_opf_config.meshed = 1; csrc/opf_sparse.hpp, csrc/opf_sparse.hip;
DESIGN.md section 25) without a GPU —
  1. the exported elimination program, executed in numpy on the blocks of the oracle's Jacobian with TWO right-hand sides in the two
     columns of its right-hand-side blocks, for every net and every S that fits, against the extended reference; a column does not
     depend on what it is paired with;
  2. csrc/opf_sparse.hpp built for the host (tests/opf_sparse_check.cpp): the blocks against meshed_edge_nets.program_jacobian, M V,
     g and H against tests/opf_ref.linearise, g on k9_hv against central differences of the oracle's loss;
  3. the conditions the GPU tests stand on, by the reference alone;
  4. host-only handles: the switch, what it lets through and what stays refused; the layout of mapdn_opf_config;
  5. the E64 constants of the bars."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from mapdn_amd import _lib
from mapdn_amd.baselines import OPFConfig
from mapdn_amd.netspec import add_fused_buses, case33_meshed, make_case
from oracle.pp_restated import make_ybus
from tests import grad_sparse_cases as GS
from tests import kernel_matrix as km
from tests import meshed_edge_nets as M
from tests import opf_kernel_cases as K
from tests import opf_ref as R
from tests import opf_sparse_cases as OS
from tests import whatif_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD_MESHED_TEXT = "opf: meshed nets and handles on another solver than the tree solver are not supported"
STATE_ENV = 2                                    # a noon env with random set-points and pinned sgens
FD_H, FD_BOUND = 1e-3, 1e-6                      # tests/test_opf_kernels_gpu.py's figures


def state(key, e=STATE_ENV):
    """(net, V of the oracle at the env's set-points, lim)"""
    net = OS.make(key)[0]
    _, _, pv, smax = OS.inputs(key, e)
    return net, OS.oracle_voltage(key, e, OS.setpoints(key, OS.B_MAX)[e]).V, R.limits(pv, smax)


# ---- 1. the program with two columns a run -----------------------------------------------------------------------------------------------
PROGRAM_CASES = [(key, 64 // L) for key in OS.NETS for L in OS.fits(key)]


@pytest.mark.parametrize("key,S", PROGRAM_CASES, ids=[f"{k}-S{s}" for k, s in PROGRAM_CASES])
def test_program_with_paired_columns_gives_the_sensitivities(key, S):
    net, V, lim = state(key)
    ref = K.linearise_ext(net, V, lim)
    got = OS.columns_by_program(key, S, V, lim)
    err = K.rel_err(got, ref.S)
    print(f"\n[opf sparse] {key} S={S}: paired columns, S relative error {err:.2e} (bar {OS.bar(key, 'S'):.2e})")
    assert err <= OS.bar(key, "S"), (key, S, err)
    ns = net.n_sgen
    if ns > 1:                                   # the same column beside another partner (and scaled): the same bits in column 0
        other = OS.columns_by_program(key, S, V, lim, partner=1)
        assert np.array_equal(got[:, 0::2], other[:, 0::2]), (key, S)
        assert K.rel_err(other, ref.S) <= OS.bar(key, "S")
    for j, b in enumerate(net.sgen_bus):
        if b == net.ext_grid_bus:
            assert (got[:, j] == 0).all()


# ---- 2. csrc/opf_sparse.hpp on the host ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("opf_sparse")
    exe = str(d / "opf_sparse_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "mapdn_amd", "csrc"),
                        os.path.join(ROOT, "tests", "opf_sparse_check.cpp"), "-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(key, V, lim):
        net = OS.make(key)[0]
        n, pos, *_ = OS.host_program(key, 4)
        ns = net.n_sgen
        Yp, Vp = GS.ybus_by_position(net, pos), V[np.array(pos)]
        node = {int(b): i for i, b in enumerate(pos)}
        rec = np.concatenate([[n, ns], np.stack([Yp.real, Yp.imag], axis=-1).ravel(), Vp.real, Vp.imag,
                              [node[int(b)] for b in net.sgen_bus], lim * net.sgen_scaling / net.sn_mva])
        fi, fo = str(d / "in.bin"), str(d / "out.bin")
        np.ascontiguousarray(rec, dtype=np.float64).tofile(fi)
        p = subprocess.run([exe, fi, fo], capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stderr)
        out = np.fromfile(fo, dtype=np.float64)
        cut = np.cumsum([4 * n * n, 2 * n, 1, ns, ns * ns, n * ns])
        assert out.shape[0] == cut[-1]
        J, mv, loss, g, H, S = np.split(out, cut[:-1])
        Sb = np.zeros((net.n_bus, ns))
        Sb[np.array(pos[:n])] = S.reshape(n, ns)
        return dict(J=J.reshape(2 * n, 2 * n), mv=mv.reshape(n, 2) @ [1, 1j], loss=float(loss[0]), g=g, H=H.reshape(ns, ns), S=Sb, pos=pos)
    return run


@pytest.mark.parametrize("key", ["tri3", "k9_hv"])
def test_host_blocks_rows_of_m_and_sums(host_check, key):
    net, V, lim = state(key)
    got = host_check(key, V, lim)
    pos, n = got["pos"], net.n_bus - 1
    J = M.program_jacobian(net, pos, V)
    err = float(np.abs(got["J"] - J).max() / np.abs(J).max())
    print(f"\n[opf sparse host] {key}: blocks of J, relative error {err:.2e}")
    assert err <= 1e-12, (key, err)
    Y = make_ybus(net)[0].toarray()
    if key == "k9_hv":
        assert np.abs(Y - Y.T).max() > 1.0                                   # Ybus is not symmetric: the imaginary part of M matters
    Mh = 0.5 * (Y + Y.conj().T)
    mv = (Mh @ V)[np.array(pos[:n])]
    assert np.abs(got["mv"] - mv).max() <= 64 * np.finfo(np.float64).eps * np.abs(Y).max() * np.abs(V).max()
    ybus = make_ybus(net)[0]
    ref = K.linearise_ext(net, V, lim)
    errs = dict(S=K.rel_err(got["S"], ref.S), g=K.rel_err(got["g"], ref.g), H=K.rel_err(got["H"], ref.H), loss=K.rel_err([got["loss"]], [ref.loss]))
    L = R.linearise(net, V, lim)
    plain = dict(S=K.rel_err(L.S, ref.S), g=K.rel_err(L.g, ref.g), H=K.rel_err(L.H, ref.H), loss=K.rel_err([R.loss_pu(ybus, V)], [ref.loss]))
    print(f"[opf sparse host] {key}: host", {q: f"{v:.2e}" for q, v in errs.items()}, "opf_ref.linearise", {q: f"{v:.2e}" for q, v in plain.items()})
    for q, v in errs.items():
        assert v <= OS.bar(key, q), (key, q, v, OS.bar(key, q))
    assert np.array_equal(got["H"], got["H"].T)


def test_host_gradient_against_central_differences_with_a_phase_shifter(host_check):
    """the oracle's loss V^H Ybus V is summed in numpy.longdouble here: on this lightly loaded net the float64 sum cancels to 1e-8 of
    the loss (E64's loss column), which over 2 h = 2e-3 is 2.6e-6 of |g|inf — the extended reference shows the same gap — whatever g is"""
    key, e = "k9_hv", STATE_ENV
    net, _, lim = state(key, e)
    Yx = make_ybus(net)[0].toarray().astype(K.CLD)
    lp, lq, pv, _ = OS.inputs(key, e)
    a = np.clip(OS.setpoints(key, OS.B_MAX)[e], -0.9, 0.9)                   # (keep a +- h inside the box)
    solve = lambda x: OS.runpp_of(key)(net, lp, lq, pv, lim * x).V
    got = host_check(key, solve(a), lim)

    def f(x):
        Vx = solve(x).astype(K.CLD)
        return float((Vx.conj() @ (Yx @ Vx)).real)
    eye = np.eye(net.n_sgen)
    fd = np.array([(f(a + FD_H * eye[j]) - f(a - FD_H * eye[j])) / (2.0 * FD_H) for j in range(net.n_sgen)])
    err = float(np.abs(fd - got["g"]).max() / np.abs(fd).max())
    print(f"\n[opf sparse host] {key}: g against central differences {err:.2e} (bound {FD_BOUND:.0e})")
    assert err <= FD_BOUND, err


# ---- 3. the conditions of the GPU tests, by the reference alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("key", OS.LOOP_NETS + ("case33_meshed",))
def test_reference_converges_on_the_chosen_rows(key):
    scale = 1.0 if key == "case33_meshed" else OS.LOOP_SCALE
    runs = [OS.reference_run(key, e, scale) for e in range(6)]               # (the states repeat with period 6)
    print(f"\n[opf sparse ref] {key} x{scale}: status", [r.status for r in runs], "power flows", [r.iterations for r in runs])
    assert all(r.status == 0 for r in runs), key
    if key in OS.LOOP_NETS:
        assert all(OS.reference_run(key, e, 1.0).status == 0 for e in range(6)), key


@pytest.mark.parametrize("key", OS.CAPPED_NETS)
def test_reference_hits_the_qp_cap_under_the_narrow_band(key):
    r = OS.reference_run(key, OS.CAPPED_ENV, OS.CAPPED_SCALE, OS.CAPPED_BAND)
    print(f"\n[opf sparse ref] {key}: status {r.status} after {r.iterations} power flows, violation {r.violation:.3e}")
    assert r.status == 1 and r.iterations < 50 and r.violation > 5e-6, key


@pytest.mark.parametrize("key", list(OS.ACTIVE_BAND))
def test_reference_has_an_active_voltage_row_at_status_0(key):
    band = OS.ACTIVE_BAND[key]
    r = OS.reference_run(key, OS.ACTIVE_ENV, 1.0, band)
    rows = OS.active_rows(key, OS.ACTIVE_ENV, band)
    print(f"\n[opf sparse ref] {key} band {band}: status {r.status}, {rows} voltage rows on a bound")
    assert r.status == 0 and rows >= 1, key


def test_k9_hv_needs_the_dc_start():
    from oracle.pp_restated import runpp_restated
    net = OS.make("k9_hv")[0]
    lp, lq, pv, smax = OS.inputs("k9_hv", 0)
    assert not runpp_restated(net, lp, lq, pv, np.zeros(net.n_sgen)).converged
    assert OS.runpp_of("k9_hv")(net, lp, lq, pv, np.zeros(net.n_sgen)).converged


# ---- 4. the C ABI on host-only handles ------------------------------------------------------------------------------------------------------
def test_meshed_handle_with_the_switch_stops_at_the_host_only_refusal():
    for key in ("case33_meshed", "tri3"):
        for cfg, want_rc, text in ((None, -1, OLD_MESHED_TEXT), (dict(meshed=0), -1, OLD_MESHED_TEXT), (dict(meshed=1), -4, "host-only"),
                                   (OPFConfig(meshed=1), -4, "host-only")):
            rc, msg = OS.opf_error(key, cfg)
            assert rc == want_rc and (msg == text if want_rc == -1 else (text in msg and "not supported" not in msg)), (key, cfg, rc, msg)


def test_radial_handles_with_the_switch():
    """a radial net pinned to the sparse solver answers with the switch and is refused without; on the tree solver the switch changes
    nothing; nr_init = 2 is accepted as on the tree"""
    for tune, cfg, want_rc in ((dict(nr_solver="sparse"), None, -1), (dict(nr_solver="sparse"), dict(meshed=1), -4), (None, dict(meshed=1), -4),
                               (None, None, -4), (dict(nr_solver="sparse", nr_init="dc"), dict(meshed=1), -4), (dict(nr_init="dc"), None, -4)):
        rc, msg = OS.opf_error("case33", cfg, tune)
        assert rc == want_rc, (tune, cfg, rc, msg)
        if want_rc == -1:
            assert msg == OLD_MESHED_TEXT


def test_other_values_of_the_switch_are_invalid():
    for key, tune in (("case33", None), ("case33_meshed", None)):
        for v in (2, -1):
            rc, msg = OS.opf_error(key, dict(meshed=v), tune)
            assert rc == -1 and msg == "opf: meshed must be 0 or 1", (key, v, rc, msg)


def test_dense_handles_stay_refused_by_name():
    rc, msg = OS.opf_error("case33_meshed", dict(meshed=1), dict(nr_solver="dense"))
    assert rc == -1 and msg.startswith("opf:") and "dense" in msg and "not supported" in msg, (rc, msg)
    rc, msg = OS.opf_error("case33_meshed", None, dict(nr_solver="dense"))
    assert rc == -1 and msg == OLD_MESHED_TEXT


@pytest.mark.parametrize("which,text", [
    ("zip", "opf: voltage-dependent (ZIP) loads are not supported"), ("fused", "opf: fused buses are not supported"),
    ("sgens", "opf: more than 64 sgens are not supported"), ("gen", "opf_actions: nets with generators"), ("gen_start", "opf_actions: a start other than ext_grid_vm_pu")])
def test_still_refused_with_the_switch_in_todays_words(which, text):
    net = case33_meshed(make_case("case33")[0], 5)
    tune = None
    if which == "zip":
        net, tune = km.make_net("case33_zip")[0], dict(nr_solver="sparse")
    elif which == "fused":
        net, tune = add_fused_buses(make_case("case33")[0], [3, 7]), dict(nr_solver="sparse")
    elif which == "sgens":
        buses = (6 + np.arange(65) % 27).astype(np.int32)                     # (buses 6 .. 32 lie in the non-main zones)
        net = dataclasses.replace(net, sgen_bus=buses, sgen_zone=np.asarray(net.bus_zone)[buses].astype(np.int32), sgen_scaling=np.zeros(0))
    elif which == "gen":
        net = dataclasses.replace(net, gen_bus=np.array([3], np.int32), gen_p_mw=np.array([0.1]), gen_vm_pu=np.array([1.0]), gen_scaling=np.array([1.0]))
    else:
        net = dataclasses.replace(net, vm_init_pu=net.ext_grid_vm_pu + 0.01)
    for cfg in (dict(meshed=1), None):
        rc, msg = OS.opf_error("case33", cfg, tune, net=net)
        if cfg is None:                             # (every handle here is on the sparse solver)
            assert rc == -1 and msg == OLD_MESHED_TEXT
        else:
            assert rc == -1 and msg.startswith(text), (which, cfg, rc, msg)
    assert text in open(os.path.join(ROOT, "mapdn_amd", "csrc", "baselines_host.hpp")).read()


def test_opf_config_layout_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = [f[0] for f in _lib.COPFConfig._fields_]
    assert fields[-2:] == ["max_backtrack", "meshed"] and _lib.COPFConfig._fields_[-1][1] is C.c_int32
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mapdn.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(mapdn_opf_config));\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(mapdn_opf_config, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == C.sizeof(_lib.COPFConfig)
    for line in out[1:]:
        if line:
            name, off = line.split()
            assert getattr(_lib.COPFConfig, name).offset == int(off), name
    hdr = open(os.path.join(ROOT, "include", "mapdn.h")).read()
    body = hdr[hdr.index("typedef struct mapdn_opf_config"):hdr.index("} mapdn_opf_config;")]
    names = [n.strip() for f in re.findall(r"^\s*(?:int32_t|double)\s+([\w, ]+);", body, flags=re.M) for n in f.split(",")]
    assert names == fields
    assert _lib.make_opf_config(None).meshed == 0 and _lib.make_opf_config(OPFConfig()).meshed == 0
    assert _lib.make_opf_config(OPFConfig(meshed=1)).meshed == 1 and _lib.make_opf_config(dict(meshed=1)).meshed == 1


def test_kernel_lists():
    assert W.global_kernels("opf_sparse.hip") == ["k_opf_sens_sparse", "k_opf_reduce_sparse"]
    assert W.global_kernels("opf.hip") == ["k_opf_linearise", "k_opf_qp", "k_opf_update"]
    assert W.global_kernels("grad_sparse.hip") == ["k_action_grad_sparse"]


# ---- 5. the E64 constants of the bars -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", OS.NETS)
def test_e64_constants_are_what_the_float64_reference_gives(key):
    got = OS.e64(key)
    print(f"\n[opf sparse e64] {key}:", {q: f"{v:.2e}" for q, v in got.items()})
    for q in K.QUANTITIES:
        want = OS.E64[key][q]
        assert (want == 0.0 and got[q] == 0.0) or 0.5 * want <= got[q] <= 2.0 * want, (key, q, got[q], want)
