"""CPU: voltage_vjp (mapdn_voltage_vjp, csrc/vjp.hpp) without a GPU —
  1. the reference tests/vjp_ref.py against central differences of the oracle's |V| and angles in the actions, on the envs and with the
     step sizes of tests/test_action_grad_cpu.py, for random cotangents and unit cotangents on single buses;
  2. csrc/vjp.hpp built for the host (tests/vjp_check.cpp), g++ -O2 and again with -fsanitize=address,undefined: one factorisation and
     M = 3 cotangents in k_voltage_vjp's order against the extended reference;
  3. with the barrier's cotangent the reference is tests/grad_ref.reward_gradient minus its direct term;
  4. a host-only handle names a bad argument first and then what the tree solve does not cover;
  5. the header, the exports, the kernel sets and the source hash."""
import ctypes as C
import dataclasses
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from mapdn_amd import _lib, build
from mapdn_amd.netspec import add_fused_buses, case33_meshed, make_case
from oracle.pp_restated import make_ybus
from tests import grad_edge_nets as EN
from tests import grad_ref as G
from tests import kernel_matrix as km
from tests import opf_kernel_cases as OK
from tests import vjp_ref as VR
from tests import whatif_cases as W
from tests.test_action_grad_cpu import CPU_ENVS, H, K, host_handle, seven_bus_state, special_state
from tests.test_opf_cpu import tree_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CD_NETS = ("tiny", "small17", "special", "crowded", "case33")
M_CD = 4                                                          # random, unit on a |V|, unit on an angle, random
# The worst disagreement between the reference and a central difference of the oracle's sum_b cot_vm_b |V_b| + cot_va_b va_degree_b,
# relative to the row's |g|inf, over every solved row of CD_NETS and every cotangent at H and at H / 2, measured on the CPU (DESIGN.md
# section 29: `tiny`, whose truncation error at H shows; every other net stays below 3.8e-8); the bound is ten times that (section 22's
# rule).
CD_MEASURED = 5.803e-7
CD_TOL = 10 * CD_MEASURED
ULP = np.finfo(np.float64).eps


@functools.lru_cache(maxsize=None)
def rows_of(name):
    """the solved rows of a net's scenario: dicts of the oracle env o, the candidate a and the power-flow result r"""
    os_, ref, cand = G.reference(name, CPU_ENVS[name], K)
    assert (ref["solved"] == W.expected_pattern(K)).all(), name
    return [dict(o=o, a=cand[e, k], r=ref["rows"][e][k]["r"]) for e, o in enumerate(os_) for k in range(K) if ref["solved"][e, k]]


def voltages(name, o, a):
    p = W.predict(name, o, a)
    assert p["solved"]
    V = p["r"].V
    return np.abs(V), np.degrees(np.angle(V))


# ---- 1. the reference against central differences ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CD_NETS)
def test_reference_against_central_differences(name):
    worst = 0.0
    for i, r in enumerate(rows_of(name)):
        o, a = r["o"], r["a"]
        net, lim = o.net, G.limits(o)
        cvm, cva = VR.cotangents(net, M_CD, seed=100 + i)
        g = np.stack([VR.voltage_vjp(net, r["r"].V, lim, cvm[m], cva[m]) for m in range(M_CD)])
        for h in (H, H / 2):
            cd = np.zeros_like(g)
            for j in range(net.n_sgen):
                ap, am = a.copy(), a.copy()
                ap[j] += h
                am[j] -= h
                (vp, tp), (vn, tn) = voltages(name, o, ap), voltages(name, o, am)
                cd[:, j] = (cvm @ (vp - vn) + cva @ (tp - tn)) / (2 * h)
            worst = max(worst, max(G.rel_inf(cd[m], g[m]) for m in range(M_CD)))
    print(f"\n[vjp cd] {name}: worst relative disagreement {worst:.3e} (bound {CD_TOL:.1e})")
    assert worst <= CD_TOL, (name, worst)


def test_slack_entries_are_not_read_and_the_slack_sgen_gets_zero():
    r = rows_of("special")[0]
    o = r["o"]
    net, lim, j = o.net, G.limits(o), 8
    assert int(net.sgen_bus[j]) == int(net.ext_grid_bus)
    cvm, cva = VR.cotangents(net, 1, seed=7)
    g = VR.voltage_vjp(net, r["r"].V, lim, cvm[0], cva[0])
    cvm[0, net.ext_grid_bus], cva[0, net.ext_grid_bus] = np.nan, np.nan
    g2 = VR.voltage_vjp(net, r["r"].V, lim, cvm[0], cva[0])
    assert np.array_equal(g, g2) and g[j] == 0.0 and np.isfinite(g).all()


# ---- 2. csrc/vjp.hpp on the host -------------------------------------------------------------------------------------------------------------
def chain40_state():
    os_, ref, cand = G.reference("chain40", (0,), EN.K_MAX)
    o = os_[0]
    assert ref["solved"][0, 1]
    return o.net, ref["rows"][0][1]["r"].V, G.limits(o), cand[0, 1]


STATES = dict(seven_bus=seven_bus_state, special=special_state, chain40=chain40_state)
M_HOST = 3


@pytest.fixture(scope="module", params=["O2", "sanitized"])
def host_vjp(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("vjp_" + request.param)
    exe = str(d / "vjp_check")
    flags = ["-O2"] if request.param == "O2" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run(["g++", *flags, "-std=c++17", "-I", os.path.join(ROOT, "mapdn_amd", "csrc"), os.path.join(ROOT, "tests", "vjp_check.cpp"),
                        "-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(rec):
        fi, fo = str(d / "in.bin"), str(d / "out.bin")
        np.ascontiguousarray(rec, dtype=np.float64).tofile(fi)
        p = subprocess.run([exe, fi, fo], capture_output=True, text=True)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr)
        return np.fromfile(fo, dtype=np.float64)
    return run


@pytest.mark.parametrize("which", list(STATES))
def test_host_sweeps_against_the_extended_reference(host_vjp, which):
    """one factorisation, then M = 3 cotangents by the two transposed sweeps on the stored factors, in k_voltage_vjp's order, against the
    extended reference at the same V: within 16 x the float64 reference's own error and never tighter than 64 ulp of the row's largest
    entry (tests/opf_kernel_cases.bar's rule)"""
    net, V, lim, _ = STATES[which]()
    slack = int(net.ext_grid_bus)
    bus_of_pos, par, cptr, cidx, yt = tree_tables(make_ybus(net)[0].toarray(), slack, net.ext_grid_vm_pu)
    n = net.n_bus - 1
    if which == "chain40":                                         # one chain, rooted at the slack's neighbour: every node has one child
        assert par[n - 1] == n and bus_of_pos[n - 1] == 1 and all(par[k] == k + 1 for k in range(n - 1))
    pos = {b: i for i, b in enumerate(bus_of_pos)}
    Vp = V[bus_of_pos]
    cvm, cva = VR.cotangents(net, M_HOST, seed=31)
    sg = np.array([[pos.get(int(b), n), lim[j], net.sgen_scaling[j]] for j, b in enumerate(net.sgen_bus)])
    cot = np.stack([cvm[:, bus_of_pos], cva[:, bus_of_pos]], axis=2)                  # [M][n][2]
    out = host_vjp(np.concatenate([[n, len(cidx), net.n_sgen, M_HOST], par, cptr, cidx, yt.ravel(), Vp.real, Vp.imag, np.abs(Vp),
                                   [net.sn_mva], sg.ravel(), cot.ravel()]))
    got, va = out[:M_HOST * net.n_sgen].reshape(M_HOST, net.n_sgen), out[M_HOST * net.n_sgen:]
    assert np.abs(va - np.degrees(np.angle(Vp))).max() <= 4 * ULP * 180.0
    for m in range(M_HOST):
        ext = VR.voltage_vjp(net, V, lim, cvm[m], cva[m], ext=True)
        e64 = G.rel_inf(VR.voltage_vjp(net, V, lim, cvm[m], cva[m]), ext)
        err = G.rel_inf(got[m], ext)
        bar = max(OK.BAR_FACTOR * e64, OK.BAR_FLOOR)
        print(f"\n[vjp host] {which} m={m}: e64 {e64:.2e} host {err:.2e} bar {bar:.2e}")
        assert err <= bar, (which, m, err, bar)
        for j, b in enumerate(net.sgen_bus):
            if int(b) == slack:
                assert got[m, j] == 0.0, (which, m, j)


# ---- 3. consistency with action_gradients ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CD_NETS)
def test_barrier_cotangent_gives_the_reward_gradient_without_its_direct_term(name):
    for r in rows_of(name):
        o, a, V = r["o"], r["a"], r["r"].V
        lim = G.limits(o)
        g = VR.voltage_vjp(o.net, V, lim, VR.barrier_cotangent(o, np.abs(V)), None)
        want = G.reward_gradient(o.net, G.env_args(o), V, a, lim) - VR.direct_term(o, a, lim)
        scale = max(np.abs(want).max(), np.abs(G.reward_gradient(o.net, G.env_args(o), V, a, lim)).max())
        assert np.abs(g - want).max() <= 64 * ULP * scale, (name, np.abs(g - want).max(), scale)


# ---- 4. the C ABI on a host-only handle ---------------------------------------------------------------------------------------------------
def refused_net(which):
    net, _ = make_case("case33")
    tuning = None
    if which.startswith("sparse"):
        net, tuning = case33_meshed(net, 5), dict(grad_meshed=int(which[-1]))
    elif which == "dense":
        tuning = dict(nr_solver="dense")
    elif which == "zip":
        net = km.make_net("case33_zip")[0]
    elif which == "gen":
        net = dataclasses.replace(net, gen_bus=np.array([3], np.int32), gen_p_mw=np.array([0.1]), gen_vm_pu=np.array([1.0]), gen_scaling=np.array([1.0]))
    else:
        net = add_fused_buses(net, [3, 7])
    return net, tuning


@pytest.mark.parametrize("which,word", [("sparse0", "sparse solver"), ("sparse1", "sparse solver"), ("dense", "dense solver"), ("zip", "ZIP"),
                                        ("gen", "generators"), ("fused", "fused")])
def test_named_refusals_on_host_only_handle(lib, which, word):
    net, tuning = refused_net(which)
    h, keep = host_handle(lib, net, tuning=tuning)
    try:
        one = C.c_void_p(1)
        rc = lib.mapdn_voltage_vjp(h, one, 1, 1, 1, one, None, one, None, None, one, None, None)
        msg = lib.mapdn_last_error(h).decode()
        assert rc == -1 and msg.startswith("voltage_vjp:") and word in msg and msg.endswith("not supported"), (which, rc, msg)
        # the argument checks come first: a bad K on a refused handle names K
        rc = lib.mapdn_voltage_vjp(h, one, 1, 0, 1, one, None, one, None, None, one, None, None)
        assert rc == -1 and "n_candidates" in lib.mapdn_last_error(h).decode()
    finally:
        lib.mapdn_destroy(h)


def test_argument_refusals_on_host_only_handle(lib):
    net, _ = make_case("case33")
    one = C.c_void_p(1)
    h, keep = host_handle(lib, net)
    try:
        #      actions dtype K  M  cot_vm cot_va grad vm    va    status iterations stream
        ok = [one, 1, 3, 2, one, None, one, None, None, one, None, None]
        for change, word in (({2: 0}, "n_candidates"), ({2: 1025}, "n_candidates"), ({3: -1}, "n_cotangents"), ({3: 1025}, "n_cotangents"),
                             ({4: None}, "cot_vm or cot_va"), ({3: 0}, "grad must be NULL"), ({6: None}, "grad must be NULL"),
                             ({1: 7}, "dtype"), ({0: None}, "null buffer"), ({9: None}, "null buffer")):
            call = list(ok)
            for i, v in change.items():
                call[i] = v
            rc = lib.mapdn_voltage_vjp(h, *call)
            msg = lib.mapdn_last_error(h).decode()
            assert rc == -1 and msg.startswith("voltage_vjp:") and word in msg, (change, rc, msg)
        for call in (ok, [one, 1, 1024, 1024, None, one, one, one, one, one, one, None], [one, 0, 1, 0, None, None, None, None, None, one, None, None]):
            assert lib.mapdn_voltage_vjp(h, *call) == -4, lib.mapdn_last_error(h).decode()    # MAPDN_E_STATE: a host-only handle launches nothing
        assert lib.mapdn_voltage_vjp(None, *ok) == -1
    finally:
        lib.mapdn_destroy(h)


# ---- 5. header, exports, kernel sets, source hash -----------------------------------------------------------------------------------------
def test_header_exports_and_kernel_sets(lib):
    from tests.test_capi_cpu import test_exports_match_header
    test_exports_match_header(lib)
    hdr = open(os.path.join(ROOT, "include", "mapdn.h")).read()
    assert "int mapdn_voltage_vjp(" in hdr and "#define MAPDN_VJP_MAX_COTANGENTS 1024" in hdr
    assert "mapdn_voltage_vjp" in _lib.EXPORTS and hasattr(lib, "mapdn_voltage_vjp")
    assert W.global_kernels("vjp.hip") == ["k_voltage_vjp", "k_vjp_mask"]
    assert W.global_kernels("grad.hip") == ["k_action_grad"] and W.global_kernels("grad_sparse.hip") == ["k_action_grad_sparse"]
    assert W.global_kernels("whatif.hip") == ["k_whatif_start", "k_whatif_score"]
    src = open(os.path.join(W.CSRC, "kernels.hip")).read()
    assert src.rstrip().endswith('#include "vjp.hip"')


def test_source_hash_covers_the_new_files(tmp_path, monkeypatch):
    assert {"vjp.hpp", "vjp.hip"} <= set(build.HEADERS)
    before = build.source_hash()
    copy = tmp_path / "csrc"
    shutil.copytree(build.CSRC, copy)
    (tmp_path / "include").mkdir()
    shutil.copy(os.path.join(ROOT, "include", "mapdn.h"), tmp_path / "include" / "mapdn.h")
    # build.HEADERS reaches the header as ../../include/mapdn.h from csrc
    nested = tmp_path / "pkg" / "csrc"
    nested.parent.mkdir()
    shutil.move(str(copy), str(nested))
    monkeypatch.setattr(build, "CSRC", str(nested))
    assert build.source_hash() == before
    for f in ("vjp.hpp", "vjp.hip"):
        with open(nested / f, "a") as fh:
            fh.write("\n// edited\n")
        after = build.source_hash()
        assert after != before, f
        before = after
