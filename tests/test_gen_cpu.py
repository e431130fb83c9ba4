"""Generators (net.gen: GEN BUSES — |V| held, P given, Q free) without a GPU: the converter (from_pandapower(gens="runpp"), load_scenario,
MAPDN_GENS), NetSpec validation and the netspec.npz round trip, the refusals of the converter and of mapdn_create, the host plan on
host-only handles (geometry, masked flat-start factors, DC angles) and the test-side oracle tests/gen_nets.py::runpp_gen against
runpp_restated, its own residual, a closed form and the power balance."""
import ctypes as C
import dataclasses
import os
import pickle
import subprocess

import numpy as np
import pandas as pd
import pytest

from mapdn_amd import _lib, data
from mapdn_amd.data import from_pandapower, load_netspec, save_netspec
from mapdn_amd.netspec import make_case
from oracle.pp_restated import _cached_ybus, bus_demand, dc_angles, jacobian, runpp_restated
from tests.gen_nets import (RADIAL, gen_case, gen_p_bus, gen_residual_inf, gen_substation, inputs, runpp_gen, start_vm, tiny_case,
                            tiny_net, with_gens)
from tests.zip_nets import with_zip

ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0, voltage_barrier_type="bowl", seed=0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_NETS = RADIAL + ("meshed",)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def host_handle(lib, net, tuning=None, B=64):
    cn, keep = _lib.make_cnetspec(net)
    cc = _lib.make_cconfig(ARGS, 0, tuning)
    h = C.c_void_p()
    rc = lib.mapdn_create(C.byref(cn), C.byref(cc), B, -1, C.byref(h))
    return rc, h, (lib.mapdn_last_error(None) or b"").decode()


# ---- data layer --------------------------------------------------------------------------------------------------------------
def test_converter_refuses_by_default_and_converts_with_gens_runpp():
    pnet = gen_substation()
    with pytest.raises(NotImplementedError, match="net.gen has in-service rows: not part of the MAPDN hot path"):
        from_pandapower(pnet)
    with pytest.raises(ValueError, match="gens"):
        from_pandapower(pnet, gens="yes")
    net = from_pandapower(pnet, gens="runpp")
    assert net.has_gens and net.n_gen == 1                      # the out-of-service row is no gen bus ...
    assert np.array_equal(net.gen_bus, [2]) and np.array_equal(net.gen_p_mw, [0.6]) and np.array_equal(net.gen_vm_pu, [1.01])
    assert np.array_equal(net.gen_scaling, [0.9])
    assert net.vm_init_pu == np.mean([1.02, 1.01, 1.05])        # ... but its vm_pu counts in the start of the PQ buses
    assert net.start_vm_pu == net.vm_init_pu
    one = from_pandapower(gen_substation(out_of_service_row=False), gens="runpp")
    assert one.vm_init_pu == np.mean([1.02, 1.01])
    pnet = gen_substation()
    del pnet["gen"]
    plain = from_pandapower(pnet, gens="runpp")
    assert not plain.has_gens and plain.vm_init_pu == 0.0 and plain.start_vm_pu == 1.02


def test_converter_refuses_what_it_does_not_cover():
    def gen_rows(**over):
        pnet = gen_substation()
        for k, v in over.items():
            pnet["gen"][k] = v
        return pnet
    with pytest.raises(NotImplementedError, match="two in-service gens on one bus"):
        from_pandapower(gen_rows(bus=[2, 2], in_service=[True, True]), gens="runpp")
    with pytest.raises(NotImplementedError, match="ext_grid bus"):
        from_pandapower(gen_rows(bus=[0, 4]), gens="runpp")
    with pytest.raises(NotImplementedError, match="slack=True"):
        from_pandapower(gen_rows(slack=[True, False]), gens="runpp")
    pnet = gen_substation()                                     # a closed bus-bus switch: fused buses
    pnet["switch"] = pd.concat([pnet["switch"], pd.DataFrame({"bus": [4], "element": [5], "et": ["b"], "type": ["CB"], "closed": [True]})],
                               ignore_index=True)
    with pytest.raises(NotImplementedError, match="fused buses"):
        from_pandapower(pnet, gens="runpp")
    pnet = gen_substation()
    pnet["load"]["const_z_percent"] = [0.0, 30.0, 20.0, 50.0, 50.0]
    with pytest.raises(NotImplementedError, match="voltage-dependent loads"):
        from_pandapower(pnet, gens="runpp", zip_loads="runpp")


def test_netspec_validates_the_gen_columns_and_round_trips_them(tmp_path):
    net, _ = make_case("case33")
    assert not net.has_gens and net.n_gen == 0 and net.vm_init_pu == 0.0 and net.start_vm_pu == net.ext_grid_vm_pu
    assert dataclasses.replace(net, vm_init_pu=float("nan")).vm_init_pu == 0.0       # NaN and 0 both mean: derive it
    with pytest.raises(ValueError, match="one entry per gen"):
        dataclasses.replace(net, gen_bus=np.array([3, 4]), gen_p_mw=np.array([0.1]), gen_vm_pu=np.array([1.0, 1.0]))
    with pytest.raises(ValueError, match="gen_vm_pu must be > 0"):
        with_gens(net, [(3, 0.1, 0.0)])
    with pytest.raises(ValueError, match="finite"):
        with_gens(net, [(3, np.nan, 1.0)])
    with pytest.raises(ValueError, match="gen_bus out of range"):
        with_gens(net, [(33, 0.1, 1.0)])
    with pytest.raises(ValueError, match="vm_init_pu"):
        dataclasses.replace(net, vm_init_pu=-1.0)
    g = with_gens(net, [(32, 0.3, 1.02), (2, 0.5, 1.0)], vm_init_pu=1.015)
    assert g.has_gens and g.start_vm_pu == 1.015
    assert with_gens(net, [(32, 0.3, 1.02)]).start_vm_pu == np.mean([1.0, 1.02])
    save_netspec(g, str(tmp_path / "netspec.npz"))
    back = load_netspec(str(tmp_path / "netspec.npz"))
    for k in ("gen_bus", "gen_p_mw", "gen_vm_pu", "gen_scaling"):
        assert np.array_equal(getattr(back, k), getattr(g, k)) and getattr(back, k).dtype == getattr(g, k).dtype
    assert back.vm_init_pu == 1.015
    save_netspec(net, str(tmp_path / "plain.npz"))
    assert load_netspec(str(tmp_path / "plain.npz")).vm_init_pu == 0.0
    z = dict(np.load(str(tmp_path / "netspec.npz")))           # a file written before the fields existed loads without generators
    for k in ("gen_bus", "gen_p_mw", "gen_vm_pu", "gen_scaling", "vm_init_pu"):
        del z[k]
    np.savez_compressed(str(tmp_path / "old.npz"), **z)
    assert not load_netspec(str(tmp_path / "old.npz")).has_gens


def test_mapdn_gens_and_the_env_key_reach_the_converter(tmp_path, monkeypatch):
    (tmp_path / "model.p").write_bytes(pickle.dumps({}))
    monkeypatch.setattr(data, "read_pandapower_pickle", lambda path: gen_substation())
    monkeypatch.setattr(data, "load_profiles_csv", lambda *a, **k: "prof")
    monkeypatch.delenv("MAPDN_GENS", raising=False)
    with pytest.raises(NotImplementedError, match="net.gen"):
        data.load_scenario(str(tmp_path))
    net, _ = data.load_scenario(str(tmp_path), gens="runpp")
    assert net.has_gens
    monkeypatch.setenv("MAPDN_GENS", "runpp")
    net, _ = data.load_scenario(str(tmp_path))
    assert np.array_equal(net.gen_bus, [2])
    with pytest.raises(NotImplementedError):
        data.load_scenario(str(tmp_path), gens="refuse")        # the argument wins over the environment
    from mapdn_amd import env as env_mod
    monkeypatch.delenv("MAPDN_GENS")
    net, _ = env_mod._resolve_data(dict(data_path=str(tmp_path), gens="runpp"))
    assert net.has_gens


# ---- mapdn_create ------------------------------------------------------------------------------------------------------------
def test_mapdn_create_refuses_by_name(lib):
    net, _ = make_case("case33")
    g = with_gens(net, [(32, 0.3, 1.0)])
    rc, h, msg = host_handle(lib, g, dict(nr_solver="dense"))
    assert rc != 0 and "dense" in msg and "generators" in msg
    rc, h, msg = host_handle(lib, with_gens(with_zip(net, 0.3, 0.2), [(32, 0.3, 1.0)]))
    assert rc != 0 and "voltage-dependent loads" in msg and "generators" in msg
    alias = np.arange(net.n_bus); alias[21] = 20
    rc, h, msg = host_handle(lib, dataclasses.replace(g, bus_alias=alias))
    assert rc != 0 and "fused buses" in msg and "generators" in msg
    rc, h, msg = host_handle(lib, with_gens(net, [(int(net.ext_grid_bus), 0.3, 1.0)]))
    assert rc != 0 and "ext_grid bus" in msg and "slack" in msg
    rc, h, msg = host_handle(lib, with_gens(net, [(5, 0.3, 1.0), (5, 0.1, 1.0)]))
    assert rc != 0 and "two in-service gens on one bus" in msg
    rc, h, msg = host_handle(lib, g)
    assert rc == 0, msg
    dims = _lib.CDims()
    assert lib.mapdn_dims(h, C.byref(dims)) == 0 and dims.n_gen == 1
    lib.mapdn_destroy(h)


@pytest.mark.parametrize("name", ["leaf", "mixed", "chain", "all", "c141"])
@pytest.mark.parametrize("init", ["flat", "dc"])
def test_the_gen_geometry_is_the_chooser_s_geometry_without_gens(lib, name, init):
    net, _ = gen_case(name)
    plain = dataclasses.replace(net, gen_bus=np.zeros(0, np.int32), gen_p_mw=np.zeros(0), gen_vm_pu=np.zeros(0), gen_scaling=np.zeros(0))
    out = []
    for n_ in (net, plain):
        rc, h, msg = host_handle(lib, n_, dict(nr_init=init), B=4096)
        assert rc == 0, msg
        g = _lib.nr_geometry(h)
        out.append({k: g[k] for k in ("solver", "waves", "lanes", "lean", "rows", "h_lds", "g_lds", "rec_lds", "flat_lds", "line_lds")})
        lib.mapdn_destroy(h)
    assert out[0] == out[1] and out[0]["solver"] == 0


def masked_jacobian(net, v0):
    """the Newton matrix in the kernels' unknowns z = [dtheta, d|V| / |V|], per bus a 2x2 block, the Q row and the |V| column of every gen
    bus struck out and a 1 on its diagonal; rows / columns (2 b, 2 b + 1) of the non-slack buses in bus order"""
    ybus = _cached_ybus(net)[0]
    nb = net.n_bus
    allb = np.arange(nb)
    J = jacobian(ybus, v0, allb, allb).toarray()               # [[dP/dth, dP/dVm], [dQ/dth, dQ/dVm]]
    vm = np.abs(v0)
    A = np.zeros((2 * nb, 2 * nb))
    A[0::2, 0::2] = J[:nb, :nb]; A[0::2, 1::2] = J[:nb, nb:] * vm[None, :]
    A[1::2, 0::2] = J[nb:, :nb]; A[1::2, 1::2] = J[nb:, nb:] * vm[None, :]
    for b in net.gen_bus:
        A[2 * b + 1, :] = 0.0; A[:, 2 * b + 1] = 0.0; A[2 * b + 1, 2 * b + 1] = 1.0
    keep = np.setdiff1d(np.arange(2 * nb), [2 * net.ext_grid_bus, 2 * net.ext_grid_bus + 1])
    return A[np.ix_(keep, keep)], keep


@pytest.mark.parametrize("name", ["mixed", "chain"])
def test_flat_factors_are_the_factorisation_of_the_masked_jacobian_at_the_rule_3_start(lib, name):
    """mapdn_get_flat_factors replayed on the host (the kernel's flat sweep pair) against numpy's solve of the masked Jacobian at the
    non-uniform start, for an arbitrary Sbus: the bar of tests/test_capi_cpu.py::test_flat_start_factorisation_is_the_first_newton_step"""
    net, prof = gen_case(name)
    rc, h, msg = host_handle(lib, net)
    assert rc == 0, msg
    nb, n = net.n_bus, net.n_bus - 1
    fac = np.zeros((n, 12)); bop = np.zeros(n + 1, np.int32); par = np.zeros(n, np.int32)
    assert lib.mapdn_get_flat_factors(h, _lib._p(fac, _lib._pd), _lib._p(bop, _lib._pi)) == 0
    assert lib.mapdn_get_schedule(h, 1, C.byref(C.c_int32()), None, _lib._p(par, _lib._pi)) == 0
    ins = [x[0] for x in inputs(net, prof, 1, 1)]
    pd_, qd = bus_demand(net, *ins)
    sbus = -((pd_ - gen_p_bus(net)) + 1j * qd) / net.sn_mva
    v0 = np.full(nb, start_vm(net), dtype=np.complex128)       # (the test side's own mean, tests/gen_nets.py)
    v0[net.ext_grid_bus] = net.ext_grid_vm_pu; v0[net.gen_bus] = net.gen_vm_pu
    assert name != "mixed" or len(set(np.abs(v0).tolist())) >= 4   # (`mixed`: a non-uniform start, not the factors of one magnitude)
    ybus = _cached_ybus(net)[0]
    mis = v0 * np.conj(ybus @ v0) - sbus
    F = np.zeros(2 * nb); F[0::2] = mis.real; F[1::2] = mis.imag
    F[2 * net.gen_bus + 1] = 0.0
    A, keep = masked_jacobian(net, v0)
    z = np.zeros(2 * nb); z[keep] = np.linalg.solve(A, F[keep])
    isgen = np.isin(bop[:n], net.gen_bus)
    S = fac[:, 0] + 1j * fac[:, 1]
    Iinv = fac[:, 2:6].reshape(n, 2, 2); apk = fac[:, 6:8]; G = fac[:, 8:12].reshape(n, 2, 2)
    assert np.all(Iinv[isgen, 0, 1] == 0.0) and np.all(Iinv[isgen, 1, 0] == 0.0) and np.all(Iinv[isgen, 1, 1] == 1.0)
    assert np.all(G[isgen, 1, :] == 0.0)
    hvec = np.zeros((n, 2)); acc = np.zeros((n + 1, 2)); x = np.zeros((n + 1, 2))
    for k in range(n):
        Fk = S[k] - sbus[bop[k]]
        rhs = np.array([Fk.real, Fk.imag]) - acc[k]
        if isgen[k]:
            rhs[1] = 0.0                                       # (the kernel's select: r1 = 0 at a gen node)
        hvec[k] = Iinv[k] @ rhs
        ar, ai = apk[k]
        acc[par[k]] += (ai * hvec[k, 0] + ar * hvec[k, 1], ai * hvec[k, 1] - ar * hvec[k, 0])
    for k in range(n - 1, -1, -1):
        x[k] = hvec[k] - G[k] @ (x[par[k]] if par[k] < n else np.zeros(2))
    assert np.abs(x[:n, 0] - z[2 * bop[:n]]).max() < 1e-10
    assert np.abs(x[:n, 1] - z[2 * bop[:n] + 1]).max() < 1e-10
    assert np.all(x[:n][isgen, 1] == 0.0)
    lib.mapdn_destroy(h)


def test_the_library_derives_the_start_itself_when_vm_init_pu_is_zero(lib, monkeypatch):
    """gen rows and vm_init_pu = 0 straight into mapdn_netspec (what a C caller passes): plan.cpp's own mean over the ext_grid and the
    gen rows.  S_calc of a PQ leaf (bus 17 of `mixed`: one neighbour, a PQ bus too) is |V0|^2 conj(Y_kk + Y_kp), so it shows the
    magnitude the library started from; and all factors equal those of a handle that was handed the test side's mean"""
    net, _ = gen_case("mixed")
    want = (1.03 + 1.02 + 1.00 + 1.01) / 4.0
    assert start_vm(net) == want and net.vm_init_pu == 0.0

    def factors():
        rc, h, msg = host_handle(lib, net)
        assert rc == 0, msg
        n = net.n_bus - 1
        fac = np.zeros((n, 12)); bop = np.zeros(n + 1, np.int32)
        assert lib.mapdn_get_flat_factors(h, _lib._p(fac, _lib._pd), _lib._p(bop, _lib._pi)) == 0
        lib.mapdn_destroy(h)
        return fac, bop
    orig = _lib.make_cnetspec
    seen = []

    def zeroed(n_):
        s, keep = orig(n_)
        seen.append(s.vm_init_pu)
        s.vm_init_pu = 0.0
        return s, keep
    given, bop = factors()
    monkeypatch.setattr(_lib, "make_cnetspec", zeroed)
    derived, _ = factors()
    assert seen == [want]                                      # (the Python side had passed the mean; the second handle got 0)
    assert np.array_equal(given, derived)
    ybus = _cached_ybus(net)[0]
    k = int(np.flatnonzero(bop == 17)[0])
    s_calc = want * want * np.conj(ybus[17, 17] + ybus[17, 16])
    assert abs(derived[k, 0] + 1j * derived[k, 1] - s_calc) <= 1e-12 * abs(ybus[17, 17]) * want * want


def test_a_start_other_than_the_ext_grid_set_point_without_gens(lib):
    """only out-of-service gen rows: no gen bus, but vm_init_pu moves the start.  The solvers run their GEN form; what cannot is
    refused by name, without calling the net one with generators"""
    net, _ = make_case("case33")
    moved = dataclasses.replace(net, vm_init_pu=1.02)
    rc, h, msg = host_handle(lib, moved)
    assert rc == 0, msg
    k = _lib.nr_kernel(h)
    assert k["GEN"] == 1 and k["ZIP"] == 0
    dims = _lib.CDims()
    assert lib.mapdn_dims(h, C.byref(dims)) == 0 and dims.n_gen == 0
    lib.mapdn_destroy(h)
    rc, h, msg = host_handle(lib, net)
    assert rc == 0 and _lib.nr_kernel(h)["GEN"] == 0
    lib.mapdn_destroy(h)
    rc, h, msg = host_handle(lib, moved, dict(nr_solver="dense"))
    assert rc != 0 and "vm_init_pu other than ext_grid_vm_pu" in msg and "dense" in msg and "generators" not in msg
    rc, h, msg = host_handle(lib, with_zip(moved, 0.3, 0.2))
    assert rc != 0 and "vm_init_pu other than ext_grid_vm_pu" in msg and "voltage-dependent loads" in msg
    alias = np.arange(net.n_bus); alias[21] = 20
    rc, h, msg = host_handle(lib, dataclasses.replace(moved, bus_alias=alias, line_in_service=np.where((net.line_from_bus == 20) & (net.line_to_bus == 21), 0, 1)))
    assert rc != 0 and "vm_init_pu other than ext_grid_vm_pu" in msg and "fused buses" in msg
    # the converter names the same cases
    pnet = gen_substation()
    pnet["gen"]["in_service"] = [False, False]
    assert from_pandapower(pnet, gens="runpp").n_gen == 0 and from_pandapower(pnet, gens="runpp").vm_init_pu == np.mean([1.02, 1.01, 1.05])
    pnet["load"]["const_z_percent"] = [0.0, 30.0, 20.0, 50.0, 50.0]
    with pytest.raises(NotImplementedError, match="out-of-service net.gen rows"):
        from_pandapower(pnet, gens="runpp", zip_loads="runpp")
    pnet = gen_substation()
    pnet["gen"]["in_service"] = [False, False]
    pnet["switch"] = pd.concat([pnet["switch"], pd.DataFrame({"bus": [4], "element": [5], "et": ["b"], "type": ["CB"], "closed": [True]})],
                               ignore_index=True)
    with pytest.raises(NotImplementedError, match="out-of-service net.gen rows"):
        from_pandapower(pnet, gens="runpp")


@pytest.mark.parametrize("name,solver", [("leaf", "tree"), ("leaf", "sparse"), ("c141", "tree"), ("meshed", "auto")])
def test_dc_angles_with_gens_match_the_oracle(lib, name, solver):
    from tests.dc_nets import hv_front
    net, prof = gen_case(name)
    net = hv_front(net, 150.0)
    assert net.va_init == "dc" and net.has_gens
    rc, h, msg = host_handle(lib, net, dict(nr_solver=solver, nr_init="dc"))
    assert rc == 0, msg
    ins = [x[0] for x in inputs(net, prof, 1, 3)]
    pd_, _ = bus_demand(net, *ins)
    va = np.zeros(net.n_bus)
    assert lib.mapdn_get_dc_angles(h, _lib._p(pd_, _lib._pd), _lib._p(va, _lib._pd)) == 0
    ref = dc_angles(net, pd_ - gen_p_bus(net))
    assert np.abs(va - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert np.abs(ref - dc_angles(net, pd_)).max() > 1e-6      # (P_gen moves the angles: the check above is not vacuous)
    lib.mapdn_destroy(h)


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["case33", "case141"])
def test_runpp_gen_without_gens_is_runpp_restated_bit_for_bit(case):
    net, prof = make_case(case)
    for e in range(4):
        ins = [x[e] for x in inputs(net, prof, 4, 2)]
        a, b = runpp_gen(net, *ins), runpp_restated(net, *ins)
        assert a.iterations == b.iterations and a.converged == b.converged
        for k in ("vm_pu", "va_degree", "p_mw", "q_mvar", "pl_mw", "V", "Sbus"):
            assert np.array_equal(a[k], b[k]), k
        assert a.res_gen["q_mvar"].shape == (0,)


@pytest.mark.parametrize("name", ALL_NETS)
def test_runpp_gen_solves_its_own_equations(name):
    """the residual over [P at pvpq; Q at pq] is below tolerance wherever runpp_gen reports convergence; |V| of a gen bus is its
    set-point; the power balance closes: sum res_bus.p_mw + line losses = 0"""
    net, prof = gen_case(name)
    B = 8
    ins = inputs(net, prof, B, 5)
    n_conv = 0
    for e in range(B):
        x = [a[e] for a in ins]
        r = runpp_gen(net, *x)
        if not r.converged:
            continue
        n_conv += 1
        assert gen_residual_inf(net, r.V, *x) < 1e-8 / net.sn_mva
        assert np.abs(r.vm_pu[net.gen_bus] - net.gen_vm_pu).max() < 1e-13
        assert np.array_equal(r.res_gen["p_mw"], net.gen_p_mw * net.gen_scaling)
        assert abs(r.p_mw.sum() + r.pl_mw.sum()) < 1e-7 * max(1.0, np.abs(r.p_mw).sum())
        # Q balance at a gen bus: what the network takes is what the bus's elements and the generator supply
        assert np.abs(r.q_mvar[net.gen_bus] - (bus_demand(net, *x)[1][net.gen_bus] - r.res_gen["q_mvar"])).max() < 1e-9
    assert n_conv >= (4 if name != "far" else 1)


def test_the_two_bus_net_has_a_closed_form():
    """slack (V1, angle 0) - line y = g + jb - gen bus (|V2| held, P injected): P2 = V2^2 g - V1 V2 (g cos th + b sin th), so
    g cos th + b sin th = |y| cos(th - phi) = (V2^2 g - P2) / (V1 V2) with phi = atan2(b, g), and th = phi + acos(...) (the root that
    is 0 for P2 = 0, V1 = V2)"""
    net = tiny_net(2)
    pl, ql, pv, qs = np.array([0.3]), np.array([0.1]), np.array([0.2]), np.array([0.05])
    r = runpp_gen(net, pl, ql, pv, qs)
    assert r.converged
    base = net.bus_vn_kv[0] ** 2 / net.sn_mva
    y = 1.0 / ((0.5 + 0.4j) / base)
    g, b = y.real, y.imag
    v1, v2 = net.ext_grid_vm_pu, net.gen_vm_pu[0]
    p2 = (net.gen_p_mw[0] - pl[0] + pv[0]) / net.sn_mva
    c = (v2 * v2 * g - p2) / (v1 * v2)
    th = np.arctan2(b, g) + np.arccos(c / abs(y))
    assert abs(np.radians(r.va_degree[1]) - th) < 1e-12 and abs(r.vm_pu[1] - v2) < 1e-15
    # Q the generator supplies: Q2 = -V2^2 b - V1 V2 (g sin th - b cos th), plus the bus's own demand
    q2 = (-v2 * v2 * b - v1 * v2 * (g * np.sin(th) - b * np.cos(th))) * net.sn_mva
    assert abs(r.res_gen["q_mvar"][0] - (q2 + ql[0] - qs[0])) < 1e-10


def test_three_bus_chain_converges_and_holds_the_set_point():
    net, prof = tiny_case(3)
    ins = [x[0] for x in inputs(net, prof, 1, 0)]
    r = runpp_gen(net, *ins)
    assert r.converged and abs(r.vm_pu[2] - 1.02) < 1e-14 and gen_residual_inf(net, r.V, *ins) < 1e-8


# ---- the shared pivot helper under a sanitizer, as a stand-alone host program -----------------------------------------------------
def test_gen_mask_helper_compiles_with_gcc_and_masks_a_pivot(tmp_path):
    """csrc/gen_mask.hpp is plain C++: g++ builds it with -fsanitize=address,undefined into a small program of its own that checks the
    masked pivot of a gen node (I = [[1 / D0, 0], [0, 1]], h1 = 0, G2 = G3 = 0) and that a PQ node is left alone"""
    src = tmp_path / "gen_mask_main.cpp"
    src.write_text('''
#include <cmath>
#include <cstdio>
#include "gen_mask.hpp"
int main() {
  using namespace mapdn;
  for (int gen = 0; gen < 2; ++gen) {
    const double D0 = 3.5;
    double D1 = 0.25, D2 = -0.5, D3 = 2.0, r1 = 0.7;
    gen_mask_pivot(gen != 0, D1, D2, D3, r1);
    const double idet = 1.0 / (D0 * D3 - D1 * D2);
    double I0, I1, I2, I3;
    gen_pivot_inverse(gen != 0, D0, D1, D2, D3, idet, I0, I1, I2, I3);
    double G2 = I2 * 0.3 - I3 * 0.4, G3 = I2 * 0.4 + I3 * 0.3;
    gen_mask_factor(gen != 0, G2, G3);
    const double fq = gen_mask_fq(gen != 0, 0.9);
    if (gen) {
      if (!(D1 == 0 && D2 == 0 && D3 == 1 && r1 == 0 && I0 == 1.0 / D0 && I1 == 0 && I2 == 0 && I3 == 1 && G2 == 0 && G3 == 0 && fq == 0)) return 1;
    } else {
      if (!(D1 == 0.25 && D2 == -0.5 && D3 == 2.0 && r1 == 0.7 && fq == 0.9)) return 2;
      if (std::fabs(I0 * D0 + I1 * D2 - 1.0) > 1e-15 || std::fabs(I2 * D1 + I3 * D3 - 1.0) > 1e-15) return 3;
    }
  }
  std::puts("ok");
  return 0;
}
''')
    exe = tmp_path / "gen_mask_main"
    inc = os.path.join(ROOT, "mapdn_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", inc, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True)
    assert out.stdout.strip() == "ok"
