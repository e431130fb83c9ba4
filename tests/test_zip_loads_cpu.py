"""Voltage-dependent (ZIP) loads without a GPU: the converter (from_pandapower(zip_loads="runpp"), load_scenario, MAPDN_ZIP_LOADS),
NetSpec validation and the netspec.npz round trip, the refusals of the converter and of mapdn_create, and the test-side oracle
tests/zip_nets.py::runpp_zip against closed forms and runpp_restated."""
import ctypes as C
import dataclasses
import pickle

import numpy as np
import pandas as pd
import pytest

from mapdn_amd import _lib, data
from mapdn_amd.data import from_pandapower, load_netspec, save_netspec
from mapdn_amd.netspec import NetSpec, case33_meshed, make_case
from oracle.pp_restated import runpp_restated
from tests.dc_nets import hv_front
from tests.test_data_ingestion import substation_net
from tests.zip_nets import runpp_zip, with_zip, zip_iterate_norms, zip_residual_inf

ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0)


def create(lib, net, tuning=None, B=64):
    cn, keep = _lib.make_cnetspec(net)
    cc = _lib.make_cconfig(ARGS, 0, tuning)
    h = C.c_void_p()
    rc = lib.mapdn_create(C.byref(cn), C.byref(cc), B, -1, C.byref(h))
    if rc == 0:
        lib.mapdn_destroy(h)
        return rc, ""
    return rc, lib.mapdn_last_error(None).decode()


def zip_substation(cz=(0.0, 30.0, 20.0, 50.0, 50.0), ci=(0.0, 20.0, 40.0, 10.0, 10.0)):
    pnet = substation_net()
    pnet["load"]["const_z_percent"] = list(cz)
    pnet["load"]["const_i_percent"] = list(ci)
    return pnet


def elements(name, seed=0):
    """load / sgen values of one profile row of make_case(name), with random sgen q"""
    _, prof = make_case(name)
    rng = np.random.default_rng(seed)
    row = int(rng.integers(prof.n_rows))
    pv = prof.pv[row]
    return prof.load_p[row], prof.load_q[row], pv, rng.uniform(-0.3, 0.3, pv.shape[0]) * pv


# ---- data layer --------------------------------------------------------------------------------------------------------------
def test_converter_maps_the_percentages_to_fractions_and_refuses_by_default():
    pnet = zip_substation()
    with pytest.raises(NotImplementedError, match="const_z_percent"):
        from_pandapower(pnet)
    with pytest.raises(ValueError, match="zip_loads"):
        from_pandapower(pnet, zip_loads="yes")
    net = from_pandapower(pnet, zip_loads="runpp")
    assert np.array_equal(net.load_const_z, [0.0, 0.3, 0.2, 0.5, 0.5])
    assert np.array_equal(net.load_const_i, [0.0, 0.2, 0.4, 0.1, 0.1])
    assert net.has_zip_loads
    plain = from_pandapower(substation_net(), zip_loads="runpp")        # no ZIP columns: constant power, as before
    assert not plain.has_zip_loads and np.array_equal(plain.load_const_z, np.zeros(plain.n_load))


def test_netspec_validates_the_fractions():
    net, _ = make_case("case33")
    with pytest.raises(ValueError, match="less or equal to 100%"):
        with_zip(net, 0.7, 0.4)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        with_zip(net, -0.1, 0.0)
    with pytest.raises(ValueError, match="one entry per load"):
        dataclasses.replace(net, load_const_z=np.zeros(3))
    assert with_zip(net, 1.0, 0.0).has_zip_loads and not net.has_zip_loads


def test_zip_columns_round_trip_through_netspec_npz(tmp_path):
    net = from_pandapower(zip_substation(), zip_loads="runpp")
    save_netspec(net, str(tmp_path / "netspec.npz"))
    back = load_netspec(str(tmp_path / "netspec.npz"))
    assert np.array_equal(back.load_const_z, net.load_const_z) and np.array_equal(back.load_const_i, net.load_const_i)
    # a file written before the fields existed loads as constant power
    z = dict(np.load(str(tmp_path / "netspec.npz")))
    del z["load_const_z"], z["load_const_i"]
    np.savez_compressed(str(tmp_path / "old.npz"), **z)
    old = load_netspec(str(tmp_path / "old.npz"))
    assert np.array_equal(old.load_const_z, np.zeros(net.n_load)) and not old.has_zip_loads


def test_mapdn_zip_loads_and_the_env_key_reach_the_converter(tmp_path, monkeypatch):
    (tmp_path / "model.p").write_bytes(pickle.dumps({}))
    monkeypatch.setattr(data, "read_pandapower_pickle", lambda path: zip_substation())
    monkeypatch.setattr(data, "load_profiles_csv", lambda *a, **k: "prof")
    monkeypatch.delenv("MAPDN_ZIP_LOADS", raising=False)
    with pytest.raises(NotImplementedError, match="const_z_percent"):
        data.load_scenario(str(tmp_path))
    net, _ = data.load_scenario(str(tmp_path), zip_loads="runpp")
    assert net.has_zip_loads
    monkeypatch.setenv("MAPDN_ZIP_LOADS", "runpp")
    net, _ = data.load_scenario(str(tmp_path))
    assert np.array_equal(net.load_const_i, [0.0, 0.2, 0.4, 0.1, 0.1])
    with pytest.raises(NotImplementedError):
        data.load_scenario(str(tmp_path), zip_loads="refuse")      # the argument wins over the environment
    # the reference class's kwargs: env_args key zip_loads beside hv_init
    from mapdn_amd import env as env_mod
    monkeypatch.delenv("MAPDN_ZIP_LOADS")
    net, _ = env_mod._resolve_data(dict(data_path=str(tmp_path), zip_loads="runpp"))
    assert net.has_zip_loads


def test_converter_refuses_what_it_does_not_cover():
    pnet = zip_substation(cz=(0.0, 30.0, 20.0, 50.0, 40.0))             # two loads of bus 5 with different fractions
    with pytest.raises(NotImplementedError, match="different const_z_percent"):
        from_pandapower(pnet, zip_loads="runpp")
    pnet = substation_net()                                              # a ZIP load on the ext_grid bus
    pnet["load"] = pd.concat([pnet["load"], pd.DataFrame({"name": [None], "bus": [0], "p_mw": [0.5], "q_mvar": [0.1],
                                                          "const_z_percent": [10.0], "const_i_percent": [0.0], "sn_mva": [np.nan],
                                                          "scaling": [1.0], "in_service": [True], "type": ["wye"]})], ignore_index=True)
    with pytest.raises(NotImplementedError, match="ext_grid bus"):
        from_pandapower(pnet, zip_loads="runpp")
    pnet = zip_substation()                                              # ZIP loads with bus fusion
    pnet["switch"] = pd.DataFrame({"bus": [2], "element": [3], "et": ["b"], "type": ["CB"], "closed": [True]})
    with pytest.raises(NotImplementedError, match="fused buses"):
        from_pandapower(pnet, zip_loads="runpp")


def test_mapdn_create_refuses_what_the_solvers_do_not_cover(lib):
    net, _ = make_case("case33")
    z = with_zip(net, 0.3, 0.2)
    assert create(lib, z) == (0, "")
    assert create(lib, with_zip(case33_meshed(net, 5), 0.3, 0.2)) == (0, "")
    rc, msg = create(lib, z, dict(nr_solver="dense"))
    assert rc == -1 and "dense" in msg and "voltage-dependent" in msg
    rc, msg = create(lib, z, dict(overlap_advance=1, fuse_inject=2))
    assert rc == -1 and "overlap_advance" in msg
    lb = net.load_bus.copy()
    lb[1] = lb[2]                                                        # two loads on one bus, only one of them voltage-dependent
    rc, msg = create(lib, dataclasses.replace(z, load_bus=lb, load_const_z=np.where(np.arange(net.n_load) == 1, 0.0, z.load_const_z)))
    assert rc == -1 and "different" in msg, msg
    # on the ext_grid bus
    lb = net.load_bus.copy()
    lb[0] = net.ext_grid_bus
    rc, msg = create(lib, dataclasses.replace(net, load_bus=lb, load_const_z=np.where(np.arange(net.n_load) == 0, 0.5, 0.0)))
    assert rc == -1 and "ext_grid" in msg
    # with fused buses
    alias = np.arange(net.n_bus); alias[5] = 4
    rc, msg = create(lib, dataclasses.replace(z, bus_alias=alias))
    assert rc == -1 and "fused" in msg
    # out of range (bypassing NetSpec's own check): the host validates as well
    bad = with_zip(net, 0.3, 0.2)
    object.__setattr__(bad, "load_const_z", np.full(net.n_load, 0.9))
    rc, msg = create(lib, bad)
    assert rc == -1 and "100%" in msg


def test_the_zip_geometry_is_the_chooser_geometry(lib):
    """the ZIP variants are compiled for the geometries the chooser returns on the three feeder classes"""
    for name in ("case33", "case141", "case322"):
        net, _ = make_case(name)
        for B in (64, 4096):
            g = []
            for n in (net, with_zip(net, 0.3, 0.2)):
                cn, keep = _lib.make_cnetspec(n)
                h = C.c_void_p()
                assert lib.mapdn_create(C.byref(cn), C.byref(_lib.make_cconfig(ARGS, 0, None)), B, -1, C.byref(h)) == 0
                g.append(_lib.nr_geometry(h))
                lib.mapdn_destroy(h)
            assert g[0] == g[1], (name, B)


# ---- the oracle --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("init", ["flat", "dc"])
def test_runpp_zip_at_zero_fractions_is_runpp_restated(init):
    for name in ("case33", "case141"):
        net, _ = make_case(name)
        if init == "dc":
            net = hv_front(net, 0.0)
        ins = elements(name, seed=3)
        a, b = runpp_zip(net, *ins, init=init), runpp_restated(net, *ins, init=init)
        assert np.array_equal(a.V, b.V) and a.iterations == b.iterations and a.converged == b.converged
        for k in ("vm_pu", "va_degree", "p_mw", "q_mvar", "pl_mw"):
            assert np.array_equal(a[k], b[k]), k


def two_bus(z_line=0.01 + 0.02j, s_load=(0.3, 0.1), s_sgen=None, vm0=1.0):
    """slack bus 0 -> one line -> bus 1 with one load (and optionally a sgen); sn = 1 MVA, 1 kV so that the line's ohms are p.u."""
    r, x = z_line.real, z_line.imag
    kw = dict(name="two_bus", bus_vn_kv=np.array([1.0, 1.0]), bus_zone=np.array([0, 1]), line_from_bus=np.array([0]),
              line_to_bus=np.array([1]), line_r_ohm_per_km=np.array([r]), line_x_ohm_per_km=np.array([x]),
              line_c_nf_per_km=np.array([0.0]), line_g_us_per_km=np.array([0.0]), line_length_km=np.array([1.0]),
              line_parallel=np.array([1]), line_in_service=np.array([1]), load_bus=np.array([1]), load_const_z=np.array([1.0]),
              sgen_bus=np.array([1]), sgen_zone=np.array([1]), ext_grid_bus=0, ext_grid_vm_pu=vm0, sn_mva=1.0)
    net = NetSpec(**kw)
    sg = s_sgen or (0.0, 0.0)
    return net, (np.array([s_load[0]]), np.array([s_load[1]]), np.array([sg[0]]), np.array([sg[1]]))


@pytest.mark.parametrize("sgen", [None, (0.12, -0.05)])
def test_constant_z_load_is_the_voltage_divider(sgen):
    """constant-Z: S(|V|) = S0 |V|^2 is the impedance Zl = |V|^2 / conj(S) = 1 / conj(S0), so V2 = V1 Zl / (Zl + Zline).  With a sgen at
    the bus, S0 = S_load - S_sgen: runpp scales the bus's whole net demand (rule 2 of tests/zip_nets.py)"""
    zl_line = 0.01 + 0.02j
    net, ins = two_bus(zl_line, (0.3, 0.1), sgen)
    s0 = complex(ins[0][0] - ins[2][0], ins[1][0] - ins[3][0])
    zload = 1.0 / np.conj(s0)
    v2 = 1.0 * zload / (zload + zl_line)
    r = runpp_zip(net, *ins, tolerance_mva=1e-13)                     # (at the default 1e-8 the iterate is 2e-11 from the fixed point)
    assert r.converged
    assert abs(r.V[1] - v2) < 1e-12, (r.V[1], v2)
    # res_bus: the load at |V|^2, the sgen as it is
    vm = abs(v2)
    assert abs(r.p_mw[1] - (0.3 * vm ** 2 - (sgen[0] if sgen else 0.0))) < 1e-12
    assert abs(r.q_mvar[1] - (0.1 * vm ** 2 - (sgen[1] if sgen else 0.0))) < 1e-12


@pytest.mark.parametrize("name", ["case33", "case141", "case322"])
@pytest.mark.parametrize("cz,ci", [(0.3, 0.2), (1.0, 0.0), (0.0, 1.0)])
def test_runpp_zip_converges_to_the_zip_fixed_point(name, cz, ci):
    net, _ = make_case(name)
    z = with_zip(net, cz, ci)
    ins = elements(name, seed=7)
    r = runpp_zip(z, *ins)
    assert r.converged
    assert zip_residual_inf(z, r.V, *ins) < 1e-8 / net.sn_mva
    c = runpp_restated(net, *ins)                                       # a different answer from constant power
    assert np.abs(r.V - c.V).max() > 1e-6
    norms = zip_iterate_norms(z, *ins)
    assert norms[r.iterations] < 1e-8 / net.sn_mva <= norms[r.iterations - 1]


def test_the_first_mismatch_is_the_constant_power_one():
    """ext_grid_vm_pu != 1: at the flat start |V| = 1.03, so the ZIP Sbus differs from the constant-power one — F0 uses the latter
    (newtonpf evaluates F(x0) with the Sbus makeSbus gave without vm)"""
    net, _ = make_case("case33")
    z = with_zip(dataclasses.replace(net, ext_grid_vm_pu=1.03), 0.5, 0.3)
    ins = elements("case33", seed=11)
    from oracle.pp_restated import _cached_ybus, bus_demand, make_sbus
    ybus = _cached_ybus(z)[0]
    v0 = np.full(z.n_bus, 1.03, dtype=complex)
    sb = make_sbus(z, *bus_demand(z, *ins))
    f0 = v0 * np.conj(ybus @ v0) - sb
    f0 = np.delete(f0, z.ext_grid_bus)
    assert zip_iterate_norms(z, *ins)[0] == max(np.abs(f0.real).max(), np.abs(f0.imag).max())
    r = runpp_zip(z, *ins)
    assert r.converged and zip_residual_inf(z, r.V, *ins) < 1e-8
