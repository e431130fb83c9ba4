"""CPU (-m "not gpu") tests of the DC-angle start (runpp init="dc", mapdn_env_config.nr_init = 2): the plan's constants against
oracle.pp_restated.dc_angles (mapdn_get_dc_angles on host-only handles), the converter's hv_init="auto", NetSpec.va_init on disk, and
the refusals of mapdn_create."""
import ctypes as C

import numpy as np
import pytest

from mapdn_amd import _lib, data
from mapdn_amd.data import from_pandapower, load_netspec, save_netspec
from mapdn_amd.netspec import case33_meshed, make_case
from oracle.pp_restated import bus_demand, dc_angles
from tests.dc_nets import hv_front
from tests.test_data_ingestion import hv_line_net, substation_net

ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0)


def create(lib, net, tuning=None, B=64):
    cn, keep = _lib.make_cnetspec(net)
    cc = _lib.make_cconfig(ARGS, 0, tuning)
    h = C.c_void_p()
    rc = lib.mapdn_create(C.byref(cn), C.byref(cc), B, -1, C.byref(h))
    return rc, (h if rc == 0 else lib.mapdn_last_error(None).decode())


def host_dc_angles(lib, net, pd_, tuning=None):
    rc, h = create(lib, net, dict(nr_init="dc", **(tuning or {})))
    assert rc == 0, h
    try:
        va = np.zeros(net.n_bus)
        assert lib.mapdn_get_dc_angles(h, _lib._p(np.ascontiguousarray(pd_, np.float64), _lib._pd), _lib._p(va, _lib._pd)) == 0
        return va, _lib.nr_geometry(h)
    finally:
        lib.mapdn_destroy(h)


def random_demand(net, prof, rng):
    row = int(rng.integers(prof.n_rows))
    pl = prof.load_p[row] * rng.uniform(0.5, 1.5, net.n_load)
    ql = prof.load_q[row] * rng.uniform(0.5, 1.5, net.n_load)
    pv = prof.pv[row] * rng.uniform(0.0, 1.5, net.n_sgen)
    return bus_demand(net, pl, ql, pv, rng.uniform(-0.3, 0.3, net.n_sgen) * pv)[0]


def test_dc_angles_of_the_150_degree_hv_net_match_the_oracle(lib):
    pnet = hv_line_net()
    net = from_pandapower(pnet, hv_init="auto")
    pd_ = bus_demand(net, pnet.load["p_mw"].to_numpy(), pnet.load["q_mvar"].to_numpy(), pnet.sgen["p_mw"].to_numpy(),
                     pnet.sgen["q_mvar"].to_numpy())[0]
    ref = dc_angles(net, pd_)
    for solver in ("tree", "sparse"):
        va, g = host_dc_angles(lib, net, pd_, dict(nr_solver=solver))
        assert g["nr_init"] == 2 and g["solver"] == (0 if solver == "tree" else 1)
        assert np.abs(va - ref).max() <= 1e-12, solver
        assert abs(np.degrees(va[1]) + 150.0) < 5.0 and va[net.ext_grid_bus] == 0.0


@pytest.mark.parametrize("case", ["case33", "case141", "case322"])
@pytest.mark.parametrize("hv", [False, True])
def test_dc_angles_of_the_feeders_match_the_oracle(lib, case, hv):
    net, prof = make_case(case)
    if hv:
        net = hv_front(net, 150.0)
    rng = np.random.default_rng(7)
    for _ in range(3):
        pd_ = random_demand(net, prof, rng)
        ref = dc_angles(net, pd_)
        va, g = host_dc_angles(lib, net, pd_)
        assert g["solver"] == 0
        assert np.abs(va - ref).max() <= 1e-12


@pytest.mark.parametrize("hv", [False, True])
def test_dc_angles_of_a_meshed_net_match_the_oracle(lib, hv):
    net0, prof = make_case("case33")
    net = case33_meshed(net0, 5)
    if hv:
        net = hv_front(net, 30.0)
    rng = np.random.default_rng(3)
    for _ in range(3):
        pd_ = random_demand(net, prof, rng)
        va, g = host_dc_angles(lib, net, pd_)
        assert g["solver"] == 1                                  # meshed: the sparse block program
        assert np.abs(va - dc_angles(net, pd_)).max() <= 1e-12


def test_hv_init_auto_records_the_dc_start_exactly_when_runpp_would():
    assert from_pandapower(hv_line_net(), hv_init="auto").va_init == "dc"
    assert from_pandapower(hv_line_net(), hv_init="flat").va_init == "flat"
    assert from_pandapower(substation_net(), hv_init="auto").va_init == "flat"     # no line above 70 kV: runpp starts flat
    assert from_pandapower(substation_net()).va_init == "flat"
    with pytest.raises(ValueError):
        from_pandapower(hv_line_net(), hv_init="dc")


def test_va_init_round_trips_through_netspec_npz(tmp_path):
    net = from_pandapower(hv_line_net(), hv_init="auto")
    save_netspec(net, str(tmp_path / "netspec.npz"))
    assert load_netspec(str(tmp_path / "netspec.npz")).va_init == "dc"
    # a file written before the field existed loads with the flat start
    z = dict(np.load(str(tmp_path / "netspec.npz")))
    del z["va_init"]
    np.savez_compressed(str(tmp_path / "old.npz"), **z)
    assert load_netspec(str(tmp_path / "old.npz")).va_init == "flat"


def test_mapdn_hv_init_auto_reaches_the_converter(tmp_path, monkeypatch):
    import pickle
    (tmp_path / "model.p").write_bytes(pickle.dumps({}))
    seen = []
    monkeypatch.setattr(data, "read_pandapower_pickle", lambda path: "pnet")
    monkeypatch.setattr(data, "from_pandapower", lambda net, hv_init="refuse": seen.append(hv_init) or "spec")
    monkeypatch.setattr(data, "load_profiles_csv", lambda *a, **k: "prof")
    monkeypatch.setenv("MAPDN_HV_INIT", "auto")
    assert data.load_scenario(str(tmp_path)) == ("spec", "prof")
    assert seen == ["auto"]
    # end to end, the real converter on the real HV net
    monkeypatch.undo()
    monkeypatch.setenv("MAPDN_HV_INIT", "auto")
    monkeypatch.setattr(data, "read_pandapower_pickle", lambda path: hv_line_net())
    monkeypatch.setattr(data, "load_profiles_csv", lambda *a, **k: "prof")
    net, _ = data.load_scenario(str(tmp_path))
    assert net.va_init == "dc"


def test_mapdn_create_refuses_what_the_dc_start_does_not_cover(lib):
    net, _ = make_case("case33")
    hv = hv_front(net)
    assert create(lib, hv, dict(nr_init="dc"))[0] == 0
    rc, msg = create(lib, hv, dict(nr_init=1))                   # init="results": still reserved
    assert rc == -1 and "not built" in msg
    rc, msg = create(lib, hv, dict(nr_init=3))
    assert rc == -1 and "nr_init" in msg
    rc, msg = create(lib, hv, dict(nr_init="dc", nr_solver="dense"))
    assert rc == -1 and "dense" in msg and "init" in msg
    from mapdn_amd.netspec import add_fused_buses
    fused = add_fused_buses(hv, [3, 7])
    assert create(lib, fused)[0] == 0                            # the flat start is fine with fused buses ...
    rc, msg = create(lib, fused, dict(nr_init="dc"))             # ... the DC start is refused by name, as the oracle refuses it
    assert rc == -1 and "fused buses" in msg
    with pytest.raises(ValueError):
        _lib.make_cconfig(ARGS, 0, dict(nr_init="results"))


def test_dc_start_geometries_outside_the_list_are_refused(lib):
    net, _ = make_case("case141")
    hv = hv_front(net)
    rc, h = create(lib, hv, dict(nr_init="dc"), B=4096)
    assert rc == 0, h
    g = _lib.nr_geometry(h)
    lib.mapdn_destroy(h)
    assert g["nr_init"] == 2 and (g["waves"], g["lanes"]) in ((1, 16), (2, 16), (4, 16), (4, 8))
    rc, h = create(lib, hv, dict(nr_waves=4, nr_lanes=16, nr_lean=2), B=4096)
    assert rc == 0, h                                            # (compiled for the flat start ...)
    lib.mapdn_destroy(h)
    for pin in (dict(nr_waves=1, nr_lanes=8, nr_lean=2), dict(nr_waves=4, nr_lanes=4, nr_lean=2), dict(nr_waves=1, nr_lanes=32, nr_lean=1)):
        assert create(lib, hv, pin, B=4096)[0] == 0              # ... these pairs exist for the flat start only
        rc, msg = create(lib, hv, dict(nr_init="dc", **pin), B=4096)
        assert rc == -1 and "not compiled in" in msg, (pin, msg)
