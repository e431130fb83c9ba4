"""Pins the [PP-recalled] points of res_line / res_trafo on real pandapower, wherever it is installed: every column
of both tables on a small net with a transformer and an out-of-service line — the out-of-service row, the current and the loading formulas
(trafo_loading="current", df, parallel).  Skipped where pandapower is not importable; the definitions are then only restated
(tests/branch_ref.py)."""
import numpy as np
import pytest

pp = pytest.importorskip("pandapower")

from mapdn_amd.data import from_pandapower           # noqa: E402
from tests import branch_ref as R                    # noqa: E402


def small_net():
    net = pp.create_empty_network(sn_mva=10.0)
    b = [pp.create_bus(net, vn_kv=v, zone=z) for v, z in ((110.0, "main"), (20.0, "main"), (20.0, "zone1"), (20.0, "zone1"), (20.0, "zone2"), (20.0, "zone2"))]
    pp.create_ext_grid(net, b[0], vm_pu=1.02)
    pp.create_transformer_from_parameters(net, b[0], b[1], sn_mva=25.0, vn_hv_kv=110.0, vn_lv_kv=20.0, vk_percent=12.0, vkr_percent=0.41,
                                          pfe_kw=14.0, i0_percent=0.07, shift_degree=0.0, tap_side="hv", tap_neutral=0, tap_min=-9, tap_max=9,
                                          tap_step_percent=1.5, tap_pos=-2, parallel=2, df=0.9)
    for f, t, km, par, mi, df, on in ((1, 2, 2.0, 1, 0.4, 1.0, True), (2, 3, 1.5, 2, 0.21, 0.8, True), (1, 4, 3.0, 1, 0.3, 1.0, True),
                                      (4, 5, 1.0, 1, 0.25, 0.9, True), (3, 5, 1.2, 1, 0.3, 1.0, False)):
        pp.create_line_from_parameters(net, b[f], b[t], length_km=km, r_ohm_per_km=0.25, x_ohm_per_km=0.11, c_nf_per_km=230.0, max_i_ka=mi,
                                       parallel=par, df=df, in_service=on)
    for bus, p, q in ((2, 1.0, 0.3), (3, 0.8, 0.2), (4, 1.2, 0.4), (5, 0.5, 0.1)):
        pp.create_load(net, b[bus], p_mw=p, q_mvar=q)
    pp.create_sgen(net, b[3], p_mw=1.5, q_mvar=0.2, name="zone1")
    pp.create_sgen(net, b[5], p_mw=0.7, q_mvar=-0.1, name="zone2")
    return net


LINE = dict(p_from_mw="p_from_mw", q_from_mvar="q_from_mvar", p_to_mw="p_to_mw", q_to_mvar="q_to_mvar", pl_mw="pl_mw", ql_mvar="ql_mvar",
            i_from_ka="i_from_ka", i_to_ka="i_to_ka", i_ka="i_ka", loading_percent="loading_percent")


def test_every_column_on_a_net_with_a_transformer_and_a_dead_line():
    net = small_net()
    pp.runpp(net, trafo_loading="current")
    spec = from_pandapower(net, hv_init="flat")
    vm, va = net.res_bus.vm_pu.to_numpy(), net.res_bus.va_degree.to_numpy()
    line, trafo = R.tables(spec, vm, va, np.float64)
    for k, col in LINE.items():
        want = net.res_line[col].to_numpy()
        assert np.allclose(line[k], want, rtol=1e-7, atol=1e-9), k
    assert (net.res_line.iloc[4][list(LINE.values())].to_numpy(dtype=float) == 0).all() or np.isnan(net.res_line.iloc[4].loading_percent)
    for k, col in R.TRAFO_NAMES.items():
        assert np.allclose(trafo[k], net.res_trafo[col].to_numpy(), rtol=1e-7, atol=1e-9), col
