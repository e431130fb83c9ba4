"""The pin of tests/gen_nets.py::runpp_gen (generators, net.gen): wherever pandapower is installed, build nets with gen rows, run the REAL
`pp.runpp` at its defaults and compare voltages, res_bus, res_gen and the iteration count.  This is the test that decides the rules of
tests/gen_nets.py: P = p_mw * scaling, Q free and unlimited (enforce_q_lims=False), the start of the PQ buses at the mean vm_pu of the
ext_grid and of every gen row — an out-of-service row included —, and what pandapower does in the cases the converter refuses.  Skipped
where pandapower is absent."""
import numpy as np
import pytest

pp = pytest.importorskip("pandapower")
if not hasattr(pp, "create_empty_network"):      # oracle/pp_stub on sys.path is not pandapower
    pytest.skip("the pandapower on sys.path is the test stub", allow_module_level=True)

from mapdn_amd.data import from_pandapower          # noqa: E402
from mapdn_amd.netspec import make_case             # noqa: E402
from tests.gen_nets import GENS, runpp_gen, with_gens  # noqa: E402
from tests.test_pandapower_pin import to_pandapower  # noqa: E402


def pp_net(net, x, gens, out_of_service=()):
    n = to_pandapower(net, *x)
    for b, p, vm in gens:
        pp.create_gen(n, int(b), p_mw=p, vm_pu=vm, min_q_mvar=-0.01, max_q_mvar=0.01)     # limits that would bind if they were read
    for b, p, vm in out_of_service:
        pp.create_gen(n, int(b), p_mw=p, vm_pu=vm, in_service=False)
    return n


def element_values(net, prof, rng):
    row = int(rng.integers(0, prof.n_rows))
    pv = prof.pv[row]
    return prof.load_p[row], prof.load_q[row], pv, rng.uniform(-0.8, 0.8, net.n_sgen) * np.sqrt(prof.s_max() ** 2 - pv ** 2)


@pytest.mark.parametrize("name", ["leaf", "mixed", "chain"])
def test_runpp_gen_matches_real_pandapower(name):
    net, prof = make_case("case33")
    rng = np.random.default_rng(1)
    for _ in range(3):
        x = element_values(net, prof, rng)
        n = pp_net(net, x, GENS[name])
        pp.runpp(n)
        back = from_pandapower(n, gens="runpp")
        assert np.array_equal(back.gen_bus, [b for b, _, _ in GENS[name]]) and back.vm_init_pu == with_gens(net, GENS[name]).start_vm_pu
        r = runpp_gen(back, *x)
        rb, rg = n.res_bus.sort_index(), n.res_gen.sort_index()
        assert np.abs(rb.vm_pu.to_numpy() - r.vm_pu).max() < 1e-9
        assert np.abs(rb.va_degree.to_numpy() - r.va_degree).max() < 1e-7
        assert np.abs(rb.p_mw.to_numpy() - r.p_mw).max() < 1e-8 and np.abs(rb.q_mvar.to_numpy() - r.q_mvar).max() < 1e-8
        for k in ("p_mw", "q_mvar", "vm_pu", "va_degree"):
            assert np.abs(rg[k].to_numpy() - r.res_gen[k]).max() < 1e-7, k
        assert int(n._ppc["iterations"]) == r.iterations


def test_runpp_gen_matches_real_pandapower_on_the_substation_net():
    """the 110/20 kV substation feeder of tests/test_pandapower_pin.py (transformer, shunt, scaled and out-of-service elements, sn_mva 10)
    with the gen rows of tests/gen_nets.py::gen_substation — one in service (scaling 0.9), one not: voltages, iterations, res_bus and
    res_gen of the real runpp against runpp_gen on the converted net"""
    n = pp.create_empty_network(sn_mva=10.0)
    hv = pp.create_bus(n, vn_kv=110.0, zone="main")
    b = [pp.create_bus(n, vn_kv=20.0, zone=z) for z in ("main", "zone1", "zone1", "zone2", "zone2")]
    pp.create_transformer_from_parameters(n, hv, b[0], sn_mva=25.0, vn_hv_kv=110.0, vn_lv_kv=20.0, vk_percent=12.0, vkr_percent=0.41,
                                          pfe_kw=14.0, i0_percent=0.07, shift_degree=150.0, tap_side="hv", tap_neutral=0, tap_min=-9,
                                          tap_max=9, tap_step_percent=1.5, tap_pos=-2)
    for f, t, l, r, x, c in ((0, 1, 2.0, 0.2, 0.12, 250.0), (1, 2, 1.5, 0.3, 0.1, 200.0), (0, 3, 3.0, 0.25, 0.11, 240.0), (3, 4, 1.0, 0.4, 0.1, 210.0)):
        pp.create_line_from_parameters(n, b[f], b[t], length_km=l, r_ohm_per_km=r, x_ohm_per_km=x, c_nf_per_km=c, max_i_ka=0.4)
    for bus, p, q, sc, on in ((1, 1.0, 0.3, 1.0, True), (2, 0.8, 0.2, 1.0, True), (3, 1.2, 0.4, 0.9, True), (4, 0.5, 0.1, 1.0, True), (4, 0.3, 0.1, 1.0, False)):
        pp.create_load(n, b[bus], p_mw=p, q_mvar=q, scaling=sc, in_service=on)
    pp.create_sgen(n, b[2], p_mw=1.5, q_mvar=0.2, name="zone1")
    pp.create_sgen(n, b[4], p_mw=0.7, q_mvar=-0.1, name="zone2", scaling=0.5)
    pp.create_shunt(n, b[3], q_mvar=-0.25, p_mw=0.0, step=2, max_step=3)
    pp.create_ext_grid(n, hv, vm_pu=1.02)
    pp.create_gen(n, b[1], p_mw=0.6, vm_pu=1.01, scaling=0.9, min_q_mvar=-0.1, max_q_mvar=0.1)
    pp.create_gen(n, b[3], p_mw=0.3, vm_pu=1.05, in_service=False)
    pp.runpp(n)
    net = from_pandapower(n, gens="runpp")
    assert net.n_gen == 1 and net.vm_init_pu == np.mean([1.02, 1.01, 1.05])
    r = runpp_gen(net, n.load.p_mw.to_numpy(), n.load.q_mvar.to_numpy(), n.sgen.p_mw.to_numpy(), n.sgen.q_mvar.to_numpy())
    rb = n.res_bus.sort_index()
    rg = n.res_gen.sort_index()[n.gen.sort_index().in_service.to_numpy(bool)]
    assert np.abs(rb.vm_pu.to_numpy() - r.vm_pu).max() < 1e-9
    assert np.abs(rb.p_mw.to_numpy() - r.p_mw).max() < 1e-8 and np.abs(rb.q_mvar.to_numpy() - r.q_mvar).max() < 1e-8
    for k in ("p_mw", "q_mvar", "vm_pu", "va_degree"):
        assert np.abs(rg[k].to_numpy() - r.res_gen[k]).max() < 1e-7, k
    assert int(n._ppc["iterations"]) == r.iterations


def test_an_out_of_service_gen_row_moves_the_start():
    """the iteration count decides it: with a far-off vm_pu on an out-of-service row the PQ buses start elsewhere"""
    net, prof = make_case("case33")
    x = element_values(net, prof, np.random.default_rng(2))
    n = pp_net(net, x, GENS["leaf"], out_of_service=[(10, 0.1, 1.3)])
    pp.runpp(n)
    back = from_pandapower(n, gens="runpp")
    assert back.n_gen == 1 and back.vm_init_pu == np.mean([1.0, 1.0, 1.3])
    r = runpp_gen(back, *x)
    assert int(n._ppc["iterations"]) == r.iterations
    assert np.abs(n.res_bus.sort_index().vm_pu.to_numpy() - r.vm_pu).max() < 1e-9


def test_what_pandapower_does_in_the_refused_cases():
    """two gens on one bus: one voltage-controlled bus whose Q pandapower splits between them; a gen on the ext_grid bus: the slack keeps
    its set-point — neither is what one gen bus per row would compute, which is why the converter refuses them"""
    net, prof = make_case("case33")
    x = element_values(net, prof, np.random.default_rng(3))
    n = pp_net(net, x, [(32, 0.2, 1.0), (32, 0.1, 1.0)])
    pp.runpp(n)
    assert abs(n.res_bus.vm_pu[32] - 1.0) < 1e-9 and len(n.res_gen) == 2
    with pytest.raises(NotImplementedError, match="two in-service gens on one bus"):
        from_pandapower(n, gens="runpp")
    n = pp_net(net, x, [(int(net.ext_grid_bus), 0.2, 1.02)])
    pp.runpp(n)
    with pytest.raises(NotImplementedError, match="ext_grid bus"):
        from_pandapower(n, gens="runpp")
