"""The pin of tests/zip_nets.py::runpp_zip (voltage-dependent loads, runpp voltage_depend_loads=True): wherever pandapower is installed,
build a small net with ZIP loads — some of them on buses with sgens — run the REAL `pp.runpp` at its defaults and compare voltages,
res_bus and the iteration count.  This is the test that decides rules 2 (the sgens of a ZIP bus are scaled with its loads during the
iteration) and 3 (constant-power F0, no load derivative in the Jacobian) of tests/zip_nets.py.  Skipped where pandapower is absent."""
import numpy as np
import pytest

pp = pytest.importorskip("pandapower")
if not hasattr(pp, "create_empty_network"):      # oracle/pp_stub on sys.path is not pandapower
    pytest.skip("the pandapower on sys.path is the test stub", allow_module_level=True)

from mapdn_amd.data import from_pandapower          # noqa: E402
from mapdn_amd.netspec import make_case             # noqa: E402
from tests.test_pandapower_pin import to_pandapower  # noqa: E402
from tests.zip_nets import runpp_zip, with_zip      # noqa: E402


@pytest.mark.parametrize("cz,ci", [(0.3, 0.2), (1.0, 0.0), (0.0, 1.0)])
def test_runpp_zip_matches_real_pandapower(cz, ci):
    net, prof = make_case("case33")
    sgb = np.unique(net.sgen_bus)
    assert np.isin(sgb, net.load_bus).any()                     # ZIP loads on buses with sgens: rule 2 is exercised
    z = with_zip(net, cz, ci)
    rng = np.random.default_rng(1)
    for _ in range(4):
        row = int(rng.integers(0, prof.n_rows))
        pv = prof.pv[row]
        q = rng.uniform(-0.8, 0.8, net.n_sgen) * np.sqrt(prof.s_max() ** 2 - pv ** 2)
        n = to_pandapower(net, prof.load_p[row], prof.load_q[row], pv, q)
        n.load["const_z_percent"] = z.load_const_z * 100.0
        n.load["const_i_percent"] = z.load_const_i * 100.0
        pp.runpp(n)                                             # all defaults: voltage_depend_loads=True
        r = runpp_zip(z, prof.load_p[row], prof.load_q[row], pv, q)
        rb = n.res_bus.sort_index()
        assert np.abs(rb.vm_pu.to_numpy() - r.vm_pu).max() < 1e-9
        assert np.abs(rb.va_degree.to_numpy() - r.va_degree).max() < 1e-7
        assert np.abs(rb.p_mw.to_numpy() - r.p_mw).max() < 1e-8 and np.abs(rb.q_mvar.to_numpy() - r.q_mvar).max() < 1e-8
        assert int(n._ppc["iterations"]) == r.iterations
        back = from_pandapower(n, zip_loads="runpp")
        assert np.allclose(back.load_const_z, z.load_const_z) and np.allclose(back.load_const_i, z.load_const_i)
