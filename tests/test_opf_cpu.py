"""CPU (-m "not gpu") tests of the OPF baseline: the numpy restatement (tests/opf_ref.py) against finite differences and against the
stored optima (tests/golden/opf_golden.npz, made by tests/golden/make_opf_golden.py), the arithmetic of mapdn_amd/csrc/opf.hpp
compiled for the host (tests/opf_check.cpp) against a dense solve and against the stored QP optima, and the refusals of
mapdn_opf_actions on host-only handles."""
import ctypes as C
import dataclasses
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from mapdn_amd import _lib
from mapdn_amd.baselines import OPFConfig
from mapdn_amd.netspec import NetSpec, add_fused_buses, case33_meshed, make_case
from oracle.pp_restated import jacobian, make_ybus, runpp_restated
from tests import kernel_matrix as km
from tests import opf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "opf_golden.npz"))
CASES = [str(c) for c in GOLDEN["cases"]]
ROWS = [int(r) for r in GOLDEN["rows"]]
V_LOWER, V_UPPER = (float(x) for x in GOLDEN["v_bounds"])
V_TOL = 5e-6


@pytest.fixture(scope="module")
def cases():
    out = {}
    for c in CASES:
        net, prof = make_case(c, days=3)
        out[c] = (net, prof, prof.s_max(1.2))
    return out


@pytest.mark.parametrize("case", CASES)
def test_gradient_against_central_differences(cases, case):
    """opf_ref's g = 2 Re(dV^H M V) against (f(a + h e_j) - f(a - h e_j)) / 2h of the oracle's loss at a random interior a, profile
    row 700.  Observed max error relative to |g|inf, case33 / case141:  h = 1e-1: 9.9e-4 / 5.6e-5,  1e-2: 9.9e-6 / 5.8e-7,
    1e-3: 9.9e-8 / 2.2e-7,  1e-4: 4.0e-8 / 2.6e-6,  1e-5: 3.1e-7 / 2.3e-5.  Truncation (~0.1 h^2) and the round-off of a power flow
    converged to 1e-8 MVA (~2e-10 / h) cross near h = 1e-3, where both are <= 2.2e-7: h = 1e-3, bound 1e-6."""
    net, prof, smax = cases[case]
    lp, lq, pv = prof.load_p[700], prof.load_q[700], prof.pv[700]
    lim = R.limits(pv, smax)
    ybus = make_ybus(net)[0]
    a0 = np.random.default_rng(0).uniform(-0.5, 0.5, net.n_sgen)
    f = lambda a: R.loss_pu(ybus, runpp_restated(net, lp, lq, pv, lim * a).V)
    g = R.linearise(net, runpp_restated(net, lp, lq, pv, lim * a0).V, lim).g
    h, eye = 1e-3, np.eye(net.n_sgen)
    fd = np.array([(f(a0 + h * eye[j]) - f(a0 - h * eye[j])) / (2.0 * h) for j in range(net.n_sgen)])
    err = float(np.abs(fd - g).max() / np.abs(g).max())
    print(case, "relative error", err)
    assert err <= 1e-6, err


@pytest.mark.parametrize("case", CASES)
def test_sensitivity_against_central_differences(cases, case):
    """opf_ref's S = d|V| / da — which the maker's polish, the KKT certificate and the QP all use — against (|V|(a + h e_j) -
    |V|(a - h e_j)) / 2h of the oracle's power flow, same point as above.  Observed max error relative to |S|max, case33 / case141:
    h = 1e-1: 1.2e-4 / 2.8e-6,  1e-2: 1.2e-6 / 2.8e-8,  1e-3: 1.2e-8 / 8.1e-9,  1e-4: 9.8e-10 / 1.2e-7,  1e-5: 8.6e-9 / 1.4e-6.
    Truncation (~1e-2 h^2) and round-off (~1e-11 / h) are both <= 1.3e-8 at h = 1e-3: h = 1e-3, bound 1e-7."""
    net, prof, smax = cases[case]
    lp, lq, pv = prof.load_p[700], prof.load_q[700], prof.pv[700]
    lim = R.limits(pv, smax)
    a0 = np.random.default_rng(0).uniform(-0.5, 0.5, net.n_sgen)
    vm = lambda a: np.abs(runpp_restated(net, lp, lq, pv, lim * a).V)
    S = R.linearise(net, runpp_restated(net, lp, lq, pv, lim * a0).V, lim).S
    h, eye = 1e-3, np.eye(net.n_sgen)
    fd = np.stack([(vm(a0 + h * eye[j]) - vm(a0 - h * eye[j])) / (2.0 * h) for j in range(net.n_sgen)], 1)
    err = float(np.abs(fd - S).max() / np.abs(S).max())
    print(case, "relative error", err)
    assert err <= 1e-7, err


@pytest.mark.parametrize("case", CASES)
def test_sqp_reaches_the_stored_optima(cases, case):
    """the restated SQP from a = 0 on the twelve golden rows: status 0, loss within a relative 1e-8 of the stored optimum, violation
    <= v_tol; and the iterates the GPU tests compare with (stored by the maker) are the ones it produces"""
    net, prof, smax = cases[case]
    for t in ROWS:
        r = R.opf_ref(net, prof.load_p[t], prof.load_q[t], prof.pv[t], smax, None, V_LOWER, V_UPPER)
        gold = float(GOLDEN[f"{case}_{t}_loss_mw"])
        gap = abs(r.loss_mw - gold) / gold
        print(case, t, "iterations", r.iterations, "gap", gap, "violation", r.violation)
        assert r.status == 0, (case, t, r.status)
        assert gap <= 1e-8, (case, t, gap)
        assert r.violation <= V_TOL, (case, t, r.violation)
        assert r.iterations == int(GOLDEN[f"{case}_{t}_ref_iterations"]), (case, t)
        assert np.abs(r.actions - GOLDEN[f"{case}_{t}_ref_a"]).max() <= 1e-9, (case, t)


def test_golden_rows_are_certified_optima():
    for case in CASES:
        for t in ROWS:
            assert float(GOLDEN[f"{case}_{t}_kkt"].max()) < 1e-8, (case, t)
    assert float(np.abs(GOLDEN["case33_100_a"]).max()) < 1.0            # no PV: an interior optimum
    assert any(float(np.abs(GOLDEN[f"case141_{t}_vm_pu"]).max()) > V_UPPER - 1e-7 for t in ROWS)       # active voltage bounds


# ---- csrc/opf.hpp on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_opf(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("opf")
    exe = str(d / "opf_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "mapdn_amd", "csrc"),
                        os.path.join(ROOT, "tests", "opf_check.cpp"), "-o", exe, "-lpthread", "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(rec):
        fi, fo = str(d / "in.bin"), str(d / "out.bin")
        np.ascontiguousarray(rec, dtype=np.float64).tofile(fi)
        p = subprocess.run([exe, fi, fo], capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stderr)
        return np.fromfile(fo, dtype=np.float64)
    return run


def seven_bus():
    """slack 0 -- 1, a junction with the four children 2, 3, 4, 5; 5 -- 6 through a transformer with ratio 0.97 and a 3 degree shift"""
    i32 = np.int32
    return NetSpec(name="seven_bus", bus_vn_kv=np.full(7, 12.66), bus_zone=np.array([0, 1, 1, 1, 2, 2, 2], i32),
                   line_from_bus=np.array([0, 1, 1, 1, 1], i32), line_to_bus=np.array([1, 2, 3, 4, 5], i32),
                   line_r_ohm_per_km=np.array([0.5, 0.9, 1.2, 0.7, 0.8]), line_x_ohm_per_km=np.array([0.4, 0.6, 0.9, 0.5, 0.7]),
                   line_c_nf_per_km=np.array([10.0, 0.0, 20.0, 0.0, 5.0]), line_g_us_per_km=np.zeros(5), line_length_km=np.ones(5),
                   line_parallel=np.ones(5, i32), line_in_service=np.ones(5, np.uint8),
                   load_bus=np.array([2, 3, 4, 5, 6], i32), sgen_bus=np.array([3, 6, 4], i32), sgen_zone=np.array([1, 2, 2], i32),
                   br_from_bus=np.array([5], i32), br_to_bus=np.array([6], i32), br_r_pu=np.array([0.02]), br_x_pu=np.array([0.08]),
                   br_b_pu=np.array([-0.01]), br_ratio=np.array([0.97]), br_shift_deg=np.array([3.0]))


def tree_tables(Y, slack, vroot):
    """what opf_prepare (csrc/baselines_host.hpp) builds from the plan, from a dense Ybus of a radial net: positions (children before parents),
    parent, children in the canonical order (the chain child k - 1 first, then ascending) and the OPF_YT constants per node"""
    nb = Y.shape[0]
    adj = [[m for m in range(nb) if m != k and Y[k, m] != 0] for k in range(nb)]
    parent, order, stack = {}, [], [(w, -1) for w in reversed(adj[slack])]
    while stack:
        u, p = stack.pop()
        parent[u] = p
        order.append(u)
        stack += [(w, u) for w in reversed(adj[u]) if w != p and w != slack]
    bus_of_pos = order[::-1]
    pos = {b: i for i, b in enumerate(bus_of_pos)}
    n = nb - 1
    par = [pos[parent[b]] if parent[b] >= 0 else n for b in bus_of_pos]
    kids = [[] for _ in range(n)]
    for k in range(n):
        if par[k] < n:
            kids[par[k]].append(k)
    for k in range(n):
        if kids[k] and kids[k][-1] == k - 1:
            kids[k] = [k - 1] + kids[k][:-1]
    cptr = np.cumsum([0] + [len(c) for c in kids])
    cidx = [c for cs in kids for c in cs]
    yt = np.zeros((n, 12))
    for k, b in enumerate(bus_of_pos):
        p = parent[b]
        ykp, ypk = (Y[b, p], Y[p, b]) if p >= 0 else (0.0, 0.0)
        mkp = 0.5 * (ykp + np.conj(ypk))
        cks, msv = Y[b, slack] * vroot, 0.5 * (Y[b, slack] + np.conj(Y[slack, b])) * vroot
        yt[k] = [Y[b, b].real, Y[b, b].imag, np.real(ykp), np.imag(ykp), np.real(ypk), np.imag(ypk), cks.real, cks.imag,
                 np.real(mkp), np.imag(mkp), msv.real, msv.imag]
    return bus_of_pos, par, cptr, cidx, yt


def test_tree_elimination_against_a_dense_solve(host_opf):
    net = seven_bus()
    lp, lq = np.array([0.8, 0.6, 0.5, 0.7, 0.4]), np.array([0.3, 0.2, 0.2, 0.3, 0.1])
    pv, q = np.array([0.9, 1.1, 0.3]), np.array([0.2, -0.3, 0.1])
    res = runpp_restated(net, lp, lq, pv, q)
    assert res.converged
    V, ybus = res.V, make_ybus(net)[0]
    Y = ybus.toarray()
    assert abs(Y[5, 6] - Y[6, 5]) > 1e-3                               # the shift makes Ybus unsymmetric
    bus_of_pos, par, cptr, cidx, yt = tree_tables(Y, 0, net.ext_grid_vm_pu)
    n, ns = 6, 3
    assert max(len(cidx[cptr[k]:cptr[k + 1]]) for k in range(n)) == 4  # the junction
    w = np.array([0.7, 1.3, 0.9])
    sg = [bus_of_pos.index(int(b)) for b in net.sgen_bus]
    Vp = V[bus_of_pos]
    rec = np.concatenate([[0, n, ns, len(cidx)], par, cptr, cidx, yt.ravel(), Vp.real, Vp.imag, sg, w])
    x = host_opf(rec).reshape(n, ns, 2)
    pq = np.arange(1, 7)
    J = jacobian(ybus, V, pq, pq).toarray()
    E = np.zeros((2 * n, ns))
    for j, b in enumerate(net.sgen_bus):
        E[n + int(b) - 1, j] = w[j]
    X = np.linalg.solve(J, E)
    rows = np.array(bus_of_pos) - 1
    dth, dvm = X[:n][rows], X[n:][rows]
    got_th, got_vm = x[:, :, 0], x[:, :, 1] * np.abs(Vp)[:, None]
    err = max(np.abs(got_th - dth).max() / np.abs(dth).max(), np.abs(got_vm - dvm).max() / np.abs(dvm).max())
    print("tree elimination: relative error", err)
    assert err <= 1e-12, err


@pytest.mark.parametrize("case", CASES)
def test_qp_routine_against_the_stored_qp_optima(host_opf, case):
    """opf_qp_solve on the stored QP of every golden row against the optimum scipy found for it.  The routine stops at stationarity
    r <= eps |g|inf, violation <= eps, complementarity <= eps |g|inf (eps = 1e-10), and for a convex QP such a point (d, y) has
    q(d) - q(d*) <= |r|inf |d - d*|_1 + |y|_1 (violation of d*) + (rows) x complementarity for every d*: that is the bound, plus the
    rounding of the two objective values themselves (8 ulp of the sum of the magnitudes of their terms)."""
    eps = 1e-10
    for t in ROWS:
        k = f"{case}_{t}_qp_"
        g, H, S, v, a, dstar = (GOLDEN[k + x] for x in ("g", "H", "S", "v", "a", "d"))
        n, ns = S.shape
        out = host_opf(np.concatenate([[1, n, ns, V_LOWER, V_UPPER], g, H.ravel(), S.ravel(), v, a]))
        d, y = out[:ns], out[ns:2 * ns + n]
        newton, capped, kkt, st, vi, co = out[2 * ns + n:]
        gs = np.abs(g).max()
        assert capped == 0 and st <= eps * gs and vi <= eps and co <= eps * gs, (case, t, capped, st / gs, vi, co / gs)
        mag = lambda x: np.abs(g) @ np.abs(x) + 0.5 * np.abs(x) @ (np.abs(H) @ np.abs(x))
        bound = st * np.abs(d - dstar).sum() + np.abs(y).sum() * float(GOLDEN[k + "viol"]) + (n + ns) * co \
            + 8.0 * np.finfo(np.float64).eps * (mag(d) + mag(dstar))
        gap = R.qp_objective(g, H, d) - R.qp_objective(g, H, dstar)
        print(case, t, "newton", int(newton), "objective gap", gap, "bound", bound, "|d - d*|inf", np.abs(d - dstar).max())
        assert gap <= bound, (case, t, gap, bound)
        assert np.all(d >= -1.0 - a - eps) and np.all(d <= 1.0 - a + eps)
        # feasibility of the voltage rows and the stationarity, recomputed here and not taken from the routine (twice its tolerance
        # on the stationarity: numpy sums g + H d + A' y in another order)
        Sd = S @ d
        assert max(float((Sd - (V_UPPER - v)).max()), float(((V_LOWER - v) - Sd).max())) <= eps, (case, t)
        assert float(np.abs(g + H @ d + y[:ns] + S.T @ y[ns:]).max()) <= 2.0 * eps * gs, (case, t)
        sign_ok = (y <= 0) | (np.concatenate([d, Sd]) >= np.concatenate([1.0 - a, V_UPPER - v]) - 1e-6)
        assert sign_ok.all(), (case, t)           # a positive multiplier only at an upper bound
        # shared by a team of lanes, as the kernel's sub-lanes share it (16 as there, and 5: no divisor of anything): the same step
        for lanes in ((16, 5) if t == ROWS[1] else ()):      # (one row with active bounds: host threads at a barrier are slow)
            tout = host_opf(np.concatenate([[2, lanes, n, ns, V_LOWER, V_UPPER], g, H.ravel(), S.ravel(), v, a]))
            assert tout[2 * ns + n + 1] == 0 and np.abs(tout[:ns] - d).max() <= 1e-9, (case, t, lanes, np.abs(tout[:ns] - d).max())
        # and the numpy restatement of the routine finds the same step
        q = R.qp_solve(g, H, S, -1.0 - a, 1.0 - a, V_LOWER - v, V_UPPER - v)
        assert not q.capped and np.abs(q.d - d).max() <= 1e-7, (case, t, np.abs(q.d - d).max())


def test_update_decision_replays_the_restated_loop(host_opf, cases):
    """opf_decide / k_opf_update's branches, failed power flows included.  Honest inputs that reach the retry and status 2 on the GPU
    exist only near voltage collapse (found by the search of tests/golden/make_opf_backtrack.py and run by
    tests/test_opf_kernels_gpu.py); the other failure paths (at the first solve, at max_iter, after several retries) are replayed here: the
    restated loop runs with a power flow that is made to fail at chosen calls, records what it saw before every decision, and opf_decide, replayed
    on those records, takes the same path (retry with half the step, at most max_backtrack times in a row; status 2 at the first
    solve, after too many failures and at max_iter; status 1 at max_iter) and ends where the loop ends."""
    net, prof, smax = cases["case33"]
    lp, lq, pv = prof.load_p[260], prof.load_q[260], prof.pv[260]
    plans = [(set(), None), ({1}, None), ({3}, None), ({3, 4, 5}, None), ({3, 4, 5}, dict(max_backtrack=2)), ({4}, dict(max_iter=4)),
             (set(), dict(max_iter=3)), (set(range(2, 60)), None), (set(), dict(v_lower=0.999, v_upper=1.001))]
    seen = set()
    for fail, cfg in plans:
        calls = []

        def runpp(*a, **k):
            calls.append(1)
            r = runpp_restated(*a, **k)
            return types.SimpleNamespace(converged=False) if len(calls) in fail else r
        log = []
        ref = R.opf_ref(net, lp, lq, pv, smax, cfg, V_LOWER, V_UPPER, runpp=runpp, decisions=log)
        c = R.resolve(cfg, V_LOWER, V_UPPER)
        rec = [3, c["step_tol"], c["v_tol"], c["max_iter"], c["max_backtrack"]]
        nback, t, status, a_trace = 0, 1.0, 255, []
        for i, d in enumerate(log):
            rec += [d["iter"], d["solved"], nback, t, d["dn"], d["viol"], d["prev_viol"], d["capped"]]
            run, st, nback, t = host_opf(np.array(rec[:5] + rec[-8:], dtype=np.float64))
            assert t == d["t_after"] and int(nback) == d["nback_after"], (fail, cfg, i)
            assert (int(run) in (2, 3)) == (i == len(log) - 1), (fail, cfg, i, run)
            seen.add((int(run), int(st)))
            status = int(st)
        assert status == ref.status and len(log) == ref.iterations, (fail, cfg, status, ref.status)
    assert seen >= {(1, 255), (4, 255), (2, 0), (2, 1), (3, 2)}, seen


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0)
BAD = [dict(v_lower=1.06), dict(v_upper=0.9), dict(v_lower=-0.5), dict(v_tol=-1e-6), dict(step_tol=-1.0), dict(max_iter=-1),
       dict(max_iter=1001), dict(max_backtrack=-2), dict(max_backtrack=61)]


def host_handle(lib, net, args=ARGS, tuning=None):
    cn, keep = _lib.make_cnetspec(net)
    cc = _lib.make_cconfig(args, tuning=tuning)
    h = C.c_void_p()
    assert lib.mapdn_create(C.byref(cn), C.byref(cc), 4, -1, C.byref(h)) == 0, lib.mapdn_last_error(None)
    return h, keep


def test_header_and_export_present(lib):
    hdr = open(os.path.join(ROOT, "include", "mapdn.h")).read()
    assert "mapdn_opf_actions(" in hdr and "typedef struct mapdn_opf_config" in hdr
    assert "mapdn_opf_actions" in _lib.EXPORTS and hasattr(lib, "mapdn_opf_actions")
    assert "mapdn_opf_probe(" in hdr and "mapdn_opf_probe" in _lib.EXPORTS and hasattr(lib, "mapdn_opf_probe")
    assert os.path.exists(os.path.join(ROOT, "mapdn_amd", "csrc", "opf.hpp")) and os.path.exists(os.path.join(ROOT, "mapdn_amd", "csrc", "opf.hip"))


def test_config_refusals_on_host_only_handle(lib):
    net, _ = make_case("case33")
    h, keep = host_handle(lib, net)
    try:
        for bad in BAD:
            oc = _lib.make_opf_config(bad)
            rc = lib.mapdn_opf_actions(h, C.byref(oc), None, None, None, None, None, None, None)
            assert rc == -1, bad                                          # MAPDN_E_INVALID
            assert lib.mapdn_last_error(h).decode().startswith("opf:"), bad
        for ok in (None, dict(v_lower=0.94, v_upper=1.06, v_tol=1e-5, step_tol=1e-5, max_iter=1000, max_backtrack=60)):
            oc = _lib.make_opf_config(ok)
            rc = lib.mapdn_opf_actions(h, C.byref(oc), None, None, None, None, None, None, None)
            assert rc == -1 and "null buffer" in lib.mapdn_last_error(h).decode()
            one = C.c_void_p(1)
            assert lib.mapdn_opf_actions(h, C.byref(oc), one, None, None, None, one, one, None) == -4      # MAPDN_E_STATE: host-only
        assert lib.mapdn_opf_actions(h, None, None, None, None, None, None, None, None) == -1               # NULL config = the defaults
        assert "null buffer" in lib.mapdn_last_error(h).decode()
    finally:
        lib.mapdn_destroy(h)


def probe(lib, h, cfg, a, ns):
    """mapdn_opf_probe with no output asked for"""
    return lib.mapdn_opf_probe(h, C.byref(cfg) if cfg is not None else None, a, ns, *([None] * 13))


def test_probe_refusals_on_host_only_handle(lib):
    """mapdn_opf_probe refuses what mapdn_opf_actions refuses, with the same words, then a NULL a and a wrong ns by name, and only then
    notices that the handle has no device: nothing was launched"""
    net, _ = make_case("case33")
    h, keep = host_handle(lib, net)
    one = C.c_void_p(1)
    try:
        for bad in BAD:
            assert probe(lib, h, _lib.make_opf_config(bad), one, net.n_sgen) == -1, bad
            assert lib.mapdn_last_error(h).decode().startswith("opf:"), bad
        for ok in (None, _lib.make_opf_config(dict(v_lower=0.94, v_upper=1.06, max_iter=1000, max_backtrack=60))):
            assert probe(lib, h, ok, None, net.n_sgen) == -1 and "opf_probe: a is NULL" in lib.mapdn_last_error(h).decode()
            for ns in (0, -1, net.n_sgen - 1, net.n_sgen + 1, 65):
                assert probe(lib, h, ok, one, ns) == -1 and "opf_probe: ns" in lib.mapdn_last_error(h).decode(), ns
            assert probe(lib, h, ok, one, net.n_sgen) == -4                # MAPDN_E_STATE: host-only
        assert lib.mapdn_opf_probe(None, None, one, net.n_sgen, *([None] * 13)) == -1
    finally:
        lib.mapdn_destroy(h)


@pytest.mark.parametrize("which,word", [("meshed", "meshed"), ("zip", "ZIP"), ("fused", "fused"), ("sgens", "64 sgens")])
def test_probe_named_refusals_on_host_only_handle(lib, which, word):
    net, _ = make_case("case33")
    if which == "meshed":
        net = case33_meshed(net, 5)
    elif which == "zip":
        net = km.make_net("case33_zip")[0]
    elif which == "fused":
        net = add_fused_buses(net, [3, 7])
    else:
        net = _many_sgens(make_case("case322")[0])
    h, keep = host_handle(lib, net)
    try:
        rc = probe(lib, h, None, C.c_void_p(1), net.n_sgen)
        msg = lib.mapdn_last_error(h).decode()
        assert rc == -1 and msg.startswith("opf:") and word in msg, (which, rc, msg)
    finally:
        lib.mapdn_destroy(h)


# ---- the nets and the bars of tests/test_opf_kernels_gpu.py ------------------------------------------------------------------------------
def test_special_net_carries_what_it_claims(lib):
    """the special net of the kernel matrix: an unsymmetric Ybus (the phase shifter), iron losses, a shunt, sgen scalings, an sgen on the
    slack bus, and in the handle's elimination order a junction with four children whose chain child k - 1 is not its lowest-numbered
    one; and on it the restated g, which the GPU test holds the kernel's to, against central differences of the oracle's loss.
    Observed max error relative to |g|inf at envs 0 / 2 / 16:  h = 1e-2: 1.1e-5 / 2.1e-6 / 2.0e-6,  1e-3: 1.1e-7 / 2.8e-8 / 4.7e-8,
    1e-4: 3.8e-7 / 1.7e-7 / 1.3e-7: truncation (~0.1 h^2) and round-off cross near h = 1e-3, as in
    test_gradient_against_central_differences, whose h = 1e-3 and bound 1e-6 serve here too."""
    from tests import opf_kernel_cases as K
    net, prof, rows, a, smax = K.state("special")
    Y = make_ybus(net)[0].toarray()
    assert np.abs(Y - Y.T).max() > 1e-3 * np.abs(Y).max() and net.br_shift_deg[0] == 3.0 and net.br_g_pu[0] != 0
    assert net.shunt_bus.shape[0] == 1 and (net.sgen_scaling != 1).all() and net.sgen_bus[-1] == net.ext_grid_bus
    assert 0 not in (int(net.br_from_bus[0]), int(net.br_to_bus[0]))       # an inner branch
    h, keep = host_handle(lib, net)
    try:
        n = net.n_bus - 1
        nr, sched, par = C.c_int32(), np.zeros(4 * n + 8, np.int32), np.zeros(n + 1, np.int32)
        assert lib.mapdn_get_schedule(h, 1, C.byref(nr), _lib._p(sched, _lib._pi), _lib._p(par, _lib._pi)) == 0
        fac, bop = np.zeros(n * 12), np.zeros(n + 1, np.int32)
        assert lib.mapdn_get_flat_factors(h, _lib._p(fac, _lib._pd), _lib._p(bop, _lib._pi)) == 0
    finally:
        lib.mapdn_destroy(h)
    kids = [[c for c in range(n) if par[c] == k] for k in range(n)]
    four = [k for k in range(n) if len(kids[k]) == 4]
    assert four and all(k - 1 in kids[k] and min(kids[k]) < k - 1 for k in four), kids
    assert int(bop[four[0]]) == K.special_hub()
    ybus = make_ybus(net)[0]
    eye = np.eye(net.n_sgen)
    for e in (0, 2, 16):
        t = rows[e]
        lim = R.limits(prof.pv[t], smax)
        f = lambda x: R.loss_pu(ybus, runpp_restated(net, prof.load_p[t], prof.load_q[t], prof.pv[t], lim * x).V)
        g = R.linearise(net, runpp_restated(net, prof.load_p[t], prof.load_q[t], prof.pv[t], lim * a[e]).V, lim).g
        for hh in (1e-2, 1e-3, 1e-4):
            fd = np.array([(f(a[e] + hh * eye[j]) - f(a[e] - hh * eye[j])) / (2.0 * hh) for j in range(net.n_sgen)])
            err = float(np.abs(fd - g).max() / np.abs(g).max())
            print("special env", e, "h", hh, "relative error", err)
            assert hh != 1e-3 or err <= 1e-6, (e, err)
        assert g[-1] == 0 and fd[-1] == 0                                 # the slack sgen moves nothing


def _kernel_cases():
    from tests import opf_kernel_cases as K
    return list(K.BATCHES)


@pytest.mark.parametrize("case", _kernel_cases())
def test_e64_constants_are_what_the_float64_reference_gives(case):
    """tests/test_opf_kernels_gpu.py holds k_opf_linearise to 16 x E64, E64 the error of opf_ref.linearise against the extended-precision
    reference.  Recomputed here: every constant within a factor 2 either way (another LAPACK rounds otherwise), so that none is inflated."""
    from tests import opf_kernel_cases as K
    now = K.e64(case)
    print(case, {q: f"{v:.2e}" for q, v in now.items()})
    for q in K.QUANTITIES:
        assert 0.5 * K.E64[case][q] <= now[q] <= 2.0 * K.E64[case][q], (case, q, now[q], K.E64[case][q])


# the error of the host build of opf.hpp (opf_check mode 4: its elimination and k_opf_linearise's sums in the kernel's order, float64,
# g++ -O2, no fused multiply-add) against the extended-precision reference at the oracle's V of the reference envs, per case and
# quantity, as measured when the test was written: what the arithmetic of the kernel is good for on each net, apart from the GPU
HOST_ERR = dict(
    tiny=dict(S=1.2e-14, g=2.8e-14, H=1.0e-14, loss=2.2e-13),
    small15=dict(S=6.6e-15, g=2.2e-13, H=9.7e-15, loss=7.9e-13),
    small16=dict(S=2.4e-14, g=4.3e-13, H=1.6e-14, loss=1.1e-12),
    small17=dict(S=1.6e-14, g=1.1e-12, H=1.9e-14, loss=6.7e-13),
    wide33=dict(S=9.3e-14, g=6.1e-13, H=7.4e-14, loss=4.1e-12),
    wide48=dict(S=4.9e-14, g=1.6e-13, H=4.2e-14, loss=1.3e-12),
    wide49=dict(S=3.6e-14, g=5.1e-13, H=3.1e-14, loss=3.7e-12),
    wide64=dict(S=1.2e-13, g=4.0e-12, H=1.2e-13, loss=4.2e-12),
    case33=dict(S=2.6e-14, g=4.6e-13, H=2.3e-14, loss=3.6e-12),
    case141=dict(S=2.6e-13, g=2.7e-12, H=2.2e-13, loss=6.7e-12),
    special=dict(S=2.0e-14, g=8.4e-13, H=3.8e-14, loss=4.2e-12),
)


@pytest.mark.parametrize("case", _kernel_cases())
def test_host_build_of_the_linearisation_meets_the_kernel_bars(host_opf, case):
    """the kernel's arithmetic on the host against the extended-precision reference, under the bar the GPU test sets the kernel"""
    from tests import opf_kernel_cases as K
    net, prof, rows, a, smax = K.state(case)
    ybus = make_ybus(net)[0]
    Y = ybus.toarray()
    slack, vroot = int(net.ext_grid_bus), net.ext_grid_vm_pu
    bus_of_pos, par, cptr, cidx, yt = tree_tables(Y, slack, vroot)
    n, ns = net.n_bus - 1, net.n_sgen
    pos = {b: i for i, b in enumerate(bus_of_pos)}
    sg = [pos.get(int(b), n) for b in net.sgen_bus]                      # (n: an sgen on the slack bus)
    per_env = []
    for e in K.ref_envs(len(rows)):
        t = rows[e]
        lim = R.limits(prof.pv[t], smax)
        res = runpp_restated(net, prof.load_p[t], prof.load_q[t], prof.pv[t], lim * a[e])
        assert res.converged
        Vp = res.V[bus_of_pos]
        w = lim * net.sgen_scaling / net.sn_mva
        out = host_opf(np.concatenate([[4, n, ns, len(cidx)], par, cptr, cidx, yt.ravel(), Vp.real, Vp.imag, sg, w, np.abs(Vp),
                                       [Y[slack, slack].real * vroot * vroot]]))
        S = np.zeros((net.n_bus, ns))
        S[bus_of_pos] = out[:n * ns].reshape(n, ns)
        got = dict(S=S, g=out[n * ns:n * ns + ns], H=out[n * ns + ns:-1].reshape(ns, ns), loss=out[-1],
                   violation=R.violation_of(np.abs(res.V), net, *K.V_BAND))
        per_env.append(K.errors(net, res.V, lim, got))
    worst = K.worst(per_env)
    print(f"    {case}=dict(" + ", ".join(f"{q}={v:.1e}" for q, v in worst.items() if q != "violation") + "),")
    for q in ("S", "g", "H", "loss"):
        assert worst[q] <= K.bar(case, q), (case, q, worst[q], K.bar(case, q))


def _many_sgens(net, ns=65):
    reps = -(-ns // net.n_sgen)
    return dataclasses.replace(net, name=net.name + "_65", sgen_bus=np.tile(net.sgen_bus, reps)[:ns], sgen_zone=np.tile(net.sgen_zone, reps)[:ns],
                               sgen_scaling=np.ones(ns))


@pytest.mark.parametrize("which,word", [("meshed", "meshed"), ("dense", "meshed"), ("zip", "ZIP"), ("fused", "fused"), ("sgens", "64 sgens")])
def test_named_refusals_on_host_only_handle(lib, which, word):
    net, _ = make_case("case33")
    tuning = None
    if which == "meshed":
        net = case33_meshed(net, 5)
    elif which == "dense":
        tuning = dict(nr_solver="dense")                                  # a radial net pinned to the dense solver
    elif which == "zip":
        net = km.make_net("case33_zip")[0]
    elif which == "fused":
        net = add_fused_buses(net, [3, 7])
    else:
        net = _many_sgens(make_case("case322")[0])
    h, keep = host_handle(lib, net, tuning=tuning)
    try:
        one = C.c_void_p(1)
        rc = lib.mapdn_opf_actions(h, None, one, None, None, None, one, one, None)
        msg = lib.mapdn_last_error(h).decode()
        assert rc == -1 and msg.startswith("opf:") and word in msg, (which, rc, msg)
    finally:
        lib.mapdn_destroy(h)


def test_make_opf_config():
    with pytest.raises(KeyError):
        _lib.make_opf_config(dict(v_tolerance=1e-3))
    c = _lib.make_opf_config(OPFConfig(max_iter=7))
    assert c.max_iter == 7 and c.v_lower == 0.0 and c.v_tol == 5e-6 and c.max_backtrack == 8
    assert R.resolve(OPFConfig(), 0.95, 1.05)["v_lower"] == 0.95
