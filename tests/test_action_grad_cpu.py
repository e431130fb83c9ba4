"""CPU: action_gradients (mapdn_action_gradients, csrc/grad.hpp) without a GPU —
  1. the reference tests/grad_ref.py against central differences of the oracle's predicted reward (signs, units, scaling, the sgen on the
     slack bus), on rows that keep clear of every kink;
  2. csrc/grad.hpp built for the host (tests/grad_check.cpp): the transposed tree solve against numpy.linalg.solve(J.T, c), the barrier
     derivatives against their longdouble forms (kinks included), the whole gradient in k_action_grad's order against the reference;
  3. a host-only handle refuses what the adjoint tree solve does not cover, by name;
  4. a small step along the gradient raises the oracle's reward by at least half of what the gradient promises."""
import ctypes as C
import dataclasses
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from mapdn_amd import _lib
from mapdn_amd.netspec import add_fused_buses, case33_meshed, make_case
from oracle.env_restated import BARRIER_IDS
from oracle.pp_restated import build_branches, jacobian, make_ybus, runpp_restated
from tests import grad_ref as G
from tests import kernel_matrix as km
from tests import whatif_cases as W
from tests.test_opf_cpu import seven_bus, tree_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 4
# env ids whose solved rows keep clear of the kinks (searched on the CPU with the oracle alone; test_kink_condition asserts it)
CPU_ENVS = dict(tiny=(0, 1, 3), small17=(0, 1, 3), special=(0, 2, 3), crowded=(0, 3, 5), one_sgen=(1, 3, 5), all_pv=(0, 1, 4), case33=(0, 4, 5))
VARIANT_NETS = ("crowded", "special")
VARIANTS = [(("voltage_barrier_type", b),) for b in G.BARRIER_TYPES if b != "bowl"] + [G.LINE_ARGS]
CASES = [(name, ()) for name in G.NETS] + [(name, v) for name in VARIANT_NETS for v in VARIANTS]
CASE_IDS = [name + "".join("-" + str(v) for _, v in args) for name, args in CASES]
V_MARGIN, Q_MARGIN = 1e-4, 1e-6
H = 2e-4
# The worst disagreement between the reference and a central difference of the oracle's predicted reward, relative to the row's |g|inf,
# over every row of CASES at H and at H / 2, measured on the CPU (crowded with the bump barrier; every other case
# stays below 1.6e-7); the bound is ten times that.
CD_MEASURED = 3.604e-7
CD_TOL = 10 * CD_MEASURED
ETA_STEP = 1e-4


def envs_of(name, args):
    return CPU_ENVS[name] if not args else CPU_ENVS[name][:1]


@functools.lru_cache(maxsize=None)
def rows_of(name, args):
    """the solved rows of a case: dicts of the oracle env o, the candidate a, the reference gradient g and the row's prediction p"""
    os_, ref, cand = G.reference(name, envs_of(name, args), K, args)
    assert (ref["solved"] == W.expected_pattern(K)).all(), (name, args)
    out = []
    for e, o in enumerate(os_):
        for k in range(K):
            if ref["solved"][e, k]:
                p = ref["rows"][e][k]
                out.append(dict(o=o, a=cand[e, k], p=p, g=G.reward_gradient(o.net, G.env_args(o), p["r"].V, cand[e, k], G.limits(o))))
    return out


# ---- 1. the reference against central differences ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,args", CASES, ids=CASE_IDS)
def test_kink_condition(name, args):
    """asserted, not skipped: every non-slack solved voltage at least 1e-4 from 0.95, 1.05 and 1.0, every |q_j| at least 1e-6 apart from the
    all-zero candidate"""
    os_, ref, cand = G.reference(name, envs_of(name, args), K, args)
    dv, dq = G.kink_margins(os_, ref, cand)
    assert dv >= V_MARGIN and dq >= Q_MARGIN, (name, dv, dq)
    assert (cand[:, 0] == 0.0).all()


@pytest.mark.parametrize("name,args", CASES, ids=CASE_IDS)
def test_reference_against_central_differences(name, args):
    worst = 0.0
    for r in rows_of(name, args):
        for h in (H, H / 2):                                 # (relative to |g|inf; absolute on an all-zero row)
            worst = max(worst, G.rel_inf(G.central_difference(name, r["o"], r["a"], h), r["g"]))
    print(f"\n[grad cd] {name} {dict(args)}: worst relative disagreement {worst:.3e} (bound {CD_TOL:.1e})")
    assert worst <= CD_TOL, (name, args, worst)


def test_slack_sgen_gets_the_direct_term_alone():
    """special's ninth sgen sits on the ext_grid bus: its entry is -q_weight sign(q) lim scaling / ns, and 0 with line_weight"""
    for args in ((), G.LINE_ARGS):
        for r in rows_of("special", args):
            o, j = r["o"], 8
            assert int(o.net.sgen_bus[j]) == int(o.net.ext_grid_bus)
            lim, s = G.limits(o)[j], o.net.sgen_scaling[j]
            want = 0.0 if args else -o.q_weight / o.net.n_sgen * np.sign(lim * r["a"][j] * s) * lim * s
            assert r["g"][j] == want


# ---- 2. csrc/grad.hpp on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_grad(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("grad")
    exe = str(d / "grad_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "mapdn_amd", "csrc"),
                        os.path.join(ROOT, "tests", "grad_check.cpp"), "-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(rec):
        fi, fo = str(d / "in.bin"), str(d / "out.bin")
        np.ascontiguousarray(rec, dtype=np.float64).tofile(fi)
        p = subprocess.run([exe, fi, fo], capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stderr)
        return np.fromfile(fo, dtype=np.float64)
    return run


def seven_bus_state():
    net = seven_bus()
    lp, lq = np.array([0.8, 0.6, 0.5, 0.7, 0.4]), np.array([0.3, 0.2, 0.2, 0.3, 0.1])
    pv, lim, a = np.array([0.9, 1.1, 0.3]), np.array([0.5, 0.75, 0.4]), np.array([0.4, -0.4, 0.25])
    res = runpp_restated(net, lp, lq, pv, lim * a)
    assert res.converged
    return net, res.V, lim, a


def special_state():
    os_, ref, cand = G.reference("special", CPU_ENVS["special"][:1], K)
    o = os_[0]
    return o.net, ref["rows"][0][1]["r"].V, G.limits(o), cand[0, 1]


STATES = dict(seven_bus=seven_bus_state, special=special_state)


def tables_of(net, V):
    Y = make_ybus(net)[0].toarray()
    slack = int(net.ext_grid_bus)
    bus_of_pos, par, cptr, cidx, yt = tree_tables(Y, slack, net.ext_grid_vm_pu)
    n = net.n_bus - 1
    assert max(cptr[k + 1] - cptr[k] for k in range(n)) == 4              # the four-child junction
    return bus_of_pos, [n, len(cidx)], np.concatenate([par, cptr, cidx, yt.ravel()])


@pytest.mark.parametrize("which", list(STATES))
def test_transposed_tree_solve_against_a_dense_solve(host_grad, which):
    net, V, _, _ = STATES[which]()
    bus_of_pos, dims, tab = tables_of(net, V)
    n = dims[0]
    pq = np.setdiff1d(np.arange(net.n_bus), [net.ext_grid_bus])
    J = jacobian(make_ybus(net)[0], V, pq, pq).toarray()
    c = np.random.default_rng(5).uniform(-1.0, 1.0, 2 * n)               # rows (theta of pq, |V| of pq)
    lam = np.linalg.solve(J.T, c)
    where = {int(b): i for i, b in enumerate(pq)}
    idx = np.array([where[b] for b in bus_of_pos])
    Vp = V[bus_of_pos]
    # the kernel's unknowns are (theta, u = d|V| / |V|): its right-hand side by u is |V| times the one by |V|; lambda is the same vector
    cc = np.stack([c[idx], c[n + idx] * np.abs(Vp)], axis=1)
    got = host_grad(np.concatenate([[0], dims, tab, Vp.real, Vp.imag, cc.ravel()])).reshape(n, 2)
    want = np.stack([lam[idx], lam[n + idx]], axis=1)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"\n[grad host] {which}: transposed solve, relative error {err:.2e}")
    assert err <= 1e-12, err


KINKS = [1.0, 0.95, 1.05, 1.0 - 0.05, 1.0 + 0.05, np.nextafter(0.95, 0), np.nextafter(0.95, 2), np.nextafter(1.05, 0), np.nextafter(1.05, 2),
         np.nextafter(1.0, 0), np.nextafter(1.0, 2)]


@pytest.mark.parametrize("kind", G.BARRIER_TYPES)
def test_barrier_derivatives_against_longdouble(host_grad, kind):
    v = np.concatenate([KINKS, np.linspace(0.85, 1.15, 61), [0.0, 0.5, 2.0, 2.5, 3.0, 3.5, -0.5]])
    got = host_grad(np.concatenate([[1, BARRIER_IDS[kind], v.shape[0]], v]))
    want = G.barrier_derivative(kind, v.astype(G.LD))
    # at the kinks the float64 predicate decides (the longdouble form is given the same float64 v, so both take one branch)
    scale = max(float(np.abs(want).max()), 1.0)
    err = float(np.abs(got.astype(G.LD) - want).max()) / scale
    print(f"\n[grad host] barrier {kind}: error {err:.2e} of {scale:.2e}")
    assert err <= 64 * np.finfo(np.float64).eps, (kind, err)
    k = dict(zip(KINKS, got[:len(KINKS)]))
    if kind == "l1":
        assert k[1.0] == 0.0 and k[np.nextafter(1.0, 0)] == -1.0 and k[np.nextafter(1.0, 2)] == 1.0
    if kind == "bowl":                                       # |v - 1| > 0.05 is the forward form's predicate, in float64
        for x in KINKS:
            assert (abs(k[x]) == 2.0) == (abs(x - 1.0) > 0.05), x
    if kind == "courant_beltrami":
        assert k[0.95] == 0.0 and k[1.05] == 0.0 and k[np.nextafter(0.95, 0)] < 0.0 and k[np.nextafter(1.05, 2)] > 0.0
    if kind == "bump":
        assert k[1.0] == 0.0


def line_records(net, bus_of_pos):
    """plan.hpp LineFlow of every net.line row: fpos, tpos, gff, gtt, gft + gtf, bft - btf"""
    pos = {b: i for i, b in enumerate(bus_of_pos)}
    pos[int(net.ext_grid_bus)] = net.n_bus - 1
    f, t, r, x, bc, tap, is_line = build_branches(net)
    assert net.line_in_service.all()
    ys = 1.0 / (r + 1j * x)
    ytt = ys + 1j * bc / 2
    yff, yft, ytf = ytt / (tap * np.conj(tap)), -ys / np.conj(tap), -ys / tap
    return np.array([[pos[int(f[i])], pos[int(t[i])], yff[i].real, ytt[i].real, yft[i].real + ytf[i].real, yft[i].imag - ytf[i].imag]
                     for i in np.flatnonzero(is_line)])


@pytest.mark.parametrize("args", [(("voltage_barrier_type", b),) for b in G.BARRIER_TYPES] + [G.LINE_ARGS], ids=lambda a: str(a[0][1]))
@pytest.mark.parametrize("which", list(STATES))
def test_host_gradient_against_the_extended_reference(host_grad, which, args):
    """the right-hand side, the two sweeps and the read-out in k_action_grad's order, g++ -O2, against the extended reference at the same
    V: within 16 x the float64 reference's own error and never tighter than 64 ulp of the row's largest entry (the kernel's bar)"""
    net, V, lim, a = STATES[which]()
    a = a.copy()
    a[0] = 0.0                                               # a planted zero: sign(0) = 0
    cfg = dict(voltage_barrier_type="bowl", voltage_weight=1.0, q_weight=0.1, line_weight=None)
    cfg.update(dict(args))
    bus_of_pos, dims, tab = tables_of(net, V)
    n = dims[0]
    Vp = np.concatenate([V[bus_of_pos], [V[net.ext_grid_bus]]])
    pos = {b: i for i, b in enumerate(bus_of_pos)}
    lines = line_records(net, bus_of_pos)
    sg = np.array([[pos.get(int(b), n), lim[j], net.sgen_scaling[j], a[j]] for j, b in enumerate(net.sgen_bus)])
    head = [net.n_bus, int(cfg["line_weight"] is not None), BARRIER_IDS[cfg["voltage_barrier_type"]], cfg["voltage_weight"],
            cfg["q_weight"] or 0.0, cfg["line_weight"] or 0.0, net.sn_mva]
    got = host_grad(np.concatenate([[2], dims, [net.n_sgen, lines.shape[0]], tab, Vp.real, Vp.imag, np.abs(Vp), head, lines.ravel(), sg.ravel()]))
    ext = G.reward_gradient(net, cfg, V, a, lim, ext=True)
    e64 = G.rel_inf(G.reward_gradient(net, cfg, V, a, lim), ext)
    err = G.rel_inf(got, ext)
    bar = max(16 * e64, 64 * np.finfo(np.float64).eps)
    print(f"\n[grad host] {which} {dict(args)}: e64 {e64:.2e} host {err:.2e} bar {bar:.2e}")
    assert err <= bar, (which, args, err, bar)
    slack_sgens = [j for j, b in enumerate(net.sgen_bus) if int(b) == int(net.ext_grid_bus)]
    for j in slack_sgens:                                    # the power-flow part is exactly zero there
        want = 0.0 if cfg["line_weight"] is not None else -cfg["q_weight"] / net.n_sgen * np.sign(lim[j] * a[j] * net.sgen_scaling[j]) * (lim[j] * net.sgen_scaling[j])
        assert got[j] == want, j


# ---- 3. the C ABI on a host-only handle ---------------------------------------------------------------------------------------------------
ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0)


def host_handle(lib, net, tuning=None):
    cn, keep = _lib.make_cnetspec(net)
    cc = _lib.make_cconfig(ARGS, tuning=tuning)
    h = C.c_void_p()
    assert lib.mapdn_create(C.byref(cn), C.byref(cc), 4, -1, C.byref(h)) == 0, lib.mapdn_last_error(None)
    return h, keep


def test_header_and_export_present(lib):
    hdr = open(os.path.join(ROOT, "include", "mapdn.h")).read()
    assert "mapdn_action_gradients(" in hdr and "mapdn_action_gradients" in _lib.EXPORTS and hasattr(lib, "mapdn_action_gradients")
    assert W.global_kernels("grad.hip") == ["k_action_grad"]
    for f in ("grad.hpp", "grad.hip"):
        assert os.path.exists(os.path.join(ROOT, "mapdn_amd", "csrc", f))


@pytest.mark.parametrize("which,word", [("meshed", "meshed"), ("dense", "meshed"), ("zip", "ZIP"), ("gen", "generators"), ("fused", "fused")])
def test_named_refusals_on_host_only_handle(lib, which, word):
    net, _ = make_case("case33")
    tuning = None
    if which == "meshed":
        net = case33_meshed(net, 5)
    elif which == "dense":
        tuning = dict(nr_solver="dense")
    elif which == "zip":
        net = km.make_net("case33_zip")[0]
    elif which == "gen":
        net = dataclasses.replace(net, gen_bus=np.array([3], np.int32), gen_p_mw=np.array([0.1]), gen_vm_pu=np.array([1.0]), gen_scaling=np.array([1.0]))
    else:
        net = add_fused_buses(net, [3, 7])
    h, keep = host_handle(lib, net, tuning=tuning)
    try:
        one = C.c_void_p(1)
        rc = lib.mapdn_action_gradients(h, one, 1, 1, one, one, one, one, None, None, None)
        msg = lib.mapdn_last_error(h).decode()
        assert rc == -1 and msg.startswith("action_gradients:") and word in msg and "not supported" in msg, (which, rc, msg)
    finally:
        lib.mapdn_destroy(h)


def test_argument_refusals_on_host_only_handle(lib):
    net, _ = make_case("case33")
    one = C.c_void_p(1)
    for tuning in (None, dict(nr_init="dc")):                  # the DC start is accepted: the gradient depends on the converged V alone
        h, keep = host_handle(lib, net, tuning=tuning)
        try:
            f64 = 1
            ok = [one, f64, 3, one, one, one, one, None, None, None]
            for i, bad, word in ((0, None, "null buffer"), (3, None, "null buffer"), (4, None, "null buffer"), (5, None, "null buffer"),
                                 (6, None, "null buffer"), (1, 7, "dtype"), (2, 0, "n_candidates"), (2, 1025, "n_candidates")):
                call = list(ok)
                call[i] = bad
                rc = lib.mapdn_action_gradients(h, *call)
                msg = lib.mapdn_last_error(h).decode()
                assert rc == -1 and msg.startswith("action_gradients:") and word in msg, (i, bad, rc, msg)
            assert lib.mapdn_action_gradients(h, *ok) == -4          # MAPDN_E_STATE: a host-only handle launches nothing
        finally:
            lib.mapdn_destroy(h)


# ---- 4. ascent -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,args", CASES, ids=CASE_IDS)
def test_a_step_along_the_gradient_raises_the_reward(name, args):
    """a' = a + eta g with eta = 1e-4 / |g|inf: the oracle's r(a') - r(a) >= eta |g|2^2 / 2 on every solved row.
    The planted zeros: with sign(0) = 0 the gradient leaves the term -q_weight |q_j scaling_j| / ns of an entry with q_j == 0 out, which
    is no derivative of it (the term falls in both directions); for exactly these entries the term's own change, known in closed form, is
    taken out of r(a') - r(a) before the comparison.  Every other entry of every row is held to the inequality as it stands."""
    exempt = planted = 0
    for r in rows_of(name, args):
        o, a, g = r["o"], r["a"], r["g"]
        zero = a == 0.0
        planted += int(zero.all())
        gi = np.abs(g).max()
        if gi == 0.0:
            exempt += 1
            continue
        eta = ETA_STEP / gi
        a2 = a + eta * g
        p2 = W.predict(name, o, a2)
        assert p2["solved"]
        gain = p2["reward"] - r["p"]["reward"]
        if o.line_weight is None and zero.any():
            gain += o.q_weight * np.sum(np.abs(G.limits(o) * a2 * o.net.sgen_scaling)[zero]) / o.net.n_sgen
        assert gain >= 0.5 * eta * float(g @ g), (name, args, gain, eta * float(g @ g))
    assert exempt <= planted


# ---- the E64 constants of the GPU bars ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,args", list(G.E64), ids=[n + "".join("-" + str(v) for _, v in a) for n, a in G.E64])
def test_e64_constants_are_what_the_float64_reference_gives(name, args):
    got = G.e64(name, args)
    print(f"\n[grad e64] {name} {dict(args)}: {got:.2e} (constant {G.E64[(name, args)]:.2e})")
    assert 0.5 * G.E64[(name, args)] <= got <= 2.0 * G.E64[(name, args)], (name, args, got)
