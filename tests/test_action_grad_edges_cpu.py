"""CPU: action_gradients at the edges of its frame (csrc/grad.hpp) without a GPU, on the hand-built nets of
tests/grad_edge_nets.py — one node, a 40-bus chain, a star, three feeders off the slack bus, a comb, out-of-service / parallel / charged
net.line rows, and the shipped case141:
  1. every net holds the edge it was built for, a host-only handle takes it and action_gradients does not refuse it;
  2. the conditions of the scenario, asserted on the oracle alone: the pattern solved, solved, unsolvable, solved on every env the GPU
     tests use, limits strictly between 0 and s_max, the kink margins of tests/test_action_grad_cpu.py on the rows the CPU tests use, and
     on chain40 and case141 a voltage outside [0.95, 1.05];
  3. the reference against central differences of the oracle on pair, chain40 and ties;
  4. the out-of-service rows of `ties` add nothing to the right-hand side and count in the mean;
  5. csrc/grad.hpp built for the host (tests/grad_check.cpp) on every net against the extended reference, at the kernel's bar, so that a
     GPU failure can be told apart as arithmetic or device;
  6. the E64 constants of the new cases."""
import ctypes as C

import numpy as np
import pytest

from mapdn_amd import _lib
from oracle.env_restated import BARRIER_IDS
from oracle.pp_restated import build_branches, make_ybus
from tests import grad_edge_nets as EN
from tests import grad_ref as G
from tests import whatif_cases as W
from tests.test_action_grad_cpu import H, Q_MARGIN, V_MARGIN, host_grad, host_handle  # noqa: F401  (host_grad: the fixture)
from tests.test_opf_cpu import tree_tables

K = EN.K_MAX
# env ids whose solved rows keep clear of the kinks (searched on the CPU with the oracle alone; test_scenario_conditions asserts it); on
# chain40 and case141 they include rows with a voltage outside the band
CPU_ENVS = dict(pair=(0, 3, 6), chain40=(6, 8, 16), star12=(0, 1, 3), feeders3=(1, 6, 7), comb10=(0, 1, 16), ties=(1, 3, 28), case141=(1, 2, 11))
LINE_NETS = ("ties", "feeders3")
CASES = [(name, ()) for name in EN.NETS] + [(name, G.LINE_ARGS) for name in LINE_NETS]
CASE_IDS = [name + "".join("-" + str(v) for _, v in args) for name, args in CASES]
CD_CASES = [("pair", ()), ("chain40", ()), ("ties", ()), ("ties", G.LINE_ARGS)]
# The worst disagreement between the reference and a central difference of the oracle's predicted reward, relative to the row's |g|inf,
# over every row of CD_CASES at H = 2e-4 and at H / 2, measured on the CPU (pair; chain40 1.03e-8, ties 2.2e-9, ties with line_weight
# 1.18e-8); the bound is ten times that, the factor of tests/test_action_grad_cpu.py.
CD_MEASURED = 2.369e-8
CD_TOL = 10 * CD_MEASURED
ULP = np.finfo(np.float64).eps


def rows_of(name, args):
    """the solved rows of the CPU envs of a case: (oracle env, candidate, prediction)"""
    os_, ref, cand = G.reference(name, CPU_ENVS[name], K, args)
    assert (ref["solved"] == W.expected_pattern(K)).all(), (name, args)
    return [(o, cand[e, k], ref["rows"][e][k]) for e, o in enumerate(os_) for k in range(K) if ref["solved"][e, k]]


# ---- 1. the nets ------------------------------------------------------------------------------------------------------------------------------
def plan_parents(lib, net):
    """(bus_of_pos, parent position of every node; n: the slack) of the plan a host-only handle makes of `net`"""
    h, keep = host_handle(lib, net)
    try:
        fac, bop = np.zeros((net.n_bus - 1) * 12), np.zeros(net.n_bus, np.int32)
        assert lib.mapdn_get_flat_factors(h, _lib._p(fac, _lib._pd), _lib._p(bop, _lib._pi)) == 0
    finally:
        lib.mapdn_destroy(h)
    n = net.n_bus - 1
    bop = [int(b) for b in bop[:n]]
    pos = {b: i for i, b in enumerate(bop)}
    on = net.line_in_service.astype(bool)
    adj = {b: set() for b in range(net.n_bus)}
    for a, b in zip(net.line_from_bus[on], net.line_to_bus[on]):
        adj[int(a)].add(int(b)); adj[int(b)].add(int(a))
    par = []
    for k, b in enumerate(bop):                                   # children come before parents: the one neighbour at a higher position
        up = [pos[w] for w in adj[b] if w != net.ext_grid_bus and pos[w] > k]
        assert len(up) <= 1, (k, up)
        par.append(up[0] if up else n)
    return bop, par


@pytest.mark.parametrize("name", EN.NETS)
def test_nets_hold_their_edges(lib, name):
    net, prof, _ = G.make(name)
    assert net.n_gen == 0 and not net.has_fused_buses and not net.has_zip_loads
    h, keep = host_handle(lib, net)
    try:                                                          # not refused by name: a host-only handle answers MAPDN_E_STATE
        one = C.c_void_p(1)
        assert lib.mapdn_action_gradients(h, one, 1, 3, one, one, one, one, None, None, None) == -4, lib.mapdn_last_error(h).decode()
    finally:
        lib.mapdn_destroy(h)
    bop, par = plan_parents(lib, net)
    n = net.n_bus - 1
    kids = [[c for c in range(n) if par[c] == k] for k in range(n)]
    if name == "case141":
        return
    assert (net.bus_vn_kv == 12.66).all() and net.n_load == n
    depth, tree_kids = EN.depth_and_children(EN.PARENTS[name])
    roots = len(tree_kids[0])
    assert sum(p == n for p in par) == roots                     # one elimination tree per feeder leaving the slack bus
    if name == "pair":
        assert n == 1 and par == [1] and kids == [[]]
    if name == "chain40":
        assert n == 40 and max(depth) == 40 and max(len(c) for c in tree_kids) == 1 and sorted(depth[b] for b in net.sgen_bus) == [1, 20, 40]
        assert max(len(c) for c in kids) <= 2                    # (the plan roots a tree at its centre: two chains of 20 meet there)
    if name == "star12":
        hub = bop.index(1)
        assert len(kids[hub]) == 12 and all(not kids[c] for c in kids[hub]) and int(net.sgen_bus[0]) == 1
        assert sum(depth[b] == 2 for b in net.sgen_bus) == 3
        # Positions are a reversed pre-order, so node k - 1 is the first child of every node k that has one: a junction none of whose
        # children is k - 1 cannot come out of the plan (the branch of opf_tables that skips the reordering is taken by leaves alone)
        assert hub - 1 in kids[hub]
    if name == "feeders3":
        assert roots == 3 and sorted(len([b for b in range(1, net.n_bus) if _feeder(b, EN.PARENTS[name]) == r]) for r in tree_kids[0]) == [2, 5, 9]
        on_slack = [j for j, b in enumerate(net.sgen_bus) if int(b) == int(net.ext_grid_bus)]
        assert on_slack == [3] and len({_feeder(int(b), EN.PARENTS[name]) for b in net.sgen_bus[:3]}) == 3
    if name == "comb10":
        trunk = [b for b in range(1, net.n_bus) if tree_kids[b]]
        assert len(trunk) == 10 and all(sum(not tree_kids[c] for c in tree_kids[b]) == 1 for b in trunk)
        assert all(not tree_kids[int(b)] for b in net.sgen_bus) and net.n_sgen == 5
    if name == "ties":
        off = np.flatnonzero(net.line_in_service == 0)
        assert net.n_bus == 12 and list(off) == [row for _, _, row in EN.TIES_OUT] and net.n_line == 13
        assert int(net.line_in_service.sum()) == n               # radial for the plan: the open rows would close loops
        for a, b, row in EN.TIES_OUT:
            assert (int(net.line_from_bus[row]), int(net.line_to_bus[row])) == (a, b) and EN.PARENTS[name][b] != a and EN.PARENTS[name][a] != b
        both = (net.line_c_nf_per_km > 0) & (net.line_g_us_per_km > 0) & (net.line_in_service == 1)
        assert (net.line_parallel == 2).sum() == 1 and both[net.line_parallel == 2].all()
        assert ((net.line_c_nf_per_km > 0) & (net.line_in_service == 1)).sum() >= 3 and ((net.line_g_us_per_km > 0) & (net.line_in_service == 1)).sum() >= 3


def _feeder(b, parent):
    while parent[b] != 0:
        b = parent[b]
    return b


def test_ref_envs64():
    assert EN.ref_envs64(1) == [0] and EN.ref_envs64(64) == [0, 1, 2, 15, 16, 17, 61, 62, 63]
    assert EN.ref_envs64(65) == [0, 1, 2, 15, 16, 17, 62, 63, 64]
    assert EN.ref_envs64(130) == [0, 1, 2, 15, 16, 17, 62, 63, 64, 65, 127, 128, 129]
    for name in ("crowded", "special", "tiny", "case33"):        # the arrays the present tests see are what they were
        c = G.candidates(name, W.B_MAX, W.K_MAX)
        assert c.shape[:2] == (33, 7) and (c[:, 2] == W.UNSOLVABLE).all() and (c[:, 0] == 0).all()


# ---- 2. the conditions of the scenario (asserted, never skipped) ---------------------------------------------------------------------------
def gpu_batch(name):
    return 65 if name == "case141" else EN.B_MAX


@pytest.mark.parametrize("name", EN.NETS)
def test_scenario_conditions(name):
    B = gpu_batch(name)
    os_, ref, cand = G.reference(name, B, K)
    assert (ref["solved"] == W.expected_pattern(K)).all(), name   # solved, solved, unsolvable, solved on every env the GPU tests use
    assert (ref["reward"][:, 2] < -200.0).all() and (ref["info"][:, 2, 10] == 1.0).all()
    for o in os_:
        lim = G.limits(o)
        assert (lim > 0.0).all() and (lim < o.s_max).all() and (o.sgen_p > 0.0).all(), (name, o.env_id)
    envs = list(CPU_ENVS[name])
    sub = dict(solved=ref["solved"][envs], vm=ref["vm"][envs])
    dv, dq = G.kink_margins([os_[e] for e in envs], sub, cand[envs])
    assert dv >= V_MARGIN and dq >= Q_MARGIN, (name, dv, dq)
    if name in ("chain40", "case141"):                            # the steep branches of the barrier on the deep trees
        pq = np.setdiff1d(np.arange(os_[0].net.n_bus), [os_[0].net.ext_grid_bus])
        vm = ref["vm"][envs][ref["solved"][envs]][:, pq]
        assert (vm < 0.95).any() or (vm > 1.05).any(), name
        out = [(ref["vm"][e][ref["solved"][e]][:, pq] < 0.95).any() or (ref["vm"][e][ref["solved"][e]][:, pq] > 1.05).any() for e in EN.ref_envs64(B)]
        assert any(out), name                                     # and among the envs the GPU test holds to the reference


# ---- 3. the reference against central differences ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,args", CD_CASES, ids=[n + ("-line" if a else "") for n, a in CD_CASES])
def test_reference_against_central_differences(name, args):
    """step H = 2e-4 and H / 2 of tests/test_action_grad_cpu.py; measured worst case 2.369e-8 (pair), bound 2.369e-7 = 10 x that"""
    worst = 0.0
    for o, a, p in rows_of(name, args):
        g = G.reward_gradient(o.net, G.env_args(o), p["r"].V, a, G.limits(o))
        for h in (H, H / 2):
            worst = max(worst, G.rel_inf(G.central_difference(name, o, a, h), g))
    print(f"\n[grad cd] {name} {dict(args)}: worst relative disagreement {worst:.3e} (bound {CD_TOL:.1e})")
    assert worst <= CD_TOL, (name, args, worst)


# ---- 4. out-of-service rows ---------------------------------------------------------------------------------------------------------------------
def test_out_of_service_rows_count_in_the_mean_and_nothing_else():
    """`ties` under line_weight against the same net with the two open rows deleted: the same gradient once the weight is rescaled by the
    ratio of the row counts (the open rows add nothing to c), and, the barrier term set aside, 11 / 13 of it when it is not (they count in
    n_line).  Float64
    reference; the two evaluations differ by the rounding of weight / n_line and what the solve makes of it: 64 ulp of |g|inf."""
    short = EN.ties_without_the_open_rows()
    for o, a, p in rows_of("ties", G.LINE_ARGS):
        net = o.net
        assert (net.n_line, short.n_line) == (13, 11)
        assert np.array_equal(make_ybus(net)[0].toarray(), make_ybus(short)[0].toarray())
        args = G.env_args(o)
        V, lim = p["r"].V, G.limits(o)
        g = G.reward_gradient(net, args, V, a, lim)
        assert np.abs(g).max() > 0.0
        same = G.reward_gradient(short, dict(args, line_weight=args["line_weight"] * short.n_line / net.n_line), V, a, lim)
        assert G.rel_inf(g, same) <= 64 * ULP
        lines_only = dict(args, voltage_weight=0.0)            # (the barrier term does not scale with the row count)
        g0, plain = G.reward_gradient(net, lines_only, V, a, lim), G.reward_gradient(short, lines_only, V, a, lim)
        assert np.abs(g0).max() > 0.0 and G.rel_inf(g0 * net.n_line / short.n_line, plain) <= 64 * ULP
        # and the oracle's reward is that mean: pl_mw of an open row is 0, and the row counts
        pl = p["r"].pl_mw
        assert pl.shape == (13,) and (pl[[row for _, _, row in EN.TIES_OUT]] == 0.0).all() and (np.delete(pl, [4, 9]) != 0.0).all()


# ---- 5. csrc/grad.hpp on the host -----------------------------------------------------------------------------------------------------------
def line_records(net, pos):
    """plan.hpp LineFlow of every net.line row: fpos, tpos, gff, gtt, gft + gtf, bft - btf; an out-of-service row: both ends at the slack
    position and zero constants"""
    n = net.n_bus - 1
    f, t, r, x, bc, tap, is_line = build_branches(net)
    ys = 1.0 / (r + 1j * x)
    ytt = ys + 1j * bc / 2
    yff, yft, ytf = ytt / (tap * np.conj(tap)), -ys / np.conj(tap), -ys / tap
    out, i = [], 0
    for l in range(net.n_line):
        if not net.line_in_service[l]:
            out.append([n, n, 0.0, 0.0, 0.0, 0.0])
            continue
        assert is_line[i] and (int(f[i]), int(t[i])) == (int(net.line_from_bus[l]), int(net.line_to_bus[l]))
        out.append([pos[int(f[i])], pos[int(t[i])], yff[i].real, ytt[i].real, yft[i].real + ytf[i].real, yft[i].imag - ytf[i].imag])
        i += 1
    return np.array(out)


@pytest.mark.parametrize("name,args", CASES, ids=CASE_IDS)
def test_host_gradient_against_the_extended_reference(host_grad, name, args):
    """the right-hand side, the two sweeps and the read-out in k_action_grad's order, g++ -O2, at the oracle's V of the solved rows of the
    CPU envs, against the extended reference: within G.bar, 16 x the float64 reference's own error on the case and never below 64 ulp of
    the row's largest entry.  The tables are tests/test_opf_cpu.tree_tables: trees rooted at the slack's neighbours, so chain40 is one
    chain of 40 here (the plan's own order, rooted at the centre, runs on the GPU)."""
    worst = 0.0
    bar = G.bar(name, args)
    for o, a, p in rows_of(name, args):
        net, V, lim, cfg = o.net, p["r"].V, G.limits(o), G.env_args(o)
        Y = make_ybus(net)[0].toarray()
        bus_of_pos, par, cptr, cidx, yt = tree_tables(Y, int(net.ext_grid_bus), net.ext_grid_vm_pu)
        n = net.n_bus - 1
        pos = {b: i for i, b in enumerate(bus_of_pos)}
        pos[int(net.ext_grid_bus)] = n
        Vp = np.concatenate([V[bus_of_pos], [V[net.ext_grid_bus]]])
        lines = line_records(net, pos)
        sg = np.array([[pos[int(b)], lim[j], net.sgen_scaling[j], a[j]] for j, b in enumerate(net.sgen_bus)])
        head = [net.n_bus, int(cfg["line_weight"] is not None), BARRIER_IDS[cfg["voltage_barrier_type"]], cfg["voltage_weight"],
                cfg["q_weight"] or 0.0, cfg["line_weight"] or 0.0, net.sn_mva]
        tab = np.concatenate([par, cptr, cidx, yt.ravel()])
        got = host_grad(np.concatenate([[2, n, len(cidx), net.n_sgen, lines.shape[0]], tab, Vp.real, Vp.imag, np.abs(Vp), head, lines.ravel(), sg.ravel()]))
        ext = G.reward_gradient(net, cfg, V, a, lim, ext=True)
        err = G.rel_inf(got, ext)
        worst = max(worst, err)
        assert err <= bar, (name, args, o.env_id, err, bar)
        for j, b in enumerate(net.sgen_bus):                      # an sgen on the slack bus: the direct term alone
            if int(b) == int(net.ext_grid_bus):
                want = 0.0 if cfg["line_weight"] is not None else -cfg["q_weight"] / net.n_sgen * np.sign(lim[j] * a[j] * net.sgen_scaling[j]) * (lim[j] * net.sgen_scaling[j])
                assert got[j] == want, (name, j)
    print(f"\n[grad host] {name} {dict(args)}: e64 {G.E64[(name, tuple(args))]:.2e} host {worst:.2e} bar {bar:.2e}")


def test_host_gradient_of_a_non_finite_slack_action_is_what_grad_entry_gives(host_grad):
    """grad_entry itself keeps sign0(NaN) = 0 (a finite entry for a NaN action on the slack-bus sgen); k_action_grad tests lim_j a_j of the
    whole row before it calls it (tests/test_action_grad_edges_gpu.py) — this pins where the rule lives"""
    o, a, p = rows_of("feeders3", ())[1]
    net, V, lim, cfg = o.net, p["r"].V, G.limits(o), G.env_args(o)
    Y = make_ybus(net)[0].toarray()
    bus_of_pos, par, cptr, cidx, yt = tree_tables(Y, 0, net.ext_grid_vm_pu)
    n = net.n_bus - 1
    pos = {b: i for i, b in enumerate(bus_of_pos)}
    pos[0] = n
    Vp = np.concatenate([V[bus_of_pos], [V[0]]])
    a = a.copy()
    a[3] = np.nan
    sg = np.array([[pos[int(b)], lim[j], net.sgen_scaling[j], a[j]] for j, b in enumerate(net.sgen_bus)])
    head = [net.n_bus, 0, BARRIER_IDS["bowl"], cfg["voltage_weight"], cfg["q_weight"], 0.0, net.sn_mva]
    got = host_grad(np.concatenate([[2, n, len(cidx), net.n_sgen, 0], par, cptr, cidx, yt.ravel(), Vp.real, Vp.imag, np.abs(Vp), head, sg.ravel()]))
    assert got[3] == 0.0 and np.isfinite(got).all()


# ---- 6. the E64 constants of the new cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,args", CASES, ids=CASE_IDS)
def test_e64_constants_are_what_the_float64_reference_gives(name, args):
    got = G.e64(name, args)
    print(f"\n[grad e64] {name} {dict(args)}: {got:.2e} (constant {G.E64[(name, args)]:.2e})")
    assert 0.5 * G.E64[(name, args)] <= got <= 2.0 * G.E64[(name, args)], (name, args, got)
