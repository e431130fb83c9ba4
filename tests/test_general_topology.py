"""General-topology power flow (meshed nets): pp.runpp (voltage_control_env.py:557) solves any connected net; the
product solves radial feeders with the tree kernel and everything else with k_nr_dense (dense Jacobian in LDS, blocked
LU with 2x2 block pivots and v_mfma_f64_16x16x4_f64 trailing updates).  Checker: oracle/pp_restated.py (SuperLU
spsolve on the sparse Jacobian, as pandapower) + the solver-independent residual certificate."""
import ctypes as C

import numpy as np
import pytest

from mapdn_amd import _lib
from mapdn_amd.netspec import NetSpec, Profiles, add_lines, case33_meshed, make_case
from tests.edge_rule import same_newton_count
from tests.meshed_edge_nets import dense_newton, emulate_program as _emulate_program, positions as _positions
from oracle.pp_restated import make_ybus, residual_inf, runpp_restated


def random_meshed_net(seed, nb_max=60):
    """random tree + random extra links (loops), slack anywhere, random line data / loads / sgens / shunts"""
    rng = np.random.default_rng(1000 + seed)
    nb = int(rng.integers(5, nb_max))
    parent = np.array([-1] + [int(rng.integers(max(0, i - int(rng.integers(1, 6))), i)) for i in range(1, nb)])
    perm = rng.permutation(nb)
    f = list(perm[parent[1:]]); t = list(perm[np.arange(1, nb)])
    pairs = {(min(a, b), max(a, b)) for a, b in zip(f, t)}
    n_extra = int(rng.integers(1, max(2, nb // 4)))
    while n_extra:
        a, b = (int(x) for x in rng.integers(0, nb, 2))
        if a == b or (min(a, b), max(a, b)) in pairs:
            continue
        pairs.add((min(a, b), max(a, b))); f.append(a); t.append(b); n_extra -= 1
    n_line = len(f)
    slack = int(perm[int(rng.integers(0, nb))])
    nz = int(rng.integers(1, 4))
    zone = rng.integers(1, nz + 1, nb).astype(np.int32); zone[slack] = 0
    ns = int(rng.integers(1, 7))
    cand = np.array([b for b in range(nb) if b != slack])
    sgen_bus = rng.choice(cand, size=ns, replace=True).astype(np.int32)
    nl = int(rng.integers(1, 2 * nb))
    load_bus = rng.integers(0, nb, nl).astype(np.int32)
    vn = float(rng.choice([0.4, 11.0, 20.0])); sn = float(rng.choice([0.5, 1.0, 10.0])); zb = vn * vn / sn
    nsh = int(rng.integers(0, 3))
    net = NetSpec(name=f"mesh{seed}", bus_vn_kv=np.full(nb, vn), bus_zone=zone, line_from_bus=np.array(f), line_to_bus=np.array(t),
                  line_r_ohm_per_km=rng.uniform(0.05, 0.5, n_line) * zb * 0.02, line_x_ohm_per_km=rng.uniform(0.0, 0.4, n_line) * zb * 0.02,
                  line_c_nf_per_km=rng.uniform(0, 50, n_line), line_g_us_per_km=rng.uniform(0, 1, n_line),
                  line_length_km=rng.uniform(0.2, 1.5, n_line), line_parallel=rng.integers(1, 3, n_line).astype(np.int32),
                  line_in_service=np.ones(n_line, np.uint8), load_bus=load_bus, sgen_bus=sgen_bus, sgen_zone=zone[sgen_bus],
                  ext_grid_bus=slack, ext_grid_vm_pu=float(rng.uniform(0.98, 1.03)), sn_mva=sn, f_hz=50.0,
                  shunt_bus=rng.integers(0, nb, nsh).astype(np.int32), shunt_p_mw=rng.uniform(0, 0.01 * sn, nsh),
                  shunt_q_mvar=rng.uniform(-0.05 * sn, 0.05 * sn, nsh))
    T = 1500
    pv = rng.uniform(0, 0.3 * sn / ns, (T, ns)); lp = rng.uniform(0, 0.4 * sn / nl, (T, nl)); lq = lp * rng.uniform(0.1, 0.5, (T, nl))
    return net, Profiles(pv=pv, load_p=lp, load_q=lq, time_delta_min=3)


def host_handle(net, args=None):
    lib = _lib.load()
    a = dict(episode_limit=240, action_scale=0.8, action_bias=0.0, voltage_barrier_type="l1")
    a.update(args or {})
    cnet, keep = _lib.make_cnetspec(net)
    ccfg = _lib.make_cconfig(a)
    h = C.c_void_p()
    rc = lib.mapdn_create(C.byref(cnet), C.byref(ccfg), 4, -1, C.byref(h))
    return lib, h, rc, keep


# ------------------------------------------------------------------------------------------------ CPU
def test_meshed_nets_are_accepted_and_ybus_matches_the_oracle():
    base, _ = make_case("case33")
    for net in [case33_meshed(base, 1), case33_meshed(base, 5)] + [random_meshed_net(s)[0] for s in range(6)]:
        lib, h, rc, keep = host_handle(net)
        assert rc == 0, lib.mapdn_last_error(None)
        dims = _lib.CDims()
        assert lib.mapdn_dims(h, C.byref(dims)) == 0 and dims.is_radial == 0 and dims.n_bus == net.n_bus
        out = np.zeros((net.n_bus, net.n_bus, 2))
        assert lib.mapdn_get_ybus_dense(h, _lib._p(out, _lib._pd)) == 0
        yo = make_ybus(net)[0].toarray()
        assert np.abs(out[..., 0] + 1j * out[..., 1] - yo).max() <= 1e-12 * np.abs(yo).max()
        # the tree-only debug exports refuse a meshed plan instead of returning garbage
        nrows = C.c_int32()
        assert lib.mapdn_get_schedule(h, 1, C.byref(nrows), None, None) == _lib_E_TOPOLOGY
        lib.mapdn_destroy(h)


_lib_E_TOPOLOGY = -2


def test_large_meshed_nets_are_accepted_and_disconnected_ones_refused_loudly(monkeypatch):
    net, _ = make_case("case141")
    meshed = add_lines(net, [5], [77], 0.3, 0.2)
    lib, h, rc, keep = host_handle(meshed)                  # general sparse solver: any meshed net whose blocks fit in LDS
    assert rc == 0, lib.mapdn_last_error(None)
    lib.mapdn_destroy(h)
    monkeypatch.setenv("MAPDN_NR_DENSE", "1")               # the dense MFMA solver: Jacobian in LDS up to 65 buses, in global memory
    lib, h, rc, keep = host_handle(meshed)                  # (one thread per row) up to 513
    assert rc == 0, lib.mapdn_last_error(None)
    lib.mapdn_destroy(h)
    from mapdn_amd.netspec import _radial_case
    huge, _ = _radial_case("rand601", 601, 300, 20, 10, 21, 12.47, 10.0, 10.0, 5, 0.05)
    lib, h, rc, keep = host_handle(huge)
    assert rc == _lib_E_TOPOLOGY and b"513 buses" in lib.mapdn_last_error(None)
    monkeypatch.delenv("MAPDN_NR_DENSE")
    island = net.copy(); island.line_in_service[3] = 0
    lib, h, rc, keep = host_handle(island)
    assert rc == _lib_E_TOPOLOGY and b"not connected" in lib.mapdn_last_error(None)


def test_oracle_on_meshed_nets_meets_the_residual_certificate_and_a_dense_solve():
    """the checker itself on loops: SuperLU path vs the residual certificate and vs a dense numpy Newton iteration"""
    for seed in range(6):
        net, prof = random_meshed_net(seed)
        rng = np.random.default_rng(seed)
        r = int(rng.integers(0, prof.n_rows))
        qs = rng.uniform(-0.2, 0.2, net.n_sgen) * prof.pv[r]
        res = runpp_restated(net, prof.load_p[r], prof.load_q[r], prof.pv[r], qs)
        assert res.converged
        assert residual_inf(net, res.V, prof.load_p[r], prof.load_q[r], prof.pv[r], qs) < 1e-8 / net.sn_mva
        # independent dense Newton in rectangular coordinates (tests/meshed_edge_nets.py)
        v = dense_newton(net, prof.load_p[r], prof.load_q[r], prof.pv[r], qs, n_it=20)
        assert np.abs(v - res.V).max() < 1e-9


# ------------------------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("n", [2, 14, 16, 30, 32, 48, 64, 66, 96, 126, 128, 130, 280, 322, 642])
def test_dense_lu_matches_numpy(n):
    """(n > 128: the same LU on a matrix in global memory — one thread per row, up to 11 waves — as k_nr_dense runs beyond 65 buses)
    the kernel's LDS-resident blocked LU (2x2 block pivots, f64 MFMA trailing updates) against numpy.linalg.solve;
    includes matrices whose scalar diagonal is ZERO (rotation-like bus blocks: only a block pivot survives) and an
    asymmetric identity-like case that would expose a swapped MFMA fragment layout"""
    import torch
    lib = _lib.load()
    rng = np.random.default_rng(n)
    batch = 7
    A = rng.normal(0, 1, (batch, n, n))
    for s in range(batch):
        for k in range(0, n, 2):                     # strong 2x2 diagonal blocks [[a, b], [-b, a]]
            a_, b_ = (0.0 if s % 2 else rng.uniform(1, 2)), rng.uniform(2, 3) * n ** 0.5
            A[s, k:k + 2, k:k + 2] = [[a_, b_], [-b_, a_]]
    A[0] = np.triu(rng.normal(0, 1, (n, n)), 2)      # A[0]: identity + a strictly upper part (asymmetric)
    A[0] += np.eye(n)
    b = rng.normal(0, 1, (batch, n))
    x = torch.zeros(batch, n, dtype=torch.float64, device="cuda:0")
    ta, tb = torch.as_tensor(A, device="cuda:0").contiguous(), torch.as_tensor(b, device="cuda:0").contiguous()
    rc = lib.mapdn_dense_solve(ta.data_ptr(), tb.data_ptr(), x.data_ptr(), n, batch, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    ref = np.linalg.solve(A, b[..., None])[..., 0]
    err = np.abs(x.cpu().numpy() - ref).max() / np.abs(ref).max()
    assert err < 1e-11, err


def _solve_inputs(net, prof, B, seed):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, prof.n_rows, B)
    pv = prof.pv[rows]
    qs = rng.uniform(-0.8, 0.8, (B, net.n_sgen)) * np.sqrt(prof.s_max() ** 2 - pv ** 2)
    return prof.load_p[rows], prof.load_q[rows], pv, qs


def _meshed(which):
    if which.startswith("case33"):
        base, prof = make_case("case33")
        return case33_meshed(base, int(which[-1])), prof
    if which == "case141_ties":
        base, prof = make_case("case141")
        return add_lines(base, [5, 40, 77, 100], [77, 120, 130, 12], 0.3, 0.2), prof
    if which == "case322_ties":
        base, prof = make_case("case322")
        return add_lines(base, [5, 40, 177, 200, 300], [77, 120, 30, 12, 150], 0.3, 0.2), prof
    if which.startswith("big"):
        return random_meshed_net(int(which[3:]), nb_max=160)
    return random_meshed_net(int(which[4:]))


@gpu
@pytest.mark.parametrize("solver,which", [("sparse", w) for w in ["case33_tie1", "case33_tie5", "case141_ties", "case322_ties", "big1", "big2", "big3"]
                                          + [f"rand{s}" for s in range(8)]]
                         + [("dense", w) for w in ["case33_tie1", "case33_tie5", "case141_ties", "case322_ties", "big2"] + [f"rand{s}" for s in range(8)]])
def test_meshed_solve_matches_oracle(solver, which, monkeypatch):
    """both general-topology solvers — the sparse block program (default for meshed nets, any size that fits LDS) and the
    dense LU with f64 MFMA (MAPDN_NR_DENSE=1; Jacobian in LDS up to 65 buses, in global memory beyond: the 141- / 322-bus nets) —
    against the oracle's SuperLU Newton"""
    import torch
    from mapdn_amd.env import VoltageControlBatch
    net, prof = _meshed(which)
    if solver == "dense":
        monkeypatch.setenv("MAPDN_NR_DENSE", "1")
    B = 70 if not (solver == "dense" and net.n_bus > 65) else 24
    a = dict(episode_limit=240, action_scale=0.8, action_bias=0.0, voltage_barrier_type="l2", seed=1)
    env = VoltageControlBatch(net, prof, a, n_envs=B, device="cuda:0", obs_dtype=torch.float64)
    assert not env.is_radial
    pl, ql, pv, qs = _solve_inputs(net, prof, B, 5)
    vm, va, it, cv = (t.cpu().numpy() for t in env.solve(pl, ql, pv, qs))
    assert cv.all()
    worst = 0.0
    for e in range(B):
        r = runpp_restated(net, pl[e], ql[e], pv[e], qs[e])
        assert r.converged and same_newton_count(net, (pl[e], ql[e], pv[e], qs[e]), it[e], True, r)
        worst = max(worst, np.abs(vm[e] - r.vm_pu).max(), np.abs(va[e] - r.va_degree).max() * np.pi / 180)
        v = vm[e] * np.exp(1j * va[e] * np.pi / 180)
        assert residual_inf(net, v, pl[e], ql[e], pv[e], qs[e]) < 1e-8 / net.sn_mva
    assert worst < 1e-9, worst
    env.close()


@gpu
@pytest.mark.parametrize("solver,case", [("MAPDN_NR_DENSE", "case33"), ("MAPDN_NR_SPARSE", "case33"), ("MAPDN_NR_SPARSE", "case141"),
                                         ("MAPDN_NR_SPARSE", "case322"), ("MAPDN_NR_DENSE", "case141"), ("MAPDN_NR_DENSE", "case322")])
def test_general_solvers_equal_the_tree_solver_on_radial_feeders(solver, case, monkeypatch):
    """MAPDN_NR_DENSE=1 / MAPDN_NR_SPARSE=1 force a general solver onto a radial feeder: same Newton iterates as the tree
    elimination (a tree has no fill: the sparse program is then the tree elimination in minimum-degree order)"""
    import torch
    from mapdn_amd.env import VoltageControlBatch
    net, prof = make_case(case)
    a = dict(episode_limit=240, action_scale=0.8, action_bias=0.0, voltage_barrier_type="bowl", seed=0)
    B = 130 if not (solver == "MAPDN_NR_DENSE" and net.n_bus > 65) else 40
    ins = _solve_inputs(net, prof, B, 9)
    tree = VoltageControlBatch(net, prof, a, n_envs=B, device="cuda:0")
    rt = [t.cpu().numpy() for t in tree.solve(*ins)]
    tree.close()
    monkeypatch.setenv(solver, "1")
    dense = VoltageControlBatch(net, prof, a, n_envs=B, device="cuda:0")
    rd = [t.cpu().numpy() for t in dense.solve(*ins)]
    dense.close()
    assert (rt[2] == rd[2]).all() and rd[3].all()
    assert np.abs(rt[0] - rd[0]).max() < 1e-12 and np.abs(rt[1] - rd[1]).max() < 1e-10


@gpu
@pytest.mark.parametrize("solver,which", [("sparse", "case33_tie5"), ("sparse", "rand2"), ("sparse", "case141_ties"), ("sparse", "big2"),
                                          ("dense", "case33_tie5"), ("dense", "rand5"), ("dense", "case141_ties")])
def test_meshed_env_episode_matches_the_oracle_env(solver, which, monkeypatch):
    """the whole step (inject -> general solve -> fused reward epilogue -> commit -> obs) on a meshed net"""
    import torch
    from mapdn_amd.env import VoltageControlBatch
    from oracle.env_restated import INFO_KEYS, VoltageControlOracle
    net, prof = _meshed(which)
    if solver == "dense":
        monkeypatch.setenv("MAPDN_NR_DENSE", "1")
    a = dict(episode_limit=240, action_scale=0.8, action_bias=0.0, voltage_barrier_type="bowl", seed=3)
    B = 5
    env = VoltageControlBatch(net, prof, a, n_envs=B, device="cuda:0", obs_dtype=torch.float64)
    oracles = [VoltageControlOracle(net, prof, a, env_id=e, do_reset=False) for e in range(B)]
    obs, state = env.reset()
    for e, o in enumerate(oracles):
        oo, os_ = o.reset()
        assert np.abs(np.array(oo) - obs[e].cpu().numpy()).max() < 1e-9 and np.abs(os_ - state[e].cpu().numpy()).max() < 1e-7
    rng = np.random.default_rng(0)
    for t in range(4):
        act = rng.uniform(-0.8, 0.8, (B, net.n_sgen))
        r, term, info = env.step(torch.as_tensor(act, device="cuda:0"))
        res = env.results(); obs = env.get_obs()
        for e, o in enumerate(oracles):
            ro, to, io = o.step(act[e])
            assert abs(ro - r[e].item()) < 1e-9 and to == bool(term[e].item())
            assert max(abs(io[k] - info[e, c].item()) for c, k in enumerate(INFO_KEYS)) < 1e-9
            assert np.abs(res["vm_pu"][e].cpu().numpy() - o.res.vm_pu).max() < 1e-9
            assert np.abs(res["p_mw"][e].cpu().numpy() - o.res.p_mw).max() < 1e-9
            assert np.abs(res["pl_mw"][e].cpu().numpy() - o.res.pl_mw).max() < 1e-9
            assert np.abs(np.array(o.get_obs()) - obs[e].cpu().numpy()).max() < 1e-9
    env.close()


# ------------------------------------------------------------------------------------------------ sparse program (CPU)
# (the numpy interpreter of the program and the position export live in tests/meshed_edge_nets.py, which runs them on more shapes)
@pytest.mark.parametrize("which,S", [("case33_tie5", 4), ("case33_tie5", 16), ("rand3", 8), ("rand6", 32), ("case141_ties", 8), ("case322_ties", 16), ("case141_radial", 8)])
def test_sparse_elimination_program_solves_the_jacobian(which, S):
    """host symbolic factorisation (minimum degree, fill) + list-scheduled block program, executed in numpy, against
    scipy's spsolve on the oracle's Jacobian — for weakly meshed 141 / 322-bus nets too"""
    import scipy.sparse.linalg as spla
    from oracle.pp_restated import jacobian
    if which.startswith("case33"):
        net = case33_meshed(make_case("case33")[0], 5)
    elif which == "case141_ties":
        net = add_lines(make_case("case141")[0], [5, 40, 77, 100], [77, 120, 130, 12], 0.3, 0.2)
    elif which == "case322_ties":
        net = add_lines(make_case("case322")[0], [5, 40, 177, 200, 300], [77, 120, 30, 12, 150], 0.3, 0.2)
    elif which == "case141_radial":
        net = make_case("case141")[0]
    else:
        net = random_meshed_net(int(which[4:]))[0]
    lib, h, rc, keep = host_handle(net)
    assert rc == 0, lib.mapdn_last_error(None)
    n = net.n_bus - 1
    dims = np.zeros(6, np.int32)
    assert lib.mapdn_get_sparse_program(h, S, _lib._p(dims, _lib._pi), None, None, None) == 0
    ops = np.zeros(dims[2] * S * 4, np.int32); order = np.zeros(n, np.int32); sl = np.zeros(3 * dims[5], np.int32)
    assert lib.mapdn_get_sparse_program(h, S, _lib._p(dims, _lib._pi), _lib._p(ops, _lib._pi), _lib._p(order, _lib._pi), _lib._p(sl, _lib._pi)) == 0
    assert sorted(order.tolist()) == list(range(n))
    # positions: ask the library which bus sits where (flat-factor export is tree-only; use the schedule-free bus_of_pos via ybus order)
    # meshed plans order positions by ascending bus id without the slack; radial ones by the elimination forest: rebuild J in
    # POSITION order from the library's own dense Ybus permuted accordingly
    pos_bus = _positions(lib, h, net)
    rng = np.random.default_rng(0)
    v = (1.0 + 0.05 * rng.standard_normal(net.n_bus)) * np.exp(1j * 0.05 * rng.standard_normal(net.n_bus))
    ybus = make_ybus(net)[0]
    pq = np.array(pos_bus[:n])
    Jpp = jacobian(ybus, v, pq, pq).toarray()          # [[dP/dth, dP/dVm], [dQ/dth, dQ/dVm]] over pq in position order
    Jpp[:, n:] *= np.abs(v[pq])[None, :]                # scaled unknowns d|V|/|V|
    perm = np.ravel(np.column_stack([np.arange(n), n + np.arange(n)]))   # interleave (theta_k, v_k) / (P_k, Q_k) per node
    J = Jpp[np.ix_(perm, perm)]
    b = rng.standard_normal(2 * n)
    x = _emulate_program(n, S, dims, ops, sl, J, b)
    ref = spla.spsolve(__import__("scipy.sparse", fromlist=["csc_matrix"]).csc_matrix(J), b)
    assert np.abs(x - ref).max() < 1e-9 * max(1.0, np.abs(ref).max())
    nph = int(dims[2])
    if which == "case141_radial":
        assert dims[1] == 0 and nph < 200                # a tree has no fill; list scheduling finds its parallelism
    lib.mapdn_destroy(h)

