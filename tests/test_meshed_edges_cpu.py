"""The nets of tests/meshed_edge_nets.py without a GPU: which solver and geometry a host-only handle settles on per shape and pin (the
LDS ladder of k_nr_sparse with its refusal texts), the program dims that make each shape an edge, the host-compiled elimination
program executed in numpy for every S = 64 / sp_lanes against spsolve on the oracle's Jacobian, Ybus against make_ybus (the doubled
line merged into one entry), the conditions on the input pools by the oracle alone, and the oracle-only preconditions of the step()
replays."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from mapdn_amd import _lib
from oracle.pp_restated import make_ybus
from tests import element_edge_nets as N
from tests import meshed_edge_nets as M


# ---- solver and geometry ------------------------------------------------------------------------------------------------------------
def _pin_id(pin):
    return "auto" if pin is None else ("dense" if pin["nr_solver"] == "dense" else f"sp{pin['sp_lanes']}")


@pytest.mark.parametrize("key", M.KEYS)
def test_solver_and_geometry_per_shape(key):
    """is_radial, the kernel and lds_bytes of a host-only handle under the automatic choice and under every pin"""
    net, _ = M.make_net(key)
    base = M.base_of(key)
    n = net.n_bus - 1
    dc, zip_ = M.variant_of(key)
    radial = int(base in M.RADIAL)
    refused = M.LDS_REFUSED[base]
    fits = [L for L in M.SP_LANES if L not in refused]
    for pin in M.PINS:
        r = M.host_report(key, pin)
        what = (key, _pin_id(pin), r)
        if pin is not None and pin["nr_solver"] == "dense":
            if dc or zip_:                                               # refused by name (pinned in tests/kernel_matrix.py REFUSALS)
                assert r["rc"] == M.E_INVALID and "not built for nr_solver = dense" in r["error"], what
                continue
            N_ = M.dense_order(n)
            ga = int(N_ > 128)
            W = (1 if N_ <= 64 else 2) if not ga else next(w for w in (3, 4, 5, 6, 8, 11, 13, 16) if 64 * w >= N_)
            assert r["rc"] == 0 and r["is_radial"] == radial and r["kernel"] == dict(solver=2, W=W, GA=ga), what
            assert r["lds_bytes"] == M.dense_lds_bytes(n, N_, W, ga) <= M.CU_LDS - 256, what
            continue
        if not fits:                                                     # grid16: no sp_lanes holds two envs of it
            assert r["rc"] == M.E_TOPOLOGY and M.FILL_REFUSAL in r["error"] and f"{net.n_bus} buses" in r["error"], what
            continue
        if pin is not None and pin["sp_lanes"] in refused:
            assert r["rc"] == M.E_INVALID and r["error"] == M.LDS_REFUSAL, what
            continue
        assert r["rc"] == 0 and r["is_radial"] == radial, what
        k = r["kernel"]
        if pin is None and radial:                                       # the doubled line is one branch of a tree
            assert k["solver"] == 0 and (k["DC"], k["ZIP"]) == (dc, zip_), what
            assert (k["W"], k["L"], k["HL"], k["GL"], k["RES"]) == (1, 16, 1, 1, 1), what     # one wave, everything LDS-resident
            assert r["lds_bytes"] == M.TREE_LDS_BYTES[base], what
            continue
        assert k["solver"] == 1 and (k["DC"], k["ZIP"]) == (dc, zip_), what
        L = k["L"]
        assert L in fits and (pin is None or L == pin["sp_lanes"]), what          # the automatic choice never lands on a refused L
        d = M.program_dims(key, 64 // L, pin)
        assert r["lds_bytes"] == M.sparse_lds_bytes(n, d["blocks"], L) <= M.CU_LDS, what
    for L in refused:                                                    # refused for the reason given: the blocks of L envs exceed a CU's LDS
        if fits:
            blocks = M.program_dims(key, 64 // L)["blocks"]
            assert M.sparse_lds_bytes(n, blocks, L) > M.CU_LDS, (key, L)
    for L in fits:
        assert M.sparse_lds_bytes(n, M.program_dims(key, 64 // L, None if not radial else dict(nr_solver="sparse"))["blocks"], L) <= M.CU_LDS


def test_the_lds_ladder_of_the_lattices():
    """grid16 fits nowhere (4103 blocks) but under the dense solver; the automatic handle of every shape that is refused somewhere
    settles on 2 lanes (test_solver_and_geometry_per_shape holds every pin of every shape to meshed_edge_nets.LDS_REFUSED)"""
    r = M.host_report("grid16")
    assert r["rc"] == M.E_TOPOLOGY and "needs 4103 Jacobian blocks after fill" in r["error"]
    r = M.host_report("grid16", dict(nr_solver="dense"))
    assert r["rc"] == 0 and r["kernel"] == dict(solver=2, W=8, GA=1)
    for key, L in (("grid6", 2), ("grid8", 2), ("grid10", 2), ("ladder65", 2), ("ladder66", 2)):
        assert M.host_report(key)["kernel"]["L"] == L


# ---- the dims that make a shape an edge -----------------------------------------------------------------------------------------------
PF = 8                                                                    # depth of both prefetch rings of k_nr_sparse


@pytest.mark.parametrize("S", [4, 8, 16, 32])
def test_program_dims_hold_the_edges(S):
    sparse = dict(nr_solver="sparse")
    d = M.program_dims("tri3", S)
    assert d["phases"] < PF and d["rows_per_sub"] * d["max_nnz"] < PF and 2 < S
    d = M.program_dims("pair2x", S, sparse)
    assert d["phases"] == 2 and d["rows_per_sub"] * d["max_nnz"] == 2 and d["fill"] == 0
    d = M.program_dims("k9", S)
    assert d["fill"] == 0 and d["max_nnz"] == 9 and d["slots"] == 8 * 7
    d = M.program_dims("ring33", S)
    assert d["fill"] > 0 and d["phases"] >= d["blocks"]
    assert d["fill"] == 2 * (32 - 3)                                      # a fill pair at every step until a triangle is left
    d = M.program_dims("wheel_rim", S)
    assert d["max_nnz"] == 25 and d["fill"] == 0
    d = M.program_dims("wheel_hub", S)
    assert d["max_nnz"] <= 4 and d["fill"] == 42
    d = M.program_dims("grid6", S)
    assert d["fill"] == 130 and d["blocks"] == 317 and 35 % S != 0
    for key, n in (("k9", 8), ("ring33", 32), ("ladder65", 64)):          # full last rows: n == S or a multiple of it
        assert n % S == 0 or n < S, (key, S)
        assert M.program_dims(key, S)["rows_per_sub"] == max(1, n // S)
    assert M.program_dims("ladder66", S)["rows_per_sub"] == 65 // S + 1   # one live row in the last round


# ---- the program, executed ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 8, 16, 32])
@pytest.mark.parametrize("key", M.EMULATED)
def test_program_emulation_solves_the_jacobian(key, S):
    """symbolic() + sparse_program() of the shape at S sub-lanes, run by meshed_edge_nets.emulate_program (which checks one write per
    block per phase, wave-uniform hints, at most S real operations a phase, no-ops on the scratch slot), against spsolve on the
    oracle's Jacobian at a perturbed voltage profile: the 1e-9 relative bound of test_sparse_elimination_program_solves_the_jacobian"""
    net, _ = M.make_net(key)
    n = net.n_bus - 1
    lib, h, rc, x = M.host_open(key, M.B_POOL, dict(nr_solver="sparse", sp_lanes=2))
    assert rc == 0, x
    try:
        dims, ops, order, slots = M.sparse_program(lib, h, n, S)
        assert sorted(order.tolist()) == list(range(n))
        pos_bus = M.positions(lib, h, net)
    finally:
        lib.mapdn_destroy(h)
    assert dims[0] == 2 * n + dims[5] + 1 and dims[3] == -(-n // S)
    rng = np.random.default_rng(S + n)
    v = (1.0 + 0.05 * rng.standard_normal(net.n_bus)) * np.exp(1j * 0.05 * rng.standard_normal(net.n_bus))
    J = M.program_jacobian(net, pos_bus, v)
    b = rng.standard_normal(2 * n)
    xs = M.emulate_program(n, S, dims, ops, slots, J, b)
    ref = spla.spsolve(sp.csc_matrix(J), b) if n > 1 else np.linalg.solve(J, b)
    assert np.abs(xs - ref).max() < 1e-9 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("key", M.EMULATED)
def test_fill_blocks_are_the_slots_the_jacobian_does_not_have(key):
    """k_nr_sparse zeroes the fill blocks before every assembly (fill_slots, padded to a multiple of S with the scratch slot; the list
    itself is not exported): for every S the slots cover every structural block once, and exactly n_fill of them belong to blocks the
    Jacobian does not have"""
    net, _ = M.make_net(key)
    n = net.n_bus - 1
    lib, h, rc, x = M.host_open(key, M.B_POOL, dict(nr_solver="sparse", sp_lanes=2))
    assert rc == 0, x
    try:
        pos_bus = M.positions(lib, h, net)
        J = M.program_jacobian(net, pos_bus, np.full(net.n_bus, 1.0 + 0.1j))
        structural = {(i, j) for i in range(n) for j in range(n) if i != j and J[2 * i:2 * i + 2, 2 * j:2 * j + 2].any()}
        for S in (4, 8, 16, 32):
            dims, ops, order, slots = M.sparse_program(lib, h, n, S)
            slotted = {(int(i), int(j)) for i, j, _ in slots}
            assert structural <= slotted and len(slotted - structural) == dims[1], (key, S)
            assert len({int(s) for _, _, s in slots}) == len(slots) == len(slotted)       # one slot per block
            assert all((j, i) in slotted for i, j in slotted)                            # the pattern is symmetric
    finally:
        lib.mapdn_destroy(h)


# ---- Ybus -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", M.KEYS)
def test_ybus_matches_the_oracle(key):
    net, _ = M.make_net(key)
    pin = dict(nr_solver="dense") if key == "grid16" else None
    lib, h, rc, x = M.host_open(key, 4, pin)
    assert rc == 0, x
    try:
        out = np.zeros((net.n_bus, net.n_bus, 2))
        assert lib.mapdn_get_ybus_dense(h, _lib._p(out, _lib._pd)) == 0
    finally:
        lib.mapdn_destroy(h)
    y = out[..., 0] + 1j * out[..., 1]
    yo = make_ybus(net)[0].toarray()
    assert np.abs(y - yo).max() <= 1e-12 * np.abs(yo).max()
    if M.base_of(key) in M.RADIAL:                                        # the doubled line: one entry holding both admittances
        a, b = int(net.line_from_bus[-1]), int(net.line_to_bus[-1])
        assert {(a, b), (b, a)} == {(int(f), int(t)) for f, t in zip(net.line_from_bus[-2:], net.line_to_bus[-2:])}
        z = (net.line_r_ohm_per_km[-2:] + 1j * net.line_x_ohm_per_km[-2:]) * net.line_length_km[-2:] / (net.bus_vn_kv[0] ** 2 / net.sn_mva)
        assert abs(y[a, b] + (1.0 / z).sum()) <= 1e-12 * abs(y[a, b])
        assert np.count_nonzero(y[a]) == (2 if a in (0, net.n_bus - 1) else 3)


# ---- the pools --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", M.POOLED)
def test_pool_conditions(key):
    """the conditions of tests/meshed_edge_nets.py on every pool, from the oracle only"""
    it, cv = M.pool_conditions(key)
    pl, ql, pv, qs = M.pool(key)
    assert pl.shape[0] == M.B_POOL == 35 and all(M.B_POOL % L for L in M.SP_LANES)
    print(f"\n[meshed edges] {key}: " + "".join(str(i) if c else "F" for i, c in zip(it, cv)))


# ---- the oracle alone on the step() replays --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", list(N.PLANS))
@pytest.mark.parametrize("name", M.STEP_SHAPES + (M.STEP_DOUBLED,))
def test_the_oracle_alone_runs_the_replayed_trajectories(name, plan):
    """element_edge_nets.replay() on the meshed shapes: it asserts, call by call, that no step but the forced one is unsolvable and that
    every reset takes its first draw"""
    n_forced = n_restart = n_frozen = n_reset = 0
    for kind, call, x, os_ in N.replay(name, plan, unsolvable=M.STEP_UNSOLVABLE):
        if kind == "reset":
            n_reset += 1
            continue
        act, expect = x
        for k, r, t, info in expect:
            n_restart += k == "restart"
            n_frozen += k == "frozen"
            n_forced += k == "step" and info["destroy"] == 1.0
    assert n_forced == 1
    if plan == "auto":
        assert n_reset == 1 and n_frozen == 0 and n_restart >= 2 * N.B_WATCH
    else:
        assert n_reset == 2 and n_restart == 0 and n_frozen == N.B_WATCH + 1
