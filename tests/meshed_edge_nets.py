"""Meshed nets at the edges of the general-topology solvers' elimination programs: test infrastructure of
tests/test_meshed_edges_cpu.py (solver choice and LDS ladder per shape, the dims that make a shape an edge, the host program executed
in numpy for every S, Ybus, the conditions on the input pools) and tests/test_meshed_edges_gpu.py (k_nr_sparse at every sp_lanes that
fits, k_nr_dense, and k_nr_tree on the doubled-line feeders, against the oracle; position invariance; step()).

    key          graph                                        reaches
    tri3         3-bus triangle                               7 phases and 3 assembly entries per sub-lane: both prefetch rings (8 deep)
                                                              are deeper than the work; n = 2 < S for every S
    pair2x       2 buses, one line listed as (0, 1) and as    radial (the CSR merges the pair): k_nr_tree by default; pinned sparse
                 (1, 0)                                       2 phases, 2 entries, n = 1; pinned dense 2 real rows of 16
    tail2x       4-bus chain, the last line doubled           the doubled line away from the slack, on all three solvers
    k9           complete graph, 9 buses                      n = 8 = S at sp_lanes 8; every block present, max_nnz = 9, no fill
    ring33       one 32-bus loop fed by the slack through     n = 32 = S at sp_lanes 2; one fill pair per step, a long and empty program
                 one line (33 buses)                          (with the slack ON the loop the unknowns form a chain, which never fills)
    wheel_rim    hub + 24-bus rim, slack on the rim           one 25-entry row among 4-entry rows (rows are padded to max_nnz)
    wheel_hub    the same, slack at the hub                   every row has a slack column, max_nnz 4, 42 fill blocks
    grid6        6 x 6 lattice, slack in a corner             n = 35 ragged for every S, fill-heavy, refused at sp_lanes 16
    grid8        8 x 8 lattice, slack inside                  fits at sp_lanes 4 and 2 only; dense N = 128, the last LDS-resident size
    ladder65     32-rung ladder + 1 bus closing a triangle    n = 64: full last rows for every S; refused at sp_lanes 16
    ladder66     ladder65 + 1 bus closing another triangle    n = 65: dense N = 144, the first Jacobian in global memory; ragged last row
    grid10       10 x 10 lattice                              fits at sp_lanes 2 only (host checks and solve() only)
    grid16       16 x 16 lattice                              refused by the sparse solver, accepted by the dense one (host only)
Variants (suffixes, as tests/kernel_matrix.py): "_zip" = with_zip(net, 0.3, 0.2) on wheel_rim and grid6, "_hv" = hv_front(net, 150.0)
on k9 and grid6 (the DC-angle start; two more buses in front of the slack); a variant keeps its shape's graph, loads and sgens and has
an impedance scale of its own (VARIANT_Z).

mesh() is test_topology_stress.feeder() for a graph: a load on every non-slack bus, 1-4 sgens, line_c_nf_per_km > 0, seeded line data
in feeder()'s ranges — times a per-shape impedance scale, because with feeder()'s own ohms these small nets are so stiff that every
power flow takes 2-3 iterations whatever the load.

The input pool of a shape: B = 35 envs (ragged for every sp_lanes; the last workgroup is part padding at 16, 8 and 4), seeded profile
rows and reactive set-points, the load rows of env e times LOAD_SCALES[e] (x the shape's load gain) so that the envs sharing one
wavefront leave the Newton loop at different iterations and some never do.  What a pool must hold, by the oracle alone
(pool_conditions(), asserted in tests/test_meshed_edges_cpu.py; a shape that misses one gets other line data or gains, never another bar):
  * over envs 0-15 the iteration counts of the converged envs take at least three distinct values;
  * at least one env of 0-15 does not converge (10 iterations), and env B - 1 does not either;
  * each of the pairs {0, 1} and {2, 3} (one wavefront's envs at sp_lanes 2) holds two different verdicts or counts;
  * at least half the pool converges;
  * every converged env: the oracle agrees to 1e-10 p.u. with an independent dense Newton iteration in rectangular coordinates
    (dense_newton()), and its residual_inf is below 1e-8 / sn_mva."""
import ctypes as C
import functools
import zlib

import numpy as np

from mapdn_amd import _lib
from mapdn_amd.netspec import NetSpec, synth_profiles
from oracle.pp_restated import bus_demand, dc_angles, make_sbus, make_ybus, residual_inf, runpp_restated
from tests.dc_nets import dc_oracle, hv_front
from tests.edge_rule import same_newton_count
from tests.zip_nets import with_zip, zip_bus_coeffs, zip_oracle, zip_residual_inf

ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0, voltage_barrier_type="bowl", seed=0)
DAYS = 4
ZIP_FRACTIONS = (0.3, 0.2)
HV_SHIFT_DEG = 150.0
B_POOL = 35
SP_LANES = (16, 8, 4, 2)
CU_LDS = 160 * 1024
LDS_REFUSAL = "sp_lanes (MAPDN_SP_LANES): does not fit in LDS"
FILL_REFUSAL = "Jacobian blocks after fill"
E_INVALID, E_TOPOLOGY = -1, -2


# ---- graphs -----------------------------------------------------------------------------------------------------------------------
def ring(n):
    return [(i, (i + 1) % n) for i in range(n)]


def complete(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def wheel(rim):
    """hub = bus 0, rim = buses 1 .. rim"""
    return [(0, i) for i in range(1, rim + 1)] + [(i, i % rim + 1) for i in range(1, rim + 1)]


def grid(r, c):
    return [(i * c + j, i * c + j + 1) for i in range(r) for j in range(c - 1)] + [(i * c + j, (i + 1) * c + j) for i in range(r - 1) for j in range(c)]


def ladder(k):
    """k rungs (2 i, 2 i + 1) joined by two rails"""
    return [(2 * i, 2 * i + 1) for i in range(k)] + [(2 * i, 2 * i + 2) for i in range(k - 1)] + [(2 * i + 1, 2 * i + 3) for i in range(k - 1)]


# ---- the builder ------------------------------------------------------------------------------------------------------------------
def mesh(name, n_bus, edges, slack, seed, n_sgen=3, z_scale=1.0, p_total=4.0, vn_kv=12.47, sn_mva=10.0):
    """NetSpec + Profiles of the graph `edges` on buses 0 .. n_bus - 1 (an edge listed twice is two line rows): a load on every
    non-slack bus, n_sgen sgens on seeded buses (one zone each, the other buses dealt round the zones), line data in the ranges of
    test_topology_stress.feeder() with r and x times z_scale, DAYS days of synth_profiles"""
    rng = np.random.default_rng(seed)
    f = np.array([a for a, _ in edges])
    t = np.array([b for _, b in edges])
    swap = rng.random(len(edges)) < 0.4                                   # (an edge listed twice keeps its two directions)
    twice = np.array([edges.count((a, b)) + edges.count((b, a)) > 1 for a, b in edges])
    swap &= ~twice
    f, t = np.where(swap, t, f), np.where(swap, f, t)
    nl_ = len(edges)
    others = np.array([b for b in range(n_bus) if b != slack])
    w = rng.uniform(0.5, 1.5, n_bus - 1)
    p_nom = p_total * w / w.sum()
    ns = min(n_sgen, n_bus - 1)
    sgen_bus = rng.choice(others, size=ns, replace=False).astype(np.int32)
    zone = np.zeros(n_bus, np.int32)
    zone[others] = 1 + (np.arange(n_bus - 1) % ns)
    for j, b in enumerate(sgen_bus):
        zone[b] = j + 1
    net = NetSpec(name=name, bus_vn_kv=np.full(n_bus, vn_kv), bus_zone=zone, line_from_bus=f, line_to_bus=t,
                  line_r_ohm_per_km=rng.uniform(0.1, 0.4, nl_) * z_scale, line_x_ohm_per_km=rng.uniform(0.05, 0.3, nl_) * z_scale,
                  line_c_nf_per_km=rng.uniform(5.0, 15.0, nl_), line_g_us_per_km=np.zeros(nl_), line_length_km=rng.uniform(0.2, 0.8, nl_),
                  line_parallel=np.ones(nl_, np.int32), line_in_service=np.ones(nl_, np.uint8), load_bus=others.astype(np.int32),
                  sgen_bus=sgen_bus, sgen_zone=(np.arange(ns) + 1).astype(np.int32), ext_grid_bus=int(slack), ext_grid_vm_pu=1.01,
                  sn_mva=sn_mva, f_hz=50.0)
    prof = synth_profiles(p_nom, p_nom * 0.33, np.full(ns, 0.8 * p_total / ns), days=DAYS, seed=seed)
    return net, prof


_LADDER65 = ladder(32) + [(63, 64), (64, 62)]
# key: (n_bus, edges, slack, seed, n_sgen, impedance scale, total nominal load MW, load gain of the pool)
SHAPES = {
    "tri3": (3, ring(3), 0, 31, 2, 4.0, 2.0, 10.0),
    "pair2x": (2, [(0, 1), (1, 0)], 0, 32, 1, 5.0, 1.5, 10.0),
    "tail2x": (4, [(0, 1), (1, 2), (2, 3), (3, 2)], 0, 33, 2, 2.0, 2.0, 6.0),
    "k9": (9, complete(9), 0, 34, 3, 2.0, 4.0, 15.0),
    "ring33": (33, [(0, 1)] + [(a + 1, b + 1) for a, b in ring(32)], 0, 35, 4, 0.2, 4.0, 6.0),
    "wheel_rim": (25, wheel(24), 5, 36, 3, 1.5, 4.0, 10.0),
    "wheel_hub": (25, wheel(24), 0, 37, 3, 2.0, 4.0, 15.0),
    "grid6": (36, grid(6, 6), 0, 38, 4, 0.6, 4.0, 10.0),
    "grid8": (64, grid(8, 8), 27, 39, 4, 1.0, 4.0, 15.0),
    "ladder65": (65, _LADDER65, 0, 40, 4, 0.1, 4.0, 15.0),
    "ladder66": (66, _LADDER65 + [(64, 65), (65, 63)], 0, 41, 4, 0.1, 4.0, 15.0),
    "grid10": (100, grid(10, 10), 0, 42, 4, 0.6, 4.0, 10.0),
    "grid16": (256, grid(16, 16), 0, 43, 4, 0.3, 4.0, 10.0),
}
VARIANTS = ("wheel_rim_zip", "grid6_zip", "k9_hv", "grid6_hv")
# the variants' own impedance scales (the graph, loads and sgens of the shape; stiffer lines): the ZIP iteration has no load derivative
# in its Jacobian and converges linearly, so its last iterate sits just under the tolerance of 1e-9 p.u. and |J^-1| x 1e-9 from the
# fixed point — the impedances must be small enough for that to stay below NEWTON_AGREEMENT; hv_front adds a transformer to every path
VARIANT_Z = {"wheel_rim_zip": 0.5, "grid6_zip": 0.1, "k9_hv": 1.0, "grid6_hv": 0.2}
HOST_ONLY = ("grid16",)                                       # no pool, no solve
SOLVE_ONLY = ("grid10",)                                      # solve() at sp_lanes 2 and dense, 8 oracle envs
EMULATED = tuple(k for k in SHAPES if k not in ("grid10", "grid16"))     # every shape up to grid8 and both ladders
KEYS = tuple(SHAPES) + VARIANTS
POOLED = tuple(k for k in KEYS if k not in HOST_ONLY)
STEP_SHAPES = ("tri3", "wheel_rim", "grid6")
STEP_DOUBLED = "tail2x"                                       # step() also here: res_line / the line-loss term with two rows on one bus pair
STEP_UNSOLVABLE = -600.0      # the forced action of element_edge_nets.replay here: these stiffer nets ride through +60 (the voltage rises), not through sgens that absorb


def base_of(key):
    return key.replace("_hv", "").replace("_zip", "")


def variant_of(key):
    """(DC start, ZIP loads) of a key"""
    return int(key.endswith("_hv")), int(key.endswith("_zip"))


@functools.lru_cache(maxsize=None)
def make_net(key):
    """(NetSpec, Profiles) of a key; cached, so treat both as read-only"""
    n_bus, edges, slack, seed, ns, zs, p_total, _ = SHAPES[base_of(key)]
    zs = VARIANT_Z.get(key, zs)
    net, prof = mesh(base_of(key), n_bus, edges, slack, seed, ns, zs, p_total)
    dc, zip_ = variant_of(key)
    if dc:
        net = hv_front(net, HV_SHIFT_DEG)
    if zip_:
        net = with_zip(net, *ZIP_FRACTIONS)
    return net, prof


def tuning_for(net, tuning):
    """the tuning VoltageControlBatch passes for this net (nr_init = "dc" on the hv_front nets)"""
    t = dict(tuning or {})
    if net.va_init == "dc":
        t.setdefault("nr_init", "dc")
    return t


# ---- what the host must report per shape --------------------------------------------------------------------------------------------
# sp_lanes at which k_nr_sparse does NOT fit the 160 KB of a CU (topological: the blocks after fill), by unvaried shape
LDS_REFUSED = {"tri3": (), "pair2x": (), "tail2x": (), "k9": (), "ring33": (), "wheel_rim": (), "wheel_hub": (), "grid6": (16,),
               "grid8": (16, 8), "ladder65": (16,), "ladder66": (16,), "grid10": (16, 8, 4), "grid16": (16, 8, 4, 2)}
RADIAL = ("pair2x", "tail2x")                                 # the doubled line is one branch of a tree: k_nr_tree by default
PINS = (None,) + tuple(dict(nr_solver="sparse", sp_lanes=L) for L in SP_LANES) + (dict(nr_solver="dense"),)


def sparse_lds_bytes(n, n_blocks, L):
    """k_nr_sparse's dynamic LDS: [n + 2] voltages and [n_blocks] 2x2 blocks of L envs, 16 bytes a pair, + 640 doubles of epilogue"""
    return ((n + 2) * L + n_blocks * 2 * L) * 16 + 10 * 64 * 8


def dense_order(n):
    return (2 * n + 15) // 16 * 16


def dense_lds_bytes(n, N, W, ga):
    """k_nr_dense's dynamic LDS: A[N][N + 2] (LDS-resident Jacobian only) | rhs[N] | dinv[2 N] | V[n + 2] pairs | 10 doubles a thread"""
    return 8 * ((0 if ga else N * (N + 2)) + 3 * N + 2 * (n + 2) + 10 * 64 * W)


# lds_bytes of the automatic k_nr_tree<1, 16, true, true, 1> handle of the doubled-line feeders (B = B_POOL)
TREE_LDS_BYTES = {"pair2x": 10336, "tail2x": 13168}


def host_open(key, B=B_POOL, tuning=None):
    """(lib, handle, 0, keep) of a host-only handle (device = -1), or (lib, None, error code, message)"""
    net, _ = make_net(key)
    lib = _lib.load()
    cn, keep = _lib.make_cnetspec(net)
    cc = _lib.make_cconfig(ARGS, 0, tuning_for(net, tuning))
    h = C.c_void_p()
    rc = lib.mapdn_create(C.byref(cn), C.byref(cc), int(B), -1, C.byref(h))
    if rc:
        return lib, None, rc, lib.mapdn_last_error(None).decode()
    return lib, h, 0, keep


def host_report(key, tuning=None, B=B_POOL):
    """dict(rc, error | is_radial, kernel (dict of _lib.nr_kernel), lds_bytes) of a host-only handle"""
    lib, h, rc, x = host_open(key, B, tuning)
    if rc:
        return dict(rc=rc, error=x)
    try:
        d = _lib.CDims()
        assert lib.mapdn_dims(h, C.byref(d)) == 0
        return dict(rc=0, is_radial=int(d.is_radial), kernel=_lib.nr_kernel(h), lds_bytes=_lib.nr_geometry(h)["lds_bytes"])
    finally:
        lib.mapdn_destroy(h)


def sparse_program(lib, h, n, S):
    """(dims [n_blocks, n_fill, n_phases, rows_per_sub, max_nnz, n_slots], ops [n_phases, S, 4], order [n], slots_ij [n_slots, 3])"""
    dims = np.zeros(6, np.int32)
    assert lib.mapdn_get_sparse_program(h, S, _lib._p(dims, _lib._pi), None, None, None) == 0
    ops = np.zeros(dims[2] * S * 4, np.int32)
    order = np.zeros(n, np.int32)
    sl = np.zeros(3 * dims[5], np.int32)
    assert lib.mapdn_get_sparse_program(h, S, _lib._p(dims, _lib._pi), _lib._p(ops, _lib._pi), _lib._p(order, _lib._pi), _lib._p(sl, _lib._pi)) == 0
    return dims, ops.reshape(dims[2], S, 4), order, sl.reshape(-1, 3)


def program_dims(key, S, tuning=None):
    lib, h, rc, x = host_open(key, B_POOL, tuning)
    assert rc == 0, x
    try:
        dims = np.zeros(6, np.int32)
        assert lib.mapdn_get_sparse_program(h, S, _lib._p(dims, _lib._pi), None, None, None) == 0
        return dict(zip(("blocks", "fill", "phases", "rows_per_sub", "max_nnz", "slots"), (int(v) for v in dims)))
    finally:
        lib.mapdn_destroy(h)


# ---- the host program in numpy (moved here from tests/test_general_topology.py) ------------------------------------------------------
def positions(lib, h, net):
    """bus id of every position (position n = slack): meshed plans use ascending bus ids, radial ones export it"""
    n = net.n_bus - 1
    dims = _lib.CDims()
    assert lib.mapdn_dims(h, C.byref(dims)) == 0
    if dims.is_radial:
        fac = np.zeros((n, 12)); bop = np.zeros(n + 1, np.int32)
        assert lib.mapdn_get_flat_factors(h, _lib._p(fac, _lib._pd), _lib._p(bop, _lib._pi)) == 0
        return bop.tolist()
    return [b for b in range(net.n_bus) if b != net.ext_grid_bus] + [int(net.ext_grid_bus)]


def emulate_program(n, S, dims, ops, slots_ij, J, b):
    """execute the host-compiled elimination program in numpy: blocks B[slot] (2x2), rhs as [b | 0] blocks.  Checks on the way: every
    structural block has a slot, the phase hints are wave-uniform and true, one write per block per phase, at most S real operations a
    phase, every no-op record names the scratch slot (the last block)"""
    nblk, nph = dims[0], dims[2]
    scratch = nblk - 1
    B = np.zeros((nblk, 2, 2))
    for i in range(n):
        B[i] = J[2 * i:2 * i + 2, 2 * i:2 * i + 2]
        B[n + i][:, 0] = b[2 * i:2 * i + 2]
    covered = np.zeros((n, n), bool)
    for i, j, s in np.asarray(slots_ij).reshape(-1, 3):
        B[s] = J[2 * i:2 * i + 2, 2 * j:2 * j + 2]
        covered[i, j] = True
        assert 2 * n <= s < scratch
    for i in range(n):
        for j in range(n):
            if i != j and not covered[i, j]:
                assert not J[2 * i:2 * i + 2, 2 * j:2 * j + 2].any()      # every structural block has a slot
    ops = np.asarray(ops).reshape(nph, S, 4)
    assert ops[..., 1:].min() >= 0 and ops[..., 1:].max() < nblk
    for p in range(nph):
        rd = [(B[a].copy(), B[bb].copy(), B[c].copy()) for (t, c, a, bb) in ops[p]]          # all lanes read, then all write
        writes = set()
        hints = {int(t) >> 8 for (t, c, a, bb) in ops[p]}
        assert len(hints) == 1                                        # the phase hints are wave-uniform
        kinds = {int(t) & 255 for (t, c, a, bb) in ops[p]}
        assert ((1 in kinds) == bool(next(iter(hints)) & 1)) and ((3 in kinds) == bool(next(iter(hints)) & 2))
        assert kinds <= {0, 1, 2, 3} and kinds != {0}, "an empty phase"
        n_real = 0
        for (t, c, a, bb), (Aa, Bb, Cc) in zip(ops[p], rd):
            t = int(t) & 255
            if t == 0:
                assert (c, a, bb) == (scratch, scratch, scratch), "a no-op record off the scratch slot"
                continue
            n_real += 1
            assert c != scratch and a != scratch and bb != scratch
            assert c not in writes, "two writes of one block in a phase"
            writes.add(c)
            B[c] = np.linalg.inv(Aa) if t == 1 else (Aa @ Bb if t == 2 else Cc - Aa @ Bb)
        assert n_real >= 1                                           # (at most S by the record layout: a phase IS S records)
    return np.concatenate([B[n + i][:, 0] for i in range(n)])


def program_jacobian(net, pos_bus, v):
    """the oracle's Jacobian at v over the non-slack buses in position order, in the kernel's unknowns: columns (theta_k, d|V_k| / |V_k|)
    and rows (P_k, Q_k) interleaved per node"""
    from oracle.pp_restated import jacobian
    n = net.n_bus - 1
    pq = np.array(pos_bus[:n])
    Jpp = jacobian(make_ybus(net)[0], v, pq, pq).toarray()            # [[dP/dth, dP/dVm], [dQ/dth, dQ/dVm]] over pq in position order
    Jpp[:, n:] *= np.abs(v[pq])[None, :]                              # scaled unknowns d|V|/|V|
    perm = np.ravel(np.column_stack([np.arange(n), n + np.arange(n)]))
    return Jpp[np.ix_(perm, perm)]


# ---- the input pools ----------------------------------------------------------------------------------------------------------------
# load scale of env e (times the shape's gain): light, heavy and hopeless envs side by side in every wavefront; the pairs (0, 1), (2, 3)
# differ; env B - 1 is hopeless
LOAD_SCALES = np.array([0.02, 12.0, 1.0, 200.0, 4.0, 0.3, 25.0, 1.0, 60.0, 2.0, 8.0, 0.1, 16.0, 1.0, 120.0, 0.5,
                        3.0, 6.0, 0.05, 10.0, 1.0, 150.0, 2.0, 20.0, 0.7, 5.0, 1.0, 80.0, 14.0, 0.2, 9.0, 1.0, 30.0, 2.5, 200.0])
assert LOAD_SCALES.shape == (B_POOL,)
FAILING_ENV = B_POOL - 1
# the variants' own gains: hv_front puts a transformer and a 110 kV line in front of the net, ZIP loads shed power as the voltage sags
POOL_GAIN = {"k9_hv": 1.5, "grid6_hv": 2.0, "wheel_rim_zip": 20.0, "grid6_zip": 20.0}
NEWTON_AGREEMENT = 1e-10                                      # |V oracle - V dense Newton| of every converged env of every pool, p.u.


@functools.lru_cache(maxsize=None)
def pool(key):
    """(p_load, q_load, p_sgen, q_sgen) [B_POOL, .] of a key: seeded profile rows, the load rows scaled per env"""
    net, prof = make_net(key)
    gain = POOL_GAIN.get(key, SHAPES[base_of(key)][7])
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    rows = rng.integers(0, prof.n_rows, B_POOL)
    pv = prof.pv[rows]
    qs = rng.uniform(-0.8, 0.8, (B_POOL, net.n_sgen)) * np.sqrt(np.maximum(prof.s_max() ** 2 - pv ** 2, 0.0))
    sc = (LOAD_SCALES * gain)[:, None]
    return prof.load_p[rows] * sc, prof.load_q[rows] * sc, pv, qs


@functools.lru_cache(maxsize=None)
def oracle(key, e):
    """(result, agreement rule of the iteration count) of env e of the pool, by the oracle of the key's variant"""
    net, _ = make_net(key)
    ins = [x[e] for x in pool(key)]
    dc, zip_ = variant_of(key)
    if zip_:
        return zip_oracle(net, *ins)
    if dc:
        return dc_oracle(net, *ins)
    r = runpp_restated(net, *ins)
    return r, lambda it, conv: same_newton_count(net, ins, it, conv, r)


def oracle_residual(key, e, v):
    """||mismatch||inf (p.u.) of voltages v at the inputs of env e, by the fixed point of the key's variant"""
    net, _ = make_net(key)
    ins = [x[e] for x in pool(key)]
    return zip_residual_inf(net, v, *ins) if variant_of(key)[1] else residual_inf(net, v, *ins)


def dense_newton(net, p_load, q_load, p_sgen, q_sgen, v0=None, n_it=30):
    """an independent Newton iteration in rectangular coordinates on the dense Ybus (numpy.linalg.solve), from v0 (default: the flat
    start); constant-power loads, or the ZIP rule of tests/zip_nets.py on a net with voltage-dependent loads (then with the load
    derivative in the Jacobian, which runpp_zip leaves out: another iteration to the same fixed point).  Returns V"""
    y = make_ybus(net)[0].toarray()
    sb0 = make_sbus(net, *bus_demand(net, p_load, q_load, p_sgen, q_sgen))
    ci, cz = zip_bus_coeffs(net) if net.has_zip_loads else (np.zeros(net.n_bus), np.zeros(net.n_bus))
    pq = np.array([b for b in range(net.n_bus) if b != net.ext_grid_bus])
    v = np.full(net.n_bus, net.ext_grid_vm_pu, complex) if v0 is None else np.array(v0, complex)
    for _ in range(n_it):
        i_ = y @ v
        vm = np.abs(v)
        sb = sb0 * ((1.0 - (ci + cz)) + ci * vm + cz * vm ** 2)
        mis = (v * np.conj(i_) - sb)[pq]
        # dS/de = diag(conj(I)) + diag(V) conj(Y),  dS/df = j diag(conj(I)) - j diag(V) conj(Y);  d|V|/de = e / |V|, d|V|/df = f / |V|
        dsb = sb0 * (ci + 2.0 * cz * vm) / vm
        de = np.diag(np.conj(i_)) + np.diag(v) @ np.conj(y) - np.diag(dsb * v.real)
        df = 1j * np.diag(np.conj(i_)) - 1j * np.diag(v) @ np.conj(y) - np.diag(dsb * v.imag)
        J = np.block([[de[np.ix_(pq, pq)].real, df[np.ix_(pq, pq)].real], [de[np.ix_(pq, pq)].imag, df[np.ix_(pq, pq)].imag]])
        dx = np.linalg.solve(J, -np.r_[mis.real, mis.imag])
        v[pq] += dx[:len(pq)] + 1j * dx[len(pq):]
        if np.abs(dx).max() < 1e-14:
            break
    return v


def pool_conditions(key):
    """assert the conditions of the module docstring on the pool of `key`; returns (iterations [B], converged [B])"""
    net, _ = make_net(key)
    res = [oracle(key, e)[0] for e in range(B_POOL)]
    it = np.array([r.iterations for r in res])
    cv = np.array([bool(r.converged) for r in res])
    assert (it[~cv] == 10).all() and (it[cv] <= 10).all()
    head = np.arange(16)
    assert len(set(it[head][cv[head]].tolist())) >= 3, (key, it[head].tolist(), cv[head].tolist())
    assert (~cv[head]).any() and not cv[FAILING_ENV], (key, cv.tolist())
    for a, b in ((0, 1), (2, 3)):
        assert (it[a], cv[a]) != (it[b], cv[b]), (key, a, b, it[a], it[b])
    assert cv.mean() >= 0.5, (key, cv.mean())
    for e in np.flatnonzero(cv):
        ins = [x[e] for x in pool(key)]
        r = res[e]
        assert oracle_residual(key, e, r.V) < 1e-8 / net.sn_mva, (key, e)
        v0 = None
        if net.va_init == "dc":                                          # (from the flat start nothing finds a solution 150 degrees away)
            v0 = np.full(net.n_bus, net.ext_grid_vm_pu, complex) * np.exp(1j * dc_angles(net, bus_demand(net, *ins)[0]))
        gap = float(np.abs(dense_newton(net, *ins, v0=v0) - r.V).max())
        assert gap < NEWTON_AGREEMENT, (key, e, gap)
    return it, cv
