"""The OPF baseline on handles of the sparse solver (mapdn_opf_config.meshed = 1; k_opf_sens_sparse, k_opf_reduce_sparse; DESIGN.md
section 25): what tests/test_opf_sparse_cpu.py and tests/test_opf_sparse_gpu.py share.  Test infrastructure only, independent of the
product code: the references are tests/opf_ref.py (dense, topology-agnostic) and tests/opf_kernel_cases.linearise_ext (the same
definition above float64); the nets are those of tests/meshed_edge_nets.py, crowded_meshed of tests/element_edge_nets.py, and the
shipped case33, pinned to the sparse solver and with five tie lines closed; the keys of tests/sparse_table_cases.py (DESIGN.md section 27:
the edges of the sgen table, feeder size) are handed on to that module's make() and fits().

States: env e stands at profile row rows_of(prof, B)[e] — noon (per_day / 2) and 03:00 (per_day / 8: no PV, the whole s_max is
reactive headroom) of the first two days — with its loads times `scale` (1, or 8: scaled(prof, 8)); s_max = 1.2 x max pv.  The k9_hv net
starts every power flow from the DC angles (runpp init="dc"), in the references too (runpp_of, with_runpp)."""
import contextlib
import ctypes as C
import dataclasses
import functools

import numpy as np

from mapdn_amd import _lib
from mapdn_amd.netspec import case33_meshed, make_case
from oracle.pp_restated import make_ybus
from tests import grad_sparse_cases as GS
from tests import meshed_edge_nets as M
from tests import opf_kernel_cases as K
from tests import opf_ref as R
from tests import sparse_table_cases as ST

B_MAX = 35
BATCHES = (1, 5, 17, 35)                       # a partly filled last workgroup at every sp_lanes
NETS = ("pair2x", "tri3", "tail2x", "k9", "wheel_rim", "grid6", "crowded_meshed", "k9_hv", "case33", "case33_meshed")
LOOP_NETS = ("tri3", "wheel_rim", "grid6", "k9_hv")
CAPPED_NETS = ("tri3", "tail2x", "grid6")       # status 1 (the QP cap) at load scale 8 under CAPPED_BAND
CAPPED_BAND, CAPPED_SCALE = (1.0, 1.012), 8.0
CAPPED_ENV = 4                                  # ... on the 03:00 row of day 0 (tri3 stops with status 0 on the noon rows)
LOOP_SCALE = 8.0                                # the loads of the loop tests on LOOP_NETS (case33_meshed: 1)
ACTIVE_ENV = 0
V_BAND = K.V_BAND
CASE_ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0, voltage_barrier_type="bowl", seed=0)
CASE_DAYS = 3
runpp_of = GS.runpp_of


@functools.lru_cache(maxsize=None)
def make(key):
    """(NetSpec, Profiles, base env args); cached: read-only"""
    if key in ST.KEYS:
        return ST.make(key)
    if key in M.SHAPES:
        return (*M.make_net(key), M.ARGS)
    if key in ("case33", "case33_meshed"):
        net, prof = make_case("case33", days=CASE_DAYS)
        return (case33_meshed(net, 5) if key == "case33_meshed" else net), prof, CASE_ARGS
    return GS.make(key)


def fits(key):
    """the sp_lanes at which k_nr_sparse (so k_opf_sens_sparse) fits the net"""
    if key in ST.KEYS:
        return ST.fits(key)
    if M.base_of(key) in M.SHAPES:
        return [L for L in M.SP_LANES if L not in M.LDS_REFUSED[M.base_of(key)]]
    return list(M.SP_LANES)                     # crowded_meshed (15 nodes), case33 (32 nodes, little fill)


def tuning(key, L=None):
    """the handle's tuning: the sparse solver (pinned: pair2x, tail2x and case33 are radial), sp_lanes = L (None: automatic)"""
    t = dict(nr_solver="sparse")
    if L is not None:
        t["sp_lanes"] = int(L)
    return t


def scaled(prof, scale):
    return prof if scale == 1.0 else dataclasses.replace(prof, load_p=prof.load_p * scale, load_q=prof.load_q * scale)


def rows_of(prof, B):
    per_day = prof.intervals_per_day
    return np.array([(e % 2) * per_day + (per_day // 8 if e % 3 == 1 else per_day // 2) for e in range(B)])


def setpoints(key, B):
    """tests/opf_kernel_cases.setpoints of the largest batch (env 0 all zero, every third env +-1 on some sgens, the last env pinned at
    +-1 everywhere, the rest random); a smaller B is its leading rows with ITS last env pinned everywhere"""
    ns = make(key)[0].n_sgen
    a = K.setpoints(key, B_MAX, ns)[:B].copy()
    if 1 < B < B_MAX:
        a[B - 1] = np.where(np.random.default_rng(B).random(ns) < 0.5, -1.0, 1.0)
    return a


def inputs(key, e, scale=1.0):
    """(load_p, load_q, pv, s_max) of env e"""
    net, prof, _ = make(key)
    t = rows_of(prof, B_MAX)[e]
    return prof.load_p[t] * scale, prof.load_q[t] * scale, prof.pv[t], prof.s_max(1.2)


@contextlib.contextmanager
def with_runpp(key):
    """tests/opf_ref's own power flows (kkt_nonlinear) with the start of the key"""
    keep, R.runpp_restated = R.runpp_restated, runpp_of(key)
    try:
        yield
    finally:
        R.runpp_restated = keep


@functools.lru_cache(maxsize=None)
def reference_run(key, e, scale=1.0, band=V_BAND):
    """tests/opf_ref.opf_ref of env e (the defaults; the band); cached, read-only"""
    net = make(key)[0]
    lp, lq, pv, smax = inputs(key, e, scale)
    return R.opf_ref(net, lp, lq, pv, smax, None, band[0], band[1], runpp=runpp_of(key))


def kkt_of(key, e, a, scale=1.0, band=V_BAND):
    """tests/opf_ref.kkt_nonlinear at a: (stationarity, complementarity, violation)"""
    net = make(key)[0]
    lp, lq, pv, smax = inputs(key, e, scale)
    with with_runpp(key):
        return R.kkt_nonlinear(net, lp, lq, pv, smax, np.asarray(a, np.float64), band[0], band[1])


def oracle_voltage(key, e, a, scale=1.0):
    net = make(key)[0]
    lp, lq, pv, smax = inputs(key, e, scale)
    res = runpp_of(key)(net, lp, lq, pv, R.limits(pv, smax) * a)
    assert res.converged, (key, e)
    return res


def active_rows(key, e, band, scale=1.0, near=1e-6):
    """the voltage rows within `near` of a bound at the reference's returned point"""
    net = make(key)[0]
    r = reference_run(key, e, scale, band)
    vm = np.delete(r.vm_pu, net.ext_grid_bus)
    return int(((band[1] - vm <= near) | (vm - band[0] <= near)).sum())


# bands under which the reference stops with status 0 and a voltage row on its bound (found with the reference alone, on env 0: the noon
# row of day 0; asserted in tests/test_opf_sparse_cpu.py)
ACTIVE_BAND = {"wheel_rim": (0.95, 1.01), "case33_meshed": (0.95, 1.045)}


# ---- the bars (DESIGN.md section 16's rule) -----------------------------------------------------------------------------------------------
def e64(key):
    """the error of the plain float64 dense reference against the extended one at the oracle's V of the reference envs of the largest
    batch, per quantity (tests/opf_kernel_cases.e64 on these states)"""
    net = make(key)[0]
    ybus = make_ybus(net)[0]
    a = setpoints(key, B_MAX)
    per_env = []
    for e in K.ref_envs(B_MAX):
        lp, lq, pv, smax = inputs(key, e)
        lim = R.limits(pv, smax)
        res = oracle_voltage(key, e, a[e])
        L = R.linearise(net, res.V, lim)
        got = dict(S=L.S, g=L.g, H=L.H, loss=R.loss_pu(ybus, res.V), violation=R.violation_of(np.abs(res.V), net, *V_BAND))
        per_env.append(K.errors(net, res.V, lim, got))
    return K.worst(per_env)


# measured on the CPU by e64() (tests/test_opf_sparse_cpu.py recomputes them)
E64 = {
    "pair2x": dict(S=2.19e-16, g=1.39e-13, H=3.76e-16, loss=1.98e-10, violation=0.00e+00),
    "tri3": dict(S=3.88e-16, g=3.52e-13, H=8.21e-16, loss=8.68e-10, violation=0.00e+00),
    "tail2x": dict(S=1.69e-15, g=1.46e-13, H=2.35e-15, loss=3.79e-10, violation=0.00e+00),
    "k9": dict(S=9.47e-16, g=3.99e-12, H=1.18e-15, loss=5.89e-09, violation=0.00e+00),
    "wheel_rim": dict(S=1.50e-15, g=1.59e-12, H=2.65e-15, loss=3.54e-09, violation=0.00e+00),
    "grid6": dict(S=1.25e-14, g=5.27e-12, H=1.00e-14, loss=7.49e-09, violation=0.00e+00),
    "crowded_meshed": dict(S=1.22e-14, g=7.17e-13, H=2.29e-14, loss=5.33e-12, violation=3.48e-15),
    "k9_hv": dict(S=5.98e-14, g=1.47e-10, H=2.41e-13, loss=1.05e-08, violation=0.00e+00),
    "case33": dict(S=1.31e-14, g=4.22e-13, H=2.08e-14, loss=4.55e-12, violation=1.32e-15),
    "case33_meshed": dict(S=5.14e-15, g=1.00e-13, H=9.75e-15, loss=2.48e-12, violation=9.19e-15),
    # tests/sparse_table_cases.py
    "ring33_s16": dict(S=1.53e-14, g=1.32e-11, H=2.41e-14, loss=1.25e-08, violation=0.00e+00),
    "ring33_s17": dict(S=2.22e-14, g=1.11e-11, H=2.69e-14, loss=5.89e-09, violation=0.00e+00),
    "ladder66_s33": dict(S=1.21e-13, g=3.07e-11, H=8.92e-14, loss=1.45e-07, violation=0.00e+00),
    "ladder66_s64": dict(S=1.74e-13, g=3.10e-11, H=1.08e-13, loss=1.64e-07, violation=0.00e+00),
    "ladder65_s4": dict(S=1.36e-13, g=4.73e-11, H=6.32e-14, loss=5.45e-08, violation=0.00e+00),
    "special_meshed": dict(S=2.08e-14, g=1.01e-12, H=1.84e-14, loss=6.62e-12, violation=1.09e-14),
    "case141_ties": dict(S=1.41e-13, g=3.08e-12, H=1.40e-13, loss=4.44e-11, violation=0.00e+00),
}


def bar(key, q):
    return max(K.BAR_FACTOR * E64[key][q], K.BAR_FLOOR)


# ---- host-only handles ------------------------------------------------------------------------------------------------------------------
def host_open(key, tune=None, B=B_MAX, net=None):
    """(lib, handle, 0, keep) of a host-only handle (device = -1) of the key's net (or `net`), or (lib, None, error code, message)"""
    base_net, _, args = make(key)
    net = base_net if net is None else net
    lib = _lib.load()
    cn, keep = _lib.make_cnetspec(net)
    cc = _lib.make_cconfig(args, 0, M.tuning_for(net, tune))
    h = C.c_void_p()
    rc = lib.mapdn_create(C.byref(cn), C.byref(cc), int(B), -1, C.byref(h))
    if rc:
        return lib, None, rc, lib.mapdn_last_error(None).decode()
    return lib, h, 0, keep


def opf_error(key, cfg, tune=None, net=None):
    """(return code, message) of mapdn_opf_actions on a host-only handle: the refusals come before the handle's own"""
    lib, h, rc, keep = host_open(key, tune, net=net)
    assert rc == 0, keep
    try:
        cc = _lib.make_opf_config(cfg)
        one = C.c_void_p(1)
        rc = lib.mapdn_opf_actions(h, C.byref(cc), one, None, one, one, one, one, None)
        return rc, lib.mapdn_last_error(h).decode()
    finally:
        lib.mapdn_destroy(h)


@functools.lru_cache(maxsize=None)
def host_program(key, S):
    """(n, pos_bus, dims, ops, slots_ij) of the key's exported elimination program packed for S sub-lanes"""
    net = make(key)[0]
    lib, h, rc, x = host_open(key, dict(nr_solver="sparse", sp_lanes=64 // S))
    assert rc == 0, x
    try:
        n = net.n_bus - 1
        pos_bus = M.positions(lib, h, net)
        dims, ops, order, slots = M.sparse_program(lib, h, n, S)
        return n, pos_bus, dims, ops, slots
    finally:
        lib.mapdn_destroy(h)


# ---- the host program on the blocks of J itself, two columns a run ------------------------------------------------------------------------
def emulate_pair(n, S, dims, ops, slots_ij, J, b0, b1):
    """tests/meshed_edge_nets.emulate_program with two right-hand sides riding in the two columns of the right-hand-side blocks (its
    checks of the program are not repeated here).  Returns (x0, x1), interleaved per node"""
    nblk, nph = dims[0], dims[2]
    B = np.zeros((nblk, 2, 2))
    for i in range(n):
        B[i] = J[2 * i:2 * i + 2, 2 * i:2 * i + 2]
        B[n + i][:, 0] = b0[2 * i:2 * i + 2]
        B[n + i][:, 1] = b1[2 * i:2 * i + 2]
    for i, j, s in np.asarray(slots_ij).reshape(-1, 3):
        B[s] = J[2 * i:2 * i + 2, 2 * j:2 * j + 2]
    for p in np.asarray(ops).reshape(nph, S, 4):
        rd = [(B[a].copy(), B[bb].copy(), B[c].copy()) for (t, c, a, bb) in p]
        for (t, c, a, bb), (Aa, Bb, Cc) in zip(p, rd):
            t = int(t) & 255
            if t:
                B[c] = np.linalg.inv(Aa) if t == 1 else (Aa @ Bb if t == 2 else Cc - Aa @ Bb)
    return tuple(np.concatenate([B[n + i][:, c] for i in range(n)]) for c in (0, 1))


def columns_by_program(key, S, V, lim, partner=None):
    """S [n_bus, ns] = d|V| / da by the exported program for S sub-lanes on the oracle's Jacobian blocks at V, the columns paired
    (j, j + 1), j even, as the kernel pairs them — or, partner = k: every column j paired with column (j + k) % ns in its slot's other
    half (what a column's result must not depend on)"""
    net = make(key)[0]
    n, pos_bus, dims, ops, slots = host_program(key, S)
    J = M.program_jacobian(net, pos_bus, V)
    ns = net.n_sgen
    w = lim * net.sgen_scaling / net.sn_mva
    node = {int(b): i for i, b in enumerate(pos_bus[:n])}
    rhs = np.zeros((ns, 2 * n))
    for j, b in enumerate(np.asarray(net.sgen_bus)):
        if int(b) in node:
            rhs[j, 2 * node[int(b)] + 1] = w[j]
    X = np.zeros((ns, 2 * n))
    if partner is None:
        for j in range(0, ns, 2):
            x0, x1 = emulate_pair(n, S, dims, ops, slots, J, rhs[j], rhs[j + 1] if j + 1 < ns else np.zeros(2 * n))
            X[j] = x0
            if j + 1 < ns:
                X[j + 1] = x1
    else:
        for j in range(ns):
            X[j] = emulate_pair(n, S, dims, ops, slots, J, rhs[j], rhs[(j + partner) % ns] * 3.0)[0]
    out = np.zeros((net.n_bus, ns))
    out[np.array(pos_bus[:n])] = (X[:, 1::2] * np.abs(V[np.array(pos_bus[:n])])[None, :]).T
    return out
