"""Nets at the edges of the sgen table and at feeder size for the kernels that run the sparse program (k_action_grad_sparse,
k_opf_sens_sparse, k_opf_reduce_sparse): what tests/test_sparse_tables_cpu.py and tests/test_sparse_tables_gpu.py
share.  Test infrastructure only, independent of the product code.  tests/opf_sparse_cases.make and tests/grad_sparse_cases.make hand these
keys on to make() here, so that the states, set-points, references, bars and checks of those two modules serve them unchanged.

    key              built from                                              reaches
    ring33_s16       meshed_edge_nets.mesh() on ring33's graph, 16 sgens     ns = DS: the last full single turn of k_opf_reduce_sparse
    ring33_s17       ... 17 sgens                                            its first second turn (column 16), with an odd last pair
    ladder66_s33     mesh() on ladder66's graph (n = 65), 33 sgens           ns > S at sp_lanes 2 in the gradient's read-out; odd
    ladder66_s64     ... 64 sgens                                            OPF_MAX_NS: 32 reassemblies, the widest exports
    ladder66_s65     ... 65 sgens (one on every non-slack bus)               one past it: refused by opf, served by action_gradients
    ladder65_s4      the ladder65 shape as it is (n = 64)                    full last node rows for every S in the kernels' node loops
    special_meshed   opf_kernel_cases._special() + three line rows           a ratio-and-shift transformer on a cycle, a shunt, sgen
                                                                             scalings, a slack sgen, 9 sgens, a dead net.line row
    case141_ties     case141 + the four ties of test_general_topology        n = 140, ns = 22 (two on one bus)
(the two feeders with SMALL_SGENS of their sgens at SMALL_PV of their PV table: below)

The mesh() nets keep the graph, seed, impedance scale and total load of their shape; the load scale of the loop states (LOOP_SCALE) is
chosen here so that the reference alone meets the conditions of tests/test_sparse_tables_cpu.py.  Tune the data,
never a bar: the rule of tests/meshed_edge_nets.py."""
import ctypes as C
import dataclasses
import functools

import numpy as np

from mapdn_amd import _lib
from mapdn_amd.netspec import add_lines, make_case
from tests import meshed_edge_nets as M
from tests import opf_kernel_cases as K

DS = 16                                          # sub-lanes of an env in k_opf_reduce_sparse (ctlloop.hpp)
OPF_MAX_NS = 64
CASE_ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0, voltage_barrier_type="bowl", seed=0)
CASE_DAYS = 3
# key: (shape of meshed_edge_nets.SHAPES: its graph, slack, seed, impedance scale and total load; sgens)
MESH = {"ring33_s16": ("ring33", 16), "ring33_s17": ("ring33", 17), "ladder66_s33": ("ladder66", 33), "ladder66_s64": ("ladder66", 64),
        "ladder66_s65": ("ladder66", 65)}
KEYS = tuple(MESH) + ("ladder65_s4", "special_meshed", "case141_ties")
OPF_KEYS = tuple(k for k in KEYS if k != "ladder66_s65")
MANY_SGENS = ("ring33_s17", "ladder66_s33", "ladder66_s64", "ladder66_s65", "case141_ties")     # ns > DS
LOOP_KEYS = ("ring33_s17", "special_meshed", "case141_ties")
KKT_KEY = "ladder66_s64"
BITS_KEYS = ("ring33_s17", "ladder66_s64", "case141_ties")
# The two feeders' PV tables give every sgen an s_max far above what the loss minimum asks of it, so at 03:00 (no PV) every sgen ends
# strictly inside the box.  SMALL_SGENS of them get SMALL_PV times their PV column (small units beside large ones): their s_max is then
# what the minimum asks for and more, and they end on the box on every row.  case141_ties keeps the columns from DS on as they are.
SMALL_PV = 0.02
SMALL_SGENS = {"special_meshed": (0, 3, 6), "case141_ties": (0, 3, 6, 9, 12, 15)}
# the load scale of the loop tests (opf_sparse_cases.scaled), found with tests/opf_ref.py alone (test_reference_meets_the_pool_conditions).
# At scale 1 the mesh() nets end with every sgen inside the box, from 4 on with every sgen on it after 2 iterations
LOOP_SCALE = {"ring33_s17": 3.0, "special_meshed": 1.0, "case141_ties": 1.0, "ladder66_s64": 3.3}
# special_meshed: (from, to, r ohm / km, x ohm / km, c nF / km, km) of (a) the tie that closes a cycle through the transformer: bus 9 is
# the leaf behind the transformer's other bus; (b) a tie between two other branches of the feeder; and the row that is out of service
SPECIAL_TIES = ((0, 9, 0.25, 0.2, 6.0, 0.6), (20, 2, 0.3, 0.2, 0.0, 0.5))
SPECIAL_DEAD = (1, 8, 0.2, 0.1, 4.0, 0.4)
CASE141_TIES = ([5, 40, 77, 100], [77, 120, 130, 12], 0.3, 0.2)                 # tests/test_general_topology._meshed
# the forced action of the UNSOLVABLE column: the stiff mesh() shapes ride through whatever absorbs (meshed_edge_nets.STEP_UNSOLVABLE)
UNSOLVABLE = {k: M.STEP_UNSOLVABLE for k in tuple(MESH) + ("ladder65_s4",)}
UNSOLVABLE.update(special_meshed=-60.0, case141_ties=-60.0)


def special_meshed():
    """(NetSpec, Profiles, (hv, lv) buses of the transformer, index of the dead line row): opf_kernel_cases' special with (a) a tie from
    the ext_grid bus to a leaf below the transformer's lv bus, (b) a tie between two buses on the other side, (c) one more net.line row
    that is out of service"""
    net, prof, hub = K._special()
    hv, lv = int(net.br_from_bus[0]), int(net.br_to_bus[0])
    slack = int(net.ext_grid_bus)
    # the feeder reaches the hub (the lv bus) from the slack; the transformer's other bus and the leaf behind it hang below the hub
    assert (slack, hv, lv) == (0, 12, 19) and lv == hub and SPECIAL_TIES[0][:2] == (slack, 9)
    rows = SPECIAL_TIES + (SPECIAL_DEAD,)
    out = add_lines(net, *([r[i] for r in rows] for i in range(6)))
    alive = np.asarray(out.line_in_service).copy()
    dead = alive.shape[0] - 1
    alive[dead] = 0
    out = dataclasses.replace(out, line_in_service=alive, name="special_meshed")
    return out, prof, (hv, lv), dead


@functools.lru_cache(maxsize=None)
def make(key):
    """(NetSpec, Profiles, base env args); cached: read-only"""
    if key in MESH:
        shape, ns = MESH[key]
        n_bus, edges, slack, seed, _, zs, p_total, _ = M.SHAPES[shape]
        return (*M.mesh(key, n_bus, edges, slack, seed, ns, zs, p_total), M.ARGS)
    if key == "ladder65_s4":
        return (*M.make_net("ladder65"), M.ARGS)
    if key == "special_meshed":
        net, prof = special_meshed()[:2]
    else:
        assert key == "case141_ties", key
        net, prof = make_case("case141", days=CASE_DAYS)
        net = dataclasses.replace(add_lines(net, *CASE141_TIES), name=key)
    gain = np.ones(net.n_sgen)
    gain[list(SMALL_SGENS[key])] = SMALL_PV
    return net, dataclasses.replace(prof, pv=prof.pv * gain), CASE_ARGS


@functools.lru_cache(maxsize=None)
def fits(key):
    """the sp_lanes a host-only handle of the key accepts when pinned to the sparse solver (the handle's own answer; pinned as
    tests/test_sparse_tables_cpu.ACCEPTED)"""
    net, _, args = make(key)
    lib = _lib.load()
    ok = []
    for L in M.SP_LANES:
        cn, keep = _lib.make_cnetspec(net)
        cc = _lib.make_cconfig(args, 0, M.tuning_for(net, dict(nr_solver="sparse", sp_lanes=L)))
        h = C.c_void_p()
        rc = lib.mapdn_create(C.byref(cn), C.byref(cc), 35, -1, C.byref(h))
        if rc == 0:
            assert _lib.nr_kernel(h)["solver"] == 1 and _lib.nr_kernel(h)["L"] == L
            lib.mapdn_destroy(h)
            ok.append(L)
        else:
            assert M.LDS_REFUSAL in lib.mapdn_last_error(None).decode(), (key, L, lib.mapdn_last_error(None))
    return ok


def cycle_through(net, a, b):
    """True when buses a and b stay connected by in-service lines and branches after every direct a - b element is taken out: the
    a - b element lies on a cycle"""
    alive = np.asarray(net.line_in_service).astype(bool)
    edges = [(int(x), int(y)) for x, y, s in zip(net.line_from_bus, net.line_to_bus, alive) if s]
    edges += [(int(x), int(y)) for x, y in zip(net.br_from_bus, net.br_to_bus)]
    edges = [e for e in edges if set(e) != {a, b}]
    seen, todo = {a}, [a]
    while todo:
        u = todo.pop()
        for x, y in edges:
            for p, q in ((x, y), (y, x)):
                if p == u and q not in seen:
                    seen.add(q)
                    todo.append(q)
    return b in seen


def strided_reduce(g, H, ds=DS, slip=None):
    """k_opf_reduce_sparse's column turns restated in numpy: sub-lane sl fills g[j] and H[i][j], i <= j (mirrored), for j = sl, sl + ds,
    ...; returns (g, H) as the turns leave them in arrays that start as 0.  slip = "stride": the later turns step by ds + 1 (columns
    are left unwritten); slip = "turns": one turn only"""
    ns = g.shape[0]
    go, Ho = np.zeros(ns), np.zeros((ns, ns))
    for sl in range(ds):
        j = sl
        while j < ns:
            go[j] = g[j]
            Ho[:j + 1, j] = H[:j + 1, j]
            Ho[j, :j + 1] = H[:j + 1, j]
            if slip == "turns":
                break
            j += ds + (1 if slip == "stride" else 0)
    return go, Ho
