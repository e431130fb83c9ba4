"""Hand-built nets at the edges of k_action_grad's tree sweeps and of its line-loss right-hand side, and their scenario: test
infrastructure of tests/test_action_grad_edges_cpu.py and tests/test_action_grad_edges_gpu.py, independent of the product code
(tests/grad_ref.py knows these names: G.make, G.candidates, G.first_action, G.reference).

Every net is a NetSpec written out from a parent list (bus 0 is the slack; net.line row i - 1 joins parent[i] and i), 12.66 kV, sn_mva 1,
a constant-power load on every non-slack bus, one zone per sgen, no gens, no fused buses:
    pair       2 buses, one sgen on the only node: n = 1, no child, the parent is the slack
    chain40    41 buses in one chain, sgens at depth 1, 20 and 40
    star12     slack - hub - 12 leaves, sgens on the hub and on three leaves
    feeders3   three chains of 2, 5 and 9 buses leaving the slack bus (three trees), an sgen on each and one on the slack bus
    comb10     a trunk of 10 buses with a leaf on each, sgens on every other leaf
    ties       a 12-bus tree and two out-of-service net.line rows (in the middle of the table) that would close loops, a row with
               line_parallel = 2, rows with c_nf_per_km and g_us_per_km (one row with both, on the doubled line)
    case141    the shipped case, as tests/opf_kernel_cases.py makes it
The loads are scaled to a linearised voltage drop (DROP), every sgen is sized from the impedance of its path to the slack so that an
action of 0.8 moves its bus by a few percent and the UNSOLVABLE action has no power-flow solution.  The profiles of the hand-built nets
are tests/gen_nets.flat_profiles (a PV value drawn for every row), and every env starts at a daytime row (tests/opf_kernel_cases.rows_of),
so that sqrt(smax^2 - p^2) is neither 0 nor smax.

The scenario is that of tests/grad_ref.py: reset (here at those rows), one random step, then the candidates {0, random, UNSOLVABLE,
random}; B up to 130."""
import functools

import numpy as np

from mapdn_amd.netspec import NetSpec
from tests import opf_kernel_cases as OK
from tests.element_edge_nets import UNSOLVABLE, row_to_start
from tests.gen_nets import flat_profiles

B_MAX, K_MAX = 130, 4
CASE_ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0, voltage_barrier_type="bowl", seed=0)
VN_KV, SN_MVA = 12.66, 1.0
Q_SWING = 0.025                      # |Z_path| pv_nom of an sgen, p.u.: what an action of 1 moves its bus by, about


def _chain(first, n, root=0):
    """parents of n buses first .. first + n - 1 in a chain hanging off `root`"""
    return [root] + list(range(first, first + n - 1))


PARENTS = dict(
    pair=[-1, 0],
    chain40=[-1] + _chain(1, 40),
    star12=[-1, 0] + [1] * 12,
    feeders3=[-1] + _chain(1, 2) + _chain(3, 5) + _chain(8, 9),
    comb10=[-1] + _chain(1, 10) + list(range(1, 11)),
    ties=[-1, 0, 1, 2, 2, 4, 4, 1, 7, 8, 8, 10],
)
SGENS = dict(pair=[1], chain40=[1, 20, 40], star12=[1, 3, 7, 13], feeders3=[2, 5, 16, 0], comb10=[11, 13, 15, 17, 19], ties=[3, 6, 9, 11])
#           linearised drop at the nominal loads, seed
SHAPE = dict(pair=(0.03, 9401), chain40=(0.075, 9402), star12=(0.04, 9403), feeders3=(0.045, 9404), comb10=(0.05, 9405), ties=(0.04, 9406))
SWING = dict(pair=0.06)              # (one line: Newton's flat start still finds the high-voltage solution of a smaller injection)
TIES_OUT = ((3, 6, 4), (5, 11, 9))   # (from, to, row of net.line) of the out-of-service rows of `ties`
TIES_PARALLEL_ROW = 2
HAND_BUILT = tuple(PARENTS)
NETS = HAND_BUILT + ("case141",)


def depth_and_children(parent):
    """(depth of every bus below the slack, children lists) of a parent list"""
    nb = len(parent)
    kids = [[] for _ in range(nb)]
    depth = [0] * nb
    for i in range(1, nb):
        kids[parent[i]].append(i)
        depth[i] = depth[parent[i]] + 1
    return depth, kids


def _build(name):
    parent, sgen_bus = PARENTS[name], np.array(SGENS[name], np.int32)
    drop_target, seed = SHAPE[name]
    rng = np.random.default_rng(seed)
    nb = len(parent)
    nl = nb - 1
    f, t = np.array(parent[1:], np.int32), np.arange(1, nb, dtype=np.int32)
    r = rng.uniform(0.3, 0.7, nl)
    x = r * rng.uniform(0.5, 1.0, nl)
    length = rng.uniform(0.5, 1.5, nl)
    c_nf, g_us, par, ins = np.zeros(nl), np.zeros(nl), np.ones(nl, np.int32), np.ones(nl, np.uint8)
    if name == "ties":
        c_nf[[0, 2, 5, 7]] = [12.0, 9.0, 15.0, 7.0]
        g_us[[1, 2, 8]] = [4.0, 2.5, 6.0]                         # row 2: charging, conductance and two parallel lines
        par[TIES_PARALLEL_ROW] = 2
    # loads on every non-slack bus, scaled to the linearised (DistFlow) drop
    w = rng.uniform(0.5, 1.5, nl)
    zbase = VN_KV ** 2 / SN_MVA
    r_pu, x_pu = r * length / par / zbase, x * length / par / zbase
    tan = np.tan(np.arccos(0.95))
    down = np.concatenate([[0.0], w])
    for i in range(nb - 1, 0, -1):
        down[parent[i]] += down[i]
    drop, zpath = np.zeros(nb), np.zeros(nb)
    for i in range(1, nb):                                        # (parent[i] < i)
        drop[i] = drop[parent[i]] + (r_pu[i - 1] + x_pu[i - 1] * tan) * down[i]
        zpath[i] = zpath[parent[i]] + np.hypot(r_pu[i - 1], x_pu[i - 1])
    p_nom = w * drop_target / drop.max() * SN_MVA
    swing = SWING.get(name, Q_SWING)
    pv_nom = np.array([swing / zpath[b] if b else 0.0 for b in sgen_bus])
    pv_nom[pv_nom == 0.0] = pv_nom[pv_nom > 0.0].mean()          # the sgen on the slack bus
    zone = np.zeros(nb, np.int32)
    zone[1:] = 1 + (np.arange(nl) % len(sgen_bus))
    zone[sgen_bus] = 1 + np.arange(len(sgen_bus))
    if name == "ties":                                            # the out-of-service rows, in the middle of the table
        for a, b, row in TIES_OUT:
            f, t = np.insert(f, row, a), np.insert(t, row, b)
            r, x, length = np.insert(r, row, 0.4), np.insert(x, row, 0.3), np.insert(length, row, 0.8)
            c_nf, g_us = np.insert(c_nf, row, 10.0), np.insert(g_us, row, 3.0)
            par, ins = np.insert(par, row, 1), np.insert(ins, row, 0)
    net = NetSpec(name=name, bus_vn_kv=np.full(nb, VN_KV), bus_zone=zone, line_from_bus=f, line_to_bus=t, line_r_ohm_per_km=r,
                  line_x_ohm_per_km=x, line_c_nf_per_km=c_nf, line_g_us_per_km=g_us, line_length_km=length, line_parallel=par,
                  line_in_service=ins, load_bus=np.arange(1, nb, dtype=np.int32), sgen_bus=sgen_bus,
                  sgen_zone=1 + np.arange(len(sgen_bus), dtype=np.int32), ext_grid_bus=0, ext_grid_vm_pu=1.0, sn_mva=SN_MVA, f_hz=50.0)
    return net, flat_profiles(net, p_nom, p_nom * tan, pv_nom, seed=seed)


@functools.lru_cache(maxsize=None)
def make(name):
    """(NetSpec, Profiles, base env args); cached, read-only"""
    if name == "case141":
        return (*OK.make(name), CASE_ARGS)
    return (*_build(name), CASE_ARGS)


def ties_without_the_open_rows():
    """`ties` with its out-of-service net.line rows deleted: the same electrical net, two rows fewer in the mean of the line losses"""
    import dataclasses
    net = make("ties")[0]
    keep = net.line_in_service.astype(bool)
    cols = {k: getattr(net, k)[keep] for k in ("line_from_bus", "line_to_bus", "line_r_ohm_per_km", "line_x_ohm_per_km", "line_c_nf_per_km",
                                               "line_g_us_per_km", "line_length_km", "line_parallel", "line_in_service")}
    return dataclasses.replace(net, **cols)


# ---- the scenario ---------------------------------------------------------------------------------------------------------------------------
def start_rows(name, B):
    """[B] daytime table rows, another one per env id"""
    return OK.rows_of(make(name)[1], B)


def start_of(name, e):
    """(day, hour, interval) of env id e, for the oracle's reset(start=...)"""
    prof = make(name)[1]
    return row_to_start(prof, start_rows(name, e + 1)[e])


def first_action(name, B):
    ns = make(name)[0].n_sgen
    return np.random.default_rng(11 + sum(map(ord, name))).uniform(-0.8, 0.8, (B_MAX, ns))[:B]


def candidates(name, B, K=K_MAX):
    """[B, K, ns] float64: {0, random, UNSOLVABLE, random}[:K] of every env; a smaller B or K is the leading rows of the larger one"""
    ns = make(name)[0].n_sgen
    c = np.random.default_rng(23 + sum(map(ord, name))).uniform(-0.8, 0.8, (B_MAX, K_MAX, ns))
    c[:, 0] = 0.0
    c[:, 2] = UNSOLVABLE
    return np.ascontiguousarray(c[:B, :K])


def ref_envs64(B):
    """tests/opf_kernel_cases.ref_envs and the envs around the 64-env workgroup edges of k_action_grad"""
    return sorted(set(OK.ref_envs(B)) | {e for e in (62, 63, 64, 65, 127, 128, 129) if e < B})
