"""The compiled power-flow kernels and one row per kernel that reaches it: test infrastructure of tests/test_kernel_matrix_cpu.py (every
row's handle reports its kernel, the rows cover the compiled set) and tests/test_kernel_matrix_gpu.py (every row against the oracle).

The compiled set is parsed from the sources, not restated: the k_nr_tree instantiations of csrc/nr_inst_list.hpp (NR_INSTS_*, NR_INSTS_DC_*,
NR_INSTS_ZIP_* and NR_INSTS_GEN_*, the latter two once per start), k_nr_sparse<L, DC> for every L of SP_FOR_EACH (sparse_prog.hpp), and
k_nr_dense<W, GA> for the LDS-resident pair of dense_fn and every W of DENSE_GA_W (dense.hip).  A kernel is a tuple:
    ("tree", W, L, HL, GL, RES, DC, ZIP, GEN)   ("sparse", L, DC, ZIP, GEN)   ("dense", W, GA)
k_nr_sparse decides ZIP and GEN at run time, so its compiled kernel is ("sparse", L, DC) and its rows cover every (L, DC, ZIP) without
generators and every (L, DC) with them (no kernel serves ZIP loads and generators together)."""
import collections
import ctypes as C
import functools
import os
import re
from typing import NamedTuple

import numpy as np

from mapdn_amd import _lib
from mapdn_amd.netspec import _radial_case, case33_meshed, make_case, synth_profiles
from tests.dc_nets import hv_front
from tests.gen_nets import with_gens
from tests.zip_nets import with_zip

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mapdn_amd", "csrc")
ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0, voltage_barrier_type="bowl", seed=0)
ZIP_FRACTIONS = (0.3, 0.2)                                   # (cz, ci) of every ZIP net here


# ---- the compiled set ----------------------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"//[^\n]*", "", f.read())


def _macro(src, name):
    """the body of `#define name(X) ...` (continuation lines joined)"""
    m = re.search(r"#define\s+" + name + r"\(X\)((?:[^\n]*\\\n)*[^\n]*)", src)
    assert m, name
    return m.group(1).replace("\\\n", " ")


def _tree_entries(body):
    out = []
    for args in re.findall(r"X\(([^)]*)\)", body):
        w, l, hl, gl, res = (a.strip() for a in args.split(","))
        out.append((int(w), int(l), int(hl == "true"), int(gl == "true"), int(res)))
    return out


def tree_kernels():
    src = _src("nr_inst_list.hpp")
    parts = sorted(set(re.findall(r"#define\s+NR_INSTS_(\d+)\(X\)", src)))
    assert parts, "no NR_INSTS_<part> in nr_inst_list.hpp"
    out = []
    for p in parts:
        out += [("tree", *e, 0, 0, 0) for e in _tree_entries(_macro(src, f"NR_INSTS_{p}"))]
        out += [("tree", *e, 1, 0, 0) for e in _tree_entries(_macro(src, f"NR_INSTS_DC_{p}"))]
        for e in _tree_entries(_macro(src, f"NR_INSTS_ZIP_{p}")):            # NR_ENTRY_ZIP: the flat and the DC start
            out += [("tree", *e, 0, 1, 0), ("tree", *e, 1, 1, 0)]
        for e in _tree_entries(_macro(src, f"NR_INSTS_GEN_{p}")):            # NR_ENTRY_GEN: the flat and the DC start
            out += [("tree", *e, 0, 0, 1), ("tree", *e, 1, 0, 1)]
    return out


def sparse_kernels():
    lanes = [int(x) for x in re.findall(r"X\((\d+)\)", _macro(_src("sparse_prog.hpp"), "SP_FOR_EACH"))]
    return [("sparse", l, dc) for l in lanes for dc in (0, 1)]


def dense_kernels():
    src = _src("dense.hip")
    m = re.search(r"DENSE_GA_W\[\]\s*=\s*\{([^}]*)\}", src)
    assert m, "DENSE_GA_W"
    ga = [int(x) for x in m.group(1).split(",")]
    body = src[src.index("static const void* dense_fn"):]
    body = body[:body.index("\n}")]
    lds = sorted({int(w) for w in re.findall(r"k_nr_dense<(\d+), false>", body)})
    return [("dense", w, 0) for w in lds] + [("dense", w, 1) for w in ga]


def compiled_kernels():
    """every power-flow kernel instantiation the library holds (a list, so that an entry listed twice in the sources shows)"""
    return tree_kernels() + sparse_kernels() + dense_kernels()


def compiled_of(kernel):
    """the compiled instantiation a row's kernel runs (k_nr_sparse: ZIP and GEN are run-time flags)"""
    return kernel[:3] if kernel[0] == "sparse" else kernel


# ---- nets ----------------------------------------------------------------------------------------------------------------------
# keys: "case33" | "case141" | "case322" | "case33_meshed" | "radial<nb>", then optional suffixes "_hv" (hv_front(..., 150): the DC
# start), "_zip" (with_zip(..., 0.3, 0.2)) and "_gen" (generators at gen_sites of the base net, put on before hv_front).  No row carries
# "_zip" and "_gen" together: mapdn_create refuses such a net (REFUSALS holds the one key that has both)
GEN_VM_PU = (1.00, 1.01, 0.99, 1.00)                         # of the sites, in their order
RADIAL = {61: (5, 8), 81: (9, 8), 113: (9, 8), 177: (9, 8), 241: (9, 8), 385: (9, 8), 481: (9, 8)}   # nb: (trunk buses, zones)


def _radial(nb):
    trunk, zones = RADIAL[nb]
    net, p_nom = _radial_case(f"radial{nb}", nb, (6 * nb) // 10, max(zones, nb // 6), zones, trunk, 12.47, 10.0, 20.0 * nb / 141,
                              nb, 0.05)
    q_nom = p_nom * np.tan(np.arccos(0.95))
    w = np.random.default_rng(nb + 7).uniform(0.7, 1.3, net.n_sgen)
    return net, synth_profiles(p_nom, q_nom, 4.0 * p_nom.sum() * w / w.sum(), days=4, seed=nb)


def bfs_tree(net):
    """(order, parent, depth, children) of the breadth-first tree from the ext_grid bus over the in-service lines, neighbours taken
    in ascending bus order"""
    adj = collections.defaultdict(set)
    for f, t, on in zip(net.line_from_bus, net.line_to_bus, net.line_in_service):
        if on:
            adj[int(f)].add(int(t))
            adj[int(t)].add(int(f))
    root = int(net.ext_grid_bus)
    order, parent, depth, children = [root], {root: -1}, {root: 0}, collections.defaultdict(list)
    for b in order:                                              # (grows while it is read: the queue)
        for c in sorted(adj[b]):
            if c not in parent:
                parent[c], depth[c] = b, depth[b] + 1
                children[b].append(c)
                order.append(c)
    return order, parent, depth, children


def gen_sites(net):
    """where the "_gen" nets carry their generators, by a rule on the tree of the base net (ties: the lowest bus index): (a) the first
    child of the slack bus — Q_gen beside the slack is large and sensitive; (b) the non-slack bus with the most children — the longest
    Ybus row; (c) the deepest leaf; (d) that leaf's parent — two adjacent gens, one of them with a gen child.  Duplicates dropped."""
    order, parent, depth, children = bfs_tree(net)
    root = order[0]
    rest = sorted(order[1:])
    a = children[root][0]
    b = max(rest, key=lambda k: (len(children[k]), -k))
    c = max((k for k in rest if not children[k]), key=lambda k: (depth[k], -k))
    return list(dict.fromkeys([a, b, c, parent[c]]))


def _with_matrix_gens(net, prof, sites):
    p = round(0.05 * float(prof.load_p.mean(0).sum()), 3)
    return with_gens(net, [(b, p, v) for b, v in zip(sites, GEN_VM_PU)])


@functools.lru_cache(maxsize=None)
def make_net(key):
    """(NetSpec, Profiles) of a net key"""
    base = key.replace("_hv", "").replace("_zip", "").replace("_gen", "")
    if base.startswith("radial"):
        net, prof = _radial(int(base[len("radial"):]))
    else:
        net, prof = make_case(base.replace("_meshed", ""))
    sites = gen_sites(net) if "_gen" in key else None            # (case33_meshed: on case33, before the ties close)
    if base == "case33_meshed":
        net = case33_meshed(net, 5)
    if "_gen" in key:
        net = _with_matrix_gens(net, prof, sites)
    if "_hv" in key:
        net = hv_front(net, 150.0)
    if "_zip" in key:
        net = with_zip(net, *ZIP_FRACTIONS)
    return net, prof


def variant_of(key):
    """(DC, ZIP, GEN) of the kernel that serves a net key"""
    dc, zip_, gen = int("_hv" in key), int("_zip" in key), int("_gen" in key)
    assert not (zip_ and gen), f"{key}: no kernel serves ZIP loads and generators together"
    return dc, zip_, gen


def tuning_for(net, tuning):
    """the tuning VoltageControlBatch passes for this net (it sets nr_init = "dc" on nets runpp starts from DC angles)"""
    t = dict(tuning or {})
    if net.va_init == "dc":
        t.setdefault("nr_init", "dc")
    return t


def host_kernel(key, B, tuning=None):
    """(0, kernel dict) of a host-only handle (device = -1) of this row, or (error code, message)"""
    net, _ = make_net(key)
    lib = _lib.load()
    cn, keep = _lib.make_cnetspec(net)
    cc = _lib.make_cconfig(ARGS, 0, tuning_for(net, tuning))
    h = C.c_void_p()
    rc = lib.mapdn_create(C.byref(cn), C.byref(cc), int(B), -1, C.byref(h))
    if rc:
        return rc, lib.mapdn_last_error(None).decode()
    try:
        return 0, _lib.nr_kernel(h)
    finally:
        lib.mapdn_destroy(h)


def kernel_tuple(k):
    """a kernel dict of _lib.nr_kernel as the tuple used here"""
    if k["solver"] == 0:
        return ("tree", k["W"], k["L"], k["HL"], k["GL"], k["RES"], k["DC"], k["ZIP"], k["GEN"])
    if k["solver"] == 1:
        return ("sparse", k["L"], k["DC"], k["ZIP"], k["GEN"])
    return ("dense", k["W"], k["GA"])


# ---- the rows ------------------------------------------------------------------------------------------------------------------
class Row(NamedTuple):
    kernel: tuple
    net: str
    B: int          # ragged (not a multiple of 64); the handle of the row runs `kernel` at this batch size
    tuning: dict


def row_id(r):
    """the test id of a row: net and kernel; a kernel without generators without its GEN field (the ids of before GEN was one)"""
    k = r.kernel if r.kernel[0] == "dense" or r.kernel[-1] else r.kernel[:-1]
    return f"{r.net}-" + "-".join(str(x) for x in k)


def _pin(W, L, lean, h, g=None, rec=None, flat=None):
    """a tuning that pins a k_nr_tree geometry: lean 1 lean / 2 fat, the residency switches 1 on / 2 off (None: automatic)"""
    t = dict(nr_waves=W, nr_lanes=L, nr_lean=lean, nr_h_lds=h)
    for k, v in (("nr_g_lds", g), ("nr_rec_lds", rec), ("nr_flat_lds", flat)):
        if v is not None:
            t[k] = v
    return t


B_ROW = 70                                                   # ragged: the last workgroups are part padding
_RES_PINS = {1: (1, 1), 2: (2, 2), 3: (1, 2)}                # RES -> (nr_rec_lds, nr_flat_lds) that selects it


def T(net, W, L, HL, GL, RES, rec=None, flat=None):
    """a k_nr_tree row: the geometry pinned fat, with the residency of RES (or, for the generic body RES = 0, the given one: a
    residency that no specialised instantiation of this geometry serves); the variant follows from the net's suffixes"""
    rec, flat = _RES_PINS[RES] if RES else (rec, flat)
    return Row(("tree", W, L, HL, GL, RES, *variant_of(net)), net, B_ROW, _pin(W, L, 2, 1 if HL else 2, 1 if GL else 2, rec, flat))


def S(net, L):
    """a k_nr_sparse row: sp_lanes pinned"""
    return Row(("sparse", L, *variant_of(net)), net, B_ROW, dict(nr_solver="sparse", sp_lanes=L))


def D(net, W, GA):
    """a k_nr_dense row: a radial feeder whose Jacobian order 2 (n_bus - 1), rounded up to 16, selects W"""
    return Row(("dense", W, GA), net, B_ROW, dict(nr_solver="dense"))


ROWS = [
    # ---- k_nr_tree
    # flat start
    T("case141", 4, 16, 1, 0, 1), T("case141", 4, 16, 1, 0, 3), T("case141", 4, 16, 1, 0, 0, rec=2, flat=2),
    T("case33", 4, 16, 1, 1, 0, rec=2, flat=2), T("case141", 4, 16, 0, 0, 0, rec=1, flat=2), T("case33", 1, 16, 1, 1, 1),
    T("case33", 1, 16, 1, 1, 0, rec=2, flat=2), T("case33", 1, 16, 1, 0, 0, rec=2, flat=2), T("case33", 1, 16, 0, 0, 0, rec=2, flat=2),
    T("case141", 2, 16, 0, 0, 2), T("case141", 2, 16, 0, 0, 0, rec=1, flat=2), T("case141", 2, 16, 1, 0, 0, rec=2, flat=2),
    T("case33", 2, 16, 1, 1, 0, rec=2, flat=2), T("case322", 4, 8, 1, 0, 3), T("case322", 4, 8, 1, 0, 2),
    T("case141", 4, 8, 1, 0, 0, rec=2, flat=1), T("case141", 4, 8, 1, 1, 0, rec=2, flat=2), T("case322", 4, 8, 0, 0, 0, rec=2, flat=2),
    T("case322", 4, 16, 0, 0, 2), T("case141", 1, 8, 1, 1, 0, rec=2, flat=2), T("case141", 1, 8, 1, 0, 0, rec=2, flat=2),
    T("case141", 1, 8, 0, 0, 0, rec=2, flat=2), T("case141", 2, 8, 1, 1, 0, rec=2, flat=2), T("case141", 2, 8, 1, 0, 0, rec=2, flat=2),
    T("case141", 2, 8, 0, 0, 0, rec=2, flat=2), T("case141", 1, 32, 0, 0, 0, rec=2, flat=2), T("case33", 1, 32, 1, 0, 0, rec=2, flat=2),
    T("case33", 1, 32, 1, 1, 0, rec=2, flat=2), T("case141", 4, 4, 1, 0, 0, rec=2, flat=2), T("case141", 4, 4, 1, 1, 0, rec=2, flat=2),
    T("case141", 4, 4, 0, 0, 0, rec=2, flat=2), T("case141", 2, 4, 1, 0, 0, rec=2, flat=2), T("case141", 2, 4, 1, 1, 0, rec=2, flat=2),
    T("case141", 2, 4, 0, 0, 0, rec=2, flat=2), T("case141", 1, 4, 1, 0, 0, rec=2, flat=2), T("case141", 1, 4, 1, 1, 0, rec=2, flat=2),
    # DC start (hv_front nets)
    T("case33_hv", 1, 16, 1, 1, 1), T("case141_hv", 4, 16, 1, 0, 1), T("case141_hv", 4, 16, 1, 0, 0, rec=2, flat=2),
    T("case33_hv", 4, 16, 1, 1, 0, rec=2, flat=2), T("case141_hv", 4, 16, 0, 0, 0, rec=1, flat=2), T("case33_hv", 1, 16, 1, 1, 0, rec=2, flat=2),
    T("case141_hv", 2, 16, 0, 0, 2), T("case33_hv", 2, 16, 1, 1, 0, rec=2, flat=2), T("case141_hv", 2, 16, 1, 0, 0, rec=2, flat=2),
    T("case141_hv", 2, 16, 0, 0, 0, rec=1, flat=2), T("case33_hv", 1, 16, 1, 0, 0, rec=2, flat=2), T("case33_hv", 1, 16, 0, 0, 0, rec=2, flat=2),
    T("case322_hv", 4, 8, 1, 0, 3), T("case322_hv", 4, 16, 0, 0, 2), T("case322_hv", 4, 8, 1, 0, 0, rec=2, flat=2),
    T("case141_hv", 4, 8, 1, 1, 0, rec=2, flat=2), T("case322_hv", 4, 8, 0, 0, 0, rec=2, flat=2),
    # ZIP loads, flat start
    T("case33_zip", 1, 16, 1, 1, 1), T("case141_zip", 4, 16, 1, 0, 1), T("case141_zip", 4, 16, 0, 0, 0, rec=1, flat=2),
    T("case141_zip", 2, 16, 0, 0, 2), T("case141_zip", 4, 16, 1, 0, 3), T("case33_zip", 1, 16, 0, 0, 0, rec=2, flat=2),
    T("case141_zip", 2, 16, 0, 0, 0, rec=1, flat=2), T("case322_zip", 4, 8, 1, 0, 3), T("case322_zip", 4, 8, 1, 0, 2),
    T("case322_zip", 4, 16, 0, 0, 2), T("case322_zip", 4, 8, 0, 0, 0, rec=2, flat=2),
    # ZIP loads, DC start
    T("case33_hv_zip", 1, 16, 1, 1, 1), T("case141_hv_zip", 4, 16, 1, 0, 1), T("case141_hv_zip", 4, 16, 0, 0, 0, rec=1, flat=2),
    T("case141_hv_zip", 2, 16, 0, 0, 2), T("case141_hv_zip", 4, 16, 1, 0, 3), T("case33_hv_zip", 1, 16, 0, 0, 0, rec=2, flat=2),
    T("case141_hv_zip", 2, 16, 0, 0, 0, rec=1, flat=2), T("case322_hv_zip", 4, 8, 1, 0, 3), T("case322_hv_zip", 4, 8, 1, 0, 2),
    T("case322_hv_zip", 4, 16, 0, 0, 2), T("case322_hv_zip", 4, 8, 0, 0, 0, rec=2, flat=2),
    # generators, flat start (the geometries and tunings of the ZIP rows)
    T("case33_gen", 1, 16, 1, 1, 1), T("case141_gen", 4, 16, 1, 0, 1), T("case141_gen", 4, 16, 0, 0, 0, rec=1, flat=2),
    T("case141_gen", 2, 16, 0, 0, 2), T("case141_gen", 4, 16, 1, 0, 3), T("case33_gen", 1, 16, 0, 0, 0, rec=2, flat=2),
    T("case141_gen", 2, 16, 0, 0, 0, rec=1, flat=2), T("case322_gen", 4, 8, 1, 0, 3), T("case322_gen", 4, 8, 1, 0, 2),
    T("case322_gen", 4, 16, 0, 0, 2), T("case322_gen", 4, 8, 0, 0, 0, rec=2, flat=2),
    # generators, DC start
    T("case33_hv_gen", 1, 16, 1, 1, 1), T("case141_hv_gen", 4, 16, 1, 0, 1), T("case141_hv_gen", 4, 16, 0, 0, 0, rec=1, flat=2),
    T("case141_hv_gen", 2, 16, 0, 0, 2), T("case141_hv_gen", 4, 16, 1, 0, 3), T("case33_hv_gen", 1, 16, 0, 0, 0, rec=2, flat=2),
    T("case141_hv_gen", 2, 16, 0, 0, 0, rec=1, flat=2), T("case322_hv_gen", 4, 8, 1, 0, 3), T("case322_hv_gen", 4, 8, 1, 0, 2),
    T("case322_hv_gen", 4, 16, 0, 0, 2), T("case322_hv_gen", 4, 8, 0, 0, 0, rec=2, flat=2),
    # ---- k_nr_sparse: every sp_lanes with the flat and the DC start, each plain, with ZIP loads and with generators
    *(S("case33_meshed" + suf, L) for suf in ("", "_hv", "_zip", "_hv_zip", "_gen", "_hv_gen") for L in (16, 8, 4, 2)),
    # ---- k_nr_dense: Jacobian order N = roundup16(2 n) in LDS up to 128, else in global memory with W = the first of DENSE_GA_W
    # with 64 W >= N
    D("case33", 1, 0), D("radial61", 2, 0), D("radial81", 3, 1), D("radial113", 4, 1), D("case141", 5, 1), D("radial177", 6, 1),
    D("radial241", 8, 1), D("case322", 11, 1), D("radial385", 13, 1), D("radial481", 16, 1),
]


# A pinned residency that has no instantiation of the handle's variant is refused at mapdn_create — never served by another kernel;
# the dense solver refuses the DC start, ZIP loads and generators by name, every solver generators with ZIP loads.  (net, B, tuning, text
# of the refusal)
NOT_COMPILED = "not compiled in"
REFUSALS = [
    # ZIP, fat (4, 16) with h in LDS and only the flat-start constants resident (RES 0): the ZIP list has no generic body of that layout
    ("case141_zip", B_ROW, _pin(4, 16, 2, 1, 2, 2, 1), NOT_COMPILED),
    ("case141_hv_zip", B_ROW, _pin(4, 16, 2, 1, 2, 2, 1), NOT_COMPILED),
    # ZIP, (4, 16) with G in LDS too, both residents (RES 1): only (4, 16, T, F, 1) is compiled
    ("case33_zip", B_ROW, _pin(4, 16, 2, 1, 1, 1, 1), NOT_COMPILED),
    # ZIP, (4, 8) with h in LDS and only the flat-start constants resident: no generic (4, 8, T, F) ZIP body
    ("case141_zip", B_ROW, _pin(4, 8, 2, 1, 2, 2, 1), NOT_COMPILED),
    ("case141_hv_zip", B_ROW, _pin(4, 8, 2, 1, 2, 2, 1), NOT_COMPILED),
    # DC start on pairs the chooser never takes: no DC instantiation at all
    ("case33_hv", B_ROW, _pin(1, 8, 2, 1, 1, 1, 1), NOT_COMPILED),
    ("case141_hv", B_ROW, _pin(4, 4, 2, 2, 2, 2, 2), NOT_COMPILED),
    # the dense solver refuses the variants by name
    ("case141_hv", B_ROW, dict(nr_solver="dense"), "nr_init = 2 (runpp init=\"dc\") is not built for nr_solver = dense"),
    ("case141_zip", B_ROW, dict(nr_solver="dense"), "voltage-dependent loads (load_const_z / load_const_i) are not built for nr_solver = dense"),
    # (new entries go to the end: the ids of the refusal tests carry the index)
    # generators, (4, 8) with h in LDS and only the flat-start constants resident: no generic (4, 8, T, F) GEN body
    ("case141_gen", B_ROW, _pin(4, 8, 2, 1, 2, 2, 1), NOT_COMPILED),
    # generators on a pair the chooser never takes: no GEN instantiation at all
    ("case33_gen", B_ROW, _pin(1, 8, 2, 1, 1, 1, 1), NOT_COMPILED),
    ("case141_gen", B_ROW, dict(nr_solver="dense"), "generators (net.gen, gen buses) are not built for nr_solver = dense"),
    # generators together with ZIP loads: refused whatever the solver (the one key with both suffixes; it has no variant)
    ("case33_gen_zip", B_ROW, None, "generators (net.gen) together with voltage-dependent loads"),
]
