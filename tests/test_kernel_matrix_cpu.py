"""CPU tests of the power-flow kernel matrix (tests/kernel_matrix.py): every row's host-only handle reports exactly its kernel through
mapdn_get_nr_kernel, the rows cover the compiled set parsed from the sources — an instantiation added without a row fails here — and the
refusal rows are refused with their text."""
import ctypes as C
import re

import pytest

from mapdn_amd import _lib
from mapdn_amd.netspec import make_case
from tests import kernel_matrix as km


def uncovered(compiled, rows):
    """compiled kernels without a row, and row kernels that are not compiled"""
    have = {km.compiled_of(r.kernel) for r in rows}
    return sorted(set(compiled) - have), sorted(have - set(compiled))


def test_the_compiled_set_parses():
    """the parser reads every entry of the macros (none lost, none twice) and each one is a well-formed instantiation"""
    tree, sparse, dense = km.tree_kernels(), km.sparse_kernels(), km.dense_kernels()
    src = km._src("nr_inst_list.hpp")
    n_x = {fam: sum(km._macro(src, m).count("X(") for m in re.findall(r"#define\s+(" + fam + r"\d+)\(X\)", src))
           for fam in ("NR_INSTS_", "NR_INSTS_DC_", "NR_INSTS_ZIP_", "NR_INSTS_GEN_")}
    assert all(n_x.values()), n_x
    assert len(tree) == n_x["NR_INSTS_"] + n_x["NR_INSTS_DC_"] + 2 * n_x["NR_INSTS_ZIP_"] + 2 * n_x["NR_INSTS_GEN_"], n_x
    assert sum(k[8] for k in tree) == 2 * n_x["NR_INSTS_GEN_"]
    assert len(set(tree)) == len(tree) and len(set(sparse)) == len(sparse) and len(set(dense)) == len(dense)
    for _, W, L, HL, GL, RES, DC, ZIP, GEN in tree:
        assert W in (1, 2, 4, 8) and L in (4, 8, 16, 32) and RES in (0, 1, 2, 3) and (HL or not GL) and not (ZIP and GEN)
    assert {k[1] for k in sparse} == {16, 8, 4, 2}
    assert [k[1] for k in dense if not k[2]] == [1, 2]
    total = len(tree) + len(sparse) + len(dense)
    print(f"[kernel matrix] compiled: {len(tree)} k_nr_tree + {len(sparse)} k_nr_sparse + {len(dense)} k_nr_dense = {total}; "
          f"{len(km.ROWS)} rows")


def test_the_rows_cover_the_compiled_set_exactly():
    """one row per k_nr_tree / k_nr_dense instantiation, one per (L, DC, ZIP) of k_nr_sparse without generators and one per (L, DC)
    with them, and no row for a kernel that is not compiled"""
    missing, extra = uncovered(km.compiled_kernels(), km.ROWS)
    assert not missing, f"compiled kernels without a row in tests/kernel_matrix.py: {missing}"
    assert not extra, f"rows for kernels that are not compiled: {extra}"
    kernels = [r.kernel for r in km.ROWS]
    assert len(set(kernels)) == len(kernels), "two rows for one kernel"
    cells = [(L, dc, z) for L in (16, 8, 4, 2) for dc in (0, 1) for z in (0, 1)]
    want = {("sparse", L, dc, z, 0) for L, dc, z in cells} | {("sparse", L, dc, 0, 1) for L, dc, _ in cells}
    have = {k for k in kernels if k[0] == "sparse"}
    assert have == want, f"k_nr_sparse cells without a row: {sorted(want - have)}; rows for no cell: {sorted(have - want)}"
    assert not [r for r in km.ROWS if r.kernel[0] != "dense" and r.kernel[-2] and r.kernel[-1]], "a row with ZIP and GEN together"
    assert all(r.kernel[0] == "dense" or r.kernel[-3:] == km.variant_of(r.net) for r in km.ROWS)
    assert all(r.B % 64 for r in km.ROWS)


def test_an_instantiation_without_a_row_is_caught():
    """the coverage check of the test above, on a copy of nr_inst_list.hpp with one more X(...) in NR_INSTS_3 / NR_INSTS_ZIP_3 /
    NR_INSTS_GEN_3"""
    real = km._src
    for macro, new, want in (("NR_INSTS_3(X)", "X(2, 8, true, true, 1) ", [("tree", 2, 8, 1, 1, 1, 0, 0, 0)]),
                             ("NR_INSTS_ZIP_3(X)", "X(1, 8, false, false, 0)",
                              [("tree", 1, 8, 0, 0, 0, 0, 1, 0), ("tree", 1, 8, 0, 0, 0, 1, 1, 0)]),
                             ("NR_INSTS_GEN_3(X)", "X(1, 8, false, false, 0)",
                              [("tree", 1, 8, 0, 0, 0, 0, 0, 1), ("tree", 1, 8, 0, 0, 0, 1, 0, 1)])):
        def patched(name, _m=macro, _n=new):
            s = real(name)
            return s.replace("#define " + _m, "#define " + _m + " " + _n, 1) if name == "nr_inst_list.hpp" else s
        km._src = patched
        try:
            compiled = km.compiled_kernels()
        finally:
            km._src = real
        assert uncovered(compiled, km.ROWS) == (want, []), macro


@pytest.mark.parametrize("row", km.ROWS, ids=km.row_id)
def test_every_row_reports_its_kernel(row):
    rc, k = km.host_kernel(row.net, row.B, row.tuning)
    assert rc == 0, k
    assert km.kernel_tuple(k) == row.kernel, (km.kernel_tuple(k), row)


@pytest.mark.parametrize("net,B,tuning,text", km.REFUSALS, ids=[f"{r[0]}-{i}" for i, r in enumerate(km.REFUSALS)])
def test_a_pinned_layout_without_its_variant_is_refused(net, B, tuning, text):
    rc, msg = km.host_kernel(net, B, tuning)
    assert rc == -1, (rc, msg)                                   # MAPDN_E_INVALID
    assert text in msg, msg


def _handle(net, B, tuning=None):
    lib = _lib.load()
    cn, keep = _lib.make_cnetspec(net)
    h = C.c_void_p()
    assert lib.mapdn_create(C.byref(cn), C.byref(_lib.make_cconfig(km.ARGS, 0, km.tuning_for(net, tuning))), B, -1, C.byref(h)) == 0, \
        lib.mapdn_last_error(None).decode()
    return lib, h, keep


@pytest.mark.parametrize("key,B", [("case33", 1), ("case141", 70), ("case141", 8192), ("case322", 1000), ("case322", 8190),
                                   ("case141_hv_zip", 4096), ("case33_meshed", 70), ("case33_meshed_hv", 70), ("case322_gen", 8190),
                                   ("case141_hv_gen", 4096), ("case33_meshed_gen", 70)])
def test_the_kernel_agrees_with_the_geometry_export(key, B):
    """mapdn_get_nr_kernel and mapdn_get_nr_geometry describe the same launch: the tree geometry's (W, L, h, G) and its residency
    (the specialised RES when one is compiled), the sparse envs per workgroup that the host stage settled on — on host-only handles
    too, where the sparse choice used to be skipped"""
    net, _ = km.make_net(key)
    lib, h, keep = _handle(net, B)
    try:
        g, k = _lib.nr_geometry(h), _lib.nr_kernel(h)
    finally:
        lib.mapdn_destroy(h)
    assert k["solver"] == g["solver"]
    if k["solver"] == 0:
        assert (k["W"], k["L"], k["HL"], k["GL"]) == (g["waves"], g["lanes"], g["h_lds"], g["g_lds"]), (k, g)
        res = {(1, 1): 1, (0, 0): 2, (1, 0): 3}.get((g["rec_lds"], g["flat_lds"]), 0)
        assert k["RES"] in (0, res), (k, g)
        assert (k["DC"], k["ZIP"], k["GEN"]) == km.variant_of(key)
    else:
        assert k["L"] == g["lanes"] and g["lds_bytes"] > 0, (k, g)
        assert (k["DC"], k["ZIP"], k["GEN"]) == km.variant_of(key)


def test_the_dense_kernel_follows_from_the_bus_count():
    """k_nr_dense<W, GA>: N = roundup16(2 n) Jacobian rows (n non-slack buses); in LDS up to 128 rows (W = 1 up to 64), else in global
    memory with the first W of DENSE_GA_W whose 64 W threads cover N"""
    ga_w = [k[1] for k in km.dense_kernels() if k[2]]
    for key in ("case33", "case141", "case322"):
        net, _ = make_case(key)
        lib, h, keep = _handle(net, 70, dict(nr_solver="dense"))
        try:
            k = _lib.nr_kernel(h)
        finally:
            lib.mapdn_destroy(h)
        N = (2 * (net.n_bus - 1) + 15) // 16 * 16
        want = (1 if N <= 64 else 2, 0) if N <= 128 else (min(w for w in ga_w if 64 * w >= N), 1)
        assert (k["W"], k["GA"]) == want, (key, k)
