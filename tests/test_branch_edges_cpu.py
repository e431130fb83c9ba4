"""CPU (-m "not gpu") side of the res_line / res_trafo edge tests: what tests/test_branch_edges_gpu.py relies on, shown
of the nets, ratings and references of tests/branch_edge_cases.py alone — every net converges in the oracle at its test rows, its bars are
finite, the rows that carry an edge carry it, the top two loadings are apart (comb) or bitwise equal and far above the rest (twins) — and
mapdn_amd/csrc/branch.hpp built by g++ (tests/branch_check.cpp, also under ASan + UBSan as a stand-alone program) on the new nets against
the extended reference, with the altered and the flat voltages of the GPU tests."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mapdn_amd import _lib
from tests import branch_edge_cases as E
from tests import branch_ref as R
from tests.test_branch_cpu import ROOT, host_branch, host_handle    # noqa: F401  (host_branch: the fixture that builds branch_check)

N_ENVS = 5                                             # oracle states per net of the host checks
COMBS = [T for T, _ in E.SIZES]


def loadings(key, rset="A"):
    """float64 reference: (net, loading_percent [B, n_line + n_trafo], bar) at the oracle's voltages of all B test rows"""
    net, _ = E.make(key, rset) if key == "twins" else E.make(key)
    vm, va = E.oracle_voltages(key, E.BATCHES[key])
    line, trafo = R.batch_tables(net, vm, va, np.float64)
    bl, bt = R.bars(net, vm, va)
    return net, np.concatenate([line["loading_percent"], trafo["loading_percent"]], 1), max(bl["loading_percent"], bt["loading_percent"])


@pytest.mark.parametrize("key", E.KEYS)
def test_nets_converge_and_their_bars_are_finite(key):
    net, _ = E.make(key)
    vm, va = E.oracle_voltages(key, E.BATCHES[key])                     # asserts convergence row by row
    assert vm.shape == (E.BATCHES[key], net.n_bus) and np.isfinite(vm).all() and np.isfinite(va).all()
    for tab, e, b in zip(("line", "trafo"), R.e64(net, vm, va), R.bars(net, vm, va)):
        assert set(e) == set(R.COLUMNS)
        for k in R.COLUMNS:
            assert np.isfinite(e[k]) and np.isfinite(b[k]) and R.BAR_FLOOR <= b[k] < 1e-9, (key, tab, k, e[k], b[k])


def test_sizes_sit_on_the_tile_edges():
    src = open(os.path.join(ROOT, "mapdn_amd", "csrc", "kernels.hpp")).read()
    tile, waves = (int(re.search(name + r" = (\d+)", src).group(1)) for name in ("BR_TILE", "LS_WAVES"))
    assert {T - tile for T, _ in E.SIZES} >= {-1, 0, 1} and any(T > 2 * tile for T, _ in E.SIZES) and (1, 64) in E.SIZES
    assert {B % 64 for _, B in E.SIZES} >= {0, 1, 63} and any(B == 64 for _, B in E.SIZES) and any(B > 128 for _, B in E.SIZES)
    (a, b), (c, d) = E.TWIN_ROWS
    assert a < b and a % waves != b % waves and b % waves == 0         # wave 0 holds row 8 and must hand over to the LOWER row 3 of a later wave
    assert c < d and c % waves == d % waves                             # one wave: keep the first
    assert E.TWINS_B == 65 and E.NAN_VA_ENV == dict(E.SIZES)[17] - 1 and E.NAN_VM[0] < 64 <= E.ZERO_VM[0] < 128 <= E.NAN_VA_ENV


@pytest.mark.parametrize("T", COMBS)
def test_comb_is_a_radial_net_with_both_tables_of_length_T(lib, T):
    net, _ = E.comb(T)
    assert net.n_line == net.n_branch_pu == T and net.n_bus == (3 if T == 1 else 2 * T)
    assert (net.bus_vn_kv[net.br_from_bus] == 33.0).all() and (net.bus_vn_kv[net.br_to_bus] == 12.47).all()
    h, keep = host_handle(lib, net)
    try:
        dims = _lib.CDims()
        assert lib.mapdn_dims(h, C.byref(dims)) == 0 and dims.is_radial == 1 and dims.n_line == T      # the tree solver takes it
    finally:
        lib.mapdn_destroy(h)
    for k in ("br_r_pu", "br_x_pu", "br_ratio", "br_shift_deg", "line_r_ohm_per_km", "line_x_ohm_per_km", "line_length_km"):
        assert np.unique(getattr(net, k)).shape[0] == T, k               # a row of its own everywhere
    assert ((net.br_ratio > 0.976) & (net.br_ratio < 1.029)).all() and (np.abs(net.br_shift_deg) < 3.0).all()
    if T > 1:
        assert set(net.line_parallel) == {1, 2} and (net.br_g_pu != 0).any() and (net.br_b_pu != 0).any() and (net.br_g_pu == 0).any()
        assert (net.line_c_nf_per_km[::2] == 0).all() and (net.line_c_nf_per_km[1::2] > 0).all()
        assert set(net.br_vn_lv_kv) == {12.0, 12.9} and (net.br_vn_hv_kv == 33.0).all()


@pytest.mark.parametrize("T", [T for T in COMBS if T > 1])
def test_comb_carries_what_it_claims(host_branch, T):
    """tests/test_branch_cpu.py::test_tree8_carries_what_it_claims for comb(T): both sides of the transformer's max, charging and uncharged
    lines, and the three special rows where the GPU test expects them — in the extended reference and in branch.hpp on the host"""
    net, _ = E.comb(T)
    vm, va = E.oracle_voltages(f"comb{T}", min(N_ENVS, E.BATCHES[f"comb{T}"]))
    ref = R.batch_tables(net, vm, va)
    for line, trafo in (ref, host_branch(net, vm, va)):
        hv, lv = trafo["i_from_ka"] * net.br_vn_hv_kv, trafo["i_to_ka"] * net.br_vn_lv_kv
        # both sides of max(i_hv vn_hv, i_lv vn_lv), clear of the bar in every env: lv / hv is about ratio x vn_lv / 12.47 less the magnetising
        # current, so the 12.0 kV nameplates (even rows) all end on the hv side and at least three of the 12.9 kV ones on the lv side
        assert (hv[:, 0::2] > 1.004 * lv[:, 0::2]).all() and (lv[:, 1::2] > 1.004 * hv[:, 1::2]).all(0).sum() >= 3
        d = np.abs(line["i_from_ka"] - line["i_to_ka"]) / np.where(line["i_ka"] > 0, line["i_ka"], 1.0)
        cable = net.line_c_nf_per_km == 320.0
        cable[E.OOS_ROW] = False
        assert cable.sum() >= 3 and (d[:, cable] > 1e-3).all() and (d[:, net.line_c_nf_per_km == 0] < 1e-12).all()
        assert not net.line_in_service[E.OOS_ROW] and net.line_in_service.sum() == T - 1
        assert all((line[k][:, E.OOS_ROW] == 0).all() for k in R.COLUMNS)
        assert (np.delete(line["i_ka"], E.OOS_ROW, axis=1) > 0).all() and (trafo["i_from_ka"] > 0).all()
        assert np.array_equal(np.flatnonzero(np.isnan(np.asarray(line["loading_percent"], float)).all(0)), [E.UNRATED_LINE])
        assert np.array_equal(np.flatnonzero(np.isnan(np.asarray(trafo["loading_percent"], float)).all(0)), [E.UNRATED_TRAFO])
        assert np.isfinite(np.delete(np.asarray(line["loading_percent"], float), E.UNRATED_LINE, axis=1)).all()
    # rated as branch_ref.make rates: 30 % .. 130 % at the rating row, no two alike
    l0, t0 = R.tables(net, *(x[0] for x in E.oracle_voltages(f"comb{T}", 1, q_scale=0.0)), np.float64)
    u = np.concatenate([np.delete(l0["loading_percent"], [E.OOS_ROW, E.UNRATED_LINE]), np.delete(t0["loading_percent"], E.UNRATED_TRAFO)])
    assert u.min() > 29.9 and u.max() < 130.1 and np.diff(np.sort(u)).min() > 1.0 and (u > 100).any() and (u < 100).any()


@pytest.mark.parametrize("T", COMBS)
def test_top_two_loadings_are_apart_on_the_combs(T):
    """tests/test_branch_cpu.py::test_top_two_loadings_are_apart for comb(T): by the reference alone, at most 5 % of the envs are undecided"""
    key = f"comb{T}"
    net, load, bar = loadings(key)
    *_, gap = R.summary_ref(net, load[:, :T], load[:, T:], 100.0)
    share = float((gap <= 2.0 * bar).mean())
    print(key, "B", E.BATCHES[key], "smallest gap", gap.min(), "bar", bar, "share left out", share)
    assert share <= 0.05


def test_twins_tie_exactly_and_stand_clear_of_the_rest():
    for rset, (lo, hi) in zip("AB", E.TWIN_ROWS):
        net, load, bar = loadings("twins", rset)
        assert load.shape == (E.TWINS_B, 13)
        assert np.array_equal(load[:, lo].view(np.int64), load[:, hi].view(np.int64)), "the twins' loadings are the same bits"
        rest = np.delete(load, [lo, hi], axis=1)
        assert np.isfinite(load).all() and (load[:, lo] - rest.max(1) > 2.0 * bar * load[:, lo]).all()
        print("twins", rset, "twin loading", load[:, lo].min(), "..", load[:, lo].max(), "the rest at most", rest.max())
        assert (load[:, lo] > 4.0 * rest.max(1)).all()                   # a wide margin, in every env
        mx, wb, no, _ = R.summary_ref(net, load[:, :12], load[:, 12:], 100.0)
        assert (wb == lo).all()                                          # numpy's argmax: the lowest index that attains it
    for a, b in E.TWIN_ROWS:                                             # every column, not the loading alone
        net, _ = E.make("twins", "A")
        line, _ = R.batch_tables(net, *E.oracle_voltages("twins", N_ENVS), np.float64)
        assert all(np.array_equal(line[k][:, a], line[k][:, b]) for k in R.COLUMNS)
    sets = E.rating_sets()
    _, load, _ = loadings("twins", "C")
    assert np.array_equal(np.flatnonzero(~np.isnan(load).all(0)), [12]) and np.isfinite(load[:, 12]).all()     # exactly one branch is rated
    assert np.isnan(loadings("twins", "D")[1]).all() and all(v is None for v in sets["D"])
    assert np.array_equal(sets["E"][0], 2.0 * sets["A"][0]) and all(np.array_equal(x, y) for x, y in zip(sets["E"][1:], sets["A"][1:]))
    assert np.array_equal(loadings("twins", "E")[1][:, :12] * 2.0, loadings("twins", "A")[1][:, :12])            # a power of two: exact
    assert np.isnan(sets["A11"][0][11]) and np.array_equal(sets["A11"][0][:11], sets["A"][0][:11])


def test_twins_fold_into_one_edge_for_the_solver(lib):
    """two rows between the same two buses are one entry of Ybus and one edge of the plan's graph: the handle calls the net radial and the
    tree solver runs it, while res_line keeps the twelve rows"""
    net, _ = E.make("twins")
    h, keep = host_handle(lib, net)
    try:
        dims = _lib.CDims()
        assert lib.mapdn_dims(h, C.byref(dims)) == 0 and dims.is_radial == 1 and dims.n_line == 12
        p = lambda a: None if a is None else _lib._p(np.ascontiguousarray(a, dtype=np.float64), _lib._pd)
        for name, rset in E.rating_sets().items():                       # every set is one the entry point takes
            assert lib.mapdn_set_branch_ratings(h, *[p(a) for a in rset]) == 0, (name, lib.mapdn_last_error(h))
    finally:
        lib.mapdn_destroy(h)


@pytest.mark.parametrize("key", E.KEYS + ("twins/C",))
def test_host_arithmetic_on_the_edge_nets(host_branch, key):
    """every column of both tables from branch.hpp (g++) against ref at the oracle's voltages, within 16 x e64 (>= 64 ulp) per column"""
    key, rset = (key.split("/") + ["A"])[:2]
    net, _ = E.make(key, rset) if key == "twins" else E.make(key)
    vm, va = E.oracle_voltages(key, min(N_ENVS, E.BATCHES[key]))
    got = host_branch(net, vm, va)
    err, bar = R.errors(net, vm, va, *got), R.bars(net, vm, va)
    for tab, e, b in zip(("line", "trafo"), err, bar):
        print(key, rset, tab, {k: f"{e[k]:.1e}/{b[k]:.1e}" for k in e})
        for k in e:
            assert e[k] <= b[k], (key, tab, k, e[k], b[k])


def test_host_arithmetic_at_nan_and_zero_voltages(host_branch):
    """the altered voltages of the GPU test on branch.hpp: NaN exactly where the extended reference has it, an exact 0 current at the
    |V| = 0 end, everything else the same bits as at the clean voltages"""
    T, B = 17, dict(E.SIZES)[17]
    net, _ = E.comb(T)
    vm, va = E.oracle_voltages("comb17", B)
    vm2, va2, touched = E.altered(vm, va, T)
    clean, got = host_branch(net, vm, va), host_branch(net, vm2, va2)
    err, bar = R.errors(net, vm2, va2, *got), R.bars(net, vm2, va2)     # rel_err asserts the NaN pattern
    for sl, tab, c, g, e, b in zip((slice(0, T), slice(T, None)), ("line", "trafo"), clean, got, err, bar):
        for k in R.COLUMNS:
            assert e[k] <= b[k], (tab, k, e[k], b[k])
            assert np.array_equal(c[k][~touched[:, sl]], g[k][~touched[:, sl]], equal_nan=True), (tab, k)
    line, trafo = got
    assert all(np.isnan(line[k][E.NAN_VM]) for k in R.COLUMNS) and all(np.isnan(trafo[k][E.NAN_VA_ENV]).all() for k in R.COLUMNS)
    assert line["i_to_ka"][E.ZERO_VM] == 0.0 and line["p_to_mw"][E.ZERO_VM] == 0.0 and line["i_from_ka"][E.ZERO_VM] > 0
    assert all((line[k][:, E.OOS_ROW] == 0).all() for k in R.COLUMNS)


def test_host_arithmetic_gives_exact_zeros_at_flat_voltages(host_branch):
    """uncharged lines, one voltage everywhere: yff = -yft bit for bit, so every flow, loss, current and loading of a rated line is 0.0"""
    net, _ = E.make("twins", "A11")
    line, trafo = host_branch(net, np.ones((2, 12)), np.zeros((2, 12)))
    for k in R.COLUMNS:
        rows = slice(0, 11) if k == "loading_percent" else slice(None)
        assert (line[k][:, rows] == 0.0).all(), k
    assert np.isnan(line["loading_percent"][:, 11]).all() and (trafo["i_from_ka"] > 0).all()
    ref = R.batch_tables(net, np.ones((2, 12)), np.zeros((2, 12)))[0]
    assert all((np.nan_to_num(np.asarray(ref[k], float)) == 0.0).all() for k in R.COLUMNS)
