"""Nets, ratings and voltages of the res_line / res_trafo edge tests (tests/test_branch_edges_cpu.py, tests/test_branch_edges_gpu.py; DESIGN.md
section 28): test infrastructure only, independent of the product code.  The references are those of tests/branch_ref.py (tables, bars,
summary_ref), which take any NetSpec.

comb(T)   a radial net with BOTH tables of length T: bus 0 (33 kV, slack); pi branch k joins bus 0 to the mid bus 1 + k (12.47 kV); line k
          joins mid bus 1 + k to its leaf, which carries a load, every third leaf an sgen.  Every row has constants of its own, smoothly
          varied in k with a seeded jitter, so that a record read from the wrong row or the wrong table gives another number.  From T = 15 on
          line OOS_ROW is out of service.  A connected net of 2T + 1 buses needs 2T branches in service and T + T - 1 are left, so that row
          cannot own a leaf: it is a spur from the leaf before it to its own mid bus (which carries the load instead), and the net has 2T
          buses.  Line UNRATED_LINE and pi branch UNRATED_TRAFO carry no rating.  T = 1 is the plain 3-bus net, all rated, all in service.
twins     a 12-bus feeder behind one transformer whose lines 3, 8 and 1, 9 are the same line entered twice (same buses, same constants, same
          rating): one entry of Ybus and one edge of the solver's graph (the handle calls the net radial), two rows of res_line with the same bits.  LS_WAVES = 8: rows 3 and 8 sit in
          waves 3 and 0 of k_loading_summary, rows 1 and 9 both in wave 1.  No line charges (c_nf_per_km = 0).  Six rating sets, rating_sets()."""
import dataclasses
import functools

import numpy as np

from oracle.pp_restated import runpp_restated
from tests import branch_ref as R

SIZES = ((1, 64), (15, 63), (16, 128), (17, 129), (33, 2))           # (T, B): tile edges of both tables x env-tile edges
OOS_ROW, UNRATED_LINE, UNRATED_TRAFO = 5, 2, 3                        # rows of comb(T), T >= 15
VN_HV, VN_LV = 33.0, (12.0, 12.9)                                     # nameplates: even rows 33 / 12.0 (the hv side wins the max), odd rows 33 / 12.9 (lv)
TWIN_ROWS = ((3, 8), (1, 9))
TWINS_B = 65
RATING_FIELDS = ("line_max_i_ka", "line_df", "br_vn_hv_kv", "br_vn_lv_kv", "br_rating_mva")
KEYS = tuple(f"comb{T}" for T, _ in SIZES) + ("twins",)
BATCHES = dict({f"comb{T}": B for T, B in SIZES}, twins=TWINS_B)


def leaf_of(T):
    """bus of line k's far end; -1 for the out-of-service row, which has no leaf of its own"""
    k = np.arange(T)
    if T == 1:
        return 1 + T + k
    return np.where(k == OOS_ROW, -1, 1 + T + k - (k > OOS_ROW))


@functools.lru_cache(maxsize=None)
def comb_base(T):
    """(NetSpec without ratings, Profiles)"""
    rng = np.random.default_rng(7700 + T)
    jit = lambda: 1.0 + 0.01 * rng.uniform(-1, 1, T)
    k = np.arange(T)
    leaf = leaf_of(T)
    dead = T > 1
    n_bus = 2 * T + (0 if dead else 1)
    f, t = 1 + k, leaf.copy()
    if dead:
        f[OOS_ROW], t[OOS_ROW] = leaf[OOS_ROW - 1], 1 + OOS_ROW
    c_nf = np.where(k % 2 == 0, 0.0, np.where(k % 4 == 1, 320.0, 10.0))                  # overhead | cable | a little
    length = np.where(k % 4 == 1, 3.0, 0.6) + 1.2 * np.sin(0.45 * k + 0.5) ** 2
    lines = [(f[i], t[i], r, x, c_nf[i], ln, 1 + (i % 5 == 3), not (dead and i == OOS_ROW))
             for i, (r, x, ln) in enumerate(zip((0.30 + 0.12 * np.sin(0.6 * k)) * jit(), (0.25 + 0.08 * np.cos(0.8 * k + 1.0)) * jit(), length * jit()))]
    zone = np.zeros(n_bus, int)
    for i in k:
        zone[1 + i] = 1 + (i // 3) % 4
        if leaf[i] >= 0:
            zone[leaf[i]] = zone[1 + i]
    load_bus = [int(leaf[i]) if leaf[i] >= 0 else 1 + int(i) for i in k]
    sg = [int(i) for i in k if i % 3 == 0]
    net = R._net(f"comb{T}", [VN_HV] + [12.47] * (n_bus - 1), zone, lines, load_bus, [int(leaf[i]) for i in sg],
                 br_from_bus=np.zeros(T, int), br_to_bus=1 + k, br_r_pu=(0.006 + 0.003 * np.cos(0.9 * k)) * jit(),
                 br_x_pu=(0.09 + 0.03 * np.sin(0.7 * k + 0.3)) * jit(), br_b_pu=np.where(k % 3 == 2, -0.004, 0.0) * jit(),
                 br_g_pu=np.where(k % 4 == 1, 0.001, 0.0) * jit(), br_ratio=1.0025 + 0.024 * np.sin(1.3 * k + 1.0) + 0.002 * rng.uniform(-1, 1, T),
                 br_shift_deg=2.7 * np.sin(0.5 * k + 2.0) + 0.2 * rng.uniform(-1, 1, T))
    prof = R._prof((0.35 + 0.25 * np.abs(np.sin(0.8 * k + 0.2))) * jit(), 0.9 * np.ones(len(sg)), 7800 + T)
    return net, prof


def _rating_state(net, prof):
    """the unrated float64 tables of the oracle's power flow at the first test row, no reactive set-points: where the ratings are chosen"""
    t = int(R.rows_of(prof, 1)[0])
    r = runpp_restated(net, prof.load_p[t], prof.load_q[t], prof.pv[t], np.zeros(net.n_sgen))
    assert r.converged, net.name
    return R.tables(dataclasses.replace(net, **{k: np.zeros(0) for k in RATING_FIELDS}), r.vm_pu, r.va_degree, np.float64)


def _trafo_s(trafo, vn_hv, vn_lv):
    return np.sqrt(3.0) * np.maximum(trafo["i_from_ka"] * vn_hv, trafo["i_to_ka"] * vn_lv)


@functools.lru_cache(maxsize=None)
def comb(T):
    """(NetSpec with ratings, Profiles).  Rated on the CPU as branch_ref.make rates: at the first test row the 2T branches are loaded at the
    2T values of linspace(30 %, 130 %) in a seeded order — no two alike, limit_percent = 100 splits them."""
    net, prof = comb_base(T)
    rng = np.random.default_rng(7900 + T)
    line, trafo = _rating_state(net, prof)
    u = rng.permutation(np.linspace(0.3, 1.3, 2 * T))
    i_ka = line["i_ka"]
    df = rng.choice([1.0, 0.9, 0.8], T)
    max_i = np.where(i_ka > 1e-3 * i_ka.max(), i_ka, i_ka.max()) / u[:T] / df / net.line_parallel          # (the dead row: the largest rating)
    vn_hv, vn_lv = np.full(T, VN_HV), np.array([VN_LV[i % 2] for i in range(T)])
    mva = _trafo_s(trafo, vn_hv, vn_lv) / u[T:]
    if T > 1:
        max_i[UNRATED_LINE] = np.nan
        mva[UNRATED_TRAFO] = np.nan
    return dataclasses.replace(net, line_max_i_ka=max_i, line_df=df, br_vn_hv_kv=vn_hv, br_vn_lv_kv=vn_lv, br_rating_mva=mva), prof


# ---- twins ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def twins_base():
    """0 (33 kV) = transformer = 1 - 2 - 3 - 4 - 5 - 6;  2 - 7 - 8 - 9;  3 - 10 - 11;  rows 8 and 9 repeat rows 3 (4 - 5) and 1 (2 - 3).
    The loads behind the twins outweigh the sgens there, so the twins carry current in every env."""
    a, b = (0.28, 0.22, 0.0, 0.9, 1, 1), (0.33, 0.27, 0.0, 1.3, 1, 1)
    lines = [(1, 2, 0.20, 0.18, 0.0, 0.8, 1, 1), (2, 3) + a, (3, 4, 0.31, 0.24, 0.0, 1.1, 1, 1), (4, 5) + b, (5, 6, 0.36, 0.29, 0.0, 0.7, 1, 1),
             (2, 7, 0.27, 0.21, 0.0, 1.4, 1, 1), (7, 8, 0.38, 0.26, 0.0, 0.6, 1, 1), (8, 9, 0.42, 0.31, 0.0, 1.0, 1, 1), (4, 5) + b, (2, 3) + a,
             (3, 10, 0.35, 0.23, 0.0, 0.9, 1, 1), (10, 11, 0.44, 0.33, 0.0, 0.5, 1, 1)]
    net = R._net("twins", [VN_HV] + [12.47] * 11, [0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 3, 3], lines, [3, 4, 5, 6, 7, 8, 9, 10, 11], [6, 9, 11],
                 br_from_bus=np.array([0]), br_to_bus=np.array([1]), br_r_pu=np.array([0.004]), br_x_pu=np.array([0.05]), br_b_pu=np.array([-0.010]),
                 br_g_pu=np.array([0.002]), br_ratio=np.array([0.98]), br_shift_deg=np.array([1.0]))
    assert all(lines[i] == lines[j] for i, j in TWIN_ROWS) and (net.line_c_nf_per_km == 0).all()
    return net, R._prof([0.3, 0.4, 0.9, 0.8, 0.3, 0.2, 0.3, 0.3, 0.4], [0.3, 0.5, 0.4], 8100)


@functools.lru_cache(maxsize=None)
def rating_sets():
    """name -> the five arrays of mapdn_set_branch_ratings in RATING_FIELDS' order (None = NULL), chosen at the first test row:
    A  rows 3, 8 loaded at 120 %, every other branch at 5 %         B  rows 1, 9 at 120 %, the others at 5 %
    C  no line rated, the transformer at 60 %                       D  nothing rated
    E  A with every line_max_i_ka doubled                           A11  A with line 11 unrated (the exact-zero test's NaN row)"""
    net, prof = twins_base()
    line, trafo = _rating_state(net, prof)
    i_ka, n = line["i_ka"], net.n_line
    df = np.array([1.0, 0.9, 1.0, 0.8, 0.9, 1.0, 0.8, 0.9, 0.8, 0.9, 1.0, 0.9])
    hv, lv = np.array([VN_HV]), np.array([12.47])
    s = _trafo_s(trafo, hv, lv)

    def lines_with(pair):
        u = np.full(n, 0.05)
        u[list(pair)] = 1.2
        m = i_ka / u / df
        m[pair[1]] = m[pair[0]]                                       # the twins: one rating, bit for bit
        return m
    a = lines_with(TWIN_ROWS[0])
    a11 = a.copy(); a11[11] = np.nan
    return dict(A=(a, df, hv, lv, s / 0.05), B=(lines_with(TWIN_ROWS[1]), df, hv, lv, s / 0.05), C=(None, None, hv, lv, s / 0.6),
                D=(None,) * 5, E=(2.0 * a, df, hv, lv, s / 0.05), A11=(a11, df, hv, lv, s / 0.05))


def rated(net, rset):
    """the NetSpec that carries a rating set: what the references read"""
    return dataclasses.replace(net, **{k: np.zeros(0) if v is None else np.array(v) for k, v in zip(RATING_FIELDS, rset)})


@functools.lru_cache(maxsize=None)
def make(key, rset="A"):
    """(NetSpec, Profiles) of "comb<T>" or of "twins" under a rating set"""
    if key == "twins":
        net, prof = twins_base()
        return rated(net, rating_sets()[rset]), prof
    return comb(int(key[4:]))


@functools.lru_cache(maxsize=None)
def oracle_voltages(key, B, q_scale=0.5):
    """vm_pu, va_degree [B, n_bus] of the oracle's power flows at the key's test rows with seeded reactive set-points (branch_ref's
    oracle_voltages for these nets); every one of them must converge"""
    net, prof = make(key)
    rng = np.random.default_rng(B + sum(map(ord, key)))
    smax = prof.s_max(1.2)
    vm, va = [], []
    for t in R.rows_of(prof, B):
        q = q_scale * rng.uniform(-1, 1, net.n_sgen) * np.sqrt(np.maximum(smax ** 2 - prof.pv[t] ** 2, 0.0))
        r = runpp_restated(net, prof.load_p[t], prof.load_q[t], prof.pv[t], q)
        assert r.converged, (key, int(t))
        vm.append(r.vm_pu); va.append(r.va_degree)
    return np.stack(vm), np.stack(va)


# ---- the altered voltages of the non-finite test: comb(17), B = 129 -----------------------------------------------------------------------------
NAN_VM = (5, 8)            # (env, line row): vm = NaN at that row's leaf
ZERO_VM = (70, 10)         # vm = 0 at that row's leaf
NAN_VA_ENV = 128           # va = NaN at bus 0, in the LAST env: the pad lanes of the third env tile clamp onto it


def altered(vm, va, T=17):
    """copies of vm, va [B, n_bus] with the three alterations, and touched[B, 2T]: the rows (lines, then pi branches) that read an altered bus"""
    vm, va = vm.copy(), va.copy()
    leaf = leaf_of(T)
    touched = np.zeros((vm.shape[0], 2 * T), bool)
    vm[NAN_VM[0], leaf[NAN_VM[1]]] = np.nan; touched[NAN_VM[0], NAN_VM[1]] = True
    vm[ZERO_VM[0], leaf[ZERO_VM[1]]] = 0.0; touched[ZERO_VM[0], ZERO_VM[1]] = True
    va[NAN_VA_ENV, 0] = np.nan; touched[NAN_VA_ENV, T:] = True
    return vm, va, touched
