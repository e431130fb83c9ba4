"""GPU (-m gpu) tests of res_line / res_trafo / loading_summary (csrc/branch.hip) at the edges of their tiles, of the summary's merge and of
the ratings, through the C ABI between sentinel guards.  Nets, ratings and altered voltages: tests/branch_edge_cases.py;
references and bars: tests/branch_ref.py at the kernel's own input voltages (16 x e64, never below 64 ulp); what these tests rely on is
asserted without a GPU in tests/test_branch_edges_cpu.py.

comb(T) x B = (1, 64), (15, 63), (16, 128), (17, 129), (33, 2): both tables one row short of a tile, a full tile, one row into the second
tile and into the third; a full env tile without pad lanes (B == Bp), one env short of it, two full tiles, one env into the third.
twins x 65: two pairs of identical rows, one pair across two waves of the summary and one inside a wave, the rating sets applied in turn
to one live handle."""
import numpy as np
import pytest
import torch

from mapdn_amd import _lib
from tests import branch_edge_cases as E
from tests import branch_ref as R
from tests.test_branch_results_gpu import DEV, LIMIT, c_summary, c_tables, check_against_ref, check_summary, make_env, same_tables

pytestmark = pytest.mark.gpu

COMBS = [T for T, _ in E.SIZES]
NO_COLS = ()


def single_envs(B):
    """one env of the first env tile and, where there is one, one of the second"""
    return (min(5, B - 1),) + ((B - 1,) if B > 64 else ())


def routes(env, vm, va):
    """the full request twice, the trafo-only request in both its forms and the line-only request in both, on one voltage route"""
    return dict(tables=c_tables(env, vm, va), again=c_tables(env, vm, va),
                trafo_only_null=c_tables(env, vm, va, NO_COLS, R.COLUMNS, null=("line",)), trafo_only_empty=c_tables(env, vm, va, NO_COLS, R.COLUMNS),
                line_only_null=c_tables(env, vm, va, R.COLUMNS, NO_COLS, null=("trafo",)), line_only_empty=c_tables(env, vm, va, R.COLUMNS, NO_COLS))


_COMB = {}


def run_comb(T):
    """comb(T)'s batch through both routes, once, shared by the tests below"""
    if T in _COMB:
        return _COMB[T]
    net, prof = E.comb(T)
    B = dict(E.SIZES)[T]
    rows = R.rows_of(prof, B)
    rng = np.random.default_rng(100 + T)
    out = dict(net=net, B=B)
    env = make_env(net, prof, B)
    try:
        assert env.is_radial and env.n_line == T and env.n_trafo == T
        q = 0.5 * rng.uniform(-1, 1, (B, net.n_sgen)) * np.sqrt(np.maximum(prof.s_max(1.2) ** 2 - prof.pv[rows] ** 2, 0.0))
        vm, va, _, conv = env.solve(prof.load_p[rows], prof.load_q[rows], prof.pv[rows], q)
        assert bool(conv.all())
        out["solve"] = dict(routes(env, vm, va), vm=vm.cpu().numpy(), va=va.cpu().numpy())
        if T == 17:                                                   # the non-finite voltages: three envs altered, the rest as solve() left them
            vm2, va2, touched = E.altered(out["solve"]["vm"], out["solve"]["va"], T)
            out["altered"] = dict(vm=vm2, va=va2, touched=touched, tables=c_tables(env, torch.as_tensor(vm2, device=DEV), torch.as_tensor(va2, device=DEV)))
        env.reset(start_rows=torch.as_tensor(rows), add_noise=False)
        res = {k: v.cpu().numpy() for k, v in env.results(("vm_pu", "va_degree")).items()}
        out["reset"] = dict(routes(env, None, None), vm=res["vm_pu"], va=res["va_degree"], summary=c_summary(env), summary_again=c_summary(env))
    finally:
        env.close()
    out["single"] = {}
    for e in single_envs(B):
        env = make_env(net, prof, 1, env_id_offset=e)
        try:
            env.reset(start_rows=torch.as_tensor(rows[e:e + 1]), add_noise=False)
            out["single"][e] = dict(vm=env.results(("vm_pu",))["vm_pu"].cpu().numpy(), tables=c_tables(env), summary=c_summary(env))
        finally:
            env.close()
    _COMB[T] = out
    return out


@pytest.mark.parametrize("route", ["solve", "reset"])
@pytest.mark.parametrize("T", COMBS)
def test_tile_and_batch_edges_against_the_extended_reference(T, route):
    """every column of both tables within its bar on both voltage routes (c_tables: guards intact, unrequested columns untouched); two runs and
    the one-table requests give the same bits.  Pins `b0 + w < nrow`, `b0 + j < nrow`, `base + b0 + w`, `ty - a.line_tiles` and the pad lanes."""
    r = run_comb(T)
    s, net = r[route], r["net"]
    check_against_ref(f"comb{T}x{r['B']}", route, net, s["vm"], s["va"], s["tables"])
    same_tables(s["tables"], s["again"], "two runs")
    line, trafo = s["tables"]
    for form in ("trafo_only_null", "trafo_only_empty"):              # line_tiles = 0: the trafo tiles start at blockIdx.y = 0
        assert s[form][0] == {}
        same_tables((trafo,), (s[form][1],), form)
    for form in ("line_only_null", "line_only_empty"):
        assert s[form][1] == {}
        same_tables((line,), (s[form][0],), form)
    if T > 1:
        assert all((line[k][:, E.OOS_ROW] == 0).all() for k in R.COLUMNS)
        assert np.array_equal(np.flatnonzero(np.isnan(line["loading_percent"]).any(0)), [E.UNRATED_LINE])
        assert np.array_equal(np.flatnonzero(np.isnan(trafo["loading_percent"]).any(0)), [E.UNRATED_TRAFO])


@pytest.mark.parametrize("T", COMBS)
def test_summary_on_the_combs(T):
    """k_loading_summary over 2T branches (T = 33: eight or nine a wave) against summary_ref of the getter's loadings of the same state"""
    r = run_comb(T)
    s, net = r["reset"], r["net"]
    bar = R.bars(net, s["vm"], s["va"])
    check_summary(f"comb{T}x{r['B']}", "reset", net, s["summary"], s["tables"], bar)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(s["summary"], s["summary_again"]))
    if T > 1:
        wb = s["summary"][1]
        assert ((wb >= 0) & (wb < 2 * T) & (wb != E.OOS_ROW) & (wb != E.UNRATED_LINE) & (wb != T + E.UNRATED_TRAFO)).all()


@pytest.mark.parametrize("T", COMBS)
def test_rows_do_not_depend_on_the_batch(T):
    """an env alone (B = 1, its own env id) and inside the batch: the same state, the same table rows and summary bits"""
    r = run_comb(T)
    for e, one in r["single"].items():
        assert np.array_equal(one["vm"][0], r["reset"]["vm"][e]), "the single env is not in the batch env's state"
        for a, b in zip(one["tables"], r["reset"]["tables"]):
            for k in a:
                assert np.array_equal(a[k][0], b[k][e], equal_nan=True), (T, e, k)
        for a, b in zip(one["summary"], r["reset"]["summary"]):
            assert np.array_equal(a[0], b[e], equal_nan=True), (T, e)


def test_nan_and_zero_voltages_stay_in_their_rows():
    """comb(17) x 129, caller-supplied voltages: vm = NaN at a leaf in env 5, vm = 0 at a leaf in env 70, va = NaN at bus 0 in env 128 — the
    last env, which the pad lanes of the third env tile clamp onto.  Pins the [64][17] LDS transposition and `er = min(e0 + lane, B - 1)`."""
    r = run_comb(17)
    net, a, clean = r["net"], r["altered"], r["solve"]["tables"]
    T, touched = 17, a["touched"]
    err, bar = R.errors(net, a["vm"], a["va"], *a["tables"]), R.bars(net, a["vm"], a["va"])      # rel_err: NaN exactly where the reference has it
    for sl, tab, c, g, e, b in zip((slice(0, T), slice(T, None)), ("line", "trafo"), clean, a["tables"], err, bar):
        print("comb17x129 altered", tab, {k: f"{e[k]:.1e}/{b[k]:.1e}" for k in e})
        for k in R.COLUMNS:
            assert e[k] <= b[k], (tab, k, e[k], b[k])
            assert np.array_equal(c[k][~touched[:, sl]], g[k][~touched[:, sl]], equal_nan=True), (tab, k)      # bitwise the clean call
    line, trafo = a["tables"]
    assert all(np.isnan(line[k][E.NAN_VM]) for k in R.COLUMNS) and all(np.isnan(trafo[k][E.NAN_VA_ENV]).all() for k in R.COLUMNS)
    assert not any(np.isnan(np.delete(line[k], E.UNRATED_LINE, axis=1)[np.arange(129) != E.NAN_VM[0]]).any() for k in R.COLUMNS)
    assert all((line[k][:, E.OOS_ROW] == 0).all() for k in R.COLUMNS)
    assert line["i_to_ka"][E.ZERO_VM] == 0.0 and line["p_to_mw"][E.ZERO_VM] == 0.0 and line["q_to_mvar"][E.ZERO_VM] == 0.0
    assert line["i_from_ka"][E.ZERO_VM] > 0 and line["i_ka"][E.ZERO_VM] == line["i_from_ka"][E.ZERO_VM]


# ---- twins: ties, strictness, re-rating, exact zeros ----------------------------------------------------------------------------------------------
REFUSALS = (("line_df", 4, -0.9), ("br_vn_lv_kv", 0, 0.0), ("line_max_i_ka", 7, np.inf))
STRICT_ENVS = (0, 33, 64)


def set_ratings(env, rset):
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in rset]
    with torch.cuda.device(env.device):
        return env._lib.mapdn_set_branch_ratings(env._h, *[None if a is None else _lib._p(a, _lib._pd) for a in arrs])


_TWINS = {}


def run_twins():
    """one handle of 65 envs after reset; the rating sets applied in turn, then the refused calls, the limits and the flat voltages"""
    if _TWINS:
        return _TWINS
    net, prof = E.make("twins", "D")                                   # created unrated: every rating below arrives through the live handle
    sets = E.rating_sets()
    B = E.TWINS_B
    rows = R.rows_of(prof, B)
    out = dict(net=net)
    env = make_env(net, prof, B)
    try:
        env.reset(start_rows=torch.as_tensor(rows), add_noise=False)
        res = {k: v.cpu().numpy() for k, v in env.results(("vm_pu", "va_degree")).items()}
        out.update(vm=res["vm_pu"], va=res["va_degree"], D0=dict(tables=c_tables(env), summary=c_summary(env)))
        for name, rset in (("A", "A"), ("B", "B"), ("C", "C"), ("D", "D"), ("A2", "A"), ("E", "E"), ("A3", "A")):
            assert set_ratings(env, sets[rset]) == 0, env._lib.mapdn_last_error(env._h)
            out[name] = dict(tables=c_tables(env), summary=c_summary(env))
        out["refused"] = []
        for col, row, x in REFUSALS:                                   # under set A
            bad = [None if a is None else a.copy() for a in sets["A"]]
            bad[E.RATING_FIELDS.index(col)][row] = x
            rc = set_ratings(env, bad)
            out["refused"].append(dict(rc=rc, msg=env._lib.mapdn_last_error(env._h).decode(), tables=c_tables(env), summary=c_summary(env)))
        mx = out["A3"]["summary"][0]
        out["strict"] = {e: (c_summary(env, float(mx[e])), c_summary(env, float(np.nextafter(mx[e], -np.inf)))) for e in STRICT_ENVS}
        out["inf"] = (c_summary(env, np.inf), c_summary(env, -np.inf))
        assert set_ratings(env, sets["A11"]) == 0
        flat = torch.ones(B, 12, dtype=torch.float64, device=DEV)
        out["flat"] = c_tables(env, flat, torch.zeros_like(flat))
    finally:
        env.close()
    _TWINS.update(out)
    return _TWINS


def twin_net(rset):
    return E.make("twins", rset)[0]


def test_twins_against_the_extended_reference():
    r = run_twins()
    for name, rset in (("D0", "D"), ("A", "A"), ("B", "B"), ("C", "C"), ("D", "D"), ("E", "E")):
        check_against_ref("twinsx65", "reset/" + name, twin_net(rset), r["vm"], r["va"], r[name]["tables"])
    same_tables(r["D0"]["tables"], r["D"]["tables"], "unrated again")


def test_a_tie_goes_to_the_lowest_index():
    """set A: rows 3 and 8 tie for the top — wave 0 holds row 8 and must take row 3 from wave 3 (`mq == m && iq < idx`); set B: rows 1 and 9
    tie inside wave 1 (`l > m` keeps the first)"""
    r = run_twins()
    bars = R.bars(twin_net("A"), r["vm"], r["va"])
    for name, (lo, hi) in (("A", E.TWIN_ROWS[0]), ("B", E.TWIN_ROWS[1])):
        line, trafo = r[name]["tables"]
        for a, b in E.TWIN_ROWS:
            assert all(np.array_equal(line[k][:, a], line[k][:, b]) for k in R.COLUMNS), "the twins' rows are the same bits in every column"
        mx, wb, no = r[name]["summary"]
        assert (wb == lo).all(), (name, wb)                              # in every env: no undecided share here
        load = line["loading_percent"][:, lo]
        assert (np.abs(mx - load) <= bars[0]["loading_percent"] * np.abs(line["loading_percent"]).max()).all()
        assert np.array_equal(no, 2 * (load > LIMIT)) and (no == 2).any() and (no == 0).any()      # the twins cross 100 % together, the rest stay below 20 %


def test_partials_without_a_candidate():
    """set C: only the transformer (index n_line, wave 4) is rated — waves 0 to 3 come empty-handed (idx = -1) and wave 0 adopts wave 4's
    candidate; set D: nothing rated"""
    r = run_twins()
    line, trafo = r["C"]["tables"]
    mx, wb, no = r["C"]["summary"]
    assert np.isnan(line["loading_percent"]).all() and np.isfinite(trafo["loading_percent"]).all()
    assert (wb == 12).all() and ((no == 0) | (no == 1)).all()
    bar = R.bars(twin_net("C"), r["vm"], r["va"])[1]["loading_percent"]
    t = trafo["loading_percent"][:, 0]
    assert (np.abs(mx - t) <= bar * np.abs(t).max()).all()
    away = np.abs(t - LIMIT) > bar * np.abs(t).max()
    assert away.all() and np.array_equal(no[away], (t > LIMIT)[away].astype(np.int32))      # consistent with the getter
    for name in ("D0", "D"):
        mx, wb, no = r[name]["summary"]
        assert np.isnan(mx).all() and (wb == -1).all() and (no == 0).all()
        assert all(np.isnan(tab["loading_percent"]).all() for tab in r[name]["tables"])


def test_a_call_replaces_the_ratings_of_the_call_before():
    """mapdn_set_branch_ratings on a live handle (the hipMemcpy of the device records): A, B, C, D and back to A give A's bits again; E = A
    with every line_max_i_ka doubled halves the line loadings exactly and moves nothing else"""
    r = run_twins()
    for again in ("A2", "A3"):
        same_tables(r["A"]["tables"], r[again]["tables"], again)
        assert all(np.array_equal(a, b) for a, b in zip(r["A"]["summary"], r[again]["summary"]))
    assert not np.array_equal(r["A"]["tables"][0]["loading_percent"], r["B"]["tables"][0]["loading_percent"])
    (la, ta), (le, te) = r["A"]["tables"], r["E"]["tables"]
    assert np.array_equal(le["loading_percent"] * 2.0, la["loading_percent"])
    assert all(np.array_equal(la[k], le[k]) for k in R.COLUMNS if k != "loading_percent")
    same_tables((ta,), (te,), "trafo rows under E")
    mxa, wba, _ = r["A"]["summary"]
    mxe, wbe, noe = r["E"]["summary"]
    assert np.array_equal(mxe * 2.0, mxa) and np.array_equal(wba, wbe) and (noe == 0).all()      # 60 %: nothing above 100 any more


def test_a_refused_call_leaves_the_old_ratings_in_place():
    r = run_twins()
    assert len(r["refused"]) == len(REFUSALS)
    for (col, row, x), got in zip(REFUSALS, r["refused"]):
        assert got["rc"] == -1 and f"{col}[{row}]" in got["msg"], (col, row, got["rc"], got["msg"])      # MAPDN_E_INVALID, by column and row
        same_tables(r["A3"]["tables"], got["tables"], col)
        assert all(np.array_equal(a, b) for a, b in zip(r["A3"]["summary"], got["summary"])), col


def test_overloaded_means_strictly_above_the_limit():
    """`l > a.limit`: at limit = max_loading[e], the summary's own output, env e counts nothing; one ulp below, it counts the two twins"""
    r = run_twins()
    mx = r["A3"]["summary"][0]
    for e, (at, below) in r["strict"].items():
        assert at[2][e] == 0 and below[2][e] == 2, (e, at[2][e], below[2][e])
        assert np.array_equal(at[0], mx) and np.array_equal(at[1], r["A3"]["summary"][1])              # the limit moves the count alone
    up, down = r["inf"]
    assert (up[2] == 0).all() and (down[2] == 13).all()                  # +inf: nothing; -inf: every rated in-service branch


def test_flat_voltages_give_exact_zeros():
    """uncharged lines at one voltage: plan.cpp forms yft = -yff bit for bit, so every flow, loss, current and loading of a rated line is 0.0,
    never NaN; the unrated line's loading is NaN; the transformer (ratio, shift, iron) carries current"""
    line, trafo = run_twins()["flat"]
    for k in R.COLUMNS:
        cols = slice(0, 11) if k == "loading_percent" else slice(None)
        assert (line[k][:, cols] == 0.0).all(), k
    assert np.isnan(line["loading_percent"][:, 11]).all()
    assert (trafo["i_from_ka"] > 0).all() and np.isfinite(trafo["loading_percent"]).all()
