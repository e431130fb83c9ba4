"""GPU (-m gpu) tests of res_line / res_trafo (csrc/branch.hip) through the C ABI between sentinel guards: k_branch_results on both voltage
routes — caller-supplied voltages fed from solve(), env state after reset() and after a few step()s — against the extended-precision
reference at the kernel's own input voltages (tests/branch_ref.py: every column within 16 x e64, never below 64 ulp), k_loading_summary
against the getter's loading_percent of the same state, bit-identical repeats, batch-size independence of the summary's bits, and the
Python surface (VoltageControlBatch.res_line / res_trafo / loading_summary, the B = 1 getters) against the C route.

Nets (tests/branch_ref.py): the 3-bus feeder; an 8-node tree with a ratio-and-shift transformer with iron losses, a shunt, a parallel = 2
line, a cable whose i_from != i_to, an out-of-service line, an unrated line and a dead end without current; case33 with five tie lines
closed (the sparse solver); case33 with fused buses and a line that ends on a fused (non-representative) bus; case141 (140 rows: nine
branch tiles).  Batches 1, 17, 3, 33 and 65 envs: the padding to 64 and a second env tile."""
import ctypes as C

import numpy as np
import pytest
import torch

from mapdn_amd import _lib
from mapdn_amd.env import VoltageControl, VoltageControlBatch
from tests import branch_ref as R

pytestmark = pytest.mark.gpu

ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0, voltage_barrier_type="bowl", seed=0)
DEV = "cuda:0"
GUARD, SENT = 64, -7.25e300                     # doubles before and after every output array, and what they (and the array) hold before a call
LIMIT = 100.0
PL_RESULTS_BAR_MW = 1e-9                        # what tests/test_gpu_parity.py holds results()["pl_mw"] to against the oracle


class Guarded:
    """a device array of `shape` between two guard zones, all SENT"""

    def __init__(self, shape, dtype=torch.float64):
        self.shape, self.n = shape, int(np.prod(shape))
        self.sent = SENT if dtype == torch.float64 else -77
        self.buf = torch.full((self.n + 2 * GUARD,), self.sent, dtype=dtype, device=DEV)
        self.ptr = self.buf.data_ptr() + GUARD * self.buf.element_size()

    def get(self):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == self.sent).all() and (b[GUARD + self.n:] == self.sent).all(), "guard zone written"
        return b[GUARD:GUARD + self.n].reshape(self.shape).copy()


def make_env(net, prof, B, **kw):
    return VoltageControlBatch(net, prof, dict(ARGS), n_envs=B, device=DEV, obs_dtype=torch.float64, **kw)


def c_tables(env, vm=None, va=None, line_cols=R.COLUMNS, trafo_cols=R.COLUMNS, null=()):
    """mapdn_get_branch_results through ctypes; every column of the struct gets a guarded array, only the requested ones are handed over.
    Returns (line, trafo): dicts of the requested columns; the others must still hold the sentinel.  null: the tables ("line", "trafo")
    whose struct pointer itself is NULL (their columns must be empty)."""
    assert not (("line" in null and line_cols) or ("trafo" in null and trafo_cols))
    B = env.n_envs
    tabs = []
    for cols, n in ((line_cols, env.n_line), (trafo_cols, env.n_trafo)):
        g = {k: Guarded((B, n)) for k in R.COLUMNS}
        s = _lib.CBranchOut()
        for k in cols:
            setattr(s, k, g[k].ptr)
        tabs.append((g, s, cols))
    with torch.cuda.device(env.device):
        rc = env._lib.mapdn_get_branch_results(env._h, None if vm is None else vm.data_ptr(), None if va is None else va.data_ptr(),
                                               None if "line" in null else C.byref(tabs[0][1]), None if "trafo" in null else C.byref(tabs[1][1]),
                                               env._stream())
    _lib.check(rc, env._h)
    torch.cuda.synchronize()
    out = []
    for g, _, cols in tabs:
        got = {k: g[k].get() for k in R.COLUMNS}
        for k in R.COLUMNS:
            if k not in cols:
                assert (got[k] == SENT).all(), ("a column that was not asked for was written", k)
        out.append({k: got[k] for k in cols})
    return tuple(out)


def c_summary(env, limit=LIMIT):
    B = env.n_envs
    mx, wb, no = Guarded((B,)), Guarded((B,), torch.int32), Guarded((B,), torch.int32)
    with torch.cuda.device(env.device):
        _lib.check(env._lib.mapdn_get_loading_summary(env._h, limit, mx.ptr, wb.ptr, no.ptr, env._stream()), env._h)
    torch.cuda.synchronize()
    return mx.get(), wb.get(), no.get()


def same_tables(x, y, what):
    for a, b in zip(x, y):
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def check_against_ref(case, route, net, vm, va, got):
    """every column of both tables within its bar of the extended reference at vm, va — the arrays the kernel was given"""
    assert np.isfinite(vm).all() and np.isfinite(va).all()
    err, bar = R.errors(net, vm, va, *got), R.bars(net, vm, va)
    for tab, e, b in zip(("line", "trafo"), err, bar):
        print(case, route, tab, {k: f"{e[k]:.1e}/{b[k]:.1e}" for k in e})
        for k in e:
            assert e[k] <= b[k], (case, route, tab, k, e[k], b[k])
    return bar


def check_summary(case, route, net, got, tables, bar):
    """max_loading and n_overloaded against the getter's loading_percent of the same state; worst_branch where the top two are apart"""
    line, trafo = tables
    mx, wb, no = got
    scale = np.nanmax(np.abs(np.concatenate([line["loading_percent"], trafo["loading_percent"]], 1)))
    tol = max(bar[0]["loading_percent"], bar[1]["loading_percent"]) * scale
    rmx, rwb, _, gap = R.summary_ref(net, line["loading_percent"], trafo["loading_percent"], LIMIT)
    assert np.abs(mx - rmx).max() <= tol, (case, route)
    lo = R.summary_ref(net, line["loading_percent"], trafo["loading_percent"], LIMIT + tol)[2]
    hi = R.summary_ref(net, line["loading_percent"], trafo["loading_percent"], LIMIT - tol)[2]
    assert ((lo <= no) & (no <= hi)).all(), (case, route)
    decided = gap * np.abs(rmx) > 2.0 * tol
    print(case, route, "max_loading", mx[:3], "overloaded", no[:3], "undecided envs", int((~decided).sum()))
    assert (~decided).mean() <= 0.05 and np.array_equal(wb[decided], rwb[decided]), (case, route)
    assert (no > 0).any() or case == "feeder3"                    # the ratings put some branch above the limit


_RUNS = {}


def run(case):
    """the case's batch through all routes, once, shared by the tests below"""
    if case in _RUNS:
        return _RUNS[case]
    net, prof = R.make(case)
    B = R.BATCHES[case]
    rows = R.rows_of(prof, B)
    rng = np.random.default_rng(B)
    out = dict(net=net, prof=prof, rows=rows)
    env = make_env(net, prof, B)
    try:
        # route 1: the caller's voltages, straight from solve() — before any reset: env state is neither read nor needed
        q = 0.5 * rng.uniform(-1, 1, (B, net.n_sgen)) * np.sqrt(np.maximum(prof.s_max(1.2) ** 2 - prof.pv[rows] ** 2, 0.0))
        vm, va, _, conv = env.solve(prof.load_p[rows], prof.load_q[rows], prof.pv[rows], q)
        assert bool(conv.all())
        out["solve"] = dict(vm=vm.cpu().numpy(), va=va.cpu().numpy(), tables=c_tables(env, vm, va), again=c_tables(env, vm, va),
                            subset=c_tables(env, vm, va, ("pl_mw", "loading_percent"), ("i_to_ka",)),
                            trafo_only=c_tables(env, vm, va, (), ("ql_mvar", "i_from_ka")))
        # route 2: env state
        env.reset(start_rows=torch.as_tensor(rows), add_noise=False)
        for key, steps in (("reset", 0), ("steps", 3)):
            for _ in range(steps):
                env.step(torch.as_tensor(rng.uniform(-0.8, 0.8, (B, net.n_sgen)), device=DEV))
            res = {k: v.cpu().numpy() for k, v in env.results(("vm_pu", "va_degree", "pl_mw")).items()}
            out[key] = dict(vm=res["vm_pu"], va=res["va_degree"], pl=res["pl_mw"], tables=c_tables(env), again=c_tables(env),
                            summary=c_summary(env), summary_again=c_summary(env),
                            py_line={k: v.cpu().numpy() for k, v in env.res_line().items()},
                            py_trafo={k: v.cpu().numpy() for k, v in env.res_trafo().items()},
                            py_summary=tuple(x.cpu().numpy() for x in env.loading_summary(LIMIT)))
    finally:
        env.close()
    _RUNS[case] = out
    return out


@pytest.mark.parametrize("case", R.CASES)
def test_caller_supplied_voltages_against_the_extended_reference(case):
    r = run(case)
    s = r["solve"]
    check_against_ref(case, "solve", r["net"], s["vm"], s["va"], s["tables"])
    same_tables(s["tables"], s["again"], "two runs")
    for tab, sub in zip(s["tables"], s["subset"]):                 # a subset of the columns: the same bits, nothing else written (c_tables)
        for k in sub:
            assert np.array_equal(tab[k], sub[k], equal_nan=True), k
    assert s["trafo_only"][0] == {} and all(np.array_equal(s["tables"][1][k], v, equal_nan=True) for k, v in s["trafo_only"][1].items())


@pytest.mark.parametrize("route", ["reset", "steps"])
@pytest.mark.parametrize("case", R.CASES)
def test_env_state_against_the_extended_reference(case, route):
    r = run(case)
    s, net = r[route], r["net"]
    bar = check_against_ref(case, route, net, s["vm"], s["va"], s["tables"])
    same_tables(s["tables"], s["again"], "two runs")
    # res_line.pl_mw is the number results() reports: within this column's bar plus the one results()["pl_mw"] is held to
    pl = s["tables"][0]["pl_mw"]
    assert np.abs(pl - s["pl"]).max() <= bar[0]["pl_mw"] * np.abs(pl).max() + PL_RESULTS_BAR_MW
    check_summary(case, route, net, s["summary"], s["tables"], bar)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(s["summary"], s["summary_again"]))


def test_special_rows_of_the_tree():
    r = run("tree8")
    for route in ("solve", "reset", "steps"):
        line, trafo = r[route]["tables"]
        assert all((line[k][:, 6] == 0).all() for k in R.COLUMNS)                       # out of service
        assert np.isnan(line["loading_percent"][:, 4]).all()                            # unrated
        assert np.isfinite(np.delete(line["loading_percent"], 4, axis=1)).all() and np.isfinite(trafo["loading_percent"]).all()
        assert (line["i_ka"][:, 5] <= 1e-9 * line["i_ka"].max()).all() and not np.isnan(line["i_ka"]).any()      # the dead end
        assert (np.abs(line["i_from_ka"][:, 1] - line["i_to_ka"][:, 1]) > 1e-3 * line["i_ka"][:, 1]).all()       # the cable
    mx, wb, no = r["reset"]["summary"]
    assert (wb != 4).all() and (wb != 6).all() and (wb >= 0).all()                      # never the unrated or the dead line


def test_fused_buses_share_their_voltage():
    r = run("case33_fused")
    net = r["net"]
    li = int(np.flatnonzero(net.line_to_bus >= 33)[0])                                   # the line that ends on a fused, non-representative bus
    for route in ("solve", "reset"):
        s = r[route]
        assert np.array_equal(s["vm"][:, net.line_to_bus[li]], s["vm"][:, net.bus_alias[net.line_to_bus[li]]])
        assert (s["tables"][0]["i_ka"][:, li] > 0).all()


@pytest.mark.parametrize("case", R.CASES)
def test_python_surface_agrees_with_the_c_route(case):
    r = run(case)
    for route in ("reset", "steps"):
        s = r[route]
        line, trafo = s["tables"]
        for k in R.COLUMNS:
            assert np.array_equal(s["py_line"][k], line[k], equal_nan=True), k
        for k, name in R.TRAFO_NAMES.items():
            assert np.array_equal(s["py_trafo"][name], trafo[k], equal_nan=True), name
        assert set(s["py_trafo"]) == set(R.TRAFO_NAMES.values())
        net = r["net"]
        assert np.array_equal(s["py_line"]["vm_from_pu"], s["vm"][:, net.line_from_bus]) and np.array_equal(s["py_line"]["va_to_degree"], s["va"][:, net.line_to_bus])
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(s["py_summary"], s["summary"]))


def test_summary_bits_do_not_depend_on_the_batch():
    """an env alone (B = 1, its own env id) and the same env inside the batch of 33: the same state, the same summary bits and tables"""
    r = run("case33_fused")
    net, prof, rows = r["net"], r["prof"], r["rows"]
    for e in (0, 17, 32):
        env = make_env(net, prof, 1, env_id_offset=e)
        try:
            env.reset(start_rows=torch.as_tensor(rows[e:e + 1]), add_noise=False)
            vm = env.results(("vm_pu",))["vm_pu"].cpu().numpy()
            assert np.array_equal(vm[0], r["reset"]["vm"][e]), "the single env is not in the batch env's state"
            one, tabs = c_summary(env), c_tables(env)
        finally:
            env.close()
        for a, b in zip(one, r["reset"]["summary"]):
            assert np.array_equal(a[0], b[e], equal_nan=True), e
        for a, b in zip(tabs, r["reset"]["tables"]):
            for k in a:
                assert np.array_equal(a[k][0], b[k][e], equal_nan=True), (e, k)


def test_unrated_net_and_refusals():
    net, prof = R._base("case33_meshed")                             # no ratings at all
    env = make_env(net, prof, 3)
    try:
        with pytest.raises(_lib.MapdnError) as ei:
            env.res_line()
        assert ei.value.code == -4                                   # env state before reset
        with pytest.raises(_lib.MapdnError) as ei:
            env.loading_summary()
        assert ei.value.code == -4
        env.reset()
        assert torch.isnan(env.res_line(("loading_percent",))["loading_percent"]).all()
        assert env.res_trafo()["loading_percent"].shape == (3, 0)
        mx, wb, no = (x.cpu().numpy() for x in env.loading_summary())
        assert np.isnan(mx).all() and (wb == -1).all() and (no == 0).all()
        with pytest.raises(ValueError):
            env.res_line(vm_pu=torch.ones(3, 33, dtype=torch.float64, device=DEV))
        with pytest.raises(KeyError):
            env.res_line(("i_hv_ka",))
    finally:
        env.close()


def test_drop_in_getters():
    net, prof = R.make("tree8")
    vc = VoltageControl(dict(ARGS, net=net, profiles=prof), device=DEV)
    try:
        vc.step(vc.get_action())
        line, trafo = c_tables(vc._b, line_cols=("loading_percent",), trafo_cols=("loading_percent",))
        a, b = vc._get_res_line_loading(), vc._get_res_trafo_loading()
        assert isinstance(a, np.ndarray) and a.shape == (7,) and b.shape == (1,)
        assert np.array_equal(a, line["loading_percent"][0], equal_nan=True) and np.array_equal(b, trafo["loading_percent"][0])
        assert np.array_equal(vc._get_res_line_loss(), vc._b.results(("pl_mw",))["pl_mw"][0].cpu().numpy())
    finally:
        vc.close()
