"""CPU (-m "not gpu") tests of res_line / res_trafo: the arithmetic of mapdn_amd/csrc/branch.hpp compiled for the host
(tests/branch_check.cpp, also under AddressSanitizer + UBSan as a stand-alone program) against the extended-precision reference
(tests/branch_ref.py) and against a closed form; the ratings on NetSpec, through the npz round trip and from_pandapower; the
refusals of mapdn_set_branch_ratings and of the two getters on host-only handles; the testers' opt-in loading record."""
import ctypes as C
import dataclasses
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from mapdn_amd import _lib
from mapdn_amd.baselines import BaselineTester, NoControl
from mapdn_amd.data import from_pandapower, load_netspec, save_netspec
from mapdn_amd.netspec import case33bw_base, make_case
from mapdn_amd.tester import LOADING_RECORD_KEYS, RECORD_KEYS
from oracle.pp_restated import make_ybus, runpp_restated
from tests import branch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0)
RATING_FIELDS = ("line_max_i_ka", "line_df", "br_vn_hv_kv", "br_vn_lv_kv", "br_rating_mva")
N_ENVS = 5                                             # oracle states per case of the host checks


def records(net):
    """the 17 doubles per branch that branch_check reads, from the oracle's Yf / Yt: what plan.cpp puts into a BranchRec"""
    _, yf, yt = make_ybus(net)
    yf, yt = yf.toarray(), yt.toarray()
    on = net.line_in_service.astype(bool)
    row_of = np.full(net.n_line, -1); row_of[on] = np.arange(on.sum())
    df = net.line_df if net.line_df.shape[0] else np.ones(net.n_line)
    rec = []
    for l in range(net.n_line):
        f, t = int(net.line_from_bus[l]), int(net.line_to_bus[l])
        y = [yf[row_of[l], f], yf[row_of[l], t], yt[row_of[l], f], yt[row_of[l], t]] if on[l] else [0j] * 4
        rate = net.line_max_i_ka[l] * df[l] * net.line_parallel[l] if net.line_max_i_ka.shape[0] else np.nan
        rec.append([f, t, float(on[l]), 0.0] + [c for z in y for c in (z.real, z.imag)] + [net.bus_vn_kv[f], net.bus_vn_kv[t], rate, 1.0, 1.0])
    rated = bool(net.br_rating_mva.shape[0] and net.br_vn_hv_kv.shape[0] and net.br_vn_lv_kv.shape[0])
    for k in range(net.n_branch_pu):
        f, t, i = int(net.br_from_bus[k]), int(net.br_to_bus[k]), int(on.sum()) + k
        y = [yf[i, f], yf[i, t], yt[i, f], yt[i, t]]
        tail = [net.br_rating_mva[k], net.br_vn_hv_kv[k], net.br_vn_lv_kv[k]] if rated else [np.nan, 1.0, 1.0]
        rec.append([f, t, 1.0, 1.0] + [c for z in y for c in (z.real, z.imag)] + [net.bus_vn_kv[f], net.bus_vn_kv[t]] + tail)
    return np.array(rec, dtype=np.float64).reshape(-1, 17)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_branch(request, tmp_path_factory):
    """run(net, vm, va, want) -> (line, trafo) dicts of [B, n] columns from branch.hpp on the host"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("branch_" + request.param)
    exe = str(d / "branch_check")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", os.path.join(ROOT, "mapdn_amd", "csrc"),
                        os.path.join(ROOT, "tests", "branch_check.cpp"), "-o", exe, "-lm"], capture_output=True, text=True)
    if r.returncode != 0 and request.param == "sanitized" and "sanitize" in r.stderr:
        pytest.skip("g++ has no sanitizer runtime here")
    assert r.returncode == 0, r.stderr

    def run(net, vm, va, want=0x3ff):
        rec = records(net)
        B, nb = vm.shape
        fi, fo = str(d / "in.bin"), str(d / "out.bin")
        np.concatenate([[rec.shape[0], B, nb, net.sn_mva, want], rec.ravel(), np.ravel(vm), np.ravel(va)]).astype(np.float64).tofile(fi)
        p = subprocess.run([exe, fi, fo], capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stderr)
        out = np.fromfile(fo, dtype=np.float64).reshape(B, rec.shape[0], len(R.COLUMNS))
        return tuple({k: out[:, sl, c] for c, k in enumerate(R.COLUMNS)} for sl in (slice(0, net.n_line), slice(net.n_line, None)))
    return run


@pytest.mark.parametrize("case", R.CASES)
def test_host_arithmetic_against_the_extended_reference(host_branch, case):
    """every column of both tables from branch.hpp (g++) against ref at the oracle's voltages, within 16 x e64 (>= 64 ulp) per column"""
    net, _ = R.make(case)
    vm, va = R.oracle_voltages(case, min(N_ENVS, R.BATCHES[case]))
    got = host_branch(net, vm, va)
    err, bar = R.errors(net, vm, va, *got), R.bars(net, vm, va)
    for tab, e, b in zip(("line", "trafo"), err, bar):
        print(case, tab, {k: f"{e[k]:.1e}/{b[k]:.1e}" for k in e})
        for k in e:
            assert e[k] <= b[k], (case, tab, k, e[k], b[k])


def test_tree8_carries_what_it_claims(host_branch):
    net, _ = R.make("tree8")
    vm, va = R.oracle_voltages("tree8", 3)
    line, trafo = host_branch(net, vm, va)
    assert net.line_parallel[0] == 2 and not net.line_in_service[6] and np.isnan(net.line_max_i_ka[4])
    assert (np.abs(line["i_from_ka"][:, 1] - line["i_to_ka"][:, 1]) > 1e-3 * line["i_ka"][:, 1]).all()       # the cable charges
    assert all((line[k][:, 6] == 0).all() for k in R.COLUMNS)                                                # out of service: 0 everywhere
    assert np.isnan(line["loading_percent"][:, 4]).all() and np.isfinite(np.delete(line["loading_percent"], 4, axis=1)).all()
    assert (line["i_ka"][:, 5] <= 1e-12 * line["i_ka"].max()).all() and (line["loading_percent"][:, 5] <= 1e-9).all()   # the dead end
    assert np.isfinite(trafo["loading_percent"]).all() and (trafo["pl_mw"] > 0).all()                         # copper + iron losses
    assert (np.abs(trafo["i_from_ka"] * 33.0 - trafo["i_to_ka"] * 12.47) > 0).all()


def test_closed_form_on_the_three_bus_feeder(host_branch):
    """two series impedances without charging: I = (Vf - Vt) / z, so Sf, i_ka and loading_percent follow from a chosen V by hand"""
    net, _ = R.make("feeder3")
    vm = np.array([[1.0, 0.97, 0.955], [1.02, 1.0, 1.01]])
    va = np.array([[0.0, -1.2, -1.9], [0.0, 0.4, 1.1]])
    line, trafo = host_branch(net, vm, va)
    assert all(v.shape == (2, 0) for v in trafo.values())
    V = vm * np.exp(1j * np.deg2rad(va))
    zb = 12.47 ** 2 / net.sn_mva
    for l, (f, t) in enumerate(((0, 1), (1, 2))):
        z = (net.line_r_ohm_per_km[l] + 1j * net.line_x_ohm_per_km[l]) * net.line_length_km[l] / zb
        I = (V[:, f] - V[:, t]) / z
        sf, st = V[:, f] * np.conj(I) * net.sn_mva, -V[:, t] * np.conj(I) * net.sn_mva
        i_ka = np.abs(I) * net.sn_mva / (np.sqrt(3.0) * 12.47)
        want = dict(p_from_mw=sf.real, q_from_mvar=sf.imag, p_to_mw=st.real, q_to_mvar=st.imag, pl_mw=(np.abs(I) ** 2 * z.real) * net.sn_mva,
                    ql_mvar=(np.abs(I) ** 2 * z.imag) * net.sn_mva, i_from_ka=i_ka, i_to_ka=i_ka, i_ka=i_ka,
                    loading_percent=100.0 * i_ka / (net.line_max_i_ka[l] * net.line_df[l]))
        for k, w in want.items():
            assert np.abs(line[k][:, l] - w).max() <= 1e-11 * np.abs(w).max(), (l, k)     # V differences of a few 1e-2 lose two digits


def test_zero_apparent_power_gives_zero_current_not_nan(host_branch):
    net, _ = R.make("feeder3")
    line, _ = host_branch(net, np.zeros((1, 3)), np.zeros((1, 3)))                        # |V| = 0: S = 0 over |V| = 0
    assert all((line[k] == 0).all() for k in R.COLUMNS)


@pytest.mark.parametrize("case", ["tree8", "case33_meshed", "case141"])
def test_pl_mw_describes_the_number_of_runpp(host_branch, case):
    """the four-term pl_mw against runpp_restated(...).pl_mw (= Re Sf + Re St in float64) at the oracle's own solution: both are float64
    evaluations of one quantity, so they agree within the kernel's bar plus e64 of that column"""
    net, prof = R.make(case)
    t = int(R.rows_of(prof, 1)[0])
    r = runpp_restated(net, prof.load_p[t], prof.load_q[t], prof.pv[t], np.zeros(net.n_sgen))
    vm, va = r.vm_pu[None], r.va_degree[None]
    line, _ = host_branch(net, vm, va, want=1 << 4)
    e, b = R.e64(net, vm, va)[0]["pl_mw"], R.bars(net, vm, va)[0]["pl_mw"]
    gap = np.abs(line["pl_mw"][0] - r.pl_mw).max() / np.abs(r.pl_mw).max()
    print(case, "gap", gap, "bound", e + b)
    assert gap <= e + b


@pytest.mark.parametrize("case", R.CASES)
def test_top_two_loadings_are_apart(case):
    """worst_branch is compared only where the two largest loadings differ by more than the bar: with the ratings of branch_ref.make the
    reference alone leaves out at most 5 % of a case's envs"""
    net, _ = R.make(case)
    B = R.BATCHES[case]
    vm, va = R.oracle_voltages(case, B)
    line, trafo = R.batch_tables(net, vm, va, np.float64)
    bl, bt = R.bars(net, vm, va)
    bar = max(bl["loading_percent"], bt["loading_percent"])
    *_, gap = R.summary_ref(net, line["loading_percent"], trafo["loading_percent"], 100.0)
    share = float((gap <= 2.0 * bar).mean())
    print(case, "B", B, "smallest gap", gap.min(), "bar", bar, "share left out", share)
    assert share <= 0.05


# ---- NetSpec, npz, from_pandapower ---------------------------------------------------------------------------------------------------------
def test_builtin_cases_carry_no_ratings():
    for net in (make_case("case33")[0], make_case("case141")[0], case33bw_base()[0] if isinstance(case33bw_base(), tuple) else case33bw_base()):
        for k in RATING_FIELDS:
            assert getattr(net, k).shape == (0,), k
        cn, _ = _lib.make_cnetspec(net)                       # the C netspec has no such fields: what mapdn_create sees is what it saw


@pytest.mark.parametrize("rated", [False, True])
def test_netspec_npz_round_trip(tmp_path, rated):
    net = R.make("tree8")[0] if rated else R._base("case33_meshed")[0]
    path = str(tmp_path / "netspec.npz")
    save_netspec(net, path)
    back = load_netspec(path)
    for f in dataclasses.fields(net):
        assert np.array_equal(np.asarray(getattr(net, f.name)), np.asarray(getattr(back, f.name)), equal_nan=f.name in RATING_FIELDS), f.name
    assert all(getattr(back, k).shape[0] == (0 if not rated else n) for k, n in zip(RATING_FIELDS, (7, 7, 1, 1, 1)))
    # a file written before the columns existed loads as before
    z = dict(np.load(path, allow_pickle=False))
    for k in RATING_FIELDS:
        z.pop(k)
    np.savez_compressed(path, **z)
    old = load_netspec(path)
    assert all(getattr(old, k).shape == (0,) for k in RATING_FIELDS)
    assert np.array_equal(old.line_r_ohm_per_km, net.line_r_ohm_per_km)


def test_netspec_refuses_ratings_of_the_wrong_length():
    net = R._base("tree8")[0]
    with pytest.raises(ValueError, match="line_max_i_ka"):
        dataclasses.replace(net, line_max_i_ka=np.ones(3))
    with pytest.raises(ValueError, match="br_rating_mva"):
        dataclasses.replace(net, br_rating_mva=np.ones(2))


def test_from_pandapower_fills_the_ratings():
    from tests.test_data_ingestion import TRAFO, substation_net
    pnet = substation_net(dict(TRAFO, parallel=2, df=0.9))
    pnet["line"]["max_i_ka"] = [0.4, 0.21, np.nan, 0.3]
    pnet["line"]["df"] = [1.0, 0.8, 1.0, np.nan]
    pnet["line"]["parallel"] = [1, 2, 1, 1]
    net = from_pandapower(pnet, hv_init="flat")
    assert np.array_equal(net.line_max_i_ka, [0.4, 0.21, np.nan, 0.3], equal_nan=True)
    assert np.array_equal(net.line_df, [1.0, 0.8, 1.0, 1.0]) and np.array_equal(net.line_parallel, [1, 2, 1, 1])
    assert np.array_equal(net.br_vn_hv_kv, [110.0]) and np.array_equal(net.br_vn_lv_kv, [20.0])       # the nameplate, not the tapped voltage
    assert np.array_equal(net.br_rating_mva, [25.0 * 2 * 0.9])
    assert net.br_from_bus[0] == 0 and net.br_to_bus[0] == 1                                        # from = hv, to = lv
    del pnet["line"]["max_i_ka"]
    assert from_pandapower(pnet, hv_init="flat").line_max_i_ka.shape == (0,)
    # the tables of the converted net: the reference rates line 1 with its parallel, leaves line 2 unrated
    r = runpp_restated(net, np.array([1.0, 0.8, 1.2, 0.5, 0.3]), np.array([0.3, 0.2, 0.4, 0.1, 0.1]), np.array([1.5, 0.7]), np.array([0.2, -0.1]))
    line, trafo = R.tables(net, r.vm_pu, r.va_degree, np.float64)
    assert np.isclose(line["loading_percent"][1], 100.0 * line["i_ka"][1] / (0.21 * 0.8 * 2)) and np.isnan(line["loading_percent"][2])
    assert np.isfinite(trafo["loading_percent"]).all() and trafo["i_from_ka"][0] < trafo["i_to_ka"][0]


# ---- the C ABI on a host-only handle ---------------------------------------------------------------------------------------------------------
def host_handle(lib, net, B=4):
    cn, keep = _lib.make_cnetspec(net)
    cc = _lib.make_cconfig(ARGS)
    h = C.c_void_p()
    assert lib.mapdn_create(C.byref(cn), C.byref(cc), B, -1, C.byref(h)) == 0, lib.mapdn_last_error(None)
    return h, keep


def test_set_branch_ratings_on_a_host_only_handle(lib):
    net = R.make("tree8")[0]
    h, keep = host_handle(lib, net)
    p = lambda a: None if a is None else _lib._p(np.ascontiguousarray(a, dtype=np.float64), _lib._pd)
    good = dict(line_max_i_ka=net.line_max_i_ka, line_df=net.line_df, br_vn_hv_kv=net.br_vn_hv_kv, br_vn_lv_kv=net.br_vn_lv_kv, br_rating_mva=net.br_rating_mva)
    call = lambda **kw: lib.mapdn_set_branch_ratings(h, *[p(kw.get(k, good[k])) for k in RATING_FIELDS])
    try:
        assert call() == 0                                                   # a NaN in line_max_i_ka: that line stays unrated
        assert lib.mapdn_set_branch_ratings(h, None, None, None, None, None) == 0
        assert call(line_df=None) == 0 and call(br_rating_mva=None) == 0
        bad = lambda v, i, x: np.where(np.arange(len(v)) == i, x, v)
        for k, i, x in (("line_max_i_ka", 2, 0.0), ("line_max_i_ka", 5, -0.1), ("line_max_i_ka", 1, np.inf), ("line_df", 3, np.nan), ("line_df", 0, 0.0),
                        ("br_vn_hv_kv", 0, np.nan), ("br_vn_lv_kv", 0, -20.0), ("br_rating_mva", 0, 0.0), ("br_rating_mva", 0, -np.inf)):
            assert call(**{k: bad(good[k], i, x)}) == -1, (k, i, x)
            msg = lib.mapdn_last_error(h).decode()
            assert f"{k}[{i}]" in msg, msg                                   # the refusal names the column and the row
        # the getters: refused as mapdn_reset is on such a handle (MAPDN_E_STATE), whichever voltage route
        out = _lib.CBranchOut()
        assert lib.mapdn_reset(h, None, 0, 1, None) == -4
        assert lib.mapdn_get_branch_results(h, None, None, C.byref(out), C.byref(out), None) == -4
        assert lib.mapdn_get_branch_results(h, C.c_void_p(8), C.c_void_p(8), C.byref(out), None, None) == -4
        assert lib.mapdn_get_branch_results(h, C.c_void_p(8), None, C.byref(out), None, None) == -1      # exactly one of the two
        assert lib.mapdn_get_branch_results(h, None, C.c_void_p(8), C.byref(out), None, None) == -1
        assert lib.mapdn_get_loading_summary(h, 100.0, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None) == -4
        assert lib.mapdn_set_branch_ratings(None, None, None, None, None, None) == -1
    finally:
        lib.mapdn_destroy(h)


def test_branch_out_struct_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "mapdn.h")).read()
    body = hdr[hdr.index("typedef struct mapdn_branch_out {"):hdr.index("} mapdn_branch_out;")]
    names = [w.strip(" *,;\n") for w in body.split("double", 1)[1].replace("\n", " ").split(",")]
    assert tuple(n for n in names if n) == _lib.BRANCH_COLUMNS == R.COLUMNS
    assert C.sizeof(_lib.CBranchOut) == 8 * len(R.COLUMNS)
    assert "pf_res_plot.py:142-150" in hdr and "pf_res_plot.py:161-163" in hdr


# ---- the testers' record ----------------------------------------------------------------------------------------------------------------------
class ScriptedEnv:
    """what BaselineTester touches of a VoltageControlBatch, on the CPU: B envs, step t reports loading 40 + 30 t per cent on line 0"""
    n_envs, n_sgen, n_line, n_trafo, device = 3, 2, 4, 1, torch.device("cpu")

    def __init__(self):
        self.t = 0

    def reset(self):
        self.t = 0

    def manual_reset(self, day, hour, interval):
        self.t = 0

    def step(self, actions, add_noise=True):
        self.t += 1
        return torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.bool), torch.full((3, 11), float(self.t), dtype=torch.float64)

    def results(self, keys=None):
        w = dict(vm_pu=5, va_degree=5, p_mw=5, q_mvar=5, pl_mw=4, sgen_p=2, sgen_q=2)
        return {k: torch.full((3, n), float(self.t), dtype=torch.float64) for k, n in w.items()}

    def _loading(self):
        x = torch.full((3, 4), 10.0, dtype=torch.float64)
        x[:, 0] = 40.0 + 30.0 * self.t
        return x

    def res_line(self, keys=None, **kw):
        return {"loading_percent": self._loading()}

    def res_trafo(self, keys=None, **kw):
        return {"loading_percent": torch.full((3, 1), 55.0, dtype=torch.float64)}

    def loading_summary(self, limit_percent=100.0):
        x = torch.cat([self._loading(), torch.full((3, 1), 55.0, dtype=torch.float64)], 1)
        return x.max(1).values, x.argmax(1).int(), (x > limit_percent).sum(1).int()


def test_tester_record_keys_default_and_opt_in():
    args = types.SimpleNamespace(max_steps=4)
    plain = BaselineTester(args, NoControl(), ScriptedEnv())
    rec = plain.run(0, 12, 0)
    assert list(rec) == list(RECORD_KEYS) and all(len(v) == 5 for v in rec.values())          # the reference's keys, nothing else
    stat = plain.batch_run(3)
    assert list(stat) == ["mean_test_" + k for k in _lib.INFO_KEYS]
    opt = BaselineTester(args, NoControl(), ScriptedEnv(), record_loading=True)
    rec2 = opt.run(0, 12, 0)
    assert list(rec2) == list(RECORD_KEYS) + list(LOADING_RECORD_KEYS)
    assert all(np.array_equal(a, b) for k in RECORD_KEYS for a, b in zip(rec[k], rec2[k]))
    assert [float(x[0]) for x in rec2["line_loading"]] == [40.0, 70.0, 100.0, 130.0, 160.0] and rec2["trafo_loading"][0].shape == (1,)
    stat2 = opt.batch_run(3)
    assert list(stat2)[:len(stat)] == list(stat) and all(stat2[k] == stat[k] for k in stat)
    assert list(stat2)[len(stat):] == ["mean_test_max_loading_percent", "mean_test_overloaded_steps_ratio"]
    assert stat2["mean_test_max_loading_percent"][0] == pytest.approx(np.mean([70.0, 100.0, 130.0, 160.0]))
    assert stat2["mean_test_overloaded_steps_ratio"][0] == pytest.approx(0.5)                  # 130 and 160 are above 100, 100 is not


def test_pgtester_takes_the_same_switch():
    import inspect
    from mapdn_amd.tester import PGTester
    for cls in (PGTester, BaselineTester):
        sig = inspect.signature(cls.__init__)
        assert sig.parameters["record_loading"].default is False
