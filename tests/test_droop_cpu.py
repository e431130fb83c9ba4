"""CPU (-m "not gpu") tests of the droop baseline: the law, the damped update, the norm's terms and the reactive_ratio target of
mapdn_amd/csrc/droop.hpp compiled for the host against the numpy restatement (tests/droop_ref.py) bit for bit, the restated loop against the fixed point a = f(v(a)) that a bisection finds on a
3-bus feeder, and the config refusals of mapdn_droop_actions on a host-only handle."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from mapdn_amd import _lib
from mapdn_amd.baselines import DroopConfig
from mapdn_amd.netspec import NetSpec, make_case
from oracle.pp_restated import runpp_restated
from tests.droop_ref import damped, droop_ref, law, target

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = (0.95, 1.0, 1.0, 1.05)
DEADBAND = (0.95, 0.98, 1.02, 1.05)


@pytest.mark.parametrize("bp,table", [
    (DEFAULT, [(0.90, 1.0), (0.95, 1.0), (0.975, 0.5), (1.0, 0.0), (1.025, -0.5), (1.05, -1.0), (1.10, -1.0)]),
    (DEADBAND, [(0.95, 1.0), (0.965, 0.5), (0.98, 0.0), (1.0, 0.0), (1.02, 0.0), (1.035, -0.5), (1.05, -1.0), (1.06, -1.0)]),
])
def test_law_table(bp, table):
    for v, want in table:
        assert abs(float(law(v, *bp)) - want) < 1e-12, (bp, v)
    # the branches are taken in the script's order: v == va is +1, v == vd is the falling slope's end (-1), the deadband is closed
    assert law(bp[0], *bp) == 1.0 and law(bp[2], *bp) == 0.0 and law(bp[1], *bp) == 0.0
    assert law(np.nextafter(bp[3], 2.0), *bp) == -1.0


def _voltages(bp, n=10000, seed=0):
    rng = np.random.default_rng(seed)
    edges = np.array([x for b in bp for x in (b, np.nextafter(b, 0.0), np.nextafter(b, 2.0))])
    return np.concatenate([edges, rng.uniform(0.85, 1.15, n - edges.size)])


@pytest.fixture(scope="module")
def host_law(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("droop")
    exe = str(d / "droop_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "mapdn_amd", "csrc"),
                        os.path.join(ROOT, "tests", "droop_check.cpp"), "-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(rec):
        fi, fo = str(d / "in.bin"), str(d / "out.bin")
        np.ascontiguousarray(rec, dtype=np.float64).tofile(fi)
        p = subprocess.run([exe, fi, fo], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        return np.fromfile(fo, dtype=np.float64).reshape(-1, 4)
    return run


@pytest.mark.parametrize("bp", [DEFAULT, DEADBAND])
def test_device_header_matches_reference_bit_for_bit(host_law, bp):
    v = _voltages(bp)
    rng = np.random.default_rng(1)
    a = rng.uniform(-1.0, 1.0, v.size)
    damping = rng.choice([0.1, 0.25, 1.0], v.size)
    v_last = v + rng.normal(0.0, 1e-3, v.size)
    rec = np.column_stack([v, np.tile(bp, (v.size, 1)), a, damping, v_last, np.ones((v.size, 4))])
    out = host_law(rec)
    f = law(v, *bp)
    assert np.array_equal(out[:, 0].view(np.uint64), f.view(np.uint64))
    assert np.array_equal(out[:, 1].view(np.uint64), damped(a, f, damping).view(np.uint64))
    assert np.array_equal(out[:, 2].view(np.uint64), (0.25 + (v - v_last) * (v - v_last)).view(np.uint64))


def test_device_target_matches_reference_bit_for_bit(host_law):
    """droop_target = f * fmin(1, ratio * smax / lim) against droop_ref.target: ratio 0.3 / 1 / 2, lim from 0 (inf inside the fmin) through
    denormal and tiny values to smax itself and its neighbours, f = +-1, +-0, slope values and the law's own output"""
    rng = np.random.default_rng(2)
    smax0 = np.array([1e-3, 0.37, 1.0, 2.4, 96.0])
    lim_of = lambda sm: np.concatenate([[0.0, 5e-324, 1e-310, 1e-300, 1e-30, 1e-9, 0.3 * sm, np.nextafter(0.3 * sm, 0.0), np.nextafter(0.3 * sm, 9.0),
                                         0.5 * sm, np.nextafter(sm, 0.0), sm], sm * np.sqrt(1.0 - rng.uniform(0.0, 1.0, 24) ** 2)])
    fs = np.concatenate([[1.0, -1.0, 0.0, -0.0, 0.5, -0.5, 1.0 / 3.0, -2.0 / 3.0], law(rng.uniform(0.93, 1.07, 16), *DEADBAND)])
    rows = [(f, ratio, sm, lim) for ratio in (0.3, 1.0, 2.0) for sm in smax0 for lim in lim_of(sm) for f in fs]
    q = np.array(rows)
    rec = np.column_stack([np.ones((q.shape[0], 8)), q])
    rec[:, 1:5] = DEFAULT
    out = host_law(rec)
    want = target(q[:, 0], q[:, 1], q[:, 2], q[:, 3])
    assert np.array_equal(out[:, 3].view(np.uint64), want.view(np.uint64))
    assert np.isfinite(want).all() and (np.abs(want) <= np.abs(q[:, 0])).all()
    with np.errstate(divide="ignore", over="ignore"):
        binds = q[:, 1] * q[:, 2] / q[:, 3] < 1.0
    assert binds[q[:, 1] == 0.3].any() and not binds[q[:, 1] >= 1.0].any()      # the min binds under ratio 0.3 alone
    one = (q[:, 1] >= 1.0)
    assert np.array_equal(want[one].view(np.uint64), q[one, 0].view(np.uint64))  # ratio >= 1: the factor is exactly 1


def three_bus():
    """slack -- 1 -- 2 at 12.66 kV, loads at 1 and 2, one sgen at 2"""
    i32, f64 = np.int32, np.float64
    return NetSpec(name="three_bus", bus_vn_kv=np.full(3, 12.66), bus_zone=np.array([0, 1, 1], i32),
                   line_from_bus=np.array([0, 1], i32), line_to_bus=np.array([1, 2], i32),
                   line_r_ohm_per_km=np.array([0.9, 1.2], f64), line_x_ohm_per_km=np.array([0.6, 0.9], f64),
                   line_c_nf_per_km=np.zeros(2), line_g_us_per_km=np.zeros(2), line_length_km=np.ones(2),
                   line_parallel=np.ones(2, i32), line_in_service=np.ones(2, np.uint8),
                   load_bus=np.array([1, 2], i32), sgen_bus=np.array([2], i32), sgen_zone=np.array([1], i32))


def test_loop_converges_to_the_fixed_point():
    net = three_bus()
    lp, lq, pv, smax = np.array([1.2, 1.0]), np.array([0.5, 0.4]), np.array([0.3]), np.array([1.5])
    lim = np.sqrt(smax * smax - pv * pv)
    cfg = DroopConfig(v_tol=1e-12, max_iter=20000)
    r = droop_ref(net, lp, lq, pv, smax, cfg)
    assert r.status == 0, r

    def g(a):                                         # a - f(v(a)): increasing in a, one root in [-1, 1]
        v = runpp_restated(net, lp, lq, pv, lim * np.array([a])).vm_pu[2]
        return a - float(law(v, *DEFAULT))
    lo, hi = -1.0, 1.0
    assert g(lo) < 0.0 < g(hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if g(mid) < 0.0 else (lo, mid)
    a_star = 0.5 * (lo + hi)
    assert 0.05 < a_star < 0.95                       # the fixed point lies on the law's rising slope, not at a saturation
    assert abs(r.actions[0] - a_star) < 1e-9, (r.actions[0], a_star, r.iterations)


def test_defaults_need_at_least_two_solves():
    net, prof = make_case("case33")
    t = 1000
    r = droop_ref(net, prof.load_p[t], prof.load_q[t], prof.pv[t], prof.s_max(1.2))
    assert r.status in (0, 1) and r.iterations >= 2


BAD = [dict(va=1.0), dict(vb=1.06), dict(vc=0.99), dict(vd=1.0), dict(va=0.99, vb=0.98), dict(damping=-0.1), dict(damping=1.5),
       dict(max_iter=-1), dict(max_iter=10001), dict(v_tol=-1e-4), dict(reactive_ratio=-1.0)]


def test_config_refusals_on_host_only_handle(lib):
    net, _ = make_case("case33")
    cn, keep = _lib.make_cnetspec(net)
    cc = _lib.make_cconfig(dict(episode_limit=240, action_scale=0.8, action_bias=0.0))
    h = C.c_void_p()
    assert lib.mapdn_create(C.byref(cn), C.byref(cc), 4, -1, C.byref(h)) == 0
    try:
        for bad in BAD:
            dc = _lib.make_droop_config(bad)
            rc = lib.mapdn_droop_actions(h, C.byref(dc), None, None, None, None, None)
            assert rc == -1, bad                                          # MAPDN_E_INVALID
            assert lib.mapdn_last_error(h).decode().startswith("droop:"), bad
        # a valid config (all zero = the script's values; a deadband) passes the check and stops at the host-only refusal
        for ok in (None, dict(vb=0.98, vc=1.02, damping=1.0, max_iter=10000)):
            dc = _lib.make_droop_config(ok)
            rc = lib.mapdn_droop_actions(h, C.byref(dc), None, None, None, None, None)
            assert rc == -1 and "null buffer" in lib.mapdn_last_error(h).decode()
            one = C.c_void_p(1)
            assert lib.mapdn_droop_actions(h, C.byref(dc), one, None, one, one, None) == -4      # MAPDN_E_STATE: host-only
    finally:
        lib.mapdn_destroy(h)


def test_make_droop_config_rejects_unknown_keys():
    with pytest.raises(KeyError):
        _lib.make_droop_config(dict(v_tolerance=1e-3))
    c = _lib.make_droop_config(DroopConfig(max_iter=7))
    assert c.max_iter == 7 and c.va == 0.95 and c.v_tol == 1e-4
