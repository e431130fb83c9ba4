"""CPU side of evaluate_actions (mapdn_evaluate_actions): the export, its refusals on a host-only handle, the
reporting function csrc/whatif.hpp::whatif_report — totals -> the reward and the 11 infos of a step — built for the host with g++
(tests/whatif_check.cpp) and held to oracle/env_restated.py::_calc_reward and the oracle's unsolvable branch, and the kernel list of
csrc/whatif.hip."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from mapdn_amd import _lib
from mapdn_amd.netspec import make_case
from oracle.env_restated import BARRIER_IDS, INFO_KEYS, VoltageControlOracle
from tests import whatif_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_STATE = -1, -4
REPORT_TOL = 1e-12


def test_symbol_is_declared_exported_and_linked(lib):
    hdr = open(os.path.join(ROOT, "include", "mapdn.h")).read()
    assert re.search(r"\bint mapdn_evaluate_actions\s*\(", hdr) and "#define MAPDN_WHATIF_MAX_CANDIDATES 1024" in hdr
    assert "mapdn_evaluate_actions" in _lib.EXPORTS
    assert hasattr(lib, "mapdn_evaluate_actions") and lib.mapdn_evaluate_actions.restype is C.c_int


def test_refusals_on_host_only_handle(lib):
    net, _ = make_case("case33")
    cn, keep = _lib.make_cnetspec(net)
    cc = _lib.make_cconfig(dict(episode_limit=240, action_scale=0.8, action_bias=0.0))
    h = C.c_void_p()
    assert lib.mapdn_create(C.byref(cn), C.byref(cc), 4, -1, C.byref(h)) == 0
    one = C.c_void_p(1)                                       # never dereferenced: every call below is refused before any launch
    try:
        def call(actions=one, dtype=_lib.F64, K=3, reward=one, info=one, status=one):
            rc = lib.mapdn_evaluate_actions(h, actions, dtype, K, reward, info, status, None, None, None)
            return rc, lib.mapdn_last_error(h).decode()
        for K in (0, -1, 1025, 2 ** 31 - 1):
            rc, msg = call(K=K)
            assert rc == E_INVALID and msg.startswith("evaluate_actions: n_candidates"), (K, msg)
        for null in ("actions", "reward", "info", "status"):
            rc, msg = call(**{null: None})
            assert rc == E_INVALID and msg.startswith("evaluate_actions: null buffer"), (null, msg)
        for dtype in (-1, 2, 7):
            rc, msg = call(dtype=dtype)
            assert rc == E_INVALID and msg == "evaluate_actions: bad actions dtype", (dtype, msg)
        for K, dtype in ((1, _lib.F64), (1024, _lib.F32)):    # valid arguments stop at the host-only refusal
            rc, msg = call(K=K, dtype=dtype)
            assert rc == E_STATE and "host-only" in msg, (K, msg)
        assert lib.mapdn_evaluate_actions(None, one, _lib.F64, 1, one, one, one, None, None, None) == E_INVALID
    finally:
        lib.mapdn_destroy(h)


def test_kernels_of_whatif_hip_are_the_ones_the_gpu_tests_name():
    found = W.global_kernels()
    assert sorted(found) == sorted(W.KERNELS) and len(found) == len(set(found))
    gpu = open(os.path.join(ROOT, "tests", "test_whatif_gpu.py")).read()
    for k in W.KERNELS:
        assert k in gpu, k
    assert '#include "whatif.hip"' in open(os.path.join(W.CSRC, "kernels.hip")).read()
    from mapdn_amd import build
    assert {"whatif.hip", "whatif.hpp"} <= set(build.HEADERS)


# ---- whatif_report on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_report(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("whatif")
    exe = str(d / "whatif_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "mapdn_amd", "csrc"),
                        os.path.join(ROOT, "tests", "whatif_check.cpp"), "-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(records):
        fi, fo = str(d / "in.bin"), str(d / "out.bin")
        np.concatenate([np.asarray(x, np.float64).ravel() for rec in records for x in rec]).tofile(fi)
        p = subprocess.run([exe, fi, fo], capture_output=True, text=True)
        assert p.returncode == 0, (p.returncode, p.stderr)
        out = np.fromfile(fo, dtype=np.float64).reshape(len(records), 1 + len(INFO_KEYS))
        return out[:, 0], out[:, 1:]
    return run


def _oracle_env(barrier, line_weight, n_sgen):
    """a VoltageControlOracle that holds only what _calc_reward and the unsolvable branch of step() read"""
    o = VoltageControlOracle.__new__(VoltageControlOracle)
    from oracle.env_restated import BARRIERS
    o.voltage_barrier = BARRIERS[barrier]
    o.voltage_weight, o.q_weight, o.line_weight = 1.3, (None if line_weight is not None else 0.1), line_weight
    o.v_lower, o.v_upper = 0.95, 1.05
    return o


def _case(rng, barrier, line_weight, n_bus, n_line, n_sgen, solved, v=None):
    """(record for whatif_check, expected reward, expected infos) of one seeded state"""
    v = rng.uniform(0.9, 1.1, n_bus) if v is None else v
    pl = rng.uniform(0.0, 0.05, n_line)
    scale = rng.uniform(0.5, 1.3, n_sgen)
    q_committed, q_cand = rng.uniform(-1, 1, n_sgen), rng.uniform(-40, 40, n_sgen)
    o = _oracle_env(barrier, line_weight, n_sgen)
    o.res = types.SimpleNamespace(vm_pu=v, pl_mw=pl)
    o.res_sgen_q = (q_cand if solved else q_committed) * scale
    reward, info = o._calc_reward()
    if not solved:                                            # VoltageControlOracle.step, the branch after `else:` (:188-196)
        reward -= 200.
        info["destroy"] = 1.
        info["totally_controllable_ratio"] = 0.
        info["q_loss"] = np.mean(np.abs(q_cand))
    head = [n_bus, n_line, n_sgen, BARRIER_IDS[barrier], float(line_weight is not None), o.voltage_weight,
            0.0 if o.q_weight is None else o.q_weight, 0.0 if line_weight is None else line_weight, o.v_lower, o.v_upper, float(solved)]
    return (head, v, pl, o.res_sgen_q, q_cand), reward, np.array([info[k] for k in INFO_KEYS])


@pytest.mark.parametrize("line_weight", [None, 0.7])
@pytest.mark.parametrize("barrier", sorted(BARRIER_IDS))
def test_report_matches_calc_reward_and_the_unsolvable_branch(host_report, barrier, line_weight):
    rng = np.random.default_rng(sum(map(ord, barrier)) + (1 if line_weight else 0))
    cases = [_case(rng, barrier, line_weight, nb, nl, ns, solved)
             for nb, nl, ns in ((13, 12, 1), (33, 37, 6), (141, 140, 22), (322, 330, 38)) for solved in (True, False) for _ in range(8)]
    reward, info = host_report([c[0] for c in cases])
    for i, (_, r, inf) in enumerate(cases):
        assert abs(reward[i] - r) <= REPORT_TOL, (i, reward[i], r)
        assert np.abs(info[i] - inf).max() <= REPORT_TOL, (i, info[i] - inf)
    solved = np.array([c[0][0][10] for c in cases], bool)
    assert (info[solved, 10] == 0).all() and (info[~solved, 10] == 1).all() and (info[~solved, 3] == 0).all()
    assert (reward[~solved] < -200).all() and (reward[solved] > -5).all()


@pytest.mark.parametrize("side", ["low", "high"])
def test_exactly_one_bus_out_of_band(host_report, side):
    """totally_controllable_ratio is 1 while the share of buses out of band is <= 1e-3: one bus of 33 (1/n > 1e-3) loses it, one of 1500
    (1/n < 1e-3) keeps it; nothing out of band keeps it on both"""
    rng = np.random.default_rng(5)
    cases = []
    for nb in (33, 1500):
        for n_out in (1, 0):
            v = rng.uniform(0.96, 1.04, nb)
            if n_out:
                v[nb // 2] = 0.93 if side == "low" else 1.07
            cases.append((_case(rng, "bowl", None, nb, nb - 1, 4, True, v=v), nb, n_out))
    reward, info = host_report([c[0][0] for c in cases])
    for i, ((_, r, inf), nb, n_out) in enumerate(cases):
        assert abs(reward[i] - r) <= REPORT_TOL and np.abs(info[i] - inf).max() <= REPORT_TOL, (nb, n_out)
        assert info[i, 3] == inf[3] == (0.0 if (n_out and nb == 33) else 1.0), (nb, n_out)
        assert info[i, 0] == n_out / nb and info[i, 1 if side == "low" else 2] == n_out / nb
        assert abs(info[i, 6 if side == "low" else 7] - (0.02 if n_out else 0.0)) < 1e-15 and info[i, 7 if side == "low" else 6] == 0.0
