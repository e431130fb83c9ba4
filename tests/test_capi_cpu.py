"""CPU (-m "not gpu") tests of the C-ABI library: it loads, exports every symbol of include/mapdn.h,
and its HOST side (per-unit Ybus, elimination plan, integer gather tables) matches the oracle.
No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mapdn_amd import _lib
from mapdn_amd.netspec import make_case
from oracle.pp_restated import make_ybus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0)


def host_handle(lib, net, args=ARGS, B=4):
    cn, keep = _lib.make_cnetspec(net)
    cc = _lib.make_cconfig(args)
    h = C.c_void_p()
    rc = lib.mapdn_create(C.byref(cn), C.byref(cc), B, -1, C.byref(h))
    return rc, h


def test_exports_match_header(lib):
    hdr = open(os.path.join(ROOT, "include", "mapdn.h")).read()
    declared = set(re.findall(r"\b(mapdn_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name


@pytest.mark.parametrize("case", ["case33", "case141", "case322"])
def test_host_ybus_matches_oracle(lib, case):
    net, _ = make_case(case)
    rc, h = host_handle(lib, net)
    assert rc == 0, lib.mapdn_last_error(None)
    out = np.zeros((net.n_bus, net.n_bus, 2))
    assert lib.mapdn_get_ybus_dense(h, _lib._p(out, _lib._pd)) == 0
    y = out[..., 0] + 1j * out[..., 1]
    yo = make_ybus(net)[0].toarray()
    assert np.abs(y - yo).max() <= 1e-12 * np.abs(yo).max()
    assert np.array_equal(y != 0, yo != 0)          # sparsity pattern bit-exact
    lib.mapdn_destroy(h)


@pytest.mark.parametrize("case", ["case33", "case141", "case322"])
def test_obs_index_tables_bit_exact(lib, case):
    """zone masks / gather indices / padding are integer artefacts: must equal the oracle's exactly"""
    net, _ = make_case(case)
    rc, h = host_handle(lib, net)
    assert rc == 0
    dims = _lib.CDims()
    assert lib.mapdn_dims(h, C.byref(dims)) == 0
    assert dims.obs_size == net.obs_size() and dims.state_size == net.state_size()
    assert dims.n_agents == net.n_sgen and dims.n_actions == 1 and dims.n_info == 11 and dims.is_radial == 1
    n = dims.n_agents * dims.obs_size
    kind = np.zeros(n, np.int32)
    idx = np.zeros(n, np.int32)
    assert lib.mapdn_get_obs_index(h, _lib._p(kind, _lib._pi), _lib._p(idx, _lib._pi)) == 0
    kind, idx = kind.reshape(dims.n_agents, -1), idx.reshape(dims.n_agents, -1)
    for i in range(net.n_sgen):
        rows = net.zone_buses(int(net.sgen_zone[i]))       # oracle: ascending bus index of the zone
        Z = rows.shape[0]
        want_kind = [1] * Z + [2] * Z + [3, 4] + [5] * Z + [6] * Z
        want_idx = list(rows) + list(rows) + [i, i] + list(rows) + list(rows)
        pad = dims.obs_size - len(want_kind)
        assert list(kind[i]) == want_kind + [0] * pad
        assert list(idx[i][:len(want_idx)]) == want_idx
    lib.mapdn_destroy(h)


def test_state_space_subset(lib):
    net, _ = make_case("case33")
    rc, h = host_handle(lib, net, dict(ARGS, state_space=["vm_pu", "pv"]))
    assert rc == 0
    dims = _lib.CDims()
    lib.mapdn_dims(h, C.byref(dims))
    assert dims.obs_size == 12 + 1 and dims.state_size == 33 + 6
    lib.mapdn_destroy(h)


def test_error_paths(lib):
    net, _ = make_case("case33")
    # meshed: close a loop with a tie line (Baran-Wu tie 21-8)
    m = net.copy()
    for k in ("line_from_bus", "line_to_bus", "line_parallel"):
        setattr(m, k, np.append(getattr(m, k), {"line_from_bus": 20, "line_to_bus": 7, "line_parallel": 1}[k]).astype(np.int32))
    for k, v in (("line_r_ohm_per_km", 2.0), ("line_x_ohm_per_km", 2.0), ("line_c_nf_per_km", 0.0),
                 ("line_g_us_per_km", 0.0), ("line_length_km", 1.0)):
        setattr(m, k, np.append(getattr(m, k), v))
    m.line_in_service = np.append(m.line_in_service, 1).astype(np.uint8)
    rc, h = host_handle(lib, m)           # a 33-bus meshed net is accepted (general-topology solver, tests/test_general_topology.py)
    assert rc == 0
    dims = _lib.CDims()
    assert lib.mapdn_dims(h, C.byref(dims)) == 0 and dims.is_radial == 0
    lib.mapdn_destroy(h)
    # the same tie line out of service: radial again
    m.line_in_service[-1] = 0
    rc, h = host_handle(lib, m)
    assert rc == 0
    assert lib.mapdn_dims(h, C.byref(dims)) == 0 and dims.is_radial == 1
    lib.mapdn_destroy(h)
    # disconnected
    d = net.copy()
    d.line_in_service[5] = 0
    rc, h = host_handle(lib, d)
    assert rc == -2 and b"not connected" in lib.mapdn_last_error(None)
    # sgen outside its zone -> the reference's get_obs would raise KeyError
    s = net.copy()
    s.sgen_bus[0] = 3
    rc, h = host_handle(lib, s)
    assert rc == -1 and b"KeyError" in lib.mapdn_last_error(None)
    # neither weight
    rc, h = host_handle(lib, net, dict(ARGS, q_weight=None, line_weight=None))
    assert rc == -1 and b"NotImplementedError" in lib.mapdn_last_error(None)
    # a host-only handle refuses device entry points; a device handle fails loudly without a GPU
    rc, h = host_handle(lib, net)
    assert lib.mapdn_step(h, None, 0, 0, None, None, None, None) != 0
    assert lib.mapdn_get_obs(h, C.c_void_p(8), 0, None) == -4
    lib.mapdn_destroy(h)


def test_no_gpu_fails_loudly(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    net, _ = make_case("case33")
    cn, keep = _lib.make_cnetspec(net)
    cc = _lib.make_cconfig(ARGS)
    h = C.c_void_p()
    assert lib.mapdn_create(C.byref(cn), C.byref(cc), 4, 0, C.byref(h)) == -3
    from mapdn_amd.env import VoltageControlBatch
    with pytest.raises(Exception):
        VoltageControlBatch(net, make_case("case33")[1], ARGS, n_envs=2, device="cpu")


@pytest.mark.parametrize("case", ["case33", "case141", "case322"])
@pytest.mark.parametrize("W", [1, 2, 4, 8, 16])
def test_nr_schedule_is_a_valid_tree_elimination(lib, case, W):
    """Hu schedule: every node exactly once, children strictly before their parent, one node per
    (wave,row), rows bounded below by tree depth and n/W and above by n."""
    net, _ = make_case(case)
    rc, h = host_handle(lib, net)
    assert rc == 0
    n = net.n_bus - 1
    R = C.c_int32()
    assert lib.mapdn_get_schedule(h, W, C.byref(R), None, None) == 0
    R = R.value
    rows = np.zeros(W * R, np.int32)
    par = np.zeros(n, np.int32)
    assert lib.mapdn_get_schedule(h, W, C.byref(C.c_int32()), _lib._p(rows, _lib._pi), _lib._p(par, _lib._pi)) == 0
    rows = rows.reshape(W, R)
    nodes = rows[rows >= 0]
    assert sorted(nodes.tolist()) == list(range(n))
    row_of = np.zeros(n, int)
    for w in range(W):
        for r in range(R):
            if rows[w, r] >= 0:
                row_of[rows[w, r]] = r
    depth = np.zeros(n + 1, int)
    for k in range(n - 1, -1, -1):
        assert par[k] > k                      # parents are eliminated after their children
        depth[k] = depth[par[k]] + 1
        if par[k] < n:
            assert row_of[par[k]] > row_of[k]
    assert max(depth.max(), -(-n // W)) <= R <= n
    if W == 1:
        assert R == n
    lib.mapdn_destroy(h)


@pytest.mark.parametrize("case", ["case33", "case141", "case322"])
def test_flat_start_factorisation_is_the_first_newton_step(lib, case):
    """plan.cpp factorises the flat-start Jacobian once per topology (the NR kernel's first iteration only
    substitutes the right-hand side).  Replaying that substitution on the host with the exported constants
    must give the oracle's first Newton step dx = -J(V0)^-1 F(V0) for an arbitrary Sbus."""
    from scipy.sparse.linalg import spsolve
    from oracle.pp_restated import make_ybus, bus_demand, make_sbus, jacobian, _fx
    net, prof = make_case(case)
    rc, h = host_handle(lib, net)
    assert rc == 0
    nb, n = net.n_bus, net.n_bus - 1
    fac = np.zeros((n, 12)); bop = np.zeros(n + 1, np.int32); par = np.zeros(n, np.int32)
    assert lib.mapdn_get_flat_factors(h, _lib._p(fac, _lib._pd), _lib._p(bop, _lib._pi)) == 0
    assert lib.mapdn_get_schedule(h, 1, C.byref(C.c_int32()), None, _lib._p(par, _lib._pi)) == 0
    assert bop[n] == net.ext_grid_bus and sorted(bop.tolist()) == list(range(nb))
    rng = np.random.default_rng(1)
    row = int(rng.integers(0, prof.n_rows))
    pv = prof.pv[row]
    q = rng.uniform(-0.6, 0.6, net.n_sgen) * np.sqrt(prof.s_max() ** 2 - pv ** 2)
    sbus = make_sbus(net, *bus_demand(net, prof.load_p[row], prof.load_q[row], pv, q))
    # ---- oracle: one Newton step from the flat start
    ybus = make_ybus(net)[0]
    pq = np.setdiff1d(np.arange(nb), [net.ext_grid_bus])
    v0 = np.full(nb, net.ext_grid_vm_pu, dtype=np.complex128)
    dx = -spsolve(jacobian(ybus, v0, pq, pq).tocsc(), _fx(ybus, v0, sbus, pq, pq))
    dth = np.zeros(nb); dvm = np.zeros(nb)
    dth[pq] = dx[:n]; dvm[pq] = dx[n:]
    # ---- host replay of the kernel's flat sweep pair with the exported constants
    S = fac[:, 0] + 1j * fac[:, 1]
    Iinv = fac[:, 2:6].reshape(n, 2, 2); apk = fac[:, 6:8]; G = fac[:, 8:12].reshape(n, 2, 2)
    hvec = np.zeros((n, 2)); acc = np.zeros((n + 1, 2)); x = np.zeros((n + 1, 2))
    for k in range(n):                                            # children have smaller positions
        F = S[k] - sbus[bop[k]]
        hvec[k] = Iinv[k] @ (np.array([F.real, F.imag]) - acc[k])
        ar, ai = apk[k]
        acc[par[k]] += (ai * hvec[k, 0] + ar * hvec[k, 1], ai * hvec[k, 1] - ar * hvec[k, 0])
    for k in range(n - 1, -1, -1):
        x[k] = hvec[k] - G[k] @ (x[par[k]] if par[k] < n else np.zeros(2))
    assert np.abs(-x[:n, 0] - dth[bop[:n]]).max() < 1e-10
    assert np.abs(-x[:n, 1] * abs(v0[0]) - dvm[bop[:n]]).max() < 1e-10
    lib.mapdn_destroy(h)


def test_drop_in_class_covers_the_whole_env_protocol():
    """every call of the PyMARL env protocol (environments/multiagentenv.py) is implemented by the drop-in
    class, with the reference's positional arguments"""
    import inspect
    from mapdn_amd.env import VoltageControl
    from mapdn_amd.marl_env_api import PROTOCOL, MultiAgentEnv
    assert issubclass(VoltageControl, MultiAgentEnv)
    for name, call in PROTOCOL.items():
        fn = getattr(VoltageControl, name)
        if call.required and name not in ("get_stats", "seed", "save_replay"):      # never called by MAPDN, absent in its env too
            assert fn is not getattr(MultiAgentEnv, name), name
        params = [p for p in inspect.signature(fn).parameters if p != "self"]
        assert tuple(params[:len(call.args)]) == call.args or name == "render", (name, params)
    with pytest.raises(NotImplementedError):
        MultiAgentEnv().get_stats()


def test_header_is_plain_c_and_usable_from_a_c_host(lib, tmp_path):
    """include/mapdn.h must be consumable by any FFI: compile examples/c_abi_host.c as strict C99 against it,
    link the shared library and run it (host-only handle: no GPU involved)."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "c_abi_host")
    libdir = os.path.join(root, "mapdn_amd")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "examples", "c_abi_host.c"), "-o", exe, "-L" + libdir, "-lmapdn_hip",
                    "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "n_bus 5" in out and "radial 1" in out and "n_agents 2" in out
    from mapdn_amd import build
    assert "MAPDN_SRC_HASH=" + build.source_hash() in out
    assert "mapdn_reset on a host-only handle -> -4" in out


def test_allocation_failure_inside_create_comes_back_as_a_code(lib, tmp_path):
    """VERDICT r5 weak #7 / SURVEY 8(b) "never throw across the boundary": tests/alloc_fail_host.c caps its address space so that the
    plan's allocations for a 3 000-bus feeder fail inside mapdn_create — the C host must read MAPDN_E_NOMEM (-5) and a text, not die of
    an uncaught std::bad_alloc, and the next call must work."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    if "asan" in os.environ.get("LD_PRELOAD", ""):
        pytest.skip("AddressSanitizer's own allocator cannot run under the RLIMIT_AS cap this test sets (`make asan` runs)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "alloc_fail_host")
    libdir = os.path.join(root, "mapdn_amd")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "alloc_fail_host.c"), "-o", exe, "-L" + libdir, "-lmapdn_hip", "-Wl,-rpath," + libdir], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    assert "capped create -> -5" in res.stdout and "bad_alloc" in res.stdout and "handle null" in res.stdout


def test_every_entry_point_of_the_env_library_is_exception_tight():
    """every `int mapdn_*` defined in capi.hip (the entry points that run host C++: plan, exporters, event pools) is a
    function-try-block ending in MAPDN_CATCH; mapdn_create wraps its body explicitly (it owns the half-built handle)"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "mapdn_amd", "csrc", "capi.hip")).read()
    body = src[src.index('extern "C" {'):]
    names = re.findall(r"^int (mapdn_\w+)\(", body, flags=re.M)
    assert len(names) >= 24
    for name in names:
        start = body.index("int " + name + "(")
        head = body[start:body.index("{", start) + 1]
        if name == "mapdn_create":
            assert "MAPDN_CATCH(nullptr)" in body[start:body.index("void mapdn_destroy")]
        else:
            assert head.rstrip().endswith("try {"), name
    assert body.count("} MAPDN_CATCH(") == len(names)          # (create: its inner `try { throw; } MAPDN_CATCH(nullptr)`)
    hdr = open(os.path.join(root, "include", "mapdn.h")).read()
    assert "MAPDN_E_NOMEM (-5)" in hdr and "MAPDN_E_INTERNAL (-6)" in hdr


def _geometry(lib, net, B, tuning=None):
    cn, keep = _lib.make_cnetspec(net)
    cc = _lib.make_cconfig(ARGS, 0, tuning)
    h = C.c_void_p()
    rc = lib.mapdn_create(C.byref(cn), C.byref(cc), B, -1, C.byref(h))
    if rc:
        return rc, lib.mapdn_last_error(None).decode()
    g = _lib.nr_geometry(h)
    lib.mapdn_destroy(h)
    return 0, g


@pytest.mark.parametrize("case,B,want", [
    # the measured-best launch of every BASELINE size (profiles/r02_nr_geometry_case141.txt, profiles/r03_geometry_case322.txt):
    # (waves, envs per workgroup, lean, h in LDS)
    ("case33", 4096, (1, 16, 0, 1)), ("case141", 1, (4, 16, 0, 1)), ("case141", 4096, (4, 16, 0, 1)), ("case141", 8192, (2, 16, 1, 0)),
    ("case141_deep", 4096, (4, 16, 0, 1)), ("case322", 1024, (4, 8, 0, 1)), ("case322", 4096, (4, 16, 0, 0)), ("case322", 8192, (4, 16, 0, 0)),
])
def test_nr_geometry_model_reproduces_the_measured_defaults(lib, case, B, want):
    """The chooser is a launch-time model over the compiled (waves, lanes, lean) candidates (capi.hip::nr_model_ns, fitted by
    tools/nr_geometry_fit.py), no longer two thresholds on n: at the shapes that were swept on hardware it must pick what
    the sweeps found fastest — for host-only handles too (they assume the MI355X's 256 CUs)."""
    net, _ = make_case(case)
    rc, g = _geometry(lib, net, B)
    assert rc == 0, g
    assert (g["waves"], g["lanes"], g["lean"], g["h_lds"]) == want, g
    assert g["solver"] == 0 and g["lds_bytes"] <= 160 * 1024 and g["model_ns"] > 0
    assert g["workgroups"] == (B + 63) // 64 * 64 // g["lanes"]


def test_nr_geometry_for_feeders_nobody_tuned(lib):
    """a 69-bus feeder (Baran & Wu) and a ~200-bus random feeder get a geometry from the same model, without environment
    variables: more than one worker per env, everything the solve touches in LDS at a small batch, a layout with more envs per
    CU once the batch needs several rounds of workgroups; pinned fields are honoured; an uncompiled pair is refused loudly"""
    from tests.golden.literature_cases import bw69
    from mapdn_amd.netspec import _radial_case
    net69 = bw69()[0]
    rc, g = _geometry(lib, net69, 4096)
    assert rc == 0, g
    assert g["waves"] * 64 // g["lanes"] >= 4 and g["h_lds"] == 1 and g["rounds"] == 1, g
    net200, _ = _radial_case("rand200", 201, 120, 20, 10, 21, 12.47, 10.0, 10.0, 5, 0.05)
    rc, small = _geometry(lib, net200, 1024)
    assert rc == 0 and small["h_lds"] == 1 and small["rounds"] == 1 and small["waves"] == 4, small
    rc, big = _geometry(lib, net200, 16384)
    assert rc == 0 and big["workgroups"] / big["resident_per_cu"] <= small["workgroups"] * 16 / small["resident_per_cu"], big
    assert big["rounds"] * big["lanes"] * big["resident_per_cu"] * 256 >= 16384
    # the model's estimate grows with the batch once the chip is full and is not below the one-round time
    assert big["model_ns"] > small["model_ns"]
    rc, g = _geometry(lib, net200, 1024, dict(nr_waves=2, nr_lanes=16, nr_lean=1))
    assert rc == 0 and (g["waves"], g["lanes"], g["lean"], g["h_lds"], g["model_ns"]) == (2, 16, 1, 0, 0), g
    rc, g = _geometry(lib, net200, 1024, dict(nr_h_lds=2))
    assert rc == 0 and g["h_lds"] == 0 and g["mm_pass"] == 0, g
    rc, msg = _geometry(lib, net200, 1024, dict(nr_waves=8, nr_lanes=16, nr_lean=1))
    assert rc == -1 and "not compiled in" in msg
    rc, msg = _geometry(lib, net200, 1024, dict(nr_waves=3))
    assert rc == -1 and "nr_waves" in msg


def test_env_config_layout_matches_the_header(lib, tmp_path):
    """ctypes mirror of mapdn_env_config == the C struct (size and the offset of every appended tuning field)"""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = [f[0] for f in _lib.CEnvConfig._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mapdn.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(mapdn_env_config));\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(mapdn_env_config, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == C.sizeof(_lib.CEnvConfig)
    for line in out[1:]:
        if line:
            name, off = line.split()
            assert getattr(_lib.CEnvConfig, name).offset == int(off), name


def test_tolerance_options(lib):
    """mapdn_env_config.tolerance_mva / tolerance_is_pu: the stopping rule is tolerance_mva / sn_mva per unit by default (the rule
    as restated from pandapower, unpinned) or tolerance_mva itself; visible through the plan on a net with sn_mva != 1"""
    net, _ = make_case("case141")                       # sn_mva = 10
    assert net.sn_mva == 10.0
    for tuning, ok in ((None, True), (dict(tolerance_is_pu=1), True), (dict(tolerance_mva=1e-6), True), (dict(tolerance_mva=-1.0), False)):
        rc, g = _geometry(lib, net, 64, tuning)
        assert (rc == 0) == ok, g


def test_step_composition_switches_are_validated_for_every_solver(lib, monkeypatch):
    """fuse_inject = 1 exists on the tree solver only and needs a handle without auto_reset and inject_full; overlap_advance and
    xcd_map were removed and are refused on every solver.  mapdn_create checks all of it before the device set-up, so a host-only
    handle refuses what a device handle refuses.  The geometry export reports the fuse_inject the handle was created with, whatever
    the environment says afterwards."""
    for v in ("MAPDN_FUSE_INJECT", "MAPDN_INJECT_FULL", "MAPDN_NR_SPARSE", "MAPDN_NR_DENSE"):
        monkeypatch.delenv(v, raising=False)
    net, _ = make_case("case33")

    def create(tuning, **args):
        cn, keep = _lib.make_cnetspec(net)
        cc = _lib.make_cconfig(dict(ARGS, **args), 0, tuning)
        h = C.c_void_p()
        rc = lib.mapdn_create(C.byref(cn), C.byref(cc), 8, -1, C.byref(h))
        return rc, h, "" if rc == 0 else lib.mapdn_last_error(None).decode()

    for solver in ("tree", "sparse", "dense"):
        for removed in ("overlap_advance", "xcd_map"):
            rc, _, msg = create(dict(nr_solver=solver, **{removed: 1}))
            assert rc == -1 and removed in msg and "removed" in msg, (solver, msg)
        rc, h, msg = create(dict(nr_solver=solver, fuse_inject=1))
        if solver == "tree":
            assert rc == 0, msg
            assert _lib.nr_geometry(h)["fuse_inject"] == 1
            lib.mapdn_destroy(h)
        else:
            assert rc == -1 and "tree solver only" in msg, (solver, msg)
    rc, _, msg = create(dict(fuse_inject=1), auto_reset=True)
    assert rc == -1 and "auto_reset" in msg, msg
    rc, _, msg = create(dict(fuse_inject=1, inject_full=1))
    assert rc == -1 and "inject_full" in msg, msg
    # what the handle was created with, not what the environment says now
    for tuning, env, want in ((dict(fuse_inject=2), "2", 0), (None, "0", 1)):
        rc, h, msg = create(tuning)
        assert rc == 0, msg
        monkeypatch.setenv("MAPDN_FUSE_INJECT", env)
        assert _lib.nr_geometry(h)["fuse_inject"] == want
        lib.mapdn_destroy(h)
        monkeypatch.delenv("MAPDN_FUSE_INJECT")
