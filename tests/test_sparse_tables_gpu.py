"""GPU (-m gpu): k_opf_sens_sparse, k_opf_reduce_sparse and k_action_grad_sparse at the edges of their sgen table and at feeder size
(tests/sparse_table_cases.py): 16, 17, 33, 64 and 65 sgens, 64, 65 and 140 nodes, a ratio-and-shift transformer on
a cycle with a dead net.line row beside it — at every sp_lanes the handle accepts, B = 5 and 17 (ragged at every sp_lanes), K = 4.

The references, bars and checks are those of tests/test_opf_sparse_gpu.py and tests/test_action_grad_sparse_gpu.py, unchanged: the
extended-precision references at the kernel's own V, 16 x the float64 reference's own error on the key (the E64 dicts) and never below
64 ulp.  Every condition on the inputs is asserted of the references alone in tests/test_sparse_tables_cpu.py.  Every caller-owned
output of the two parity tests sits between guard zones (tests/test_branch_results_gpu.Guarded's scheme).  What the kernels showed on an
MI355X is tabulated in DESIGN.md section 27 (the worst fraction of a bar: 0.22)."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from mapdn_amd import _lib
from mapdn_amd.env import N_INFO
from tests import grad_ref as G
from tests import grad_sparse_cases as GS
from tests import opf_kernel_cases as K
from tests import opf_ref as R
from tests import opf_sparse_cases as OS
from tests import sparse_table_cases as ST
from tests import test_branch_results_gpu as TB
from tests import test_action_grad_sparse_gpu as TG
from tests import test_opf_sparse_gpu as TS
from tests import whatif_cases as W
from tests.test_action_grad_gpu import gradients
from tests.test_opf_gpu import place

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BATCHES = (5, 17)                                # ragged at every sp_lanes (16, 8, 4 and 2 envs a wavefront)
KC = 4                                           # candidates: {0, random, UNSOLVABLE, random}
V_BAR = 1e-9                                     # |V| of the probe against the oracle, p.u.: what tests/test_opf_sparse_gpu.check_loop holds the loop's |V| to
SENT_INT = {torch.uint8: 0xA5, torch.int32: -77}


class Guarded(TB.Guarded):
    """tests/test_branch_results_gpu.Guarded with a sentinel for uint8 as well"""

    def __init__(self, shape, dtype=torch.float64):
        self.shape, self.n = shape, int(np.prod(shape))
        self.sent = TB.SENT if dtype == torch.float64 else SENT_INT[dtype]
        self.buf = torch.full((self.n + 2 * TB.GUARD,), self.sent, dtype=dtype, device=DEV)
        self.ptr = self.buf.data_ptr() + TB.GUARD * self.buf.element_size()


def guarded_probe(env, a, cfg=TS.MESHED):
    """env.opf_probe with every output between guard zones; the same fields as tests/test_opf_sparse_gpu.probe"""
    cc = _lib.make_opf_config(cfg)
    B, ns, n = env.n_envs, env.n_sgen, env.n_bus - 1
    a = torch.as_tensor(a, dtype=torch.float64, device=DEV).contiguous()
    assert a.shape == (B, ns)
    out = dict(v_re=Guarded((B, n)), v_im=Guarded((B, n)), vm=Guarded((B, n)), S=Guarded((B, n, ns)), g=Guarded((B, ns)), H=Guarded((B, ns, ns)),
               loss_mw=Guarded((B,)), violation=Guarded((B,)), d=Guarded((B, ns)), y=Guarded((B, ns + n)),
               linearised=Guarded((B,), torch.uint8), qp_capped=Guarded((B,), torch.uint8))
    with torch.cuda.device(env.device):
        _lib.check(env._lib.mapdn_opf_probe(env._h, C.byref(cc), a.data_ptr(), ns, *[g.ptr for g in out.values()], env._stream()), env._h)
    torch.cuda.synchronize()
    got = {k: g.get() for k, g in out.items()}
    for k, x in got.items():                                     # every entry was written
        assert (x != out[k].sent).all(), ("an entry that was not written", k)
    got["v"] = got.pop("v_re") + 1j * got.pop("v_im")
    got["linearised"], got["qp_capped"] = got["linearised"].astype(bool), got["qp_capped"].astype(bool)
    got["bus_of_node"] = np.array([b for b in range(env.n_bus) if b != int(env.net.ext_grid_bus)], np.int64)
    return types.SimpleNamespace(**got)


def guarded_gradients(env, cand):
    """env.action_gradients(cand, vm_pu=True) with every output between guard zones: (grad, reward, info, status, iterations, vm_pu)"""
    a = torch.as_tensor(cand, dtype=torch.float64, device=DEV).contiguous()
    B, Kc, ns = a.shape
    assert (B, ns) == (env.n_envs, env.n_sgen)
    out = (Guarded((B, Kc, ns)), Guarded((B, Kc)), Guarded((B, Kc, N_INFO)), Guarded((B, Kc), torch.uint8), Guarded((B, Kc), torch.int32),
           Guarded((B, Kc, env.n_bus)))
    with torch.cuda.device(env.device):
        _lib.check(env._lib.mapdn_action_gradients(env._h, a.data_ptr(), env._code(a.dtype), Kc, *[g.ptr for g in out], env._stream()), env._h)
    torch.cuda.synchronize()
    got = tuple(g.get() for g in out)
    for i, x in enumerate(got):
        assert (x != out[i].sent).all(), ("an entry that was not written", i)
    return got


# ---- 1. the probe against the extended reference --------------------------------------------------------------------------------------------
PROBE = [(key, L) for key in ST.OPF_KEYS for L in OS.fits(key)]


@functools.lru_cache(maxsize=None)
def _column_errors(key, e, bus, v_bytes, s_bytes, g_bytes, h_bytes):
    """per column j the error of S[:, j], g[j] and H[j, :] of env e against the extended reference at the probe's V, each relative to
    the largest magnitude of its whole reference array (the scale of tests/opf_kernel_cases.errors)"""
    net = OS.make(key)[0]
    n, ns = net.n_bus - 1, net.n_sgen
    _, _, pv, smax = OS.inputs(key, e)
    V = np.full(net.n_bus, net.ext_grid_vm_pu, np.complex128)
    S = np.zeros((net.n_bus, ns))
    V[list(bus)], S[list(bus)] = np.frombuffer(v_bytes, np.complex128), np.frombuffer(s_bytes).reshape(n, ns)
    ref = K.linearise_ext(net, V, R.limits(pv, smax))
    g, H = np.frombuffer(g_bytes).astype(K.LD), np.frombuffer(h_bytes).reshape(ns, ns).astype(K.LD)
    return (np.abs(S.astype(K.LD) - ref.S).max(axis=0) / np.abs(ref.S).max(), np.abs(g - ref.g) / np.abs(ref.g).max(),
            np.abs(H - ref.H).max(axis=1) / np.abs(ref.H).max())


def probe_once(key, L, B, scale=1.0):
    prof = OS.make(key)[1]
    env = TS.make_env(key, B, L, scale)
    try:
        assert env.nr_kernel()["solver"] == 1 and (L is None or env.nr_kernel()["L"] == L)
        place(env, OS.scaled(prof, scale), OS.rows_of(prof, B))
        return guarded_probe(env, OS.setpoints(key, B))
    finally:
        env.close()


@pytest.mark.parametrize("key,L", PROBE, ids=[f"{k}-{L}" for k, L in PROBE])
def test_probe_against_the_extended_reference(key, L):
    net = OS.make(key)[0]
    n, ns = net.n_bus - 1, net.n_sgen
    slack_sgens = [j for j, b in enumerate(net.sgen_bus) if b == net.ext_grid_bus]
    assert bool(slack_sgens) == (key == "special_meshed")
    total, total_v = {q: 0.0 for q in K.QUANTITIES}, 0.0
    c = np.ascontiguousarray
    for B in BATCHES:
        out = probe_once(key, L, B)
        assert out.linearised.all() and out.v.shape == (B, n) and out.S.shape == (B, n, ns) and out.H.shape == (B, ns, ns)
        for k in ("S", "g", "H", "loss_mw", "violation", "d", "y"):
            assert np.isfinite(getattr(out, k)).all(), (key, L, B, k)
        assert np.array_equal(out.H, out.H.transpose(0, 2, 1))              # H == H' bitwise
        for j in slack_sgens:
            assert (out.S[:, :, j] == 0).all() and (out.g[:, j] == 0).all() and (out.H[:, j, :] == 0).all() and (out.H[:, :, j] == 0).all()
        worst = TS.linearisation_errors(key, out, B)
        for q in K.QUANTITIES:
            total[q] = max(total[q], worst[q])
            assert worst[q] <= OS.bar(key, q), (key, L, B, q, worst[q], OS.bar(key, q))
        bus = tuple(int(b) for b in out.bus_of_node)
        a = OS.setpoints(key, B)
        for e in K.ref_envs(B):                                             # V itself, against the oracle at the env's set-points
            dv = float(np.abs(out.vm[e] - OS.oracle_voltage(key, e, a[e]).vm_pu[list(bus)]).max())
            total_v = max(total_v, dv)
            assert dv <= V_BAR, (key, L, B, e, dv)
        for e in K.ref_envs(B) if ns > ST.DS else ():                       # the columns of a second turn, one by one
            eS, eg, eH = _column_errors(key, e, bus, c(out.v[e]).tobytes(), c(out.S[e]).tobytes(), c(out.g[e]).tobytes(), c(out.H[e]).tobytes())
            for j in range(ST.DS, ns):
                turn = f"column {j}: turn {j // ST.DS} of sub-lane {j % ST.DS} in k_opf_reduce_sparse, pair {j // 2} half {j % 2} in k_opf_sens_sparse"
                assert eS[j] <= OS.bar(key, "S") and eg[j] <= OS.bar(key, "g") and eH[j] <= OS.bar(key, "H"), (key, L, B, e, turn, eS[j], eg[j], eH[j])
        TS.check_kkt_of_the_qp(key, out, a)
    print(f"\n[sparse tables gpu] opf {key} sp_lanes={L}: |V| against the oracle {total_v:.2e} (bar {V_BAR:.0e}); gpu", {q: f"{v:.2e}" for q, v in total.items()}, "bar", {q: f"{OS.bar(key, q):.2e}" for q in K.QUANTITIES},
          "fraction", {q: f"{total[q] / OS.bar(key, q):.2f}" for q in K.QUANTITIES})


# ---- 2. the gradient against the extended reference ----------------------------------------------------------------------------------------
GRAD = [(key, L) for key in ST.KEYS for L in GS.fits(key)]


def gradient_once(key, L, B, args=()):
    env = TG.make_env(key, B, L, **dict(args))
    try:
        kern = env.nr_kernel()
        assert kern["solver"] == 1 and kern["L"] == L
        TG.scenario(env, key)
        return guarded_gradients(env, GS.candidates(key, B, KC))
    finally:
        env.close()


@pytest.mark.parametrize("key,L", GRAD, ids=[f"{k}-{L}" for k, L in GRAD])
def test_gradient_against_the_extended_reference(key, L):
    """compare() asserts the oracle's solved pattern (every candidate but the UNSOLVABLE column, for every env: no env is skipped), the
    status and NaN rows exactly where the reference has no solution, |V|, and the gradient at the bar"""
    assert W.global_kernels("grad_sparse.hip") == TG.KERNELS
    worst = 0.0
    for B in BATCHES:
        got = gradient_once(key, L, B)
        worst = max(worst, TG.compare(key, (), got, B, KC, where=f"sp_lanes={L}"))
        assert np.isnan(got[0][:, 2]).all() and np.isfinite(got[0][:, [0, 1, 3]]).all()
    print(f"[sparse tables gpu] grad {key} sp_lanes={L}: fraction of the bar {worst / GS.bar(key):.2f}")


@pytest.mark.parametrize("L", GS.fits("special_meshed"))
def test_gradient_with_the_line_weight_and_a_dead_line_row(L):
    """special_meshed with G.LINE_ARGS: the line term walks every net.line row, the one out of service included"""
    key, args = "special_meshed", G.LINE_ARGS
    B, Kc = GS.VARIANT_SHAPE
    assert (B, Kc) == (BATCHES[0], KC)
    net = GS.make(key)[0]
    assert int(np.asarray(net.line_in_service).sum()) == net.n_line - 1
    worst = TG.compare(key, args, gradient_once(key, L, B, args), B, Kc, where=f"sp_lanes={L}")
    print(f"[sparse tables gpu] grad {key} line weight sp_lanes={L}: fraction of the bar {worst / GS.bar(key, args):.2f}")


# ---- 3. place invariance --------------------------------------------------------------------------------------------------------------------
FROZEN_ENV = 7


def grad_run(key, L, B, first=0):
    env = TG.make_env(key, B, L, env_id_offset=first)
    try:
        TG.scenario(env, key, first=first)
        return gradients(env, GS.candidates(key, first + B, KC)[first:])
    finally:
        env.close()


@pytest.mark.parametrize("key", ST.BITS_KEYS)
def test_every_env_has_the_same_bits_wherever_it_runs(key):
    """probe and gradient: alone at B = 1 with its env_id_offset; in another batch size; after a permutation (the probe) or in a batch
    that begins at another env id (the gradient); across every sp_lanes that fits"""
    B = 17
    lanes = OS.fits(key)
    first = TS.probe_run(key, lanes[0], B)
    grad = grad_run(key, lanes[0], B)
    for e in (0, B - 1):
        TS.same_bits(first, TS.probe_run(key, lanes[0], B, only=e), slice(e, e + 1), slice(0, 1), f"env {e} alone")
    TG.same_bits([x[6:7] for x in grad], grad_run(key, lanes[0], 1, first=6), "env 6 alone")
    small = TS.probe_run(key, lanes[0], 5)                       # (the last env of a batch has set-points of its own: OS.setpoints)
    TS.same_bits(first, small, slice(0, 4), slice(0, 4), "B = 5")
    TG.same_bits([x[:5] for x in grad], grad_run(key, lanes[0], 5), "B = 5")
    TG.same_bits([x[13:] for x in grad], grad_run(key, lanes[0], 4, first=13), "env ids from 13, B = 4")
    order = np.array([(7 * i + 3) % B for i in range(B)])
    assert sorted(order.tolist()) == list(range(B))
    TS.same_bits(first, TS.probe_run(key, lanes[0], B, order=order), order, slice(None), "permuted")
    for L in lanes[1:]:
        TS.same_bits(first, TS.probe_run(key, L, B), what=f"sp_lanes {L} against {lanes[0]}")
        other = grad_run(key, L, B)
        TG.same_bits((other[0], other[5]), (grad[0], grad[5]), f"sp_lanes {L} against {lanes[0]}")


@pytest.mark.parametrize("key", ST.BITS_KEYS)
def test_mixed_wavefronts(key):
    """env 7 frozen by an unsolvable step (no auto_reset) between ordinary envs, and the UNSOLVABLE candidate in every env: the frozen
    env is not linearised and gets NaN rows of status 3; every other env keeps the bits it has in a batch where env 7 stepped like the
    others — in the probe and in the gradient"""
    B = 17
    ns = GS.make(key)[0].n_sgen
    a1 = np.random.default_rng(7).uniform(-0.5, 0.5, (B, ns))
    a_frozen = a1.copy()
    a_frozen[FROZEN_ENV] = GS.unsolvable(key)
    cand, a = GS.candidates(key, B, KC), OS.setpoints(key, B)
    ordinary = [e for e in range(B) if e != FROZEN_ENV]
    lanes = GS.fits(key)
    for L in (lanes[0], lanes[-1]):
        runs = {}
        for which, act in (("plain", a1), ("mixed", a_frozen)):
            env = TG.make_env(key, B, L)
            try:
                TG.scenario(env, key)
                _, term, _ = env.step(torch.as_tensor(act, device=DEV))
                assert term.cpu().numpy().tolist() == [which == "mixed" and e == FROZEN_ENV for e in range(B)]
                runs[which] = (TS.probe(env, a), gradients(env, cand))
            finally:
                env.close()
        probe, got = runs["mixed"]
        assert not probe.linearised[FROZEN_ENV] and probe.linearised[ordinary].all()
        assert (probe.d[FROZEN_ENV] == 0).all() and (probe.y[FROZEN_ENV] == 0).all()
        assert (got[3][FROZEN_ENV] == W.NOT_EVALUATED).all() and np.isnan(got[0][FROZEN_ENV]).all()
        assert (got[3][ordinary] == np.where(TG.PATTERN, W.SOLVED, W.PF_FAILED)).all()
        assert np.isnan(got[0][ordinary][:, 2]).all() and np.isfinite(got[0][ordinary][:, [0, 1, 3]]).all()
        TS.same_bits(probe, runs["plain"][0], ordinary, ordinary, f"sp_lanes {L}: probe beside a stopped env")
        TG.same_bits([x[ordinary] for x in got], [x[ordinary] for x in runs["plain"][1]], f"sp_lanes {L}: gradient beside a stopped env")


# ---- 4. the loop ------------------------------------------------------------------------------------------------------------------------------
LOOP_BATCH = {"ring33_s17": 17, "special_meshed": 17, "case141_ties": 5, ST.KKT_KEY: 5}


@pytest.mark.parametrize("key", ST.LOOP_KEYS)
def test_loop_against_the_restated_sqp(key):
    B, scale = LOOP_BATCH[key], ST.LOOP_SCALE[key]
    out = TS.loop_run(key, None, B, scale=scale)
    worst = TS.check_loop(key, out, B, scale)
    print(f"\n[sparse tables gpu] {key} x{scale}: status {out[4].tolist()} power flows {out[3].tolist()} kkt residual gpu {worst[0]:.2e} reference {worst[1]:.2e}")


def test_loop_at_64_sgens_ends_at_a_kkt_point():
    """ladder66_s64: 64 columns on 65 nodes may leave the QP's minimiser flat in some directions, so the returned point is held to the
    KKT conditions — of every QP (the probe at the loop's states) and of the nonlinear problem (against the reference's own residual) —
    and to the oracle's violation, not to the reference's actions or counts"""
    key = ST.KKT_KEY
    B, scale = LOOP_BATCH[key], ST.LOOP_SCALE[key]
    net = OS.make(key)[0]
    TS.check_kkt_of_the_qp(key, probe_once(key, None, B, scale), OS.setpoints(key, B))
    a, loss, viol, it, st, vm = TS.loop_run(key, None, B, scale=scale)
    for e in range(B):
        r = OS.reference_run(key, e, scale)
        assert r.status == 0 and st[e] == 0 and 1 <= it[e] < R.DEFAULTS["max_iter"], (e, st[e], it[e])
        res = OS.oracle_voltage(key, e, a[e], scale)
        v = R.violation_of(res.vm_pu, net, *OS.V_BAND)
        assert abs(vm[e] - res.vm_pu).max() < 1e-9 and abs(viol[e] - v) < 1e-9 and v <= TS.V_TOL, (e, v)
        mine, ref = (max(OS.kkt_of(key, e, x, scale)[:2]) for x in (a[e], r.actions))
        print(f"[sparse tables gpu] {key} env {e}: power flows {it[e]} (reference {r.iterations}) kkt residual gpu {mine:.3e} reference {ref:.3e}")
        assert mine <= TS.KKT_FACTOR * ref, (e, mine, ref)
