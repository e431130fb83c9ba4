"""action_gradients on handles of the sparse solver (mapdn_env_config.grad_meshed = 1, k_action_grad_sparse): what
tests/test_action_grad_sparse_cpu.py and tests/test_action_grad_sparse_gpu.py share.  Test infrastructure only, independent of the
product code: the reference is tests/grad_ref.py (dense, topology-agnostic), the nets are those of tests/meshed_edge_nets.py,
crowded_meshed of tests/element_edge_nets.py and the shipped case33 pinned to the sparse solver; the keys of tests/sparse_table_cases.py
 are handed on to that module's make(), fits() and UNSOLVABLE.

The scenario is that of tests/grad_ref.py: reset, one random step, then the candidates {0, random, UNSOLVABLE, random, ...} of every env.
The meshed shapes are stiff: their unsolvable action is meshed_edge_nets.STEP_UNSOLVABLE.  The k9_hv net starts every power flow from
the DC angles (runpp init="dc"), in the oracle env too (oracle_class)."""
import copy
import functools

import numpy as np

from oracle.env_restated import INFO_KEYS
from oracle.pp_restated import build_branches, make_ybus, runpp_restated
from tests import element_edge_nets as N
from tests import grad_ref as G
from tests import meshed_edge_nets as M
from tests import opf_kernel_cases as OK
from tests import sparse_table_cases as ST
from tests import whatif_cases as W

B_MAX, K_MAX = 35, 4
MESHED = ("tri3", "tail2x", "k9", "wheel_rim", "grid6", "k9_hv")            # keys of tests/meshed_edge_nets.py
PARITY_NETS = ("tri3", "tail2x", "k9", "wheel_rim", "grid6", "crowded_meshed", "k9_hv")
PROGRAM_NETS = ("tri3", "tail2x", "k9", "wheel_rim", "grid6", "k9_hv")
CD_NETS = ("crowded_meshed", "tri3", "wheel_rim")
VARIANT_NET, LINE_NET = "wheel_rim", "tail2x"                              # the other four barriers; line_weight (two net.line rows on one bus pair)
VARIANTS = [(("voltage_barrier_type", b),) for b in G.BARRIER_TYPES if b != "bowl"]
VARIANT_SHAPE = (5, 4)


def make(key):
    """(NetSpec, Profiles, base env args)"""
    if key in ST.KEYS:
        return ST.make(key)
    if key in MESHED:
        return (*M.make_net(key), M.ARGS)
    return W.make(key)


def unsolvable(key):
    if key in ST.KEYS:
        return ST.UNSOLVABLE[key]
    return M.STEP_UNSOLVABLE if key in MESHED else W.UNSOLVABLE


def fits(key):
    """the sp_lanes at which k_nr_sparse (so k_action_grad_sparse) fits the net"""
    if key in ST.KEYS:
        return ST.fits(key)
    if key in MESHED:
        return [L for L in M.SP_LANES if L not in M.LDS_REFUSED[M.base_of(key)]]
    return list(M.SP_LANES)                                   # crowded_meshed (15 nodes), case33 (32 nodes, no fill)


def tuning(key, L=None, grad_meshed=1):
    """the handle's tuning: the sparse solver (pinned: tail2x and case33 are radial), sp_lanes = L (None: automatic), the switch"""
    t = dict(nr_solver="sparse", grad_meshed=grad_meshed)
    if L is not None:
        t["sp_lanes"] = int(L)
    return t


def first_action(key, B):
    ns = make(key)[0].n_sgen
    return np.random.default_rng(11 + sum(map(ord, key))).uniform(-0.8, 0.8, (B_MAX, ns))[:B]


def candidates(key, B, K=K_MAX):
    """[B, K, ns] float64: {0, random, UNSOLVABLE, random}[:K] of every env; a smaller B or K is the leading rows of the larger one"""
    ns = make(key)[0].n_sgen
    c = np.random.default_rng(23 + sum(map(ord, key))).uniform(-0.8, 0.8, (B_MAX, K_MAX, ns))
    c[:, 0] = 0.0
    c[:, 2] = unsolvable(key)
    return np.ascontiguousarray(c[:B, :K])


def runpp_of(key):
    return functools.partial(runpp_restated, init="dc") if key.endswith("_hv") else runpp_restated


def oracle_class(key):
    """VoltageControlOracle; on the _hv nets every power flow of it starts from the DC angles (as tests/element_edge_nets.oracle_class
    swaps the ZIP power flow in, per instance)"""
    import oracle.env_restated as R
    if not key.endswith("_hv"):
        return N.oracle_class(key)

    class DcOracle(R.VoltageControlOracle):
        def _run(self, f, *a, **kw):
            keep, R.runpp_restated = R.runpp_restated, runpp_of(key)
            try:
                return f(*a, **kw)
            finally:
                R.runpp_restated = keep

        def reset(self, *a, **kw):
            return self._run(super().reset, *a, **kw)

        def step(self, *a, **kw):
            return self._run(super().step, *a, **kw)
    return DcOracle


def predict(key, o, a):
    """tests/whatif_cases.predict with the power flow of the key (the DC start on the _hv nets)"""
    a = np.asarray(a, np.float64)
    inputs = (o.load_p, o.load_q, o.sgen_p, o._clip_reactive_power(a, o.sgen_p))
    r = runpp_of(key)(o.net, *inputs)
    c = copy.copy(o)
    c._runpp_override = r
    reward, _, info = c.step(a)
    assert c._runpp_override is None and info["destroy"] == (0.0 if r.converged else 1.0)
    return dict(reward=reward, info=np.array([info[k] for k in INFO_KEYS]), solved=bool(r.converged), iterations=int(r.iterations),
                vm=np.asarray(r.vm_pu), r=r, inputs=inputs)


@functools.lru_cache(maxsize=None)
def reference(key, envs, K, args=()):
    """(oracles after reset and one random step, rows[e][k] = predict() of candidates(key, ., K), those candidates [len(envs), K, ns],
    solved [len(envs), K]) for the env ids `envs` (a tuple; an int B: 0 .. B - 1); cached, read-only"""
    envs = tuple(range(envs)) if isinstance(envs, int) else tuple(envs)
    net, prof, base = make(key)
    cls = oracle_class(key)
    os_ = [cls(net, prof, dict(base, **dict(args)), env_id=e, do_reset=False) for e in envs]
    a0 = first_action(key, max(envs) + 1)
    for e, o in zip(envs, os_):
        N.first_draw_reset(o)
        _, term, info = o.step(a0[e])
        assert info["destroy"] == 0.0 and not term, (key, e)
    cand = np.ascontiguousarray(candidates(key, max(envs) + 1, K)[list(envs)])
    rows = [[predict(key, o, cand[i, k]) for k in range(K)] for i, o in enumerate(os_)]
    solved = np.array([[p["solved"] for p in row] for row in rows])
    return os_, rows, cand, solved


def kink_margins(os_, rows, cand):
    """tests/grad_ref.kink_margins on the rows of reference()"""
    ref = dict(solved=np.array([[p["solved"] for p in row] for row in rows]),
               vm=np.array([[p["vm"] if p["solved"] else np.full(os_[0].net.n_bus, np.nan) for p in row] for row in rows]))
    return G.kink_margins(os_, ref, cand)


def central_difference(key, o, a, h):
    """tests/grad_ref.central_difference with the power flow of the key"""
    g = np.zeros(a.shape[0])
    for j in range(a.shape[0]):
        ap, am = a.copy(), a.copy()
        ap[j] += h
        am[j] -= h
        rp, rm = predict(key, o, ap), predict(key, o, am)
        assert rp["solved"] and rm["solved"]
        g[j] = (rp["reward"] - rm["reward"]) / (2 * h)
    return g


# ---- the right-hand side c of the adjoint system, as tests/grad_ref.reward_gradient forms it ---------------------------------------------
def reference_c(net, args, V, ext=False):
    """(c_theta [n_bus], c_vm [n_bus]) = d reward / d (theta, |V|) at V: the lines of grad_ref.reward_gradient that form c, restated
    here because that function returns the gradient alone.  ext: in numpy.longdouble, as reward_gradient(ext=True) forms it"""
    R, C = (G.LD, G.CLD) if ext else (np.float64, np.complex128)
    nb = net.n_bus
    ybus, yf, yt = make_ybus(net)
    Vx = np.asarray(V).astype(C)
    vm = np.abs(Vx)
    c_th, c_vm = np.zeros(nb, R), np.zeros(nb, R)
    c_vm += -(R(args["voltage_weight"]) / R(nb)) * G.barrier_derivative(args["voltage_barrier_type"], vm)
    if args["line_weight"] is not None:
        f, t, _, _, _, _, is_line = build_branches(net)
        Yf, Yt = yf.toarray().astype(C), yt.toarray().astype(C)
        If, It = Yf @ Vx, Yt @ Vx
        for D, tgt in ((np.diag(C(1j) * Vx), c_th), (np.diag(Vx / vm), c_vm)):
            dS = D[f] * np.conj(If)[:, None] + Vx[f][:, None] * np.conj(Yf @ D) + D[t] * np.conj(It)[:, None] + Vx[t][:, None] * np.conj(Yt @ D)
            tgt += -(R(args["line_weight"]) / R(net.n_line)) * R(net.sn_mva) * dS.real[is_line].sum(axis=0)
    return c_th, c_vm


# ---- the host program and the transposed blocks -------------------------------------------------------------------------------------------
def host_program(key, S):
    """(n, pos_bus, dims, ops, slots_ij) of the key's exported elimination program packed for S sub-lanes (a host-only handle pinned to
    the sparse solver at sp_lanes = 64 / S)"""
    net = make(key)[0]
    lib, h, rc, x = M.host_open(key, M.B_POOL, dict(nr_solver="sparse", sp_lanes=64 // S))
    assert rc == 0, x
    try:
        n = net.n_bus - 1
        pos_bus = M.positions(lib, h, net)
        dims, ops, order, slots = M.sparse_program(lib, h, n, S)
        return n, pos_bus, dims, ops, slots
    finally:
        lib.mapdn_destroy(h)


def converged_pool_voltage(key, e=0):
    r = M.oracle(key, e)[0]
    assert r.converged
    return r.V


def ybus_by_position(net, pos_bus):
    """dense Ybus with rows and columns in position order (position n: the slack)"""
    y = make_ybus(net)[0].toarray()
    p = np.array(pos_bus)
    return y[np.ix_(p, p)]


def transposed_blocks_from_ybus(Yp, Vp, swap=False):
    """J' over the n non-slack positions, interleaved per node, from the kernel's formulas in numpy: slot (i, j) = (J_ji)' from
    A_ji = V_j conj(Y_ji V_i).  swap=True takes Y_ij in place of Y_ji: what a kernel that assumed a symmetric Ybus would form"""
    n = Yp.shape[0] - 1
    A = Vp[:, None] * np.conj(Yp * Vp[None, :])                       # A_ij
    S = A.sum(axis=1)
    JT = np.zeros((2 * n, 2 * n))
    for i in range(n):
        for j in range(n):
            if i == j:
                a = A[i, i]
                JT[2 * i:2 * i + 2, 2 * i:2 * i + 2] = [[-(S[i].imag - a.imag), S[i].real - a.real], [S[i].real + a.real, S[i].imag + a.imag]]
            else:
                a = Vp[j] * np.conj((Yp[i, j] if swap else Yp[j, i]) * Vp[i])
                JT[2 * i:2 * i + 2, 2 * j:2 * j + 2] = [[a.imag, -a.real], [a.real, a.imag]]
    return JT


# ---- the bars of tests/test_action_grad_sparse_gpu.py ---------------------------------------------------------------
# E64: per case the error of the plain float64 reward_gradient against the extended one, relative to the row's largest entry, at the
# oracle's V of the solved rows of the reference envs (B = 35, K = 4; the barrier / line_weight variants B = 5, K = 4), measured on the
# CPU (e64 below; tests/test_action_grad_sparse_cpu.py recomputes them).  The bar is tests/grad_ref.bar's rule, unchanged: 16 x E64 and
# never tighter than 64 ulp.
E64 = {
    ("tri3", ()): 1.76e-14, ("tail2x", ()): 2.41e-14, ("k9", ()): 9.78e-15, ("wheel_rim", ()): 7.03e-15, ("grid6", ()): 6.93e-15,
    ("crowded_meshed", ()): 1.55e-14, ("k9_hv", ()): 3.86e-14,
    ("wheel_rim", (("voltage_barrier_type", "l1"),)): 1.82e-15, ("wheel_rim", (("voltage_barrier_type", "l2"),)): 1.05e-14,
    ("wheel_rim", (("voltage_barrier_type", "courant_beltrami"),)): 1.47e-16, ("wheel_rim", (("voltage_barrier_type", "bump"),)): 2.54e-13,
    ("tail2x", G.LINE_ARGS): 7.78e-13,
    # tests/sparse_table_cases.py
    ("ring33_s16", ()): 2.68e-14, ("ring33_s17", ()): 2.96e-14, ("ladder66_s33", ()): 5.29e-14, ("ladder66_s64", ()): 1.20e-13,
    ("ladder66_s65", ()): 1.39e-13, ("ladder65_s4", ()): 1.60e-13, ("special_meshed", ()): 1.99e-14, ("case141_ties", ()): 1.49e-13,
    ("special_meshed", G.LINE_ARGS): 1.66e-12,
}


def shape_of(args):
    return (B_MAX, K_MAX) if not args else VARIANT_SHAPE


@functools.lru_cache(maxsize=None)
def e64(key, args=()):
    B, K = shape_of(args)
    os_, rows, cand, solved = reference(key, B, K, args)
    worst = 0.0
    for e in OK.ref_envs(B):
        o = os_[e]
        for k in range(K):
            if solved[e, k]:
                V = rows[e][k]["r"].V
                g = [G.reward_gradient(o.net, G.env_args(o), V, cand[e, k], G.limits(o), ext=x) for x in (False, True)]
                worst = max(worst, G.rel_inf(*g))
    return worst


def bar(key, args=()):
    return max(OK.BAR_FACTOR * E64[(key, tuple(args))], OK.BAR_FLOOR)
