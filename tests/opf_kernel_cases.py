"""Nets, states, set-points and the extended-precision reference of the OPF kernel tests (tests/test_opf_kernels_gpu.py; the host-only
half in tests/test_opf_cpu.py): test infrastructure only, independent of the product code.

Nets (seeded, netspec._radial_case + synth_profiles, placed at daytime rows so that sqrt(smax^2 - p^2) is neither 0 nor smax):
    tiny                        8 nodes, 1 sgen        sub-lanes of k_opf_linearise with no column and no node
    small15 / small16 / small17 24 nodes               the first stride edge of the columns j = sl, sl + 16, ...
    wide33 / 48 / 49 / 64       72 nodes               the third and fourth column per sub-lane, and the documented maximum
    case33, case141                                    the shipped feeders (case141: two sgens on one bus)
    special                     24 nodes, 9 sgens      a ratio-and-shift transformer with iron losses on an inner branch, a shunt,
                                                       sgen scalings != 1, a junction with four children, an sgen on the slack bus
The reference: the dense Jacobian and M = (Ybus + Ybus^H) / 2 assembled in numpy.longdouble (x87 extended, 64-bit mantissa) from the
float64 Ybus and V, the solve J X = E by a float64 LU refined with longdouble residuals until the correction stops shrinking (at most 2^-54 of the
solution), and everything after it (S, g, H, the loss) in longdouble: the same definition as tests/opf_ref.linearise, a function of V alone."""
import dataclasses
import functools

import numpy as np
import scipy.linalg as sla

from mapdn_amd.netspec import _radial_case, make_case, synth_profiles
from oracle.pp_restated import make_ybus

LD, CLD = np.longdouble, np.clongdouble
REFINE_FLOOR = 2.0 ** -54                          # the last correction of the refined solve, relative: 1 / 256 of the tightest bar (64 ulp)
#          nb  sgens zones trunk seed
RADIAL = dict(tiny=(9, 1, 1, 3, 9001), small15=(25, 15, 3, 4, 9015), small16=(25, 16, 3, 4, 9016), small17=(25, 17, 3, 4, 9017),
              wide33=(73, 33, 8, 9, 9033), wide48=(73, 48, 8, 9, 9048), wide49=(73, 49, 8, 9, 9049), wide64=(73, 64, 8, 9, 9064))
DAYS = 3
BATCHES = dict(tiny=5, small15=3, small16=17, small17=5, wide33=5, wide48=3, wide49=17, wide64=33, case33=33, case141=17, special=17)


def _profiles(net, p_nom, seed):
    q_nom = p_nom * np.tan(np.arccos(0.95))
    w = np.random.default_rng(seed + 7).uniform(0.7, 1.3, net.n_sgen)
    return synth_profiles(p_nom, q_nom, 4.0 * p_nom.sum() * w / w.sum(), days=DAYS, seed=seed)


def _special():
    """22 seeded buses, then: three more leaves on the child end of an inner line, so that this bus is a junction with four children; that
    inner line replaced by a transformer (ratio 0.98, shift 3 degrees, iron losses); a shunt; sgen scalings in 0.8 .. 1.1; a ninth sgen
    on the slack bus"""
    seed = 9100
    net, p_nom = _radial_case("special", 22, 13, 8, 3, 4, 12.47, 10.0, 3.0, seed, 0.05)
    nb = net.n_bus
    f, t = net.line_from_bus.astype(int), net.line_to_bus.astype(int)
    deg = np.bincount(np.concatenate([f, t]), minlength=nb)
    inner = [i for i in range(f.shape[0]) if 0 not in (f[i], t[i]) and deg[f[i]] >= 2 and deg[t[i]] == 2]
    assert inner, "no inner line whose one end has exactly one further neighbour"
    li = inner[0]
    hub = int(t[li])                                 # degree 2: its parent or its one child is the other end; three leaves make 4 or 3 + 1
    new = np.arange(nb, nb + 3)
    zbase = 12.47 ** 2 / net.sn_mva
    keep = np.arange(f.shape[0]) != li
    cat = lambda a, b: np.concatenate([a, b])
    rng = np.random.default_rng(seed)
    net = dataclasses.replace(
        net, bus_vn_kv=cat(net.bus_vn_kv, np.full(3, 12.47)), bus_zone=cat(np.where(np.arange(nb) == net.ext_grid_bus, net.sgen_zone[0], net.bus_zone), np.full(3, net.bus_zone[hub])),
        bus_alias=np.zeros(0, np.int32),
        line_from_bus=cat(net.line_from_bus[keep], np.full(3, hub)), line_to_bus=cat(net.line_to_bus[keep], new),
        line_r_ohm_per_km=cat(net.line_r_ohm_per_km[keep], [0.05, 0.08, 0.06]), line_x_ohm_per_km=cat(net.line_x_ohm_per_km[keep], [0.03, 0.05, 0.05]),
        line_c_nf_per_km=cat(net.line_c_nf_per_km[keep], [8.0, 0.0, 12.0]), line_g_us_per_km=np.zeros(f.shape[0] + 2),
        line_length_km=cat(net.line_length_km[keep], [0.4, 0.7, 0.5]), line_parallel=np.ones(f.shape[0] + 2, np.int32),
        line_in_service=np.ones(f.shape[0] + 2, np.uint8),
        load_bus=cat(net.load_bus, new), load_scaling=np.zeros(0), load_const_z=np.zeros(0), load_const_i=np.zeros(0),
        sgen_bus=cat(net.sgen_bus, [net.ext_grid_bus]), sgen_zone=cat(net.sgen_zone, [net.sgen_zone[0]]),
        sgen_scaling=rng.uniform(0.8, 1.1, 9),
        br_from_bus=np.array([f[li]]), br_to_bus=np.array([t[li]]),
        br_r_pu=np.array([net.line_r_ohm_per_km[li] * net.line_length_km[li] / zbase]),
        br_x_pu=np.array([net.line_x_ohm_per_km[li] * net.line_length_km[li] / zbase + 0.01]),
        br_b_pu=np.array([-0.01]), br_ratio=np.array([0.98]), br_shift_deg=np.array([3.0]), br_g_pu=np.array([0.004]),
        shunt_bus=np.array([int(f[li])]), shunt_p_mw=np.array([0.02]), shunt_q_mvar=np.array([-0.15]))
    p_nom = cat(p_nom, [0.12, 0.2, 0.16])
    return net, _profiles(net, p_nom, seed), hub


@functools.lru_cache(maxsize=None)
def make(name):
    """(NetSpec, Profiles) of a case of this matrix"""
    if name in ("case33", "case141"):
        return make_case(name, days=DAYS)
    if name == "special":
        return _special()[:2]
    nb, ns, zones, trunk, seed = RADIAL[name]
    net, p_nom = _radial_case(name, nb, (6 * nb) // 10, ns, zones, trunk, 12.47, 10.0, 20.0 * nb / 141, seed, 0.05)
    return net, _profiles(net, p_nom, seed)


@functools.lru_cache(maxsize=None)
def backtrack_net(i):
    """the i-th seeded 13-bus feeder (4 sgens) of the backtracking search (tests/golden/make_opf_backtrack.py)"""
    seed = 9200 + i
    net, p_nom = _radial_case(f"backtrack{i}", 13, 8, 4, 2, 3, 12.47, 10.0, 2.0, seed, 0.05)
    return net, _profiles(net, p_nom, seed)


def special_hub():
    return _special()[2]


def rows_of(prof, B):
    """daytime profile rows 09:00 .. 15:00, another one per env"""
    return np.array([prof.start_row(e % (DAYS - 1), 9 + (e * 5) % 7, (e * 7) % prof.intervals_per_hour) for e in range(B)])


def setpoints(name, B, ns):
    """mixed set-points: env 0 all zero; every third env +-1 on some sgens (box rows active at d = 0); the rest seeded uniform in
    (-0.9, 0.9); the last env pinned at +-1 everywhere"""
    rng = np.random.default_rng(sum(map(ord, name)) * 1000 + B)
    a = rng.uniform(-0.9, 0.9, (B, ns))
    a[0] = 0.0
    for e in range(1, B, 3):
        pin = rng.random(ns) < 0.4
        pin[e % ns] = True
        a[e, pin] = np.where(rng.random(int(pin.sum())) < 0.5, -1.0, 1.0)
    if B > 1:
        a[B - 1] = np.where(rng.random(ns) < 0.5, -1.0, 1.0)
    return a


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
class Ref:
    """S [n_bus, ns] (slack row 0), g [ns], H [ns, ns], loss (p.u.), all numpy.longdouble"""

    def __init__(self, S, g, H, loss):
        self.S, self.g, self.H, self.loss = S, g, H, loss


def linearise_ext(net, V, lim) -> Ref:
    """tests/opf_ref.linearise and loss_pu carried above float64 (module docstring).  V complex128 [n_bus], lim = sqrt(smax^2 - p^2)"""
    Y = make_ybus(net)[0].toarray().astype(CLD)
    nb, ns = net.n_bus, net.n_sgen
    pq = np.setdiff1d(np.arange(nb), [net.ext_grid_bus])
    n = pq.shape[0]
    Vx = np.asarray(V).astype(CLD)
    vm = np.abs(Vx)
    I = Y @ Vx
    Vn = Vx / vm
    dS_dVm = Vx[:, None] * np.conj(Y * Vn[None, :]) + np.diag(np.conj(I) * Vn)
    dS_dVa = CLD(1j) * Vx[:, None] * np.conj(np.diag(I) - Y * Vx[None, :])
    sub = lambda A: A[np.ix_(pq, pq)]
    J = np.block([[sub(dS_dVa).real, sub(dS_dVm).real], [sub(dS_dVa).imag, sub(dS_dVm).imag]]).astype(LD)
    E = np.zeros((2 * n, ns), LD)
    where = {int(b): i for i, b in enumerate(pq)}
    w = np.asarray(lim, LD) * np.asarray(net.sgen_scaling, LD) / LD(net.sn_mva)
    for j, b in enumerate(np.asarray(net.sgen_bus)):
        if int(b) in where:
            E[n + where[int(b)], j] = w[j]
    lu = sla.lu_factor(J.astype(np.float64))
    X = np.zeros((2 * n, ns), LD)
    last = np.inf
    for _ in range(12):                              # every pass gains a factor cond(J) 2^-53, down to the floor cond(J) 2^-64
        dx = sla.lu_solve(lu, (E - J @ X).astype(np.float64)).astype(LD)
        X = X + dx
        step = float(np.abs(dx).max() / np.abs(X).max())
        if step <= 2.0 ** -62 or step > 0.25 * last:
            break
        last = step
    assert step <= REFINE_FLOOR, step
    dth, dvm = np.zeros((nb, ns), LD), np.zeros((nb, ns), LD)
    dth[pq], dvm[pq] = X[:n], X[n:]
    dV = (dvm / vm[:, None] + CLD(1j) * dth) * Vx[:, None]
    M = (Y + Y.conj().T) / LD(2)
    MV = M @ Vx
    g = LD(2) * (dV.conj().T @ MV).real
    H = LD(2) * (dV.conj().T @ (M @ dV)).real
    loss = (Vx.conj() @ MV).real
    return Ref(dvm, g, (H + H.T) / LD(2), loss)


def rel_err(x, ref):
    """max |x - ref| relative to the largest magnitude of ref, formed in longdouble"""
    ref = np.asarray(ref, LD)
    scale = np.abs(ref).max()
    return float(np.abs(np.asarray(x, LD) - ref).max() / scale) if scale > 0 else float(np.abs(np.asarray(x, LD)).max())


# ---- states and error figures ---------------------------------------------------------------------------------------------------------
QUANTITIES = ("S", "g", "H", "loss", "violation")
V_BAND = (0.95, 1.05)


def state(name):
    """(net, prof, profile rows [B], set-points [B, ns], s_max [ns]) of a case"""
    net, prof = make(name)
    B = BATCHES[name]
    return net, prof, rows_of(prof, B), setpoints(name, B, net.n_sgen), prof.s_max(1.2)


def ref_envs(B):
    """the envs that get a reference: the first three, the three across the 16-env workgroup edge of k_opf_linearise, the last three"""
    return sorted({e for e in (0, 1, 2, 15, 16, 17, B - 3, B - 2, B - 1) if 0 <= e < B})


def violation_ext(net, V, band=V_BAND):
    vm = np.delete(np.abs(np.asarray(V).astype(CLD)), net.ext_grid_bus)
    return max((vm - LD(band[1])).max(), (LD(band[0]) - vm).max(), LD(0))


def errors(net, V, lim, got, band=V_BAND):
    """the error of `got` = dict(S [n_bus, ns], g, H, loss (p.u.), violation) against the extended reference at V: S, g, H and the loss
    relative to the largest magnitude of the reference array, the violation absolute, with the reference's violation beside it"""
    ref = linearise_ext(net, V, lim)
    viol = violation_ext(net, V, band)
    return dict(S=rel_err(got["S"], ref.S), g=rel_err(got["g"], ref.g), H=rel_err(got["H"], ref.H), loss=rel_err([got["loss"]], [ref.loss]),
                violation=float(abs(LD(got["violation"]) - viol))), float(viol)


def worst(per_env):
    """per quantity the worst error over the envs of a case: [(errors, reference violation)] -> dict; the violation relative to the
    largest violation among them"""
    vmax = max(v for _, v in per_env)
    out = {q: max(e[q] for e, _ in per_env) for q in QUANTITIES}
    if vmax > 0:
        out["violation"] /= vmax
    return out


def e64(name):
    """the error of the plain float64 dense reference (tests/opf_ref.linearise, loss_pu, violation_of) against the extended one, at the
    oracle's converged V of the case's reference envs: what a float64 evaluation of the definition is good for on this net"""
    from oracle.pp_restated import runpp_restated
    from tests import opf_ref as R
    net, prof, rows, a, smax = state(name)
    ybus = make_ybus(net)[0]
    per_env = []
    for e in ref_envs(len(rows)):
        t = rows[e]
        lim = R.limits(prof.pv[t], smax)
        res = runpp_restated(net, prof.load_p[t], prof.load_q[t], prof.pv[t], lim * a[e])
        assert res.converged, (name, e)
        L = R.linearise(net, res.V, lim)
        got = dict(S=L.S, g=L.g, H=L.H, loss=R.loss_pu(ybus, res.V), violation=R.violation_of(np.abs(res.V), net, *V_BAND))
        per_env.append(errors(net, res.V, lim, got))
    return worst(per_env)


# ---- the bars of the linearisation in tests/test_opf_kernels_gpu.py -----------------------------------------------
# E64: per case and quantity the error of the plain float64 dense reference (opf_ref.linearise) against the extended one, measured on the
# CPU at the oracle's V of the same states (e64 above; tests/test_opf_cpu.py recomputes all of them).  S, g, H per env relative to the
# largest magnitude of the array, the loss relative to itself, the violation relative to the largest violation of the case.  The
# kernel's bar is 16 x E64 — its block LU takes no pivoting and sums in another order — and never tighter than 64 ulp.
E64 = dict(
    tiny=dict(S=1.04e-14, g=9.74e-15, H=2.75e-15, loss=6.90e-13, violation=1.11e-15),
    small15=dict(S=4.91e-15, g=1.96e-13, H=7.39e-15, loss=4.55e-13, violation=5.89e-16),
    small16=dict(S=1.64e-14, g=1.93e-13, H=2.42e-14, loss=4.07e-12, violation=6.99e-15),
    small17=dict(S=2.48e-14, g=1.84e-13, H=1.50e-14, loss=1.04e-12, violation=3.73e-15),
    wide33=dict(S=3.86e-14, g=1.07e-12, H=3.10e-14, loss=9.40e-12, violation=2.53e-15),
    wide48=dict(S=4.67e-14, g=6.00e-13, H=5.59e-14, loss=8.15e-12, violation=2.32e-15),
    wide49=dict(S=3.09e-14, g=8.97e-13, H=3.44e-14, loss=4.45e-12, violation=3.14e-15),
    wide64=dict(S=8.20e-14, g=4.39e-12, H=1.18e-13, loss=9.76e-12, violation=4.84e-15),
    case33=dict(S=1.68e-14, g=3.10e-13, H=2.82e-14, loss=1.94e-12, violation=1.68e-15),
    case141=dict(S=1.42e-13, g=5.60e-12, H=1.64e-13, loss=8.90e-12, violation=3.24e-15),
    special=dict(S=8.03e-14, g=7.73e-13, H=2.38e-14, loss=1.16e-12, violation=4.85e-15),
)
BAR_FACTOR, BAR_FLOOR = 16.0, 64.0 * np.finfo(np.float64).eps


def bar(case, q):
    return max(BAR_FACTOR * E64[case][q], BAR_FLOOR)
