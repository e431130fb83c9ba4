"""The reference of voltage_vjp and what tests/test_voltage_vjp_cpu.py and tests/test_voltage_vjp_gpu.py share: test
infrastructure only, independent of the product code.

voltage_vjp(): for one converged V and one cotangent (cot_vm, cot_va) over the buses,
    g_j = sum_b cot_vm_b d|V_b| / da_j + cot_va_b d va_degree_b / da_j
from the definition: the power flow's Jacobian J by (theta, |V|) of the non-slack buses is oracle.pp_restated.jacobian, the right-hand
side is c = (cot_va 180 / pi, cot_vm) over those buses, J' lambda = c is numpy.linalg.solve, and an action a_j moves the scheduled Q of
its bus by w_j = lim_j scaling_j / sn_mva:  g_j = w_j lambda_(Q row of the bus)  (0 for a bus that is the slack).  There is no direct term.
ext=True carries the same evaluation above float64 the way tests/grad_ref.reward_gradient does: numpy.longdouble assembly of J, the solve
by a float64 LU refined with longdouble residuals (exact residuals where those stall above the floor)."""
import numpy as np
import scipy.linalg as sla

from oracle.pp_restated import jacobian, make_ybus
from tests import grad_ref as G
from tests import opf_kernel_cases as OK

LD, CLD = G.LD, G.CLD


class Adjoint:
    """J' of the power flow at V over pq = the non-slack buses, rows (theta of pq, |V| of pq), factorised once: solve(c) -> lambda [2n]"""

    def __init__(self, net, V, ext=False):
        nb = net.n_bus
        self.ext = ext
        self.pq = pq = np.setdiff1d(np.arange(nb), [net.ext_grid_bus])
        self.n = pq.shape[0]
        ybus = make_ybus(net)[0]
        if not ext:
            self.JT = jacobian(ybus, np.asarray(V).astype(np.complex128), pq, pq).toarray().T
            return
        Vx = np.asarray(V).astype(CLD)
        vm = np.abs(Vx)
        Y = ybus.toarray().astype(CLD)
        I = Y @ Vx
        Vn = Vx / vm
        dS_dVm = Vx[:, None] * np.conj(Y * Vn[None, :]) + np.diag(np.conj(I) * Vn)
        dS_dVa = CLD(1j) * Vx[:, None] * np.conj(np.diag(I) - Y * Vx[None, :])
        sub = lambda A: A[np.ix_(pq, pq)]
        self.JT = np.block([[sub(dS_dVa).real, sub(dS_dVm).real], [sub(dS_dVa).imag, sub(dS_dVm).imag]]).astype(LD).T
        self.lu = sla.lu_factor(self.JT.astype(np.float64))

    def solve(self, c):
        if not self.ext:
            return np.linalg.solve(self.JT, np.asarray(c, np.float64))
        JT, c = self.JT, np.asarray(c, LD)
        lam = np.zeros(2 * self.n, LD)
        if np.abs(c).max() == 0:
            return lam
        last, exact, step = np.inf, False, np.inf
        for _ in range(24):
            res = G._exact_residual(JT, lam, c) if exact else c - JT @ lam
            dx = sla.lu_solve(self.lu, res.astype(np.float64)).astype(LD)
            lam = lam + dx
            step = float(np.abs(dx).max() / np.abs(lam).max())
            if step <= 2.0 ** -62:
                break
            if step > 0.25 * last:
                if exact or step <= OK.REFINE_FLOOR:
                    break
                exact = True
            last = step
        assert step <= OK.REFINE_FLOOR, step
        return lam


def voltage_vjp(net, V, lim, cot_vm, cot_va=None, ext=False, adjoint=None):
    """g [ns] for one cotangent (cot_vm, cot_va: [n_bus] each, None = zeros) at the converged V (complex [n_bus]) and the limits lim [ns];
    float64, or longdouble with ext.  The slack's cotangent entries are not read.  adjoint: Adjoint(net, V, ext), to share one among
    several cotangents."""
    R = LD if ext else np.float64
    nb, ns = net.n_bus, net.n_sgen
    pq = np.setdiff1d(np.arange(nb), [net.ext_grid_bus])
    n = pq.shape[0]
    cvm = np.zeros(nb, R) if cot_vm is None else np.asarray(cot_vm).astype(R)
    cva = np.zeros(nb, R) if cot_va is None else np.asarray(cot_va).astype(R)
    deg = R(180) / np.arccos(R(-1))
    lam = (adjoint or Adjoint(net, V, ext)).solve(np.concatenate([cva[pq] * deg, cvm[pq]]))
    where = {int(b): i for i, b in enumerate(pq)}
    w = np.asarray(lim).astype(R) * np.asarray(net.sgen_scaling).astype(R) / R(net.sn_mva)
    g = np.zeros(ns, R)
    for j, b in enumerate(np.asarray(net.sgen_bus)):
        if int(b) in where:
            g[j] = w[j] * lam[n + where[int(b)]]
    return g


def barrier_cotangent(o, vm):
    """cot_vm [n_bus] under which voltage_vjp is the barrier part of the env's reward gradient: -voltage_weight / n_bus barrier'(|V_b|)"""
    vm = np.asarray(vm, np.float64)
    return -(np.float64(o.voltage_weight) / np.float64(o.net.n_bus)) * G.barrier_derivative(o.args["voltage_barrier_type"], vm)


def direct_term(o, a, lim):
    """the part of tests/grad_ref.reward_gradient that does not go through the power flow (absent with line_weight)"""
    net = o.net
    if o.line_weight is not None:
        return np.zeros(net.n_sgen)
    sc = np.asarray(net.sgen_scaling, np.float64)
    return -(np.float64(o.q_weight) / np.float64(net.n_sgen)) * np.sign(lim * a * sc) * lim * sc


def cotangents(net, M, seed):
    """(cot_vm, cot_va) [M, n_bus] each: row 0 random in both, row 1 a unit cotangent on one non-slack bus's |V|, row 2 on one bus's angle,
    the rest random; the magnitudes keep the two parts of a row comparable (an angle in degrees moves about 60 times a |V|)"""
    rng = np.random.default_rng(seed)
    nb = net.n_bus
    cvm, cva = rng.uniform(-1.0, 1.0, (M, nb)), rng.uniform(-1.0, 1.0, (M, nb)) / 60.0
    pq = np.setdiff1d(np.arange(nb), [net.ext_grid_bus])
    if M > 1:
        cvm[1], cva[1] = 0.0, 0.0
        cvm[1, pq[rng.integers(len(pq))]] = 1.0
    if M > 2:
        cvm[2], cva[2] = 0.0, 0.0
        cva[2, pq[rng.integers(len(pq))]] = 1.0
    return cvm, cva
