"""Nets and oracle helpers for the DC-angle start (runpp init="dc", mapdn_env_config.nr_init = 2): test infrastructure only."""
import dataclasses

import numpy as np

from mapdn_amd.netspec import NetSpec
from oracle.pp_restated import (MAX_ITER, _cached_ybus, _fx, bus_demand, dc_angles, iterations_agree, jacobian, make_sbus,
                                runpp_restated)
import scipy.sparse.linalg as spla


def hv_front(net: NetSpec, shift_deg: float = 150.0, line_km: float = 30.0) -> NetSpec:
    """`net` fed from a 110 kV grid: a new slack bus -> 110 kV line -> a second 110 kV bus -> transformer (phase shift `shift_deg`) -> the
    old ext_grid bus.  A line at a bus above 70 kV: runpp's defaults start this net from the DC power flow's angles."""
    nb = net.n_bus
    hv, tb, lv = nb, nb + 1, int(net.ext_grid_bus)
    sn = net.sn_mva
    cat = lambda a, b, dt=None: np.concatenate([np.asarray(a), np.asarray(b, dtype=dt if dt else np.asarray(a).dtype)])
    x_tr = 0.12 * sn / 25.0                                   # a 25 MVA unit with vk = 12 %, on the net's base
    return dataclasses.replace(
        net, name=f"{net.name}_hv{int(shift_deg)}", va_init="dc",
        bus_vn_kv=cat(net.bus_vn_kv, [110.0, 110.0]), bus_zone=cat(net.bus_zone, [0, 0]),
        line_from_bus=cat(net.line_from_bus, [hv]), line_to_bus=cat(net.line_to_bus, [tb]),
        line_r_ohm_per_km=cat(net.line_r_ohm_per_km, [0.06]), line_x_ohm_per_km=cat(net.line_x_ohm_per_km, [0.4]),
        line_c_nf_per_km=cat(net.line_c_nf_per_km, [9.0]), line_g_us_per_km=cat(net.line_g_us_per_km, [0.0]),
        line_length_km=cat(net.line_length_km, [line_km]), line_parallel=cat(net.line_parallel, [1]),
        line_in_service=cat(net.line_in_service, [1]),
        br_from_bus=cat(net.br_from_bus, [tb], np.int32), br_to_bus=cat(net.br_to_bus, [lv], np.int32),
        br_r_pu=cat(net.br_r_pu, [0.004 * sn / 25.0], np.float64), br_x_pu=cat(net.br_x_pu, [x_tr], np.float64),
        br_b_pu=cat(net.br_b_pu, [0.0], np.float64), br_ratio=cat(net.br_ratio, [1.0], np.float64),
        br_shift_deg=cat(net.br_shift_deg, [shift_deg], np.float64), br_g_pu=cat(net.br_g_pu, [0.0], np.float64),
        ext_grid_bus=hv, bus_alias=np.arange(nb + 2))


def dc_iterate_norms(net, p_load, q_load, p_sgen, q_sgen, n_it=MAX_ITER + 2):
    """||F||inf of the DC start and of the first n_it Newton iterates from it (oracle.pp_restated.iterate_norms for init="dc")"""
    ybus = _cached_ybus(net)[0]
    nb = net.n_bus
    pq = np.setdiff1d(np.arange(nb), [net.ext_grid_bus])
    pd_, qd = bus_demand(net, p_load, q_load, p_sgen, q_sgen)
    sbus = make_sbus(net, pd_, qd)
    v = np.full(nb, net.ext_grid_vm_pu, dtype=np.complex128) * np.exp(1j * dc_angles(net, pd_))
    va, vm = np.angle(v), np.abs(v)
    out = []
    for _ in range(n_it + 1):
        f = _fx(ybus, v, sbus, pq, pq)
        out.append(float(np.linalg.norm(f, np.inf)))
        if not np.isfinite(out[-1]) or out[-1] > 1e6:
            out += [np.inf] * (n_it + 1 - len(out)); break
        dx = -spla.spsolve(jacobian(ybus, v, pq, pq), f)
        va[pq] += dx[:len(pq)]; vm[pq] += dx[len(pq):]
        v = vm * np.exp(1j * va); vm = np.abs(v); va = np.angle(v)
    return np.array(out)


def dc_oracle(net, p_load, q_load, p_sgen, q_sgen):
    """runpp_restated(init="dc") and the agreement rule of the parity tests for its iteration count"""
    r = runpp_restated(net, p_load, q_load, p_sgen, q_sgen, init="dc")
    norms = dc_iterate_norms(net, p_load, q_load, p_sgen, q_sgen)

    def agrees(it, conv):
        return iterations_agree(int(it), bool(conv), r.iterations, r.converged, norms, net_tol(net))
    return r, agrees


def net_tol(net):
    return 1e-8 / net.sn_mva
