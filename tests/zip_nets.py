"""Nets and the oracle for voltage-dependent (ZIP) loads (runpp voltage_depend_loads=True, NetSpec.load_const_z / load_const_i):
test infrastructure only, independent of the product code.

runpp_zip restates pandapower 2.x's scheme [PP-recalled; tests/test_zip_pandapower_pin.py decides it wherever pandapower exists]:
  1. per bus, (ci, cz) = the row-count mean of the fractions of every net.load row at the bus (in service or not);
  2. Sbus(vm) = Sbus * (cp + ci vm + cz vm^2), cp = 1 - (ci + cz), with Sbus the bus's whole net demand (loads minus sgens: the sgens
     of a ZIP bus are scaled too — makeSbus scales PD + jQD, which already holds the sgens);
  3. newtonpf: F0 against the constant-power Sbus; after every voltage update Sbus = makeSbus(vm=|V|), then F; the Jacobian is the
     plain dSbus_dV one (no load derivative);
  4. the DC-angle start uses the constant-power Pbus;
  5. res_bus p / q: each load x scaling x (cp_l + ci_l vm + cz_l vm^2) at the converged vm, minus the sgens (unscaled), plus shunts;
     the slack bus as ever."""
import dataclasses

import numpy as np
import scipy.sparse.linalg as spla

from oracle.pp_restated import (MAX_ITER, TOLERANCE_MVA, PPResult, _cached_ybus, _fx, bus_demand, dc_angles, iterations_agree,
                                jacobian, make_sbus)


def with_zip(net, cz, ci, buses=None):
    """`net` with the loads at `buses` (default: every load off the ext_grid bus) at fractions (cz, ci)"""
    lb = np.asarray(net.load_bus)
    on = lb != net.ext_grid_bus if buses is None else np.isin(lb, buses)
    return dataclasses.replace(net, load_const_z=np.where(on, float(cz), 0.0), load_const_i=np.where(on, float(ci), 0.0))


def zip_bus_coeffs(net):
    """rule 1: (ci, cz) per bus = the row-count mean over the loads at the bus"""
    nb = net.n_bus
    cnt = np.bincount(net.load_bus, minlength=nb).astype(np.float64)
    ci = np.bincount(net.load_bus, weights=net.load_const_i, minlength=nb)
    cz = np.bincount(net.load_bus, weights=net.load_const_z, minlength=nb)
    nz = cnt > 0
    ci[nz] /= cnt[nz]
    cz[nz] /= cnt[nz]
    return ci, cz


def _newton(net, v0, sbus0, ci, cz, tol, max_it, stop=True):
    """rules 2-3; returns (V, converged, iterations, ||F||inf of every iterate formed)"""
    ybus = _cached_ybus(net)[0]
    nb = net.n_bus
    pq = np.setdiff1d(np.arange(nb), [net.ext_grid_bus])
    cp = 1.0 - (ci + cz)
    v = v0.astype(np.complex128).copy()
    va, vm = np.angle(v), np.abs(v)
    f = _fx(ybus, v, sbus0, pq, pq)                       # F0: constant power
    norms = [float(np.linalg.norm(f, np.inf))]
    converged = norms[-1] < tol
    i = 0
    while (not stop or not converged) and i < max_it:
        i += 1
        dx = -spla.spsolve(jacobian(ybus, v, pq, pq), f)
        va[pq] = va[pq] + dx[:len(pq)]
        vm[pq] = vm[pq] + dx[len(pq):]
        v = vm * np.exp(1j * va)
        vm = np.abs(v)
        va = np.angle(v)
        sbus = sbus0 * (cp + ci * vm + cz * vm ** 2)      # makeSbus(baseMVA, bus, gen, vm=Vm)
        f = _fx(ybus, v, sbus, pq, pq)
        norms.append(float(np.linalg.norm(f, np.inf)))
        if not stop and (not np.isfinite(norms[-1]) or norms[-1] > 1e6):
            norms += [np.inf] * (max_it + 1 - len(norms))
            break
        converged = norms[-1] < tol
    return v, bool(converged), i, np.array(norms)


def _start(net, pd_, init):
    v0 = np.full(net.n_bus, net.ext_grid_vm_pu, dtype=np.complex128)
    if init == "dc":
        v0 = v0 * np.exp(1j * dc_angles(net, pd_))      # rule 4: constant-power Pbus
    return v0


def runpp_zip(net, p_load, q_load, p_sgen, q_sgen, raise_on_fail=False, cache=True, tolerance_mva=TOLERANCE_MVA,
              tolerance_is_pu=False, init=None):
    """pp.runpp(net) with voltage_depend_loads=True; the keys of oracle.pp_restated.runpp_restated.  init: "flat" | "dc" | None
    (NetSpec.va_init).  The signature of runpp_restated, so that oracle.env_restated can run on it."""
    if getattr(net, "has_fused_buses", False):
        raise NotImplementedError("runpp_zip: nets with fused buses")
    init = init or getattr(net, "va_init", "flat")
    ybus, yf, yt, br = _cached_ybus(net)
    f, t, _, _, _, _, is_line = br
    ref = int(net.ext_grid_bus)
    pd_, qd = bus_demand(net, p_load, q_load, p_sgen, q_sgen)
    sbus0 = make_sbus(net, pd_, qd)
    ci, cz = zip_bus_coeffs(net)
    tol = tolerance_mva / (1.0 if tolerance_is_pu else net.sn_mva)
    v, converged, it, _ = _newton(net, _start(net, pd_, init), sbus0, ci, cz, tol, MAX_ITER)
    if not converged and raise_on_fail:
        raise RuntimeError(f"Power Flow nr did not converge after {MAX_ITER} iterations!")
    vm = np.abs(v)
    va_deg = np.angle(v) * 180.0 / np.pi
    s_inj = v * np.conj(ybus @ v) * net.sn_mva
    # rule 5: per load, at the converged vm of its bus
    lb = net.load_bus
    vl = vm[lb]
    poly = (1.0 - (net.load_const_z + net.load_const_i)) + net.load_const_i * vl + net.load_const_z * vl ** 2
    p_bus = np.zeros(net.n_bus)
    q_bus = np.zeros(net.n_bus)
    np.add.at(p_bus, lb, np.asarray(p_load) * net.load_scaling * poly)
    np.add.at(q_bus, lb, np.asarray(q_load) * net.load_scaling * poly)
    np.add.at(p_bus, net.sgen_bus, -np.asarray(p_sgen) * net.sgen_scaling)
    np.add.at(q_bus, net.sgen_bus, -np.asarray(q_sgen) * net.sgen_scaling)
    p_bus[ref] = -s_inj[ref].real
    q_bus[ref] = -s_inj[ref].imag
    if net.shunt_bus.shape[0]:
        np.add.at(p_bus, net.shunt_bus, net.shunt_p_mw * vm[net.shunt_bus] ** 2)
        np.add.at(q_bus, net.shunt_bus, net.shunt_q_mvar * vm[net.shunt_bus] ** 2)
    sf = v[f] * np.conj(yf @ v) * net.sn_mva
    st = v[t] * np.conj(yt @ v) * net.sn_mva
    pl_full = np.zeros(net.n_line)
    pl_full[net.line_in_service.astype(bool)] = (sf.real + st.real)[is_line]
    return PPResult(vm_pu=vm, va_degree=va_deg, p_mw=p_bus, q_mvar=q_bus, pl_mw=pl_full,
                    converged=converged, iterations=it, V=v, Sbus=sbus0 * ((1.0 - (ci + cz)) + ci * vm + cz * vm ** 2))


def zip_iterate_norms(net, p_load, q_load, p_sgen, q_sgen, init=None, n_it=MAX_ITER + 2):
    """||F||inf of the start and of the first n_it iterates of runpp_zip's scheme without its stopping rule (tests/edge_rule.py)"""
    init = init or getattr(net, "va_init", "flat")
    pd_, qd = bus_demand(net, p_load, q_load, p_sgen, q_sgen)
    ci, cz = zip_bus_coeffs(net)
    return _newton(net, _start(net, pd_, init), make_sbus(net, pd_, qd), ci, cz, 0.0, n_it, stop=False)[3]


def zip_oracle(net, p_load, q_load, p_sgen, q_sgen, init=None):
    """runpp_zip and the agreement rule of the parity tests for its iteration count"""
    r = runpp_zip(net, p_load, q_load, p_sgen, q_sgen, init=init)
    norms = zip_iterate_norms(net, p_load, q_load, p_sgen, q_sgen, init=init)

    def agrees(it, conv):
        return iterations_agree(int(it), bool(conv), r.iterations, r.converged, norms, 1e-8 / net.sn_mva)
    return r, agrees


def zip_residual_inf(net, v, p_load, q_load, p_sgen, q_sgen):
    """||V conj(Ybus V) - Sbus(|V|)||inf over the non-slack buses (p.u.): the fixed point runpp_zip converges to"""
    ybus = _cached_ybus(net)[0]
    pd_, qd = bus_demand(net, p_load, q_load, p_sgen, q_sgen)
    ci, cz = zip_bus_coeffs(net)
    vm = np.abs(v)
    mis = v * np.conj(ybus @ v) - make_sbus(net, pd_, qd) * ((1.0 - (ci + cz)) + ci * vm + cz * vm ** 2)
    mis = np.delete(mis, net.ext_grid_bus)
    return float(max(np.abs(mis.real).max(), np.abs(mis.imag).max()))
