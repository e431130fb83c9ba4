"""Nets and the oracle for generators (net.gen: voltage-controlled GEN BUSES, NetSpec.gen_bus / gen_p_mw / gen_vm_pu / gen_scaling):
test infrastructure only, independent of the product code.

runpp_gen restates what pp.runpp does with net.gen at its defaults [PP-recalled; tests/test_gen_pandapower_pin.py decides it wherever
pandapower exists], from the oracle's own pieces (_cached_ybus, bus_demand, make_sbus, newtonpf(pv=...), dc_angles):
  1. an in-service net.gen row makes its bus a gen bus: |V| held at vm_pu, P = p_mw * scaling injected, Q free (enforce_q_lims=False);
  2. Sbus_k = (P_gen - PD_k - j QD_k) / sn_mva; unknowns theta on gen and PQ buses, |V| on PQ buses; F = [Re mis[pvpq]; Im mis[pq]];
  3. start: the slack at its set-point, a gen bus at its vm_pu, every PQ bus at the mean of the vm_pu of the ext_grid and of ALL gen rows
     (NetSpec.start_vm_pu: vm_init_pu, which the converter computes from the full table); the DC-angle start uses Pbus with P_gen;
  4. res_gen p_mw = p_mw * scaling, q_mvar = Im(V_k conj((Ybus V)_k)) sn_mva + QD_k (QD with the shunt's q |V|^2), vm_pu / va_degree of
     the bus; res_bus of a gen bus: p = loads - sgens - P_gen (+ shunt), q = -Im(V conj(Ybus V)) sn_mva (the slack row's form)."""
import dataclasses

import numpy as np
import scipy.sparse.linalg as spla

from mapdn_amd.netspec import NetSpec, Profiles, case33_meshed, make_case
from oracle.pp_restated import (MAX_ITER, TOLERANCE_MVA, PPResult, _cached_ybus, _fx, bus_demand, dc_angles, iterations_agree, jacobian,
                                make_sbus, newtonpf, runpp_restated)


def with_gens(net, gens, vm_init_pu=0.0):
    """`net` with the generators [(bus, p_mw, vm_pu), ...] (scaling 1)"""
    g = list(gens)
    return dataclasses.replace(net, gen_bus=np.array([b for b, _, _ in g], np.int32), gen_p_mw=np.array([p for _, p, _ in g], np.float64),
                               gen_vm_pu=np.array([v for _, _, v in g], np.float64), gen_scaling=np.ones(len(g)), vm_init_pu=vm_init_pu)


def _types(net):
    ref = int(net.ext_grid_bus)
    pv = np.asarray(net.gen_bus, np.int64)
    pq = np.setdiff1d(np.arange(net.n_bus), np.r_[ref, pv])
    return ref, pv, pq


def gen_p_bus(net):
    """P_gen per bus (MW)"""
    pg = np.zeros(net.n_bus)
    np.add.at(pg, net.gen_bus, net.gen_p_mw * net.gen_scaling)
    return pg


def start_vm(net):
    """rule 3, computed here (not NetSpec.start_vm_pu, which the product passes to the library): the converter's mean over the FULL gen
    table when the NetSpec carries one (vm_init_pu > 0), else the mean over the ext_grid and the NetSpec's own gen rows"""
    if net.vm_init_pu > 0.0:
        return float(net.vm_init_pu)
    total = float(net.ext_grid_vm_pu)
    for v in net.gen_vm_pu:                                       # in table order, the ext_grid first
        total += float(v)
    return total / (1 + net.n_gen)


def _start(net, pd_eff, init):
    """rule 3"""
    v0 = np.full(net.n_bus, start_vm(net), dtype=np.complex128)
    v0[net.ext_grid_bus] = net.ext_grid_vm_pu
    v0[net.gen_bus] = net.gen_vm_pu
    if init == "dc":
        v0 = v0 * np.exp(1j * dc_angles(net, pd_eff))           # P_gen as negative demand
    return v0


def runpp_gen(net, p_load, q_load, p_sgen, q_sgen, raise_on_fail=False, cache=True, tolerance_mva=TOLERANCE_MVA, tolerance_is_pu=False,
              init=None):
    """pp.runpp(net) on a net with generators; the keys of oracle.pp_restated.runpp_restated plus res_gen.  init: "flat" | "dc" | None
    (NetSpec.va_init).  The signature of runpp_restated, so that oracle.env_restated can run on it."""
    init = init or getattr(net, "va_init", "flat")
    if getattr(net, "has_fused_buses", False):
        if net.n_gen:
            raise NotImplementedError("runpp_gen: generators on a net with fused buses")
        return runpp_restated(net, p_load, q_load, p_sgen, q_sgen, raise_on_fail, cache, tolerance_mva, tolerance_is_pu, init)
    ybus, yf, yt, br = _cached_ybus(net)
    f, t, _, _, _, _, is_line = br
    ref, pv, pq = _types(net)
    pd_, qd = bus_demand(net, p_load, q_load, p_sgen, q_sgen)
    pg = gen_p_bus(net)
    sbus = make_sbus(net, pd_ - pg, qd)                         # rule 2
    tol = tolerance_mva / (1.0 if tolerance_is_pu else net.sn_mva)
    v, converged, it = newtonpf(ybus, sbus, _start(net, pd_ - pg, init), np.array([ref]), pv, pq, tol)
    if not converged and raise_on_fail:
        raise RuntimeError(f"Power Flow nr did not converge after {MAX_ITER} iterations!")
    vm = np.abs(v)
    va_deg = np.angle(v) * 180.0 / np.pi
    s_inj = v * np.conj(ybus @ v) * net.sn_mva
    p_bus, q_bus = pd_ - pg, qd.copy()
    p_bus[ref] = -s_inj[ref].real
    q_bus[ref] = -s_inj[ref].imag
    if net.shunt_bus.shape[0]:
        np.add.at(p_bus, net.shunt_bus, net.shunt_p_mw * vm[net.shunt_bus] ** 2)
        np.add.at(q_bus, net.shunt_bus, net.shunt_q_mvar * vm[net.shunt_bus] ** 2)
    q_gen = s_inj[pv].imag + q_bus[pv]                          # rule 4: QD_k holds the shunt
    q_bus[pv] = -s_inj[pv].imag
    sf = v[f] * np.conj(yf @ v) * net.sn_mva
    st = v[t] * np.conj(yt @ v) * net.sn_mva
    pl_full = np.zeros(net.n_line)
    pl_full[net.line_in_service.astype(bool)] = (sf.real + st.real)[is_line]
    res_gen = dict(p_mw=net.gen_p_mw * net.gen_scaling, q_mvar=q_gen, vm_pu=vm[pv], va_degree=va_deg[pv])
    return PPResult(vm_pu=vm, va_degree=va_deg, p_mw=p_bus, q_mvar=q_bus, pl_mw=pl_full, converged=converged, iterations=it, V=v,
                    Sbus=sbus, res_gen=res_gen)


def gen_iterate_norms(net, p_load, q_load, p_sgen, q_sgen, init=None, n_it=MAX_ITER + 2):
    """||F||inf over [P at pvpq; Q at pq] of the start and of the first n_it Newton iterates (newtonpf's arithmetic, no stopping rule)"""
    init = init or getattr(net, "va_init", "flat")
    ybus = _cached_ybus(net)[0]
    ref, pv, pq = _types(net)
    pvpq = np.r_[pv, pq]
    pd_, qd = bus_demand(net, p_load, q_load, p_sgen, q_sgen)
    pg = gen_p_bus(net)
    sbus = make_sbus(net, pd_ - pg, qd)
    v = _start(net, pd_ - pg, init)
    va, vm = np.angle(v), np.abs(v)
    out = []
    for _ in range(n_it + 1):
        fx = _fx(ybus, v, sbus, pvpq, pq)
        out.append(float(np.linalg.norm(fx, np.inf)))
        if not np.isfinite(out[-1]) or out[-1] > 1e6:
            out += [np.inf] * (n_it + 1 - len(out))
            break
        dx = -spla.spsolve(jacobian(ybus, v, pvpq, pq), fx)
        va[pvpq] += dx[:len(pvpq)]
        vm[pq] += dx[len(pvpq):]
        v = vm * np.exp(1j * va)
        vm, va = np.abs(v), np.angle(v)
    return np.array(out)


def gen_oracle(net, p_load, q_load, p_sgen, q_sgen, init=None):
    """runpp_gen and the agreement rule of the parity tests for its iteration count"""
    r = runpp_gen(net, p_load, q_load, p_sgen, q_sgen, init=init)
    norms = gen_iterate_norms(net, p_load, q_load, p_sgen, q_sgen, init=init)

    def agrees(it, conv):
        return iterations_agree(int(it), bool(conv), r.iterations, r.converged, norms, 1e-8 / net.sn_mva)
    return r, agrees


def gen_residual_inf(net, v, p_load, q_load, p_sgen, q_sgen):
    """||[Re mis[pvpq]; Im mis[pq]]||inf of V conj(Ybus V) - Sbus (p.u.): the equations runpp_gen solves"""
    ybus = _cached_ybus(net)[0]
    _, pv, pq = _types(net)
    pd_, qd = bus_demand(net, p_load, q_load, p_sgen, q_sgen)
    return float(np.abs(_fx(ybus, v, make_sbus(net, pd_ - gen_p_bus(net), qd), np.r_[pv, pq], pq)).max())


def q_bars(net, V, Vref):
    """per gen bus: bar (i) 4 (m + 2) 2^-52 sn sum_j |V_k| |Y_kj| |V_j| — the forward-error bound of the m-term dot product with a factor 4
    for the complex products — and the first-order propagation of a voltage difference, sn sum_j |Y_kj| (|V_k| d_j + |V_j| d_k)"""
    ybus = _cached_ybus(net)[0]
    bar_i, prop = [], []
    d = np.abs(V - Vref)
    for k in net.gen_bus:
        row = ybus.getrow(int(k))
        cols, ay = row.indices, np.abs(row.data)
        m = cols.shape[0]
        bar_i.append(4.0 * (m + 2) * 2.0 ** -52 * net.sn_mva * np.sum(np.abs(V[k]) * ay * np.abs(V[cols])))
        prop.append(net.sn_mva * np.sum(ay * (np.abs(V[k]) * d[cols] + np.abs(V[cols]) * d[k])))
    return np.array(bar_i), np.array(prop)


def inputs(net, prof, B, seed):
    """random profile rows, q from U(-0.8, 0.8) x limit (the inputs of tests/test_zip_loads_gpu.py)"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, prof.n_rows, B)
    smax = prof.s_max()
    pl, ql, pv = prof.load_p[rows], prof.load_q[rows], prof.pv[rows]
    qs = rng.uniform(-0.8, 0.8, (B, net.n_sgen)) * np.sqrt(np.maximum(smax ** 2 - pv ** 2, 0.0))
    return pl, ql, pv, qs


# ---- the nets of the parity tests ------------------------------------------------------------------------------------------
GENS = dict(
    leaf=[(32, 0.3, 1.00)],
    mixed=[(32, 0.3, 1.02), (2, 0.5, 1.00), (1, 0.2, 1.01)],
    chain=[(5, 0.4, 1.0), (6, 0.4, 1.0), (7, 0.2, 1.0)],
    meshed=[(32, 0.3, 1.0), (2, 0.5, 1.02)],
    c141=[(10, 2.0, 1.00), (60, 1.0, 1.01), (140, 0.5, 0.99)],
    far=[(32, 0.3, 1.25)],
)
RADIAL = ("leaf", "mixed", "chain", "all", "c141", "far")


def gen_case(name):
    """(NetSpec with generators, Profiles) of a row of the table"""
    if name == "c141":
        net, prof = make_case("case141")
        return with_gens(net, GENS[name]), prof
    net, prof = make_case("case33")
    if name == "mixed":
        net = dataclasses.replace(net, ext_grid_vm_pu=1.03)
    if name == "meshed":
        net = case33_meshed(net, 5)
    if name == "all":
        return with_gens(net, [(b, 0.05, 1.0) for b in range(net.n_bus) if b != net.ext_grid_bus]), prof
    return with_gens(net, GENS[name]), prof


def tiny_net(n_bus):
    """a hand-built chain: slack - gen (2 buses) or slack - PQ - gen (3 buses), 12.66 kV, sn_mva 1; the gen bus carries the one sgen
    (an agent is mandatory) and a load"""
    assert n_bus in (2, 3)
    nl = n_bus - 1
    zone = np.zeros(n_bus, np.int32); zone[-1] = 1
    net = NetSpec(name=f"tiny{n_bus}", bus_vn_kv=np.full(n_bus, 12.66), bus_zone=zone,
                  line_from_bus=np.arange(nl, dtype=np.int32), line_to_bus=np.arange(1, n_bus, dtype=np.int32),
                  line_r_ohm_per_km=np.full(nl, 0.5), line_x_ohm_per_km=np.full(nl, 0.4), line_c_nf_per_km=np.zeros(nl),
                  line_g_us_per_km=np.zeros(nl), line_length_km=np.ones(nl), line_parallel=np.ones(nl, np.int32),
                  line_in_service=np.ones(nl, np.uint8), load_bus=np.arange(1, n_bus, dtype=np.int32),
                  sgen_bus=np.array([n_bus - 1], np.int32), sgen_zone=np.array([1], np.int32), ext_grid_bus=0, ext_grid_vm_pu=1.0,
                  sn_mva=1.0, f_hz=50.0)
    return with_gens(net, [(n_bus - 1, 0.4, 1.02)])


def flat_profiles(net, p_load, q_load, pv, T=1440, seed=0, spread=0.25):
    """a profile table of T rows around the given element values (x U(1 - spread, 1 + spread) per row), two days of 3-minute rows"""
    rng = np.random.default_rng(seed)
    f = 1.0 - spread + 2.0 * spread * rng.random((T, 1))
    return Profiles(pv=np.asarray(pv)[None, :] * rng.uniform(0.0, 1.2, (T, net.n_sgen)), load_p=np.asarray(p_load)[None, :] * f,
                    load_q=np.asarray(q_load)[None, :] * f, time_delta_min=3, days=2)


def tiny_case(n_bus):
    net = tiny_net(n_bus)
    return net, flat_profiles(net, np.full(net.n_load, 0.3), np.full(net.n_load, 0.1), np.array([0.2]))


def gen_substation(out_of_service_row=True):
    """tests/test_data_ingestion.py::substation_net with a generator at bus 2 (20 kV, zone1) and, optionally, an out-of-service gen row
    whose vm_pu still counts in the start of the PQ buses"""
    import pandas as pd

    from tests.test_data_ingestion import substation_net
    pnet = substation_net()
    rows = dict(name=["g0", "g1"], bus=[2, 4], p_mw=[0.6, 0.3], vm_pu=[1.01, 1.05], sn_mva=[np.nan, np.nan], min_q_mvar=[-0.1, -0.1],
                max_q_mvar=[0.1, 0.1], scaling=[0.9, 1.0], slack=[False, False], in_service=[True, False], type=[None, None])
    df = pd.DataFrame(rows)
    pnet["gen"] = df if out_of_service_row else df.iloc[:1].copy()
    return pnet
