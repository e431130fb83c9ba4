"""On-disk formats on either side of the hot path.

* the three CSV profile tables of a MAPDN scenario directory — same parsing rules as the reference
  loaders (voltage_control_env.py:407-438): first column = timestamp, remaining columns = one
  element each, multiplied by pv_scale / demand_scale; the sampling interval and the day count
  come from the index exactly like `_select_start_day` (:394-398);
* `NetSpec` <-> `netspec.npz` (the pandapower columns the path reads, see netspec.py);
* `from_pandapower(net)`: pandapower tables -> NetSpec, i.e. what pd2ppc builds for runpp's defaults — lines with their
  switches, two-winding transformers (T -> pi, tap changer), load / sgen scaling and in_service, shunts; everything
  the hot path cannot represent is refused loudly.
"""
from __future__ import annotations

import dataclasses
import os

import numpy as np

from .netspec import NetSpec, Profiles

CSV_NAMES = ("pv_active.csv", "load_active.csv", "load_reactive.csv")


def load_profiles_csv(data_path: str, pv_scale: float = 1.0, demand_scale: float = 1.0) -> Profiles:
    import pandas as pd
    tabs = []
    for name, scale in zip(CSV_NAMES, (pv_scale, demand_scale, demand_scale)):
        df = pd.read_csv(os.path.join(data_path, name), index_col=None, float_precision="round_trip")   # :412,423,434
        idx = pd.to_datetime(df.iloc[:, 0])                                        # :413
        tabs.append((idx, df.iloc[::1, 1:].to_numpy(dtype=np.float64) * scale))    # :415
    idx = tabs[0][0]
    pv_days = (idx.iloc[-1] - idx.iloc[0]).days                                    # :395
    time_delta = (idx.iloc[1] - idx.iloc[0]).seconds // 60                         # :396
    if not all(t[1].shape[0] == tabs[0][1].shape[0] for t in tabs):
        raise ValueError("the three profile tables must have the same number of rows")
    return Profiles(pv=tabs[0][1], load_p=tabs[1][1], load_q=tabs[2][1], time_delta_min=int(time_delta), days=int(pv_days))


def save_profiles_csv(prof: Profiles, data_path: str, start="2012-01-01 00:00:00", float_format="%.17g") -> None:
    """Write tables in the reference's CSV layout (used by tests and to export synthetic scenarios).
    %.17g text round-trips through `float_precision="round_trip"` (load_profiles_csv); pandas' default parser —
    the one the reference uses (:412) — is exact only for <= 15 significant digits."""
    import pandas as pd
    os.makedirs(data_path, exist_ok=True)
    idx = pd.date_range(start=start, periods=prof.n_rows, freq=f"{prof.time_delta_min}min")
    for name, tab in zip(CSV_NAMES, (prof.pv, prof.load_p, prof.load_q)):
        df = pd.DataFrame(tab, columns=[str(i) for i in range(tab.shape[1])])
        df.insert(0, "time", idx.strftime("%Y-%m-%d %H:%M:%S"))
        df.to_csv(os.path.join(data_path, name), index=False, float_format=float_format)


def save_netspec(net: NetSpec, path: str) -> None:
    d = {}
    for f in dataclasses.fields(net):
        v = getattr(net, f.name)
        d[f.name] = np.asarray(v) if not isinstance(v, str) else np.array(v)
    np.savez_compressed(path, **d)


def load_netspec(path: str) -> NetSpec:
    z = np.load(path, allow_pickle=False)
    kw = {}
    for f in dataclasses.fields(NetSpec):
        if f.name not in z.files:
            continue
        v = z[f.name]
        kw[f.name] = str(v) if f.name == "name" else (v.item() if v.shape == () else v)
    return NetSpec(**kw)


def _col(df, name, default):
    """column `name` of a pandapower table as float64, `default` where the column is missing or NaN"""
    if name not in df:
        return np.full(len(df), float(default))
    v = df[name].to_numpy(dtype=np.float64, na_value=np.nan)
    return np.where(np.isnan(v), float(default), v)


def _rating(v):
    """a thermal rating column: NaN (= unrated, loading_percent NaN) wherever the table holds no finite positive number"""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(v) & (v > 0.0), v, np.nan)


def trafo_to_pi(trafo, bus_vn_kv: np.ndarray, net_sn_mva: float, calculate_voltage_angles: bool = False):
    """pandapower 2.7.0 build_branch._calc_branch_values_from_trafo_df with runpp's defaults (trafo_model="t",
    no tap-dependent impedance), restated [PP-recalled; SURVEY.md Appendix A.2]: two-winding transformers ->
    ppc branch columns (f = hv_bus, t = lv_bus, r, x, b, g, ratio, shift) in per unit on `net_sn_mva`.

      _calc_tap_from_dataframe      vn_hv/lv *= 1 + (tap_pos - tap_neutral) * tap_step_percent / 100 on tap_side
      _calc_nominal_ratio_...       ratio = (vn_trafo_hv / vn_hv_bus) / (vn_trafo_lv / vn_lv_bus)
      _calc_r_x_from_dataframe      tap_lv = (vn_trafo_lv / vn_lv_bus)^2 * net_sn;  z = vk% / 100 / sn_trafo * tap_lv;
                                    r = vkr% / 100 / sn_trafo * tap_lv;  x = sign(z) sqrt(z^2 - r^2);  both / parallel
      _calc_y_from_dataframe        baseR = vn_lv_bus^2 / net_sn;  b_real = pfe_kw * 1e-3 / vn_lv_kv^2 * baseR;
                                    b_img = sqrt(max(0, (i0% / 100 * sn_trafo)^2 - (pfe_kw * 1e-3)^2)) * baseR / vn_lv_kv^2;
                                    y = (-1j * b_real - b_img * sign(i0%)) / (vn_trafo_lv / vn_lv_kv)^2 * parallel
      _wye_delta (T -> pi)          za = (r + jx) / 2; zc = -1j / y; zs = za^2 + 2 za zc; (r + jx) = zs / zc; y = -2j / (zs / za)
    The ppc branch then has BR_B = y (= b - 1j*g), TAP = ratio, SHIFT = shift_degree when voltage angles are calculated
    (runpp calculate_voltage_angles="auto": only if a line touches a bus above 70 kV), else 0.
    Also returned: the ratings of res_trafo.loading_percent (NetSpec.br_vn_hv_kv, br_vn_lv_kv, br_rating_mva).
    Out-of-service transformers are dropped.  Phase-shifting / cross regulators (tap_step_degree != 0, tap_phase_shifter)
    and tap-dependent impedance are refused."""
    t = trafo.sort_index()
    on = t["in_service"].to_numpy(bool) if "in_service" in t else np.ones(len(t), bool)
    t = t[on]
    n = len(t)
    if n == 0:
        z = np.zeros(0)
        return dict(br_from_bus=np.zeros(0, np.int32), br_to_bus=np.zeros(0, np.int32), br_r_pu=z, br_x_pu=z, br_b_pu=z,
                    br_g_pu=z, br_ratio=z, br_shift_deg=z, br_vn_hv_kv=z, br_vn_lv_kv=z, br_rating_mva=z)
    if "tap_phase_shifter" in t and t["tap_phase_shifter"].fillna(False).to_numpy(bool).any():
        raise NotImplementedError("transformers with tap_phase_shifter=True are not converted")
    if np.any(_col(t, "tap_step_degree", 0.0) != 0.0):
        raise NotImplementedError("transformers with tap_step_degree != 0 (cross / phase regulators) are not converted")
    if "tap_dependent_impedance" in t and t["tap_dependent_impedance"].fillna(False).to_numpy(bool).any():
        raise NotImplementedError("tap-dependent transformer impedance is not converted")
    hv = t["hv_bus"].to_numpy(np.int64); lv = t["lv_bus"].to_numpy(np.int64)
    vn_hv_bus, vn_lv_bus = bus_vn_kv[hv], bus_vn_kv[lv]
    vnh, vnl = t["vn_hv_kv"].to_numpy(np.float64).copy(), t["vn_lv_kv"].to_numpy(np.float64).copy()
    vn_lv_kv = vnl.copy()                                        # nameplate, before the tap changer
    tap_diff = _col(t, "tap_pos", 0.0) - _col(t, "tap_neutral", 0.0)
    tap_step = _col(t, "tap_step_percent", 0.0) / 100.0
    side = t["tap_side"].to_numpy() if "tap_side" in t else np.full(n, None)
    vnh = np.where(side == "hv", vnh * (1.0 + tap_diff * tap_step), vnh)
    vnl = np.where(side == "lv", vnl * (1.0 + tap_diff * tap_step), vnl)
    ratio = (vnh / vn_hv_bus) / (vnl / vn_lv_bus)
    shift = _col(t, "shift_degree", 0.0) if calculate_voltage_angles else np.zeros(n)
    parallel = _col(t, "parallel", 1.0)
    sn_t = t["sn_mva"].to_numpy(np.float64)
    tap_lv = np.square(vnl / vn_lv_bus) * net_sn_mva
    z_sc = t["vk_percent"].to_numpy(np.float64) / 100.0 / sn_t * tap_lv
    r_sc = t["vkr_percent"].to_numpy(np.float64) / 100.0 / sn_t * tap_lv
    x_sc = np.sign(z_sc) * np.sqrt(np.maximum(z_sc ** 2 - r_sc ** 2, 0.0))
    r, x = r_sc / parallel, x_sc / parallel
    base_r = np.square(vn_lv_bus) / net_sn_mva
    pfe = t["pfe_kw"].to_numpy(np.float64) * 1e-3
    i0 = t["i0_percent"].to_numpy(np.float64)
    b_real = pfe / np.square(vn_lv_kv) * base_r
    b_img = np.sqrt(np.maximum((i0 / 100.0 * sn_t) ** 2 - pfe ** 2, 0.0)) * base_r / np.square(vn_lv_kv)
    y = (-1j * b_real - b_img * np.sign(i0)) / np.square(vnl / vn_lv_kv) * parallel
    nz = y != 0                                                  # _wye_delta: T -> pi for transformers with a magnetising branch
    za = (r[nz] + 1j * x[nz]) / 2.0
    zc = -1j / y[nz]
    zs = za * za + 2.0 * za * zc
    zab = zs / zc
    r, x, y = r.copy(), x.copy(), y.copy()
    r[nz], x[nz], y[nz] = zab.real, zab.imag, -2j / (zs / za)
    # res_trafo.loading_percent (results_branch._get_trafo_results, trafo_loading="current") reads the nameplate voltages and
    # sn_mva x parallel x df [PP-recalled]
    return dict(br_from_bus=hv.astype(np.int32), br_to_bus=lv.astype(np.int32), br_r_pu=r, br_x_pu=x, br_b_pu=y.real,
                br_g_pu=-y.imag, br_ratio=ratio, br_shift_deg=shift, br_vn_hv_kv=t["vn_hv_kv"].to_numpy(np.float64).copy(),
                br_vn_lv_kv=vn_lv_kv, br_rating_mva=_rating(sn_t * parallel * _col(t, "df", 1.0)))


def from_pandapower(net, hv_init: str = "refuse", zip_loads: str = "refuse", gens: str = "refuse") -> NetSpec:
    """pandapowerNet (`pp.from_pickle(model.p)`, voltage_control_env.py:400-405) -> NetSpec: what pd2ppc would build for
    runpp's defaults.  Converted: buses (0..n-1, all in service), lines (an open line / trafo switch takes the branch out
    when that is exact — no shunt terms, or open at both ends — and is refused otherwise), two-winding transformers (trafo_to_pi), loads / sgens with `scaling` and `in_service`,
    non-consecutive bus indices (mapped to the positions of the sorted index, pd2ppc's bus lookup),
    shunts (step, in_service), one ext_grid, closed bus-bus switches (bus fusion -> NetSpec.bus_alias).  Refused loudly, never guessed: voltage-dependent loads
    (const_z_percent / const_i_percent != 0) unless zip_loads="runpp", generators (net.gen) unless gens="runpp", three-winding transformers, impedances, wards, dc lines, storage,
    closed bus-bus switches with z_ohm > 0 (pandapower models them as impedance branches, not as fused buses), fused buses of different vn_kv, and
    — by default (hv_init="refuse") — nets with a line at a bus above 70 kV: runpp's defaults then turn calculate_voltage_angles on AND start
    the Newton iteration from a DC power flow's angles (init="auto" -> "dc").
    hv_init="auto" does what runpp's defaults do: the DC-angle start (NetSpec.va_init = "dc", run by the solvers as mapdn_env_config.nr_init
    = 2) exactly when a line touches a bus above 70 kV, the flat start otherwise.  hv_init="flat" converts such a net with the flat start
    anyway: the converged answer is the same where both converge, the iteration count (and with it the 10-iteration verdict of
    voltage_control_env.py:188-196) need not be, and with a vector-group shift such as 150 degrees the flat start does not converge.
    zip_loads="runpp" converts voltage-dependent loads as runpp's voltage_depend_loads=True solves them (NetSpec.load_const_z /
    load_const_i = percent / 100).  Still refused with it: loads of different fractions on one bus (runpp solves
    with their row-count mean but reports each load with its own), a voltage-dependent load on the ext_grid bus, and voltage-dependent
    loads on a net with fused buses.
    gens="runpp" converts the in-service rows of net.gen as runpp's defaults solve them (NetSpec.gen_bus / gen_p_mw / gen_vm_pu /
    gen_scaling): the gen's bus holds |V| = vm_pu and injects p_mw * scaling, its Q is free (enforce_q_lims=False:
    min_q_mvar / max_q_mvar are not read), and every bus without a set-point starts the Newton iteration at the mean of the vm_pu of the
    ext_grid and of ALL net.gen rows, in service or not (NetSpec.vm_init_pu; init_vm_pu="auto").  Gens are not agents.  Still refused with
    it, by name: two in-service gens on one bus, a gen on the ext_grid's bus or with slack=True, gens on a net with fused buses, gens
    together with voltage-dependent loads."""
    if gens not in ("refuse", "runpp"):
        raise ValueError("gens must be 'refuse' or 'runpp'")
    if hv_init not in ("refuse", "flat", "auto"):
        raise ValueError("hv_init must be 'refuse', 'flat' or 'auto'")
    if zip_loads not in ("refuse", "runpp"):
        raise ValueError("zip_loads must be 'refuse' or 'runpp'")
    def table(name):
        t = net[name] if name in net else None
        return t if t is not None and len(t) else None
    for name in (("gen",) if gens == "refuse" else ()) + ("trafo3w", "impedance", "ward", "xward", "dcline", "storage", "motor", "asymmetric_load", "asymmetric_sgen"):
        t = table(name)
        if t is not None and (("in_service" not in t) or t["in_service"].to_numpy(bool).any()):
            raise NotImplementedError(f"net.{name} has in-service rows: not part of the MAPDN hot path, not converted")
    if len(net.ext_grid) != 1 or not bool(net.ext_grid["in_service"].iloc[0] if "in_service" in net.ext_grid else True):
        raise NotImplementedError("exactly one in-service ext_grid expected")
    bus = net.bus.sort_index()
    bus_index = bus.index.to_numpy()
    # pandapower bus indices -> consecutive positions of the sorted index (pd2ppc's bus lookup; the env reads every
    # result table through `.sort_index()`, voltage_control_env.py:219,370,536,584, so sorted order is its bus order too)
    if np.array_equal(bus_index, np.arange(len(bus_index))):
        rb = lambda a: np.asarray(a, dtype=np.int64)
    else:
        lut = {int(b): i for i, b in enumerate(bus_index)}
        rb = lambda a: np.array([lut[int(x)] for x in np.asarray(a)], dtype=np.int64)
    if "in_service" in bus and not bus["in_service"].to_numpy(bool).all():
        raise NotImplementedError("out-of-service buses are not converted")
    vn = bus["vn_kv"].to_numpy(np.float64)

    def zid(z):
        return 0 if z == "main" else int(str(z).replace("zone", ""))
    line = net.line.sort_index()
    line_on = line["in_service"].to_numpy(bool).copy()
    trafo = table("trafo")
    trafo_on = None if trafo is None else trafo.sort_index()["in_service"].to_numpy(bool).copy()
    sw = table("switch")
    fused_alias = None
    if sw is not None:
        closed = sw["closed"].to_numpy(bool)
        et = sw["et"].to_numpy()
        # closed bus-bus switches: bus fusion (pd2ppc's bus lookup merges the buses into one ppc bus) -> NetSpec.bus_alias;
        # the representative of a group is the ext_grid's bus if the group holds it, else the smallest bus (any choice gives
        # the same result tables)
        bb = (et == "b") & closed
        if np.any(bb) and "z_ohm" in sw and np.any(np.nan_to_num(_col(sw, "z_ohm", 0.0)[bb]) > 0.0):
            raise NotImplementedError("a closed bus-bus switch has z_ohm > 0: pandapower 2.x models it as an impedance branch between the two "
                                      "buses, not as one fused bus; not converted")
        if np.any(bb):
            parent_ = np.arange(len(bus_index))

            def find(x):
                while parent_[x] != x:
                    parent_[x] = parent_[parent_[x]]
                    x = parent_[x]
                return x
            for a_, b_ in zip(rb(sw["bus"].to_numpy()[bb]), rb(sw["element"].to_numpy()[bb])):
                ra, rb_ = find(int(a_)), find(int(b_))
                if ra != rb_:
                    parent_[max(ra, rb_)] = min(ra, rb_)
            fused_alias = np.array([find(i) for i in range(len(bus_index))])
            eg = int(rb([net.ext_grid["bus"].iloc[0]])[0])
            grp = fused_alias == fused_alias[eg]
            fused_alias[grp] = eg
            vn_rep = vn[fused_alias]
            if np.any(vn_rep != vn):
                bad = int(np.nonzero(vn_rep != vn)[0][0])
                raise NotImplementedError(f"bus {int(bus_index[bad])} (vn_kv {vn[bad]}) is fused by a closed bus-bus switch with bus "
                                          f"{int(bus_index[fused_alias[bad]])} (vn_kv {vn_rep[bad]}): the per-unit base of the merged node would be "
                                          "ambiguous; not converted")
        # An OPEN line / trafo switch: runpp's default (neglect_open_switch_branches=False, build_branch._switch_branches)
        # re-terminates the open end on an auxiliary bus, so the branch stays energised from its closed end and still draws
        # its charging / magnetising current.  That is the same as taking the branch out ONLY if it has no shunt terms, or
        # if it is open at both ends; anything else is refused rather than approximated.
        sw_bus = sw["bus"].to_numpy()
        el_all = sw["element"].to_numpy()
        pos = {idx: i for i, idx in enumerate(line.index)}
        line_c = line["c_nf_per_km"].to_numpy(np.float64); line_g = _col(line, "g_us_per_km", 0.0)
        for el in np.unique(el_all[(et == "l") & ~closed]):
            i = pos[int(el)]
            ends = set(sw_bus[(et == "l") & ~closed & (el_all == el)].tolist())
            if len(ends) < 2 and line_on[i] and (line_c[i] != 0.0 or line_g[i] != 0.0):
                raise NotImplementedError(f"line {int(el)} has an open switch at one end and non-zero c_nf_per_km / g_us_per_km: pandapower keeps "
                                          "it energised from the closed end (auxiliary bus); not converted")
            line_on[i] = False
        if trafo is not None:
            ts = trafo.sort_index()
            tpos = {idx: i for i, idx in enumerate(ts.index)}
            t_i0 = _col(ts, "i0_percent", 0.0); t_pfe = _col(ts, "pfe_kw", 0.0)
            for el in np.unique(el_all[(et == "t") & ~closed]):
                i = tpos[int(el)]
                ends = set(sw_bus[(et == "t") & ~closed & (el_all == el)].tolist())
                if len(ends) < 2 and trafo_on[i] and (t_i0[i] != 0.0 or t_pfe[i] != 0.0):
                    raise NotImplementedError(f"trafo {int(el)} has an open switch at one end and a magnetising branch (i0_percent / pfe_kw): "
                                              "pandapower keeps it energised from the closed end; not converted")
                trafo_on[i] = False
    load, sgen = net.load, net.sgen
    zip_cols = {}
    for col in ("const_z_percent", "const_i_percent"):
        if col in load and np.any(_col(load, col, 0.0) != 0.0):
            if zip_loads != "runpp":
                raise NotImplementedError(f"net.load.{col} != 0: voltage-dependent loads (runpp voltage_depend_loads=True) are not converted "
                                          "by default; pass zip_loads='runpp' (or MAPDN_ZIP_LOADS=runpp) to solve them as runpp does")
            zip_cols[col] = _col(load, col, 0.0) / 100.0
    on = lambda t: (t["in_service"].to_numpy(bool) if "in_service" in t else np.ones(len(t), bool)).astype(np.float64)
    kw = dict(
        name=str(net["name"] if "name" in net and net["name"] else "net"), bus_vn_kv=vn,
        bus_zone=np.array([zid(z) for z in bus["zone"].to_numpy()]),
        line_from_bus=rb(line["from_bus"].to_numpy()), line_to_bus=rb(line["to_bus"].to_numpy()),
        line_r_ohm_per_km=line["r_ohm_per_km"].to_numpy(), line_x_ohm_per_km=line["x_ohm_per_km"].to_numpy(),
        line_c_nf_per_km=line["c_nf_per_km"].to_numpy(), line_g_us_per_km=_col(line, "g_us_per_km", 0.0),
        line_length_km=line["length_km"].to_numpy(), line_parallel=line["parallel"].to_numpy(),
        line_in_service=line_on.astype(np.uint8),
        load_bus=rb(load["bus"].to_numpy()), sgen_bus=rb(sgen["bus"].to_numpy()),
        sgen_zone=np.array([zid(z) for z in sgen["name"].to_numpy()]),
        load_scaling=_col(load, "scaling", 1.0) * on(load), sgen_scaling=_col(sgen, "scaling", 1.0) * on(sgen),
        ext_grid_bus=int(rb([net.ext_grid["bus"].iloc[0]])[0]), ext_grid_vm_pu=float(net.ext_grid["vm_pu"].iloc[0]),
        sn_mva=float(net.sn_mva), f_hz=float(net.f_hz))
    if "max_i_ka" in line:                                       # res_line.loading_percent; a missing max_i_ka stays NaN (unrated)
        kw.update(line_max_i_ka=_rating(line["max_i_ka"].to_numpy(dtype=np.float64, na_value=np.nan)), line_df=_col(line, "df", 1.0))
    if fused_alias is not None:
        kw["bus_alias"] = fused_alias
    if zip_cols:
        cz = zip_cols.get("const_z_percent", np.zeros(len(load)))
        ci = zip_cols.get("const_i_percent", np.zeros(len(load)))
        lb = kw["load_bus"]
        zip_bus = (cz != 0.0) | (ci != 0.0)
        if fused_alias is not None:
            raise NotImplementedError("voltage-dependent loads on a net with fused buses (closed bus-bus switches) are not converted")
        if np.any(zip_bus & (lb == kw["ext_grid_bus"])):
            raise NotImplementedError("a voltage-dependent load on the ext_grid bus is not converted (runpp reports the slack bus from the "
                                      "network injection; its own load's polynomial is not modelled)")
        for b in np.unique(lb):
            at = lb == b
            if np.ptp(cz[at]) != 0.0 or np.ptp(ci[at]) != 0.0:
                raise NotImplementedError(f"the loads at bus {int(load['bus'].to_numpy()[at][0])} carry different const_z_percent / "
                                          "const_i_percent: runpp solves with their row-count mean and reports each load with its own "
                                          "polynomial, which is not converted")
        kw.update(load_const_z=cz, load_const_i=ci)
    gen = table("gen")
    if gen is not None and gens == "runpp":
        gen = gen.sort_index()
        g_on = gen["in_service"].to_numpy(bool) if "in_service" in gen else np.ones(len(gen), bool)
        g_bus = rb(gen["bus"].to_numpy())
        g_vm = gen["vm_pu"].to_numpy(np.float64)
        # init_vm_pu="auto" (_init_runpp_options): the mean over the ext_grid and EVERY gen row, in service or not
        kw["vm_init_pu"] = float(np.mean(np.r_[kw["ext_grid_vm_pu"], g_vm]))
        if not g_on.any() and kw["vm_init_pu"] != kw["ext_grid_vm_pu"]:
            # no gen bus, but the out-of-service rows still move the start of every bus: the solvers' start-only form
            if fused_alias is not None:
                raise NotImplementedError("out-of-service net.gen rows (they move the start of runpp's Newton iteration: init_vm_pu='auto') on a "
                                          "net with fused buses (closed bus-bus switches) are not converted")
            if zip_cols:
                raise NotImplementedError("out-of-service net.gen rows (they move the start of runpp's Newton iteration: init_vm_pu='auto') "
                                          "together with voltage-dependent loads are not converted")
        if g_on.any():
            if "slack" in gen and gen["slack"].fillna(False).to_numpy(bool)[g_on].any():
                raise NotImplementedError("an in-service net.gen row has slack=True (a second reference bus): not converted")
            if np.any(g_bus[g_on] == kw["ext_grid_bus"]):
                raise NotImplementedError("an in-service gen sits on the ext_grid bus (the slack bus already holds that voltage): not converted")
            if np.unique(g_bus[g_on]).shape[0] != int(g_on.sum()):
                raise NotImplementedError("two in-service gens on one bus (runpp merges them into one voltage-controlled bus and splits Q "
                                          "between them): not converted")
            if fused_alias is not None:
                raise NotImplementedError("gens on a net with fused buses (closed bus-bus switches) are not converted")
            if zip_cols:
                raise NotImplementedError("gens together with voltage-dependent loads (const_z_percent / const_i_percent) are not converted")
            kw.update(gen_bus=g_bus[g_on], gen_p_mw=gen["p_mw"].to_numpy(np.float64)[g_on], gen_vm_pu=g_vm[g_on],
                      gen_scaling=_col(gen, "scaling", 1.0)[g_on])
    # runpp calculate_voltage_angles="auto": True only if a line touches a bus above 70 kV — and then init="auto" means init_va_degree="dc"
    hv_buses = set(np.nonzero(vn > 70.0)[0].tolist())
    touched = set(rb(line["from_bus"].to_numpy()).tolist()) | set(rb(line["to_bus"].to_numpy()).tolist())
    calc_va = bool(hv_buses & touched)
    if calc_va and hv_init == "refuse":
        raise NotImplementedError("a line touches a bus above 70 kV: pp.runpp's defaults (voltage_control_env.py:557) switch calculate_voltage_angles on "
                                  "and initialise the voltage angles from a DC power flow (init='auto' -> 'dc'); the solvers here start flat, so the "
                                  "Newton iteration count — and the 10-iteration non-convergence verdict — could differ from pandapower's.  Pass "
                                  "hv_init='auto' to start from the DC power flow as runpp does (NetSpec.va_init = 'dc'), or hv_init='flat' to convert "
                                  "with the flat start anyway (transformer phase shifts applied; same converged voltages where the flat start "
                                  "converges — with a vector-group shift such as 150 degrees it does not, see tests/test_data_ingestion.py)")
    kw["va_init"] = "dc" if (calc_va and hv_init == "auto") else "flat"
    if trafo is not None:
        t = trafo.sort_index().copy()
        t["in_service"] = trafo_on
        t["hv_bus"] = rb(t["hv_bus"].to_numpy()); t["lv_bus"] = rb(t["lv_bus"].to_numpy())
        kw.update(trafo_to_pi(t, vn, float(net.sn_mva), calculate_voltage_angles=calc_va))
    sh = table("shunt")
    if sh is not None:
        # build_bus._calc_shunts_and_add_on_ppc: p, q per step, referred from the shunt's vn_kv to the bus voltage
        vn_bus = vn[rb(sh["bus"].to_numpy())]
        vn_sh = _col(sh, "vn_kv", np.nan)
        vn_sh = np.where(np.isnan(vn_sh), vn_bus, vn_sh)
        f = on(sh) * _col(sh, "step", 1.0) * np.square(vn_bus / vn_sh)
        kw.update(shunt_bus=rb(sh["bus"].to_numpy()), shunt_p_mw=sh["p_mw"].to_numpy(np.float64) * f,
                  shunt_q_mvar=sh["q_mvar"].to_numpy(np.float64) * f)
    return NetSpec(**kw)


# ------------------------------------------------------------------------------------------------
# model.p WITHOUT pandapower: a restricted unpickler.
#
# `pp.from_pickle(model.p)` (voltage_control_env.py:400-405) reads what pandapower 2.x `to_pickle` wrote: a plain dict
# net-key -> value, where every table is {"DF": DataFrame.to_dict("split"), "dtypes": {column: numpy dtype}} (io_utils.
# to_dict_with_coord_transform) and the rest are scalars / dicts (name, f_hz, sn_mva, version, std_types, _options ...).
# Nets pickled as objects (pickle.dump(net)) carry `pandapower.auxiliary.pandapowerNet` (a dict subclass) holding real
# pandas DataFrames.  Both forms are data: no pandapower CODE is needed to read them.  The unpickler below resolves only
#   * numpy's array / dtype / scalar reconstructors and an EXPLICIT (module, name) list of pandas' data classes and pickle
#     reconstructors (_PANDAS_OK; a module-prefix rule would also expose the helper functions pandas modules re-export —
#     round 3's rule did, and a gadget chain through them reached os.system),
#   * plain builtin containers,
#   * `pandapower.*` names, which are mapped to INERT stand-ins (a dict subclass for the net, an attribute bag for
#     anything else, e.g. controller objects inside net.controller) — their code is never imported or run,
# and refuses every other global (os, subprocess, builtins.eval, functions inside pandas ...): a pickle is a program, model.p is
# downloaded data.  (Defence in depth, not a proof: prefer netspec.npz for files of unknown origin.)
# ------------------------------------------------------------------------------------------------
class InertNet(dict):
    """attribute-style dict standing in for pandapower.auxiliary.pandapowerNet / ADict (tables are pandas DataFrames)"""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError as e:
            raise AttributeError(name) from e

    def __setstate__(self, state):               # ADict pickles as a dict subclass: items arrive through SETITEMS; any
        if isinstance(state, dict):              # extra instance state is merged as items as well
            self.update(state)
        elif isinstance(state, tuple) and len(state) == 2:
            for part in state:
                if isinstance(part, dict):
                    self.update(part)


class _InertObject:
    """stand-in for any other pandapower class found in a pickle (controllers, std-type helpers): keeps the state, runs nothing"""

    def __init__(self, *a, **k):
        pass

    def __setstate__(self, state):
        self.__dict__["_state"] = state


_NUMPY_OK = {("numpy", "dtype"), ("numpy", "ndarray"), ("numpy", "float64"), ("numpy", "int64"), ("numpy", "bool_"),
             ("numpy.core.multiarray", "_reconstruct"), ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "_reconstruct"),
             ("numpy._core.multiarray", "scalar"), ("numpy.core.numeric", "_frombuffer"), ("numpy._core.numeric", "_frombuffer")}
_BUILTINS_OK = {"dict", "list", "tuple", "set", "frozenset", "slice", "range", "complex", "bytearray", "object", "bytes", "str",
                "int", "float", "bool"}
_MISC_OK = {("collections", "OrderedDict"), ("collections", "defaultdict"), ("copyreg", "_reconstructor"), ("copy_reg", "_reconstructor"),
            ("datetime", "datetime"), ("datetime", "date"), ("datetime", "timedelta"), ("datetime", "timezone"),
            ("_codecs", "encode"), ("__builtin__", "object"), ("__builtin__", "dict"), ("__builtin__", "list"), ("__builtin__", "set"),
            ("__builtin__", "tuple"), ("__builtin__", "slice"), ("__builtin__", "long"), ("__builtin__", "unicode"),
            ("__builtin__", "bytes")}          # Python 3 writes b"" as bytes() under protocol <= 2 (the raw data of an EMPTY table's arrays)
# pandas: an explicit (module, name) list of the DATA classes and the reconstructor functions a pickled DataFrame / Series /
# Index references (enumerated with pickletools over frames of every column kind, protocols 2-5, plus the legacy paths of
# pandas.compat.pickle_compat).  NOT a module-prefix rule: pandas modules re-export functions (import helpers, file
# handles, functools.partial ...) that a hand-assembled pickle could call through REDUCE.
_PANDAS_OK = {
    ("pandas.core.frame", "DataFrame"), ("pandas.core.series", "Series"),
    ("pandas.core.internals.managers", "BlockManager"), ("pandas.core.internals.managers", "SingleBlockManager"),
    ("pandas._libs.internals", "_unpickle_block"), ("pandas._libs.arrays", "__pyx_unpickle_NDArrayBacked"),
    ("pandas.core.indexes.base", "Index"), ("pandas.core.indexes.base", "_new_Index"),
    ("pandas.core.indexes.range", "RangeIndex"), ("pandas.core.indexes.multi", "MultiIndex"),
    ("pandas.core.indexes.frozen", "FrozenList"),
    ("pandas.core.indexes.datetimes", "DatetimeIndex"), ("pandas.core.indexes.datetimes", "_new_DatetimeIndex"),
    ("pandas.core.indexes.category", "CategoricalIndex"),
    ("pandas.core.arrays.categorical", "Categorical"), ("pandas.core.arrays", "Categorical"),
    ("pandas.core.dtypes.dtypes", "CategoricalDtype"), ("pandas.core.dtypes.dtypes", "DatetimeTZDtype"),
    ("pandas.core.arrays.datetimes", "DatetimeArray"),
    ("pandas.core.arrays.boolean", "BooleanArray"), ("pandas.core.arrays.boolean", "BooleanDtype"),
    ("pandas.core.arrays.integer", "IntegerArray"), ("pandas.core.arrays.integer", "Int64Dtype"),
    ("pandas.core.arrays.integer", "Int32Dtype"), ("pandas.core.arrays.integer", "UInt32Dtype"),
    ("pandas.core.arrays.integer", "UInt64Dtype"),
    ("pandas.core.arrays.floating", "FloatingArray"), ("pandas.core.arrays.floating", "Float64Dtype"),
    ("pandas.core.arrays.floating", "Float32Dtype"),
    ("pandas.core.arrays.string_", "StringArray"), ("pandas.core.arrays.string_", "StringDtype"),
    ("pandas._libs.missing", "NA"), ("pandas._libs.tslibs.nattype", "__nat_unpickle"),
    ("pandas._libs.tslibs.timestamps", "_unpickle_timestamp"), ("pandas._libs.tslibs.timestamps", "Timestamp"),
}
# module paths of older pandas versions (pandapower 2.7.0 pins pandas 1.1.3) that pickle_compat maps onto the entries above
_PANDAS_LEGACY = {
    ("pandas.core.indexes.numeric", "Int64Index"), ("pandas.core.indexes.numeric", "UInt64Index"),
    ("pandas.core.indexes.numeric", "Float64Index"), ("pandas.core.internals.blocks", "new_block"),
    ("pandas.indexes.base", "Index"), ("pandas.indexes.base", "_new_Index"), ("pandas.indexes.multi", "MultiIndex"),
    ("pandas.indexes.numeric", "Float64Index"), ("pandas.indexes.numeric", "Int64Index"), ("pandas.indexes.range", "RangeIndex"),
    ("pandas.core.base", "FrozenList"), ("pandas.core.categorical", "Categorical"), ("pandas.core.series", "TimeSeries"),
    ("pandas.tseries.index", "DatetimeIndex"), ("pandas.tseries.index", "_new_DatetimeIndex"),
    ("pandas._libs.tslib", "__nat_unpickle"), ("pandas.tslib", "__nat_unpickle"), ("pandas._libs.tslib", "Timestamp"),
    ("pandas.tslib", "Timestamp"),
}
_PANDAS_FUNCS = {"_unpickle_block", "__pyx_unpickle_NDArrayBacked", "_new_Index", "_new_DatetimeIndex", "__nat_unpickle",
                 "_unpickle_timestamp"}


def _restricted_unpickler(f):
    import importlib
    import pickle

    def refuse(module, name):
        raise pickle.UnpicklingError(f"model.p references {module}.{name}: not a numpy / pandas / builtin data class — refused "
                                     "(mapdn_amd.data reads pandapower pickles as data, it never imports or runs their code)")

    class U(pickle.Unpickler):
        def find_class(self, module, name):
            if module == "pandapower" or module.startswith("pandapower."):
                return InertNet if name in ("pandapowerNet", "ADict") else _InertObject
            if (module, name) in _NUMPY_OK or (module, name) in _MISC_OK or (module == "builtins" and name in _BUILTINS_OK):
                if module == "__builtin__":
                    module = "builtins"
                    name = {"long": "int", "unicode": "str"}.get(name, name)
                if module == "copy_reg":
                    module = "copyreg"
                return getattr(importlib.import_module(module), name)
            if (module, name) in _PANDAS_LEGACY:
                import pandas.compat.pickle_compat as pc          # old pandas module paths -> current classes
                module, name = getattr(pc, "_class_locations_map", {}).get((module, name), (module, name))
                if (module, name) == ("pandas._libs.tslib", "Timestamp"):
                    module = "pandas._libs.tslibs.timestamps"
            if (module, name) not in _PANDAS_OK:
                refuse(module, name)
            obj = getattr(importlib.import_module(module), name)
            # belt and braces: what the name resolves to must itself live in pandas and be a class, the NA singleton or one of
            # the named reconstructors — never a function another module re-exports under an allowed name
            home = getattr(obj, "__module__", None) or getattr(type(obj), "__module__", "")
            ok = home.startswith("pandas.") and (isinstance(obj, type) or name in _PANDAS_FUNCS or name == "NA")
            if not ok:
                refuse(module, name)
            return obj
    return U(f, encoding="latin1")


def read_pandapower_pickle(path: str) -> InertNet:
    """`pp.from_pickle(path)` (voltage_control_env.py:400-405) without pandapower: the net as an attribute-style dict of
    pandas DataFrames + scalars, from either on-disk form (see above).  Only what io_utils.get_raw_data_from_pickle does to
    the tables is done here (DataFrame from the "split" dict, column dtypes restored); pandapower's convert_format
    (renaming the columns of nets saved by versions < 2.0, kW/kVA units) is NOT replayed — such a net is refused."""
    import pandas as pd
    with open(path, "rb") as f:
        raw = _restricted_unpickler(f).load()
    if not isinstance(raw, dict):
        raise ValueError(f"{path}: not a pandapower net pickle (top level is {type(raw).__name__})")
    net = InertNet()
    for key, item in raw.items():
        if isinstance(item, dict) and "DF" in item:
            d = item["DF"]
            df = pd.DataFrame(data=d.get("data"), index=d.get("index"), columns=d.get("columns")) if isinstance(d, dict) else pd.DataFrame(d)
            for col, dt in (item.get("dtypes") or {}).items():
                if col in df.columns:
                    try:
                        df[col] = df[col].astype(dt)
                    except (TypeError, ValueError):
                        pass                       # object columns with None (names, std_type): left as they are, like pandapower
            net[key] = df
        else:
            net[key] = item
    if "sn_mva" not in net or "bus" not in net or ("sn_kva" in net and "sn_mva" not in net):
        raise NotImplementedError(f"{path}: no sn_mva / bus table — a net saved by pandapower < 2.0 (kW / kVA columns) needs "
                                  "pandapower's convert_format; re-save it with pandapower >= 2.0")
    return net


def load_scenario(data_path: str, pv_scale: float = 1.0, demand_scale: float = 1.0, hv_init: str = None, zip_loads: str = None,
                  gens: str = None):
    """(NetSpec, Profiles) of a scenario directory: netspec.npz or the reference's model.p (read as data by the restricted
    unpickler above — pandapower is not needed) + the three CSVs.  hv_init ("refuse" | "flat" | "auto", see from_pandapower; default:
    the MAPDN_HV_INIT environment variable, else "refuse") decides what happens to a model.p with a line at a bus above 70 kV — runpp
    starts such a net from a DC power flow's angles, which "auto" records for the solvers (NetSpec.va_init = "dc").  zip_loads
    ("refuse" | "runpp", see from_pandapower; default: the MAPDN_ZIP_LOADS environment variable, else "refuse") decides what happens
    to a model.p with voltage-dependent loads (const_z_percent / const_i_percent), gens ("refuse" | "runpp"; default: the MAPDN_GENS
    environment variable, else "refuse") what happens to one with in-service net.gen rows."""
    npz = os.path.join(data_path, "netspec.npz")
    if hv_init is None:
        hv_init = os.environ.get("MAPDN_HV_INIT", "refuse")
    if zip_loads is None:
        zip_loads = os.environ.get("MAPDN_ZIP_LOADS", "refuse")
    if gens is None:
        gens = os.environ.get("MAPDN_GENS", "refuse")
    if os.path.exists(npz):
        net = load_netspec(npz)
    elif os.path.exists(os.path.join(data_path, "model.p")):
        # (zip_loads is passed only when it is not the default: a from_pandapower stand-in written before it existed keeps working)
        more = {} if zip_loads == "refuse" else dict(zip_loads=zip_loads)
        if gens != "refuse":
            more["gens"] = gens
        net = from_pandapower(read_pandapower_pickle(os.path.join(data_path, "model.p")), hv_init=hv_init, **more)
    else:
        raise FileNotFoundError(f"no netspec.npz / model.p in {data_path}")
    return net, load_profiles_csv(data_path, pv_scale, demand_scale)
