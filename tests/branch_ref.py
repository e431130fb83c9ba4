"""Nets, ratings and the references of the res_line / res_trafo tests (tests/test_branch_cpu.py, tests/test_branch_results_gpu.py): test
infrastructure only, independent of the product code.

The tables are functions of the bus voltages alone.  `tables(net, vm_pu, va_degree, dtype)` evaluates the definitions of DESIGN.md section 17
from the Yf, Yt of oracle.pp_restated.make_ybus at the SAME vm_pu / va_degree arrays the kernel is given:
    dtype = numpy.longdouble   `ref`: V, Sf = Vf conj(Yf V), St = Vt conj(Yt V), |S|, the currents and the loadings in x87 extended precision
    dtype = numpy.float64      `e64`: the same in plain float64 exactly as pp_restated.py:271-273 forms them (Sf, St, pl = Re Sf + Re St)
Error bars (the project's rule from the OPF kernel tests, tests/opf_kernel_cases.py): per case and column, e64 = the error of the float64
evaluation against ref relative to the column's largest magnitude in the case; the kernel's bar is 16 x e64, never below 64 ulp."""
import dataclasses
import functools

import numpy as np

from mapdn_amd.netspec import NetSpec, add_fused_buses, case33_meshed, make_case, synth_profiles
from oracle.pp_restated import make_ybus, runpp_restated

LD, CLD = np.longdouble, np.clongdouble
EPS = np.finfo(np.float64).eps
BAR_FACTOR, BAR_FLOOR = 16.0, 64.0 * EPS
DAYS = 3
COLUMNS = ("p_from_mw", "q_from_mvar", "p_to_mw", "q_to_mvar", "pl_mw", "ql_mvar", "i_from_ka", "i_to_ka", "i_ka", "loading_percent")
TRAFO_NAMES = dict(p_from_mw="p_hv_mw", q_from_mvar="q_hv_mvar", p_to_mw="p_lv_mw", q_to_mvar="q_lv_mvar", pl_mw="pl_mw", ql_mvar="ql_mvar",
                   i_from_ka="i_hv_ka", i_to_ka="i_lv_ka", loading_percent="loading_percent")
CASES = ("feeder3", "tree8", "case33_meshed", "case33_fused", "case141")
BATCHES = dict(feeder3=1, tree8=17, case33_meshed=3, case33_fused=33, case141=65)     # 1, 3, 17, 33, 65: the padding to 64 and a second env tile


# ---- nets ---------------------------------------------------------------------------------------------------------------------------------
def _net(name, vn, zone, lines, loads, sgens, **kw):
    """lines: (from, to, r, x, c_nf, length, parallel, in_service) rows"""
    L = np.array(lines, dtype=np.float64)
    return NetSpec(name=name, bus_vn_kv=np.asarray(vn, float), bus_zone=np.asarray(zone), line_from_bus=L[:, 0].astype(int), line_to_bus=L[:, 1].astype(int),
                   line_r_ohm_per_km=L[:, 2], line_x_ohm_per_km=L[:, 3], line_c_nf_per_km=L[:, 4], line_g_us_per_km=np.zeros(len(L)),
                   line_length_km=L[:, 5], line_parallel=L[:, 6].astype(int), line_in_service=L[:, 7].astype(np.uint8),
                   load_bus=np.asarray(loads), sgen_bus=np.asarray(sgens), sgen_zone=np.asarray(zone)[np.asarray(sgens)],
                   ext_grid_bus=0, ext_grid_vm_pu=1.0, sn_mva=10.0, f_hz=50.0, **kw)


def _prof(p_nom, pv_max, seed):
    p_nom = np.asarray(p_nom, float)
    return synth_profiles(p_nom, p_nom * np.tan(np.arccos(0.95)), np.asarray(pv_max, float), days=DAYS, seed=seed)


def _feeder3():
    """0 - 1 - 2, two overhead lines, rated; its flows follow in closed form from a chosen V (tests/test_branch_cpu.py)"""
    net = _net("feeder3", [12.47] * 3, [0, 1, 1], [(0, 1, 0.30, 0.25, 0.0, 1.2, 1, 1), (1, 2, 0.45, 0.30, 0.0, 0.8, 1, 1)], [1, 2], [2],
               line_max_i_ka=np.array([0.25, 0.12]), line_df=np.array([1.0, 0.9]))
    return net, _prof([0.9, 0.6], [1.0], 9301)


def _tree8():
    """bus 0 (33 kV, slack) - transformer (ratio 0.97, shift 2 degrees, iron losses) - bus 1; 1 - 2 (parallel = 2) - 3 (a cable:
    c_nf_per_km large enough that i_from != i_to); 1 - 4 (shunt) - 5; 4 - 6 (unrated) - 7 (a dead end without load: no current);
    an out-of-service tie 3 - 5"""
    lines = [(1, 2, 0.20, 0.16, 10.0, 0.9, 2, 1), (2, 3, 0.12, 0.08, 320.0, 3.5, 1, 1), (1, 4, 0.25, 0.20, 9.0, 1.1, 1, 1),
             (4, 5, 0.40, 0.30, 0.0, 0.7, 1, 1), (4, 6, 0.35, 0.28, 12.0, 0.6, 1, 1), (6, 7, 0.50, 0.35, 0.0, 0.5, 1, 1),
             (3, 5, 0.30, 0.30, 5.0, 1.0, 1, 0)]
    net = _net("tree8", [33.0] + [12.47] * 7, [0, 0, 1, 1, 2, 2, 2, 2], lines, [2, 3, 4, 5, 6], [3, 5],
               br_from_bus=np.array([0]), br_to_bus=np.array([1]), br_r_pu=np.array([0.004]), br_x_pu=np.array([0.05]), br_b_pu=np.array([-0.012]),
               br_g_pu=np.array([0.003]), br_ratio=np.array([0.97]), br_shift_deg=np.array([2.0]),
               shunt_bus=np.array([4]), shunt_p_mw=np.array([0.01]), shunt_q_mvar=np.array([-0.2]),
               br_vn_hv_kv=np.array([33.0]), br_vn_lv_kv=np.array([12.0]), br_rating_mva=np.array([4.0 * 1 * 0.95]))
    return net, _prof([0.5, 0.7, 0.4, 0.6, 0.3], [1.2, 0.9], 9308)


@functools.lru_cache(maxsize=None)
def _base(name):
    if name == "feeder3":
        return _feeder3()
    if name == "tree8":
        return _tree8()
    if name == "case141":
        return make_case("case141", days=DAYS)
    net, prof = make_case("case33", days=DAYS)
    if name == "case33_meshed":
        return case33_meshed(net, 5), prof                     # five tie lines closed: the general sparse solver
    if name == "case33_fused":                                 # two fused buses; line 6 now ends on the NEW bus of the first pair
        f = add_fused_buses(net, [3, 7], move_loads=[(int(np.flatnonzero(net.load_bus == 7)[0]), 1)] if (net.load_bus == 7).any() else ())
        li = int(np.flatnonzero(f.line_to_bus == 3)[0])
        to = f.line_to_bus.copy(); to[li] = net.n_bus
        return dataclasses.replace(f, line_to_bus=to), prof
    raise KeyError(name)


def rows_of(prof, B):
    """daytime profile rows 09:00 .. 15:00, another one per env"""
    return np.array([prof.start_row(e % (DAYS - 1), 9 + (e * 5) % 7, (e * 7) % prof.intervals_per_hour) for e in range(B)])


@functools.lru_cache(maxsize=None)
def make(name):
    """(NetSpec with ratings, Profiles).  feeder3 and tree8's transformer carry hand-set ratings.  The other lines are rated ON THE
    CPU from the oracle's power flow at the first test row: max_i_ka df = i_ka there / u, u seeded uniform in (0.3, 1.3) — loadings from
    30 % to 130 %, so that limit_percent = 100 splits the lines, and no two lines share a loading: worst_branch is decided well above
    the error bar (tests/test_branch_cpu.py::test_top_two_loadings_are_apart holds the share of undecided envs to 5 %).  tree8: line 4 stays
    unrated."""
    net, prof = _base(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "feeder3":
        return net, prof
    t = int(rows_of(prof, 1)[0])
    r = runpp_restated(net, prof.load_p[t], prof.load_q[t], prof.pv[t], np.zeros(net.n_sgen))
    unrated = dataclasses.replace(net, line_max_i_ka=np.zeros(0), line_df=np.zeros(0))
    i_ka = tables(unrated, r.vm_pu, r.va_degree, np.float64)[0]["i_ka"]
    max_i = np.where(i_ka > 1e-3 * i_ka.max(), i_ka, i_ka.max()) / rng.uniform(0.3, 1.3, net.n_line)   # (a line without current: the largest rating)
    df = rng.choice([1.0, 0.9, 0.8], net.n_line)
    if name == "tree8":
        max_i[4] = np.nan                                       # the unrated line
    return dataclasses.replace(net, line_max_i_ka=max_i / df, line_df=df), prof


# ---- the reference --------------------------------------------------------------------------------------------------------------------------
def tables(net, vm_pu, va_degree, dtype=LD):
    """(res_line, res_trafo) at vm_pu / va_degree [n_bus] by bus: dicts of the ten columns, [n_line] / [n_branch_pu], in `dtype`"""
    ext = dtype is LD
    R, Cx = (LD, CLD) if ext else (np.float64, np.complex128)
    yf, yt, f, t, on, y4 = _constants(net)
    vm, va = np.asarray(vm_pu, R), np.asarray(va_degree, R)
    if ext:
        ang = va * (LD(np.pi) / LD(180))                       # the float64 pi the product multiplies by: the same radians, to 2^-64
        v = vm * (np.cos(ang) + CLD(1j) * np.sin(ang))
        i_f, i_t = y4[0] * v[f] + y4[1] * v[t], y4[2] * v[f] + y4[3] * v[t]      # the two entries of each row of Yf / Yt
    else:
        v = vm * np.exp(1j * np.deg2rad(va))
        i_f, i_t = yf @ v, yt @ v
    sn = R(net.sn_mva)
    sf, st = v[f] * np.conj(i_f) * sn, v[t] * np.conj(i_t) * sn
    sq3 = np.sqrt(R(3))
    with np.errstate(invalid="ignore", divide="ignore"):
        cur = lambda s, b: np.where(np.abs(s) == 0, R(0), np.abs(s) / (sq3 * vm[b] * np.asarray(net.bus_vn_kv, R)[b]))
        i_from, i_to = cur(sf, f), cur(st, t)
    col = dict(p_from_mw=sf.real, q_from_mvar=sf.imag, p_to_mw=st.real, q_to_mvar=st.imag, pl_mw=sf.real + st.real, ql_mvar=sf.imag + st.imag,
               i_from_ka=i_from, i_to_ka=i_to, i_ka=np.maximum(i_from, i_to))
    nl_on, n_line, n_tr = int(on.sum()), net.n_line, net.n_branch_pu
    line = {k: np.zeros(n_line, R) for k in col}
    for k, x in col.items():
        line[k][on] = x[:nl_on]
    trafo = {k: x[nl_on:] for k, x in col.items()}
    rate = np.full(n_line, np.nan, R)
    if net.line_max_i_ka.shape[0]:
        df = np.asarray(net.line_df, R) if net.line_df.shape[0] else np.ones(n_line, R)
        rate = np.asarray(net.line_max_i_ka, R) * df * np.asarray(net.line_parallel, R)
    line["loading_percent"] = np.where(on, R(100) * line["i_ka"] / rate, R(0))
    if n_tr and net.br_rating_mva.shape[0] and net.br_vn_hv_kv.shape[0] and net.br_vn_lv_kv.shape[0]:
        s_max = np.maximum(trafo["i_from_ka"] * np.asarray(net.br_vn_hv_kv, R), trafo["i_to_ka"] * np.asarray(net.br_vn_lv_kv, R))
        trafo["loading_percent"] = R(100) * sq3 * s_max / np.asarray(net.br_rating_mva, R)
    else:
        trafo["loading_percent"] = np.full(n_tr, np.nan, R)
    return line, trafo


_CONST = {}


def _constants(net):
    """Yf, Yt of the oracle (in-service lines, then the pi branches), the two ends of their rows, and the four entries yff yft ytf ytt
    of every row in longdouble; cached per NetSpec object"""
    hit = _CONST.get(id(net))
    if hit is None or hit[0] is not net:
        _, yf, yt = make_ybus(net)
        on = net.line_in_service.astype(bool)
        f = np.concatenate([net.line_from_bus[on], net.br_from_bus]).astype(np.int64)
        t = np.concatenate([net.line_to_bus[on], net.br_to_bus]).astype(np.int64)
        i = np.arange(f.shape[0])
        y4 = tuple(np.asarray(m[i, b]).ravel().astype(CLD) for m, b in ((yf, f), (yf, t), (yt, f), (yt, t)))
        hit = _CONST[id(net)] = (net, (yf, yt, f, t, on, y4))
    return hit[1]


def rel_err(x, ref):
    """max |x - ref| relative to the largest magnitude of ref, formed in longdouble; NaN must meet NaN"""
    x, ref = np.asarray(x, LD), np.asarray(ref, LD)
    assert np.array_equal(np.isnan(x), np.isnan(ref)), "NaN pattern"
    fin = ~np.isnan(ref)
    if not fin.any():
        return 0.0
    scale = np.abs(ref[fin]).max()
    d = np.abs(x[fin] - ref[fin]).max()
    return float(d / scale) if scale > 0 else float(d)


def batch_tables(net, vm, va, dtype=LD):
    """tables() over a batch: vm, va [B, n_bus] -> (line, trafo) dicts of [B, n]"""
    per = [tables(net, vm[e], va[e], dtype) for e in range(vm.shape[0])]
    return tuple({k: np.stack([p[i][k] for p in per]) for k in COLUMNS} for i in range(2))


def errors(net, vm, va, got_line, got_trafo):
    """per table and column: the error of `got` ([B, n] arrays; a missing column is skipped) against ref at vm, va [B, n_bus]"""
    ref = batch_tables(net, vm, va, LD)
    return tuple({k: rel_err(g[k], r[k]) for k in COLUMNS if k in g} for g, r in zip((got_line, got_trafo), ref))


def e64(net, vm, va):
    """the error of the float64 evaluation against ref at the same voltages, per table and column"""
    l64, t64 = batch_tables(net, vm, va, np.float64)
    return errors(net, vm, va, l64, t64)


def bars(net, vm, va):
    """the kernel's bar per table and column at these voltages: 16 x e64, never below 64 ulp"""
    return tuple({k: max(BAR_FACTOR * e, BAR_FLOOR) for k, e in tab.items()} for tab in e64(net, vm, va))


def oracle_voltages(name, B, q_scale=0.5):
    """vm_pu, va_degree [B, n_bus] of the oracle's power flows at the case's test rows, with seeded reactive set-points: the states the
    CPU tests evaluate the bars at (the GPU tests evaluate them at the kernel's own input voltages)"""
    net, prof = make(name)
    rows = rows_of(prof, B)
    rng = np.random.default_rng(B + sum(map(ord, name)))
    smax = prof.s_max(1.2)
    vm, va = [], []
    for t in rows:
        q = q_scale * rng.uniform(-1, 1, net.n_sgen) * np.sqrt(np.maximum(smax ** 2 - prof.pv[t] ** 2, 0.0))
        r = runpp_restated(net, prof.load_p[t], prof.load_q[t], prof.pv[t], q)
        assert r.converged, (name, int(t))
        vm.append(r.vm_pu); va.append(r.va_degree)
    return np.stack(vm), np.stack(va)


def summary_ref(net, load_line, load_trafo, limit):
    """(max_loading, worst_branch, n_overloaded, gap) per env over the rated in-service branches, from loading_percent [B, n_line],
    [B, n_trafo] (NaN = unrated); gap = top loading minus the second, relative to the top (inf with fewer than two branches)"""
    L = np.concatenate([np.asarray(load_line, np.float64), np.asarray(load_trafo, np.float64)], axis=1)
    L[:, :net.n_line][:, ~net.line_in_service.astype(bool)] = np.nan
    B = L.shape[0]
    mx, wb, no, gap = np.full(B, np.nan), np.full(B, -1, np.int32), np.zeros(B, np.int32), np.full(B, np.inf)
    for e in range(B):
        ok = ~np.isnan(L[e])
        if not ok.any():
            continue
        x = np.where(ok, L[e], -np.inf)
        wb[e] = int(np.argmax(x)); mx[e] = x[wb[e]]; no[e] = int((x > limit).sum())
        s = np.sort(x[ok])
        if s.shape[0] > 1 and s[-1] > 0:
            gap[e] = (s[-1] - s[-2]) / s[-1]
    return mx, wb, no, gap
