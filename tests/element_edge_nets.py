"""Small nets at the edges of the element tables, and the layout the step-path kernels derive from them: test infrastructure of
tests/test_element_edges_cpu.py (every net holds its edges, a host-only handle takes it, the oracle alone runs the replayed
trajectories without an unsolvable step) and tests/test_element_edges_gpu.py (k_inject, k_inject_sgen, the injection prologue of
k_nr_tree, k_reset_begin, k_advance, k_commit_fused, k_gather, k_to_envminor and k_stats against the oracle env on these nets).

The shipped cases have one or two loads per bus, nothing on the ext_grid bus, a load on every PV bus, even sgen counts and scalings
of 1; the nets here are seeded 13- to 19-bus feeders of netspec._radial_case whose load_bus / sgen_bus are re-pointed by hand:
    crowded         nl = 9, ns = 5: three loads on a load-only bus, four loads and two sgens on one PV bus, a load and an sgen on the
                    ext_grid bus, a PV bus without a load, a PV bus with one load, scalings 0 / < 1 / > 1, 150 obs columns
    crowded_fused   crowded with the ext_grid bus, the crowded PV bus and the three-load bus each fused with a twin that takes over
                    some of their elements
    crowded_zip     crowded with ZIP fractions (0.3, 0.2) on every load off the ext_grid bus
    crowded_meshed  crowded plus one tie line (k_nr_sparse)
    one_sgen        nl = 10, ns = 1: nine load-only buses for the one PV bus, a load alone on the ext_grid bus, two loads on one bus,
                    38 obs columns
    all_pv          nl = 1, ns = 4: the only load on a PV bus, no load-only bus at all, 88 obs columns
layout(net) restates, by bus and from the NetSpec alone, the rule by which setup_pv_buses (csrc/capi.hip) sorts the nodes: a node is
a group of fused buses (bus_alias), named here by its representative bus."""
import ctypes as C
import dataclasses
import functools

import numpy as np

from mapdn_amd import _lib
from mapdn_amd.netspec import _radial_case, add_fused_buses, add_lines, synth_profiles
from tests.zip_nets import with_zip

DAYS = 4
ARGS = dict(episode_limit=4, action_scale=0.8, action_bias=0.0, voltage_barrier_type="bowl", seed=0)
ZIP_FRACTIONS = (0.3, 0.2)                                    # (cz, ci) of crowded_zip
NETS = ("crowded", "crowded_fused", "crowded_zip", "crowded_meshed", "one_sgen", "all_pv")


# ---- the layout ---------------------------------------------------------------------------------------------------------------
def layout(net):
    """what the step path makes of the element tables, by bus:
        pv              representative buses of the nodes with an sgen (k_inject_sgen's rows; the ext_grid node included)
        load_only       ... of the nodes with loads and no sgen (the ext_grid node included)
        multi_load_only ... of the load-only nodes off the ext_grid node with two or more loads (the `mlo` rows)
        loads_per_bus, sgens_per_bus    [n_bus] counts per ORIGINAL bus;   loads_per_node, sgens_per_node   the same per node, at the
                                        index of its representative (0 at the other members)
        ld_dest         [nl] kind of every load: 0 alone on a load-only node off the ext_grid (k_advance writes that Sbus entry),
                        1 alone on a PV node (its bus_ld row), 2 neither
        empty           original buses with no load, sgen or shunt of their own"""
    nb = net.n_bus
    alias = np.asarray(net.bus_alias, np.int64)
    ext = int(alias[net.ext_grid_bus])
    lpb = np.bincount(net.load_bus, minlength=nb)
    spb = np.bincount(net.sgen_bus, minlength=nb)
    lpn = np.bincount(alias[net.load_bus], minlength=nb)
    spn = np.bincount(alias[net.sgen_bus], minlength=nb)
    reps = np.flatnonzero(alias == np.arange(nb))
    pv = [int(b) for b in reps if spn[b] > 0]
    lo = [int(b) for b in reps if spn[b] == 0 and lpn[b] > 0]
    mlo = [b for b in lo if lpn[b] > 1 and b != ext]
    kind = np.full(net.n_load, 2, np.int64)
    for li, b in enumerate(alias[net.load_bus]):
        if lpn[b] == 1:
            kind[li] = 1 if spn[b] > 0 else (0 if b != ext else 2)
    shunted = np.bincount(net.shunt_bus, minlength=nb)
    return dict(pv=pv, load_only=lo, multi_load_only=mlo, loads_per_bus=lpb, sgens_per_bus=spb, loads_per_node=lpn, sgens_per_node=spn,
                ld_dest=kind, empty=[int(b) for b in range(nb) if lpb[b] == 0 and spb[b] == 0 and shunted[b] == 0])


def obs_columns(net):
    return net.n_sgen * net.obs_size()


def scaled_sum_nodes(net):
    """representative buses of the nodes with two or more loads of which at least two carry a scaling other than 0 and 1: there the sum
    sum p x scaling rounds differently with and without a fused multiply-add, which is how the injection paths were found to differ in
    their last bits"""
    alias = np.asarray(net.bus_alias, np.int64)
    odd = (net.load_scaling != 1.0) & (net.load_scaling != 0.0)
    n_odd = np.bincount(alias[net.load_bus], weights=odd.astype(np.float64), minlength=net.n_bus)
    return [int(b) for b in np.flatnonzero(n_odd >= 2)]


# ---- what every net must hold (raises AssertionError when an edge is lost) -----------------------------------------------------
def check_crowded(net, fused=False):
    """the edges of `crowded`; with fused = True the same facts by node (the twins share their nodes)"""
    L = layout(net)
    ext = int(net.ext_grid_bus)
    assert (net.n_load, net.n_sgen) == (9, 5)
    lpn, spn = L["loads_per_node"], L["sgens_per_node"]
    assert any(lpn[b] == 3 for b in L["multi_load_only"]), "three loads on one load-only bus"
    assert any(lpn[b] == 4 and spn[b] == 2 and b != ext for b in L["pv"]), "four loads and two sgens on one PV bus"
    assert lpn[ext] == 1 and spn[ext] == 1, "one load and one sgen on the ext_grid bus"
    assert any(lpn[b] == 0 for b in L["pv"]), "a PV bus with no load"
    assert any(lpn[b] == 1 and b != ext for b in L["pv"]), "a PV bus with exactly one load"
    assert len(L["empty"]) >= 2, "two buses with no element"
    s = net.load_scaling
    assert (s == 0.0).any() and (s > 1.0).any() and ((s > 0.0) & (s < 1.0)).any() and (net.sgen_scaling != 1.0).all()
    assert len(L["load_only"]) < len(L["pv"]), "fewer load-only buses than PV buses"
    assert obs_columns(net) % 4 != 0 and obs_columns(net) > 128
    assert set(L["ld_dest"]) == {1, 2}                        # (kind 0 needs a tenth load: one_sgen has seven)
    big = next(b for b in L["pv"] if lpn[b] == 4 and b != ext)
    three = next(b for b in L["multi_load_only"] if lpn[b] == 3)
    assert {big, three} <= set(scaled_sum_nodes(net)), "scaled loads sharing the four-load PV bus and the three-load bus"
    if not fused:
        assert not net.has_fused_buses and np.array_equal(L["loads_per_bus"], lpn)
    return L


def check_crowded_fused(net):
    """crowded_fused: the three groups, and every twin with elements of its own beside elements left on its representative"""
    L = check_crowded(net, fused=True)
    alias, nb = np.asarray(net.bus_alias), net.n_bus
    twins = np.flatnonzero(alias != np.arange(nb))
    ext = int(net.ext_grid_bus)
    big_pv = next(b for b in L["pv"] if L["loads_per_node"][b] == 4)
    three = next(b for b in L["multi_load_only"] if L["loads_per_node"][b] == 3)
    assert sorted(alias[twins]) == sorted([ext, big_pv, three])
    lpb, spb = L["loads_per_bus"], L["sgens_per_bus"]
    t = {int(alias[b]): int(b) for b in twins}
    assert lpb[t[ext]] == 1 and lpb[ext] == 0 and spb[ext] == 1, "the ext_grid bus's load sits on its twin, its sgen on itself"
    assert lpb[t[big_pv]] == 2 and lpb[big_pv] == 2 and spb[t[big_pv]] == 1 and spb[big_pv] == 1, "loads on both members of a group"
    assert lpb[t[three]] == 1 and lpb[three] == 2
    return L


def check_crowded_zip(net):
    L = check_crowded(net)
    on = np.asarray(net.load_bus) != net.ext_grid_bus
    assert net.has_zip_loads and (net.load_const_z[on] == ZIP_FRACTIONS[0]).all() and (net.load_const_i[on] == ZIP_FRACTIONS[1]).all()
    assert (net.load_const_z[~on] == 0).all() and (net.load_const_i[~on] == 0).all() and (~on).sum() == 1
    return L


def check_crowded_meshed(net):
    L = check_crowded(net)
    assert int(net.line_in_service.sum()) == net.n_bus, "one tie line beyond the spanning tree"
    return L


def check_one_sgen(net):
    L = layout(net)
    ext = int(net.ext_grid_bus)
    assert net.n_sgen == 1 and net.n_load % 2 == 0
    assert len(L["pv"]) == 1 and len(L["load_only"]) > 2, "many load-only buses for the one PV bus"
    assert ext in L["load_only"] and L["loads_per_node"][ext] == 1, "a load alone on the ext_grid bus"
    assert [L["loads_per_node"][b] for b in L["multi_load_only"]] == [2], "two loads on one load-only bus"
    assert obs_columns(net) <= 64
    assert L["multi_load_only"] == scaled_sum_nodes(net), "both loads of the two-load bus scaled"
    assert (L["ld_dest"] == 0).sum() >= 2 and (L["ld_dest"] == 2).sum() == 3
    return L


def check_all_pv(net):
    L = layout(net)
    assert (net.n_load, net.n_sgen) == (1, 4)
    assert int(net.load_bus[0]) in L["pv"] and L["load_only"] == [] and L["multi_load_only"] == []
    assert list(L["ld_dest"]) == [1]
    assert obs_columns(net) % 4 == 0
    return L


CHECKS = dict(crowded=check_crowded, crowded_fused=check_crowded_fused, crowded_zip=check_crowded_zip, crowded_meshed=check_crowded_meshed,
              one_sgen=check_one_sgen, all_pv=check_all_pv)


# ---- the nets -----------------------------------------------------------------------------------------------------------------
def _profiles(net, p_nom, pv_factor, seed):
    q_nom = p_nom * np.tan(np.arccos(0.95))
    w = np.random.default_rng(seed + 7).uniform(0.7, 1.3, net.n_sgen)
    return synth_profiles(p_nom, q_nom, pv_factor * p_nom.sum() * w / w.sum(), days=DAYS, seed=seed)


def _zones(net):
    return [np.flatnonzero(net.bus_zone == z) for z in (1, 2)]


def crowded_buses(net):
    """(ext_grid bus, the crowded PV bus, the three-load bus) of crowded and its variants"""
    L = layout(net)
    return (int(net.ext_grid_bus), next(b for b in L["pv"] if L["loads_per_node"][b] == 4),
            next(b for b in L["multi_load_only"] if L["loads_per_node"][b] == 3))


def _crowded():
    seed = 9300
    net, p_nom = _radial_case("crowded", 16, 9, 5, 2, 4, 12.47, 10.0, 2.4, seed, 0.05)
    z1, z2 = _zones(net)                                      # six buses each, ascending
    ext = int(net.ext_grid_bus)
    zone = net.bus_zone.copy()
    zone[ext] = 1                                             # an sgen on the ext_grid bus needs a non-main zone there (plan.cpp)
    big, free_pv, one_pv, three = int(z1[0]), int(z2[0]), int(z2[1]), int(z2[2])
    #                  load 0     1    2    3     4     5      6     7    8      (load 8 / sgen 4: the odd tail of a Philox pair)
    load_bus = np.array([three, big, ext, three, big, one_pv, big, three, big])
    sgen_bus = np.array([free_pv, big, ext, one_pv, big])
    net = dataclasses.replace(net, bus_zone=zone, load_bus=load_bus, sgen_bus=sgen_bus, sgen_zone=np.array([2, 1, 1, 2, 1]),
                              load_scaling=np.array([1.0, 0.0, 1.0, 1.3, 0.7, 1.0, 1.2, 0.9, 1.1]),
                              sgen_scaling=np.array([0.9, 1.05, 0.8, 1.1, 0.95]))
    return net, _profiles(net, p_nom, 3.0, seed)


def _one_sgen():
    seed = 9310
    net, p_nom = _radial_case("one_sgen", 13, 10, 1, 1, 4, 12.47, 10.0, 2.0, seed, 0.05)
    ext = int(net.ext_grid_bus)
    main = set(np.flatnonzero(net.bus_zone == 0).tolist())
    f, t = net.line_from_bus.astype(int), net.line_to_bus.astype(int)
    head = next(int(b) for a, b in list(zip(f, t)) + list(zip(t, f)) if a in main and b not in main)   # the zone bus on the trunk
    others = [int(b) for b in range(net.n_bus) if b not in (ext, head)]                               # 11 buses
    two = others[3]
    singles = [b for b in others if b != two][:7]
    load_bus = np.array([singles[0], two, singles[1], ext, singles[2], singles[3], two, singles[4], singles[5], singles[6]])
    net = dataclasses.replace(net, load_bus=load_bus, sgen_bus=np.array([head]), sgen_zone=np.array([1]),
                              load_scaling=np.array([1.0, 0.8, 1.0, 1.0, 1.1, 1.0, 1.25, 1.0, 0.9, 1.0]), sgen_scaling=np.array([0.9]))
    return net, _profiles(net, p_nom, 1.5, seed)


def _all_pv():
    seed = 9320
    # (the impedances are those of the feeder with eight spread loads of 2 MW: _radial_case scales them to the voltage drop of its own
    # loads, and one load near the head would leave lines of 20 ohm)
    net, _ = _radial_case("all_pv", 13, 8, 4, 2, 3, 12.47, 10.0, 2.0, seed, 0.05)
    z1, z2 = _zones(net)
    sgen_bus = np.array([z1[1], z2[0], z1[3], z2[4]])
    net = dataclasses.replace(net, load_bus=np.array([sgen_bus[2]]), sgen_bus=sgen_bus, sgen_zone=np.array([1, 2, 1, 2]),
                              load_scaling=np.array([1.15]), sgen_scaling=np.array([1.0, 0.9, 1.1, 0.85]),
                              load_const_z=np.zeros(0), load_const_i=np.zeros(0))
    return net, _profiles(net, np.array([0.8]), 3.0, seed)


@functools.lru_cache(maxsize=None)
def make(name):
    """(NetSpec, Profiles) of a net of this module, or of a key of tests/meshed_edge_nets.py (whose step() tests replay the plans below);
    cached, so treat both as read-only"""
    if name not in NETS:
        from tests import meshed_edge_nets
        if name not in meshed_edge_nets.KEYS:
            raise KeyError(name)
        return meshed_edge_nets.make_net(name)
    if name == "one_sgen":
        return _one_sgen()
    if name == "all_pv":
        return _all_pv()
    net, prof = _crowded()
    if name == "crowded":
        return net, prof
    ext, big, three = crowded_buses(net)
    on = lambda b: [int(i) for i in np.flatnonzero(net.load_bus == b)]
    if name == "crowded_fused":
        moves = [(on(ext)[0], 0), (on(big)[1], 1), (on(big)[3], 1), (on(three)[1], 2)]
        sg = [(int(np.flatnonzero(net.sgen_bus == big)[0]), 1)]
        return add_fused_buses(net, [ext, big, three], move_loads=moves, move_sgens=sg), prof
    if name == "crowded_zip":
        return with_zip(net, *ZIP_FRACTIONS), prof
    if name == "crowded_meshed":
        z1, z2 = _zones(net)
        out = add_lines(net, [int(z1[-1])], [int(z2[-1])], 0.4, 0.3)
        out.name = "crowded_meshed"
        return out, prof
    raise KeyError(name)


# ---- host-only handles ----------------------------------------------------------------------------------------------------------
def host_handle(name, B, tuning=None, **args):
    """(0, kernel dict of _lib.nr_kernel) of a host-only handle (device = -1) on a net of this module, or (error code, message)"""
    net, _ = make(name)
    lib = _lib.load()
    cn, keep = _lib.make_cnetspec(net)
    cc = _lib.make_cconfig(dict(ARGS, **args), 0, tuning)
    h = C.c_void_p()
    rc = lib.mapdn_create(C.byref(cn), C.byref(cc), int(B), -1, C.byref(h))
    if rc:
        return rc, lib.mapdn_last_error(None).decode()
    try:
        return 0, _lib.nr_kernel(h)
    finally:
        lib.mapdn_destroy(h)


# ---- the trajectories both test files replay --------------------------------------------------------------------------------------
# Two plans per net, B_WATCH envs, episode_limit 4 (three steps an episode), noisy, seed 0:
#   "auto"    auto_reset: reset(), then 10 step() calls with float64 actions.  Call 2 ends every episode, call 3 restarts every env; at call 4
#             env 7 gets the unsolvable action, so it restarts at call 5 and runs out of step with the others from there on.
#   "frozen"  no auto_reset (the injection runs in k_nr_tree's prologue), float32 actions: reset(), calls 0 .. 3 with env 7 unsolvable at
#             call 1 (frozen from call 2 on; call 3 finds every env frozen), a whole-batch reset(), then calls 4 .. 6.
# The oracle alone must get through both without another unsolvable step and without a second draw in any reset: replay() asserts it, so the
# GPU tests cannot hide a failure behind "unsolvable on both sides" (tests/test_element_edges_cpu.py runs replay() without a handle).
B_WATCH, FORCED_ENV, UNSOLVABLE = 21, 7, 60.0
PLANS = dict(auto=dict(auto_reset=True, dtype=np.float64, calls=10, forced_call=4, reset_before=()),
             frozen=dict(auto_reset=False, dtype=np.float32, calls=7, forced_call=1, reset_before=(4,)))


def actions(name, plan, B=B_WATCH, unsolvable=UNSOLVABLE):
    """[calls, B, ns] seeded actions in (-0.8, 0.8) of a plan, in its dtype (float32: rounded once; the oracle gets these values as float64);
    `unsolvable`: the forced action (a stiffer net needs a larger one to have no power-flow solution)"""
    p = PLANS[plan]
    net, _ = make(name)
    rng = np.random.default_rng(sum(map(ord, name + plan)))
    a = rng.uniform(-0.8, 0.8, (p["calls"], B, net.n_sgen))
    a[p["forced_call"], FORCED_ENV] = unsolvable
    return a.astype(p["dtype"])


def oracle_class(name):
    """VoltageControlOracle, for crowded_zip on tests/zip_nets.runpp_zip (as tests/test_zip_loads_gpu.py swaps it in, but per instance)"""
    import oracle.env_restated as R
    if name != "crowded_zip":
        return R.VoltageControlOracle
    from tests.zip_nets import runpp_zip

    class ZipOracle(R.VoltageControlOracle):
        def _run(self, f, *a, **kw):
            keep, R.runpp_restated = R.runpp_restated, runpp_zip
            try:
                return f(*a, **kw)
            finally:
                R.runpp_restated = keep

        def reset(self, *a, **kw):
            return self._run(super().reset, *a, **kw)

        def step(self, *a, **kw):
            return self._run(super().step, *a, **kw)
    return ZipOracle


def oracles(name, B=B_WATCH, env_id_offset=0, **args):
    net, prof = make(name)
    cls = oracle_class(name)
    return [cls(net, prof, dict(ARGS, **args), env_id=env_id_offset + e, do_reset=False) for e in range(B)]


def first_draw_reset(o, start=None):
    """o.reset() that must find a solvable start on its first draw"""
    d0 = o.draw
    out = o.reset(start=start) if start is not None else o.reset()
    assert o.draw == d0 + 1, f"env {o.env_id}: reset needed {o.draw - d0} draws"
    return out


def replay(name, plan, unsolvable=UNSOLVABLE):
    """Generator over a plan.  Yields ("reset", None, None, oracles) after every whole-batch reset and ("step", call, (act, expect), oracles)
    after every call: act [B, ns] in the plan's dtype, expect[e] = (kind, reward, terminated, info dict or None) with kind "step" |
    "restart" (auto_reset: this call was the env's reset) | "frozen"; the oracles are in the state after that call."""
    p = PLANS[plan]
    os_ = oracles(name)
    acts = actions(name, plan, unsolvable=unsolvable)
    for o in os_:
        first_draw_reset(o)
    yield "reset", None, None, os_
    done = [False] * B_WATCH
    for c in range(p["calls"]):
        if c in p["reset_before"]:
            for o in os_:
                first_draw_reset(o)
            done = [False] * B_WATCH
            yield "reset", None, None, os_
        expect = []
        for e, o in enumerate(os_):
            if done[e] and p["auto_reset"]:
                first_draw_reset(o)
                done[e] = False
                expect.append(("restart", 0.0, False, None))
            elif done[e]:
                expect.append(("frozen", 0.0, True, None))
            else:
                r, t, info = o.step(acts[c, e].astype(np.float64))
                forced = (c, e) == (p["forced_call"], FORCED_ENV)
                assert info["destroy"] == (1.0 if forced else 0.0), f"{name}/{plan}: call {c} env {e}: destroy = {info['destroy']}"
                assert t == (forced or o.steps >= ARGS["episode_limit"])
                done[e] = t
                expect.append(("step", r, t, info))
        yield "step", c, (acts[c], expect), os_


def start_rows_mix(name, B):
    """(rows int64 [B], bad bool [B]) for reset(start_rows=...): every ninth env (and the last) gets a row k_reset_begin refuses — negative,
    past the table, or the first row whose window start + episode_limit + 1 reaches T — the rest daytime and night rows of days 0 .. 2"""
    _, prof = make(name)
    T, lim = prof.n_rows, ARGS["episode_limit"]
    rng = np.random.default_rng(B + sum(map(ord, name)))
    rows = rng.integers(0, 3 * prof.intervals_per_day, B).astype(np.int64)
    bad = np.zeros(B, bool)
    bad[4::9] = True
    bad[B - 1] = True
    kinds = [-1, T - lim - 1, T + 5, -2 ** 40, 2 ** 40, T - 1]
    for i, e in enumerate(np.flatnonzero(bad)):
        rows[e] = kinds[i % len(kinds)]
    rows[0] = T - lim - 2                                     # the last good row
    return rows, bad


def row_to_start(prof, row):
    """(day, hour, interval) of a table row (the inverse of Profiles.start_row)"""
    day, rest = divmod(int(row), prof.intervals_per_day)
    hour, interval = divmod(rest, prof.intervals_per_hour)
    return day, hour, interval


def solve_inputs(name, B):
    """(p_load, q_load, p_sgen, q_sgen) [B, .] of a solve() on explicit inputs: seeded table rows and clipped actions in (-0.8, 0.8)"""
    net, prof = make(name)
    rng = np.random.default_rng(3 + B)
    rows = rng.integers(0, prof.n_rows, B)
    pv = prof.pv[rows]
    qs = rng.uniform(-0.8, 0.8, (B, net.n_sgen)) * np.sqrt(prof.s_max() ** 2 - pv ** 2)
    return prof.load_p[rows], prof.load_q[rows], pv, qs
