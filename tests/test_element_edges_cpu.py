"""The nets of tests/element_edge_nets.py without a GPU: every net holds the edges it was built for (and its check fails once an edge is
taken away), a host-only handle takes it under every tuning the GPU tests use, the oracle alone gets through the trajectories the GPU
tests replay without an unsolvable step or a second reset draw, and bus_demand / make_sbus of oracle/pp_restated.py mean, on these
nets, the plain sum by bus over the element tables."""
import dataclasses

import numpy as np
import pytest

from oracle.pp_restated import bus_demand, make_sbus, runpp_restated
from tests import element_edge_nets as N

LD = np.longdouble


# ---- the nets hold their edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", N.NETS)
def test_net_holds_its_edges(name):
    net, prof = N.make(name)
    N.CHECKS[name](net)
    assert net.n_bus <= 20 and prof.days == N.DAYS - 1 and prof.n_rows == N.DAYS * prof.intervals_per_day
    assert prof.n_start_days(N.ARGS["episode_limit"]) >= 2


def _move_load(net, li, bus):
    lb = net.load_bus.copy()
    lb[li] = bus
    return dataclasses.replace(net, load_bus=lb)


def _mutations(name):
    """(what is taken away, mutated copy) per net: each must make the net's check raise"""
    net, _ = N.make(name)
    L = N.layout(net)
    empty = L["empty"][-1]
    if name.startswith("crowded"):
        ext, big, three = N.crowded_buses(net)
        alias = np.asarray(net.bus_alias)
        third = int(np.flatnonzero(alias[net.load_bus] == three)[-1])
        yield "the third load leaves the three-load bus", _move_load(net, third, empty)
        yield "the ext_grid bus loses its load", _move_load(net, int(np.flatnonzero(alias[net.load_bus] == ext)[0]), empty)
        yield "load scalings of 1", dataclasses.replace(net, load_scaling=np.ones(net.n_load))
        sc = net.load_scaling.copy()
        sc[alias[net.load_bus] == three] = 1.0
        yield "the three-load bus with scalings of 1", dataclasses.replace(net, load_scaling=sc)
        one = next(b for b in L["pv"] if L["loads_per_node"][b] == 1 and b != ext)
        yield "no PV bus with exactly one load", _move_load(net, int(np.flatnonzero(net.load_bus == one)[0]), empty)
    if name == "crowded_fused":
        ext, big, three = N.crowded_buses(net)
        twin = int(np.flatnonzero((np.asarray(net.bus_alias) == big) & (np.arange(net.n_bus) != big))[0])
        yield "all loads of the crowded PV group on one member", _move_load(net, int(np.flatnonzero(net.load_bus == twin)[0]), big)
    if name == "crowded_zip":
        yield "no ZIP fractions", dataclasses.replace(net, load_const_z=np.zeros(0), load_const_i=np.zeros(0))
    if name == "crowded_meshed":
        keep = np.arange(net.n_line) < net.n_line - 1
        yield "the tie line opens", dataclasses.replace(net, line_in_service=np.where(keep, net.line_in_service, 0))
    if name == "one_sgen":
        ext = int(net.ext_grid_bus)
        yield "the ext_grid bus loses its load", _move_load(net, int(np.flatnonzero(net.load_bus == ext)[0]), empty)
        two = L["multi_load_only"][0]
        yield "no bus with two loads", _move_load(net, int(np.flatnonzero(net.load_bus == two)[0]), empty)
        sc = net.load_scaling.copy()
        sc[net.load_bus == two] = 1.0
        yield "the two-load bus with scalings of 1", dataclasses.replace(net, load_scaling=sc)
    if name == "all_pv":
        yield "the load leaves the PV bus", _move_load(net, 0, empty)


@pytest.mark.parametrize("name", N.NETS)
def test_the_checks_fail_once_an_edge_is_removed(name):
    muts = list(_mutations(name))
    assert muts
    for what, mutated in muts:
        with pytest.raises(AssertionError):
            N.CHECKS[name](mutated)
            print(f"{name}: '{what}' passed the check")


def test_layout_restates_the_rule_on_a_net_with_every_kind():
    """layout() by hand on crowded_fused: nodes by representative, the ext_grid node kept out of the mlo rows, kinds of ld_dest"""
    net, _ = N.make("crowded_fused")
    L = N.layout(net)
    ext, big, three = N.crowded_buses(net)
    assert ext in L["pv"] and big in L["pv"] and L["load_only"] == [three] == L["multi_load_only"]
    assert L["loads_per_node"].sum() == net.n_load == L["loads_per_bus"].sum() and L["sgens_per_node"].sum() == net.n_sgen
    assert (L["loads_per_node"][np.asarray(net.bus_alias) != np.arange(net.n_bus)] == 0).all()
    net1, _ = N.make("one_sgen")
    L1 = N.layout(net1)
    assert int(net1.ext_grid_bus) in L1["load_only"] and int(net1.ext_grid_bus) not in L1["multi_load_only"]
    for li, b in enumerate(net1.load_bus):
        alone = (net1.load_bus == b).sum() == 1
        assert L1["ld_dest"][li] == (0 if alone and b != net1.ext_grid_bus else 2)


# ---- host-only handles ----------------------------------------------------------------------------------------------------------------
TUNINGS = [None, dict(fuse_inject=1), dict(fuse_inject=2), dict(inject_full=1), dict(nr_solver="sparse"), dict(nr_solver="dense")]
# the documented refusals: ZIP loads under the dense solver; the fused prologue on a meshed net (it is part of k_nr_tree)
REFUSED = {("crowded_zip", "nr_solver"): "voltage-dependent loads (load_const_z / load_const_i) are not built for nr_solver = dense",
           ("crowded_meshed", "fuse_inject"): "fuse_inject = 1 exists on the tree solver only"}


@pytest.mark.parametrize("name", N.NETS)
def test_host_only_handles_take_every_net(name):
    for B in (1, N.B_WATCH, 70, 449):
        rc, k = N.host_handle(name, B)
        assert rc == 0, k
        assert k["solver"] == (1 if name == "crowded_meshed" else 0), k
        assert k.get("ZIP", 0) == int(name == "crowded_zip")
    for tuning in TUNINGS:
        rc, k = N.host_handle(name, 70, tuning)
        key = (name, next(iter(tuning))) if tuning else None
        refusal = REFUSED.get(key) if tuning in (dict(nr_solver="dense"), dict(fuse_inject=1)) else None
        if refusal:
            assert rc != 0 and refusal in k, k
        else:
            assert rc == 0, (tuning, k)
    rc, k = N.host_handle(name, 70, None, auto_reset=True)
    assert rc == 0, k
    rc, k = N.host_handle(name, 70, dict(inject_full=1), auto_reset=True)
    assert rc == 0, k
    if name == "crowded":                                      # the two pinned geometries of the injection-path test
        for W, L_ in ((4, 16), (1, 32)):
            rc, k = N.host_handle(name, 70, dict(nr_waves=W, nr_lanes=L_, fuse_inject=1))
            assert rc == 0 and (k["W"], k["L"]) == (W, L_), k
    if name == "crowded_meshed":
        rc, k = N.host_handle(name, 70)
        assert k["solver"] == 1                                # k_nr_sparse


# ---- the reference alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", list(N.PLANS))
@pytest.mark.parametrize("name", N.NETS)
def test_the_oracle_alone_runs_the_replayed_trajectories(name, plan):
    """replay() asserts it call by call: every step but the forced one converges, every reset takes its first draw"""
    p = N.PLANS[plan]
    n_step = n_forced = n_restart = n_frozen = n_reset = 0
    vmin, vmax = np.inf, -np.inf
    for kind, call, x, os_ in N.replay(name, plan):
        if kind == "reset":
            n_reset += 1
            continue
        act, expect = x
        assert act.dtype == p["dtype"] and act.shape == (N.B_WATCH, os_[0].net.n_sgen)
        for e, (k, r, t, info) in enumerate(expect):
            n_step += k == "step"
            n_restart += k == "restart"
            n_frozen += k == "frozen"
            n_forced += k == "step" and info["destroy"] == 1.0
            vmin, vmax = min(vmin, os_[e].res.vm_pu.min()), max(vmax, os_[e].res.vm_pu.max())
    assert n_forced == 1
    assert vmin > 0.85 and vmax < 1.15, (vmin, vmax)           # a net in working order, not one at the edge of collapse
    if plan == "auto":
        assert n_reset == 1 and n_frozen == 0 and n_restart >= 2 * N.B_WATCH
    else:
        assert n_reset == 2 and n_restart == 0 and n_frozen == N.B_WATCH + 1   # env 7 at call 2, every env at call 3


def test_the_oracle_alone_solves_the_start_row_mix_and_the_explicit_inputs():
    name, B = "crowded", 449
    net, prof = N.make(name)
    rows, bad = N.start_rows_mix(name, B)
    T, lim = prof.n_rows, N.ARGS["episode_limit"]
    assert np.array_equal(bad, (rows < 0) | (rows + lim + 1 >= T)) and 40 < bad.sum() < 60 and not bad[0] and bad[B - 1]
    assert (rows[bad] == T - lim - 1).any() and rows[0] == T - lim - 2       # the first refused row and the last good one
    assert bad[256:].any() and (~bad[256:]).any()              # both kinds beyond the first 256 envs of k_stats
    for e, o in enumerate(N.oracles(name, B)):
        if not bad[e]:
            start = N.row_to_start(prof, rows[e])
            assert prof.start_row(*start) == rows[e]
            N.first_draw_reset(o, start)
    pl, ql, pv, qs = N.solve_inputs(name, 70)
    for e in range(70):
        assert runpp_restated(net, pl[e], ql[e], pv[e], qs[e]).converged


# ---- what Sbus of a crowded bus means -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", N.NETS)
def test_bus_demand_is_the_sum_by_bus_over_the_element_tables(name):
    """bus_demand / make_sbus against a numpy.longdouble sum by bus, element by element, on table rows of the net: within 4 eps of the
    largest term of the bus (a float64 sum of up to six terms rounds at most five times, each by half an ulp of a partial sum that the
    largest term times six bounds; the longdouble sum is exact to 2^-64)"""
    net, prof = N.make(name)
    rng = np.random.default_rng(5)
    eps = np.finfo(np.float64).eps
    for row in rng.integers(0, prof.n_rows, 12):
        pl, ql, pv = prof.load_p[row], prof.load_q[row], prof.pv[row]
        qs = rng.uniform(-0.8, 0.8, net.n_sgen) * np.sqrt(prof.s_max() ** 2 - pv ** 2)
        pd_, qd = bus_demand(net, pl, ql, pv, qs)
        sb = make_sbus(net, pd_, qd)
        for b in range(net.n_bus):
            terms_p = [LD(pl[i]) * LD(net.load_scaling[i]) for i in range(net.n_load) if net.load_bus[i] == b] + \
                      [-LD(pv[j]) * LD(net.sgen_scaling[j]) for j in range(net.n_sgen) if net.sgen_bus[j] == b]
            terms_q = [LD(ql[i]) * LD(net.load_scaling[i]) for i in range(net.n_load) if net.load_bus[i] == b] + \
                      [-LD(qs[j]) * LD(net.sgen_scaling[j]) for j in range(net.n_sgen) if net.sgen_bus[j] == b]
            for got, sbus, terms in ((pd_[b], sb[b].real, terms_p), (qd[b], sb[b].imag, terms_q)):
                if not terms:
                    assert got == 0.0 and sbus == 0.0
                    continue
                big = max(abs(t) for t in terms)
                ref = sum(terms, LD(0))
                assert abs(LD(got) - ref) <= 4 * eps * big, (name, b, got, ref)
                assert abs(LD(sbus) + ref / LD(net.sn_mva)) <= 4 * eps * big / LD(net.sn_mva), (name, b)
