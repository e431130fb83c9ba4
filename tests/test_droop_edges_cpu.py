"""CPU (-m "not gpu"): what tests/test_droop_edges_gpu.py relies on, asserted of the reference alone (tests/droop_ref.py on the oracle's
power flow), so that no GPU test can hide behind "both sides odd": the nets hold their edges, the collapse case shows the mix of fates
it was tuned for at the B and start rows the GPU test uses, and the caps on what the GPU test may leave uncompared hold.

collapse needs one config only (droop_edge_cases.COLLAPSE_CFG): statuses 0, 1 and 2 all occur under it.

reactive_ratio: with s_max = 1.2 x the table's PV peak, lim = sqrt(s_max^2 - p^2) >= sqrt(1 - 1 / 1.44) s_max = 0.553 s_max for every p the
table holds, so under ratio = 0.3 the factor min(1, ratio s_max / lim) is below 1 for EVERY sgen (at most 0.543) and never exactly 1: the
min binds everywhere, which is asserted.  An env in which it binds for one sgen and is exactly 1 for another needs a ratio between 0.553
and 1; RATIO_MIXED = 0.8 gives that on the crowded daytime rows (binds where p < 0.72 peak), and the GPU file runs both ratios."""
import numpy as np
import pytest

from tests import droop_edge_cases as D
from tests import element_edge_nets as N
from tests.droop_ref import law, resolve

RATIO_BINDS, RATIO_MIXED = 0.3, 0.8


@pytest.mark.parametrize("name", D.NETS)
def test_net_holds_its_edges(name):
    net = D.check(name)
    _, prof = D.make(name)
    assert net.n_bus <= (25 if name in D.STRIDE else 20)
    assert prof.n_start_days(D.ARGS["episode_limit"]) >= 2
    if name in D.STRIDE:
        assert net.n_sgen == D.STRIDE[name][0]
        assert net.n_sgen in (16, 17)                          # DS = 16: one sgen per sub-lane, and a second one on sub-lane 0


def test_collapse_shows_the_mix_of_fates():
    B = D.B_COLLAPSE
    net, prof = D.make("collapse")
    rows = D.night_rows("collapse", B)
    assert (prof.pv[rows + 1] == 0.0).all()                    # night: p is the noise alone, lim ~ s_max
    states = D.oracle_states("collapse", B, rows)
    smax = states[0][3]
    assert all((s[2] < 0.02 * smax).all() for s in states)
    res = D.collapse_reference(B)
    st = np.array([r.status for r, _ in res])
    it = np.array([r.iterations for r, _ in res])
    dec = np.array([d for _, d in res])
    c = resolve(D.COLLAPSE_CFG)
    # every sgen sees f = -1 at every solved point: the breakpoints lie below every voltage of the net
    for r, _ in res:
        if r.status in (0, 1):
            assert (law(r.vm_pu[net.sgen_bus], c["va"], c["vb"], c["vc"], c["vd"]) == -1.0).all() and r.vm_pu.min() > c["vd"]
    failed = st == 2
    assert len(set(it[failed].tolist())) >= 2 and (it[failed] >= 2).all()
    assert all(np.abs(r.actions).min() > 0.0 for r, _ in res if r.status == 2)                # a_sol of a solved point, not the start
    # the walk 0, -0.5, -0.75, ...: a_sol of an env that failed at solve i is the action of solve i - 1
    for r, _ in res:
        if r.status == 2:
            assert np.array_equal(r.actions, np.full(net.n_sgen, -(1.0 - 0.5 ** (r.iterations - 2))))
            assert np.isnan(r.vm_pu).all()
    assert any((st[g:g + 16] == 2).any() and (st[g:g + 16] <= 1).any() for g in range(0, B - 15, 16))
    assert set(st.tolist()) == {0, 1, 2}
    assert (failed & dec).sum() >= 3 and (~dec).sum() <= B // 4, (int((failed & dec).sum()), int((~dec).sum()))
    assert len(set(it[failed & dec].tolist())) >= 2           # the compared failures alone stop at more than one solve
    assert ((st == 0) & dec).any() and ((st == 1) & dec).any()


def test_collapse_batches_and_forced_env():
    """the batch-edge test shifts nothing: env e of every B starts at row e of the B = 33 list; the all-four-statuses test forces env 7,
    which must be one the loop would otherwise run to a decidable end, beside decidable neighbours of another fate"""
    rows = D.night_rows("collapse", D.B_COLLAPSE)
    for B in D.BATCHES:
        assert np.array_equal(D.night_rows("collapse", B), rows[:B])
    res = D.collapse_reference(D.B_COLLAPSE)
    st = [r.status for r, _ in res]
    dec = [d for _, d in res]
    assert all(dec[e] for e in range(14, 19)) or sum(dec[14:19]) >= 3        # the envs across the workgroup edge are mostly compared
    assert {st[e] for e in range(14, 19)} >= {0, 2}
    # after one step without reactive power (the all-four-statuses test stops env 7 with it) the mix is still there, beside env 7
    net, prof = D.make("collapse")
    want = {0: 2, 2: 0, 23: 1}
    for e, o in enumerate(D.oracles("collapse", D.B_COLLAPSE)):
        if e in want:
            N.first_draw_reset(o, N.row_to_start(prof, rows[e]))
            _, term, info = o.step(np.zeros(net.n_sgen))
            assert not term and info["destroy"] == 0.0
            r, ok = D.robust(net, (o.load_p, o.load_q, o.sgen_p, o.s_max), D.COLLAPSE_CFG)
            assert ok and r.status == want[e], (e, r.status)


@pytest.mark.parametrize("name", [n for n in D.NETS if n != "collapse"])
def test_reference_ends_cleanly_on_the_edge_nets(name):
    """defaults and the deadband config from the seeded starts and at noon rows: every power flow of the loop converges, also with s_max
    scaled by 0.98 and 1.02, and the net stays in working order (robust()'s iteration count is no criterion here: an ordinary stop
    moves by a solve with s_max, and the GPU test holds these envs to the exact count save the documented v_tol tie)"""
    B = D.B_PARITY
    for rows in (None, D.noon_rows(name, B)):
        for cfg in (None, D.DEADBAND):
            for s in D.oracle_states(name, B, rows)[::8]:
                r = D.ref(name, s, cfg)
                assert r.status in (0, 1) and r.iterations >= 2, (name, cfg, r.status, r.iterations)
                for k in (0.98, 1.02):
                    assert D.ref(name, s[:3] + (k * s[3],), cfg).status in (0, 1)
                assert 0.85 < np.nanmin(r.vm_pu) and np.nanmax(r.vm_pu) < 1.15


def _factors(ratio):
    out = []
    for lp, lq, pv, smax in D.oracle_states("crowded", D.B_PARITY, D.noon_rows("crowded", D.B_PARITY)):
        out.append(ratio * smax / np.sqrt(smax * smax - pv * pv))
    return np.array(out)


def test_reactive_ratio_on_the_crowded_daytime_rows():
    x = _factors(RATIO_BINDS)
    assert (x < 1.0).all() and x.max() < 0.3 / np.sqrt(1.0 - 1.0 / 1.44) + 1e-3      # binds for every sgen (the docstring's bound)
    y = _factors(RATIO_MIXED)
    both = ((y < 1.0).any(axis=1)) & ((y >= 1.0).any(axis=1))
    assert both.sum() >= 3, y                                  # in one env: binds for one sgen, exactly 1 for another
    assert (_factors(2.0) >= 1.0).all()                        # ratio 2: the factor is exactly 1, the bits of ratio 1
