"""CPU: the sparse-program gradient and OPF kernels at the edges of their sgen table and at feeder size (tests/sparse_table_cases.py;
DESIGN.md section 27) without a GPU — the references and host-only handles alone:
  1. every net holds the edge it is named for;
  2. the edge is visible: the columns that only a second turn of a sub-lane reaches carry 1e-3 of the largest entry, so that a stride
     or tail slip, restated in numpy, misses the bar by three orders of magnitude;
  3. the asymmetric Ybus of special_meshed is visible in the adjoint solution;
  4. the exported program, run in numpy for every S that fits, solves the adjoint system and gives the sensitivities' columns;
  5. the conditions the loop tests stand on, by tests/opf_ref.py alone;
  6. the gradient scenario, by the oracle alone;
  7. what host-only handles refuse and accept at 64 and 65 sgens;
  8. the new E64 constants of the bars."""
import ctypes as C

import numpy as np
import pytest

from mapdn_amd import _lib
from oracle.pp_restated import make_ybus
from tests import grad_ref as G
from tests import grad_sparse_cases as GS
from tests import meshed_edge_nets as M
from tests import opf_kernel_cases as K
from tests import opf_ref as R
from tests import opf_sparse_cases as OS
from tests import sparse_table_cases as ST
from tests import test_action_grad_sparse_cpu as TGC
from tests import test_opf_sparse_cpu as TOC

VISIBLE = 1e-3                                   # of the largest entry: what a column a second turn reaches must carry
MARGIN = 1e3                                     # ... so that losing it misses the bar by this factor
STATE_ENV = TOC.STATE_ENV
VISIBLE_ENV = 0                                  # the state of the visibility checks: env 0, every set-point 0 (one of the envs the GPU tests compare)
# the sp_lanes a host-only handle pinned to the sparse solver accepts, per key (sparse_table_cases.fits asks the handle; the others
# are refused for LDS, in meshed_edge_nets.LDS_REFUSAL's words)
ACCEPTED = {"ring33_s16": [16, 8, 4, 2], "ring33_s17": [16, 8, 4, 2], "ladder66_s33": [8, 4, 2], "ladder66_s64": [8, 4, 2],
            "ladder66_s65": [8, 4, 2], "ladder65_s4": [8, 4, 2], "special_meshed": [16, 8, 4, 2], "case141_ties": [4, 2]}
# 6. env ids whose solved rows keep clear of the kinks (searched on the CPU with the oracle alone, as test_action_grad_sparse_cpu.CPU_ENVS)
KINK_ENVS = {k: (0, 1, 2) for k in ST.KEYS}
KINK_ENVS["special_meshed"] = (1, 2, 3)
ON_BOX = 1e-9                                    # an action this close to +-1 sits on the box (the QP's bound rows end a rounding inside)


# ---- 1. every net holds its edge ------------------------------------------------------------------------------------------------------------
def test_keys_and_accepted_sp_lanes():
    assert set(ACCEPTED) == set(ST.KEYS)
    for key in ST.KEYS:
        assert ST.fits(key) == ACCEPTED[key] == OS.fits(key) == GS.fits(key), (key, ST.fits(key))


def test_sgen_and_node_counts_sit_on_the_strides():
    dims = {key: (OS.make(key)[0].n_bus - 1, OS.make(key)[0].n_sgen) for key in ST.KEYS}
    assert dims == {"ring33_s16": (32, 16), "ring33_s17": (32, 17), "ladder66_s33": (65, 33), "ladder66_s64": (65, 64), "ladder66_s65": (65, 65),
                    "ladder65_s4": (64, 4), "special_meshed": (24, 9), "case141_ties": (140, 22)}
    assert dims["ring33_s16"][1] == ST.DS and dims["ring33_s17"][1] == ST.DS + 1 and dims["ring33_s17"][1] % 2 == 1
    for key in ("ring33_s16", "ring33_s17"):                     # ns > S for S = 4 and 8, ns = / > S = 16, ns < S = 32
        assert [64 // L for L in ACCEPTED[key]] == [4, 8, 16, 32]
    assert 2 in ACCEPTED["ladder66_s33"] and dims["ladder66_s33"][1] > 64 // 2 and dims["ladder66_s33"][1] % 2 == 1
    assert dims["ladder66_s64"][1] == ST.OPF_MAX_NS and dims["ladder66_s65"][1] == ST.OPF_MAX_NS + 1
    for key in ("ladder66_s33", "ladder66_s64", "ladder66_s65"):  # a ragged last node row for every S
        assert all(dims[key][0] % (64 // L) == 1 for L in ACCEPTED[key])
    assert all(dims["ladder65_s4"][0] % (64 // L) == 0 for L in ACCEPTED["ladder65_s4"])
    assert all(dims["case141_ties"][0] > 4 * (64 // L) for L in ACCEPTED["case141_ties"]) and dims["case141_ties"][1] > ST.DS
    for key in ST.MANY_SGENS:
        assert dims[key][1] > ST.DS
    for key in ST.KEYS:                                           # meshed: the default handle is on the sparse solver
        lib, h, rc, x = OS.host_open(key)
        assert rc == 0, x
        try:
            d = _lib.CDims()
            assert lib.mapdn_dims(h, C.byref(d)) == 0 and not d.is_radial and _lib.nr_kernel(h)["solver"] == 1, key
        finally:
            lib.mapdn_destroy(h)


def test_special_meshed_has_the_transformer_on_a_cycle_and_a_dead_line_row():
    net, _, (hv, lv), dead = ST.special_meshed()
    assert ST.cycle_through(net, hv, lv)
    assert not ST.cycle_through(K._special()[0], hv, lv)          # (radial before the ties)
    Y = make_ybus(net)[0].toarray()
    assert abs(Y[hv, lv] - Y[lv, hv]) > 1.0 and abs(Y[hv, lv]) > 0
    alive = np.asarray(net.line_in_service)
    assert alive[dead] == 0 and alive.sum() == alive.shape[0] - 1
    a, b = int(net.line_from_bus[dead]), int(net.line_to_bus[dead])
    assert Y[a, b] == 0 and Y[b, a] == 0                          # the dead row joins nothing
    assert net.n_sgen == 9 and int(net.sgen_bus[-1]) == int(net.ext_grid_bus) and np.abs(np.asarray(net.sgen_scaling) - 1.0).min() > 0
    assert len(net.shunt_bus) == 1
    kids = [int(y) for x, y in zip(net.line_from_bus, net.line_to_bus) if int(x) == lv] + [hv]
    assert len(kids) >= 4


def test_case141_ties_has_22_sgens_two_of_them_on_one_bus():
    net = OS.make("case141_ties")[0]
    assert net.n_sgen == 22 and np.bincount(np.asarray(net.sgen_bus)).max() == 2
    base = OS.make_case("case141", days=ST.CASE_DAYS)[0]
    assert net.line_from_bus.shape[0] == base.line_from_bus.shape[0] + 4


# ---- 2. the edge is visible -----------------------------------------------------------------------------------------------------------------
def linearisation(key, e=STATE_ENV):
    net = OS.make(key)[0]
    _, _, pv, smax = OS.inputs(key, e)
    V, lim = OS.oracle_voltage(key, e, OS.setpoints(key, OS.B_MAX)[e]).V, R.limits(pv, smax)
    return net, V, lim, R.linearise(net, V, lim)


@pytest.mark.parametrize("key", [k for k in ST.MANY_SGENS if k in ST.OPF_KEYS])
def test_columns_of_a_second_turn_are_visible_in_g_H_and_S(key):
    net, V, lim, L = linearisation(key, VISIBLE_ENV)
    ns = net.n_sgen
    g, H, S = np.abs(L.g), np.abs(L.H), np.abs(L.S)
    second = np.arange(ST.DS, ns)
    assert second.size >= 1
    assert (g[second] >= VISIBLE * g.max()).all(), (key, (g / g.max())[second].min())
    assert (H[second].max(axis=1) >= VISIBLE * H.max()).all() and (H[second, second] >= VISIBLE * H.max()).all(), key
    assert (S.max(axis=0) >= VISIBLE * S.max()).all(), key            # EVERY column: the lone last column and column 0 included
    # k_opf_reduce_sparse's turns restated: as they are they give g and H; one turn only, or a stride one off, and the second-turn
    # columns stay unwritten (0 here) or land elsewhere — by more than MARGIN bars
    go, Ho = ST.strided_reduce(L.g, L.H)
    assert np.array_equal(go, L.g) and np.array_equal(Ho, np.triu(L.H) + np.triu(L.H, 1).T)
    for slip in ("turns", "stride"):
        gs, Hs = ST.strided_reduce(L.g, L.H, slip=slip)
        eg, eH = K.rel_err(gs, L.g), K.rel_err(Hs, L.H)
        print(f"\n[sparse tables] {key}: reduce with slip '{slip}': g off by {eg:.2e} (bar {OS.bar(key, 'g'):.2e}), H by {eH:.2e} (bar {OS.bar(key, 'H'):.2e})")
        assert eg >= MARGIN * OS.bar(key, "g") and eH >= MARGIN * OS.bar(key, "H"), (key, slip, eg, eH)


def test_a_wrong_tail_of_the_last_pair_is_visible():
    """ring33_s17: ns odd.  A tail that also writes the empty half of the last pair (j + 1 <= ns) puts a zero column one past the row,
    on column 0 of the next node's row; one that drops the lone last column leaves column ns - 1 unwritten"""
    key = "ring33_s17"
    net, V, lim, L = linearisation(key, VISIBLE_ENV)
    ns = net.n_sgen
    S = np.delete(L.S, net.ext_grid_bus, axis=0)
    flat = S.copy().ravel()
    flat[np.arange(1, S.shape[0]) * ns] = 0.0                             # S[p][ns] is S[p + 1][0]
    dropped = S.copy()
    dropped[:, ns - 1] = 0.0
    for name, wrong in (("one past the row", flat.reshape(S.shape)), ("last column dropped", dropped)):
        err = K.rel_err(wrong, S)
        print(f"\n[sparse tables] {key}: tail '{name}': S off by {err:.2e} (bar {OS.bar(key, 'S'):.2e})")
        assert err >= MARGIN * OS.bar(key, "S"), (name, err)


def gradient_rows(key, envs=(0, 1, 2)):
    os_, rows, cand, solved = GS.reference(key, envs, GS.K_MAX)
    out = []
    for i, o in enumerate(os_):
        for k in range(GS.K_MAX):
            if solved[i, k]:
                out.append(G.reward_gradient(o.net, G.env_args(o), rows[i][k]["r"].V, cand[i, k], G.limits(o)))
    return np.array(out)


@pytest.mark.parametrize("key", ["ladder66_s33", "ladder66_s64", "ladder66_s65", "ring33_s17", "case141_ties"])
def test_entries_of_a_second_turn_are_visible_in_the_gradient(key):
    """the read-out's turns j = s, s + S, ...: every entry from the smallest S that fits on (so from 32 at sp_lanes 2 on the ladders)
    carries 1e-3 of the row's largest; an entry left unwritten or written to another place is off by more than MARGIN bars"""
    g = np.abs(gradient_rows(key))
    ns = g.shape[1]
    first = min(64 // L for L in ACCEPTED[key])
    assert ns > first and (not key.startswith("ladder66") or ns > 64 // 2)
    rel = g / g.max(axis=1, keepdims=True)
    print(f"\n[sparse tables] {key}: smallest gradient entry from column {first} on, relative to its row: {rel[:, first:].min():.2e}")
    assert (rel[:, first:] >= VISIBLE).all(), (key, rel[:, first:].min())
    assert VISIBLE >= MARGIN * GS.bar(key)


# ---- 3. the asymmetry is visible ------------------------------------------------------------------------------------------------------------
def adjoint_inputs(key, e=STATE_ENV):
    net = OS.make(key)[0]
    lp, lq, pv, smax = OS.inputs(key, e)
    V = OS.oracle_voltage(key, e, OS.setpoints(key, OS.B_MAX)[e]).V
    n, pos, *_ = OS.host_program(key, 64 // ACCEPTED[key][0])
    return net, V, n, pos


def test_a_symmetric_ybus_assumption_moves_the_adjoint_solution_of_special_meshed():
    key = "special_meshed"
    net, V, n, pos = adjoint_inputs(key)
    J = M.program_jacobian(net, pos, V)
    Yp, Vp = GS.ybus_by_position(net, pos), V[np.array(pos)]
    right, wrong = GS.transposed_blocks_from_ybus(Yp, Vp), GS.transposed_blocks_from_ybus(Yp, Vp, swap=True)
    assert np.abs(right - J.T).max() <= TGC.HOST_TOL * np.abs(J).max()
    c_th, c_vm = GS.reference_c(net, dict(voltage_barrier_type="bowl", voltage_weight=1.0, q_weight=0.1, line_weight=None), V)
    p = np.array(pos[:n])
    c = np.ravel(np.column_stack([c_th[p], c_vm[p] * np.abs(V[p])]))
    lam, lam_wrong = np.linalg.solve(right, c), np.linalg.solve(wrong, c)
    moved = float(np.abs(lam_wrong - lam).max() / np.abs(lam).max())
    print(f"\n[sparse tables] {key}: Y_ij read for Y_ji moves the adjoint solution by {moved:.2e} of its largest entry (gradient bar {GS.bar(key):.2e})")
    assert moved > MARGIN * GS.bar(key), moved


# ---- 4. the exported program in numpy -------------------------------------------------------------------------------------------------------
ADJOINT_CASES = [(key, 64 // L) for key in ("special_meshed", "ladder66_s33", "case141_ties") for L in ACCEPTED[key]]


@pytest.mark.parametrize("key,S", ADJOINT_CASES, ids=[f"{k}-S{s}" for k, s in ADJOINT_CASES])
def test_program_on_transposed_blocks_solves_the_adjoint_system(key, S):
    """against numpy.linalg.solve(J', c).  The bound is what float64 is good for on this system, not a measurement of the program: both
    solutions carry a forward error of the order of eps cond(J'), and 16 x that separates them at most (DESIGN.md section 16's factor)"""
    net, V, n, pos = adjoint_inputs(key)
    _, _, dims, ops, slots = OS.host_program(key, S)
    J = M.program_jacobian(net, pos, V)
    JT = np.ascontiguousarray(J.T)
    if key == "special_meshed":                                   # (the blocks the kernel forms: from Y_ji)
        JT = GS.transposed_blocks_from_ybus(GS.ybus_by_position(net, pos), V[np.array(pos)])
    c = np.random.default_rng(5 + n + S).uniform(-1.0, 1.0, 2 * n)
    got = M.emulate_program(n, S, dims, ops, slots, JT, c)
    want = np.linalg.solve(J.T, c)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    bound = K.BAR_FACTOR * np.finfo(np.float64).eps * np.linalg.cond(J.T, np.inf)
    print(f"\n[sparse tables] {key} S={S}: transposed program, relative error {err:.2e} (bound {bound:.1e})")
    assert err <= bound, (key, S, err, bound)


COLUMN_CASES = [(key, 64 // L) for key in ("ring33_s17", "ladder66_s64") for L in ACCEPTED[key]]


@pytest.mark.parametrize("key,S", COLUMN_CASES, ids=[f"{k}-S{s}" for k, s in COLUMN_CASES])
def test_program_with_paired_columns_gives_every_column(key, S):
    """as tests/test_opf_sparse_cpu.py's, at 17 and 64 columns: 9 pairs with an empty last half, 32 pairs; against the extended
    reference at the bar of S and against tests/opf_ref.linearise at that bar plus the float64 reference's own error"""
    net, V, lim, L = linearisation(key)
    ref = K.linearise_ext(net, V, lim)
    got = OS.columns_by_program(key, S, V, lim)
    other = OS.columns_by_program(key, S, V, lim, partner=1)
    bar = OS.bar(key, "S")
    for which, x in (("pairs (j, j + 1)", got), ("partner j + 1, scaled", other)):
        err, err64 = K.rel_err(x, ref.S), K.rel_err(x, L.S)
        print(f"\n[sparse tables] {key} S={S}: {which}: S relative error {err:.2e} (bar {bar:.2e}), against opf_ref.linearise {err64:.2e}")
        assert err <= bar and err64 <= bar + OS.E64[key]["S"], (key, S, which, err, err64)
        assert (np.abs(x).max(axis=0) >= VISIBLE * np.abs(x).max()).all()
    # a column does not depend on its slot's other half, nor on which half it rides in: the even columns (half 0 in both runs) beside
    # another partner, the odd columns in half 1 beside column j - 1 and in half 0 beside column j + 1 — bit for bit
    assert np.array_equal(got, other), (key, S)


# ---- 5. the pool conditions of the loop tests, by the reference alone ------------------------------------------------------------------------
@pytest.mark.parametrize("key", ST.LOOP_KEYS + (ST.KKT_KEY,))
def test_reference_meets_the_pool_conditions(key):
    """on every row of opf_sparse_cases.rows_of (the states repeat with period 6): status 0 within max_iter; on the loop keys at least 3
    SQP iterations (QPs solved); at the returned point at least a third of the sgens strictly inside the box and at least one on it"""
    scale = ST.LOOP_SCALE[key]
    runs = [OS.reference_run(key, e, scale) for e in range(6)]
    inside = [float((np.abs(r.actions) < 1.0 - ON_BOX).mean()) for r in runs]
    on_box = [int((np.abs(r.actions) >= 1.0 - ON_BOX).sum()) for r in runs]
    print(f"\n[sparse tables ref] {key} x{scale}: status", [r.status for r in runs], "power flows", [r.iterations for r in runs],
          "QPs", [len(r.steps) for r in runs], "inside", [f"{x:.2f}" for x in inside], "on the box", on_box)
    assert all(r.status == 0 and r.iterations < R.DEFAULTS["max_iter"] for r in runs), key
    if key in ST.LOOP_KEYS:
        assert all(len(r.steps) >= 3 for r in runs), key
    for e in range(6):
        assert inside[e] >= 1.0 / 3.0 and on_box[e] >= 1, (key, e, inside[e], on_box[e])


@pytest.mark.parametrize("key", ST.OPF_KEYS)
def test_power_flows_of_the_probe_states_converge_in_a_few_iterations(key):
    net = OS.make(key)[0]
    a = OS.setpoints(key, OS.B_MAX)
    its = [OS.oracle_voltage(key, e, a[e]).iterations for e in range(6)]
    assert 2 <= min(its) and max(its) <= 4, (key, its)


# ---- 6. the gradient scenario, by the oracle alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ST.KEYS)
def test_gradient_scenario(key):
    os_, rows, cand, solved = GS.reference(key, GS.B_MAX, GS.K_MAX)
    pattern = np.array([True, True, False, True])
    assert solved[:, pattern].all() and (~solved[:, 2]).any(), key       # every candidate but the UNSOLVABLE column is solved
    assert (solved == pattern).all(), key                         # (what tests/test_action_grad_sparse_gpu.compare asserts: that column, for every env)
    assert (cand[:, 2] == ST.UNSOLVABLE[key]).all() and (cand[:, 0] == 0.0).all()
    ks_, krows, kcand, _ = GS.reference(key, KINK_ENVS[key], GS.K_MAX)
    dv, dq = GS.kink_margins(ks_, krows, kcand)
    print(f"\n[sparse tables ref] {key}: kink margins of envs {KINK_ENVS[key]}: |V| {dv:.2e} (threshold {TGC.V_MARGIN:.0e}), |q| {dq:.2e} ({TGC.Q_MARGIN:.0e})")
    assert dv >= TGC.V_MARGIN and dq >= TGC.Q_MARGIN, (key, dv, dq)


def test_gradient_scenario_with_the_line_weight_on_special_meshed():
    B, Kc = GS.VARIANT_SHAPE
    os_, rows, cand, solved = GS.reference("special_meshed", B, Kc, G.LINE_ARGS)
    assert (solved == np.array([True, True, False, True])).all()
    net = os_[0].net
    assert G.env_args(os_[0])["line_weight"] == 0.7 and int(np.asarray(net.line_in_service).sum()) == net.n_line - 1


# ---- 7. refusals and acceptances on host-only handles ---------------------------------------------------------------------------------------
def test_opf_refuses_65_sgens_and_lets_64_through():
    rc, msg = OS.opf_error("ladder66_s65", dict(meshed=1))
    assert rc == -1 and msg == "opf: more than 64 sgens are not supported", (rc, msg)
    rc, msg = OS.opf_error("ladder66_s64", dict(meshed=1))
    assert rc == -4 and "host-only" in msg and "not supported" not in msg, (rc, msg)
    for L in ACCEPTED["ladder66_s64"]:
        rc, msg = OS.opf_error("ladder66_s64", dict(meshed=1), OS.tuning("ladder66_s64", L))
        assert rc == -4 and "host-only" in msg, (L, rc, msg)


def test_action_gradients_has_no_sgen_cap():
    net = GS.make("ladder66_s65")[0]
    lib = _lib.load()
    for tuning in [dict(grad_meshed=1)] + [GS.tuning("ladder66_s65", L) for L in ACCEPTED["ladder66_s65"]]:
        rc, h, keep = TGC.host_handle(lib, net, tuning)
        assert rc == 0
        try:
            assert _lib.nr_kernel(h)["solver"] == 1
            got, msg = TGC.call(lib, h)
            assert got == -4 and "host-only" in msg and "not supported" not in msg, (tuning, got, msg)
        finally:
            lib.mapdn_destroy(h)


# ---- 8. the new E64 constants -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ST.OPF_KEYS)
def test_opf_e64_constants_are_what_the_float64_reference_gives(key):
    TOC.test_e64_constants_are_what_the_float64_reference_gives(key)


def test_gradient_e64_constants_are_re_measured_by_the_existing_test():
    """tests/test_action_grad_sparse_cpu.py parametrises its E64 test over the whole dict: the new entries are measured there"""
    for key in ST.KEYS:
        assert (key, ()) in GS.E64, key
    assert ("special_meshed", G.LINE_ARGS) in GS.E64
