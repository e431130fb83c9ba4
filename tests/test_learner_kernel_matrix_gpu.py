"""Every row of the learner kernel matrix (tests/learner_kernel_matrix.py) on the GPU, through the C ABI, against the PyTorch modules of
mapdn_amd/learner/modules.py (RNNAgent, MLPCritic) deep-copied to float64.

Bars.  means: 5e-6 x max(1, max |ref|), the bar tests/test_policy_trunk.py holds against float64.  hid_out / x1_out: the error of the stock
f32 modules against float64 on the same inputs is measured, the kernel may have 8 x that (its gates carry ~1e-7 absolute error where
f32 carries 6e-8, and its products sum in another order), floored at the means bar.  Critic head: the bars of tests/test_critic_head.py
(2e-6 / 3e-6 values and row-local gradients, 3e-7 sqrt(rows) parameter gradients, 2e-4 relative for the fused value loss).  The
measured figures are printed as "[learner matrix] ..." lines; DESIGN.md ("Learner kernels against float64") records them.

Every output buffer has guard rows filled with a sentinel on both sides, every scratch / gradient buffer is filled with NaN before the
launch: a store outside the documented elements, or a read of an element nobody wrote, shows."""
import copy

import pytest
import torch
import torch.nn.functional as F

from mapdn_amd import _lib
from mapdn_amd.learner import DDPGNet, MLPCritic, make_alg_args
from tests import learner_kernel_matrix as lm

pytestmark = pytest.mark.gpu
SENT = -7777.25                 # guard rows
G = 4                           # guard rows of 64 floats on either side of an output
MEANS_BAR = 5e-6
POLICY_ROWS = [r for r in lm.ROWS if r.kernel[0].startswith("policy_fwd")]
HEAD_IDX = [i for i, r in enumerate(lm.ROWS) if r.kernel[0] == "head_bwd"]
OTHER_IDX = [i for i, r in enumerate(lm.ROWS) if not r.kernel[0].startswith("policy_fwd") and r.kernel[0] != "head_bwd"]


def _dev():
    return torch.device("cuda:0")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _row(i):
    return lm.rows_for(_cus())[i]


def _setenv(monkeypatch, env):
    for k in ("MAPDN_POLICY_FWD_V1", "MAPDN_HEAD_BWD_THREADS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _guarded(rows, width, dev):
    """[rows, width] (or [rows] for width 0) inside a buffer with G x 64 sentinel floats on either side"""
    n = rows * max(width, 1)
    buf = torch.full((2 * G * 64 + n,), SENT, dtype=torch.float32, device=dev)
    view = buf[G * 64:G * 64 + n]
    return buf, (view.view(rows, width) if width else view)


def _guards_intact(buf, n):
    return bool((buf[:G * 64] == SENT).all()) and bool((buf[G * 64 + n:] == SENT).all())


def _scale(ref):
    return max(1.0, float(ref.abs().max()))


def _err(a, ref):
    return float((a.double() - ref.double()).abs().max())


# ================================================================================================================================
# policy forward
# ================================================================================================================================
def _agent(o, ids, seed, dev):
    n = ids if ids else 5                                           # without an id the agent index only cycles (5 does not divide 16)
    torch.manual_seed(seed)
    net = DDPGNet(make_alg_args(n, o, 1, agent_id=bool(ids)), "maddpg").to(dev)
    ag = net.policy_dicts[0]
    with torch.no_grad():
        ag.layernorm.weight.copy_(1.0 + 0.3 * torch.randn(64)); ag.layernorm.bias.copy_(0.2 * torch.randn(64))
        ag.fc2.weight.mul_(3.0)
    return ag, n


def _stock(ag, obs, hid, n, ids):
    """the modules as agents/rnn_agent.py:16-32 runs them, in the dtype of `ag`: (means, hidden, x1 = the LayerNorm input)"""
    rows = obs.shape[0]
    inp = obs
    if ids:
        inp = torch.cat((obs, F.one_hot(torch.arange(rows, device=obs.device) % n, ids).to(obs.dtype)), -1)
    x1 = ag.fc1(inp)
    h = ag.rnn(torch.relu(ag.layernorm(x1)), hid)
    return ag.fc2(h).reshape(rows), h, x1


def _prm(ag):
    return [t.detach().contiguous() for t in (ag.fc1.weight, ag.fc1.bias, ag.layernorm.weight, ag.layernorm.bias, ag.rnn.weight_ih, ag.rnn.weight_hh,
                                              ag.rnn.bias_ih, ag.rnn.bias_hh, ag.fc2.weight, ag.fc2.bias)]


def _launch_policy(ag, obs, hid, n, ids, train, want_hid):
    """one launch through the C ABI into guarded buffers: (means, hid_out or None, x1 or None); asserts the guards"""
    lib, dev = _lib.load(), obs.device
    rows, o = obs.shape
    prm = _prm(ag)
    mb, means = _guarded(rows, 0, dev)
    hb, hout = _guarded(rows, 64, dev) if want_hid else (None, None)
    xb, x1 = _guarded(rows, 64, dev) if train else (None, None)
    ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    st = torch.cuda.current_stream(dev).cuda_stream
    if train:
        rc = lib.mapdn_policy_forward_train(obs.data_ptr(), hid.data_ptr(), *(t.data_ptr() for t in prm), means.data_ptr(), ptr(hout), x1.data_ptr(),
                                            rows, n, o, ids, float(ag.layernorm.eps), st)
    else:
        rc = lib.mapdn_policy_forward(obs.data_ptr(), hid.data_ptr(), *(t.data_ptr() for t in prm), means.data_ptr(), ptr(hout), rows, n, o, ids,
                                      float(ag.layernorm.eps), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _guards_intact(mb, rows), "means: a store outside [0, rows)"
    assert hb is None or _guards_intact(hb, rows * 64), "hid_out: a store outside its rows"
    assert xb is None or _guards_intact(xb, rows * 64), "x1_out: a store outside its rows"
    assert bool((means != SENT).all()) and (hout is None or bool((hout != SENT).all())) and (x1 is None or bool((x1 != SENT).all()))
    return means, hout, x1


def _policy_row_counts(n):
    k = 7
    while (n * k) % 16 == 0:
        k += 1
    big = n * (-(-(_cus() * 8 * 16 * 5 // 4) // n))                # more 16-row tiles than CUs x wavefronts: the grid-stride loop turns
    big = max(big, n * (-(-40000 // n)))
    if big % 16 == 0:
        big += n
    return [1, 15, 16, 17, n * k, big]


def _inputs(rows, o, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(rows, o, generator=g).to(dev), (0.5 * torch.randn(rows, 64, generator=g)).to(dev)


def _bars(ref, stock):
    """(bar for means, hid, x1) from the float64 reference and the stock f32 modules' error against it"""
    out = [MEANS_BAR * _scale(ref[0])]
    for k in (1, 2):
        out.append(max(8.0 * _err(stock[k], ref[k]), MEANS_BAR * _scale(ref[k])))
    return out


@pytest.mark.parametrize("row", POLICY_ROWS, ids=[r.label for r in POLICY_ROWS])
def test_policy_forward_cell_against_float64(row, monkeypatch):
    dev = _dev()
    o, ids = row.shape["obs_dim"], row.shape["id_dim"]
    _setenv(monkeypatch, row.env)
    assert lm.reported_kernel(row) == row.kernel                    # the library reports the cell before it is launched
    ag, n = _agent(o, ids, 1000 * o + ids, dev)
    ag64 = copy.deepcopy(ag).double()
    worst = {k: [0.0, 0.0, 0.0] for k in ("means", "hid", "x1")}     # stock f32 error, kernel error, bar
    with torch.no_grad():
        for rows in _policy_row_counts(n):
            obs, hid = _inputs(rows, o, rows + o, dev)
            ref = _stock(ag64, obs.double(), hid.double(), n, ids)
            stock = _stock(ag, obs, hid, n, ids)
            bars = _bars(ref, stock)
            m0, _, _ = _launch_policy(ag, obs, hid, n, ids, train=False, want_hid=False)          # the rollout entry without hid_out
            m1, h1, _ = _launch_policy(ag, obs, hid, n, ids, train=False, want_hid=True)
            m2, h2, x2 = _launch_policy(ag, obs, hid, n, ids, train=True, want_hid=True)
            m3, _, x3 = _launch_policy(ag, obs, hid, n, ids, train=True, want_hid=False)          # what _PolicyTrunk calls
            # one kernel behind every entry, deterministic: the same bits
            assert torch.equal(m0, m1) and torch.equal(m1, m2) and torch.equal(m2, m3) and torch.equal(h1, h2) and torch.equal(x2, x3), rows
            for k, got, i in (("means", m1, 0), ("hid", h1, 1), ("x1", x2, 2)):
                e_s, e_k = _err(stock[i], ref[i]), _err(got, ref[i])
                if e_k / bars[i] >= worst[k][1] / max(worst[k][2], 1e-30):
                    worst[k] = [e_s, e_k, bars[i]]
                assert e_k <= bars[i], (k, rows, e_k, bars[i], e_s)
            # row independence: a NaN in one row's observation reaches that row only — every other row keeps its bits
            if rows >= 15:
                victim = 16 if rows > 16 else 5
                bad = obs.clone(); bad[victim, o // 2] = float("nan")
                mb, hb, xb = _launch_policy(ag, bad, hid, n, ids, train=True, want_hid=True)
                keep = torch.ones(rows, dtype=torch.bool, device=dev); keep[victim] = False
                assert torch.equal(mb[keep], m1[keep]) and torch.equal(hb[keep], h1[keep]) and torch.equal(xb[keep], x2[keep]), rows
                assert bool(mb[victim].isnan()) and bool(hb[victim].isnan().all()) and bool(xb[victim].isnan().all()), rows
    print(f"[learner matrix] {row.label}: " + "; ".join(f"{k} stock f32 {v[0]:.2e} kernel {v[1]:.2e} bar {v[2]:.2e}" for k, v in worst.items()))


FWD2_ROWS = [r for r in POLICY_ROWS if r.kernel[0] == "policy_fwd2"]


@pytest.mark.parametrize("row", FWD2_ROWS, ids=[r.label for r in FWD2_ROWS])
def test_policy_forward_forms_agree(row, monkeypatch):
    """k_policy_fwd and k_policy_fwd2 on the same inputs: within twice the bar each of them is held to"""
    dev = _dev()
    o, ids = row.shape["obs_dim"], row.shape["id_dim"]
    ag, n = _agent(o, ids, 1000 * o + ids, dev)
    ag64 = copy.deepcopy(ag).double()
    with torch.no_grad():
        for rows in _policy_row_counts(n)[-2:]:
            obs, hid = _inputs(rows, o, rows + o, dev)
            bars = _bars(_stock(ag64, obs.double(), hid.double(), n, ids), _stock(ag, obs, hid, n, ids))
            _setenv(monkeypatch, {})
            a = _launch_policy(ag, obs, hid, n, ids, train=True, want_hid=True)
            _setenv(monkeypatch, {"MAPDN_POLICY_FWD_V1": "1"})
            b = _launch_policy(ag, obs, hid, n, ids, train=True, want_hid=True)
            for k, x, y, bar in zip(("means", "hid", "x1"), a, b, bars):
                assert _err(x, y) <= 2.0 * bar, (k, rows, _err(x, y), bar)


SAT_ROWS = [r for r in POLICY_ROWS if (r.shape["obs_dim"], r.shape["id_dim"]) in ((58, 22), (95, 38), (97, 38), (175, 38))]


@pytest.mark.parametrize("row", SAT_ROWS, ids=[r.label for r in SAT_ROWS])
def test_policy_forward_saturated_gates(row, monkeypatch):
    """gate pre-activations beyond +-90, where __expf overflows to inf or flushes to 0: finite outputs equal to the float64 modules"""
    dev = _dev()
    o, ids = row.shape["obs_dim"], row.shape["id_dim"]
    _setenv(monkeypatch, row.env)
    ag, n = _agent(o, ids, 77, dev)
    with torch.no_grad():
        for gate in range(3):                                       # r, z, n: eight units at +100, eight at -100 each
            ag.rnn.bias_ih[64 * gate + 16 * gate:64 * gate + 16 * gate + 8] = 100.0
            ag.rnn.bias_ih[64 * gate + 16 * gate + 8:64 * gate + 16 * gate + 16] = -100.0
        ag64 = copy.deepcopy(ag).double()
        rows = _policy_row_counts(n)[-2]
        obs, hid = _inputs(rows, o, 5, dev)
        ref = _stock(ag64, obs.double(), hid.double(), n, ids)
        bars = _bars(ref, _stock(ag, obs, hid, n, ids))
        got = _launch_policy(ag, obs, hid, n, ids, train=True, want_hid=True)
        for k, x, r, bar in zip(("means", "hid", "x1"), got, ref, bars):
            assert bool(torch.isfinite(x).all()), k
            assert _err(x, r) <= bar, (k, _err(x, r), bar)


def test_recurrent_episode_drift(monkeypatch):
    """240 steps of one feeder's shape (38 agents, width 82) on 256 envs, the hidden state fed back: float64 modules, stock f32 modules
    and the kernel (both forms) side by side on the same observations.  At every step the kernel's distance from float64 in means and
    hidden state is at most 8 x the stock f32 modules' distance at that step, floored at the means bar"""
    dev = _dev()
    n, o, envs, steps = 38, 82, 256, 240
    rows = envs * n
    ag, _ = _agent(o, n, 4242, dev)
    ag64 = copy.deepcopy(ag).double()
    g = torch.Generator(device="cpu").manual_seed(240)
    h64 = torch.zeros(rows, 64, dtype=torch.float64, device=dev)
    h32 = torch.zeros(rows, 64, device=dev)
    hk = {"policy_fwd2": torch.zeros(rows, 64, device=dev), "policy_fwd": torch.zeros(rows, 64, device=dev)}
    envs_of = {"policy_fwd2": {}, "policy_fwd": {"MAPDN_POLICY_FWD_V1": "1"}}
    worst = {f: [0.0, 0.0] for f in hk}                              # largest kernel drift / allowance over the episode: means, hid
    last = {}
    with torch.no_grad():
        for t in range(steps):
            obs = torch.randn(rows, o, generator=g).to(dev)
            m64, h64, _ = _stock(ag64, obs.double(), h64, n, n)
            m32, h32, _ = _stock(ag, obs, h32, n, n)
            d32 = (_err(m32, m64), _err(h32, h64))
            allow = (max(8.0 * d32[0], MEANS_BAR * _scale(m64)), max(8.0 * d32[1], MEANS_BAR * _scale(h64)))
            for form in hk:
                _setenv(monkeypatch, envs_of[form])
                mk, hnew, _ = _launch_policy(ag, obs, hk[form], n, n, train=False, want_hid=True)
                hk[form] = hnew.clone()
                dk = (_err(mk, m64), _err(hnew, h64))
                assert dk[0] <= allow[0] and dk[1] <= allow[1], (form, t, dk, d32, allow)
                worst[form] = [max(worst[form][0], dk[0] / allow[0]), max(worst[form][1], dk[1] / allow[1])]
                last[form] = dk
    for form in hk:
        print(f"[learner matrix] episode {form} step {steps}: means stock f32 {d32[0]:.2e} kernel {last[form][0]:.2e}; hid stock f32 {d32[1]:.2e} "
              f"kernel {last[form][1]:.2e}; largest kernel drift / allowance over the episode: means {worst[form][0]:.2f} hid {worst[form][1]:.2f}")


def test_a_width_that_does_not_fit_takes_the_modules():
    """177 + 38: no launch shape — the library refuses the call by code, DDPGNet.policy computes with the PyTorch modules"""
    dev = _dev()
    n, o = 38, 177
    net = DDPGNet(make_alg_args(n, o, 1), "maddpg").to(dev)
    obs, hid = torch.randn(4, n, o, device=dev), torch.zeros(4, n, 64, device=dev)
    with torch.no_grad():
        assert not net._fused_policy_ok(obs, hid)
        means, _, h = net.policy(obs, hid)
        ag = net.policy_dicts[0]
        ref = _stock(ag, obs.reshape(4 * n, o), hid.reshape(4 * n, 64), n, n)
    assert torch.allclose(means.reshape(-1), ref[0], rtol=1e-5, atol=1e-6) and torch.allclose(h.reshape(-1, 64), ref[1], rtol=1e-5, atol=1e-6)
    prm = _prm(ag)
    out = torch.zeros(4 * n, device=dev)
    rc = _lib.load().mapdn_policy_forward(obs.data_ptr(), hid.data_ptr(), *(t.data_ptr() for t in prm), out.data_ptr(), None, 4 * n, n, o, n, 1e-5, None)
    assert rc == -1
    net = DDPGNet(make_alg_args(n, 176, 1), "maddpg").to(dev)
    with torch.no_grad():
        assert net._fused_policy_ok(torch.randn(4, n, 176, device=dev), hid)


# ================================================================================================================================
# critic head
# ================================================================================================================================
HEAD_PARAMS = ("layernorm.weight", "layernorm.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias")
GRAD_SLICES = ((4096, 4160), (4160, 4224), (0, 4096), (4224, 4288), (4288, 4352), (4352, 4353))      # of grads, in HEAD_PARAMS order


def _critic(dev, seed):
    torch.manual_seed(seed)
    cr = MLPCritic(7, 1, make_alg_args(3, 5, 1))
    with torch.no_grad():
        cr.layernorm.weight.copy_(1.0 + 0.3 * torch.randn(64)); cr.layernorm.bias.copy_(0.2 * torch.randn(64))
        cr.fc2.weight.copy_(0.2 * torch.randn(64, 64)); cr.fc2.bias.copy_(0.1 * torch.randn(64))
        cr.fc3.weight.copy_(0.3 * torch.randn(1, 64)); cr.fc3.bias.copy_(0.1 * torch.randn(1))
    return cr.to(dev)


def _head64(cr64, x):
    """critics/mlp_critic.py:22-36 behind the first layer, through the float64 copy of the modules"""
    return cr64.fc3(torch.relu(cr64.fc2(torch.relu(cr64.layernorm(x))))).reshape(-1)


def _head_inputs(shape, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if "nb" in shape:
        nb, n = shape["nb"], shape["n"]
        x = (1.2 * torch.randn(nb, 64, generator=g)).to(dev)
        pern = (0.8 * torch.randn(n, 64, generator=g)).to(dev)
    else:
        nb, n = shape["rows"], 1
        x, pern = (1.5 * torch.randn(nb, 64, generator=g) + 0.3).to(dev), None
    rows = nb * n
    return dict(x=x, pern=pern, n=n, nb=nb, rows=rows, dv=torch.randn(rows, generator=g).to(dev), dot_w=torch.randn(n, 64, generator=g).to(dev),
                wrow=(torch.rand(nb, generator=g) < 0.7).float().to(dev))


KINK = 2e-5


def _off_the_kinks(cr, inp, seed):
    """The gradient of a ReLU jumps at 0: a row with a pre-activation (LayerNorm output or fc2 output) within f32 rounding of 0 has no
    well-defined reference — f32 and float64 may take different sides (seen: fc2 output 2e-8 in 6 462 rows).  Such rows are redrawn
    until every pre-activation of the float64 modules is at least KINK = 2e-5 from 0, ten times the f32 error of a pre-activation of
    order 1 to 10; decided by the reference alone, before any kernel runs"""
    cr64 = copy.deepcopy(cr).double()
    g = torch.Generator(device="cpu").manual_seed(seed + 1)
    formed = inp["pern"] is not None
    for _ in range(50):
        x = (inp["x"].unsqueeze(1) + inp["pern"].unsqueeze(0)).reshape(-1, 64) if formed else inp["x"]
        with torch.no_grad():
            y = cr64.layernorm(x.double())
            pre = cr64.fc2(torch.relu(y))
        bad = ((y.abs() < KINK) | (pre.abs() < KINK)).any(-1)
        if formed:
            bad = bad.view(inp["nb"], inp["n"]).any(-1)
        k = int(bad.sum())
        if not k:
            return inp
        inp["x"][bad] = ((1.2 if formed else 1.5) * torch.randn(k, 64, generator=g) + (0.0 if formed else 0.3)).to(inp["x"].device)
    raise AssertionError("could not move the rows off the ReLU kinks")


def _run_head(cr, inp, mode, weighted=False, poison=float("nan")):
    """one backward launch of `mode` through the C ABI with scratch and grads filled with `poison`; also the forward.  Output buffers
    are guarded"""
    lib, dev = _lib.load(), inp["x"].device
    rows, n, nb, formed = inp["rows"], inp["n"], inp["nb"], inp["pern"] is not None
    prm = [dict(cr.named_parameters())[k].detach().contiguous().reshape(-1) for k in HEAD_PARAMS]
    pp = [t.data_ptr() for t in prm]
    pn = inp["pern"].data_ptr() if formed else None
    eps, st = float(cr.layernorm.eps), torch.cuda.current_stream(dev).cuda_stream
    out = {}
    vb, v = _guarded(rows, 0, dev)
    assert lib.mapdn_critic_head_forward(inp["x"].data_ptr(), pn, n, pp[0], pp[1], eps, pp[2], pp[3], pp[4], pp[5], v.data_ptr(), rows, st) == 0
    torch.cuda.synchronize()
    assert _guards_intact(vb, rows)
    out["v"] = v
    ng = lm.HP + (n * 64 if formed else 0)
    gb, grads = _guarded(ng, 0, dev)
    grads.fill_(poison)
    ns = max(1, lib.mapdn_critic_head_scratch_floats(rows, n, int(formed)))
    sb, scratch = _guarded(ns, 0, dev)
    scratch.fill_(poison)
    if mode == 2:
        ab, dact = _guarded(rows, 0, dev)
        rc = lib.mapdn_critic_head_backward_dot(inp["dv"].data_ptr(), inp["x"].data_ptr(), pn, n, pp[0], pp[1], eps, pp[2], pp[3], pp[4], pp[5],
                                                inp["dot_w"].data_ptr(), dact.data_ptr(), rows, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert _guards_intact(ab, rows)
        out["dact"] = dact
        return out
    xb, dx = _guarded(nb, 64, dev)
    if mode == 3:
        wr = None
        if weighted:
            wr = inp["wrow"]
            out["scale"] = (1.0 / (wr.sum().clamp(min=1.0) * n)).reshape(1)
        else:
            out["scale"] = torch.full((1,), 1.0 / rows, device=dev)
        rc = lib.mapdn_critic_head_mse(inp["dv"].data_ptr(), wr.data_ptr() if wr is not None else None, out["scale"].data_ptr(), inp["x"].data_ptr(), pn, n,
                                       pp[0], pp[1], eps, pp[2], pp[3], pp[4], pp[5], dx.data_ptr(), grads.data_ptr(), scratch.data_ptr(), rows, st)
    else:
        rc = lib.mapdn_critic_head_backward(inp["dv"].data_ptr(), inp["x"].data_ptr(), pn, n, pp[0], pp[1], eps, pp[2], pp[3], pp[4], pp[5], dx.data_ptr(),
                                            grads.data_ptr(), scratch.data_ptr(), rows, int(mode == 0), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _guards_intact(xb, nb * 64) and _guards_intact(gb, ng) and _guards_intact(sb, ns)
    out.update(dx=dx, grads=grads, scratch=scratch)
    return out


def _check_pads(out, inp, mode, blocks):
    """the pad rule of include/mapdn.h: pad elements of an output are zero, pad columns of scratch are neither read nor written
    (they keep the NaN they were filled with), every documented element is finite"""
    formed, n = inp["pern"] is not None, inp["n"]
    grads, scratch = out["grads"], out["scratch"]
    if mode == 1:
        assert bool(grads[:lm.HP].isnan().all()), "param_grads == 0: only dper_n is written"
    else:
        assert bool(torch.isfinite(grads[:lm.HW]).all()), "a documented element of grads is not finite"
        assert bool((grads[lm.HW:lm.HP] == 0).all()), "the pad of grads is not zero"
    if formed:
        assert bool(torch.isfinite(grads[lm.HP:]).all())
    if mode == 1 and not formed:
        assert bool(scratch.isnan().all())                          # nothing to reduce: untouched
        return
    stride = lm.HP + (n * 64 if formed else 0)
    part = scratch[:blocks * stride].view(blocks, stride)
    assert bool(part[:, lm.HW:lm.HP].isnan().all()), "a pad column of scratch was written"
    if mode != 1:
        assert bool(torch.isfinite(part[:, :lm.HW]).all())
    if formed:
        assert bool(torch.isfinite(part[:, lm.HP:]).all())
    assert bool(scratch[blocks * stride:].isnan().all())


def _check_head(cr, inp, out, mode, weighted=False):
    """against autograd through the float64 modules, with the bars of tests/test_critic_head.py"""
    cr64 = copy.deepcopy(cr).double()
    prm64 = [dict(cr64.named_parameters())[k] for k in HEAD_PARAMS]
    rows, n, nb, formed = inp["rows"], inp["n"], inp["nb"], inp["pern"] is not None
    if formed:                                                        # float64 leaves; the VALUE of a row is the kernel's one f32 add
        base, pern = inp["x"].double().requires_grad_(True), inp["pern"].double().requires_grad_(True)
        x32 = (inp["x"].unsqueeze(1) + inp["pern"].unsqueeze(0)).reshape(rows, 64)
        exact = (base.unsqueeze(1) + pern.unsqueeze(0)).reshape(rows, 64)
        x64 = exact + (x32.double() - exact).detach()
        leaves = [base, pern]
    else:
        x64 = inp["x"].double().requires_grad_(True)
        leaves = [x64]
    x64.retain_grad()
    ref = _head64(cr64, x64)

    def close(a, b, tol, what):
        err, scale = _err(a, b), _scale(b)
        assert err <= tol * scale, (what, mode, err, tol * scale)
    close(out["v"], ref.detach(), 2e-6, "v")
    if mode == 2:
        ref.backward(inp["dv"].double())
        idx = torch.arange(rows, device=x64.device) % n
        close(out["dact"], (x64.grad * inp["dot_w"].double()[idx]).sum(-1), 3e-6, "dact")
        return
    if mode == 3:
        w = torch.full((rows,), 1.0, dtype=torch.float64, device=x64.device) if not weighted else inp["wrow"].double().repeat_interleave(n)
        w = w * out["scale"].double()
        loss = (w * (inp["dv"].double() - ref) ** 2).sum()
        want = torch.autograd.grad(loss, leaves + prm64)
        assert abs(float(out["grads"][4353]) - float(loss)) <= 3e-6 * max(1.0, abs(float(loss))), ("loss", float(out["grads"][4353]), float(loss))
        got = [out["dx"]] + ([out["grads"][lm.HP:].view(n, 64)] if formed else []) + [out["grads"][lo:hi] for lo, hi in GRAD_SLICES]
        for i, (a, b) in enumerate(zip(got, want)):
            err, ref_max = _err(a.reshape(-1), b.reshape(-1)), float(b.abs().max())
            assert err <= 2e-4 * ref_max, ("mse", i, err, ref_max)
        return
    want = torch.autograd.grad(ref, leaves + (prm64 if mode == 0 else []), inp["dv"].double())
    if formed:
        close(out["dx"], want[0], 3e-6, "dbase")
        close(out["grads"][lm.HP:].view(n, 64), want[1], 3e-7 * max(1.0, nb ** 0.5) * 4, "dper_n")
    else:
        close(out["dx"], want[0], 2e-6, "dx")
    if mode == 0:
        assert float(out["grads"][4353]) == 0.0                                   # the loss slot of _mse
        for name, (lo, hi), b in zip(HEAD_PARAMS, GRAD_SLICES, want[len(leaves):]):
            close(out["grads"][lo:hi], b.reshape(-1), 3e-7 * max(1.0, rows ** 0.5), name)


@pytest.mark.parametrize("i", HEAD_IDX, ids=[lm.ROWS[i].label for i in HEAD_IDX])
def test_head_backward_instantiation_against_float64(i, monkeypatch):
    row = _row(i)
    dev = _dev()
    _setenv(monkeypatch, row.env)
    assert lm.reported_kernel(row, cus=0) == row.kernel, (row, lm.reported_kernel(row, cus=0))     # asked of this device, before the launch
    _setenv(monkeypatch, row.env)
    _, bc, mode, nt = row.kernel
    cr = _critic(dev, i)
    inp = _off_the_kinks(cr, _head_inputs(row.shape, 31 * i + 7, dev), i)
    blocks = _lib.critic_head_backward_geometry(inp["rows"], inp["n"], bool(bc), mode, 0)[1]
    for weighted in ((False, True) if mode == 3 else (False,)):
        out = _run_head(cr, inp, mode, weighted)
        again = _run_head(cr, inp, mode, weighted)
        for k in out:
            if k != "scratch":                                      # deterministic: a second launch gives the same bits
                a, b = out[k], again[k]
                assert torch.equal(a.nan_to_num(nan=1.5), b.nan_to_num(nan=1.5)), k
        if mode != 2:
            _check_pads(out, inp, mode, blocks)
        _check_head(cr, inp, out, mode, weighted)


PAIR_SHAPES = [dict(rows=4101), dict(rows=40), dict(nb=333, n=6), dict(nb=27, n=38), dict(nb=203, n=1)]


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=lambda s: "-".join(f"{k}{v}" for k, v in s.items()))
def test_head_backward_256_and_512_threads_agree(shape, mode, monkeypatch):
    """the two builds of one shape: per-row arithmetic does not depend on the launch shape (as tests/test_critic_head.py asserts between
    a batch and its halves), so row-local outputs (dx, dbase, dact) are bit-identical; reduced gradients agree to f32 summation order"""
    dev = _dev()
    cr = _critic(dev, 5)
    inp = _off_the_kinks(cr, _head_inputs(shape, 99, dev), 99)
    outs = {}
    for nt in (256, 512):
        _setenv(monkeypatch, {"MAPDN_HEAD_BWD_THREADS": str(nt)})
        assert _lib.critic_head_backward_geometry(inp["rows"], inp["n"], "nb" in shape, mode, 0)[0] == nt
        outs[nt] = _run_head(cr, inp, mode)
    a, b = outs[256], outs[512]
    if mode == 2:
        assert torch.equal(a["dact"], b["dact"])
        return
    assert torch.equal(a["dx"], b["dx"])
    rows = inp["rows"]
    if "nb" in shape:
        ref = a["grads"][lm.HP:].double()
        assert _err(b["grads"][lm.HP:], ref) <= 2 * 3e-7 * max(1.0, inp["nb"] ** 0.5) * 4 * _scale(ref)
    if mode != 1:
        for lo, hi in GRAD_SLICES:
            ref = a["grads"][lo:hi].double()
            assert _err(b["grads"][lo:hi], ref) <= 2 * 3e-7 * max(1.0, rows ** 0.5) * _scale(ref), (lo, _err(b["grads"][lo:hi], ref))


@pytest.mark.parametrize("shape", [dict(rows=4101), dict(nb=333, n=6), dict(nb=35, n=88)], ids=["read", "formed-n6", "formed-n88"])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_head_poisoned_scratch(shape, mode, monkeypatch):
    """scratch and grads filled with NaN before the launch: every documented element is finite and has the bits of a launch on zeroed
    buffers, the pads follow the rule of include/mapdn.h"""
    dev = _dev()
    _setenv(monkeypatch, {})
    cr = _critic(dev, 9)
    inp = _off_the_kinks(cr, _head_inputs(shape, 123, dev), 123)
    blocks = _lib.critic_head_backward_geometry(inp["rows"], inp["n"], "nb" in shape, mode, 0)[1]
    out = _run_head(cr, inp, mode, poison=float("nan"))
    clean = _run_head(cr, inp, mode, poison=0.0)
    _check_pads(out, inp, mode, blocks)
    _check_head(cr, inp, out, mode)
    assert torch.equal(out["dx"], clean["dx"])
    if mode != 1:
        assert torch.equal(out["grads"][:lm.HP], clean["grads"][:lm.HP])
    assert torch.equal(out["grads"][lm.HP:], clean["grads"][lm.HP:])


# ================================================================================================================================
# policy backward, LayerNorm, relu-dot, head forward
# ================================================================================================================================
def _run_policy_bwd(ag, x1, hid, dm, poison):
    lib, dev = _lib.load(), x1.device
    rows = x1.shape[0]
    bufs = {k: _guarded(rows, w, dev) for k, w in (("dx1", 64), ("dG", 256), ("xn", 64))}
    sb, small = _guarded(lm.PBP, 0, dev)
    small.fill_(poison)
    ns = max(1, lib.mapdn_policy_backward_scratch_floats(rows))
    cb, scratch = _guarded(ns, 0, dev)
    scratch.fill_(poison)
    p = [t.detach().contiguous() for t in (ag.layernorm.weight, ag.layernorm.bias, ag.rnn.weight_ih, ag.rnn.weight_hh, ag.rnn.bias_ih, ag.rnn.bias_hh,
                                           ag.fc2.weight)]
    rc = lib.mapdn_policy_backward(dm.data_ptr(), x1.data_ptr(), hid.data_ptr(), p[0].data_ptr(), p[1].data_ptr(), float(ag.layernorm.eps),
                                   *(t.data_ptr() for t in p[2:]), bufs["dx1"][1].data_ptr(), bufs["dG"][1].data_ptr(), bufs["xn"][1].data_ptr(),
                                   small.data_ptr(), scratch.data_ptr(), rows, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for k, w in (("dx1", 64), ("dG", 256), ("xn", 64)):
        assert _guards_intact(bufs[k][0], rows * w), k
    assert _guards_intact(sb, lm.PBP) and _guards_intact(cb, ns)
    return dict(dx1=bufs["dx1"][1], dG=bufs["dG"][1], xn=bufs["xn"][1], small=small, scratch=scratch)


def _check_policy_bwd(ag, x1, hid, dm, out):
    """against autograd through the float64 modules.  Row-local tensors (xn, dx1) and the weight gradients formed from dgates as the
    learner forms them: the bars of tests/test_policy_trunk.py (means 5e-6; parameter gradients 4e-7 sqrt(rows) max(scale, 1) + 2e-5 scale)"""
    rows = x1.shape[0]
    ag64 = copy.deepcopy(ag).double()
    x = x1.double().requires_grad_(True)
    xn = torch.relu(ag64.layernorm(x))
    xn.retain_grad()
    means = ag64.fc2(ag64.rnn(xn, hid.double())).reshape(rows)
    means.backward(dm.double())
    assert _err(out["xn"], xn.detach()) <= 2e-6 * _scale(xn.detach())
    assert _err(out["dx1"], x.grad) <= MEANS_BAR * _scale(x.grad), (_err(out["dx1"], x.grad), _scale(x.grad))
    s, dG = out["small"].double(), out["dG"].double()

    def pg(a, w, name):
        err, scale = _err(a.reshape(-1), w.reshape(-1)), max(1e-3, float(w.abs().max()))
        assert err <= 4e-7 * max(1.0, rows ** 0.5) * max(scale, 1.0) + 2e-5 * scale, (name, err, scale)
    pg(s[:192], ag64.rnn.bias_ih.grad, "b_ih")
    pg(torch.cat((s[:128], s[192:256])), ag64.rnn.bias_hh.grad, "b_hh")
    pg(s[256:320], ag64.layernorm.weight.grad, "dgamma"); pg(s[320:384], ag64.layernorm.bias.grad, "dbeta")
    pg(s[384:448], ag64.fc2.weight.grad, "dw2"); pg(s[448:449], ag64.fc2.bias.grad, "db2")
    pg(dG[:, :192].t() @ out["xn"].double(), ag64.rnn.weight_ih.grad, "dW_ih")
    pg(torch.cat((dG[:, :128], dG[:, 192:]), 1).t() @ hid.double(), ag64.rnn.weight_hh.grad, "dW_hh")


def _check_policy_bwd_pads(out, rows):
    small, scratch = out["small"], out["scratch"]
    assert bool(torch.isfinite(small[:lm.PBW]).all()) and bool((small[lm.PBW:] == 0).all()), "small: documented finite, pad zero"
    blocks = scratch.numel() // lm.PBP
    part = scratch.view(blocks, lm.PBP)
    assert bool(torch.isfinite(part[:, :lm.PBW]).all()) and bool(part[:, lm.PBW:].isnan().all()), "scratch: pad columns neither read nor written"


def _policy_bwd_case(rows, seed, dev):
    ag, _ = _agent(5, 3, seed, dev)
    g = torch.Generator(device="cpu").manual_seed(seed)
    return ag, (1.5 * torch.randn(rows, 64, generator=g) + 0.2).to(dev), (0.5 * torch.randn(rows, 64, generator=g)).to(dev), torch.randn(rows, generator=g).to(dev)


def _f64(fn, *leaves):
    ls = [t.double().requires_grad_(True) for t in leaves]
    return fn(*ls), ls


@pytest.mark.parametrize("i", OTHER_IDX, ids=[lm.ROWS[i].label for i in OTHER_IDX])
def test_other_learner_kernels_against_float64(i, monkeypatch):
    row = _row(i)
    dev, lib = _dev(), _lib.load()
    _setenv(monkeypatch, row.env)
    assert lm.reported_kernel(row, cus=0) == row.kernel
    kind, shape = row.kernel[0], row.shape
    st = torch.cuda.current_stream(dev).cuda_stream
    if kind == "policy_bwd":
        ag, x1, hid, dm = _policy_bwd_case(shape["rows"], i, dev)
        out = _run_policy_bwd(ag, x1, hid, dm, float("nan"))
        again = _run_policy_bwd(ag, x1, hid, dm, float("nan"))
        assert all(torch.equal(out[k], again[k]) for k in ("dx1", "dG", "xn", "small"))
        _check_policy_bwd_pads(out, shape["rows"])
        _check_policy_bwd(ag, x1, hid, dm, out)
        return
    inp = _head_inputs(shape, 17 * i + 3, dev)
    rows, n, formed = inp["rows"], inp["n"], inp["pern"] is not None
    cr = _critic(dev, i)
    if kind == "head_fwd":
        out = _run_head(cr, inp, 2)
        x = (inp["x"].unsqueeze(1) + inp["pern"].unsqueeze(0)).reshape(rows, 64) if formed else inp["x"]
        ref = _head64(copy.deepcopy(cr).double(), x.double()).detach()
        assert _err(out["v"], ref) <= 2e-6 * _scale(ref)
        return
    gam, bet = cr.layernorm.weight.detach().contiguous(), cr.layernorm.bias.detach().contiguous()
    x = (inp["x"].unsqueeze(1) + inp["pern"].unsqueeze(0)).reshape(rows, 64).contiguous() if formed else inp["x"]
    pg_bar = 3e-7 * max(1.0, rows ** 0.5)
    nblk = lib.mapdn_layernorm64_backward_blocks(rows)
    pb, partial = _guarded(nblk * 128, 0, dev)
    partial.fill_(float("nan"))
    if kind.startswith("ln64"):
        relu = row.kernel[1]
        yb, y = _guarded(rows, 64, dev)
        mb, mean = _guarded(rows, 0, dev)
        rb, rstd = _guarded(rows, 0, dev)
        if formed:
            rc = lib.mapdn_layernorm64_bc_forward(inp["x"].data_ptr(), inp["pern"].data_ptr(), n, gam.data_ptr(), bet.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                                  rstd.data_ptr(), rows, 1e-5, relu, st)
        else:
            rc = lib.mapdn_layernorm64_forward(x.data_ptr(), gam.data_ptr(), bet.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, 1e-5, relu, st)
        assert rc == 0
        torch.cuda.synchronize()
        assert _guards_intact(yb, rows * 64) and _guards_intact(mb, rows) and _guards_intact(rb, rows)
        (ref, (x64, g64, b64)) = _f64(lambda a, g_, b_: (torch.relu if relu else (lambda t: t))(F.layer_norm(a, (64,), g_, b_, 1e-5)), x, gam, bet)
        assert _err(y, ref.detach()) <= 2e-6 * _scale(ref.detach())
        mu = x64.detach().mean(-1)
        rs = (x64.detach().var(-1, unbiased=False) + 1e-5).rsqrt()
        assert _err(mean, mu) <= 2e-6 * _scale(mu) and _err(rstd, rs) <= 2e-6 * _scale(rs)
        if kind == "ln64_bwd":
            dy = torch.randn(rows, 64, generator=torch.Generator(device="cpu").manual_seed(i)).to(dev)
            want = torch.autograd.grad(ref, [x64, g64, b64], dy.double())
            db_, dx = _guarded(rows, 64, dev)
            dgb, dgam = _guarded(64, 0, dev)
            dbb, dbet = _guarded(64, 0, dev)
            if formed:
                rc = lib.mapdn_layernorm64_bc_backward(dy.data_ptr(), inp["x"].data_ptr(), inp["pern"].data_ptr(), n, gam.data_ptr(), bet.data_ptr(),
                                                       mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), partial.data_ptr(),
                                                       rows, relu, st)
            else:
                rc = lib.mapdn_layernorm64_backward(dy.data_ptr(), x.data_ptr(), gam.data_ptr(), bet.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                                    dgam.data_ptr(), dbet.data_ptr(), partial.data_ptr(), rows, relu, st)
            assert rc == 0
            torch.cuda.synchronize()
            assert _guards_intact(db_, rows * 64) and _guards_intact(dgb, 64) and _guards_intact(dbb, 64) and _guards_intact(pb, nblk * 128)
            assert _err(dx, want[0]) <= 2e-6 * _scale(want[0])
            assert _err(dgam, want[1]) <= pg_bar * _scale(want[1]) and _err(dbet, want[2]) <= pg_bar * _scale(want[2])
        return
    # relu_dot64: v = relu(pre) . w + b
    w = cr.fc3.weight.detach().reshape(64).contiguous()
    vb, v = _guarded(rows, 0, dev)
    assert lib.mapdn_relu_dot64_forward(x.data_ptr(), w.data_ptr(), 0.25, v.data_ptr(), rows, st) == 0
    torch.cuda.synchronize()
    assert _guards_intact(vb, rows)
    (ref, (x64, w64)) = _f64(lambda a, w_: torch.relu(a) @ w_ + 0.25, x, w)
    assert _err(v, ref.detach()) <= 2e-6 * _scale(ref.detach())
    if kind == "relu_dot64_bwd":
        want = torch.autograd.grad(ref, [x64, w64], inp["dv"].double())
        db_, dpre = _guarded(rows, 64, dev)
        dwb, dw = _guarded(64, 0, dev)
        dbb, dbias = _guarded(64, 0, dev)
        assert lib.mapdn_relu_dot64_backward(inp["dv"].data_ptr(), x.data_ptr(), w.data_ptr(), dpre.data_ptr(), dw.data_ptr(), dbias.data_ptr(),
                                             partial.data_ptr(), rows, st) == 0
        torch.cuda.synchronize()
        assert _guards_intact(db_, rows * 64) and _guards_intact(dwb, 64) and _guards_intact(dbb, 64) and _guards_intact(pb, nblk * 128)
        assert _err(dpre, want[0]) <= 2e-6 * _scale(want[0]) and _err(dw, want[1]) <= pg_bar * _scale(want[1])
        sdv = inp["dv"].double().sum()
        assert abs(float(dbias[0]) - float(sdv)) <= pg_bar * max(1.0, abs(float(sdv))) and bool((dbias[1:] == 0).all())


@pytest.mark.parametrize("rows", [1, 4101, 70000])
def test_policy_backward_poisoned_scratch(rows):
    """scratch and `small` filled with NaN before the launch: small[0:449] finite, within its bars and bit-identical to a launch on zeroed
    buffers; small[449:512] zero; the pad columns of scratch untouched"""
    dev = _dev()
    ag, x1, hid, dm = _policy_bwd_case(rows, rows, dev)
    out = _run_policy_bwd(ag, x1, hid, dm, float("nan"))
    clean = _run_policy_bwd(ag, x1, hid, dm, 0.0)
    _check_policy_bwd_pads(out, rows)
    _check_policy_bwd(ag, x1, hid, dm, out)
    assert all(torch.equal(out[k], clean[k]) for k in ("dx1", "dG", "xn", "small"))
