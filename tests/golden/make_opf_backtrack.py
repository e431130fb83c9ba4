"""Searches for honest states on which the OPF loop backtracks, and writes those it keeps to tests/golden/opf_backtrack.npz.

k_opf_update retries a trial point whose power flow failed at half the step (opf_decide: OPF_GO_RETRY) and gives up with status 2 after
max_backtrack failures in a row.  Where that can happen: a small radial feeder (tests/opf_kernel_cases.backtrack_net) whose loads are
scaled towards voltage collapse, still solvable at a = 0, with a voltage band far below the feeder's voltages, so that the first QP asks
every inverter to absorb all the reactive power it can — and the power flow at that set-point has no solution.

The search, bounded: NETS seeded feeders x the night row (no PV: every inverter has its whole rating for reactive power) x FRACTIONS of
the collapse scale (found by bisection on the oracle's power flow at a = 0) x BANDS.  Every trial is the restated loop
(tests/opf_ref.opf_ref on the oracle) with its decisions logged, in the band and otherwise the default config.  Left alone such a
loop creeps towards the collapse point, retry after retry, and its power flows come to need all 10 Newton iterations: no state to
pin a kernel to.  So a trial is kept as two runs that stop early: "retry", max_iter = M, the iteration of the first power flow that
solves again after a failure, which ends there with status 1 after at least one OPF_GO_RETRY; and "mb1", max_backtrack = 1, which ends
with status 2 at the second failure in a row.  Both must be away from a threshold: with the loads moved by +-1e-6 and by +-1e-3
relative, every power flow that failed still fails and every one that solved still solves (the same sequence of decisions, the same
status and iteration count), and every solved power flow took at most MAX_NR of the 10 Newton iterations.

    python tests/golden/make_opf_backtrack.py        (the tests only read the npz)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle.pp_restated import runpp_restated                  # noqa: E402
from tests import opf_kernel_cases as K                         # noqa: E402
from tests import opf_ref as R                                  # noqa: E402

NETS = (0, 1, 2)
FRACTIONS = (0.60, 0.80, 0.90)
BANDS = ((0.30, 0.60), (0.30, 0.75), (0.50, 0.90), (0.50, 0.97))  # (v_lower, v_upper) as fractions of the lowest |V| at a = 0
MAX_NR = 7
KEEP = 4


def collapse_scale(net, lp, lq, pv):
    """the largest load scale (to 1e-3) at which the oracle's power flow at a = 0 converges"""
    ok = lambda k: runpp_restated(net, k * lp, k * lq, pv, np.zeros(net.n_sgen)).converged
    lo, hi = 1.0, 2.0
    while ok(hi):
        lo, hi = hi, 2.0 * hi
    while hi - lo > 1e-3 * lo:
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


def run(net, lp, lq, pv, smax, cfg):
    log, nr = [], []

    def runpp(*a, **k):
        r = runpp_restated(*a, **k)
        nr.append(int(r.iterations) if r.converged else -1)
        return r
    r = R.opf_ref(net, lp, lq, pv, smax, cfg, 0.95, 1.05, runpp=runpp, decisions=log)
    return r, log, nr


def path(log):
    return [(d["iter"], d["solved"], d["capped"], d["nback_after"]) for d in log]


def main():
    t0 = time.time()
    found, trials = [], 0
    for ni in NETS:
        net, prof = K.backtrack_net(ni)
        smax = prof.s_max(1.2)
        t = 0                                                   # midnight: no PV
        lp0, lq0, pv = prof.load_p[t], prof.load_q[t], prof.pv[t]
        kc = collapse_scale(net, lp0, lq0, pv)
        for frac in FRACTIONS:
            k = frac * kc
            lp, lq = k * lp0, k * lq0
            vmin = float(np.abs(runpp_restated(net, lp, lq, pv, np.zeros(net.n_sgen)).V).min())
            for bl, bu in BANDS:
                trials += 1
                cfg = dict(v_lower=bl * vmin, v_upper=bu * vmin)
                _, log0, _ = run(net, lp, lq, pv, smax, cfg)
                back = [i for i in range(1, len(log0)) if log0[i]["solved"] == 1 and log0[i - 1]["solved"] == 0]
                print(f"net {ni} scale {k:.4f} ({frac} of {kc:.4f}) vmin {vmin:.4f} band {bl, bu}: the default loop: "
                      f"{[d['solved'] for d in log0]}")
                if not back:
                    continue
                cfg0 = dict(cfg, max_iter=log0[back[0]]["iter"])
                cfg1 = dict(cfg, max_backtrack=1)
                r, log, nr = run(net, lp, lq, pv, smax, cfg0)
                r1, log1, nr1 = run(net, lp, lq, pv, smax, cfg1)
                print(f"    retry (max_iter {cfg0['max_iter']}): status {r.status} iterations {r.iterations} NR {nr} | mb1: status {r1.status} "
                      f"iterations {r1.iterations} NR {nr1}")
                if not (r.status == 1 and any(d["solved"] == 0 for d in log) and r1.status == 2 and r1.iterations >= 2):
                    continue
                if max(nr + nr1) > MAX_NR:
                    print("    dropped: a solved power flow needed more than", MAX_NR, "Newton iterations")
                    continue
                stable = True
                for eps in (1e-6, -1e-6, 1e-3, -1e-3):
                    p, l, _ = run(net, lp * (1 + eps), lq * (1 + eps), pv, smax, cfg0)
                    p1, l1, _ = run(net, lp * (1 + eps), lq * (1 + eps), pv, smax, cfg1)
                    stable &= path(l) == path(log) and p.status == r.status and path(l1) == path(log1) and p1.status == r1.status
                if not stable:
                    print("    dropped: the decisions change when the loads move by 1e-6 or 1e-3")
                    continue
                found.append(dict(net=ni, scale=k, lp=lp, lq=lq, pv=pv, cfg=cfg0, r=r, log=log, r1=r1, log1=log1))
                print("    kept")
    print(f"{trials} trials, {len(found)} kept, {time.time() - t0:.0f} s")
    found = found[::max(1, len(found) // KEEP)][:KEEP]           # spread over the nets and scales
    out = dict(n=np.array(len(found)))
    keys = ("iter", "solved", "dn", "viol", "prev_viol", "capped", "t_after", "nback_after")
    for i, f in enumerate(found):
        p = f"s{i}_"
        out.update({p + "net": np.array(f["net"]), p + "scale": np.array(f["scale"]), p + "load_p": f["lp"], p + "load_q": f["lq"], p + "pv": f["pv"],
                    p + "band": np.array([f["cfg"]["v_lower"], f["cfg"]["v_upper"]]), p + "max_iter": np.array(f["cfg"]["max_iter"])})
        for tag, r, log in (("retry_", f["r"], f["log"]), ("mb1_", f["r1"], f["log1"])):
            out.update({p + tag + "a": r.actions, p + tag + "status": np.array(r.status), p + tag + "iterations": np.array(r.iterations),
                        p + tag + "loss_mw": np.array(r.loss_mw), p + tag + "violation": np.array(r.violation),
                        p + tag + "decisions": np.array([[float(d[k]) for k in keys] for d in log])})
    out["decision_keys"] = np.array(keys)
    if found:
        np.savez_compressed(os.path.join(ROOT, "tests", "golden", "opf_backtrack.npz"), **out)
        print("wrote tests/golden/opf_backtrack.npz")


if __name__ == "__main__":
    main()
