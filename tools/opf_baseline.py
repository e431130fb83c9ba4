"""The OPF baseline vs no control on the MAPDN feeders: the paper's second traditional baseline, batched on the GPU.

For each case it runs BaselineTester.batch_run (the format of PGTester.batch_run: noisy seeded starts, noise-free steps) with
OPFControl and with NoControl over N episodes of --steps steps and prints
  CR / QL / PL   the means of totally_controllable_ratio, q_loss and total_line_loss (the paper's columns),
  solves / step  the OPF's power flows per env step: mean, p99, max; the share of env steps with status 0 (converged and feasible),
                 1 (max_iter or a QP cap) and 2 (a power flow failed),
  ms / call      the wall time of one opf_actions call on the whole batch (mean over the steps),
  wall time, env-steps/s and power flows/s (the OPF's solves plus the step's own).

    python tools/opf_baseline.py --cases case33 case141 case322 --episodes 4096 --steps 8 --json out.json
    python tools/opf_baseline.py --cases case33 --ties 5          # the feeder with five tie lines closed (OPFConfig(meshed=1))
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mapdn_amd.baselines import BaselineTester, NoControl, OPFConfig, OPFControl   # noqa: E402
from mapdn_amd.env import VoltageControlBatch                                     # noqa: E402
from mapdn_amd import netspec                                                     # noqa: E402
from mapdn_amd.netspec import make_case                                           # noqa: E402

ARGS = dict(episode_limit=240, action_scale=0.8, action_bias=0.0, voltage_barrier_type="bowl")


class TimedOPF(OPFControl):
    """OPFControl that also records the wall time of every call (synchronised)"""

    def __init__(self, config):
        super().__init__(config, keep_history=True)
        self.call_s = []

    def actions(self, env):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a = super().actions(env)
        torch.cuda.synchronize()
        self.call_s.append(time.perf_counter() - t0)
        return a


def run_case(case, episodes, steps, seed, cfg, device, controllers=("opf", "no_control"), loading=False, max_i_ka=None, ties=0):
    net, prof = make_case(case)
    if ties:                                                   # netspec.case33_meshed and its like: both controllers run on the meshed net
        close = getattr(netspec, f"{case}_meshed", None)
        if close is None:
            raise SystemExit(f"--ties: netspec has no {case}_meshed")
        net = close(net, ties)
    if max_i_ka is not None:                                   # the built-in cases carry no ratings: one for every line
        net = dataclasses.replace(net, line_max_i_ka=np.full(net.n_line, float(max_i_ka)))
    out = {}
    for ctrl in (TimedOPF(cfg), NoControl()):
        if ctrl.name not in controllers:
            continue
        env = VoltageControlBatch(net, prof, dict(ARGS, seed=seed), n_envs=episodes, device=device)
        try:
            tester = BaselineTester(types.SimpleNamespace(max_steps=steps), ctrl, env, record_loading=loading)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stat = tester.batch_run(episodes)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        finally:
            env.close()
        env_steps = episodes * steps
        r = dict(CR=stat["mean_test_totally_controllable_ratio"][0], QL=stat["mean_test_q_loss"][0],
                 PL=stat["mean_test_total_line_loss"][0], wall_s=wall, env_steps_per_s=env_steps / wall, stat=stat)
        if loading:
            r.update(max_loading_percent=stat["mean_test_max_loading_percent"][0], overloaded_steps_ratio=stat["mean_test_overloaded_steps_ratio"][0])
        flows = env_steps
        if isinstance(ctrl, OPFControl):
            it = torch.stack([h[2] for h in ctrl.history]).cpu().numpy()      # [steps, B]
            st = torch.stack([h[3] for h in ctrl.history]).cpu().numpy()
            viol = torch.stack([h[1] for h in ctrl.history]).cpu().numpy()
            solved = st <= 2
            n = it[solved]
            flows += int(n.sum())
            r.update(solves_mean=float(n.mean()), solves_p99=float(np.percentile(n, 99)), solves_max=int(n.max()),
                     share_status0=float((st == 0).sum() / solved.sum()), share_status1=float((st == 1).sum() / solved.sum()),
                     share_status2=float((st == 2).sum() / solved.sum()), max_violation_status0=float(np.max(viol[st == 0], initial=0.0)),
                     ms_per_call=1e3 * float(np.mean(ctrl.call_s[1:] or ctrl.call_s)), ms_first_call=1e3 * ctrl.call_s[0])
        r["power_flows_per_s"] = flows / wall
        out[ctrl.name] = r
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", nargs="+", default=["case33", "case141", "case322"])
    ap.add_argument("--episodes", type=int, default=4096, help="episodes = envs of the batch (one round)")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--controllers", nargs="+", default=["opf", "no_control"], choices=["opf", "no_control"])
    ap.add_argument("--json", default=None, help="write the results here")
    ap.add_argument("--loading", action="store_true", help="also print the mean of the largest branch loading_percent per step and the "
                    "share of steps with a branch above 100 %% (BaselineTester(record_loading=True); NaN on a net without ratings)")
    ap.add_argument("--max-i-ka", type=float, default=None, help="with --loading: rate every line at this max_i_ka (the built-in cases carry no ratings)")
    ap.add_argument("--ties", type=int, default=0, help="close this many tie lines (cases for which netspec has <case>_meshed: case33) and "
                    "run the OPF with meshed = 1, on the handle's sparse solver")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    cfg = OPFConfig(max_iter=a.max_iter, meshed=1 if a.ties else 0)
    res = dict(config=cfg.as_dict(), episodes=a.episodes, steps=a.steps, seed=a.seed, ties=a.ties, cases={})
    for case in a.cases:
        r = res["cases"][case] = run_case(case, a.episodes, a.steps, a.seed, cfg, a.device, a.controllers, a.loading, a.max_i_ka, a.ties)
        for name, x in r.items():
            line = (f"{case:8s} {name:10s} CR {x['CR']:.4f}  QL {x['QL']:.4f}  PL {x['PL']:.4f}  | {x['wall_s']:.2f} s  "
                    f"{x['env_steps_per_s']:.3e} env-steps/s  {x['power_flows_per_s']:.3e} power flows/s")
            if "solves_mean" in x:
                line += (f"  | solves/step mean {x['solves_mean']:.2f} p99 {x['solves_p99']:.0f} max {x['solves_max']}  "
                         f"status 0 {100 * x['share_status0']:.2f} %  1 {100 * x['share_status1']:.2f} %  2 {100 * x['share_status2']:.2f} %  "
                         f"| {x['ms_per_call']:.1f} ms / call (first {x['ms_first_call']:.1f})")
            if a.loading:
                line += f"  | max loading {x['max_loading_percent']:.2f} %  overloaded steps {100 * x['overloaded_steps_ratio']:.2f} %"
            print(line, flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
