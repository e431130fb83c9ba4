"""Workload for timing the res_line / res_trafo launches: case141 x 4096 envs, every line rated, then `--reps` rounds of
all ten line columns (k_branch_results), the loading summary (k_loading_summary) and get_obs (k_gather, the yardstick for a byte-bound wide
launch on this layout).  Run it under `rocprofv3 --kernel-trace --stats -- python tools/branch_profile.py`; `--summarise TRACE.csv` prints
the median time of the three kernels from the kernel trace, with their algorithmic bytes and GB/s.

    rocprofv3 --kernel-trace --stats -d out -o branch -- python tools/branch_profile.py --reps 200
    python tools/branch_profile.py --summarise out/branch_kernel_trace.csv
"""
from __future__ import annotations

import argparse
import csv
import dataclasses
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASE, B = "case141", 4096


def algorithmic_bytes(n_bus, n_line, n_obs_cols, n_env):
    """what each launch has to move at least: the voltage rows once in, the requested columns once out (f64; obs f32)"""
    volt = 2 * n_bus * n_env * 8
    return dict(k_branch_results=volt + 10 * n_line * n_env * 8, k_loading_summary=volt + n_env * 16, k_gather=None if n_obs_cols is None else n_obs_cols * n_env * (8 + 4))


def summarise(path, n_bus, n_line, n_obs_cols):
    rows = list(csv.DictReader(open(path)))
    name_key = next(k for k in rows[0] if k.lower().replace("_", "") == "kernelname")
    start = next(k for k in rows[0] if k.lower().replace("_", "") in ("starttimestamp", "start"))
    end = next(k for k in rows[0] if k.lower().replace("_", "") in ("endtimestamp", "end"))
    by = algorithmic_bytes(n_bus, n_line, n_obs_cols, B)
    for kern in ("k_branch_results", "k_loading_summary", "k_gather"):
        ns = [int(r[end]) - int(r[start]) for r in rows if kern in r[name_key]]
        if not ns:
            print(f"{kern}: not in the trace")
            continue
        med = statistics.median(ns)
        line = f"{kern:20s} launches {len(ns):5d}  median {med / 1e3:8.2f} us  min {min(ns) / 1e3:8.2f} us"
        if by[kern]:
            line += f"  algorithmic {by[kern] / 1e6:7.2f} MB  {by[kern] / med:7.1f} GB/s"
        print(line)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--summarise", default=None, help="a rocprofv3 kernel trace CSV of this workload")
    a = ap.parse_args()
    import numpy as np
    from mapdn_amd.netspec import make_case
    net, prof = make_case(CASE)
    n_obs = int(net.n_sgen * net.obs_size())
    if a.summarise:
        return summarise(a.summarise, net.n_bus, net.n_line, n_obs)
    import torch
    from mapdn_amd.env import VoltageControlBatch
    net = dataclasses.replace(net, line_max_i_ka=np.full(net.n_line, 0.4))
    env = VoltageControlBatch(net, prof, dict(episode_limit=240, action_scale=0.8, action_bias=0.0, seed=0), n_envs=B, device="cuda:0")
    env.reset()
    for _ in range(a.reps):
        env.res_line(_ALL)
        env.loading_summary(100.0)
        env.get_obs()
    torch.cuda.synchronize()
    env.close()
    print("done", a.reps)


_ALL = ("p_from_mw", "q_from_mvar", "p_to_mw", "q_to_mvar", "pl_mw", "ql_mvar", "i_from_ka", "i_to_ka", "i_ka", "loading_percent")

if __name__ == "__main__":
    main()
