"""`bench.py --dump-outputs DIR`: what the last timed step handed its caller, as .npy files that two builds can be compared on;
`--steps` is the number of timed steps (one block by default), so the dump is the state after exactly --warmup + --steps steps."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _load(d):
    return {os.path.splitext(f)[0]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_float_arrays_whole_when_small(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(1)
    outs = {"reward": rng.normal(size=16), "terminated": rng.integers(0, 2, 16).astype(bool),
            "info": rng.normal(size=(16, 11)), "obs": rng.normal(size=(16, 3, 5)).astype(np.float32)}
    bench.dump_outputs(str(tmp_path / "d"), outs)
    got = _load(str(tmp_path / "d"))
    assert set(got) == {"reward", "terminated", "info", "obs"}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert got["terminated"].dtype == np.float32 and np.array_equal(got["terminated"], outs["terminated"].astype(np.float32))
    for k in ("reward", "info", "obs"):
        assert got[k].dtype == outs[k].dtype and np.array_equal(got[k], outs[k])


def test_dump_keeps_a_fixed_sample_of_envs_under_the_cap(tmp_path):
    bench = _bench()
    n = 1000
    outs = {"reward": np.arange(n, dtype=np.float64), "obs": np.arange(n * 8, dtype=np.float32).reshape(n, 2, 4)}
    cap = 10_000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs, max_bytes=cap)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(v.nbytes for v in a.values()) <= cap
    idx = a["env_index"].astype(np.int64)
    assert idx.dtype == np.int64 and len(idx) > 1 and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(a["reward"], outs["reward"][idx]) and np.array_equal(a["obs"], outs["obs"][idx])
    assert all(np.array_equal(a[k], b[k]) for k in a)                        # the sample is seeded: the same envs every run


def _run(outdir, steps, warmup=3, envs=256):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--envs", str(envs), "--steps", str(steps), "--warmup", str(warmup),
                        "--no-traffic", "--no-cpu-baseline", "--no-other-shapes", "--dump-outputs", outdir],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_dump_is_reproducible_and_is_the_state_after_warmup_plus_steps(tmp_path):
    import torch
    from mapdn_amd.env import VoltageControlBatch
    from mapdn_amd.netspec import make_case
    steps, warmup, B = 7, 3, 256
    j = _run(str(tmp_path / "a"), steps, warmup, B)
    _run(str(tmp_path / "b"), steps, warmup, B)
    assert j["steps"] == steps and j["repeats"] == 1 and j["timed_steps"] == steps
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert set(a) == {"reward", "terminated", "info", "obs"}
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # the same path stepped by hand, warmup + steps times, with bench.py's seeded actions
    dev = torch.device("cuda", 0)
    net, prof = make_case("case141")
    scale = 0.6
    args = dict(episode_limit=240, action_scale=scale, action_bias=0.0, voltage_barrier_type="bowl", seed=0)
    env = VoltageControlBatch(net, prof, args, n_envs=B, device=dev, env_id_offset=0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    acts = torch.empty(min(steps + warmup + 60, 256), B, env.n_sgen, dtype=torch.float32, device=dev).uniform_(-scale, scale, generator=gen)
    env.reset()
    for t in range(warmup + steps):
        reward, term, info = env.step(acts[t])
        obs = env.get_obs()
    want = {"reward": reward, "terminated": term.float(), "info": info, "obs": obs}
    for k, v in want.items():
        assert a[k].shape == tuple(v.shape) and np.array_equal(a[k], v.cpu().numpy()), k
    env.close()
