"""What tests/test_rollout_glue_cpu.py and tests/test_rollout_glue_gpu.py share: the kernels csrc/rollout.hip defines (parsed, comments
stripped), and a scripted env for BatchedRollout — no power flow, it plays back seeded [T, B] reward / info / done tensors — with the
float64 host reference of the logged means computed from the script alone."""
import math
import os
import re
import types

import torch

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mapdn_amd", "csrc")
KERNELS = {"k_explore", "k_rollout_stats", "k_copy_segments"}          # every one has its tests in tests/test_rollout_glue_gpu.py

MAPDN_OK, MAPDN_E_INVALID = 0, -1


def _read(name="rollout.hip"):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def global_kernels():
    """the names of the __global__ functions of rollout.hip, comments stripped (a list, so that a name defined twice shows)"""
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", _read(), flags=re.S))
    assert src.count("__global__") == len(re.findall(r"__global__\s+void\b", src)), "a __global__ this parser does not read"
    return re.findall(r"__global__\s+void\s+(?:__launch_bounds__\s*\([^)]*\)\s*)?(\w+)\s*\(", src)


# ---- the scripted env -------------------------------------------------------------------------------------------------------------
N_ENVS, N_AGENTS, OBS, T_SCRIPT = 70, 3, 5, 64


def make_script(seed=0):
    """seeded on the CPU: reward [T, B] f64, info [T, B, 11] f64 (zeros once an env is frozen), done [T, B] bool, obs [T + 1, B, n, o] f32.
    Env e terminates at step die[e], spread over 3 .. 37.  An even env keeps reporting done while frozen, an odd one reports it once — the
    live mask has to be alive & ~done, not ~done.  The reward of a frozen env is NOT zero: only the mask keeps it out of the means."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    B, T = N_ENVS, T_SCRIPT
    die = 3 + (torch.arange(B) * 11) % 35
    assert int(die.min()) == 3 and int(die.max()) == 37
    t = torch.arange(T).unsqueeze(1)
    live = t <= die.unsqueeze(0)                                       # [T, B]: the mask BEFORE step t
    done = torch.where(torch.arange(B) % 2 == 0, t >= die.unsqueeze(0), t == die.unsqueeze(0))
    reward = torch.randn(T, B, generator=g, dtype=torch.float64) - 0.5
    info = (torch.randn(T, B, 11, generator=g, dtype=torch.float64) + torch.arange(11, dtype=torch.float64)) * live.unsqueeze(-1)
    obs = torch.randn(T + 1, B, N_AGENTS, OBS, generator=g)
    return types.SimpleNamespace(die=die, live=live, done=done, reward=reward, info=info, obs=obs)


class ScriptedEnv:
    """the members BatchedRollout reads; copy = True: every tensor handed out is fresh"""
    n_envs, n_agents, obs_size, copy = N_ENVS, N_AGENTS, OBS, True

    def __init__(self, script, device):
        self.device = torch.device(device)
        self.args = dict(action_scale=0.8, action_bias=0.0)
        self.s = types.SimpleNamespace(**{k: v.to(self.device) for k, v in vars(script).items()})
        self.t = 0
        self.actions = []

    def reset(self):
        self.t = 0
        self.actions = []
        return self.s.obs[0].clone(), None

    def step(self, actual):
        assert actual.shape == (self.n_envs, self.n_agents)
        self.actions.append(actual.clone())
        t = self.t
        self.t += 1
        return self.s.reward[t].clone(), self.s.done[t].clone(), self.s.info[t].clone()

    def get_obs(self):
        return self.s.obs[self.t].clone()


def script_steps(max_steps):
    """the number of steps run() takes: through the first t with t % 16 == 15 at which no env is alive (all are dead after step 37)"""
    return min(max_steps, 48)


def reference_stat(script, steps, prefix="mean_train_"):
    """float64 host means over the live (step, env) pairs of the script (math.fsum: exactly rounded sums)"""
    from mapdn_amd._lib import INFO_KEYS
    live = script.live[:steps]
    count = int(live.sum())
    out = {}
    for k, key in enumerate(INFO_KEYS):
        out[prefix + key] = math.fsum(script.info[:steps, :, k][live].tolist()) / count
    out[prefix + "reward"] = math.fsum(script.reward[:steps][live].tolist()) / count
    return out


def run_scripted(script, device, max_steps):
    """one BatchedRollout.run() on the scripted env: (stat, the `alive` every on_step saw (cloned, on the CPU), steps on_step saw, win.steps)"""
    from mapdn_amd.rollout import BatchedRollout
    env = ScriptedEnv(script, device)
    seen = []

    def policy(obs, hidden):
        return torch.tanh(obs.sum(-1)), hidden

    def on_step(t, obs, action, reward, done, info, nxt, alive, aux):
        assert t == len(seen)
        seen.append(alive.clone().cpu())

    ro = BatchedRollout(env, policy, max_steps=max_steps, on_step=on_step, store_window=True)
    win, stat = ro.run()
    return stat, seen, len(seen), win.steps


def check_scripted(script, max_steps, stat, seen, n_seen, win_steps):
    steps = script_steps(max_steps)
    assert n_seen == steps and win_steps == steps, (n_seen, win_steps, steps)
    ref = reference_stat(script, steps)
    assert stat.keys() == ref.keys()
    for k, v in ref.items():
        assert abs(stat[k] - v) <= 1e-12 * max(1.0, abs(v)), (k, stat[k], v)
    for t, a in enumerate(seen):
        assert a.dtype == torch.bool and torch.equal(a, script.live[t]), t
