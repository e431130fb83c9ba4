"""The `args` namespace of an algorithm (args/default.yaml + args/alg_args/*.yaml of the reference), the checks of what each net class
builds, and the batch type.  Only the configurations the reference trains with exist; anything else raises."""

from types import SimpleNamespace
from typing import Dict, Optional

import torch
import torch.nn.functional as F

# args/default.yaml:6-51 merged with args/alg_args/maddpg.yaml (== iddpg.yaml); sample_size: args/alg_args/coma.yaml (read by COMA only)
ALG_DEFAULTS = dict(
    gumbel_softmax=False, epsilon_softmax=False, softmax_eps=None, episodic=False, cuda=True, grad_clip_eps=1.0,
    save_model_freq=40, replay_warmup=0, policy_lrate=1.0e-4, value_lrate=1.0e-4, mixer_lrate=None, target=True,
    target_lr=0.1, entr=1.0e-3, max_steps=240, batch_size=32, replay=True, replay_buffer_size=5.0e3,
    agent_type="rnn", agent_id=True, shared_params=True, layernorm=True, mixer=False, gaussian_policy=False,
    LOG_STD_MIN=0.0, LOG_STD_MAX=0.5, fixed_policy_std=1.0, hid_activation="relu", init_type="normal", init_std=0.1,
    action_enforcebound=True, double_q=True, clip_c=1.0, gamma=0.99, hid_size=64, continuous=True,
    normalize_advantages=False, train_episodes_num=400, behaviour_update_freq=60, target_update_freq=120,
    policy_update_epochs=1, value_update_epochs=10, mixer_update_epochs=None, reward_normalisation=True,
    eval_freq=20, num_eval_episodes=10, sample_size=10,
    attend_heads=1, norm_in=False, soft=True, reward_scale=100,      # args/alg_args/maac.yaml (read by MAAC only)
    lambda_=0.95, eps_clip=0.6, value_loss_coef=2.0,                 # args/alg_args/mappo.yaml == ippo.yaml (read by MAPPO / IPPO only)
    ppo_old_log_prob="reference",    # not a reference key: "reference" = the ratio's old log-probability is the stored ACTION, as
                                     # Model.unpack_data fills it (models/model.py:309); "stored" = the log-probability recorded at rollout time
)
ALG_YAML = {"maac": dict(gaussian_policy=True, action_enforcebound=True),      # what an algorithm's yaml sets beyond the defaults above
            "sqddpg": dict(sample_size=10, action_enforcebound=True),          # args/alg_args/sqddpg.yaml
            "mappo": dict(policy_update_epochs=10, value_update_epochs=10, lambda_=0.95, eps_clip=0.6, value_loss_coef=2.0, reward_normalisation=True,
                          normalize_advantages=True, gaussian_policy=False, action_enforcebound=True, behaviour_update_freq=240,
                          target_update_freq=480)}                             # args/alg_args/mappo.yaml
ALG_YAML["ippo"] = dict(ALG_YAML["mappo"])                                     # args/alg_args/ippo.yaml: the same values

Batch = Dict[str, torch.Tensor]


def make_alg_args(agent_num: int, obs_size: int, action_dim: int = 1, action_scale: float = 0.8,
                  action_bias: float = 0.0, alg: Optional[str] = None, **overrides) -> SimpleNamespace:
    """The `args` namedtuple train.py:64-67 assembles, as a namespace.  alg: the algorithm whose yaml is merged over the defaults before the
    overrides (train.py:60-62) — needed for "maac", whose yaml switches the Gaussian policy head on, and for "mappo" / "ippo", whose
    yaml sets the update schedule, the clip range, lambda_ and normalize_advantages."""
    d = dict(ALG_DEFAULTS)
    unknown = set(overrides) - set(d)
    if unknown:
        raise KeyError(f"unknown algorithm argument(s): {sorted(unknown)}")
    d.update(ALG_YAML.get(alg, {}))
    d.update(overrides)
    d.update(agent_num=int(agent_num), obs_size=int(obs_size), action_dim=int(action_dim),
             action_scale=float(action_scale), action_bias=float(action_bias))
    a = SimpleNamespace(**d)
    check = {"maac": _maac_args_ok, "sqddpg": _sqddpg_args_ok, "mappo": _ppo_args_ok, "ippo": _ppo_args_ok}.get(alg)
    if check is not None:
        check(a)
        return a
    if not a.continuous or a.gaussian_policy or a.mixer or a.episodic or a.agent_type != "rnn":
        raise NotImplementedError("the DDPG-family learners here cover continuous, non-Gaussian, recurrent, "
                                  "transition-update training (args/alg_args/maddpg.yaml, iddpg.yaml)")
    return a


def _maac_args_ok(a) -> None:
    """what MAACNet builds: continuous actions, the Gaussian recurrent agent, one action per agent, at least two agents (with one the
    reference's th.stack([]) over the other agents' keys raises: critics/maac_critic.py:127-128), transition updates, no mixer"""
    if not a.continuous:
        raise NotImplementedError("MAAC: continuous=False (discrete actions) is not built")
    if a.agent_type != "rnn":
        raise NotImplementedError(f"MAAC: agent_type={a.agent_type!r} is not built (only 'rnn': agents/rnn_agent_gaussian.py)")
    if not a.gaussian_policy:
        raise NotImplementedError("MAAC: gaussian_policy=False is not built (models/maac.py always constructs the Gaussian agent)")
    if a.action_dim != 1:
        raise NotImplementedError(f"MAAC: action_dim={a.action_dim} is not built (one action per agent)")
    if a.agent_num < 2:
        raise ValueError(f"MAAC: agent_num={a.agent_num}: the attention critic attends over the OTHER agents, it needs at least 2")
    if a.mixer or a.episodic:
        raise NotImplementedError("MAAC: mixer / episodic training is not built")
    if int(a.attend_heads) < 1 or a.hid_size % int(a.attend_heads):
        raise ValueError(f"MAAC: attend_heads={a.attend_heads} must divide hid_size={a.hid_size}")


def _sqddpg_args_ok(a) -> None:
    """what SQDDPGNet builds: continuous actions, the deterministic recurrent agent, one action per agent (the coalition critic's action
    slots are one column each), transition updates, no mixer"""
    if not a.continuous:
        raise NotImplementedError("SQDDPG: continuous=False (discrete actions) is not built")
    if a.action_dim != 1:
        raise NotImplementedError(f"SQDDPG: action_dim={a.action_dim} is not built (one action per agent)")
    if a.mixer:
        raise NotImplementedError("SQDDPG: mixer=True is not built")
    if a.episodic:
        raise NotImplementedError("SQDDPG: episodic=True is not built (transition updates only)")
    if a.gaussian_policy:
        raise NotImplementedError("SQDDPG: gaussian_policy=True is not built (args/alg_args/sqddpg.yaml sets it False)")
    if a.agent_type != "rnn":
        raise NotImplementedError(f"SQDDPG: agent_type={a.agent_type!r} is not built (only 'rnn')")
    if int(a.sample_size) < 1:
        raise ValueError(f"SQDDPG: sample_size={a.sample_size} must be at least 1")


def _ppo_args_ok(a) -> None:
    """what PPONet builds: continuous actions, the deterministic recurrent agent (fixed std), one action per agent, transition updates,
    no mixer"""
    if not a.continuous:
        raise NotImplementedError("MAPPO/IPPO: continuous=False (discrete actions) is not built")
    if a.gaussian_policy:
        raise NotImplementedError("MAPPO/IPPO: gaussian_policy=True is not built (args/alg_args/mappo.yaml, ippo.yaml set it False)")
    if a.action_dim != 1:
        raise NotImplementedError(f"MAPPO/IPPO: action_dim={a.action_dim} is not built (one action per agent)")
    if a.mixer:
        raise NotImplementedError("MAPPO/IPPO: mixer=True is not built")
    if a.episodic:
        raise NotImplementedError("MAPPO/IPPO: episodic=True is not built (transition updates only)")
    if a.agent_type != "rnn":
        raise NotImplementedError(f"MAPPO/IPPO: agent_type={a.agent_type!r} is not built (only 'rnn')")
    if a.ppo_old_log_prob not in ("reference", "stored"):
        raise ValueError(f"MAPPO/IPPO: ppo_old_log_prob={a.ppo_old_log_prob!r} must be 'reference' or 'stored'")


def _activation(name: str):
    if name == "relu":
        return F.relu
    if name == "tanh":
        return torch.tanh
    raise ValueError(f"hid_activation {name!r}")
