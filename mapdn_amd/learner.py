"""MADDPG / IDDPG / MATD3 / COMA / MAAC / SQDDPG / MAPPO / IPPO learners for the batched env (BASELINE.json configs[4]).

What is learned, and every quirk of how, follows the reference (file:line cited at each piece):
`models/maddpg.py`, `models/iddpg.py`, `models/matd3.py`, `models/coma.py`, `learning_algorithms/ddpg.py`, `models/model.py`,
`agents/rnn_agent.py`, `critics/mlp_critic.py`, `utilities/trainer.py`, `utilities/util.py`,
defaults from `args/default.yaml` + `args/alg_args/{maddpg,iddpg,matd3,coma}.yaml` (equal but for COMA's `sample_size`).  Module and parameter names
are the reference's (`policy_dicts.0.fc1.weight`, `value_dicts.0.fc3.bias`, `target_net.…`,
`batchnorm.…`), so a reference `model.pt` (`{"model_state_dict": …}`, train.py:119) loads with
`strict=True` and vice versa.

What is different is how it runs: tensors in, tensors out, no Python lists or host round trips —
a batch is a dict of device tensors straight from `mapdn_amd.replay`; the centralised MADDPG critic
never materialises the reference's [batch, n, n·obs] input (maddpg.py:41-66) — its first layer is
evaluated as (shared observation term) + (agent-id column) + (joint-action term), with the
"other agents' actions are detached" rule (maddpg.py:52-58) kept by a zero-valued, gradient-carrying
own-action term; MATD3's twin (matd3.py:35-86: ONE critic valued twice, with one more input column that is 0 or 1) is that
first layer and the same plus the last column of fc1.weight, both heads in one HIP launch; COMA's counterfactual baseline (coma.py:139-151:
the critic valued sample_size more times with one agent's action redrawn) is one HIP launch over the first layer's output, a sampled row
being the taken row plus a rank-1 term; data-parallel ranks average gradients through one flat RCCL all-reduce per update.

Only the configuration the DDPG family trains with exists: continuous actions, deterministic
(non-Gaussian) policy head — and MAAC's (models/maac.py, critics/maac_critic.py, agents/rnn_agent_gaussian.py: Gaussian head, one
attention critic whose attention over the other agents is one HIP launch each way, csrc/critic_attn.hip), reached through
make_alg_args(..., alg="maac") — and SQDDPG's (models/sqddpg.py: the deterministic agents with a critic valued on sampled coalition
orders, whose b x sample_size x n rows are formed inside the kernels of csrc/critic_shap.hip from a prefix sum over positions), reached
through make_alg_args(..., alg="sqddpg") — and MAPPO's / IPPO's (models/mappo.py, models/ippo.py, learning_algorithms/ppo.py: the deterministic
agents with a state-value critic, generalised advantage estimation and the clipped surrogate / clipped value losses; the GAE recurrence over
strided chains and both losses with their gradients are the launches of csrc/ppo.hip), reached through make_alg_args(..., alg="mappo" | "ippo").
Two of the reference's quirks there are kept and stated at PPONet: the GAE chain is cut only by a row that is BOTH done and last_step, and
the ratio's old log-probability is the stored action (models/model.py:309) unless ppo_old_log_prob="stored".  Anything else raises.
"""
from __future__ import annotations

import math
import os
from types import SimpleNamespace
from typing import Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._lib import INFO_KEYS
from .replay import TransReplayBuffer
from .rollout import translate_action

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
    if alg == "maac":
        _maac_args_ok(a)
        return a
    if alg == "sqddpg":
        _sqddpg_args_ok(a)
        return a
    if alg in ("mappo", "ippo"):
        _ppo_args_ok(a)
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


class _LayerNorm64(torch.autograd.Function):
    """LayerNorm over 64 features with the ReLU that follows it in both reference modules fused in (agents/rnn_agent.py:16-21,
    critics/mlp_critic.py:22-27), forward and backward as hand-written HIP kernels (libmapdn_hip.so: mapdn_layernorm64_*): at the
    reference's update intensity a batch is millions of rows of 64, where the stock kernels run at an eighth of the HBM rate."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, relu):
        from . import _lib
        lib = _lib.load()
        x2 = x.reshape(-1, 64).contiguous()
        w, b = weight.detach().contiguous(), bias.detach().contiguous()
        rows = x2.shape[0]
        y = torch.empty_like(x2)
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        with torch.cuda.device(x.device):
            _lib.check(lib.mapdn_layernorm64_forward(x2.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                                     rows, float(eps), int(relu), torch.cuda.current_stream(x.device).cuda_stream))
        ctx.save_for_backward(x2, w, b, mean, rstd)
        ctx.relu, ctx.shape = bool(relu), x.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        from . import _lib
        lib = _lib.load()
        x2, w, b, mean, rstd = ctx.saved_tensors
        rows = x2.shape[0]
        dy2 = dy.reshape(-1, 64).contiguous()
        dx = torch.empty_like(x2)
        dw, db = torch.empty_like(w), torch.empty_like(b)
        with torch.cuda.device(x2.device):                  # the block count follows the CU count of the CURRENT device: ask inside the context
            partial = torch.empty(lib.mapdn_layernorm64_backward_blocks(rows) * 128, dtype=torch.float32, device=x2.device)
            _lib.check(lib.mapdn_layernorm64_backward(dy2.data_ptr(), x2.data_ptr(), w.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                                      dx.data_ptr(), dw.data_ptr(), db.data_ptr(), partial.data_ptr(), rows, int(ctx.relu),
                                                      torch.cuda.current_stream(x2.device).cuda_stream))
        return dx.view(ctx.shape), dw, db, None, None


class _TallLinear(torch.autograd.Function):
    """y = x W^T + b for x of MILLIONS of rows and a small weight (the 64 -> 64 and 64 -> 1 layers of the critic / agent trunks on a
    batch of 32 x 8192 transitions x 38 agents = 10 M rows).  Forward and dX are ordinary GEMMs; the WEIGHT gradient dW = dy^T x is a
    [out, in] product with the 10 M rows as its reduction dimension — the BLAS back end runs it on two workgroups (8.4 ms and 5.6 ms
    per call, the two largest GEMM entries of profiles/e2e/r04_e2e_reference_kernel_stats.txt, against 1.3 ms for the forward).  Here
    the rows are cut into blocks whose partial products are one batched GEMM, then summed (split-K by hand): same sum, other order."""

    BLOCK_ROWS = 16384

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return F.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = dy @ weight
        if ctx.needs_input_grad[1]:
            rows, blk = x.shape[0], _TallLinear.BLOCK_ROWS
            full = rows // blk * blk
            dy2, x2 = dy.reshape(rows, -1).contiguous(), x.reshape(rows, -1).contiguous()      # (a permuted upstream gradient is not viewable)
            dw = torch.bmm(dy2[:full].view(-1, blk, dy2.shape[1]).transpose(1, 2), x2[:full].view(-1, blk, x2.shape[1])).sum(0)
            if full < rows:
                dw = dw + dy2[full:].t() @ x2[full:]
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy.reshape(-1, dy.shape[-1]).sum(0)
        return dx, dw, db


def tall_linear(lin: nn.Linear, x: torch.Tensor) -> torch.Tensor:
    """lin(x); with the hand-split weight gradient when x is a tall 2-D batch on the GPU (>= 2^18 rows, <= 128 features each way)"""
    if x.dim() == 2 and _tall_ok(x, x.shape[0], lin.weight):
        return _TallLinear.apply(x, lin.weight, lin.bias)
    return lin(x)


def tall_linear_w(x: torch.Tensor, weight: torch.Tensor, bias=None) -> torch.Tensor:
    """x W^T (+ b) for a weight given as a tensor (a column slice of a larger layer): _TallLinear on a tall GPU batch under autograd.
    The central critic's observation block (K = n * obs = 2204-3116 inputs, 2^18 rows of reduction) included: its weight gradient as 16
    batched products + a sum is 0.3 ms faster per update than the back end's single GEMM (round 6, same-box A/B: value update 0.216 ->
    0.205 s per episode); MAPDN_TALL_LINEAR_WIDE=0 keeps the stock backward for weights wider than 128 inputs."""
    if (x.dim() == 2 and x.is_cuda and x.shape[0] >= (1 << 18) and torch.is_grad_enabled() and weight.requires_grad and weight.shape[0] <= 256
            and os.environ.get("MAPDN_TALL_LINEAR", "1") != "0"
            and (weight.shape[1] <= 128 or os.environ.get("MAPDN_TALL_LINEAR_WIDE", "1") != "0")):
        return _TallLinear.apply(x, weight, bias)
    return F.linear(x, weight, bias)


def _tall_ok(x: torch.Tensor, rows: int, weight: torch.Tensor) -> bool:
    return (x.is_cuda and rows >= (1 << 18) and weight.shape[0] <= 256 and weight.shape[1] <= 128 and torch.is_grad_enabled()
            and weight.requires_grad and os.environ.get("MAPDN_TALL_LINEAR", "1") != "0")


_GRU_FUSED_OK: Dict[str, bool] = {}


def _gru_fused_ok(device) -> bool:
    """one-time self-check of the route gru_cell_tall takes (input / hidden projections as _TallLinear, then ATen's fused GRU cell on
    the pre-computed gates) against nn.GRUCell, values and gradients; any exception or mismatch disables the route for the process"""
    key = str(device)
    if key not in _GRU_FUSED_OK:
        ok = False
        try:
            g = torch.Generator(device="cpu").manual_seed(1)
            with torch.random.fork_rng(devices=[]):          # nn.GRUCell's initialisation draws from the GLOBAL generator: leave the caller's stream alone
                cell = nn.GRUCell(8, 8).to(device)
            x = torch.randn(32, 8, generator=g).to(device).requires_grad_(True)
            h = torch.randn(32, 8, generator=g).to(device).requires_grad_(True)
            ref = cell(x, h)
            gr = torch.autograd.grad(ref.square().sum(), [x, h, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh])
            out = torch.ops.aten._thnn_fused_gru_cell(_TallLinear.apply(x, cell.weight_ih, None), _TallLinear.apply(h, cell.weight_hh, None),
                                                      h, cell.bias_ih, cell.bias_hh)[0]
            go = torch.autograd.grad(out.square().sum(), [x, h, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh])
            ok = bool(torch.allclose(out, ref, rtol=1e-5, atol=1e-6)) and all(bool(torch.allclose(a, b, rtol=1e-4, atol=1e-5)) for a, b in zip(go, gr))
        except Exception:                      # noqa: BLE001 — an ATen signature change must not break training: the stock cell is used
            ok = False
        _GRU_FUSED_OK[key] = ok
    return _GRU_FUSED_OK[key]


def gru_cell_tall(rnn: nn.GRUCell, x: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
    """rnn(x, h); on a tall GPU batch under autograd the two projections go through _TallLinear (their weight gradients are products
    with millions of rows of reduction) and ATen's fused cell does the gate arithmetic, as inside nn.GRUCell"""
    if x.dim() == 2 and _tall_ok(x, x.shape[0], rnn.weight_ih) and rnn.bias and _gru_fused_ok(x.device):
        ig = _TallLinear.apply(x, rnn.weight_ih, None)
        hg = _TallLinear.apply(h, rnn.weight_hh, None)
        return torch.ops.aten._thnn_fused_gru_cell(ig, hg, h, rnn.bias_ih, rnn.bias_hh)[0]
    return rnn(x, h)


class _LayerNorm64BC(torch.autograd.Function):
    """relu(LayerNorm(base[b] + per_n[i])) for every (b, i), rows ordered (b, i), WITHOUT materialising the [b, n, 64] sum — the central
    critic's first layer (DDPGNet._value_central) is exactly such a sum: W_obs·obs_all + bias per batch element plus the agent's id
    column.  HIP kernels mapdn_layernorm64_bc_* (csrc/policy.hip): the row is formed in registers (one f32 add, as PyTorch's broadcast
    add would), forward and backward; the backward hands back dx per formed row, reduced here over the agents / over the batch."""

    @staticmethod
    def forward(ctx, base, per_n, weight, bias, eps, relu):
        from . import _lib
        lib = _lib.load()
        b2, p2 = base.contiguous(), per_n.contiguous()
        w, bb = weight.detach().contiguous(), bias.detach().contiguous()
        nb, n = b2.shape[0], p2.shape[0]
        rows = nb * n
        y = torch.empty(rows, 64, dtype=torch.float32, device=base.device)
        mean = torch.empty(rows, dtype=torch.float32, device=base.device)
        rstd = torch.empty_like(mean)
        with torch.cuda.device(base.device):
            _lib.check(lib.mapdn_layernorm64_bc_forward(b2.data_ptr(), p2.data_ptr(), n, w.data_ptr(), bb.data_ptr(), y.data_ptr(), mean.data_ptr(),
                                                        rstd.data_ptr(), rows, float(eps), int(relu), torch.cuda.current_stream(base.device).cuda_stream))
        ctx.save_for_backward(b2, p2, w, bb, mean, rstd)
        ctx.relu = bool(relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import _lib
        lib = _lib.load()
        b2, p2, w, bb, mean, rstd = ctx.saved_tensors
        nb, n = b2.shape[0], p2.shape[0]
        rows = nb * n
        dy2 = dy.reshape(rows, 64).contiguous()
        dx = torch.empty_like(dy2)
        dw, db = torch.empty_like(w), torch.empty_like(bb)
        with torch.cuda.device(b2.device):
            partial = torch.empty(lib.mapdn_layernorm64_backward_blocks(rows) * 128, dtype=torch.float32, device=b2.device)
            _lib.check(lib.mapdn_layernorm64_bc_backward(dy2.data_ptr(), b2.data_ptr(), p2.data_ptr(), n, w.data_ptr(), bb.data_ptr(), mean.data_ptr(),
                                                         rstd.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(), partial.data_ptr(), rows,
                                                         int(ctx.relu), torch.cuda.current_stream(b2.device).cuda_stream))
        dx3 = dx.view(nb, n, 64)
        dbase = dx3.sum(1) if ctx.needs_input_grad[0] else None
        dpern = dx3.sum(0) if ctx.needs_input_grad[1] else None
        return dbase, dpern, dw, db, None, None


class _ReluDot64(torch.autograd.Function):
    """v = relu(pre) @ w^T + b for pre [rows, 64], w [1, 64]: the critic's activation after fc2 and its one-output fc3 as one pass
    over the pre-activation (mapdn_relu_dot64_*, csrc/policy.hip); relu(pre) is never materialised, forward or backward."""

    @staticmethod
    def forward(ctx, pre, weight, bias):
        from . import _lib
        lib = _lib.load()
        p2 = pre.contiguous()
        w = weight.detach().reshape(64).contiguous()
        rows = p2.shape[0]
        v = torch.empty(rows, 1, dtype=torch.float32, device=pre.device)
        with torch.cuda.device(pre.device):
            _lib.check(lib.mapdn_relu_dot64_forward(p2.data_ptr(), w.data_ptr(), 0.0, v.data_ptr(), rows,
                                                    torch.cuda.current_stream(pre.device).cuda_stream))
        ctx.save_for_backward(p2, w)
        return v + bias.detach()          # (the bias stays a device tensor: no host read of a parameter inside the training loop)

    @staticmethod
    def backward(ctx, dv):
        from . import _lib
        lib = _lib.load()
        p2, w = ctx.saved_tensors
        rows = p2.shape[0]
        dv2 = dv.reshape(rows).contiguous()
        dpre = torch.empty_like(p2)
        dw, db = torch.empty(64, dtype=torch.float32, device=p2.device), torch.empty(64, dtype=torch.float32, device=p2.device)
        with torch.cuda.device(p2.device):
            partial = torch.empty(lib.mapdn_layernorm64_backward_blocks(rows) * 128, dtype=torch.float32, device=p2.device)
            _lib.check(lib.mapdn_relu_dot64_backward(dv2.data_ptr(), p2.data_ptr(), w.data_ptr(), dpre.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                                     partial.data_ptr(), rows, torch.cuda.current_stream(p2.device).cuda_stream))
        return dpre, dw.view(1, 64), db[:1].clone()


def relu_dot64_ok(act, fc3: nn.Linear, pre: torch.Tensor) -> bool:
    return (pre.is_cuda and pre.dtype == torch.float32 and pre.dim() == 2 and pre.shape[1] == 64 and pre.shape[0] >= 64 * 1024 and act is F.relu
            and fc3.out_features == 1 and fc3.bias is not None and os.environ.get("MAPDN_FUSED_RELU_DOT", "1") != "0")


class _CriticHead(torch.autograd.Function):
    """v = relu(relu(LayerNorm(x)) W2^T + b2) . w3 + b3 on rows of 64 — everything of the critic behind its first layer
    (critics/mlp_critic.py:22-36) — as ONE HIP launch forward and one backward (libmapdn_hip.so: mapdn_critic_head_*, csrc/critic.hip:
    fp32 MFMA, the 16-row tile stays in registers from the LayerNorm input to v / from dv to dx and the parameter gradients; the backward
    recomputes the forward, so nothing but the inputs is saved).  x is read ([rows, 64], per_n None) or formed as base[b] + per_n[i]
    (rows ordered (b, i): the central critic); the backward then returns dbase / dper_n already summed over the agents / the batch."""

    @staticmethod
    def forward(ctx, x, per_n, ln_w, ln_b, eps, w2, b2, w3, b3):
        from . import _lib
        lib = _lib.load()
        x2 = x.contiguous()
        pn = per_n.contiguous() if per_n is not None else None
        n = pn.shape[0] if pn is not None else 1
        rows = x2.shape[0] * n
        prm = tuple(t.detach().contiguous() for t in (ln_w, ln_b, w2, b2, w3.reshape(64), b3.reshape(1)))
        v = torch.empty(rows, 1, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.mapdn_critic_head_forward(x2.data_ptr(), pn.data_ptr() if pn is not None else None, n, prm[0].data_ptr(), prm[1].data_ptr(),
                                                     float(eps), prm[2].data_ptr(), prm[3].data_ptr(), prm[4].data_ptr(), prm[5].data_ptr(), v.data_ptr(),
                                                     rows, torch.cuda.current_stream(x.device).cuda_stream))
        ctx.save_for_backward(x2, pn, *prm)
        ctx.eps, ctx.rows, ctx.n = float(eps), rows, n
        return v

    @staticmethod
    def backward(ctx, dv):
        from . import _lib
        lib = _lib.load()
        x2, pn, g, b, w2, b2, w3, b3 = ctx.saved_tensors
        rows, n, formed = ctx.rows, ctx.n, pn is not None
        need = ctx.needs_input_grad
        param_grads = bool(need[2] or need[3] or need[5] or need[6] or need[7] or need[8])
        dv2 = dv.reshape(rows).contiguous()
        dx = torch.empty_like(x2)
        dev = x2.device
        with torch.cuda.device(dev):
            grads = torch.empty(4416 + (n * 64 if formed else 0), dtype=torch.float32, device=dev)
            scratch = torch.empty(max(1, lib.mapdn_critic_head_scratch_floats(rows, n, int(formed))), dtype=torch.float32, device=dev)
            _lib.check(lib.mapdn_critic_head_backward(dv2.data_ptr(), x2.data_ptr(), pn.data_ptr() if formed else None, n, g.data_ptr(), b.data_ptr(),
                                                      ctx.eps, w2.data_ptr(), b2.data_ptr(), w3.data_ptr(), b3.data_ptr(), dx.data_ptr(), grads.data_ptr(),
                                                      scratch.data_ptr(), rows, int(param_grads), torch.cuda.current_stream(dev).cuda_stream))
        dpn = grads[4416:].view(n, 64) if formed and need[1] else None
        if not param_grads:
            return dx, dpn, None, None, None, None, None, None, None
        return (dx, dpn, grads[4096:4160], grads[4160:4224], None, grads[:4096].view(64, 64), grads[4224:4288], grads[4288:4352].view(1, 64),
                grads[4352:4353])


class _CriticHeadOwnAction(torch.autograd.Function):
    """The central critic's value as a function of every agent's OWN action only (models/maddpg.py:52-58: the other agents' actions
    enter detached): forward = _CriticHead on base[b] + id_column[i] (the own-action term (a - a.detach()) W_act[:, i] is zero in
    value), backward = d loss / d act[b, i] = dx[b, i, :] . W_act[:, i] straight from the kernel (mapdn_critic_head_backward_dot);
    no [b, n, 64] tensor exists in either direction and the critic's parameters receive no gradient — the policy optimiser does not
    own them (utilities/trainer.py:26-27, 73-98)."""

    @staticmethod
    def forward(ctx, act, base, per_n, dot_w, ln_w, ln_b, eps, w2, b2, w3, b3):
        from . import _lib
        lib = _lib.load()
        x2, pn, dw = base.detach().contiguous(), per_n.detach().contiguous(), dot_w.detach().contiguous()
        n = pn.shape[0]
        rows = x2.shape[0] * n
        prm = tuple(t.detach().contiguous() for t in (ln_w, ln_b, w2, b2, w3.reshape(64), b3.reshape(1)))
        v = torch.empty(rows, 1, dtype=torch.float32, device=base.device)
        with torch.cuda.device(base.device):
            _lib.check(lib.mapdn_critic_head_forward(x2.data_ptr(), pn.data_ptr(), n, prm[0].data_ptr(), prm[1].data_ptr(), float(eps), prm[2].data_ptr(),
                                                     prm[3].data_ptr(), prm[4].data_ptr(), prm[5].data_ptr(), v.data_ptr(), rows,
                                                     torch.cuda.current_stream(base.device).cuda_stream))
        ctx.save_for_backward(x2, pn, dw, *prm)
        ctx.eps, ctx.rows, ctx.n, ctx.act_shape = float(eps), rows, n, act.shape
        return v

    @staticmethod
    def backward(ctx, dv):
        from . import _lib
        lib = _lib.load()
        x2, pn, dw, g, b, w2, b2, w3, b3 = ctx.saved_tensors
        rows, n, dev = ctx.rows, ctx.n, x2.device
        dv2 = dv.reshape(rows).contiguous()
        dact = torch.empty(rows, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.mapdn_critic_head_backward_dot(dv2.data_ptr(), x2.data_ptr(), pn.data_ptr(), n, g.data_ptr(), b.data_ptr(), ctx.eps,
                                                          w2.data_ptr(), b2.data_ptr(), w3.data_ptr(), b3.data_ptr(), dw.data_ptr(), dact.data_ptr(), rows,
                                                          torch.cuda.current_stream(dev).cuda_stream))
        return (dact.view(ctx.act_shape),) + (None,) * 10


class _CriticHeadMSE(torch.autograd.Function):
    """The value loss of the DDPG family (learning_algorithms/ddpg.py:36-38 == models/maddpg.py:122-124),
        loss = sum_rows w[row] (returns[row] - v[row])^2,    w[row] = scale * wrow[row / n]   (wrow None: 1),
    with v the critic head of _CriticHead — as ONE launch that produces the loss AND every gradient of it (mapdn_critic_head_mse):
    d loss / d v = -2 w (returns - v) is known per row the moment v is, so the separate forward launch (a fifth 64 x 64 product over
    all rows) disappears.  backward only scales the stored gradients by the incoming one (1 for `loss.backward()`)."""

    @staticmethod
    def forward(ctx, x, per_n, ln_w, ln_b, eps, w2, b2, w3, b3, returns, wrow, scale):
        from . import _lib
        lib = _lib.load()
        x2 = x.detach().contiguous()
        pn = per_n.detach().contiguous() if per_n is not None else None
        n = pn.shape[0] if pn is not None else 1
        rows, formed, dev = x2.shape[0] * n, pn is not None, x2.device
        prm = tuple(t.detach().contiguous() for t in (ln_w, ln_b, w2, b2, w3.reshape(64), b3.reshape(1)))
        ret = returns.detach().reshape(rows).contiguous().float()
        wr = wrow.detach().contiguous().float() if wrow is not None else None
        sc = scale.detach().reshape(1).contiguous().float()
        dx = torch.empty_like(x2)
        with torch.cuda.device(dev):
            grads = torch.empty(4416 + (n * 64 if formed else 0), dtype=torch.float32, device=dev)
            scratch = torch.empty(max(1, lib.mapdn_critic_head_scratch_floats(rows, n, int(formed))), dtype=torch.float32, device=dev)
            _lib.check(lib.mapdn_critic_head_mse(ret.data_ptr(), wr.data_ptr() if wr is not None else None, sc.data_ptr(), x2.data_ptr(),
                                                 pn.data_ptr() if formed else None, n, prm[0].data_ptr(), prm[1].data_ptr(), float(eps), prm[2].data_ptr(),
                                                 prm[3].data_ptr(), prm[4].data_ptr(), prm[5].data_ptr(), dx.data_ptr(), grads.data_ptr(), scratch.data_ptr(),
                                                 rows, torch.cuda.current_stream(dev).cuda_stream))
        ctx.save_for_backward(dx, grads)
        ctx.n, ctx.formed = n, formed
        return grads[4353].clone()

    @staticmethod
    def backward(ctx, g):
        dx, grads = ctx.saved_tensors
        n, need = ctx.n, ctx.needs_input_grad
        gs = grads * g
        return (dx * g if need[0] else None, gs[4416:].view(n, 64) if ctx.formed and need[1] else None, gs[4096:4160], gs[4160:4224], None,
                gs[:4096].view(64, 64), gs[4224:4288], gs[4288:4352].view(1, 64), gs[4352:4353], None, None, None)


class _CriticTwinMSE(torch.autograd.Function):
    """MATD3's value loss (models/matd3.py:143-150) on the twin of the central critic,
        loss = sum_rows w[row] 1/2 [(returns - v1)^2 + (returns - v2)^2],   w[row] = scale * wrow[row / n]   (wrow None: 1),
    v1 / v2 = the critic head on base[b] + per_n[i] / on the same + flag_col — ONE launch for the loss and every gradient of it
    (mapdn_critic_twin_mse, csrc/critic_twin.hip): dbase, dper_n and the head's parameter gradients arrive summed over both heads,
    d flag_col is the second head's dx summed over all rows.  NOT the default route: at config 5's 10 M rows it takes 6.6 ms where two
    mapdn_critic_head_mse launches take 5.9; DDPGNet.value_mse takes it under MAPDN_TWIN_MSE_KERNEL=1."""
    launches = 0           # how often the kernel was reached (tests count through the wrapper)

    @staticmethod
    def forward(ctx, base, per_n, flag, ln_w, ln_b, eps, w2, b2, w3, b3, returns, wrow, scale):
        from . import _lib
        lib = _lib.load()
        x2, pn, fl = base.detach().contiguous(), per_n.detach().contiguous(), flag.detach().contiguous()
        n = pn.shape[0]
        rows, dev = x2.shape[0] * n, x2.device
        prm = tuple(t.detach().contiguous() for t in (ln_w, ln_b, w2, b2, w3.reshape(64), b3.reshape(1)))
        ret = returns.detach().reshape(rows).contiguous().float()
        wr = wrow.detach().contiguous().float() if wrow is not None else None
        sc = scale.detach().reshape(1).contiguous().float()
        dbase = torch.empty_like(x2)
        with torch.cuda.device(dev):
            grads = torch.empty(4480 + n * 64, dtype=torch.float32, device=dev)
            scratch = torch.empty(max(1, lib.mapdn_critic_twin_scratch_floats(rows, n)), dtype=torch.float32, device=dev)
            _lib.check(lib.mapdn_critic_twin_mse(ret.data_ptr(), wr.data_ptr() if wr is not None else None, sc.data_ptr(), x2.data_ptr(), pn.data_ptr(), n,
                                                 fl.data_ptr(), prm[0].data_ptr(), prm[1].data_ptr(), float(eps), prm[2].data_ptr(), prm[3].data_ptr(),
                                                 prm[4].data_ptr(), prm[5].data_ptr(), dbase.data_ptr(), grads.data_ptr(), scratch.data_ptr(), rows,
                                                 torch.cuda.current_stream(dev).cuda_stream))
        _CriticTwinMSE.launches += 1
        ctx.save_for_backward(dbase, grads)
        ctx.n = n
        return grads[4353].clone()

    @staticmethod
    def backward(ctx, g):
        dbase, grads = ctx.saved_tensors
        n, need = ctx.n, ctx.needs_input_grad
        gs = grads * g
        return (dbase * g if need[0] else None, gs[4480:].view(n, 64) if need[1] else None, gs[4416:4480] if need[2] else None, gs[4096:4160],
                gs[4160:4224], None, gs[:4096].view(64, 64), gs[4224:4288], gs[4288:4352].view(1, 64), gs[4352:4353], None, None, None)


def critic_twin_forward(cr: "MLPCritic", base: torch.Tensor, per_n: torch.Tensor, flag: torch.Tensor, want=("v1", "v2")):
    """the twin head without autograd (target values, evaluation): {name: [b * n, 1]} for the names in `want` out of v1, v2, vmin —
    one mapdn_critic_twin_forward launch"""
    from . import _lib
    lib = _lib.load()
    x2, pn, fl = base.detach().contiguous(), per_n.detach().contiguous(), flag.detach().contiguous()
    n = pn.shape[0]
    rows, dev, ln = x2.shape[0] * n, x2.device, cr.layernorm
    prm = tuple(t.detach().contiguous() for t in (ln.weight, ln.bias, cr.fc2.weight, cr.fc2.bias, cr.fc3.weight.reshape(64), cr.fc3.bias.reshape(1)))
    out = {k: torch.empty(rows, 1, dtype=torch.float32, device=dev) for k in want}
    ptr = [out[k].data_ptr() if k in out else None for k in ("v1", "v2", "vmin")]
    with torch.cuda.device(dev):
        _lib.check(lib.mapdn_critic_twin_forward(x2.data_ptr(), pn.data_ptr(), n, fl.data_ptr(), prm[0].data_ptr(), prm[1].data_ptr(), float(ln.eps),
                                                 prm[2].data_ptr(), prm[3].data_ptr(), prm[4].data_ptr(), prm[5].data_ptr(), ptr[0], ptr[1], ptr[2], rows,
                                                 torch.cuda.current_stream(dev).cuda_stream))
    critic_twin_forward.launches += 1
    return out


critic_twin_forward.launches = 0


class twin_pair_mse:
    """how often MATD3's value loss took the pair of single-head loss launches (tests count the routes)"""
    launches = 0


HEAD_MAX_FORMED_N = 88      # formed rows keep one [n][64] LDS accumulator per wavefront: n <= 88 fits the 160 KB of a CU with four of them


def critic_head_ok(cr: "MLPCritic", x: torch.Tensor, rows: int, formed_n: int = 0) -> bool:
    """the one-launch critic head covers the reference's default critic (LayerNorm, ReLU, hidden size 64, one output) in fp32 on the GPU
    (formed_n: the number of agents when the rows are formed as base[b] + per_n[i])"""
    return (formed_n <= HEAD_MAX_FORMED_N and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[-1] == 64 and rows >= 1024 and rows < 2 ** 31 and cr.use_ln
            and cr.act is F.relu and cr.layernorm.elementwise_affine and cr.layernorm.bias is not None and cr.fc2.in_features == 64
            and cr.fc2.out_features == 64 and cr.fc2.bias is not None and cr.fc3.out_features == 1 and cr.fc3.bias is not None
            and cr.fc2.weight.dtype == torch.float32 and os.environ.get("MAPDN_FUSED_HEAD", "1") != "0")


def critic_twin_ok(cr: "MLPCritic", base: torch.Tensor, rows: int, n: int) -> bool:
    """the one-launch twin head (csrc/critic_twin.hip) covers what critic_head_ok covers for formed rows — the default critic in fp32 on
    the GPU, enough rows, n <= 88 —; MAPDN_FUSED_TWIN=0 switches it off (the PyTorch route and the single-head kernels remain).  It gates
    the forward launch (target min, value()) and both fused forms of the value loss; of those the default is two mapdn_critic_head_mse
    launches, MAPDN_TWIN_MSE_KERNEL=1 takes mapdn_critic_twin_mse (one launch, 12 % slower at 10 M rows: DESIGN section 11)"""
    return critic_head_ok(cr, base, rows, n) and n >= 1 and os.environ.get("MAPDN_FUSED_TWIN", "1") != "0"


def critic_cf_ok(cr: "MLPCritic", x: torch.Tensor, rows: int, act_dim: int) -> bool:
    """the one-launch counterfactual baseline (csrc/critic_cf.hip) covers what critic_head_ok covers for rows that are read — the default
    critic in fp32 on the GPU, enough rows — with one action per agent; MAPDN_FUSED_CF=0 switches it off (the PyTorch loop over the samples
    remains)"""
    return act_dim == 1 and critic_head_ok(cr, x, rows) and os.environ.get("MAPDN_FUSED_CF", "1") != "0"


def critic_counterfactual(cr: "MLPCritic", x: torch.Tensor, act_col: torch.Tensor, delta: torch.Tensor, want_v0: bool = True):
    """(baseline [rows], v0 [rows] or None) without autograd: baseline = mean over s of the head on x + delta[s] * act_col[row % n], v0 = the
    head on x — one mapdn_critic_head_counterfactual launch.  x [rows, 64], act_col [n, 64], delta [S, rows]."""
    from . import _lib
    lib = _lib.load()
    x2, col, dl = x.detach().contiguous(), act_col.detach().contiguous(), delta.detach().contiguous()
    rows, dev, ln = x2.shape[0], x2.device, cr.layernorm
    if dl.dim() != 2 or dl.shape[1] != rows or col.dim() != 2 or col.shape[1] != 64 or dl.dtype != torch.float32 or col.dtype != torch.float32:
        raise ValueError("critic_counterfactual: x [rows, 64], act_col [n, 64], delta [S, rows], float32")
    prm = tuple(t.detach().contiguous() for t in (ln.weight, ln.bias, cr.fc2.weight, cr.fc2.bias, cr.fc3.weight.reshape(64), cr.fc3.bias.reshape(1)))
    baseline = torch.empty(rows, dtype=torch.float32, device=dev)
    v0 = torch.empty(rows, dtype=torch.float32, device=dev) if want_v0 else None
    with torch.cuda.device(dev):
        _lib.check(lib.mapdn_critic_head_counterfactual(x2.data_ptr(), col.shape[0], col.data_ptr(), dl.data_ptr(), dl.shape[0], prm[0].data_ptr(),
                                                        prm[1].data_ptr(), float(ln.eps), prm[2].data_ptr(), prm[3].data_ptr(), prm[4].data_ptr(),
                                                        prm[5].data_ptr(), baseline.data_ptr(), v0.data_ptr() if v0 is not None else None, rows,
                                                        torch.cuda.current_stream(dev).cuda_stream))
    critic_counterfactual.launches += 1
    return baseline, v0


critic_counterfactual.launches = 0           # how often the kernel was reached (tests count the routes)


def critic_head(cr: "MLPCritic", x: torch.Tensor, per_n: Optional[torch.Tensor] = None) -> torch.Tensor:
    ln = cr.layernorm
    return _CriticHead.apply(x, per_n, ln.weight, ln.bias, ln.eps, cr.fc2.weight, cr.fc2.bias, cr.fc3.weight, cr.fc3.bias)


def layernorm_act_bc(ln: nn.LayerNorm, act, base: torch.Tensor, per_n: torch.Tensor):
    """act(LayerNorm(base.unsqueeze(1) + per_n.unsqueeze(0))).reshape(b * n, 64) through the broadcast-input kernels, or None when the
    case is not theirs (the caller then forms the sum and takes layernorm_act)"""
    if (base.is_cuda and base.dtype == torch.float32 and per_n.dtype == torch.float32 and base.dim() == 2 and per_n.dim() == 2
            and base.shape[-1] == 64 and per_n.shape[-1] == 64 and act is F.relu and ln.elementwise_affine and ln.bias is not None
            and ln.weight.dtype == torch.float32 and base.shape[0] * per_n.shape[0] >= 1024
            and os.environ.get("MAPDN_FUSED_LN", "1") != "0" and os.environ.get("MAPDN_FUSED_LN_BC", "1") != "0"):
        return _LayerNorm64BC.apply(base, per_n, ln.weight, ln.bias, ln.eps, True)
    return None


def layernorm_act(ln: nn.LayerNorm, act, x: torch.Tensor) -> torch.Tensor:
    """act(LayerNorm(x)): one HIP launch each way for the reference's default shape (64 features, ReLU, fp32, on the GPU), the
    PyTorch modules otherwise (MAPDN_FUSED_LN=0 forces them)."""
    if (x.is_cuda and x.dtype == torch.float32 and x.shape[-1] == 64 and act is F.relu and ln.elementwise_affine and ln.bias is not None
            and ln.weight.dtype == torch.float32 and x.numel() >= 64 * 1024 and os.environ.get("MAPDN_FUSED_LN", "1") != "0"):
        return _LayerNorm64.apply(x, ln.weight, ln.bias, ln.eps, True)
    return act(ln(x))


def _splitk_dw(dy2: torch.Tensor, x2: torch.Tensor, blk: int = 16384) -> torch.Tensor:
    """dy2^T x2 ([out, in]) for [rows, out] x [rows, in] with millions of rows: the rows cut into blocks whose partial products are one
    batched GEMM, then summed (what _TallLinear.backward does for its weight).  dy2 may be a column slice of a wider tensor."""
    rows = x2.shape[0]
    full = rows // blk * blk
    dw = None
    if full:
        a = dy2[:full].unflatten(0, (-1, blk)).transpose(1, 2)
        dw = torch.bmm(a, x2[:full].unflatten(0, (-1, blk))).sum(0)
    if full < rows:
        rest = dy2[full:].t() @ x2[full:]
        dw = rest if dw is None else dw + rest
    return dw


class _PolicyTrunk(torch.autograd.Function):
    """means = fc2(GRUCell(relu(LayerNorm(fc1(obs) + id column)), last_hid)) of the shared recurrent agent (agents/rnn_agent.py:5-32) for the
    policy UPDATE (models/maddpg.py:103-125: only the means carry gradient — the loss does not read the new hidden state), forward and
    backward as HIP launches: mapdn_policy_forward_train (the rollout's one-launch forward; keeps x1 = the LayerNorm input) and
    mapdn_policy_backward (csrc/policy_bwd.hip: recomputes the trunk, writes d gate pre-activations / xn / dx1 and the small gradients).
    What is left for the BLAS back end are the three K = rows weight-gradient products, run block-wise (_splitk_dw).  The PyTorch route
    moved ~100 GB per update through the projections, ATen's fused cell and its workspace."""

    @staticmethod
    def forward(ctx, obs2, hid2, n_agents, ids, eps, w1, b1, lnw, lnb, w_ih, w_hh, b_ih, b_hh, w2, b2):
        from . import _lib
        lib = _lib.load()
        obs2, hid2 = obs2.contiguous(), hid2.contiguous()
        rows, o = obs2.shape
        prm = tuple(t.detach().contiguous() for t in (w1, b1, lnw, lnb, w_ih, w_hh, b_ih, b_hh, w2, b2))
        means = torch.empty(rows, dtype=torch.float32, device=obs2.device)
        x1 = torch.empty(rows, 64, dtype=torch.float32, device=obs2.device)
        with torch.cuda.device(obs2.device):
            _lib.check(lib.mapdn_policy_forward_train(obs2.data_ptr(), hid2.data_ptr(), *(t.data_ptr() for t in prm), means.data_ptr(), None,
                                                      x1.data_ptr(), rows, int(n_agents), o, int(ids), float(eps),
                                                      torch.cuda.current_stream(obs2.device).cuda_stream))
        ctx.save_for_backward(obs2, hid2, x1, *prm)
        ctx.n_agents, ctx.ids, ctx.eps = int(n_agents), int(ids), float(eps)
        return means

    @staticmethod
    def backward(ctx, dmeans):
        from . import _lib
        lib = _lib.load()
        obs2, hid2, x1, w1, b1, lnw, lnb, w_ih, w_hh, b_ih, b_hh, w2, b2 = ctx.saved_tensors
        rows, o = obs2.shape
        n, dev = ctx.n_agents, obs2.device
        dm = dmeans.reshape(rows).contiguous()
        dx1 = torch.empty_like(x1)
        xn = torch.empty_like(x1)
        dg = torch.empty(rows, 256, dtype=torch.float32, device=dev)
        small = torch.empty(512, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            scratch = torch.empty(max(1, lib.mapdn_policy_backward_scratch_floats(rows)), dtype=torch.float32, device=dev)
            _lib.check(lib.mapdn_policy_backward(dm.data_ptr(), x1.data_ptr(), hid2.data_ptr(), lnw.data_ptr(), lnb.data_ptr(), ctx.eps, w_ih.data_ptr(),
                                                 w_hh.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr(), w2.data_ptr(), dx1.data_ptr(), dg.data_ptr(), xn.data_ptr(),
                                                 small.data_ptr(), scratch.data_ptr(), rows, torch.cuda.current_stream(dev).cuda_stream))
        dw_ih = _splitk_dw(dg[:, :192], xn)
        dw_hh = torch.cat((_splitk_dw(dg[:, :128], hid2), _splitk_dw(dg[:, 192:], hid2)), 0)
        db_ih = small[:192].clone()
        db_hh = torch.cat((small[:128], small[192:256]))
        dw1 = torch.empty_like(w1)
        dw1[:, :o] = _splitk_dw(dx1, obs2)
        per_agent = dx1.view(-1, n, 64).sum(0)                   # [n, 64]: sum over the batch for every agent
        if ctx.ids:
            dw1[:, o:] = per_agent.t()
        db1 = per_agent.sum(0)
        return (None, None, None, None, None, dw1, db1, small[256:320], small[320:384], dw_ih, dw_hh, db_ih, db_hh, small[384:448].view(1, 64),
                small[448:449])


class RNNAgent(nn.Module):
    """fc1 -> LayerNorm -> act -> GRUCell -> fc2 (agents/rnn_agent.py:5-32)."""

    def __init__(self, input_shape: int, args):
        super().__init__()
        self.hid_size = args.hid_size
        self.fc1 = nn.Linear(input_shape, args.hid_size)
        if args.layernorm:
            self.layernorm = nn.LayerNorm(args.hid_size)
        self.rnn = nn.GRUCell(args.hid_size, args.hid_size)
        self.fc2 = nn.Linear(args.hid_size, args.action_dim)
        self.use_ln = bool(args.layernorm)
        self.act = _activation(args.hid_activation)

    def trunk(self, x: torch.Tensor, hidden: torch.Tensor):
        """x: pre-activation of fc1, [rows, hid]"""
        x = layernorm_act(self.layernorm, self.act, x) if self.use_ln else self.act(x)
        h = gru_cell_tall(self.rnn, x, hidden.reshape(-1, self.hid_size))
        return tall_linear(self.fc2, h), h

    def forward(self, inputs, hidden):
        a, h = self.trunk(self.fc1(inputs), hidden)
        return a, None, h


class MLPCritic(nn.Module):
    """fc1 -> LayerNorm -> act -> fc2 -> act -> fc3 (critics/mlp_critic.py:7-36)."""

    def __init__(self, input_shape: int, output_shape: int, args):
        super().__init__()
        self.fc1 = nn.Linear(input_shape, args.hid_size)
        if args.layernorm:
            self.layernorm = nn.LayerNorm(args.hid_size)
        self.fc2 = nn.Linear(args.hid_size, args.hid_size)
        self.fc3 = nn.Linear(args.hid_size, output_shape)
        self.use_ln = bool(args.layernorm)
        self.act = _activation(args.hid_activation)

    def trunk(self, x: torch.Tensor):
        if critic_head_ok(self, x, x.shape[0]):
            return critic_head(self, x), None                      # (no caller uses the hidden activation)
        x = layernorm_act(self.layernorm, self.act, x) if self.use_ln else self.act(x)
        return self.head(x)

    def head(self, x: torch.Tensor):
        """what follows the first layer's LayerNorm + activation: fc2 -> act -> fc3"""
        pre = tall_linear(self.fc2, x)
        if relu_dot64_ok(self.act, self.fc3, pre):
            return _ReluDot64.apply(pre, self.fc3.weight, self.fc3.bias), None      # (no caller uses the hidden activation)
        h = self.act(pre)
        return tall_linear(self.fc3, h), h

    def forward(self, inputs, hidden=None):
        return self.trunk(self.fc1(inputs))


class DDPGNet(nn.Module):
    """`MADDPG(Model)` (models/maddpg.py:10), `IDDPG(Model)` (models/iddpg.py:9), `MATD3(Model)` (models/matd3.py:10): behaviour net
    holding its target net, the per-agent reward BatchNorm (models/model.py:26) and the DDPG loss.  `COMA(Model)` is the subclass COMANet."""

    ALGS = ("maddpg", "iddpg", "matd3")         # the algorithms this class is; COMANet (below) is "coma"; net_class(alg) picks the class

    def __init__(self, args, alg: str = "maddpg", target_net: Optional["DDPGNet"] = None):
        super().__init__()
        if alg not in self.ALGS:
            raise KeyError(alg)                                    # models/model_registry.py:14-25
        self.args, self.alg = args, alg
        self.n_, self.obs_dim, self.act_dim, self.hid_dim = args.agent_num, args.obs_size, args.action_dim, args.hid_size
        self._fused_fits = None                   # does the one-launch HIP policy forward have a launch shape for this obs width?
        n, o, a = self.n_, self.obs_dim, self.act_dim
        ids = n if args.agent_id else 0
        self.batchnorm = nn.BatchNorm1d(n)
        # advantage normalisation: MADDPG re-uses `batchnorm` (maddpg.py:17,120); IDDPG's lives in its DDPG
        # helper object, which is not an nn.Module — so it is NOT part of the state_dict (ddpg.py:10,34)
        # (MATD3's is `batchnorm` too: matd3.py:18,146-147; COMA's as well: coma.py:19,183-184)
        self.__dict__["_adv_batchnorm"] = self.batchnorm if alg in ("maddpg", "matd3", "coma") else nn.BatchNorm1d(n)
        critic_in = {"maddpg": (o + a) * n + ids, "iddpg": o + a + ids, "matd3": (o + a) * n + ids + 1,
                     "coma": (n + 1) * o + n * a + ids}[alg]       # maddpg.py:20-24, iddpg.py:19-23, matd3.py:20-25, coma.py:21-27
        copies = 1 if args.shared_params else n
        self.value_dicts = nn.ModuleList([MLPCritic(critic_in, 1, args) for _ in range(copies)])
        self.policy_dicts = nn.ModuleList([RNNAgent(o + ids, args) for _ in range(copies)])   # model.py:141-164
        self.apply(self._init_weights)
        if target_net is not None:
            self.target_net = target_net
            self.reload_params_to_target()

    # ---- initialisation / target handling (models/model.py:28-48,169-177) ----------------------
    def _init_weights(self, m):
        if type(m) == nn.Linear:
            if self.args.init_type == "normal":
                nn.init.normal_(m.weight, 0.0, self.args.init_std)
            elif self.args.init_type == "orthogonal":
                nn.init.orthogonal_(m.weight, gain=nn.init.calculate_gain(self.args.hid_activation))

    def reload_params_to_target(self):
        self.target_net.policy_dicts.load_state_dict(self.policy_dicts.state_dict())
        self.target_net.value_dicts.load_state_dict(self.value_dicts.state_dict())

    @torch.no_grad()
    def update_target(self):
        """soft update over every state_dict entry of the policy and value nets (model.py:34-48)"""
        lr = self.args.target_lr
        for mine, theirs in ((self.policy_dicts, self.target_net.policy_dicts), (self.value_dicts, self.target_net.value_dicts)):
            src = mine.state_dict()
            for name, param in theirs.state_dict().items():
                param.copy_((1 - lr) * param + lr * src[name])

    def init_hidden(self, batch: int = 1):
        return self.policy_dicts[0].fc1.weight.new_zeros(batch, self.n_, self.hid_dim)    # rnn_agent.py:22-24

    # ---- policy (models/model.py:101-139) --------------------------------------------------------
    def _fused_policy_ok(self, obs: torch.Tensor, last_hid: torch.Tensor) -> bool:
        """the one-launch HIP forward (libmapdn_hip.so: mapdn_policy_forward) covers the reference's default agent — shared
        parameters, LayerNorm, ReLU, hidden size 64, one action — for inference on the GPU in fp32"""
        a = self.args
        if not (not torch.is_grad_enabled() and obs.is_cuda and obs.dtype == torch.float32 and last_hid.dtype == torch.float32
                and a.shared_params and a.layernorm and a.hid_activation == "relu" and self.hid_dim == 64 and self.act_dim == 1
                and os.environ.get("MAPDN_FUSED_POLICY", "1") != "0"):
            return False
        if self._fused_fits is None:              # the parameter set + activations of one tile must fit a CU's LDS (wide observations,
            from . import _lib                    # e.g. history > 1 on the 322-bus net, do not): those keep the PyTorch modules
            self._fused_fits = bool(_lib.load().mapdn_policy_forward_fits(self.obs_dim, self.n_ if a.agent_id else 0))
        return self._fused_fits

    def _fused_policy(self, obs: torch.Tensor, last_hid: torch.Tensor, need_hidden: bool = True):
        from . import _lib
        ag = self.policy_dicts[0]
        b, n, o = obs.shape[0], self.n_, self.obs_dim
        obs_c, hid_c = obs.contiguous(), last_hid.contiguous()
        means = torch.empty(b, n, 1, dtype=torch.float32, device=obs.device)
        hid = torch.empty(b, n, self.hid_dim, dtype=torch.float32, device=obs.device) if need_hidden else None
        keep = []                                  # contiguous views stay referenced until the launch is enqueued

        def P(t):
            keep.append(t.detach().contiguous())
            return keep[-1].data_ptr()
        ids = n if self.args.agent_id else 0
        with torch.cuda.device(obs.device):
            _lib.check(_lib.load().mapdn_policy_forward(
                obs_c.data_ptr(), hid_c.data_ptr(), P(ag.fc1.weight), P(ag.fc1.bias), P(ag.layernorm.weight), P(ag.layernorm.bias),
                P(ag.rnn.weight_ih), P(ag.rnn.weight_hh), P(ag.rnn.bias_ih), P(ag.rnn.bias_hh), P(ag.fc2.weight), P(ag.fc2.bias),
                means.data_ptr(), hid.data_ptr() if hid is not None else None, b * n, n, o, ids, float(ag.layernorm.eps),
                torch.cuda.current_stream(obs.device).cuda_stream))
        return means, torch.full_like(means, math.log(self.args.fixed_policy_std)), hid

    def _fused_policy_train_ok(self, obs: torch.Tensor, last_hid: torch.Tensor) -> bool:
        a = self.args
        if not (torch.is_grad_enabled() and obs.is_cuda and obs.dtype == torch.float32 and last_hid.dtype == torch.float32 and a.shared_params
                and a.layernorm and a.hid_activation == "relu" and self.hid_dim == 64 and self.act_dim == 1 and not last_hid.requires_grad
                and not obs.requires_grad and obs.shape[0] * self.n_ >= 4096 and os.environ.get("MAPDN_FUSED_POLICY_TRAIN", "1") != "0"):
            return False
        if self._fused_fits is None:
            from . import _lib
            self._fused_fits = bool(_lib.load().mapdn_policy_forward_fits(self.obs_dim, self.n_ if a.agent_id else 0))
        return self._fused_fits

    def policy(self, obs: torch.Tensor, last_hid: torch.Tensor, means_grad_only: bool = False):
        """obs [b, n, o], last_hid [b, n, h] -> means [b, n, a], log_stds, hiddens [b, n, h].  means_grad_only: the caller differentiates the
        means alone (the policy loss; the new hidden state is then not returned) — the HIP forward / backward pair of _PolicyTrunk."""
        b, n, o = obs.shape[0], self.n_, self.obs_dim
        if self._fused_policy_ok(obs, last_hid):
            return self._fused_policy(obs, last_hid, need_hidden=not means_grad_only)
        if means_grad_only and self._fused_policy_train_ok(obs, last_hid):
            ag = self.policy_dicts[0]
            means = _PolicyTrunk.apply(obs.reshape(b * n, o), last_hid.reshape(b * n, -1), n, n if self.args.agent_id else 0, ag.layernorm.eps,
                                       ag.fc1.weight, ag.fc1.bias, ag.layernorm.weight, ag.layernorm.bias, ag.rnn.weight_ih, ag.rnn.weight_hh,
                                       ag.rnn.bias_ih, ag.rnn.bias_hh, ag.fc2.weight, ag.fc2.bias).view(b, n, 1)
            return means, torch.full_like(means, math.log(self.args.fixed_policy_std)), None
        if self.args.shared_params:
            ag = self.policy_dicts[0]
            w = ag.fc1.weight
            if _tall_ok(obs, b * n, w):                                  # (the policy update on a replay batch: weight gradient over b * n rows)
                x = _TallLinear.apply(obs.reshape(b * n, o), w[:, :o], ag.fc1.bias).view(b, n, -1)
            else:
                x = F.linear(obs, w[:, :o], ag.fc1.bias)                 # observation columns
            if self.args.agent_id:
                x = x + w[:, o:].t().unsqueeze(0)                        # one-hot id i selects column o + i
            means, hid = ag.trunk(x.reshape(b * n, -1), last_hid)
            means, hid = means.view(b, n, -1), hid.view(b, n, -1)
            log_stds = torch.full_like(means, math.log(self.args.fixed_policy_std))       # model.py:119-120
        else:
            ms, hs = [], []
            for i, ag in enumerate(self.policy_dicts):
                w = ag.fc1.weight
                x = F.linear(obs[:, i], w[:, :o], ag.fc1.bias)
                if self.args.agent_id:
                    x = x + w[:, o + i]
                m, h = ag.trunk(x, last_hid[:, i])
                ms.append(m); hs.append(h)
            means, hid = torch.stack(ms, 1), torch.stack(hs, 1)
            log_stds = torch.zeros_like(means)                            # model.py:134-135
        return means, log_stds, hid

    # ---- critics ---------------------------------------------------------------------------------
    def value(self, obs: torch.Tensor, act: torch.Tensor, own_action_only: bool = False) -> torch.Tensor:
        """obs [b, n, o], act [b, n, a] -> [b, n, 1].  own_action_only: the caller differentiates with respect to `act` alone (the policy
        loss): the central critic may then skip the gradients of its own parameters, which the policy optimiser never reads."""
        if self.alg == "iddpg":
            return self._value_independent(obs, act)
        if self.alg == "coma":
            return self._value_coma(obs, act)
        if self.alg == "matd3" and not own_action_only:            # matd3.py:86: [2b, n, 1] = values1 over values2
            return torch.cat(self._value_twin(obs, act), 0)
        return self._value_central(obs, act, own_action_only)      # (MATD3's policy loss reads the first head only — flag column times 0)

    def _independent_first_layer(self, cr, obs, act):
        """IDDPG's shared critic, first layer on [obs_i | id_i | act_i] (iddpg.py:32-58) as  W_obs obs + id column + W_act act, [b, n, h];
        on a tall GPU batch the observation product takes _TallLinear (its weight gradient is a [h, o] product with b * n rows of
        reduction, which the BLAS back end runs on two workgroups)"""
        b, n, o = obs.shape[0], self.n_, self.obs_dim
        ids = n if self.args.agent_id else 0
        w = cr.fc1.weight
        if _tall_ok(obs, b * n, w):
            x = _TallLinear.apply(obs.reshape(b * n, o), w[:, :o], cr.fc1.bias)
            if self.act_dim == 1:        # a one-column product is an outer product: one fused multiply-add pass instead of a GEMM + an add
                x = torch.addcmul(x, act.reshape(b * n, 1), w[:, o + ids:].t()).view(b, n, -1)
            else:
                x = (x + _TallLinear.apply(act.reshape(b * n, -1), w[:, o + ids:], None)).view(b, n, -1)
        else:
            x = F.linear(obs, w[:, :o], cr.fc1.bias) + F.linear(act, w[:, o + ids:])
        if ids:
            x = x + w[:, o:o + n].t().unsqueeze(0)
        return x

    def _value_independent(self, obs, act):
        """IDDPG (iddpg.py:32-58): critic input [obs_i | id_i | act_i]"""
        b, n, o = obs.shape[0], self.n_, self.obs_dim
        ids = n if self.args.agent_id else 0

        def first_layer(cr, ob, ac, who):
            w = cr.fc1.weight
            x = F.linear(ob, w[:, :o], cr.fc1.bias) + F.linear(ac, w[:, o + ids:])
            if ids:
                x = x + (w[:, o:o + n].t().unsqueeze(0) if who is None else w[:, o + who])
            return x

        if self.args.shared_params:
            cr = self.value_dicts[0]
            v, _ = cr.trunk(self._independent_first_layer(cr, obs, act).reshape(b * n, -1))
            return v.view(b, n, -1)
        return torch.stack([cr.trunk(first_layer(cr, obs[:, i], act[:, i], i))[0] for i, cr in enumerate(self.value_dicts)], 1)

    def _central_first_layer(self, cr, obs_all, act_all, own, who, obs_term=None):
        """first layer of a central critic (maddpg.py:35-79, matd3.py:35-69 with the flag column at 0) = W_obs·obs_all + b1 + W_id[:, i]
        + W_act·act_all, where the joint action enters detached and agent i's own (act_i - act_i.detach()) — zero in value — restores
        its gradient path; [b, n, h] for who None, [b, h] for agent `who`.  obs_term: W_obs·obs_all + b1 when the caller holds it."""
        b, n, o, a = obs_all.shape[0], self.n_, self.obs_dim, self.act_dim
        ids = n if self.args.agent_id else 0
        w = cr.fc1.weight
        w_act = w[:, n * o + ids:n * o + ids + n * a]
        base = (F.linear(obs_all, w[:, :n * o], cr.fc1.bias) if obs_term is None else obs_term) + F.linear(act_all.detach(), w_act)      # [b, h]
        if who is None:                                              # all agents at once: [b, n, h]
            x = base.unsqueeze(1)
            if ids:
                x = x + w[:, n * o:n * o + n].t().unsqueeze(0)
            else:
                x = x.expand(b, n, -1)
            if own is not None:
                x = x + torch.einsum("bna,hna->bnh", own, w_act.reshape(-1, n, a))
            return x
        x = base + w[:, n * o + who] if ids else base
        if own is not None:
            x = x + F.linear(own[:, who], w_act[:, who * a:(who + 1) * a])
        return x

    def _value_central(self, obs, act, own_action_only=False):
        """MADDPG (maddpg.py:35-79): agent i's critic sees [all obs | id_i | all actions] and only its OWN
        action carries gradient.  First layer = W_obs·obs_all + W_id[:, i] + W_act·act_all, where the joint
        action enters detached and agent i's own (act_i - act_i.detach()) — zero in value — restores its
        gradient path; no [b, n, n·o] tensor is ever built."""
        b, n, o, a = obs.shape[0], self.n_, self.obs_dim, self.act_dim
        ids = n if self.args.agent_id else 0
        obs_all, act_all = obs.reshape(b, n * o), act.reshape(b, n * a)
        own = (act - act.detach()) if act.requires_grad else None
        na = n * o + ids + n * a                                         # end of the action columns (MATD3: the flag column follows)

        def first_layer(cr, who):
            return self._central_first_layer(cr, obs_all, act_all, own, who)

        if self.args.shared_params:
            cr = self.value_dicts[0]
            if ids and cr.use_ln and own is not None and a == 1 and own_action_only and critic_head_ok(cr, obs_all.new_empty(0, 64), b * n, n):
                # the policy update (maddpg.py:52-58, 103-125): value = the head on base[b] + id_column[i] (the own-action term is zero in
                # value), gradient = d/d act[b, i] only, from the kernel; the critic's own parameters are not differentiated
                w = cr.fc1.weight.detach()
                with torch.no_grad():
                    base = F.linear(obs_all, w[:, :n * o], cr.fc1.bias.detach()) + F.linear(act_all.detach(), w[:, n * o + ids:na])
                ln = cr.layernorm
                v = _CriticHeadOwnAction.apply(act, base, w[:, n * o:n * o + n].t(), w[:, n * o + ids:na].t(), ln.weight, ln.bias, ln.eps,
                                               cr.fc2.weight, cr.fc2.bias, cr.fc3.weight, cr.fc3.bias)
                return v.view(b, n, 1)
            if ids and own is None and cr.use_ln:
                # no gradient path through the actions (value loss, target values): the first layer's output is base[b] + id_column[i] —
                # LayerNorm + ReLU straight from the two small operands, the [b, n, h] sum is never written
                w = cr.fc1.weight
                base = tall_linear_w(obs_all, w[:, :n * o], cr.fc1.bias) + tall_linear_w(act_all.detach(), w[:, n * o + ids:na])
                if critic_head_ok(cr, base, b * n, n):
                    return critic_head(cr, base, w[:, n * o:n * o + n].t()).view(b, n, 1)
                xn = layernorm_act_bc(cr.layernorm, cr.act, base, w[:, n * o:n * o + n].t())
                if xn is not None:
                    return cr.head(xn)[0].view(b, n, 1)
            v, _ = cr.trunk(first_layer(cr, None).reshape(b * n, -1))
            return v.view(b, n, 1)
        return torch.stack([cr.trunk(first_layer(cr, i))[0] for i, cr in enumerate(self.value_dicts)], 1)

    def _value_twin(self, obs, act, want="both", obs_term=None):
        """MATD3 (matd3.py:35-86): the central critic valued twice, its input one column wider — 0 for values1, 1 for values2 —, i.e.
        first layer = that of _value_central, and the same + fc1.weight[:, -1].  Returns (values1, values2), each [b, n, 1], or with
        want="min" their minimum (matd3.py:141-142).  obs_term [b, h]: W_obs·obs_all + b1 of the shared critic when the caller holds it
        (PGTrainer caches it per update round).  Without a gradient path the default critic on the GPU takes ONE launch for both heads."""
        b, n, o, a = obs.shape[0], self.n_, self.obs_dim, self.act_dim
        ids = n if self.args.agent_id else 0
        obs_all, act_all = obs.reshape(b, n * o), act.reshape(b, n * a)
        own = (act - act.detach()) if act.requires_grad else None
        out = (lambda v1, v2: torch.minimum(v1, v2)) if want == "min" else (lambda v1, v2: (v1, v2))
        if self.args.shared_params:
            cr = self.value_dicts[0]
            w = cr.fc1.weight
            flag = w[:, -1]
            if ids and own is None and cr.use_ln:
                w_act = w[:, n * o + ids:n * o + ids + n * a]
                base = (tall_linear_w(obs_all, w[:, :n * o], cr.fc1.bias) if obs_term is None else obs_term) + tall_linear_w(act_all.detach(), w_act)
                per_n = w[:, n * o:n * o + n].t()
                if not (torch.is_grad_enabled() and (base.requires_grad or w.requires_grad)) and critic_twin_ok(cr, base, b * n, n):
                    if want == "min":
                        return critic_twin_forward(cr, base, per_n, flag, ("vmin",))["vmin"].view(b, n, 1)
                    r = critic_twin_forward(cr, base, per_n, flag, ("v1", "v2"))
                    return r["v1"].view(b, n, 1), r["v2"].view(b, n, 1)
                if critic_head_ok(cr, base, b * n, n):
                    return out(critic_head(cr, base, per_n).view(b, n, 1), critic_head(cr, base, per_n + flag).view(b, n, 1))
            x = self._central_first_layer(cr, obs_all, act_all, own, None, obs_term)
            return out(cr.trunk(x.reshape(b * n, -1))[0].view(b, n, 1), cr.trunk((x + flag).reshape(b * n, -1))[0].view(b, n, 1))
        xs = [self._central_first_layer(cr, obs_all, act_all, own, i) for i, cr in enumerate(self.value_dicts)]
        return out(torch.stack([cr.trunk(x)[0] for x, cr in zip(xs, self.value_dicts)], 1),
                   torch.stack([cr.trunk(x + cr.fc1.weight[:, -1])[0] for x, cr in zip(xs, self.value_dicts)], 1))

    def value_mse(self, obs, act, returns, valid=None):
        """mean over (batch, agent) of (returns - Q(obs, act))^2 — the value loss of maddpg.py:122-124 / ddpg.py:36-38 — weighted by
        `valid` [b] when given (1 everywhere = the reference).  With the default critic on the GPU the loss and its gradients come out of
        ONE head launch (_CriticHeadMSE); otherwise value() + the plain expression."""
        b, n, o = obs.shape[0], self.n_, self.obs_dim
        a = self.args
        ids = n if a.agent_id else 0
        if (a.shared_params and torch.is_grad_enabled() and not act.requires_grad and obs.is_cuda
                and os.environ.get("MAPDN_FUSED_MSE", "1") != "0"):
            cr = self.value_dicts[0]
            w = cr.fc1.weight
            x = per_n = None
            if self.alg in ("maddpg", "matd3") and ids and cr.use_ln:
                x = tall_linear_w(obs.reshape(b, n * o), w[:, :n * o], cr.fc1.bias) \
                    + tall_linear_w(act.reshape(b, n * self.act_dim), w[:, n * o + ids:n * o + ids + n * self.act_dim])
                per_n = w[:, n * o:n * o + n].t()
            elif self.alg == "iddpg":
                x = self._independent_first_layer(cr, obs, act).reshape(b * n, -1)
            elif self.alg == "coma" and cr.use_ln:                 # coma.py:179-180: the same loss on rows that are read, as IDDPG's
                x = self._coma_first_layer(cr, obs, act).reshape(b * n, -1)
            twin = self.alg == "matd3"
            if x is not None and (critic_twin_ok(cr, x, b * n, n) if twin else critic_head_ok(cr, x, b * n, n if per_n is not None else 0)):
                if valid is None:
                    scale, wrow = x.new_full((1,), 1.0 / (b * n)), None
                else:
                    vf = valid.float().view(-1)
                    scale = (1.0 / (vf.sum().clamp(min=1.0) * n)).reshape(1)
                    wrow = vf if per_n is not None else vf.repeat_interleave(n)
                ln = cr.layernorm
                if twin and os.environ.get("MAPDN_TWIN_MSE_KERNEL", "0") == "1":      # both heads in ONE launch: measured slower than the pair below
                    return _CriticTwinMSE.apply(x, per_n, w[:, -1], ln.weight, ln.bias, ln.eps, cr.fc2.weight, cr.fc2.bias, cr.fc3.weight, cr.fc3.bias,
                                                returns, wrow, scale)
                if twin:
                    # matd3.py:143-150, both heads against the same returns: two single-head loss launches, on per_n and on per_n + w_flag,
                    # each with half the weight; autograd sums the two dbase and hands the second dper_n's column sum to w_flag
                    twin_pair_mse.launches += 1
                    head = (ln.weight, ln.bias, ln.eps, cr.fc2.weight, cr.fc2.bias, cr.fc3.weight, cr.fc3.bias, returns, wrow, 0.5 * scale)
                    return _CriticHeadMSE.apply(x, per_n, *head) + _CriticHeadMSE.apply(x, per_n + w[:, -1], *head)
                return _CriticHeadMSE.apply(x, per_n, ln.weight, ln.bias, ln.eps, cr.fc2.weight, cr.fc2.bias, cr.fc3.weight, cr.fc3.bias,
                                            returns, wrow, scale)
        wm = (lambda d2: d2.mean()) if valid is None else \
            (lambda d2: (d2 * valid.float().view(-1, 1)).sum() / (valid.float().sum().clamp(min=1.0) * d2.shape[1]))
        if self.alg == "matd3":                          # matd3.py:143-150
            v1, v2 = self._value_twin(obs, act)
            return 0.5 * (wm((returns - v1.view(-1, n)).pow(2)) + wm((returns - v2.view(-1, n)).pow(2)))
        values = self.value(obs, act).view(-1, n)
        d2 = (returns - values).pow(2)
        return d2.mean() if valid is None else (d2 * valid.float().view(-1, 1)).sum() / (valid.float().sum().clamp(min=1.0) * d2.shape[1])

    # ---- action selection (maddpg.py:81-101 == iddpg.py:60-80; utilities/util.py:52-98) ----------
    def get_actions(self, state, status, exploration, actions_avail, target=False, last_hid=None, means_grad_only=False, clip=False, noise=None):
        net = self.target_net if (target and self.args.target) else self
        means, log_stds, hiddens = net.policy(state, last_hid, means_grad_only)
        if means.size(-1) > 1:                                   # maddpg.py:85-87 (action_dim > 1 sums over agents)
            means_, log_stds_ = means.sum(dim=1, keepdim=True), log_stds.sum(dim=1, keepdim=True)
        else:
            means_, log_stds_ = means, log_stds
        actions, log_prob = self._select_action(means_, log_stds_, status, exploration, clip, noise)
        restore_mask = 1.0 - (actions_avail == 0).to(actions.dtype)
        return actions, restore_mask * actions, log_prob, (means, log_stds), hiddens

    def _select_action(self, mean, log_std, status, exploration, clip=False, noise=None):
        """utilities/util.py:52-87.  clip (matd3.py:119-124 passes True for the next actions) is read ONLY without action_enforcebound: the
        bounded branch ignores it (util.py:58-66), as the reference does.  noise: the standard-normal draw to use instead of drawing."""
        a = self.args
        draw = (lambda: torch.randn_like(mean)) if noise is None else (lambda: noise.to(mean.dtype).view_as(mean))
        if status == "train":
            if not exploration:
                return mean, None
            std = log_std.exp()
            if a.action_enforcebound:                            # util.py:57-66
                x_t = mean + std * draw()                        # Normal(mean, std).rsample()
                y_t = torch.tanh(x_t)
                log_prob = -((x_t - mean) ** 2) / (2 * std ** 2) - log_std - math.log(math.sqrt(2 * math.pi))
                return y_t, log_prob - torch.log(1 - y_t.pow(2) + 1e-6)
            x_t = std * draw()                                   # util.py:67-76
            log_prob = -(x_t ** 2) / (2 * std ** 2) - log_std - math.log(math.sqrt(2 * math.pi))
            if clip:
                return mean + torch.clamp(x_t, min=-a.clip_c, max=a.clip_c), log_prob
            return mean + x_t, log_prob
        if status == "test":                                     # util.py:80-87
            return (torch.tanh(mean) if a.action_enforcebound else mean), None
        raise ValueError(status)

    # ---- loss (models/maddpg.py:103-125 == learning_algorithms/ddpg.py:15-39) ----------------------
    def normalise_reward(self, reward: torch.Tensor) -> torch.Tensor:
        """model.py:316-317: BatchNorm1d over the batch, per agent.  Data-parallel ranks (PGTrainer sets `_dp_all_reduce`) normalise with
        the statistics of the UNION of their batches — one small all-reduce of (count, sum, sum of squares) — so that an N-rank update
        equals the one-rank update on the concatenated batch and the running statistics stay identical on every replica."""
        if not self.args.reward_normalisation:
            return reward
        return self._union_batchnorm(self.batchnorm, reward)

    def _union_batchnorm(self, bn: nn.BatchNorm1d, reward: torch.Tensor) -> torch.Tensor:
        """bn(x) for x [batch, n]; in training mode under data-parallel training with the statistics of the union of the ranks' batches
        (see normalise_reward).  MAPPO / IPPO's advantage BatchNorm goes through it as well."""
        red = self.__dict__.get("_dp_all_reduce")
        if red is None or not bn.training:
            return bn(reward)
        x = reward.double()
        st = torch.cat((x.new_full((1,), float(x.shape[0])), x.sum(0), (x * x).sum(0)))
        red(st)
        cnt, n = st[0], x.shape[1]
        mean = st[1:1 + n] / cnt
        var = (st[1 + n:] / cnt - mean * mean).clamp(min=0.0)                      # biased, as BatchNorm normalises with
        with torch.no_grad():
            m = bn.momentum if bn.momentum is not None else 0.1
            bn.running_mean.mul_(1 - m).add_(m * mean.to(bn.running_mean.dtype))
            bn.running_var.mul_(1 - m).add_(m * (var * cnt / (cnt - 1).clamp(min=1.0)).to(bn.running_var.dtype))
            bn.num_batches_tracked += 1
        y = (reward - mean.to(reward.dtype)) * torch.rsqrt(var.to(reward.dtype) + bn.eps)
        return y * bn.weight + bn.bias

    def smoothed_actions(self, means: torch.Tensor, avail: torch.Tensor, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """MATD3's next actions from the next-state policy means (matd3.py:119-124: exploration=True, clip=True — see _select_action for
        what clip does), with the restore mask of get_actions; one [bs, n, 1] draw unless `noise` is given"""
        assert means.size(-1) == 1, "one action per agent (get_actions sums wider means and log_stds over the agents: not built here)"
        log_std = torch.full_like(means, math.log(self.args.fixed_policy_std)) if self.args.shared_params else torch.zeros_like(means)
        actions, _ = self._select_action(means, log_std, "train", True, True, noise)
        return (1.0 - (avail == 0).to(actions.dtype)) * actions

    def _matd3_next_values(self, batch: Batch) -> torch.Tensor:
        """min(Q1', Q2') of the target critic at the smoothed next actions (matd3.py:119-142).  The noise is drawn anew in every call, after
        the noise-free policy forward; batch["next_noise"] [bs, n, 1] replaces the draw.  PGTrainer hands over what does not change within
        an update round: the policy means (next_mean_cached) and the target critic's observation term (next_obs_term_cached)."""
        pol = self if self.args.double_q else (self.target_net if self.args.target else self)
        means = batch["next_mean_cached"] if "next_mean_cached" in batch else pol.policy(batch["next_state"], batch["hid"], True)[0]
        next_actions = self.smoothed_actions(means, batch["action_avail"], batch.get("next_noise"))
        return self.target_net._value_twin(batch["next_state"], next_actions, "min", batch.get("next_obs_term_cached"))

    def get_loss(self, batch: Batch, want=("policy", "value")):
        """batch: state/next_state [bs, n, o], action/action_avail [bs, n, a], reward [bs, n], done [bs, 1],
        last_hid/hid [bs, n, h] float32 (the `unpack_data` tensors, model.py:304-319); optional `valid`
        [bs] weights the means (1 everywhere = the reference); MATD3: optional `next_noise` [bs, n, 1] (see _matd3_next_values); COMA:
        optional `cf_noise` [S, bs, n, a] (see _coma_policy_loss; its loss is coma.py:128-191, the value half shared with the others).  Returns (policy_loss, value_loss,
        (means, log_stds)); a loss not in `want` is None and its forward passes are skipped."""
        n = self.n_
        state, actions, next_state = batch["state"], batch["action"], batch["next_state"]
        avail, last_hid, hid = batch["action_avail"], batch["last_hid"], batch["hid"]
        rewards = self.normalise_reward(batch["reward"].float())
        done = batch["done"].float().view(-1, 1)
        valid = batch.get("valid")
        wmean = (lambda t: t.mean()) if valid is None else \
            (lambda t: (t * valid.float().view(-1, 1)).sum() / (valid.float().sum().clamp(min=1.0) * t.shape[1]))
        policy_loss = value_loss = action_out = None
        if self.alg == "coma":
            policy_loss, action_out = self._coma_policy_loss(batch, wmean, "policy" in want)
        elif "policy" in want:
            _, actions_pol, _, action_out, _ = self.get_actions(state, "train", False, avail, False, last_hid, means_grad_only=True)
            advantages = self.value(state, actions_pol, own_action_only=True).view(-1, n)
            if self.args.normalize_advantages:
                advantages = self._adv_batchnorm.to(advantages.device)(advantages)
            policy_loss = wmean(-advantages)
        elif self.alg == "matd3" and self.args.normalize_advantages and self.batchnorm.training:
            # the reference evaluates BOTH losses in every get_loss call (matd3.py:113-151), so with normalize_advantages its `batchnorm`
            # — part of the state_dict — sees the advantages in the value updates too: keep its running statistics the reference's
            with torch.no_grad():
                _, a_pol, _, _, _ = self.get_actions(state, "train", False, avail, False, last_hid, means_grad_only=True)
                self._adv_batchnorm.to(a_pol.device)(self.value(state, a_pol, own_action_only=True).view(-1, n))
        if "value" in want:
            with torch.no_grad():
                if self.alg == "matd3":
                    next_values = self._matd3_next_values(batch).view(-1, n)
                elif "next_value_cached" in batch:                 # PGTrainer precomputed both for the whole replay ring (same values)
                    next_values = batch["next_value_cached"].view(-1, n)
                else:
                    if "next_action_cached" in batch:
                        next_actions = batch["next_action_cached"]
                    else:
                        _, next_actions, _, _, _ = self.get_actions(next_state, "train", False, avail,
                                                                    not self.args.double_q, hid)
                    next_values = self.target_net.value(next_state, next_actions).view(-1, n)
                returns = rewards + self.args.gamma * (1 - done) * next_values
            value_loss = self.value_mse(state, actions, returns, valid)
        return policy_loss, value_loss, action_out


class COMANet(DDPGNet):
    """`COMA(Model)` (models/coma.py:11): the policy, target handling, reward BatchNorm and value half of the loss are DDPGNet's; the
    critic input, the counterfactual baseline and the policy loss are its own.  On-policy: PGTrainer empties the replay ring after every
    update round (models/model.py:53-56)."""
    ALGS = ("coma",)

    def __init__(self, args, alg: str = "coma", target_net: Optional["COMANet"] = None):
        if alg in self.ALGS and int(args.sample_size) < 2:
            # coma.py:44 tells the sampled actions [S b, n, n a] from taken ones [b, n, a] by the batch dimension: equal at S == 1
            raise ValueError(f"sample_size must be at least 2 for COMA (got {args.sample_size})")
        super().__init__(args, alg, target_net)

    def _coma_first_layer(self, cr, obs, act, who=None):
        """first layer of COMA's critic on [all obs (n o) | own obs (o) | ids (n) | joint action (n a)] (coma.py:24, 53-80) as
        W_all·obs_all + b1 + W_act·act_all (per batch element) + W_own·obs[b, i] + id column (per agent): [b, n, h] for who None, [b, h]
        for agent `who`; never built at input width.  Every action carries gradient (coma.py has no detach in value())."""
        b, n, o, a = obs.shape[0], self.n_, self.obs_dim, self.act_dim
        ids = n if self.args.agent_id else 0
        w = cr.fc1.weight
        na = (n + 1) * o + ids
        base = tall_linear_w(obs.reshape(b, n * o), w[:, :n * o], cr.fc1.bias) + tall_linear_w(act.reshape(b, n * a), w[:, na:na + n * a])      # [b, h]
        if who is not None:
            x = base + F.linear(obs[:, who], w[:, n * o:(n + 1) * o])
            return x + w[:, (n + 1) * o + who] if ids else x
        x = tall_linear_w(obs.reshape(b * n, o), w[:, n * o:(n + 1) * o]).view(b, n, -1) + base.unsqueeze(1)
        if ids:
            x = x + w[:, (n + 1) * o:na].t().unsqueeze(0)
        return x

    def _value_coma(self, obs, act):
        """coma.py:43-104 on taken actions (obs and act of the same batch size): [b, n, 1]"""
        b, n = obs.shape[0], self.n_
        if self.args.shared_params:
            cr = self.value_dicts[0]
            return cr.trunk(self._coma_first_layer(cr, obs, act).reshape(b * n, -1))[0].view(b, n, 1)
        return torch.stack([cr.trunk(self._coma_first_layer(cr, obs, act, i))[0] for i, cr in enumerate(self.value_dicts)], 1)

    def sampled_actions(self, means: torch.Tensor, log_stds: torch.Tensor, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """coma.py:139-143: th.normal(means, std) for sample_size repeats of the batch, [S, b, n, a] — ONE draw per get_loss call, taken as
        means + std * randn (the same numbers from the same generator state; tests/golden/make_coma_golden.py asserts it), or with
        `noise` [S, b, n, a] in the place of randn"""
        S = int(self.args.sample_size)
        eps = torch.randn((S,) + tuple(means.shape), dtype=means.dtype, device=means.device) if noise is None else noise.to(means.dtype).view((S,) + tuple(means.shape))
        return means.detach().unsqueeze(0) + log_stds.detach().exp().unsqueeze(0) * eps

    @torch.no_grad()
    def counterfactual(self, obs: torch.Tensor, act: torch.Tensor, sampled: torch.Tensor):
        """(baselines [b, n], values [b, n]) of coma.py:144-152: baselines[b, i] = mean over s of Q_i(obs, act with agent i's action
        replaced by sampled[s, b, i]); values = Q(obs, act).  The critic's first layer is linear in the actions, so the replaced input
        is the taken one plus (sampled - act)[b, i] · W_act[:, i]: the [S b, n, (n + 1) o + n + n a] input of the reference is never
        built.  The default critic on the GPU with one action per agent: ONE launch for all samples and the values
        (critic_counterfactual); otherwise a loop over the samples through the PyTorch modules."""
        b, n, o, a = obs.shape[0], self.n_, self.obs_dim, self.act_dim
        ids = n if self.args.agent_id else 0
        na = (n + 1) * o + ids
        S = sampled.shape[0]
        delta = sampled - act.unsqueeze(0)                                           # [S, b, n, a]
        if self.args.shared_params:
            cr = self.value_dicts[0]
            x = self._coma_first_layer(cr, obs, act).reshape(b * n, -1)
            w_act = cr.fc1.weight[:, na:na + n * a]
            if critic_cf_ok(cr, x, b * n, a):
                base, v0 = critic_counterfactual(cr, x, w_act.t(), delta.reshape(S, b * n))
                return base.view(b, n), v0.view(b, n)
            own_col = w_act.reshape(-1, n, a)                                        # [h, n, a]: agent i's own action columns
            values = cr.trunk(x)[0].view(b, n)
            total = torch.zeros_like(values)
            for s in range(S):
                total += cr.trunk(x + torch.einsum("bna,hna->bnh", delta[s], own_col).reshape(b * n, -1))[0].view(b, n)
            return total / S, values
        xs = [self._coma_first_layer(cr, obs, act, i) for i, cr in enumerate(self.value_dicts)]
        values = torch.stack([cr.trunk(x)[0] for x, cr in zip(xs, self.value_dicts)], 1).view(b, n)
        total = torch.zeros_like(values)
        for s in range(S):
            total += torch.stack([cr.trunk(x + F.linear(delta[s][:, i], cr.fc1.weight[:, na + i * a:na + (i + 1) * a]))[0]
                                  for i, (x, cr) in enumerate(zip(xs, self.value_dicts))], 1).view(b, n)
        return total / S, values

    def _coma_policy_loss(self, batch: Batch, wmean, want_loss: bool):
        """coma.py:131-152, 181-190: policy_loss = -mean(advantages * log_prob), advantages = (Q(s, a) - baseline).detach() (through
        `batchnorm` with normalize_advantages), log_prob of the STORED action under N(mean, std), masked by the available actions.
        The sample_size draws are taken in every call, as the reference does (coma.py:143 runs for the value update too);
        batch["cf_noise"] [S, bs, n, a] replaces the standard-normal draw.  want_loss False (a value update): only what the call
        changes besides the loss is done — the draw, and with normalize_advantages the running statistics of `batchnorm`."""
        n = self.n_
        state, actions, avail = batch["state"], batch["action"], batch["action_avail"]
        if not want_loss and not (self.args.normalize_advantages and self.batchnorm.training):
            if batch.get("cf_noise") is None:                    # the call's one draw, so that the generator goes the reference's way
                torch.randn((int(self.args.sample_size),) + tuple(actions.shape), dtype=torch.float32, device=actions.device)
            return None, None
        with torch.set_grad_enabled(want_loss and torch.is_grad_enabled()):
            means, log_stds, _ = self.policy(state, batch["last_hid"], means_grad_only=True)
        sampled = self.sampled_actions(means, log_stds, batch.get("cf_noise"))
        baselines, values = self.counterfactual(state, actions, sampled)
        advantages = (values - baselines).detach()
        if self.args.normalize_advantages:
            advantages = self._adv_batchnorm.to(advantages.device)(advantages)
        if not want_loss:
            return None, None
        std = log_stds.exp()
        log_prob = -((actions - means) ** 2) / (2 * std ** 2) - log_stds - math.log(math.sqrt(2 * math.pi))      # util.py:44-46
        log_prob = ((1.0 - (avail == 0).to(log_prob.dtype)) * log_prob).sum(-1).view(-1, n)
        return wmean(-advantages * log_prob), (means, log_stds)


# ---- MAAC (models/maac.py, critics/maac_critic.py, agents/rnn_agent_gaussian.py) ---------------------------------------------------
def attention_loop_reference(sel: torch.Tensor, key: torch.Tensor, val: torch.Tensor, H: int):
    """critics/maac_critic.py:120-136 restated literally: per head and per agent, the keys / values of the OTHER agents stacked and
    permuted to [b, d, n - 1], softmax over the last dimension.  (out [b, n, hid], logit_sq [n, H] = the sum of the squared unscaled
    logits.)  What the batched route and the kernels are tested against; never on a training path."""
    b, n, hid = sel.shape
    d = hid // H
    outs, lsq = [[] for _ in range(n)], sel.new_zeros(n, H)
    for h in range(H):
        cols = slice(h * d, (h + 1) * d)
        for i in range(n):
            keys = [key[:, j, cols] for j in range(n) if j != i]
            values = [val[:, j, cols] for j in range(n) if j != i]
            logits = torch.matmul(sel[:, i, cols].reshape(b, 1, -1), torch.stack(keys).permute(1, 2, 0))          # [b, 1, n - 1]
            weights = F.softmax(logits / math.sqrt(d), dim=2)
            outs[i].append((torch.stack(values).permute(1, 2, 0) * weights).sum(dim=2))
            lsq[i, h] = (logits ** 2).sum()
    return torch.stack([torch.cat(o, 1) for o in outs], 1), lsq


def attention_core_torch(sel: torch.Tensor, key: torch.Tensor, val: torch.Tensor, H: int):
    """the same as ONE masked softmax over [b, H, n, n] (the diagonal — an agent's own key — masked out): two batched products, no loop
    over heads or agents.  The CPU route, and the GPU route where the kernels do not apply."""
    b, n, hid = sel.shape
    d = hid // H
    q, k, v = (t.reshape(b, n, H, d).transpose(1, 2) for t in (sel, key, val))                 # [b, H, n, d]
    logits = q @ k.transpose(-1, -2)                                                           # [b, H, n, n]
    own = torch.eye(n, dtype=torch.bool, device=sel.device)
    p = F.softmax((logits / math.sqrt(d)).masked_fill(own, float("-inf")), dim=-1)
    out = (p @ v).transpose(1, 2).reshape(b, n, hid)
    return out, logits.masked_fill(own, 0.0).square().sum(dim=(0, 3)).t()                      # [n, H]


class _AttentionCore(torch.autograd.Function):
    """(out, logit_sq) of attention_core_torch as one HIP launch forward and one backward (libmapdn_hip.so: mapdn_attention_*,
    csrc/critic_attn.hip): a workgroup holds one sample's three [n, 64] operands and its [H, n, n] scores in LDS; the backward recomputes
    the probabilities, so only the operands are saved."""
    launches = 0           # how often the forward kernel was reached (tests count the routes)

    @staticmethod
    def forward(ctx, sel, key, val, H):
        from . import _lib
        lib = _lib.load()
        s, k, v = sel.contiguous(), key.contiguous(), val.contiguous()
        B, n, dev = s.shape[0], s.shape[1], s.device
        out = torch.empty_like(s)
        lsq = torch.empty(n, H, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            scratch = torch.empty(max(1, lib.mapdn_attention_scratch_floats(B, n, H)), dtype=torch.float32, device=dev)
            _lib.check(lib.mapdn_attention_forward(s.data_ptr(), k.data_ptr(), v.data_ptr(), B, n, H, out.data_ptr(), lsq.data_ptr(),
                                                   scratch.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        _AttentionCore.launches += 1
        ctx.save_for_backward(s, k, v)
        ctx.H = H
        return out, lsq

    @staticmethod
    def backward(ctx, dout, dlsq):
        from . import _lib
        lib = _lib.load()
        s, k, v = ctx.saved_tensors
        B, n, dev = s.shape[0], s.shape[1], s.device
        do, dl = dout.contiguous(), dlsq.contiguous()
        ds, dk, dv = torch.empty_like(s), torch.empty_like(s), torch.empty_like(s)
        with torch.cuda.device(dev):
            _lib.check(lib.mapdn_attention_backward(do.data_ptr(), dl.data_ptr(), s.data_ptr(), k.data_ptr(), v.data_ptr(), B, n, ctx.H,
                                                    ds.data_ptr(), dk.data_ptr(), dv.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        return ds, dk, dv, None


ATTN_MAX_N = 48            # csrc/critic_attn.hip AT_MAX_N (mapdn_attention_max_agents()): one sample's operands and scores must fit a CU's LDS


def attention_ok(sel: torch.Tensor, H: int) -> bool:
    """the attention kernels cover fp32 on the GPU, hidden size 64, 2 <= n <= ATTN_MAX_N agents, 1 / 2 / 4 heads; MAPDN_FUSED_ATTN=0
    switches them off (the batched PyTorch route remains)"""
    return (sel.is_cuda and sel.dtype == torch.float32 and sel.dim() == 3 and sel.shape[-1] == 64 and 2 <= sel.shape[1] <= ATTN_MAX_N
            and H in (1, 2, 4) and sel.shape[0] >= 1 and sel.shape[0] * sel.shape[1] * 64 < 2 ** 31 and os.environ.get("MAPDN_FUSED_ATTN", "1") != "0")


def attention_core(sel: torch.Tensor, key: torch.Tensor, val: torch.Tensor, H: int):
    if attention_ok(sel, H) and key.dtype == torch.float32 and val.dtype == torch.float32:
        return _AttentionCore.apply(sel, key, val, H)
    return attention_core_torch(sel, key, val, H)


class GaussianRNNAgent(nn.Module):
    """fc1 -> LayerNorm -> act -> GRUCell -> (mean, log_std) with log_std squashed by tanh into [LOG_STD_MIN, LOG_STD_MAX]
    (agents/rnn_agent_gaussian.py:6-41).  PyTorch modules (the fused LayerNorm of RNNAgent where it applies): the one-launch policy
    kernels have a single output head and are not extended to two."""

    def __init__(self, input_shape: int, args):
        super().__init__()
        self.hid_size = args.hid_size
        self.fc1 = nn.Linear(input_shape, args.hid_size)
        if args.layernorm:
            self.layernorm = nn.LayerNorm(args.hid_size)
        self.rnn = nn.GRUCell(args.hid_size, args.hid_size)
        self.mean = nn.Linear(args.hid_size, args.action_dim)
        self.log_std = nn.Linear(args.hid_size, args.action_dim)
        self.use_ln = bool(args.layernorm)
        self.act = _activation(args.hid_activation)
        self.lo, self.hi = float(args.LOG_STD_MIN), float(args.LOG_STD_MAX)

    def trunk(self, x: torch.Tensor, hidden: torch.Tensor):
        """x: pre-activation of fc1, [rows, hid]"""
        x = layernorm_act(self.layernorm, self.act, x) if self.use_ln else self.act(x)
        h = gru_cell_tall(self.rnn, x, hidden.reshape(-1, self.hid_size))
        log_std = self.lo + 0.5 * (self.hi - self.lo) * (torch.tanh(tall_linear(self.log_std, h)) + 1)
        return tall_linear(self.mean, h), log_std, h

    def forward(self, inputs, hidden):
        return self.trunk(self.fc1(inputs), hidden)


def _named_sequential(**mods) -> nn.Sequential:
    seq = nn.Sequential()
    for k, m in mods.items():
        if m is not None:
            seq.add_module(k, m)
    return seq


class AttentionCritic(nn.Module):
    """critics/maac_critic.py:8-161 for continuous actions, with the reference's module tree (critic_encoders.{i}.enc_fc1,
    critics.{i}.critic_fc1 / critic_fc2, biases.{i}.bias_fc1 / bias_fc2, state_encoders.{i}.s_enc_fc1, key_extractors.{h},
    selector_extractors.{h}, value_extractors.{h}.0; enc_bn / s_enc_bn under norm_in), so that its state_dict is the reference's.
    forward: [b, n, o], [b, n, a] -> (q - bias [b, n], regulariser [n]).  The per-agent encoders, critics and biases run batched over
    their stacked parameters; the attention over the other agents is attention_core (HIP kernels, or one masked softmax)."""

    def __init__(self, args):
        super().__init__()
        self.hidden_dim, self.attend_heads, self.nagents = args.hid_size, int(args.attend_heads), args.agent_num
        assert self.hidden_dim % self.attend_heads == 0
        sdim, adim, hid = args.obs_size, args.action_dim, args.hid_size
        bn = (lambda k: nn.BatchNorm1d(k, affine=False)) if args.norm_in else (lambda k: None)
        self.norm_in = bool(args.norm_in)
        self.critic_encoders, self.critics, self.biases, self.state_encoders = nn.ModuleList(), nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        for _ in range(self.nagents):
            self.critic_encoders.append(_named_sequential(enc_bn=bn(sdim + adim), enc_fc1=nn.Linear(sdim + adim, hid), enc_nl=nn.LeakyReLU()))
            self.critics.append(_named_sequential(critic_fc1=nn.Linear(2 * hid, hid), critic_nl=nn.LeakyReLU(), critic_fc2=nn.Linear(hid, 1)))
            self.biases.append(_named_sequential(bias_fc1=nn.Linear(hid, hid), bias_nl=nn.LeakyReLU(), bias_fc2=nn.Linear(hid, 1)))
            self.state_encoders.append(_named_sequential(s_enc_bn=bn(sdim), s_enc_fc1=nn.Linear(sdim, hid), s_enc_nl=nn.LeakyReLU()))
        d = hid // self.attend_heads
        self.key_extractors, self.selector_extractors, self.value_extractors = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        for _ in range(self.attend_heads):
            self.key_extractors.append(nn.Linear(hid, d, bias=False))
            self.selector_extractors.append(nn.Linear(hid, d, bias=False))
            self.value_extractors.append(nn.Sequential(nn.Linear(hid, d), nn.LeakyReLU()))

    @staticmethod
    def _per_agent(x: torch.Tensor, layers) -> torch.Tensor:
        """layers[i](x[:, i]) for every agent i as one batched product over the stacked weights: [b, n, in] -> [b, n, out]"""
        w = torch.stack([m.weight for m in layers])                                        # [n, out, in]
        return torch.einsum("bni,noi->bno", x, w) + torch.stack([m.bias for m in layers])

    def forward(self, obs: torch.Tensor, act: torch.Tensor):
        b, n, H = obs.shape[0], self.nagents, self.attend_heads
        sa = torch.cat((obs, act), dim=-1)
        s_in = obs
        if self.norm_in:                                                                    # plain per-agent BatchNorm1d(affine=False) modules
            sa = torch.stack([enc.enc_bn(sa[:, i]) for i, enc in enumerate(self.critic_encoders)], 1)
            s_in = torch.stack([enc.s_enc_bn(obs[:, i]) for i, enc in enumerate(self.state_encoders)], 1)
        sa_enc = F.leaky_relu(self._per_agent(sa, [e.enc_fc1 for e in self.critic_encoders]))          # [b, n, hid]
        s_enc = F.leaky_relu(self._per_agent(s_in, [e.s_enc_fc1 for e in self.state_encoders]))
        # head h's extractor fills columns h d .. (h + 1) d: the H extractors of a kind are one [hid, hid] product
        key = F.linear(sa_enc, torch.cat([m.weight for m in self.key_extractors], 0))
        val = F.leaky_relu(F.linear(sa_enc, torch.cat([m[0].weight for m in self.value_extractors], 0),
                                    torch.cat([m[0].bias for m in self.value_extractors], 0)))
        sel = F.linear(s_enc, torch.cat([m.weight for m in self.selector_extractors], 0))
        other, logit_sq = attention_core(sel, key, val, H)                                  # [b, n, hid], [n, H]
        x = F.leaky_relu(self._per_agent(torch.cat((sa_enc, other), -1), [c.critic_fc1 for c in self.critics]))
        q = self._per_agent(x, [c.critic_fc2 for c in self.critics]).squeeze(-1)            # [b, n]
        y = F.leaky_relu(self._per_agent(s_enc, [c.bias_fc1 for c in self.biases]))
        bias = self._per_agent(y, [c.bias_fc2 for c in self.biases]).squeeze(-1)
        reg = 1e-3 * logit_sq.sum(1) / float(b * (n - 1))                                   # 1e-3 sum over heads of mean(logit^2): maac_critic.py:156-157
        return q - bias, reg


class MAACNet(DDPGNet):
    """`MAAC(Model)` (models/maac.py:10-121): Gaussian recurrent agents, ONE attention critic for all agents, the soft actor-critic loss.
    Target handling, reward BatchNorm, initialisation and the Gaussian branch of select_action are DDPGNet's.  Off-policy: the replay ring
    is kept between update rounds (models/model.py:53-56 clears it for COMA, IAC, IPPO and MAPPO only)."""
    ALGS = ("maac",)

    def __init__(self, args, alg: str = "maac", target_net: Optional["MAACNet"] = None):
        nn.Module.__init__(self)
        if alg not in self.ALGS:
            raise KeyError(alg)
        _maac_args_ok(args)
        self.args, self.alg = args, alg
        self.n_, self.obs_dim, self.act_dim, self.hid_dim = args.agent_num, args.obs_size, args.action_dim, args.hid_size
        self._fused_fits = None
        ids = self.n_ if args.agent_id else 0
        self.batchnorm = nn.BatchNorm1d(self.n_)                   # rewards AND advantages (maac.py:18, 112-113; model.py:317-318)
        self.__dict__["_adv_batchnorm"] = self.batchnorm
        self.value_dicts = nn.ModuleList([AttentionCritic(args)])                                          # maac.py:40-41
        self.policy_dicts = nn.ModuleList([GaussianRNNAgent(self.obs_dim + ids, args) for _ in range(1 if args.shared_params else self.n_)])
        self.apply(self._init_weights)
        if target_net is not None:
            self.target_net = target_net
            self.reload_params_to_target()

    def policy(self, obs: torch.Tensor, last_hid: torch.Tensor, means_grad_only: bool = False):
        """models/model.py:101-139 with gaussian_policy: obs [b, n, o], last_hid [b, n, h] -> means, log_stds [b, n, a], hiddens [b, n, h]"""
        b, n, o = obs.shape[0], self.n_, self.obs_dim
        if self.args.shared_params:
            ag = self.policy_dicts[0]
            w = ag.fc1.weight
            if _tall_ok(obs, b * n, w):
                x = _TallLinear.apply(obs.reshape(b * n, o), w[:, :o], ag.fc1.bias).view(b, n, -1)
            else:
                x = F.linear(obs, w[:, :o], ag.fc1.bias)
            if self.args.agent_id:
                x = x + w[:, o:].t().unsqueeze(0)                        # one-hot id i selects column o + i
            m, ls, h = ag.trunk(x.reshape(b * n, -1), last_hid)
            return m.view(b, n, -1), ls.view(b, n, -1), h.view(b, n, -1)
        ms, lss, hs = [], [], []
        for i, ag in enumerate(self.policy_dicts):
            w = ag.fc1.weight
            x = F.linear(obs[:, i], w[:, :o], ag.fc1.bias)
            if self.args.agent_id:
                x = x + w[:, o + i]
            m, ls, h = ag.trunk(x, last_hid[:, i])
            ms.append(m); lss.append(ls); hs.append(h)
        return torch.stack(ms, 1), torch.stack(lss, 1), torch.stack(hs, 1)

    def value(self, obs: torch.Tensor, act: torch.Tensor, own_action_only: bool = False) -> torch.Tensor:
        """maac.py:47-66: [b + 1, n] — rows 0 .. b - 1 the values, row b the per-agent attention regulariser"""
        q, reg = self.value_dicts[0](obs, act)
        return torch.cat((q, reg.unsqueeze(0)), 0)

    def get_actions(self, state, status, exploration, actions_avail, target=False, last_hid=None, means_grad_only=False, clip=False, noise=None):
        """maac.py:68-92: DDPGNet.get_actions with the log-probability masked and summed over the action dimension: [b, n]"""
        actions, restore, log_prob, out, hid = super().get_actions(state, status, exploration, actions_avail, target, last_hid, means_grad_only, clip, noise)
        if log_prob is not None:
            log_prob = ((1.0 - (actions_avail == 0).to(log_prob.dtype)) * log_prob).sum(dim=-1)
        return actions, restore, log_prob, out, hid

    def get_loss(self, batch: Batch, want=("policy", "value")):
        """maac.py:94-121.  Two draws per call, in the reference's order: the actions at `state` from the behaviour policy, then the next
        actions at `next_state` from the target policy; batch["noise"] / batch["next_noise"] [bs, n, 1] replace them.  A loss not in
        `want` is None; of its forward passes only those are kept that change state the reference's call changes (the draws, and the
        running statistics of `batchnorm` / the norm_in BatchNorms, which see every value() call while training)."""
        n, a = self.n_, self.args
        state, actions, next_state = batch["state"], batch["action"], batch["next_state"]
        avail, last_hid, hid = batch["action_avail"], batch["last_hid"], batch["hid"]
        bs = state.shape[0]
        rewards = self.normalise_reward(batch["reward"].float())
        done = batch["done"].float().view(-1, 1)
        valid = batch.get("valid")
        wmean = (lambda t: t.mean()) if valid is None else \
            (lambda t: (t * valid.float().view(-1, 1)).sum() / (valid.float().sum().clamp(min=1.0) * t.shape[1]))
        want_p, want_v = "policy" in want, "value" in want
        stats = self.training and (a.norm_in or a.normalize_advantages)      # value() calls that move running statistics cannot be skipped
        _, actions_pol, log_prob, action_out, _ = self.get_actions(state, "train", True, avail, False, last_hid, noise=batch.get("noise"))
        if want_v or (stats and a.norm_in):
            with torch.no_grad():
                _, next_actions, _, _, _ = self.get_actions(next_state, "train", True, avail, True, hid, noise=batch.get("next_noise"))
        elif batch.get("next_noise") is None:
            torch.randn_like(actions_pol)                                    # the call's second draw, so that the generator goes the reference's way
        policy_loss = value_loss = None
        values_pol = None
        if want_p or stats:
            with torch.set_grad_enabled(want_p and torch.is_grad_enabled()):
                values_pol = self.value(state, actions_pol)[:bs]             # (every agent's action carries gradient: maac.py:99 detaches nothing)
        if want_v or want_p:
            with torch.set_grad_enabled(want_v and torch.is_grad_enabled()):
                compose = self.value(state, actions.detach())
            values, attn_reg = compose[:bs], compose[bs]
        if want_v or (stats and a.norm_in):
            with torch.no_grad():
                net = self.target_net if a.target else self
                next_values = net.value(next_state, next_actions)[:bs].view(-1, n)
        if values_pol is not None:
            advantages = values_pol
            if a.normalize_advantages:
                advantages = self._adv_batchnorm.to(advantages.device)(advantages)
        if want_p:
            if a.soft:
                pl = log_prob / a.reward_scale - advantages
            else:
                pl = -advantages.detach() * log_prob
            policy_loss = wmean(pl + attn_reg)                               # the regulariser goes to the POLICY loss only (maac.py:118)
        if want_v:
            returns = rewards + a.gamma * (1 - done) * next_values - a.soft * log_prob / a.reward_scale       # log_prob NOT detached (maac.py:109)
            value_loss = wmean((returns - values).pow(2))
        return policy_loss, value_loss, (action_out if want_p else None)


# ---- SQDDPG (models/sqddpg.py) -------------------------------------------------------------------------------------------------------
def sample_coalition_positions(rows: int, n: int, device, generator=None) -> torch.Tensor:
    """sqddpg.py:38-40: ONE th.multinomial of shape [rows, n] on float64 uniform weights, without replacement -> pos [rows, n] int64,
    pos[r, i] = the position of agent i in row r's random order"""
    w = torch.full((rows, n), 1.0 / n, dtype=torch.float64, device=device)
    return torch.multinomial(w, n, replacement=False, generator=generator)


def shapley_first_layer(base: torch.Tensor, id_cols: Optional[torch.Tensor], act_cols: torch.Tensor, act: torch.Tensor, pos: torch.Tensor,
                        who: Optional[int] = None) -> torch.Tensor:
    """The first layer of the coalition critic's rows (sqddpg.py:65-93) in factored form.  base [b, h] = W_obs obs_all + b1, id_cols [n, h]
    or None, act_cols [n, h] (W_act transposed: row p is the column of action SLOT p), act [b, n], pos [b, S, n] integer.  With
    gc = argsort(pos) the agent at each position, slot p holds the action of agent gc[p]; row (b, s, i) keeps the slots up to its own
    position pos_i and zeroes the rest:
        x[b, s, i] = base[b] + id_cols[i] + P[b, s, pos_i],   P[b, s, p] = sum_{q <= p} act[b, gc[q]] act_cols[q]   (one cumsum + one gather)
    Only the own slot carries a gradient back to the action (sqddpg.py:77): P is built from the detached actions and a zero-valued
    (act_i - act_i.detach()) act_cols[pos_i] restores that path.  who: agent i's rows only ([b, S, h]; id_cols is then that agent's [h])."""
    b, S, n = pos.shape
    h = base.shape[-1]
    pos = pos.long()
    gc = pos.argsort(dim=-1)
    a_slot = act.detach().unsqueeze(1).expand(b, S, n).gather(2, gc)                  # [b, S, n]: the action in slot p
    P = (a_slot.unsqueeze(-1) * act_cols).cumsum(dim=2)                               # [b, S, n, h]
    if who is None:
        x = P.gather(2, pos.unsqueeze(-1).expand(b, S, n, h)) + base.view(b, 1, 1, h)
        if id_cols is not None:
            x = x + id_cols
        if act.requires_grad:
            x = x + (act - act.detach()).view(b, 1, n, 1) * act_cols[pos]
        return x
    pw = pos[:, :, who]
    x = P.gather(2, pw.view(b, S, 1, 1).expand(b, S, 1, h)).squeeze(2) + base.view(b, 1, h)
    if id_cols is not None:
        x = x + id_cols
    if act.requires_grad:
        x = x + (act[:, who] - act[:, who].detach()).view(b, 1, 1) * act_cols[pw]
    return x


class _ShapleyCritic(torch.autograd.Function):
    """v[b, s, i] of the coalition critic behind its first layer as HIP launches (libmapdn_hip.so: mapdn_critic_shapley_*, csrc/critic_shap.hip):
    the rows x[b, s, i] = base[b] + id_cols[i] + P[b, s, pos_i] are formed in the kernel from the prefix sum over positions, so that neither
    the reference's [b S n, (o + 1) n + n] input nor a [b S n, 64] activation exists.  The backward recomputes the forward; when only the
    action needs a gradient (the policy update) it returns d act alone and skips every parameter partial."""
    launches = 0

    @staticmethod
    def forward(ctx, act, base, id_cols, act_cols, pos32, ln_w, ln_b, eps, w2, b2, w3, b3):
        from . import _lib
        lib = _lib.load()
        b, S, n = pos32.shape
        ops = tuple(t.detach().contiguous() for t in (base, id_cols, act_cols, act.reshape(b, n)))
        prm = tuple(t.detach().contiguous() for t in (ln_w, ln_b, w2, b2, w3.reshape(64), b3.reshape(1)))
        v = torch.empty(b, S, n, dtype=torch.float32, device=base.device)
        with torch.cuda.device(base.device):
            _lib.check(lib.mapdn_critic_shapley_forward(ops[0].data_ptr(), ops[1].data_ptr(), ops[2].data_ptr(), ops[3].data_ptr(), pos32.data_ptr(),
                                                        b, S, n, prm[0].data_ptr(), prm[1].data_ptr(), float(eps), prm[2].data_ptr(), prm[3].data_ptr(),
                                                        prm[4].data_ptr(), prm[5].data_ptr(), v.data_ptr(), None,
                                                        torch.cuda.current_stream(base.device).cuda_stream))
        _ShapleyCritic.launches += 1
        ctx.save_for_backward(pos32, *ops, *prm)
        ctx.eps, ctx.act_shape = float(eps), act.shape
        return v

    @staticmethod
    def backward(ctx, dv):
        from . import _lib
        lib = _lib.load()
        pos32, base, idc, actc, act, g, be, w2, b2, w3, b3 = ctx.saved_tensors
        b, S, n = pos32.shape
        need, dev = ctx.needs_input_grad, base.device
        param_grads = any(need[i] for i in (1, 2, 3, 5, 6, 8, 9, 10, 11))
        dv2 = dv.reshape(b, S, n).contiguous()
        dact = torch.empty(b, n, dtype=torch.float32, device=dev) if need[0] else None
        dbase = grads = scratch = None
        with torch.cuda.device(dev):
            if param_grads:
                dbase = torch.empty_like(base)
                grads = torch.empty(4416 + 2 * n * 64, dtype=torch.float32, device=dev)
                scratch = torch.empty(max(1, lib.mapdn_critic_shapley_scratch_floats(b, S, n)), dtype=torch.float32, device=dev)
            ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
            _lib.check(lib.mapdn_critic_shapley_backward(dv2.data_ptr(), base.data_ptr(), idc.data_ptr(), actc.data_ptr(), act.data_ptr(), pos32.data_ptr(),
                                                         b, S, n, g.data_ptr(), be.data_ptr(), ctx.eps, w2.data_ptr(), b2.data_ptr(), w3.data_ptr(),
                                                         b3.data_ptr(), ptr(dbase), ptr(grads), ptr(scratch), ptr(dact), int(param_grads),
                                                         torch.cuda.current_stream(dev).cuda_stream))
        da = dact.view(ctx.act_shape) if dact is not None else None
        if not param_grads:
            return (da,) + (None,) * 11
        return (da, dbase, grads[4416:4416 + n * 64].view(n, 64), grads[4416 + n * 64:].view(n, 64), None, grads[4096:4160], grads[4160:4224], None,
                grads[:4096].view(64, 64), grads[4224:4288], grads[4288:4352].view(1, 64), grads[4352:4353])


_SHAP_MAX_N = None


def shapley_max_agents() -> int:
    """the largest n the coalition kernels admit (their per-wavefront LDS holds one group's prefix and two [n][64] accumulators)"""
    global _SHAP_MAX_N
    if _SHAP_MAX_N is None:
        import ctypes
        from . import _lib
        m = ctypes.c_int32(0)
        _lib.load().mapdn_critic_shapley_geometry(1, 1, 1, 0, 1, None, None, None, None, ctypes.byref(m))
        _SHAP_MAX_N = int(m.value)
    return _SHAP_MAX_N


def shapley_ok(cr: "MLPCritic", base: torch.Tensor, n: int, S: int) -> bool:
    """the coalition kernels cover the reference's default critic (LayerNorm, ReLU, hidden size 64, one output) in fp32 on the GPU for
    n <= shapley_max_agents() and fewer than 2^31 rows; MAPDN_FUSED_SHAP=0 switches them off (the factored PyTorch form remains)"""
    return (base.is_cuda and base.dtype == torch.float32 and base.dim() == 2 and base.shape[-1] == 64 and cr.use_ln and cr.act is F.relu
            and cr.layernorm.elementwise_affine and cr.layernorm.bias is not None and cr.fc2.in_features == 64 and cr.fc2.out_features == 64
            and cr.fc2.bias is not None and cr.fc3.out_features == 1 and cr.fc3.bias is not None and cr.fc2.weight.dtype == torch.float32
            and os.environ.get("MAPDN_FUSED_SHAP", "1") != "0" and base.shape[0] >= 1 and base.shape[0] * S * n < 2 ** 31 - 1
            and n <= shapley_max_agents())


class SQDDPGNet(DDPGNet):
    """`SQDDPG(Model)` (models/sqddpg.py:10-160): the deterministic recurrent agents, target handling and reward BatchNorm are DDPGNet's; the
    critic is valued on sampled coalitions — per sample `sample_size` random orders of the agents, per order and agent one row that
    sees the actions of the agents before it and its own — and the mean over the orders is the agent's approximate Shapley value.
    Off-policy: the replay ring is kept between update rounds."""
    ALGS = ("sqddpg",)

    def __init__(self, args, alg: str = "sqddpg", target_net: Optional["SQDDPGNet"] = None):
        nn.Module.__init__(self)
        if alg not in self.ALGS:
            raise KeyError(alg)
        _sqddpg_args_ok(args)
        self.args, self.alg = args, alg
        self.n_, self.obs_dim, self.act_dim, self.hid_dim = args.agent_num, args.obs_size, args.action_dim, args.hid_size
        self.sample_size = int(args.sample_size)
        self._fused_fits = None
        n, o, a = self.n_, self.obs_dim, self.act_dim
        ids = n if args.agent_id else 0
        self.batchnorm = nn.BatchNorm1d(n)                         # rewards (model.py:317-318) AND advantages (sqddpg.py:19, 155-156)
        self.__dict__["_adv_batchnorm"] = self.batchnorm
        copies = 1 if args.shared_params else n
        self.value_dicts = nn.ModuleList([MLPCritic((o + a) * n + ids, 1, args) for _ in range(copies)])       # sqddpg.py:22-31: ids AFTER the actions
        self.policy_dicts = nn.ModuleList([RNNAgent(o + ids, args) for _ in range(copies)])
        self.apply(self._init_weights)
        if target_net is not None:
            self.target_net = target_net
            self.reload_params_to_target()

    def sample_coalitions(self, batch_size: int, device) -> torch.Tensor:
        """pos [b, S, n] int64 from one multinomial draw of shape [b S, n] (sqddpg.py:37-40)"""
        return sample_coalition_positions(batch_size * self.sample_size, self.n_, device).view(batch_size, self.sample_size, self.n_)

    def marginal_contribution(self, obs: torch.Tensor, act: torch.Tensor, pos: Optional[torch.Tensor] = None,
                              own_action_only: bool = False) -> torch.Tensor:
        """sqddpg.py:65-106: obs [b, n, o], act [b, n, 1] -> [b, S, n, 1]; pos [b, S, n] replaces the draw.  Routes: (a) the coalition
        kernels where shapley_ok; (b) the factored PyTorch form (shapley_first_layer: cumsum + gather), also the CPU path; (c) without
        shared parameters the same factored form per agent critic.  own_action_only: the caller differentiates with respect to `act`
        alone (the policy loss): the first layer's operands enter detached, and route (a) then skips every parameter gradient."""
        b, n, o = obs.shape[0], self.n_, self.obs_dim
        if pos is None:
            pos = self.sample_coalitions(b, obs.device)
        S = pos.shape[1]
        ids = n if self.args.agent_id else 0
        obs_all, act2 = obs.reshape(b, n * o), act.reshape(b, n)
        if self.args.shared_params:
            cr = self.value_dicts[0]
            w, b1 = (cr.fc1.weight.detach(), cr.fc1.bias.detach()) if own_action_only else (cr.fc1.weight, cr.fc1.bias)
            base = tall_linear_w(obs_all, w[:, :n * o], b1)
            act_cols = w[:, n * o:n * o + n].t()
            id_cols = w[:, n * o + n:].t() if ids else None
            if ids and shapley_ok(cr, base, n, S):
                ln = cr.layernorm
                prm = (ln.weight, ln.bias, ln.eps, cr.fc2.weight, cr.fc2.bias, cr.fc3.weight, cr.fc3.bias)
                if own_action_only:
                    prm = tuple(t.detach() if torch.is_tensor(t) else t for t in prm)
                v = _ShapleyCritic.apply(act2, base, id_cols, act_cols, pos.to(torch.int32).contiguous(), *prm)
                return v.view(b, S, n, 1)
            x = shapley_first_layer(base, id_cols, act_cols, act2, pos)
            v, _ = cr.trunk(x.reshape(b * S * n, -1))
            return v.view(b, S, n, 1)
        vs = []
        for i, cr in enumerate(self.value_dicts):
            w, b1 = (cr.fc1.weight.detach(), cr.fc1.bias.detach()) if own_action_only else (cr.fc1.weight, cr.fc1.bias)
            base = F.linear(obs_all, w[:, :n * o], b1)
            x = shapley_first_layer(base, w[:, n * o + n + i] if ids else None, w[:, n * o:n * o + n].t(), act2, pos, who=i)
            vs.append(cr.trunk(x.reshape(b * S, -1))[0].view(b, S, 1))
        return torch.stack(vs, 2)

    def value(self, obs: torch.Tensor, act: torch.Tensor, own_action_only: bool = False) -> torch.Tensor:
        """sqddpg.py:108-109: the marginal contributions of a fresh draw, [b, S, n, 1]"""
        return self.marginal_contribution(obs, act)

    def get_loss(self, batch: Batch, want=("policy", "value")):
        """sqddpg.py:133-160.  Three coalition draws per call, in the reference's order: for the policy actions at `state`, for the replay
        actions at `state`, for the next actions at `next_state` (on the target net).  batch["coalitions"] (three pos [bs, S, n]) replaces
        them.  A loss not in `want` is None and its forward passes are skipped, but its draw is still made, so that the generator goes the
        reference's way (and `batchnorm`, under normalize_advantages, still sees the advantages while training).  The rewards pass
        `batchnorm` under reward_normalisation as for every algorithm (model.py:317-318); sqddpg.py adds nothing of its own."""
        n, a = self.n_, self.args
        state, actions, next_state = batch["state"], batch["action"], batch["next_state"]
        avail, last_hid, hid = batch["action_avail"], batch["last_hid"], batch["hid"]
        bs = state.shape[0]
        rewards = self.normalise_reward(batch["reward"].float())
        done = batch["done"].float().view(-1, 1)
        valid = batch.get("valid")
        wmean = (lambda t: t.mean()) if valid is None else \
            (lambda t: (t * valid.float().view(-1, 1)).sum() / (valid.float().sum().clamp(min=1.0) * t.shape[1]))
        want_p, want_v = "policy" in want, "value" in want
        given = batch.get("coalitions")
        draw = (lambda k: given[k].view(bs, -1, n)) if given is not None else (lambda k: self.sample_coalitions(bs, state.device))
        stats = self.training and a.normalize_advantages             # `batchnorm` sees the advantages in every call of the reference
        policy_loss = value_loss = action_out = None
        pos_pol = draw(0)
        if want_p or stats:
            with torch.set_grad_enabled(want_p and torch.is_grad_enabled()):
                _, actions_pol, _, action_out, _ = self.get_actions(state, "train", False, avail, False, last_hid, means_grad_only=True)
                advantages = self.marginal_contribution(state, actions_pol, pos_pol, own_action_only=True).mean(dim=1).view(-1, n)
                if a.normalize_advantages:
                    advantages = self._adv_batchnorm.to(advantages.device)(advantages)
            if want_p:
                policy_loss = wmean(-advantages)
        pos_val, pos_next = draw(1), draw(2)
        if want_v:
            with torch.no_grad():
                _, next_actions, _, _, _ = self.get_actions(next_state, "train", False, avail, not a.double_q, hid, means_grad_only=True)
                net = self.target_net if a.target else self
                next_sum = net.marginal_contribution(next_state, next_actions, pos_next).mean(dim=1).view(-1, n).sum(dim=-1, keepdim=True)
                returns = rewards + a.gamma * (1 - done) * next_sum.expand(bs, n)
            value_sum = self.marginal_contribution(state, actions.detach(), pos_val).mean(dim=1).view(-1, n).sum(dim=-1, keepdim=True)
            value_loss = wmean((returns - value_sum.expand(bs, n)).pow(2))
        return policy_loss, value_loss, (action_out if want_p else None)


# ---- MAPPO / IPPO (models/mappo.py, models/ippo.py, learning_algorithms/ppo.py) ---------------------------------------------------------
_LOG_SQRT_2PI = math.log(math.sqrt(2 * math.pi))
PPO_MAX_ELEMS = 1 << 40                    # csrc/capi.hip ppo_shape_ok: rows * n at most


def ppo_fused_ok(*tensors) -> bool:
    """the PPO kernels (csrc/ppo.hip: the strided GAE, the two clipped losses) cover fp32 tensors on the GPU with at most 2^40 elements;
    MAPDN_FUSED_PPO=0 switches them off (the vectorised PyTorch forms below remain, which are also the CPU route).  tensors: every tensor
    the launch would read (None for an optional one that is absent); the first is a per-agent [rows, n] one."""
    return (os.environ.get("MAPDN_FUSED_PPO", "1") != "0" and all(t is None or (t.is_cuda and t.dtype == torch.float32) for t in tensors)
            and tensors[0].dim() == 2 and 1 <= tensors[0].numel() <= PPO_MAX_ELEMS)


def ppo_gae_torch(reward, value, next_value, done, last_step, stride: int, gamma: float, lambda_: float) -> torch.Tensor:
    """ppo.py:46-54 over chains of `stride`: row i's successor is row i + stride.  reward / value / next_value [rows, n], done / last_step
    [rows] -> advantages [rows, n].  A loop over the ceil(rows / stride) chain STEPS on [stride, n] slices (newest first), never over
    rows; stride 1 is the reference's loop, operation for operation."""
    rows = reward.shape[0]
    S = int(stride)
    mask = torch.where(last_step != 0, 1.0 - done, torch.ones_like(done)).unsqueeze(-1)          # ppo.py:48-51
    delta = reward + gamma * next_value * mask - value                                            # ppo.py:52
    adv = torch.empty_like(delta)
    last = torch.zeros_like(delta[:min(S, rows)])
    for t in reversed(range(-(-rows // S))):
        lo, hi = t * S, min((t + 1) * S, rows)
        new = delta[lo:hi] + gamma * lambda_ * last[:hi - lo] * mask[lo:hi]                       # ppo.py:53
        adv[lo:hi] = new
        last = new if hi - lo == last.shape[0] else torch.cat((new, last[hi - lo:]))             # (the ragged end: the other chains start one step later)
    return adv


def ppo_gae(reward, value, next_value, done, last_step, stride: int, gamma: float, lambda_: float) -> torch.Tensor:
    """the advantages of ppo_gae_torch, without autograd: ONE launch (mapdn_ppo_gae) where ppo_fused_ok, the chain-step loop otherwise"""
    if stride < 1:
        raise ValueError(f"GAE chain stride {stride} must be at least 1")
    r, v, nv, d, ls = (t.detach() for t in (reward, value, next_value, done, last_step))
    if not ppo_fused_ok(r, v, nv, d, ls):
        with torch.no_grad():
            return ppo_gae_torch(r, v, nv, d, ls, stride, gamma, lambda_)
    from . import _lib
    r, v, nv, d, ls = (t.contiguous() for t in (r, v, nv, d, ls))
    rows, n = r.shape
    adv = torch.empty_like(r)
    with torch.cuda.device(r.device):
        _lib.check(_lib.load().mapdn_ppo_gae(r.data_ptr(), v.data_ptr(), nv.data_ptr(), d.data_ptr(), ls.data_ptr(), adv.data_ptr(), rows, n, int(stride),
                                             float(gamma), float(lambda_), torch.cuda.current_stream(r.device).cuda_stream))
    ppo_gae.launches += 1
    return adv


ppo_gae.launches = 0            # how often the kernel was reached (tests count the routes)


def _ppo_weights(valid: Optional[torch.Tensor], like: torch.Tensor):
    """(valid as f32 [rows] or None, scale [1] = 1 / (the divisor of DDPGNet.get_loss's wmean)) for a per-agent tensor [rows, n]"""
    rows, n = like.shape
    if valid is None:
        return None, like.new_full((1,), 1.0 / (rows * n))
    vf = valid.float().view(-1).contiguous()
    return vf, (1.0 / (vf.sum().clamp(min=1.0) * n)).reshape(1)


class _PPOPolicyLoss(torch.autograd.Function):
    """-wmean(min(rho A, clamp(rho, 1 -/+ eps) A)) of ppo.py:39, 62-64 and its gradient with respect to the policy means as ONE entry
    call (mapdn_ppo_policy_loss: the streaming launch + the fixed-order pass over its per-workgroup partial sums).  backward scales the
    stored gradient by the incoming one (1 for `loss.backward()`).  The log-std of the non-Gaussian agent is a constant: no gradient."""
    launches = 0

    @staticmethod
    def forward(ctx, means, actions, log_stds, avail, old_log_prob, adv, valid, scale, eps_clip):
        from . import _lib
        lib = _lib.load()
        rows, n = adv.shape
        mu, ac, ls, ol, ad = (t.detach().reshape(rows, n).contiguous() for t in (means, actions, log_stds, old_log_prob, adv))
        av = avail.detach().reshape(rows, n).contiguous() if avail is not None else None
        dev = mu.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dmean = torch.empty_like(mu)
        with torch.cuda.device(dev):
            partial = torch.empty(lib.mapdn_ppo_loss_blocks(rows * n), dtype=torch.float32, device=dev)
            _lib.check(lib.mapdn_ppo_policy_loss(ac.data_ptr(), mu.data_ptr(), ls.data_ptr(), av.data_ptr() if av is not None else None, ol.data_ptr(),
                                                 ad.data_ptr(), valid.data_ptr() if valid is not None else None, scale.data_ptr(), float(eps_clip),
                                                 loss.data_ptr(), dmean.data_ptr(), partial.data_ptr(), rows, n, torch.cuda.current_stream(dev).cuda_stream))
        _PPOPolicyLoss.launches += 1
        ctx.save_for_backward(dmean)
        ctx.shape = means.shape
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g):
        (dmean,) = ctx.saved_tensors
        return ((dmean * g).view(ctx.shape),) + (None,) * 8


class _PPOValueLoss(torch.autograd.Function):
    """coef wmean(max((V - R)^2, (V_clip - R)^2)) of ppo.py:56, 67-70 and its gradient with respect to V as ONE entry call
    (mapdn_ppo_value_loss), R = r + gamma (1 - done) V(next) formed inside; backward scales the stored gradient by the incoming one"""
    launches = 0

    @staticmethod
    def forward(ctx, values, old_values, reward, next_values, done, valid, scale, gamma, eps_clip, coef):
        from . import _lib
        lib = _lib.load()
        rows, n = old_values.shape
        v, vo, r, vn = (t.detach().reshape(rows, n).contiguous() for t in (values, old_values, reward, next_values))
        d = done.detach().reshape(rows).contiguous()
        dev = v.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dv = torch.empty_like(v)
        with torch.cuda.device(dev):
            partial = torch.empty(lib.mapdn_ppo_loss_blocks(rows * n), dtype=torch.float32, device=dev)
            _lib.check(lib.mapdn_ppo_value_loss(v.data_ptr(), vo.data_ptr(), r.data_ptr(), vn.data_ptr(), d.data_ptr(),
                                                valid.data_ptr() if valid is not None else None, scale.data_ptr(), float(gamma), float(eps_clip),
                                                float(coef), loss.data_ptr(), dv.data_ptr(), partial.data_ptr(), rows, n,
                                                torch.cuda.current_stream(dev).cuda_stream))
        _PPOValueLoss.launches += 1
        ctx.save_for_backward(dv)
        ctx.shape = values.shape
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g):
        (dv,) = ctx.saved_tensors
        return ((dv * g).view(ctx.shape),) + (None,) * 9


def _wmean(valid):
    return (lambda t: t.mean()) if valid is None else \
        (lambda t: (t * valid.float().view(-1, 1)).sum() / (valid.float().sum().clamp(min=1.0) * t.shape[1]))


def ppo_policy_loss_torch(means, actions, log_stds, avail, old_log_prob, adv, valid, eps_clip: float) -> torch.Tensor:
    """ppo.py:30-33, 39, 62-64 as written (Normal(means, stds).log_prob of utilities/util.py:44-46 spelled out); [bs, n, 1] tensors, adv
    [bs, n]; the means of the loss weighted by `valid` as in DDPGNet.get_loss"""
    std = log_stds.exp()
    log_prob = -((actions - means) ** 2) / (2 * std ** 2) - std.log() - _LOG_SQRT_2PI
    mask = 1.0 if avail is None else 1.0 - (avail == 0).to(log_prob.dtype)
    log_prob, old = (mask * log_prob).sum(dim=-1), (mask * old_log_prob).sum(dim=-1)
    ratios = torch.exp(log_prob - old.detach())
    adv = adv.detach()
    return -_wmean(valid)(torch.min(ratios * adv, torch.clamp(ratios, 1 - eps_clip, 1 + eps_clip) * adv))


def ppo_value_loss_torch(values, old_values, reward, next_values, done, valid, gamma: float, eps_clip: float, coef: float) -> torch.Tensor:
    """ppo.py:56, 67-70 as written; [bs, n] tensors, done [bs]"""
    returns = reward + gamma * (1 - done.view(-1, 1)) * next_values.detach()
    clipped = old_values + torch.clamp(values - old_values, -eps_clip, eps_clip)
    return coef * _wmean(valid)(torch.max((values - returns).pow(2), (clipped - returns).pow(2)))


def ppo_policy_loss(means, actions, log_stds, avail, old_log_prob, adv, valid, eps_clip: float) -> torch.Tensor:
    if not (ppo_fused_ok(adv, means, actions, log_stds, avail, old_log_prob) and means.shape[-1] == 1 and not log_stds.requires_grad):
        return ppo_policy_loss_torch(means, actions, log_stds, avail, old_log_prob, adv, valid, eps_clip)
    vf, scale = _ppo_weights(valid, adv)
    return _PPOPolicyLoss.apply(means, actions, log_stds, avail, old_log_prob, adv, vf, scale, eps_clip)


def ppo_value_loss(values, old_values, reward, next_values, done, valid, gamma: float, eps_clip: float, coef: float) -> torch.Tensor:
    if not ppo_fused_ok(old_values, values, reward, next_values, done):
        return ppo_value_loss_torch(values, old_values, reward, next_values, done, valid, gamma, eps_clip, coef)
    vf, scale = _ppo_weights(valid, old_values)
    return _PPOValueLoss.apply(values, old_values, reward, next_values, done, vf, scale, gamma, eps_clip, coef)


class PPONet(DDPGNet):
    """`MAPPO(Model)` (models/mappo.py:11) and `IPPO(Model)` (models/ippo.py:10) with the loss of `PPO` (learning_algorithms/ppo.py): the
    deterministic recurrent agents (their fixed std makes them a Gaussian policy for the ratio), target handling and reward BatchNorm
    are DDPGNet's; the critic is a state value V(s) — MAPPO's on [all obs | id], IPPO's on [own obs | id].  On-policy: PGTrainer empties
    the replay ring after every update round (models/model.py:53-56), stores log_prob / value / next_value with every transition, and
    sets `gae_stride` to its env count.

    Two quirks of the reference are kept.  (1) The GAE mask (ppo.py:48-51) is 1 - done on a last_step row and 1 on every other row, so
    a timeout (last_step without done) does not cut the chain, nor does a done without last_step.  (2) Model.unpack_data
    (models/model.py:309) fills old_log_prob_a from batch.action, so the reference's ratio is exp(log_prob_new - action):
    args.ppo_old_log_prob="reference" (the default; not a reference key) does the same, "stored" takes the log-probability recorded at
    rollout time (batch["log_prob"]).  The target net is built, updated and saved, and never read by the loss (ppo.py:16).

    Chain stride.  get_loss(batch, want, stride) treats row i + stride as row i's successor (default: the attribute `gae_stride`, 1
    unless the trainer set it; 1 is the reference's row-by-row walk, literally).  The replay ring holds rows in (step, env) order and
    every insertion adds one row per env, so with stride = the env count each residue class of a sampled window is one env's time
    series wherever the window starts.  A window shorter than the stride gives chains of one row (advantage = delta): on-policy
    training wants batch_size to be a multiple of the env count."""
    ALGS = ("mappo", "ippo")

    def __init__(self, args, alg: str = "mappo", target_net: Optional["PPONet"] = None):
        nn.Module.__init__(self)
        if alg not in self.ALGS:
            raise KeyError(alg)
        _ppo_args_ok(args)
        self.args, self.alg = args, alg
        self.n_, self.obs_dim, self.act_dim, self.hid_dim = args.agent_num, args.obs_size, args.action_dim, args.hid_size
        self._fused_fits = None
        n, o = self.n_, self.obs_dim
        ids = n if args.agent_id else 0
        self.batchnorm = nn.BatchNorm1d(n)                         # rewards only (model.py:317-318)
        # advantages: PPO.batchnorm (ppo.py:11, 58-59) lives on a plain object — not part of the state_dict, never switched to eval
        self.__dict__["_adv_batchnorm"] = nn.BatchNorm1d(n)
        self.__dict__["gae_stride"] = 1
        copies = 1 if args.shared_params else n
        critic_in = (n * o if alg == "mappo" else o) + ids         # mappo.py:21-26, ippo.py:20-25: a V(s), no action columns
        self.value_dicts = nn.ModuleList([MLPCritic(critic_in, 1, args) for _ in range(copies)])
        self.policy_dicts = nn.ModuleList([RNNAgent(o + ids, args) for _ in range(copies)])
        self.apply(self._init_weights)
        if target_net is not None:
            self.target_net = target_net
            self.reload_params_to_target()

    def value(self, obs: torch.Tensor, act: Optional[torch.Tensor] = None, own_action_only: bool = False) -> torch.Tensor:
        """obs [b, n, o] -> V [b, n, 1]; `act` is ignored (mappo.py:36-65, ippo.py:35-59).  MAPPO's [b, n, n o] input is never built: the
        first layer is W_obs·obs_all + b1 once per sample plus the agent's id column, and with the default critic on the GPU everything
        behind it is the one-launch head on rows formed as base[b] + per_n[i]."""
        b, n, o = obs.shape[0], self.n_, self.obs_dim
        ids = n if self.args.agent_id else 0
        if self.alg == "ippo":
            if self.args.shared_params:
                cr = self.value_dicts[0]
                w = cr.fc1.weight
                x = tall_linear_w(obs.reshape(b * n, o), w[:, :o], cr.fc1.bias)
                if ids:
                    x = (x.view(b, n, -1) + w[:, o:].t().unsqueeze(0)).reshape(b * n, -1)
                return cr.trunk(x)[0].view(b, n, 1)
            return torch.stack([cr.trunk(F.linear(obs[:, i], cr.fc1.weight[:, :o], cr.fc1.bias) + (cr.fc1.weight[:, o + i] if ids else 0.0))[0]
                                for i, cr in enumerate(self.value_dicts)], 1)
        obs_all = obs.reshape(b, n * o)
        if self.args.shared_params:
            cr = self.value_dicts[0]
            w = cr.fc1.weight
            base = tall_linear_w(obs_all, w[:, :n * o], cr.fc1.bias)                         # [b, h]: once per sample
            if ids:
                per_n = w[:, n * o:].t()                                                    # [n, h]: the id columns
                if critic_head_ok(cr, base, b * n, n):
                    return critic_head(cr, base, per_n).view(b, n, 1)
                x = base.unsqueeze(1) + per_n.unsqueeze(0)
            else:
                x = base.unsqueeze(1).expand(b, n, -1)
            return cr.trunk(x.reshape(b * n, -1))[0].view(b, n, 1)
        return torch.stack([cr.trunk(F.linear(obs_all, cr.fc1.weight[:, :n * o], cr.fc1.bias) + (cr.fc1.weight[:, n * o + i] if ids else 0.0))[0]
                            for i, cr in enumerate(self.value_dicts)], 1)

    @torch.no_grad()
    def advantages(self, batch: Batch, rewards: torch.Tensor, stride: Optional[int] = None) -> torch.Tensor:
        """GAE on the STORED value / next_value (ppo.py:46-54) over chains of `stride`, through PPO.batchnorm with normalize_advantages
        (ppo.py:58-59; the union of the ranks' batches under data-parallel training): [bs, n], no gradient"""
        n, a = self.n_, self.args
        S = int(self.__dict__.get("gae_stride", 1) if stride is None else stride)
        adv = ppo_gae(rewards, batch["value"].float().view(-1, n), batch["next_value"].float().view(-1, n), batch["done"].float().view(-1),
                      batch["last_step"].float().view(-1), S, a.gamma, a.lambda_)
        if a.normalize_advantages:
            adv = self._union_batchnorm(self._adv_batchnorm.to(adv.device), adv)
        return adv.detach()

    def get_loss(self, batch: Batch, want=("policy", "value"), stride: Optional[int] = None):
        """ppo.py:16-71.  batch: the fields of DDPGNet.get_loss plus last_step [bs, 1], value / next_value [bs, n, 1] (what the behaviour
        critic gave at rollout time) and, for ppo_old_log_prob="stored", log_prob [bs, n, 1].  stride: the GAE chain stride (see the
        class).  The returns use FRESH behaviour-net values of next_state, the advantages the STORED ones; the target net is not read.
        No random number is drawn.  Returns (policy_loss, value_loss, (means, log_stds)); a loss not in `want` is None and its forward
        passes are skipped (the reward BatchNorm sees the rewards in every call, as the reference's does)."""
        n, a = self.n_, self.args
        rewards = self.normalise_reward(batch["reward"].float())
        valid = batch.get("valid")
        policy_loss = value_loss = action_out = None
        if "policy" in want:
            actions, avail = batch["action"], batch["action_avail"]
            means, log_stds, _ = self.policy(batch["state"], batch["last_hid"], means_grad_only=True)
            action_out = (means, log_stds)
            adv = self.advantages(batch, rewards.detach(), stride)
            old = actions if a.ppo_old_log_prob == "reference" else batch["log_prob"].float()       # models/model.py:309
            policy_loss = ppo_policy_loss(means, actions, log_stds, avail, old, adv, valid, a.eps_clip)
        if "value" in want:
            values = self.value(batch["state"]).view(-1, n)
            with torch.no_grad():
                next_values = self.value(batch["next_state"]).view(-1, n)                           # ppo.py:41, 56: the behaviour net, now
            value_loss = ppo_value_loss(values, batch["value"].float().view(-1, n), rewards.detach(), next_values, batch["done"].float().view(-1),
                                        valid, a.gamma, a.eps_clip, a.value_loss_coef)
        return policy_loss, value_loss, action_out


def net_class(alg: str):
    """the module class of an algorithm name (models/model_registry.py:14-25); KeyError for a name that is not built"""
    for c in (DDPGNet, COMANet, MAACNet, SQDDPGNet, PPONet):
        if alg in c.ALGS:
            return c
    raise KeyError(alg)


def normal_entropy(log_stds: torch.Tensor) -> torch.Tensor:
    """Normal(mean, std).entropy().mean() (utilities/util.py:37-38)"""
    return (0.5 + 0.5 * math.log(2 * math.pi) + log_stds).mean()


class PGTrainer:
    """`PGTrainer` (utilities/trainer.py:9-108) + the rollout/update schedule of `Model.train_process`,
    `transition_update` and `evaluation` (models/model.py:39-70,197-302) for a batch of B envs.

    One `run()` is one episode of every env.  `steps` counts batched steps, so with B == 1 the update
    schedule is the reference's; with B envs each update still draws `batch_size` transitions (a
    contiguous window of the (step, env)-ordered replay, see mapdn_amd/replay.py).  With
    torch.distributed initialised, gradients are averaged over ranks (one flat all-reduce per
    update) before clipping, so every rank applies the same step to identical replicas."""

    def __init__(self, args, alg: str, env, device=None, data_parallel: Optional[bool] = None):
        self.args, self.env = args, env
        self.device = torch.device(device if device is not None else getattr(env, "device", "cpu"))
        Net = net_class(alg)
        target = Net(args, alg).to(self.device) if args.target else None
        self.behaviour_net = Net(args, alg, target).to(self.device)
        self.replay_buffer = TransReplayBuffer(int(args.replay_buffer_size), device=self.device, window=int(args.batch_size))   # windows are views
        rms = dict(alpha=0.99, eps=1e-5)                                                   # trainer.py:26-27
        self.policy_optimizer = torch.optim.RMSprop(self.behaviour_net.policy_dicts.parameters(), lr=args.policy_lrate, **rms)
        self.value_optimizer = torch.optim.RMSprop(self.behaviour_net.value_dicts.parameters(), lr=args.value_lrate, **rms)
        self.steps = 0
        self.episodes = 0
        self.entr = args.entr
        import torch.distributed as dist
        self._dist = dist if (data_parallel if data_parallel is not None else (dist.is_available() and dist.is_initialized())) else None
        self.collectives = {"broadcast": 0, "all_reduce_grads": 0, "all_reduce_flag": 0, "all_reduce_reward_stats": 0}   # issued so far
        if self._dist is not None:
            def _bn_reduce(t):
                self._collective(self._dist.all_reduce, t)
                self.collectives["all_reduce_reward_stats"] += 1
            self.behaviour_net.__dict__["_dp_all_reduce"] = _bn_reduce
        self.on_policy = alg in ("coma", "mappo", "ippo")         # models/model.py:53-56: the ring is emptied after every update round
        self.ppo = isinstance(self.behaviour_net, PPONet)
        if self.ppo and env is not None:
            # rows enter the ring in (step, env) order, n_envs per insertion: row i + n_envs is the same env one step later, wherever a
            # sampled window starts — the GAE chain stride (PPONet)
            self.behaviour_net.__dict__["gae_stride"] = int(env.n_envs)
        if self._dist is not None:                               # identical replicas to start from
            for t in self.behaviour_net.state_dict().values():
                self._collective(self._dist.broadcast, t, src=0)
                self.collectives["broadcast"] += 1

    def _collective(self, fn, t: torch.Tensor, **kw):
        """fn(t, **kw) in place.  RCCL ("nccl") takes the device tensor as it is; any other backend (gloo: the CPU / one-GPU pre-flight of
        the N-rank path) gets a host copy and the result is written back."""
        if t.is_cuda and self._dist.get_backend() != "nccl":
            h = t.detach().cpu()
            fn(h, **kw)
            t.copy_(h)
        else:
            fn(t, **kw)

    # ---- one optimiser step (trainer.py:73-98) ---------------------------------------------------
    def _all_reduce_grads(self, params):
        if self._dist is None:
            return
        grads = [p.grad for p in params if p.grad is not None]
        flat = torch.cat([g.reshape(-1) for g in grads])
        self._collective(self._dist.all_reduce, flat)
        self.collectives["all_reduce_grads"] += 1
        flat /= self._dist.get_world_size()
        off = 0
        for g in grads:
            g.copy_(flat[off:off + g.numel()].view_as(g)); off += g.numel()

    def replica_fingerprint(self) -> torch.Tensor:
        """[2] float64: (sum of every state_dict value, sum of their bit patterns read as integers) — equal on every rank exactly when the
        replicas are (bit-)identical, which data-parallel training must keep them (same broadcast start, same averaged gradients, same
        optimiser arithmetic).  replicas_identical() gathers and compares it."""
        tot, bits = torch.zeros((), dtype=torch.float64, device=self.device), torch.zeros((), dtype=torch.float64, device=self.device)
        for v in self.behaviour_net.state_dict().values():
            if v.dtype == torch.float32:
                tot += v.double().sum(); bits += v.contiguous().view(torch.int32).double().sum()
            else:
                tot += v.double().sum(); bits += v.double().sum()
        return torch.stack((tot, bits))

    def replicas_identical(self) -> bool:
        if self._dist is None:
            return True
        fp = self.replica_fingerprint()
        world = self._dist.get_world_size()
        mine = fp if self._dist.get_backend() == "nccl" else fp.cpu()
        out = [torch.empty_like(mine) for _ in range(world)]
        self._dist.all_gather(out, mine)
        return all(torch.equal(o, out[0]) for o in out)

    def _apply(self, optimizer, loss, stat, key):
        optimizer.zero_grad()
        loss.backward()
        params = optimizer.param_groups[0]["params"]
        self._all_reduce_grads(params)
        norm = torch.nn.utils.clip_grad_norm_(params, self.args.grad_clip_eps)          # util.py:161-163
        optimizer.step()
        stat[f"mean_train_{key}_grad_norm"] = norm
        stat[f"mean_train_{key}_loss"] = loss.detach()

    def value_transition_process(self, stat, batch: Batch):
        _, value_loss, _ = self.behaviour_net.get_loss(batch, want=("value",))
        self._apply(self.value_optimizer, value_loss, stat, "value")

    def policy_transition_process(self, stat, batch: Batch):
        policy_loss, _, (means, log_stds) = self.behaviour_net.get_loss(batch, want=("policy",))
        stat["mean_train_policy_loss_raw"] = policy_loss.detach()
        if self.entr > 0:                                        # trainer.py:39-49
            entropy = normal_entropy(log_stds)
            policy_loss = policy_loss - self.entr * entropy
            stat["mean_train_entropy"] = entropy.detach()
        self._apply(self.policy_optimizer, policy_loss, stat, "policy")

    # ---- optional per-phase device timing of an episode (examples/train_ddpg.py --phases): CUDA events on the current stream around
    # replay insertion, batch sampling, the value / policy updates and the target update; the rollout is the rest of the episode
    profile_phases = False

    class _Phase:
        def __init__(self, trainer, name):
            self.t, self.name = trainer, name

        def __enter__(self):
            if self.t.profile_phases and self.t.device.type == "cuda":
                self.a = torch.cuda.Event(enable_timing=True); self.b = torch.cuda.Event(enable_timing=True)
                self.a.record()
            return self

        def __exit__(self, *exc):
            if self.t.profile_phases and self.t.device.type == "cuda":
                self.b.record()
                self.t._phase_events.append((self.name, self.a, self.b))

    def _phase(self, name):
        if not hasattr(self, "_phase_events"):
            self._phase_events = []
        return PGTrainer._Phase(self, name)

    def phase_seconds(self):
        """{phase: seconds} accumulated since the last call (synchronises); empty unless profile_phases"""
        out = {}
        ev = getattr(self, "_phase_events", [])
        if ev:
            torch.cuda.synchronize(self.device)
            for name, a, b in ev:
                out[name] = out.get(name, 0.0) + a.elapsed_time(b) * 1e-3
            ev.clear()
        return out

    def value_replay_process(self, stat):
        with self._phase("sample"):
            batch = self.replay_buffer.get_batch(self.args.batch_size)
        with self._phase("value_update"):
            self.value_transition_process(stat, batch)

    def policy_replay_process(self, stat):
        with self._phase("sample"):
            batch = self.replay_buffer.get_batch(self.args.batch_size)
        with self._phase("policy_update"):
            self.policy_transition_process(stat, batch)

    def _cache_targets(self) -> bool:
        """The value loss needs pi(next_state) and Q_target(next_state, pi(next_state)) of every sampled transition (maddpg.py:103-125).
        The value epochs of one update round (models/model.py:46-49: ten of them) train the behaviour CRITIC only: neither the policy
        that produces those actions nor the target critic that values them changes between the epochs, and their windows overlap
        heavily (32 of the ring's 64 steps each).  Both are therefore computed ONCE for the whole ring, in chunks of one batch — the
        same kernels on the same inputs as the per-epoch passes, same values — and handed out with the sampled windows as two more
        (temporary) fields of the replay store.  Only when that is the cheaper order: a ring longer than the transitions the round's
        value epochs sample (the reference's own defaults: a 5000-transition ring against 10 x 32) keeps the per-epoch passes.
        MAPDN_CACHE_NEXT_ACTIONS=0 disables it.
        MATD3's target is NOT constant over the round: it values tanh(mean + std·eps) with eps drawn anew in every get_loss call
        (matd3.py:119-142), so no action and no value is cached — one draw would otherwise serve every epoch that samples the transition.
        Cached is what is deterministic: the next-state policy MEANS and, for the shared critic, the target's observation term
        W_obs·next_obs_all + b1 ([ring, h]; the K = n·o product is the expensive part of the target's first layer).  The smoothed action,
        the K = n action term and the twin head are formed per epoch (DDPGNet._matd3_next_values)."""
        rb, net, a = self.replay_buffer, self.behaviour_net, self.args
        if not isinstance(rb, TransReplayBuffer) or os.environ.get("MAPDN_CACHE_NEXT_ACTIONS", "1") == "0" or len(rb) == 0:
            return False
        if net.alg == "maac":              # MAAC's target values the next actions DRAWN in every get_loss call (maac.py:98-102): nothing is cached
            return False
        if net.alg == "sqddpg":            # SQDDPG's target is valued on coalitions DRAWN in every get_loss call (sqddpg.py:145): nothing is cached
            return False
        if self.ppo:                       # MAPPO / IPPO read no target net and no next action (ppo.py:16-71): nothing to cache
            return False
        st = rb.store
        if not all(k in st for k in ("next_state", "action_avail", "hid", "action")):
            return False
        n_ring = rb.size if len(rb) == rb.size else len(rb)      # (the ring fills from position 0: a partly filled ring is [0, len))
        if n_ring > int(a.value_update_epochs) * int(a.batch_size):
            return False
        if net.alg == "matd3":
            return self._cache_matd3(n_ring)
        cache = torch.empty_like(st["action"])
        values = torch.empty(st["action"].shape[0], net.n_, dtype=torch.float32, device=cache.device) if a.target else None
        chunk = max(int(a.batch_size), 1)
        with torch.no_grad():
            for lo in range(0, n_ring, chunk):
                hi = min(lo + chunk, n_ring)
                _, na, _, _, _ = net.get_actions(st["next_state"][lo:hi], "train", False, st["action_avail"][lo:hi], not a.double_q, st["hid"][lo:hi],
                                                 means_grad_only=True)          # (only the actions are read: the new hidden state is not stored)
                cache[lo:hi] = na
                if values is not None:
                    values[lo:hi] = net.target_net.value(st["next_state"][lo:hi], na).view(-1, net.n_)
            if rb.window:
                m = min(rb.window, n_ring)
                cache[rb.size:rb.size + m] = cache[:m]
                if values is not None:
                    values[rb.size:rb.size + m] = values[:m]
        st["next_action_cached"] = cache
        if values is not None:
            st["next_value_cached"] = values
        return True

    def _cache_matd3(self, n_ring: int) -> bool:
        rb, net, a = self.replay_buffer, self.behaviour_net, self.args
        st = rb.store
        pol = net if a.double_q else (net.target_net if a.target else net)
        tgt = net.target_net
        means = torch.empty_like(st["action"])
        cr = tgt.value_dicts[0]
        term = torch.empty(st["action"].shape[0], cr.fc1.out_features, dtype=cr.fc1.weight.dtype, device=means.device) if a.shared_params else None
        chunk, no = max(int(a.batch_size), 1), net.n_ * net.obs_dim
        with torch.no_grad():
            for lo in range(0, n_ring, chunk):
                hi = min(lo + chunk, n_ring)
                means[lo:hi] = pol.policy(st["next_state"][lo:hi], st["hid"][lo:hi], True)[0]
                if term is not None:
                    term[lo:hi] = F.linear(st["next_state"][lo:hi].reshape(hi - lo, no), cr.fc1.weight[:, :no], cr.fc1.bias)
            if rb.window:
                m = min(rb.window, n_ring)
                means[rb.size:rb.size + m] = means[:m]
                if term is not None:
                    term[rb.size:rb.size + m] = term[:m]
        st["next_mean_cached"] = means
        if term is not None:
            st["next_obs_term_cached"] = term
        return True

    def transition_update(self, trans: Batch, stat):
        """models/model.py:39-70 with replay=True, mixer=False"""
        a = self.args
        with self._phase("replay_insert"):
            self.replay_buffer.add_experience(trans)
        if self.steps > a.replay_warmup and len(self.replay_buffer) >= a.batch_size and self.steps % a.behaviour_update_freq == 0:
            cached = a.value_update_epochs > 1 and self._cache_targets()
            try:
                for _ in range(a.value_update_epochs):
                    self.value_replay_process(stat)
            finally:
                if cached:
                    self.replay_buffer.store.pop("next_action_cached", None)
                    self.replay_buffer.store.pop("next_value_cached", None)
                    self.replay_buffer.store.pop("next_mean_cached", None)
                    self.replay_buffer.store.pop("next_obs_term_cached", None)
            for _ in range(a.policy_update_epochs):
                self.policy_replay_process(stat)
            if self.on_policy:                                   # COMA, MAPPO, IPPO: the ring is emptied after every update round (model.py:53-56)
                self.replay_buffer.clear()
        if a.target and self.steps % a.target_update_freq == 0:
            with self._phase("target_update"):
                self.behaviour_net.update_target()

    # ---- rollouts (models/model.py:197-302): episodes run through the package's one rollout loop (rollout.BatchedRollout) ----
    def _episode(self, stat, train: bool):
        env, net, a = self.env, self.behaviour_net, self.args
        B, dv = env.n_envs, self.device
        prefix = "mean_train_" if train else "mean_test_"
        avail = env.get_avail_actions().to(dv)

        # (MAPPO / IPPO store the log-probability of the taken action, which the one-launch exploration sample does not produce)
        fused_explore = (train and self.device.type == "cuda" and a.action_dim == 1 and a.continuous and not a.gaussian_policy and not self.ppo
                         and os.environ.get("MAPDN_FUSED_ROLLOUT", "1") != "0")
        if fused_explore:
            from . import _lib
            lib = _lib.load()
            # std = exp(log_std) with log_std = log(fixed_policy_std) (model.py:119-120, util.py:56), rounded as the f32 tensors are
            std = float(torch.tensor(math.log(a.fixed_policy_std), dtype=torch.float32).exp()) if a.shared_params else 1.0

        def policy(obs, last_hid):
            if fused_explore:
                # get_actions(status="train", exploration=True) without the log-probability nobody reads in this loop (maddpg.py:81-101,
                # util.py:52-76) and with translate_action (util.py:123-132) in the same launch: mapdn_explore_actions draws nothing itself —
                # eps is torch.randn_like(means), the same draw from the same generator as Normal(mean, std).rsample()
                means, _, hid = net.policy(obs, last_hid)
                means = means.contiguous()
                eps = torch.randn_like(means)
                action, action_pol, actual = torch.empty_like(means), torch.empty_like(means), torch.empty_like(means)
                av = avail.expand_as(means).contiguous() if avail.shape != means.shape else avail.contiguous()
                with torch.cuda.device(dv):
                    _lib.check(lib.mapdn_explore_actions(means.data_ptr(), eps.data_ptr(), av.data_ptr(), std, int(bool(a.action_enforcebound)),
                                                         float(a.action_scale), float(a.action_bias), action.data_ptr(), action_pol.data_ptr(),
                                                         actual.data_ptr(), means.numel(), torch.cuda.current_stream(dv).cuda_stream))
                return action, hid, dict(action_pol=action_pol, last_hid=last_hid, hid=hid, actual=actual)
            if train:
                action, action_pol, log_prob, _, hid = net.get_actions(obs, "train", True, avail, False, last_hid)
            else:
                action, action_pol, log_prob, _, hid = net.get_actions(obs, "test", False, avail, False, last_hid)
            return action, hid, dict(action_pol=action_pol, last_hid=last_hid, hid=hid, log_prob=log_prob)

        def on_step(t, obs, action, reward, done, info, next_obs, alive, aux):
            action_pol, last_hid, hid = aux["action_pol"], aux["last_hid"], aux["hid"]
            trans = dict(state=obs, action=action_pol, reward=reward.float().unsqueeze(-1).expand(B, net.n_).contiguous(),
                         next_state=next_obs, done=done.view(B, 1).float(),
                         last_step=(done | (t == a.max_steps - 1)).view(B, 1).float(), action_avail=avail,
                         last_hid=last_hid, hid=hid, valid=alive.clone())
            if self.ppo:                                        # models/model.py:212-222: what the behaviour net gave BEFORE this step's update
                with torch.no_grad():
                    trans.update(log_prob=aux["log_prob"], value=net.value(obs), next_value=net.value(next_obs))
            self.transition_update(trans, stat)
            self.steps += 1

        def agree(flag):                                        # data-parallel ranks must agree on the early exit: `steps` drives
            if self._dist is None:                              # the update schedule and every update is a collective
                return flag
            if self._dist.get_backend() != "nccl":
                flag = flag.cpu()
            self._dist.all_reduce(flag, op=self._dist.ReduceOp.MAX)
            self.collectives["all_reduce_flag"] += 1
            return flag

        from .rollout import BatchedRollout
        ro = BatchedRollout(env, policy, a.max_steps, on_step=on_step if train else None, store_window=False, all_alive_reduce=agree,
                            action_scale=a.action_scale, action_bias=a.action_bias)
        _, ep = ro.run(prefix=prefix, hidden=net.init_hidden(B))
        for k, v in ep.items():
            stat[k] = v if train else stat.get(k, 0.0) + v

    def train_process(self, stat):
        self._episode(stat, train=True)
        self.episodes += 1
        for k, v in list(stat.items()):
            if torch.is_tensor(v):
                stat[k] = float(v)

    def evaluation(self, stat):
        """num_eval_episodes episodes in total, B at a time (model.py:265-302)"""
        rounds = max(1, -(-self.args.num_eval_episodes // self.env.n_envs))
        test = {}
        for _ in range(rounds):
            self._episode(test, train=False)
        stat.update({k: v / rounds for k, v in test.items()})

    def run(self, stat, episode: int):
        """trainer.py:110-113"""
        self.train_process(stat)
        if episode % self.args.eval_freq == self.args.eval_freq - 1 or episode == 0:
            self.evaluation(stat)

    def save(self, path):
        torch.save({"model_state_dict": self.behaviour_net.state_dict()}, path)          # train.py:119

    def load(self, path):
        self.behaviour_net.load_state_dict(torch.load(path, map_location=self.device)["model_state_dict"])
