"""MADDPG / IDDPG / MATD3 / COMA / MAAC / SQDDPG / MAPPO / IPPO learners for the batched env (BASELINE.json configs[4]).
What is learned, and every quirk of how, follows the reference (file:line cited at each piece); module and parameter names are the
reference's, so a reference `model.pt` (`{"model_state_dict": …}`, train.py:119) loads with `strict=True` and vice versa.  What differs is
how it runs: tensors in, tensors out, no Python lists or host round trips, the hot paths as HIP launches.

    args.py     make_alg_args: args/default.yaml + args/alg_args/*.yaml, and what each net class accepts
    _hip.py     launch / buffer: the one way into libmapdn_hip.so
    ops.py      LayerNorm + ReLU, ReLU + fc3, tall linear layers and their split weight gradients
    head.py     the critic behind its first layer: head, value loss, MATD3's twin, COMA's baseline; the head's parameter and gradient layout
    modules.py  RNNAgent, GaussianRNNAgent, MLPCritic, the agent trunk of the policy update
    ddpg.py     DDPGNet (MADDPG / IDDPG / MATD3), the base of COMANet (coma.py), MAACNet (maac.py), SQDDPGNet (sqddpg.py), PPONet (ppo.py)
    trainer.py  net_class, PGTrainer
Every name below is importable from here, as when this was one module."""
from .._lib import INFO_KEYS
from ..replay import TransReplayBuffer
from ..rollout import translate_action
from .args import ALG_DEFAULTS, ALG_YAML, Batch, _activation, _maac_args_ok, _ppo_args_ok, _sqddpg_args_ok, make_alg_args
from .coma import COMANet
from .ddpg import DDPGNet, _wmean
from .head import (HEAD_MAX_FORMED_N, _CriticHead, _CriticHeadMSE, _CriticHeadOwnAction, _CriticTwinMSE, critic_cf_ok, critic_counterfactual,
                   critic_head, critic_head_ok, critic_twin_forward, critic_twin_ok, twin_pair_mse)
from .maac import (ATTN_MAX_N, AttentionCritic, MAACNet, _AttentionCore, _named_sequential, attention_core, attention_core_torch,
                   attention_loop_reference, attention_ok)
from .modules import GaussianRNNAgent, MLPCritic, RNNAgent, _PolicyTrunk
from .ops import (_GRU_FUSED_OK, _LayerNorm64, _LayerNorm64BC, _ReluDot64, _TallLinear, _gru_fused_ok, _splitk_dw, _tall_ok, gru_cell_tall,
                  layernorm_act, layernorm_act_bc, relu_dot64_ok, tall_linear, tall_linear_w)
from .ppo import (_LOG_SQRT_2PI, PPO_MAX_ELEMS, PPONet, _PPOPolicyLoss, _PPOValueLoss, _ppo_weights, ppo_fused_ok, ppo_gae, ppo_gae_torch,
                  ppo_policy_loss, ppo_policy_loss_torch, ppo_value_loss, ppo_value_loss_torch)
from .sqddpg import SQDDPGNet, _ShapleyCritic, sample_coalition_positions, shapley_first_layer, shapley_max_agents, shapley_ok
from .trainer import PGTrainer, net_class, normal_entropy
