"""mapdn_amd.learner is a package of one module per algorithm; what callers import from it, and the one description of the critic head's
gradient block (learner/head.py) that four backward methods return their gradients through, are pinned here.  No GPU."""
import torch

from mapdn_amd import learner
from mapdn_amd.learner import head

# dir(mapdn_amd.learner) of the single-module learner, without imported modules and typing names, and without _SHAP_MAX_N: a module global
# that shapley_max_agents() rebound, which no re-export could follow and nothing outside read (the function caches its value itself now)
SURFACE = [
    "ALG_DEFAULTS", "ALG_YAML", "ATTN_MAX_N", "AttentionCritic", "Batch", "COMANet", "DDPGNet", "GaussianRNNAgent", "HEAD_MAX_FORMED_N",
    "INFO_KEYS", "MAACNet", "MLPCritic", "PGTrainer", "PPONet", "PPO_MAX_ELEMS", "RNNAgent", "SQDDPGNet", "TransReplayBuffer", "_AttentionCore",
    "_CriticHead", "_CriticHeadMSE", "_CriticHeadOwnAction", "_CriticTwinMSE", "_GRU_FUSED_OK", "_LOG_SQRT_2PI", "_LayerNorm64",
    "_LayerNorm64BC", "_PPOPolicyLoss", "_PPOValueLoss", "_PolicyTrunk", "_ReluDot64", "_ShapleyCritic", "_TallLinear", "_activation",
    "_gru_fused_ok", "_maac_args_ok", "_named_sequential", "_ppo_args_ok", "_ppo_weights", "_splitk_dw", "_sqddpg_args_ok", "_tall_ok", "_wmean",
    "attention_core", "attention_core_torch", "attention_loop_reference", "attention_ok", "critic_cf_ok", "critic_counterfactual", "critic_head",
    "critic_head_ok", "critic_twin_forward", "critic_twin_ok", "gru_cell_tall", "layernorm_act", "layernorm_act_bc", "make_alg_args", "net_class",
    "normal_entropy", "ppo_fused_ok", "ppo_gae", "ppo_gae_torch", "ppo_policy_loss", "ppo_policy_loss_torch", "ppo_value_loss",
    "ppo_value_loss_torch", "relu_dot64_ok", "sample_coalition_positions", "shapley_first_layer", "shapley_max_agents", "shapley_ok", "tall_linear",
    "tall_linear_w", "translate_action", "twin_pair_mse",
]


def test_every_name_of_the_single_module_resolves():
    missing = [n for n in SURFACE if not hasattr(learner, n)]
    assert not missing, missing
    # the launch counters the GPU tests read live on these objects
    for obj in (learner.critic_twin_forward, learner.critic_counterfactual, learner.ppo_gae, learner.twin_pair_mse, learner._CriticTwinMSE,
                learner._ShapleyCritic, learner._AttentionCore, learner._PPOPolicyLoss, learner._PPOValueLoss):
        assert isinstance(obj.launches, int)


def _ends(t):
    return tuple(t.shape), int(t.reshape(-1)[0]), int(t.reshape(-1)[-1])


def test_head_gradient_layout_is_the_c_abi():
    """include/mapdn.h, mapdn_critic_head_backward: dW2 [64][64] | dgamma | dbeta | db2 | dw3 [64 each] | db3 [1] | [4353] the loss | pad to
    4416 | dper_n [n][64]; slots in the order of the wrappers' .apply arguments (ln_w, ln_b, eps, w2, b2, w3, b3)"""
    n = 3
    gs = torch.arange(4416 + n * 64)
    dgamma, dbeta, deps, dw2, db2, dw3, db3 = head.head_param_grads(gs)
    assert deps is None
    assert _ends(dgamma) == ((64,), 4096, 4159)
    assert _ends(dbeta) == ((64,), 4160, 4223)
    assert _ends(dw2) == ((64, 64), 0, 4095) and int(dw2[1, 0]) == 64
    assert _ends(db2) == ((64,), 4224, 4287)
    assert _ends(dw3) == ((1, 64), 4288, 4351)
    assert _ends(db3) == ((1,), 4352, 4352)
    assert (head.HEAD_GRADS, head.HEAD_LOSS, head.TWIN_GRADS) == (4416, 4353, 4480)
    assert _ends(head.head_dper_n(gs, n)) == ((3, 64), 4416, 4607)


def test_twin_and_coalition_tails():
    """mapdn_critic_twin_mse: [4416 .. 4479] d flag_col | [4480 ..] dper_n [n][64]; mapdn_critic_shapley_backward: the head's 4416, then
    d id_cols [n][64], then d act_cols [n][64]"""
    n = 3
    twin = torch.arange(4480 + n * 64)
    dpn, dflag = head.twin_tails(twin, n)
    assert _ends(dflag) == ((64,), 4416, 4479)
    assert _ends(dpn) == ((3, 64), 4480, 4671)
    did, dactc = head.shapley_tails(torch.arange(4416 + 2 * n * 64), n)
    assert _ends(did) == ((3, 64), 4416, 4607)
    assert _ends(dactc) == ((3, 64), 4608, 4799)
