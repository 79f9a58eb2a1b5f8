"""ctypes binding of include/xarm_hip.h (libxarm_hip.so).  There is NO fallback: if the HIP
library is missing or cannot be loaded, importing the product path raises."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libxarm_hip.so")

XARM_OK = 0
ENV_PICK_AND_PLACE = 0
ENV_REACH = 1
ENV_HANDOVER = 2
ENV_STACK_TOWER = 3
ENV_REARRANGE = 4
REACH_REWARD_TYPES = {"sparse": 0, "dense": 1, "dense_diff": 2}
REWARD_TYPES = {"sparse": 0, "dense_o2g": 1, "dense": 2}
GOAL_SHAPES = {"air": 0, "ground": 1}
RESET_COOP_LIMIT_DEFAULT = STEP_COOP_LIMIT_DEFAULT = 8192   # include/xarm_hip.h XARM_*_COOP_LIMIT_DEFAULT

EXPORTS = ["xarm_create", "xarm_destroy", "xarm_dims", "xarm_reset", "xarm_step", "xarm_compute_reward",
           "xarm_get_state", "xarm_set_state", "xarm_episode_steps", "xarm_debug_substeps", "xarm_timing_enable", "xarm_timing_read", "xarm_timing_read_reset", "xarm_kernel_limits", "xarm_pipeline_info", "xarm_stage_info", "xarm_debug_counts", "xarm_debug_stage_counts", "xarm_class_keys", "xarm_last_error",
           "xarm_version", "xarm_default_camera", "xarm_render", "xarm_view_from_camera", "xarm_default_view", "xarm_render_views",
           "xarm_her_record_floats", "xarm_her_add", "xarm_her_sample",
           "xarm_replay_record_floats", "xarm_replay_add", "xarm_replay_sample",
           "xarm_eval_begin", "xarm_eval_step", "xarm_eval_summary",
           "xarm_norm_work_bytes", "xarm_norm_obs", "xarm_norm_step",
           "xarm_policy_act", "xarm_a2c_workspace_bytes", "xarm_a2c_update", "xarm_ppo_workspace_bytes", "xarm_ppo_update", "xarm_ppo_update_opt",
           "xarm_sac_workspace_bytes", "xarm_sac_act", "xarm_sac_update",
           "xarm_sacw_workspace_bytes", "xarm_sacw_act", "xarm_sacw_update",
           "xarm_td3_workspace_bytes", "xarm_td3_act", "xarm_td3_update",
           "xarm_acw_workspace_bytes", "xarm_acw_act", "xarm_ppow_workspace_bytes", "xarm_ppow_update", "xarm_ppow_update_opt",
           "xarm_a2cw_workspace_bytes", "xarm_a2cw_update",
           "xarm_perm_fill"]
HO_MAX_STAGES = 5           # XARM_HO_MAX_STAGES
RENDER_SHADOWS = 1          # include/xarm_hip.h XARM_RENDER_SHADOWS
RENDER_MAX_DIM = 2048       # XARM_RENDER_MAX_DIM
VIEW_FLOATS = 16            # XARM_VIEW_FLOATS: eye 0-2, target 3-5, up 6-8, fov_deg 9, near_z 10, far_z 11, mount 12
RENDER_MAX_VIEWS = 8        # XARM_RENDER_MAX_VIEWS
MOUNTS = {"world": 0, "hand0": 1, "hand1": 2}   # XARM_MOUNT_WORLD / _HAND0 / _HAND1
HER_STRATEGIES = {"future": 0, "final": 1, "episode": 2}   # XARM_HER_FUTURE / _FINAL / _EPISODE
HER_MAX_TRIES = 64          # csrc/xarm_her_core.h XARM_HER_MAX_TRIES
NORM_MAX_DIM = 96           # XARM_NORM_MAX_DIM
POLICY_MAX_DIM = 96         # XARM_POLICY_MAX_DIM
POLICY_MAX_ACT = 16         # XARM_POLICY_MAX_ACT
POLICY_HIDDEN = 64          # XARM_POLICY_HIDDEN


class XarmConfig(C.Structure):
    _fields_ = [("num_envs", C.c_int64), ("env_id_offset", C.c_int64), ("seed", C.c_uint64),
                ("env_kind", C.c_int32), ("num_obj", C.c_int32), ("reward_type", C.c_int32),
                ("goal_shape", C.c_int32), ("init_grasp_rate", C.c_float), ("goal_ground_rate", C.c_float),
                ("auto_reset", C.c_int32), ("device", C.c_int32), ("same_side_rate", C.c_float), ("reset_coop_limit", C.c_int32),
                ("step_coop_limit", C.c_int32), ("use_stand", C.c_int32)]


class XarmDims(C.Structure):
    _fields_ = [("obs_dim", C.c_int32), ("goal_dim", C.c_int32), ("act_dim", C.c_int32),
                ("state_dim", C.c_int32), ("max_episode_steps", C.c_int32), ("n_substeps", C.c_int32)]


class XarmCamera(C.Structure):
    """include/xarm_hip.h xarm_camera (52 bytes)"""
    _fields_ = [("target", C.c_float * 3), ("distance", C.c_float), ("yaw_deg", C.c_float), ("pitch_deg", C.c_float),
                ("roll_deg", C.c_float), ("fov_deg", C.c_float), ("near_z", C.c_float), ("far_z", C.c_float),
                ("width", C.c_int32), ("height", C.c_int32), ("flags", C.c_int32)]


class XarmHerLayout(C.Structure):
    """include/xarm_hip.h xarm_her_layout (20 bytes)"""
    _fields_ = [("num_envs", C.c_int32), ("horizon", C.c_int32), ("obs_dim", C.c_int32), ("goal_dim", C.c_int32),
                ("act_dim", C.c_int32)]


class XarmReplayLayout(C.Structure):
    """include/xarm_hip.h xarm_replay_layout (20 bytes)"""
    _fields_ = [("num_envs", C.c_int32), ("horizon", C.c_int32), ("obs_dim", C.c_int32), ("goal_dim", C.c_int32),
                ("act_dim", C.c_int32)]


class XarmEvalLayout(C.Structure):
    """include/xarm_hip.h xarm_eval_layout (8 bytes)"""
    _fields_ = [("num_envs", C.c_int32), ("n_eval_episodes", C.c_int32)]


class XarmNormLayout(C.Structure):
    """include/xarm_hip.h xarm_norm_layout (16 bytes)"""
    _fields_ = [("num_envs", C.c_int32), ("obs_dim", C.c_int32), ("goal_dim", C.c_int32), ("monitor_capacity", C.c_int32)]


class XarmNormParams(C.Structure):
    """include/xarm_hip.h xarm_norm_params (40 bytes)"""
    _fields_ = [("clip_obs", C.c_double), ("clip_reward", C.c_double), ("eps", C.c_double), ("gamma", C.c_float),
                ("t_seconds", C.c_float), ("update", C.c_int32)]


class XarmPolicyLayout(C.Structure):
    """include/xarm_hip.h xarm_policy_layout (32 bytes)"""
    _fields_ = [("num_envs", C.c_int32), ("obs_dim", C.c_int32), ("goal_dim", C.c_int32), ("act_dim", C.c_int32),
                ("hidden", C.c_int32), ("row_offset", C.c_int64)]


class XarmPolicyParams(C.Structure):
    """include/xarm_hip.h xarm_policy_params (32 bytes)"""
    _fields_ = [("seed", C.c_uint64), ("clip_obs", C.c_double), ("eps", C.c_double), ("deterministic", C.c_int32)]


POLICY_WEIGHT_FIELDS = ("pi_w1", "pi_b1", "pi_w2", "pi_b2", "pi_w3", "pi_b3", "vf_w1", "vf_b1", "vf_w2", "vf_b2", "vf_w3", "vf_b3", "log_std")


class XarmPolicyWeights(C.Structure):
    """include/xarm_hip.h xarm_policy_weights (13 device pointers)"""
    _fields_ = [(k, C.c_void_p) for k in POLICY_WEIGHT_FIELDS]


class XarmA2CLayout(C.Structure):
    """include/xarm_hip.h xarm_a2c_layout (20 bytes)"""
    _fields_ = [("num_envs", C.c_int32), ("n_steps", C.c_int32), ("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("hidden", C.c_int32)]


class XarmA2CParams(C.Structure):
    """include/xarm_hip.h xarm_a2c_params (56 bytes)"""
    _fields_ = [(k, C.c_double) for k in ("gamma", "lr", "alpha", "eps", "vf_coef", "ent_coef", "max_grad_norm")]


PPO_HYPER = ("gamma", "gae_lambda", "clip_range", "lr", "beta1", "beta2", "eps", "vf_coef", "ent_coef", "max_grad_norm")
PPO_MAX_STEPS = 4096        # optimiser steps per xarm_ppo_update call


class XarmPPOLayout(C.Structure):
    """include/xarm_hip.h xarm_ppo_layout (28 bytes)"""
    _fields_ = [(k, C.c_int32) for k in ("num_envs", "n_steps", "obs_dim", "act_dim", "hidden", "n_epochs", "batch_size")]


class XarmPPOParams(C.Structure):
    """include/xarm_hip.h xarm_ppo_params (88 bytes)"""
    _fields_ = [(k, C.c_double) for k in PPO_HYPER] + [("normalize_advantage", C.c_int32)]


class XarmPPOOptions(C.Structure):
    """include/xarm_hip.h xarm_ppo_options (16 bytes); 0 = off"""
    _fields_ = [("clip_range_vf", C.c_double), ("target_kl", C.c_double)]


SAC_MAX_ACT = 8             # XARM_SAC_MAX_ACT
SAC_HYPER = ("gamma", "lr", "tau", "ent_coef", "target_entropy", "beta1", "beta2", "eps")
SAC_TOWERS = ("actor", "q1", "q2", "q1_target", "q2_target")


class XarmSACLayout(C.Structure):
    """include/xarm_hip.h xarm_sac_layout (24 bytes)"""
    _fields_ = [(k, C.c_int32) for k in ("batch_size", "obs_dim", "act_dim", "hidden")] + [("row_offset", C.c_int64)]


class XarmSACParams(C.Structure):
    """include/xarm_hip.h xarm_sac_params (80 bytes)"""
    _fields_ = [("seed", C.c_uint64)] + [(k, C.c_double) for k in SAC_HYPER] + [("auto_ent_coef", C.c_int32), ("deterministic", C.c_int32)]


class XarmSACWeights(C.Structure):
    """include/xarm_hip.h xarm_sac_weights (31 device pointers): five towers of W1, b1, W2, b2, W3, b3 and log_alpha"""
    _fields_ = [(k, C.c_void_p * 6) for k in SAC_TOWERS] + [("log_alpha", C.c_void_p)]


SACW_MAX_LAYERS = 3         # XARM_SACW_MAX_LAYERS
SACW_WIDTHS = (64, 128, 192, 256)
SACW_ACTIVATIONS = {"tanh": 0, "relu": 1}   # XARM_SACW_TANH, XARM_SACW_RELU


class XarmSACWLayout(C.Structure):
    """include/xarm_hip.h xarm_sacw_layout (32 bytes)"""
    _fields_ = [(k, C.c_int32) for k in ("batch_size", "obs_dim", "act_dim", "hidden", "n_hidden", "activation")] + [("row_offset", C.c_int64)]


class XarmSACWWeights(C.Structure):
    """include/xarm_hip.h xarm_sacw_weights (41 device pointers): five towers of W1, b1, ..., W_out, b_out (eight slots) and log_alpha"""
    _fields_ = [(k, C.c_void_p * (2 * (SACW_MAX_LAYERS + 1))) for k in SAC_TOWERS] + [("log_alpha", C.c_void_p)]


TD3_HYPER = ("gamma", "lr", "tau", "beta1", "beta2", "eps", "target_policy_noise", "target_noise_clip", "action_noise")
TD3_TOWERS = ("actor", "q1", "q2", "actor_target", "q1_target", "q2_target")
TD3_MODES = {"deterministic": 0, "gaussian": 1, "uniform": 2}


class XarmTD3Params(C.Structure):
    """include/xarm_hip.h xarm_td3_params (88 bytes)"""
    _fields_ = [("seed", C.c_uint64)] + [(k, C.c_double) for k in TD3_HYPER] + [("policy_delay", C.c_int32), ("mode", C.c_int32)]


class XarmTD3Weights(C.Structure):
    """include/xarm_hip.h xarm_td3_weights (48 device pointers): six towers of W1, b1, ..., W_out, b_out (eight slots)"""
    _fields_ = [(k, C.c_void_p * (2 * (SACW_MAX_LAYERS + 1))) for k in TD3_TOWERS]


class XarmACWLayout(C.Structure):
    """include/xarm_hip.h xarm_acw_layout (40 bytes)"""
    _fields_ = [(k, C.c_int32) for k in ("num_rows", "obs_dim", "goal_dim", "act_dim", "hidden", "n_hidden", "activation")] + [("row_offset", C.c_int64)]


class XarmACWWeights(C.Structure):
    """include/xarm_hip.h xarm_acw_weights (17 device pointers): pi and vf as W1, b1, ..., W_out, b_out (eight slots each) and log_std"""
    _fields_ = [("pi", C.c_void_p * (2 * (SACW_MAX_LAYERS + 1))), ("vf", C.c_void_p * (2 * (SACW_MAX_LAYERS + 1))), ("log_std", C.c_void_p)]


class XarmPPOWLayout(C.Structure):
    """include/xarm_hip.h xarm_ppow_layout (36 bytes)"""
    _fields_ = [(k, C.c_int32) for k in ("num_envs", "n_steps", "obs_dim", "act_dim", "hidden", "n_hidden", "activation", "n_epochs", "batch_size")]


class XarmA2CWLayout(C.Structure):
    """include/xarm_hip.h xarm_a2cw_layout (28 bytes)"""
    _fields_ = [(k, C.c_int32) for k in ("num_envs", "n_steps", "obs_dim", "act_dim", "hidden", "n_hidden", "activation")]


class XarmNativeError(RuntimeError):
    pass


_lib = None


def load(path=None):
    """Load libxarm_hip.so and declare every entry point of include/xarm_hip.h."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # XARM_HIP_LIB: a development variant of the library (tools/coop_split.sh, tools/variant_time.sh) loaded from its own
    # path; xarm_version() tells a timing variant from the product build.  Still no fallback: a missing file raises.
    p = path or os.environ.get("XARM_HIP_LIB") or LIB_PATH
    if not os.path.exists(p):
        raise XarmNativeError(
            "HIP extension %s not found: build it with `python -m gym_xarm_amd.build` (hipcc, gfx950). "
            "gym_xarm_amd has no CPU fallback." % p)
    L = C.CDLL(p)
    vp, fp, u8p = C.c_void_p, C.c_void_p, C.c_void_p  # device pointers travel as integers
    L.xarm_create.argtypes = [C.POINTER(XarmConfig), C.POINTER(C.c_void_p)]
    L.xarm_destroy.argtypes = [vp]
    L.xarm_dims.argtypes = [vp, C.POINTER(XarmDims)]
    L.xarm_reset.argtypes = [vp, u8p, fp, fp, fp, vp]
    L.xarm_step.argtypes = [vp, fp, fp, fp, fp, fp, u8p, u8p, fp, vp]
    L.xarm_compute_reward.argtypes = [vp, fp, fp, C.c_int64, fp, vp]
    L.xarm_get_state.argtypes = [vp, fp, vp]
    L.xarm_set_state.argtypes = [vp, fp, vp]
    L.xarm_episode_steps.argtypes = [vp, fp, vp]
    L.xarm_debug_substeps.argtypes = [vp, fp, C.c_int32, vp]
    L.xarm_timing_enable.argtypes = [vp, C.c_int32]
    L.xarm_timing_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.xarm_timing_read_reset.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.xarm_kernel_limits.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.xarm_pipeline_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.xarm_stage_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.xarm_debug_counts.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp]
    L.xarm_debug_stage_counts.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp]
    L.xarm_class_keys.argtypes = [vp, vp, vp]
    L.xarm_default_camera.argtypes = [vp, C.POINTER(XarmCamera)]
    L.xarm_render.argtypes = [vp, C.POINTER(XarmCamera), vp, C.c_int32, vp, vp, vp, vp]
    L.xarm_view_from_camera.argtypes = [C.POINTER(XarmCamera), C.POINTER(C.c_float)]
    L.xarm_default_view.argtypes = [vp, C.c_int32, C.POINTER(C.c_float)]
    L.xarm_render_views.argtypes = [vp, fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, vp, fp, u8p, vp]
    hl = C.POINTER(XarmHerLayout)
    L.xarm_her_record_floats.argtypes = [hl]
    L.xarm_her_add.argtypes = [hl] + [vp] * 14
    L.xarm_her_sample.argtypes = [hl, vp, vp, vp, vp, C.c_uint64, C.c_int32, C.c_int32, C.c_int32] + [vp] * 14
    rl = C.POINTER(XarmReplayLayout)
    L.xarm_replay_record_floats.argtypes = [rl]
    L.xarm_replay_add.argtypes = [rl] + [vp] * 12
    L.xarm_replay_sample.argtypes = [rl, vp, vp, C.c_uint64, C.c_int32, C.c_int32, vp, C.c_double, C.c_double] + [vp] * 9
    el = C.POINTER(XarmEvalLayout)
    L.xarm_eval_begin.argtypes = [el] + [vp] * 6
    L.xarm_eval_step.argtypes = [el] + [vp] * 10
    L.xarm_eval_summary.argtypes = [el] + [vp] * 4
    nl, npar = C.POINTER(XarmNormLayout), C.POINTER(XarmNormParams)
    L.xarm_norm_work_bytes.argtypes = [nl, C.POINTER(C.c_int64)]
    L.xarm_norm_obs.argtypes = [nl, npar] + [vp] * 6 + [C.c_int32, vp, vp]
    L.xarm_norm_step.argtypes = [nl, npar] + [vp] * 16
    L.xarm_policy_act.argtypes = [C.POINTER(XarmPolicyLayout), C.POINTER(XarmPolicyParams), C.POINTER(XarmPolicyWeights)] + [vp] * 10
    al = C.POINTER(XarmA2CLayout)
    L.xarm_a2c_workspace_bytes.argtypes = [al, C.POINTER(C.c_int64)]
    L.xarm_a2c_update.argtypes = [al, C.POINTER(XarmA2CParams), C.POINTER(XarmPolicyWeights), C.POINTER(XarmPolicyWeights)] + [vp] * 11
    pl = C.POINTER(XarmPPOLayout)
    L.xarm_ppo_workspace_bytes.argtypes = [pl, C.POINTER(C.c_int64)]
    L.xarm_ppo_update.argtypes = [pl, C.POINTER(XarmPPOParams)] + [C.POINTER(XarmPolicyWeights)] * 3 + [vp] * 15
    L.xarm_ppo_update_opt.argtypes = [pl, C.POINTER(XarmPPOParams)] + [C.POINTER(XarmPolicyWeights)] * 3 + [vp] * 14 + [C.POINTER(XarmPPOOptions), vp]
    sl, sp, sw = C.POINTER(XarmSACLayout), C.POINTER(XarmSACParams), C.POINTER(XarmSACWeights)
    L.xarm_sac_workspace_bytes.argtypes = [sl, C.POINTER(C.c_int64)]
    L.xarm_sac_act.argtypes = [sl, sp, sw] + [vp] * 5
    L.xarm_sac_update.argtypes = [sl, sp, sw, sw, sw] + [vp] * 15
    wl, ww = C.POINTER(XarmSACWLayout), C.POINTER(XarmSACWWeights)
    L.xarm_sacw_workspace_bytes.argtypes = [wl, C.POINTER(C.c_int64)]
    L.xarm_sacw_act.argtypes = [wl, sp, ww] + [vp] * 6
    L.xarm_sacw_update.argtypes = [wl, sp, ww, ww, ww] + [vp] * 16
    tp_, tw = C.POINTER(XarmTD3Params), C.POINTER(XarmTD3Weights)
    L.xarm_td3_workspace_bytes.argtypes = [wl, C.POINTER(C.c_int64)]
    L.xarm_td3_act.argtypes = [wl, tp_, tw] + [vp] * 5
    L.xarm_td3_update.argtypes = [wl, tp_, tw, tw, tw] + [vp] * 15
    cl = C.POINTER(XarmACWLayout)
    L.xarm_acw_workspace_bytes.argtypes = [cl, C.POINTER(C.c_int64)]
    L.xarm_acw_act.argtypes = [cl, C.POINTER(XarmPolicyParams), C.POINTER(XarmACWWeights)] + [vp] * 11
    ql, cw = C.POINTER(XarmPPOWLayout), C.POINTER(XarmACWWeights)
    L.xarm_ppow_workspace_bytes.argtypes = [ql, C.POINTER(C.c_int64)]
    L.xarm_ppow_update.argtypes = [ql, C.POINTER(XarmPPOParams), cw, cw, cw] + [vp] * 15
    L.xarm_ppow_update_opt.argtypes = [ql, C.POINTER(XarmPPOParams), cw, cw, cw] + [vp] * 14 + [C.POINTER(XarmPPOOptions), vp]
    wa = C.POINTER(XarmA2CWLayout)
    L.xarm_a2cw_workspace_bytes.argtypes = [wa, C.POINTER(C.c_int64)]
    L.xarm_a2cw_update.argtypes = [wa, C.POINTER(XarmA2CParams), cw, cw] + [vp] * 11
    L.xarm_perm_fill.argtypes = [vp, C.c_int32, C.c_int64, C.c_uint64, vp, vp]
    L.xarm_last_error.argtypes = [vp]
    L.xarm_last_error.restype = C.c_char_p
    L.xarm_version.argtypes = []
    L.xarm_version.restype = C.c_char_p
    for name in EXPORTS:
        if name not in ("xarm_last_error", "xarm_version"):
            getattr(L, name).restype = C.c_int
    if path is None:
        _lib = L
    return L


def loaded_path():
    """the file the product path bound: csrc/libxarm_hip.so, or a development variant named by XARM_HIP_LIB"""
    return os.environ.get("XARM_HIP_LIB") or LIB_PATH


def check(L, handle, rc, what):
    if rc != XARM_OK:
        msg = L.xarm_last_error(handle)
        raise XarmNativeError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))
