"""ctypes binding of libsfmi.so (include/sfmi.h).

Fails loudly: if the HIP extension is missing or no GPU is usable there is NO
fallback -- importing works (so host-only helpers and symbol checks run on a
CPU box), but creating a batch raises.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# SFMI_LIB_PATH: load a differently-built libsfmi (profiling / ablation builds); still HIP-only
LIB_PATH = os.environ.get("SFMI_LIB_PATH") or os.path.join(HERE, "libsfmi.so")

SF_OK = 0
SF_ERR_PRESET, SF_ERR_ARG, SF_ERR_HIP, SF_ERR_NO_DEVICE, SF_ERR_ACTION, SF_ERR_FIELD, SF_ERR_STATE = -1, -2, -3, -4, -5, -6, -7
OBS_TYPES = {"features": 0, "normalized-features": 1, "monitors": 2, "none": 3, "image": 4, "image-raw": 5}
IMAGE_W, IMAGE_H, IMAGE_OUT = 90, 92, 84
# SF_EV_* (include/sfmi.h): bit -> the reference's event string, in the order Game::stepOneTick can emit them
EVENT_NAMES = {0x1: "press-fire", 0x2: "press-thrust", 0x4: "press-left", 0x8: "press-right", 0x10: "release-fire",
               0x20: "release-thrust", 0x40: "release-left", 0x80: "release-right", 0x100: "missile-fired",
               0x200: "ship-respawn", 0x400: "explode-bighex", 0x800: "explode-smallhex", 0x1000: "fortress-respawn",
               0x2000: "fortress-fired", 0x4000: "shell-hit-ship", 0x8000: "hit-fortress", 0x10000: "vlner-increased",
               0x20000: "fortress-destroyed", 0x40000: "vlner-reset", 0x80000: "hit-dead-fortress",
               0x100000: "missile-left", 0x200000: "game-over"}
FLAG_OBS_F64 = 1
FLAG_REAL_SHELL_COUNT = 2
FLAG_NO_AUTO_RESET = 4
FLAG_REF_RESET_OBS = 8
EPISODE_STATS_LEN = 8
# lane-state rows (sfmi.h: sf_save_lanes): SF_LANE_STATE_BYTES per env, a 16-byte header of four uint32 words
LANE_STATE_BYTES = 1136
LANE_STATE_MAGIC = 0x53464C00
LANE_STATE_VERSION = 1
ACT_I32, ACT_I64 = 4, 8
STACK_U8, STACK_F16, STACK_F32 = 1, 2, 4  # SF_STACK_* (sfmi.h: sf_gather_stacks)
EPISODE_RECORD_BYTES = 32  # sizeof(sf_episode_record) (sfmi.h: sf_eplog_read)


class SfmiError(RuntimeError):
    pass


class CreateParams(C.Structure):
    _fields_ = [
        ("gametype", C.c_char_p), ("n_envs", C.c_int32), ("device_id", C.c_int32), ("action_set", C.c_int32),
        ("obs_type", C.c_int32), ("flags", C.c_uint32), ("seed", C.c_uint32), ("spawn_skip", C.c_int32),
        ("spawn_stride", C.c_int32), ("spawn_table_len", C.c_int32),
    ]


class FieldDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("elem_size", C.c_int32), ("count", C.c_int32), ("is_float", C.c_int32)]


class Preset(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("game_time", C.c_int32),
        ("destroy_fortress", C.c_int32), ("ship_death_penalty", C.c_int32),
        ("missile_penalty", C.c_double), ("miss_penalty", C.c_int32),
        ("shell_speed", C.c_int32), ("shell_radius", C.c_int32), ("missile_speed", C.c_int32),
        ("missile_radius", C.c_int32), ("auto_turn", C.c_int32),
        ("sector_size", C.c_int32), ("lock_time", C.c_int32), ("vuln_time", C.c_int32),
        ("vuln_threshold", C.c_int32), ("fortress_radius", C.c_int32),
        ("big_hex", C.c_int32), ("small_hex", C.c_int32), ("explode_duration", C.c_int32),
        ("start_vx", C.c_double), ("start_vy", C.c_double), ("ship_radius", C.c_int32),
        ("ship_accel", C.c_double), ("turn_speed", C.c_int32), ("shaped", C.c_int32), ("n_keys", C.c_int32),
    ]


class ScoreGlyphs(C.Structure):
    """sf_score_glyphs (include/sfmi.h): the layout of a score-text glyph atlas"""
    _fields_ = [("gw", C.c_int32), ("gh", C.c_int32), ("advance", C.c_int32), ("y0", C.c_int32), ("x0", (C.c_int16 * 10) * 11)]


VIEW_FORMATS = {"bgrx": 0, "rgb": 1, "gray": 2}  # SF_VIEW_* (include/sfmi.h)


class View(C.Structure):
    """sf_view (include/sfmi.h): a view of sf_render_view"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("vp_x", C.c_double), ("vp_y", C.c_double), ("vp_w", C.c_double),
                ("vp_h", C.c_double), ("line_width", C.c_double), ("grayscale", C.c_int32), ("format", C.c_int32),
                ("glyphs", C.POINTER(ScoreGlyphs)), ("glyph_alpha", C.c_void_p)]


# every symbol include/sfmi.h declares: (restype, argtypes)
SYMBOLS = {
    "sf_create": (C.c_int, [C.POINTER(CreateParams), C.POINTER(C.c_void_p)]),
    "sf_destroy": (C.c_int, [C.c_void_p]),
    "sf_n_envs": (C.c_int, [C.c_void_p]),
    "sf_obs_dim": (C.c_int, [C.c_void_p]),
    "sf_n_actions": (C.c_int, [C.c_void_p]),
    "sf_tick_ms": (C.c_int, [C.c_void_p]),
    "sf_max_ticks": (C.c_int, [C.c_void_p]),
    "sf_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "sf_reset_lanes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sf_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sf_rollout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sf_check_actions": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sf_check_state": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sf_clear_state_errors": (C.c_int, [C.c_void_p]),
    "sf_seed_actions": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    "sf_step_sampled": (C.c_int, [C.c_void_p] * 7),
    "sf_rollout_sampled": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 6),
    "sf_n_fields": (C.c_int, []),
    "sf_field_info": (C.c_int, [C.c_int, C.POINTER(FieldDesc)]),
    "sf_field_id": (C.c_int, [C.c_char_p]),
    "sf_get_field": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "sf_set_field": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "sf_get_field_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sf_episode_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "sf_calibration_copy": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]),
    "sf_draw_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "sf_set_image_geometry": (C.c_int, [C.c_void_p] + [C.c_double] * 6),
    "sf_image_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sf_image_geometry_is_default": (C.c_int, [C.c_void_p]),
    "sf_set_score_glyphs": (C.c_int, [C.c_void_p, C.POINTER(ScoreGlyphs), C.c_void_p]),
    "sf_get_score_glyphs": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(ScoreGlyphs), C.c_void_p, C.c_size_t]),
    "sf_default_score_glyphs": (C.c_int, [C.POINTER(ScoreGlyphs), C.c_void_p, C.c_size_t]),
    "sf_view_check": (C.c_int, [C.POINTER(View), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sf_view_size": (C.c_int, [C.c_void_p, C.POINTER(View), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "sf_render_view": (C.c_int, [C.c_void_p, C.POINTER(View), C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sf_view_circle_segments": (C.c_int, [C.c_double] * 5),
    "sf_preset_get": (C.c_int, [C.c_char_p, C.POINTER(Preset)]),
    "sf_action_table": (C.c_int, [C.c_char_p, C.c_int, C.c_void_p]),
    "sf_spawn_table": (C.c_int, [C.c_uint32, C.c_int, C.c_void_p]),
    "sf_trig_table": (C.c_int, [C.c_void_p]),
    "sf_hex_points": (C.c_int, [C.c_int, C.c_void_p]),
    "sf_normalizer_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "sf_normalizer_destroy": (C.c_int, [C.c_void_p]),
    "sf_normalize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "sf_step_normalize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]),
    "sf_normalizer_get_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sf_normalizer_set_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sf_step_record": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 10),
    "sf_record_step_f32": (C.c_int, [C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.c_void_p]),
    "sf_record_step": (C.c_int, [C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.c_void_p]),
    "sf_compute_returns": (C.c_int, [C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_double, C.c_double, C.c_void_p]),
    "sf_gather_stacks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_int64,
                                   C.c_int64, C.c_void_p, C.c_int, C.c_void_p]),
    "sf_gather_errors": (C.c_int, [C.POINTER(C.c_uint64), C.c_int, C.c_void_p]),
    "sf_eplog_create": (C.c_int, [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "sf_eplog_destroy": (C.c_int, [C.c_void_p]),
    "sf_eplog_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "sf_eplog_restart": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sf_eplog_clear": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sf_eplog_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p]),
    "sf_render_stack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sf_render_shift": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "sf_frame_stack_clear": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]),
    "sf_set_event_output": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sf_set_final_obs_output": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sf_compute_returns_tl": (C.c_int, [C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_double, C.c_double, C.c_void_p]),
    "sf_render": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "sf_image_background": (C.c_int, [C.c_void_p]),
    "sf_image_background_geom": (C.c_int, [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    "sf_image_fort_alpha": (C.c_int, [C.c_int, C.c_void_p]),
    "sf_arc_table": (C.c_int, [C.c_void_p]),
    "sf_image_object_alpha": (C.c_int, [C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int] + [C.c_double] * 5 + [C.c_void_p]),
    "sf_image_explosion_host": (C.c_int, [C.c_double, C.c_double, C.c_int, C.c_int] + [C.c_double] * 5 + [C.c_void_p]),
    "sf_trig_deg": (C.c_int, [C.c_int, C.c_void_p]),
    "sf_image_arc_alpha": (C.c_int, [C.c_double] * 5 + [C.c_int, C.c_int] + [C.c_double] * 5 + [C.c_void_p]),
    "sf_image_static": (C.c_int, [C.c_int, C.c_void_p]),
    "sf_resize_area_tab": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sf_resize_area_u8": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]),
    "sf_set_render_order_hint": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "sf_lane_state_bytes": (C.c_int, []),
    "sf_lane_state_header": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sf_save_lanes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sf_load_lanes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sf_copy_lanes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sf_check_lanes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sf_last_error": (C.c_char_p, []),
    "sf_version": (C.c_int, []),
    "sf_build_id": (C.c_char_p, []),
}

# every symbol include/sfmi_masked.h declares (the masked companions of sf_reset_lanes): bound like SYMBOLS
MASKED_SYMBOLS = {
    "sf_eplog_restart_where": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
}

# every symbol include/sfmi_repeat.h declares (action repeat): bound like SYMBOLS
REPEAT_SYMBOLS = {
    "sf_step_repeat": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6),
}

# every symbol include/sfmi_hold.h declares (the masked step): bound like SYMBOLS
HOLD_SYMBOLS = {
    "sf_step_where": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6),
}

# every symbol include/sfmi_final.h declares (final frames of image batches): bound like SYMBOLS
FINAL_SYMBOLS = {
    "sf_set_final_frame_output": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "sf_final_stack_shift": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]),
}

# every symbol include/sfmi_policy.h declares (the policy head): bound like SYMBOLS
POLICY_SYMBOLS = {
    "sf_policy_sample": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}
POLICY_SAMPLE, POLICY_ARGMAX, POLICY_MAX_ACTIONS = 0, 1, 32  # SF_POLICY_* (sfmi_policy.h)

# every symbol include/sfmi_ppo.h declares (the policy head's update side: evaluate_actions, the PPO loss): bound like SYMBOLS
_PPO_IN = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_size_t, C.c_int] + [C.c_float] * 4  # logits .. returns, shape, clip, coefficients
PPO_SYMBOLS = {
    "sf_policy_evaluate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "sf_policy_evaluate_backward": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_size_t, C.c_void_p]),
    "sf_ppo_loss_workspace_bytes": (C.c_size_t, [C.c_int]),
    "sf_ppo_loss": (C.c_int, _PPO_IN + [C.c_void_p] * 5),
    "sf_ppo_loss_backward": (C.c_int, _PPO_IN + [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
}

# every symbol include/sfmi_minibatch.h declares (normalised advantages, one-launch minibatch gathers): bound like SYMBOLS
MB_MAX_COLUMNS, MB_MAX_ROW_BYTES = 8, 65536  # SF_MB_* (sfmi_minibatch.h)


class MbColumn(C.Structure):
    """sf_mb_column (include/sfmi_minibatch.h): one column of a minibatch gather"""
    _fields_ = [("src_dev", C.c_void_p), ("row_bytes", C.c_size_t), ("dst_dev", C.c_void_p)]


MINIBATCH_SYMBOLS = {
    "sf_advantages_workspace_bytes": (C.c_size_t, [C.c_int]),
    "sf_advantages": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_double] + [C.c_void_p] * 5),
    "sf_minibatch_gather": (C.c_int, [C.POINTER(MbColumn), C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p,
                                      C.c_uint32, C.c_uint32, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# every symbol include/sfmi_optim.h declares (grad-norm clip and Adam, fused): bound like SYMBOLS
OPT_MAX_TENSORS, OPT_CHUNK, ADAM_STATE_BYTES = 64, 2048, 128  # SF_OPT_* / SF_ADAM_STATE_BYTES (sfmi_optim.h)


class OptTensor(C.Structure):
    """sf_opt_tensor (include/sfmi_optim.h): one tensor of an optimiser step"""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("numel", C.c_int64)]


OPTIM_SYMBOLS = {
    "sf_adam_chunks": (C.c_int64, [C.c_int64]),
    "sf_adam_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "sf_adam_state_bytes": (C.c_size_t, []),
    "sf_adam_state_init": (C.c_int, [C.c_void_p] + [C.c_double] * 4 + [C.c_void_p]),
    "sf_adam_step": (C.c_int, [C.POINTER(OptTensor), C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# what the wrappers answer to `.reset_lanes`: their per-env memory would go stale behind a masked reset
NO_RESET_LANES = ("%s has no reset_lanes(): its per-env memory (frame stacks, return accumulators, start flags, masks) has no "
                  "rule for a masked reset yet.  Call SFVecEnv.reset_lanes on the bare env and rebuild the wrapper's state, or "
                  "use reset()")

_lib = None


def lib():
    """Load libsfmi.so; raises SfmiError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SfmiError(
                "libsfmi.so is missing (%s): build it with `python -m spacefortress_amd.build` "
                "(there is no CPU fallback)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SYMBOLS.items()) + list(MASKED_SYMBOLS.items()) + list(REPEAT_SYMBOLS.items()) \
                + list(HOLD_SYMBOLS.items()) + list(FINAL_SYMBOLS.items()) + list(POLICY_SYMBOLS.items()) + list(PPO_SYMBOLS.items()) \
                + list(MINIBATCH_SYMBOLS.items()) + list(OPTIM_SYMBOLS.items()):
            if not hasattr(L, name) and os.environ.get("SFMI_LIB_PATH"):
                continue  # an older diagnostic build (A/B against an earlier round's library): entry points added since
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def last_error():
    return lib().sf_last_error().decode("utf-8", "replace")


def check(rc):
    """Map sf_status to the exception class the reference raises for the same misuse."""
    if rc >= 0:
        return rc
    msg = last_error()
    if rc == SF_ERR_PRESET:
        raise RuntimeError(msg)  # SRC/pymodule.cpp:341
    if rc == SF_ERR_ARG:
        raise ValueError(msg)
    if rc == SF_ERR_ACTION:
        raise IndexError(msg)  # ENV:211-212
    if rc == SF_ERR_FIELD:
        raise KeyError(msg)
    if rc == SF_ERR_STATE:
        raise OverflowError(msg)
    raise SfmiError("libsfmi: %s (status %d)" % (msg, rc))


def ptr(t):
    """The address of a tensor for the C ABI; None stays None (an optional output)."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def act_types():
    """torch dtype of an action tensor -> SF_ACT_* (sfmi.h: the element size); THE table, read once by SFVecEnv's module."""
    import torch
    return {torch.uint8: 1, torch.int32: ACT_I32, torch.int64: ACT_I64}


def score_glyphs(alpha, layout, x0):
    """(ScoreGlyphs, the uint8 [11, gh, gw] array to pass beside it) of an atlas as score_glyphs() gives it: alpha, layout =
    (gw, gh, advance, y0), x0 int [11, 10] or one int.  Keep both alive across the call that takes their addresses."""
    import numpy as np
    a = np.ascontiguousarray(alpha, np.uint8)
    gw, gh, adv, y0 = (int(v) for v in layout)
    if a.shape != (11, gh, gw):
        raise ValueError("alpha must be uint8 [11, gh, gw] = [11, %d, %d]" % (gh, gw))
    g = ScoreGlyphs(gw, gh, adv, y0)
    xs = np.broadcast_to(np.asarray(x0, np.int16), (11, 10))
    for i in range(11):
        for j in range(10):
            g.x0[i][j] = int(xs[i, j])
    return g, a


def raw_stream(device):
    """The current HIP stream of `device` as a ctypes pointer.  torch.cuda.current_stream(...).cuda_stream builds a
    Stream object per call (4 us of the 8 us a step launch costs on the host); the raw getter does not."""
    import torch
    idx = device.index if device.index is not None else torch.cuda.current_device()
    get = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if get is not None:
        return C.c_void_p(get(idx))
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
