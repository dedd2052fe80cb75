"""ctypes binding of libbalatro_mi355x.so (the C ABI in include/balatro_mi355x.h).

The HIP library is the ONLY compute path: loading fails loudly if it is missing or cannot be built, and bg_create
fails if no HIP device is visible.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

from . import build as _build

OBS_KEYS = [
    "hand", "hand_size", "deck_size", "selected_cards", "chips_scored", "round_chips_scored", "progress_ratio",
    "mult", "chips_needed", "money", "ante", "round", "hands_left", "discards_left", "joker_count", "joker_ids",
    "joker_slots", "consumable_count", "consumables", "consumable_slots", "shop_items", "shop_costs",
    "shop_rerolls", "hand_levels", "phase", "action_mask", "hands_played", "best_hand_this_ante",
    "boss_blind_active", "boss_blind_type", "face_down_cards",
]
# key -> (torch/numpy dtype name, trailing shape) in the reference's dtypes (balatro_env_2.py:1488-1531)
OBS_SPEC = {
    "hand": ("int8", (8,)), "hand_size": ("int8", ()), "deck_size": ("int8", ()), "selected_cards": ("int64", (8,)),
    "chips_scored": ("int64", ()), "round_chips_scored": ("int32", ()), "progress_ratio": ("float32", ()),
    "mult": ("int32", ()), "chips_needed": ("int32", ()), "money": ("int32", ()), "ante": ("int16", ()),
    "round": ("int8", ()), "hands_left": ("int8", ()), "discards_left": ("int8", ()), "joker_count": ("int8", ()),
    "joker_ids": ("int16", (10,)), "joker_slots": ("int8", ()), "consumable_count": ("int8", ()),
    "consumables": ("int16", (5,)), "consumable_slots": ("int8", ()), "shop_items": ("int16", (10,)),
    "shop_costs": ("int16", (10,)), "shop_rerolls": ("int16", ()), "hand_levels": ("int8", (12,)),
    "phase": ("int8", ()), "action_mask": ("int8", (60,)), "hands_played": ("int32", ()),
    "best_hand_this_ante": ("int32", ()), "boss_blind_active": ("int8", ()), "boss_blind_type": ("int8", ()),
    "face_down_cards": ("int64", (8,)),
}
OBS_BYTES = 330
# packed record of bg_rollout_rows (include/balatro_mi355x.h BG_ROW_*): key -> byte offset; reward / action / terminated ride along
ROW_BYTES = 352
ROW_STRIDE_LINES = 384   # BG_RECORD_STRIDE_LINES: records as three whole 128-byte lines (the fast layout of bg_rollout_rows)
ROW_OFFSETS = {
    "selected_cards": 0, "face_down_cards": 64, "chips_scored": 128, "round_chips_scored": 144, "progress_ratio": 148,
    "mult": 152, "chips_needed": 156, "money": 160, "hands_played": 164, "best_hand_this_ante": 168, "action_mask": 176,
    "joker_ids": 236, "shop_items": 256, "shop_costs": 276, "consumables": 296, "ante": 306, "shop_rerolls": 308,
    "hand": 310, "hand_levels": 318, "hand_size": 330, "deck_size": 331, "round": 332, "hands_left": 333,
    "discards_left": 334, "joker_count": 335, "joker_slots": 336, "consumable_count": 337, "consumable_slots": 338,
    "phase": 339, "boss_blind_active": 340, "boss_blind_type": 341,
}
# (end_flags: byte BG_ROW_END_FLAGS, written by bg_step_many_rows_ex with limits -- its BG_END_* bits are below -- and 0 on every other path)
# (end_ante / end_round / end_chips: the ended episode's final state.ante, state.round and min(chips_scored, 2**32 - 1), in the records of ended steps
#  of bg_step_many_rows_ex with limits on a handle whose episode summary is on -- bg_set_episode_summary -- and 0 everywhere else)
ROW_EXTRA = {"reward": (136, "float64"), "action": (172, "int32"), "terminated": (342, "uint8"), "end_flags": (343, "uint8"),
             "end_ante": (344, "int16"), "end_round": (346, "int8"), "end_chips": (348, "uint32")}
ROW_END_FLAGS = ROW_EXTRA["end_flags"][0]
ROW_END_ANTE, ROW_END_ROUND, ROW_END_CHIPS = ROW_EXTRA["end_ante"][0], ROW_EXTRA["end_round"][0], ROW_EXTRA["end_chips"][0]
END_GAME, END_INVALID, END_MAX_STEPS = 1, 2, 4
END_STUCK = 8               # bg_step_many_rows_progress: ProgressionRewardWrapper's own ending (info['stuck_on_ante_1'])
PROGRESS_STUCK_STEPS = 300  # csrc/bg_progress.h: more steps than this on ante 1 end the episode
# bg_episode_ends_rows: the words of its report (csrc/bg_ends.h BG_ENDS_W_*; the histogram of end antes is words 16 + min(ante, 15))
ENDS_WORDS = 32
ENDS_REPORT = {"ended": 0, "game": 1, "invalid": 2, "max_steps": 3, "ante_sum": 4, "ante_max": 5, "chips_sum": 6, "chips_max": 7, "raised": 8,
               "no_summary": 9}
ENDS_HIST = 16
CURRICULUM_CAP_MAX = 255
SAFE_MIN_LIMIT = 3
INFO_KEYS = ["final_score", "error", "flags", "aux", "hand_type", "cards_played", "reward_terms", "score_breakdown"]
INFO_SPEC = {"final_score": ("int64", ()), "error": ("int32", ()), "flags": ("int32", ()), "aux": ("int32", ()),
             "hand_type": ("int8", ()), "cards_played": ("int8", ()), "reward_terms": ("float64", (8,)), "score_breakdown": ("float64", (8,))}

FLAG_SCORER_JOKERS = 1
FLAG_AUTORESET = 2
FLAG_CARD_STATES = 4
POLICY_UNIFORM, POLICY_SMALL_ONLY, POLICY_CYCLE3 = 0, 1, 2

EXPORTS = ["bg_create", "bg_destroy", "bg_last_error", "bg_num_envs", "bg_max_fused_steps", "bg_state_bytes", "bg_seed", "bg_reset",
           "bg_step", "bg_observe", "bg_rollout", "bg_rollout_rows", "bg_inject", "bg_inject_cards", "bg_inject_consumables", "bg_state_blob_bytes", "bg_get_state", "bg_set_state",
           "bg_refill", "bg_check", "bg_set_profiling", "bg_get_profile", "bg_set_max_ante", "bg_inject_deck",
           "bg_classify_batch", "bg_score_hand_batch", "bg_classify_batch_ex", "bg_score_hand_batch_ex", "bg_bench_copy", "bg_bench_fill", "bg_step_many",
           "bg_sim_evaluate_batch", "bg_sim_score_batch", "bg_create_ex", "bg_step_rows", "bg_observe_rows", "bg_step_many_rows",
           "bg_encode_cols", "bg_encode_rows", "bg_gae_rows", "bg_episode_stats_rows",
           "bg_gae_rows_ex", "bg_norm_workspace_bytes", "bg_norm_obs_rows", "bg_norm_reward_rows",
           "bg_sample_actions", "bg_evaluate_actions", "bg_ppo_loss", "bg_ppo_loss_workspace_bytes", "bg_encode_rows_ex",
           "bg_step_many_rows_ex", "bg_safe_terminal_slots",
           "bg_linear_rows", "bg_linear_rows_workspace_bytes", "bg_linear_rows_grad",
           "bg_extractor_rows", "bg_extractor_rows_workspace_bytes", "bg_extractor_rows_grad",
           "bg_get_states", "bg_set_states", "bg_copy_states",
           "bg_set_episode_summary", "bg_episode_ends_rows",
           "bg_step_many_rows_progress", "bg_progress_terminal_slots",
           "bg_dqn_loss", "bg_dqn_loss_workspace_bytes", "bg_sample_actions_eps",
           "bg_episode_outcome_rows", "bg_bc_loss", "bg_bc_loss_workspace_bytes",
           "bg_actor_sample", "bg_actor_evaluate", "bg_actor_ppo_loss", "bg_actor_ppo_loss_workspace_bytes", "bg_actor_ppo_loss_rows_per_group",
           "bg_optim_step", "bg_optim_workspace_size",
           "bg_demo_append_rows", "bg_demo_sample", "bg_demo_workspace_bytes",
           "bg_expert_actions", "bg_expert_actions_ex",
           "bg_policy_forward", "bg_policy_check", "bg_policy_tap_cols"]
# state-blob geometry (csrc/bg_device.h; tests/test_cabi_and_host.py checks these against the header): 16-byte chunks per env of the
# hot / deck / cold / template arrays, words per stored MT19937 block, words per shop-stream ring slot and where its seed sits
BLOB_NHOT, BLOB_NDECK, BLOB_NCOLD, BLOB_NTMPL, BLOB_NCST, BLOB_MTS, BLOB_SSEED = 8, 4, 7, 2, 7, 640, 128
SHOP_SLOT_WORDS, SHOP_SLOT_SEED_WORD = 64, 62
SCORE_CASE_WORDS, SCORE_OUT_WORDS = 40, 8
SIM_EVAL_BYTES, SIM_CASE_WORDS = 128, 64

# bg_encode_rows (include/balatro_mi355x.h BG_ENC_*; the column tables live in csrc/bg_encode.h, tests/test_encode_rows_host.py holds this copy to them)
ENC_PRODUCED, ENC_FIXED, ENC_EXTRACTOR = 0, 1, 2
ENC_F32, ENC_BF16 = 0, 1
ENC_LAYOUTS = {"produced": ENC_PRODUCED, "fixed": ENC_FIXED, "extractor": ENC_EXTRACTOR}
HEAD_F32, HEAD_BF16, HEAD_DETERMINISTIC = 0, 1, 1   # bg_sample_actions / bg_evaluate_actions (BG_HEAD_*)
# bg_ppo_loss: the order of stats_dev (BG_PPO_STATS floats) and its flag
PPO_STATS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "adv_mean", "adv_std", "excluded", "m")
PPO_NORMALIZE_ADV = 1
# bg_bc_loss: the order of stats_dev (BG_BC_STATS floats)
BC_STATS = ("loss", "nll_loss", "entropy_loss", "accuracy", "weight_sum", "excluded", "m")
# bg_dqn_loss: the order of stats_dev (BG_DQN_STATS floats) and its flags
DQN_STATS = ("loss", "q_mean", "target_mean", "abs_td_mean", "abs_td_max", "done_share", "excluded", "m")
DQN_MASK_NEXT, DQN_MSE, DQN_TIMEOUT_EXCLUDE = 1, 2, 4
LIN_NONE, LIN_RELU = 0, 1   # bg_linear_rows / bg_linear_rows_grad (BG_LIN_*)
LIN_ACTIVATIONS = {None: LIN_NONE, "relu": LIN_RELU}
LIN_K = 153                 # the columns of a first-layer weight that are read: the "produced" ones
ACTOR_HIN_MIN, ACTOR_HIN_MAX = 32, 1024   # bg_actor_*: the width of the last hidden activation, a multiple of 32
EXT_K = 447                 # bg_extractor_rows: the columns of the "extractor" layout (416 one-hot, 10 joker ids, 21 state features)
EXT_SPLITS = (416, 10, 21)  # the inputs of the reference's hand_net / joker_net / game_state_net first layers, in column order
# bg_optim_step (BG_OPTIM_*; csrc/bg_optim.h): algorithms, flags, the table's geometry and the fields of the 32-byte stats block
OPTIM_ADAM, OPTIM_RMSPROP_TF = 0, 1
OPTIM_ALGORITHMS = {"adam": OPTIM_ADAM, "rmsprop_tf": OPTIM_RMSPROP_TF}
OPTIM_ZERO_GRAD, OPTIM_SHADOW_ONLY = 1, 2
OPTIM_MAX_TENSORS, OPTIM_CHUNK, OPTIM_ENTRY_BYTES, OPTIM_STATS_BYTES, OPTIM_CARRY_BYTES = 1024, 1024, 64, 32, 32
OPTIM_STATS = ("grad_norm", "clip_coef", "skipped", "nonfinite", "step")
# bg_policy_forward (BG_POLICY_*; csrc/bg_policy.h): the envelope, the activations, the flag beside HEAD_DETERMINISTIC and the host table's geometry
POLICY_WIDTH_MIN, POLICY_WIDTH_MAX, POLICY_MAX_SECTION, POLICY_MAX_LAYERS = 32, 512, 4, 14
POLICY_ACTIVATIONS = {None: 0, "relu": 1, "tanh": 2}
POLICY_EVALUATE = 2
POLICY_NET_BYTES, POLICY_LAYER_BYTES = 480, 32
NORM_COLS = 153   # BG_NORM_COLS: VecNormalize's statistics are one (mean, var) per column of the "produced" layout
# the keys BalatroEnvFixed zero-fills (train_balatro_fixed.py:125-207), in the order of its observation space, with their element counts
ENC_ZERO_KEYS = [("hand_one_hot", 416), ("hand_suits", 8), ("hand_ranks", 8), ("rank_counts", 13), ("suit_counts", 4), ("straight_potential", 1),
                 ("flush_potential", 1), ("avg_score_per_hand", 1), ("hands_until_shop", 1), ("rounds_until_boss", 1), ("has_mult_jokers", 1),
                 ("has_chip_jokers", 1), ("has_xmult_jokers", 1), ("has_economy_jokers", 1), ("hand_potential_scores", 12), ("joker_synergy_score", 1),
                 ("risk_level", 1), ("economy_health", 1), ("blind_difficulty", 1), ("win_probability", 1)]
# BalatroFeaturesExtractor.forward (train_balatro_agent.py:84-119): (name, source key, elements, divisor or None)
ENC_EXTRACTOR_PARTS = [("hand_one_hot", "hand", 416, None), ("joker_ids", "joker_ids", 10, None), ("chips_scored", "chips_scored", 1, 1e6),
                       ("chips_needed", "chips_needed", 1, 1e5), ("progress_ratio", "progress_ratio", 1, None), ("money", "money", 1, 100.0),
                       ("ante", "ante", 1, 10.0), ("round", "round", 1, 3.0), ("hands_left", "hands_left", 1, 10.0),
                       ("discards_left", "discards_left", 1, 5.0), ("hand_levels", "hand_levels", 12, 10.0), ("phase", "phase", 1, 3.0)]


def _enc_columns():
    def run(parts):
        out, c = [], 0
        for name, n in parts:
            out.append((name, c, n))
            c += n
        return out
    produced = [(k, 1 if OBS_SPEC[k][1] == () else OBS_SPEC[k][1][0]) for k in OBS_KEYS]
    return {ENC_PRODUCED: run(produced), ENC_FIXED: run(produced + ENC_ZERO_KEYS), ENC_EXTRACTOR: run([(p[0], p[2]) for p in ENC_EXTRACTOR_PARTS])}


# layout -> [(name, first column, columns)]: e.g. the 60 action_mask columns of a PRODUCED / FIXED matrix
ENC_COLUMNS = _enc_columns()
ENC_COLS = {layout: cols[-1][1] + cols[-1][2] for layout, cols in ENC_COLUMNS.items()}   # what bg_encode_cols returns


class ObsPtrs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in OBS_KEYS]


class InfoPtrs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in INFO_KEYS]


class RolloutStats(C.Structure):
    _fields_ = [("steps", C.c_uint64), ("episodes", C.c_uint64), ("plays", C.c_uint64), ("score_sum", C.c_int64),
                ("reward_bits", C.c_uint64), ("obs_hash", C.c_uint64)]


class ProgressRewards(C.Structure):
    """bg_progress_rewards (include/balatro_mi355x.h)."""
    _fields_ = [("counters_dev", C.c_void_p)]


class SafeLimits(C.Structure):
    """bg_safe_limits (include/balatro_mi355x.h)."""
    _fields_ = [("max_invalid_actions", C.c_int32), ("max_episode_steps", C.c_int32), ("counters_dev", C.c_void_p),
                ("terminal_rows_dev", C.c_void_p), ("terminal_stride_bytes", C.c_uint64), ("terminal_step_dev", C.c_void_p),
                ("terminal_slots", C.c_int32)]


class Curriculum(C.Structure):
    """bg_curriculum (include/balatro_mi355x.h)."""
    _fields_ = [("cap_dev", C.c_void_p), ("hist_dev", C.c_void_p), ("count_dev", C.c_void_p), ("at_level_dev", C.c_void_p),
                ("raised_dev", C.c_void_p), ("window", C.c_int32), ("increment", C.c_int32), ("threshold", C.c_double)]


class NativeError(RuntimeError):
    pass


_lib = None


def lib_path() -> str:
    # BALATRO_MI355X_LIB points at an installed / experimental build of the same C ABI (still the HIP library: there is
    # no other implementation to fall back to)
    return os.environ.get("BALATRO_MI355X_LIB") or _build.LIB


def device_code_signature(path: str | None = None) -> str:
    """Identifies the DEVICE code that runs, reproducibly: the signature the library was built with (`bg_build_signature`: sha256
    prefix over sources + flags + compiler, `build.source_signature()`), which any rebuild of unchanged sources repeats -- the bytes
    of the code object do not (three rebuilds of unchanged sources gave three .hip_fatbin hashes).  bench.py only quotes a committed
    PMC traffic measurement (profiles/*_hbm_traffic.json) taken on exactly this signature.  Ad-hoc builds ("unsigned", e.g.
    tools/build_variant.sh) fall back to the sha256 of their .hip_fatbin section."""
    path = path or lib_path()
    try:
        L = C.CDLL(path) if (_lib is None or path != lib_path()) else _lib
        L.bg_build_signature.restype = C.c_char_p
        sig = L.bg_build_signature().decode()
        if sig and sig != "unsigned":
            return sig
    except (OSError, AttributeError):
        pass
    return fatbin_sha(path)


def fatbin_sha(path: str) -> str:
    import hashlib
    import struct
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"\x7fELF" or data[4] != 2:
        return "not-elf64"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    def sh(i):
        name, _type, _flags, _addr, off, size = struct.unpack_from("<IIQQQQ", data, shoff + i * shentsize)
        return name, off, size
    _, stroff, strsize = sh(shstrndx)
    for i in range(shnum):
        name, off, size = sh(i)
        end = data.index(b"\0", stroff + name)
        if data[stroff + name:end] == b".hip_fatbin":
            return hashlib.sha256(data[off:off + size]).hexdigest()[:16]
    return "no-fatbin"


def load(build_if_missing: bool = True):
    """Load the HIP library; raises NativeError (never falls back) when it is unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if build_if_missing and path == _build.LIB and _build.needs_build():
        try:
            _build.build()
        except Exception as exc:  # no hipcc on the box and no prebuilt .so
            if not os.path.exists(path):
                raise NativeError(f"libbalatro_mi355x.so is missing and could not be built: {exc}") from exc
    if not os.path.exists(path):
        raise NativeError(f"{path} not found: build it with `python -m balatro_gym_amd.build` (no CPU fallback exists)")
    # PyTorch-ROCm ships its own libamdhip64 (torch/lib); the process must hold ONE HIP runtime, and device tensors come
    # from torch, so torch's copy has to be the one that is resident when this library's libamdhip64.so.7 dependency is
    # resolved.  (Loading this library first brought in /opt/rocm's runtime as well: bg_create then saw no device.)
    import torch  # noqa: F401
    try:
        L = C.CDLL(path)
    except OSError as exc:
        raise NativeError(f"cannot load {path}: {exc}") from exc
    for name in EXPORTS:
        if not hasattr(L, name):
            raise NativeError(f"{path} does not export {name}")
    vp, i32, u32, u64, i64 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_int64
    L.bg_create.argtypes = [i32, i32, u32, i32, C.POINTER(vp)]
    L.bg_create_ex.argtypes = [i32, i32, u32, i32, i32, C.POINTER(vp)]
    L.bg_destroy.argtypes = [vp]
    L.bg_last_error.restype = C.c_char_p
    L.bg_last_error.argtypes = [vp]
    L.bg_num_envs.argtypes = [vp]
    L.bg_max_fused_steps.argtypes = [vp]
    L.bg_state_bytes.restype = u64
    L.bg_state_bytes.argtypes = [vp]
    L.bg_seed.argtypes = [vp, vp, vp, i32, vp]
    L.bg_reset.argtypes = [vp, vp, C.POINTER(ObsPtrs), vp]
    L.bg_step.argtypes = [vp, vp, C.POINTER(ObsPtrs), vp, vp, vp, C.POINTER(InfoPtrs), vp]
    L.bg_observe.argtypes = [vp, C.POINTER(ObsPtrs), vp]
    L.bg_step_rows.argtypes = [vp, vp, vp, u64, vp, vp, vp, C.POINTER(InfoPtrs), vp]
    L.bg_observe_rows.argtypes = [vp, vp, u64, vp]
    L.bg_step_many.argtypes = [vp, i32, vp, C.POINTER(ObsPtrs), i32, vp, vp, vp, C.POINTER(InfoPtrs), vp]
    L.bg_rollout.argtypes = [vp, i32, i32, u64, u64, u64, C.POINTER(ObsPtrs), i32, vp, vp, vp, vp, vp]
    L.bg_rollout_rows.argtypes = [vp, i32, i32, u64, u64, u64, vp, u64, i32, vp, vp]
    L.bg_step_many_rows.argtypes = [vp, i32, vp, vp, u64, i32, vp, vp]
    L.bg_step_many_rows_ex.argtypes = [vp, i32, vp, vp, u64, i32, C.POINTER(SafeLimits), vp, vp]
    L.bg_safe_terminal_slots.argtypes = [i32, i32, i32]
    L.bg_step_many_rows_progress.argtypes = [vp, i32, vp, vp, u64, i32, C.POINTER(SafeLimits), C.POINTER(ProgressRewards), vp, vp]
    L.bg_progress_terminal_slots.argtypes = [i32, i32, i32]
    L.bg_set_episode_summary.argtypes = [vp, i32]
    L.bg_episode_ends_rows.argtypes = [vp, u64, i32, i64, vp, C.POINTER(Curriculum), C.POINTER(C.c_float), vp]
    L.bg_set_gather_peers.argtypes = [vp, vp, i32, i32]
    L.bg_inject.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp]
    L.bg_inject_cards.argtypes = [vp, vp, vp, vp, vp, i32, vp]
    L.bg_inject_consumables.argtypes = [vp, vp, vp, vp, i32, vp]
    L.bg_state_blob_bytes.restype = u64
    L.bg_state_blob_bytes.argtypes = [vp]
    L.bg_get_state.argtypes = [vp, i32, vp, u64]
    L.bg_set_state.argtypes = [vp, i32, vp, u64]
    L.bg_get_states.argtypes = [vp, vp, i32, vp, u64, vp]
    L.bg_set_states.argtypes = [vp, vp, i32, vp, u64, i32, vp, vp]
    L.bg_copy_states.argtypes = [vp, vp, vp, vp, i32, vp]
    L.bg_refill.argtypes = [vp, vp]
    L.bg_check.argtypes = [vp, vp]
    L.bg_set_profiling.argtypes = [vp, i32]
    L.bg_get_profile.argtypes = [vp, C.POINTER(C.c_double)]
    L.bg_set_max_ante.argtypes = [vp, i32, vp, vp, vp]
    L.bg_inject_deck.argtypes = [vp, vp, vp, vp]
    L.bg_classify_batch.argtypes = [vp, vp, vp, i64, vp]
    L.bg_score_hand_batch.argtypes = [vp, vp, i32, vp]
    L.bg_classify_batch_ex.argtypes = [vp, vp, vp, i64, i32, vp, vp]
    L.bg_score_hand_batch_ex.argtypes = [vp, vp, i32, i32, vp, vp]
    L.bg_sim_evaluate_batch.argtypes = [vp, vp, vp, vp, i32, vp]
    L.bg_sim_score_batch.argtypes = [vp, vp, i32, vp]
    L.bg_bench_copy.argtypes = [vp, vp, u64, i32, C.POINTER(C.c_double), vp]
    L.bg_bench_fill.argtypes = [vp, u64, i32, C.POINTER(C.c_double), vp]
    L.bg_encode_cols.argtypes = [i32]
    L.bg_encode_rows.argtypes = [vp, u64, i64, i32, i32, vp, u64, C.POINTER(C.c_float), vp]
    L.bg_encode_rows_ex.argtypes = [vp, u64, i64, vp, i64, i32, i32, vp, vp, C.c_double, C.c_double, vp, u64, C.POINTER(C.c_float), vp]
    L.bg_gae_rows.argtypes = [vp, u64, i32, i64, vp, vp, C.c_double, C.c_double, vp, vp, C.POINTER(C.c_float), vp]
    L.bg_episode_stats_rows.argtypes = [vp, u64, i32, i64, vp, vp, vp, vp, C.POINTER(C.c_float), vp]
    L.bg_gae_rows_ex.argtypes = [vp, u64, i32, i64, vp, vp, C.c_double, C.c_double, vp, vp, vp, C.POINTER(C.c_float), vp]
    L.bg_norm_workspace_bytes.restype = u64
    L.bg_norm_workspace_bytes.argtypes = [i32, i64]
    L.bg_norm_obs_rows.argtypes = [vp, u64, i32, i64, i32, i32, vp, vp, vp, i32, C.c_double, C.c_double, vp, u64, vp, vp, u64, C.POINTER(C.c_float), vp]
    L.bg_norm_reward_rows.argtypes = [vp, u64, i32, i64, vp, vp, i32, C.c_double, C.c_double, C.c_double, vp, vp, vp, u64, C.POINTER(C.c_float), vp]
    L.bg_sample_actions.argtypes = [vp, i32, u64, vp, u64, i64, u32, u64, u64, u64, vp, vp, vp, C.POINTER(C.c_float), vp]
    L.bg_evaluate_actions.argtypes = [vp, i32, u64, vp, u64, i64, vp, vp, vp, C.POINTER(C.c_float), vp]
    L.bg_ppo_loss_workspace_bytes.restype = u64
    L.bg_ppo_loss_workspace_bytes.argtypes = [i64]
    L.bg_ppo_loss.argtypes = [vp, i32, u64, vp, u64, vp, vp, vp, vp, vp, vp, i64, i64, C.c_float, C.c_float, C.c_float, u32, vp, u64, vp, vp, vp, vp, vp, u64,
                              C.POINTER(C.c_float), vp]
    L.bg_episode_outcome_rows.argtypes = [vp, u64, i32, i64, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float), vp]
    L.bg_bc_loss_workspace_bytes.restype = u64
    L.bg_bc_loss_workspace_bytes.argtypes = [i64]
    L.bg_bc_loss.argtypes = [vp, i32, u64, vp, u64, vp, u64, vp, vp, i64, i64, C.c_float, vp, u64, vp, vp, vp, vp, u64, C.POINTER(C.c_float), vp]
    L.bg_dqn_loss_workspace_bytes.restype = u64
    L.bg_dqn_loss_workspace_bytes.argtypes = [i64]
    L.bg_dqn_loss.argtypes = [vp, u64, vp, u64, vp, u64, i32, vp, u64, i64, vp, vp, i64, C.c_float, u32, vp, u64, vp, vp, vp, u64, C.POINTER(C.c_float), vp]
    L.bg_sample_actions_eps.argtypes = [vp, i32, u64, vp, u64, i64, u32, u64, u64, u64, C.c_float, vp, vp, vp, C.POINTER(C.c_float), vp]
    L.bg_linear_rows.argtypes = [vp, u64, i64, vp, i64, i32, vp, vp, C.c_double, C.c_double, vp, u64, vp, i32, i32, i32, vp, u64, C.POINTER(C.c_float), vp]
    L.bg_linear_rows_workspace_bytes.restype = u64
    L.bg_linear_rows_workspace_bytes.argtypes = [i64, i32]
    L.bg_linear_rows_grad.argtypes = [vp, u64, i64, vp, i64, i32, vp, vp, C.c_double, C.c_double, vp, i32, u64, vp, i32, u64, i32, i32, vp, u64, vp, vp, u64,
                                      C.POINTER(C.c_float), vp]
    L.bg_extractor_rows.argtypes = [vp, u64, i64, vp, i64, vp, u64, vp, i32, i32, i32, vp, u64, C.POINTER(C.c_float), vp]
    L.bg_extractor_rows_workspace_bytes.restype = u64
    L.bg_extractor_rows_workspace_bytes.argtypes = [i64, i32]
    L.bg_extractor_rows_grad.argtypes = [vp, u64, i64, vp, i64, vp, i32, u64, vp, i32, u64, i32, i32, vp, u64, vp, vp, u64, C.POINTER(C.c_float), vp]
    head = [vp, u64, i32, vp, i32, u64, vp, vp, u64]   # h, its pitch, Hin, weight, its dtype, its pitch, bias, mask, its pitch
    L.bg_actor_sample.argtypes = head + [i64, u32, u64, u64, u64, vp, vp, vp, vp, u64, C.POINTER(C.c_float), vp]
    L.bg_actor_evaluate.argtypes = head + [i64, vp, vp, vp, vp, u64, C.POINTER(C.c_float), vp]
    L.bg_actor_ppo_loss_workspace_bytes.restype = u64
    L.bg_actor_ppo_loss_workspace_bytes.argtypes = [i64, i32]
    L.bg_actor_ppo_loss_rows_per_group.restype = i64
    L.bg_actor_ppo_loss_rows_per_group.argtypes = [i64, i32]
    L.bg_actor_ppo_loss.argtypes = head + [vp, vp, vp, vp, vp, vp, i64, i64, C.c_float, C.c_float, C.c_float, u32, vp, i32, u64, vp, vp, vp, vp, vp, vp, vp, u64,
                                           vp, u64, vp, u64, C.POINTER(C.c_float), vp]
    L.bg_optim_workspace_size.restype = u64
    L.bg_optim_workspace_size.argtypes = [i64]
    L.bg_optim_step.argtypes = [vp, i32, i64, i32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, u32, vp, vp, vp, C.POINTER(C.c_float), vp]
    L.bg_demo_workspace_bytes.restype = u64
    L.bg_demo_workspace_bytes.argtypes = [i64]
    L.bg_demo_append_rows.argtypes = [vp, u64, i32, i64, vp, vp, vp, u64, i64, vp, vp, vp, vp, u64, C.POINTER(C.c_float), vp]
    L.bg_demo_sample.argtypes = [vp, i64, u64, u64, u64, vp, i64, C.POINTER(C.c_float), vp]
    L.bg_expert_actions.argtypes = [vp, i64, i64, vp, i64, vp, vp, vp]
    L.bg_expert_actions_ex.argtypes = [vp, i64, i64, vp, i64, vp, vp, i32, C.POINTER(C.c_float), vp]
    L.bg_policy_check.argtypes = [vp]
    L.bg_policy_tap_cols.argtypes = [vp]
    L.bg_policy_forward.argtypes = [vp, vp, u64, vp, u64, i64, u32, u64, u64, u64, vp, vp, vp, vp, vp, u64, vp, u64, C.POINTER(C.c_float), vp]
    _lib = L
    return L
