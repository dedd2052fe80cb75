"""Shared by tests/test_encode_rows_host.py and tests/test_encode_rows.py: the numpy restatement of bg_encode_rows' three layouts (written from the
reference's definitions, not from csrc/bg_encode.h), record packing through RowBuffers views on the CPU, and the synthetic records.

PRODUCED / FIXED: SB3's CombinedExtractor over BalatroEnvFixed (train_balatro_fixed.py:125-207): every key `.float()`ed, flattened and concatenated
in the observation space's key order, the 20 never-filled keys as zeros.  EXTRACTOR: BalatroFeaturesExtractor.forward (train_balatro_agent.py:84-119).
Everything is compared as bit patterns (uint32 / uint16 views): no tolerance anywhere.

bfloat16: round to nearest even of the float32 bit pattern.  For a NaN "nearest even" says nothing and torch itself is of two minds (its scalar
conversion gives 0x7fc0, its AVX path 0xffff), so the library's rule is stated here: a NaN becomes the canonical quiet NaN 0x7fc0.  `bf16_bits` is held to
torch on every non-NaN input by `check_bf16_against_torch`."""
import os

import numpy as np

from tests.helpers import GOLD, OBS_KEYS

ZERO_KEYS = [("hand_one_hot", 416), ("hand_suits", 8), ("hand_ranks", 8), ("rank_counts", 13), ("suit_counts", 4), ("straight_potential", 1),
             ("flush_potential", 1), ("avg_score_per_hand", 1), ("hands_until_shop", 1), ("rounds_until_boss", 1), ("has_mult_jokers", 1),
             ("has_chip_jokers", 1), ("has_xmult_jokers", 1), ("has_economy_jokers", 1), ("hand_potential_scores", 12), ("joker_synergy_score", 1),
             ("risk_level", 1), ("economy_health", 1), ("blind_difficulty", 1), ("win_probability", 1)]
LAYOUTS = ("produced", "fixed", "extractor")
COLS = {"produced": 153, "fixed": 628, "extractor": 447}


def _f32_bits(a, m):
    """numpy.float32(value) of every element as uint32 [m, -1]; a float32 array is taken bit for bit."""
    a = np.asarray(a)
    f = a if a.dtype == np.float32 else a.astype(np.float32)
    return np.ascontiguousarray(f).view(np.uint32).reshape(m, -1)


def expected_bits(layout, obs):
    """obs: key -> [m, ...] array in the record's dtypes.  Returns the float32 bit patterns, uint32 [m, D]."""
    m = len(obs["hand"])
    if layout in ("produced", "fixed"):
        parts = [_f32_bits(obs[k], m) for k in OBS_KEYS]
        if layout == "fixed":
            parts.append(np.zeros((m, sum(n for _, n in ZERO_KEYS)), np.uint32))
        return np.concatenate(parts, axis=1)
    assert layout == "extractor"
    hand = np.asarray(obs["hand"]).astype(np.int64)
    one_hot = np.zeros((m, 8, 52), np.float32)
    for i in range(8):   # train_balatro_agent.py:89-93
        valid = (hand[:, i] >= 0) & (hand[:, i] < 52)   # (the reference indexes with every valid card; cards are 0..51)
        one_hot[np.flatnonzero(valid), i, hand[valid, i]] = 1
    def div(k, c):
        with np.errstate(all="ignore"):
            return _f32_bits(np.asarray(obs[k]).astype(np.float32) / np.float32(c), m)
    return np.concatenate([
        _f32_bits(one_hot, m), _f32_bits(obs["joker_ids"], m),
        div("chips_scored", 1e6), div("chips_needed", 1e5), _f32_bits(obs["progress_ratio"], m), div("money", 100), div("ante", 10), div("round", 3),
        div("hands_left", 10), div("discards_left", 5), div("hand_levels", 10), div("phase", 3)], axis=1)


def bf16_bits(bits32):
    """float32 bit patterns -> bfloat16 bit patterns: round to nearest even; NaN -> 0x7fc0 (module docstring)."""
    u = np.asarray(bits32, np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7fffffff) > 0x7f800000
    return np.where(nan, np.uint16(0x7fc0), r)


def check_bf16_against_torch(bits32):
    import torch
    bits32 = np.ascontiguousarray(bits32, np.uint32)
    nan = (bits32 & 0x7fffffff) > 0x7f800000
    t = torch.from_numpy(bits32.view(np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(t[~nan], bf16_bits(bits32)[~nan])


def pack_records(obs, stride):
    """obs: key -> [m, ...] arrays -> uint8 [m, stride] records, written through the typed views of a CPU RowBuffers (bytes no key covers stay 0)."""
    import torch
    from balatro_gym_amd.vec_env import RowBuffers
    m = len(obs["hand"])
    rb = RowBuffers(m, torch.device("cpu"), steps=1, row_stride=stride)
    for k in OBS_KEYS:
        rb.tensors[k][0].copy_(torch.from_numpy(np.ascontiguousarray(obs[k]).reshape(rb.tensors[k][0].shape)))
    return rb.rows[0].numpy()


def unpack_records(rows):
    """uint8 [m, stride] records -> key -> [m, ...] arrays in the record's dtypes (copies), through the same RowBuffers views."""
    import torch
    from balatro_gym_amd.vec_env import RowBuffers
    rows = np.ascontiguousarray(rows)
    m, stride = rows.shape
    rb = RowBuffers(m, torch.device("cpu"), steps=1, row_stride=stride)
    rb.rows[0].copy_(torch.from_numpy(rows))
    return {k: rb.tensors[k][0].contiguous().numpy().copy() for k in OBS_KEYS}


def trace_obs(name):
    """Every 31-key observation of a golden trace (the first of each seed and all stepped ones), key -> [m, ...]."""
    from tests.helpers import load_trace
    tr = load_trace(name)
    out = {}
    for k in OBS_KEYS:
        a0, a = tr["obs0_" + k], tr["obs_" + k]
        out[k] = np.concatenate([a0.reshape((a0.shape[0], 1) + a0.shape[1:]), a], axis=1).reshape((-1,) + a.shape[2:])
    return out


def sb3_fixture():
    with np.load(os.path.join(GOLD, "sb3_fixed.npz")) as z:
        return {k: z[k] for k in z.files}


def sb3_fixed_bits(g, prefix, lead):
    """The fixture's 51 keys `.astype(float32)`, flattened and concatenated in `keys` order: uint32 [prod(lead), 628]."""
    m = int(np.prod(lead))
    return np.concatenate([_f32_bits(g[prefix + str(k)].astype(np.float32), m) for k in g["keys"]], axis=1)


_INFO = {"int8": np.iinfo(np.int8), "int16": np.iinfo(np.int16), "int32": np.iinfo(np.int32), "int64": np.iinfo(np.int64)}


def synthetic_obs(n_random=10000, seed=20240607):
    """Records that no game produces: every field of a record at its dtype's minimum / maximum / 0 / -1 (progress_ratio: -FLT_MAX, FLT_MAX, 0, -1, and
    rows of inf, -inf, NaN with a payload, the smallest subnormal, -0.0); chips_scored around the float32 and float64 integer limits; and `n_random`
    records of seeded random bytes in every observation field, `hand` drawn from -1..51 (the one-hot is defined for the values the env writes)."""
    from balatro_gym_amd import _native as nat
    rng = np.random.default_rng(seed)
    chips = [2 ** 24 + 1, -(2 ** 24 + 1), 2 ** 24 + 3, 2 ** 31, 2 ** 53 + 1, -(2 ** 53 + 1), np.iinfo(np.int64).min, np.iinfo(np.int64).max,
             2 ** 62 + 2 ** 38, 2 ** 62 + 2 ** 38 + 1, 999999, 1000000, 3]
    floats = np.array([0xff7fffff, 0x7f7fffff, 0, 0xbf800000, 0x7f800000, 0xff800000, 0x7fa12345, 0xffc00001, 1, 0x80000000, 0x3f7fffff, 0x00ffffff],
                      np.uint32).view(np.float32)
    m = 4 + max(len(chips), len(floats)) + n_random
    obs = {}
    for k in OBS_KEYS:
        dt, shape = nat.OBS_SPEC[k]
        a = np.zeros((m,) + shape, np.dtype(dt))
        if dt == "float32":
            a[:4] = np.array([-np.finfo(np.float32).max, np.finfo(np.float32).max, 0, -1], np.float32)
            a[4:4 + len(floats)] = floats
            a[m - n_random:] = rng.integers(0, 2 ** 32, n_random, dtype=np.uint32).view(np.float32)
        else:
            ii = _INFO[dt]
            for r, v in enumerate((ii.min, ii.max, 0, -1)):
                a[r] = v
            if k == "hand":
                a[m - n_random:] = rng.integers(-1, 52, (n_random,) + shape)
            else:
                a[m - n_random:] = rng.integers(ii.min, ii.max, (n_random,) + shape, dtype=np.dtype(dt), endpoint=True)
        obs[k] = a
    obs["chips_scored"][4:4 + len(chips)] = np.array(chips, np.int64)
    return obs
