"""Shared by tests/test_extractor_rows_host.py, tests/test_extractor_rows.py and tests/test_extractor_large_store.py: the float64 statement of
bg_extractor_rows / bg_extractor_rows_grad and its bound.

The layer's input x is not restated here: it is the bfloat16 row of bg_encode_rows_ex for the "extractor" layout, which tests/encode_ref.py
(`expected_bits`, `bf16_bits`) gives as bit patterns and the encode tests hold to the kernel bit for bit.  Everything else is float64 numpy over the
widened bfloat16 operands, with tests/linear_ref.py's `widen`, `to_bf16_bits` and `check_close`.

The bound is linear_ref.py's, with its derivation: |got - ref| <= 2 (L + 2) 2**-24 (sum |x w| + |b|) + one rounding of the result, L = 448 forward (the
padded reduction); for the gradient L = the rows one workgroup accumulates in float32 (`grad_rows_per_group`).  A bfloat16 output is held exactly: the
round-to-nearest-even of the float32 output of the same call."""
import numpy as np

from tests import encode_ref as ref
from tests.linear_ref import U, check_close, dp_values, to_bf16_bits, widen  # noqa: F401

K = 447
KPAD = 448
ROWS = 128        # rows of one block of the gradient
PART_ROWS = 449   # rows of a partial: 448 of dweight^T and one of dbias
KSPANS = 3        # spans of k over the gradient's grid
MAX_WG = 256      # bound on row groups x unit spans x k spans


def x_bits(bits32, index=None):
    """float32 bit patterns [store, 447] of the encoded rows -> the layer's input, bfloat16 bits [m, 447]: the rows at `index`, +0.0 where it is out of
    range."""
    xb = ref.bf16_bits(np.asarray(bits32)[:, :K])
    if index is None:
        return xb
    index = np.asarray(index, np.int64)
    ok = (index >= 0) & (index < len(xb))
    out = np.zeros((len(index), K), np.uint16)
    out[ok] = xb[index[ok]]
    return out


def forward(xb, wb, bias=None, relu=False):
    """-> (ref float64 [m, H], bound float64 [m, H] for a float32 output).  xb uint16 [m, 447]; wb uint16 [H, >= 447]; bias float32 [H] or None."""
    x, w = widen(xb), widen(np.asarray(wb)[:, :K])
    b = np.zeros(len(w)) if bias is None else np.asarray(bias, np.float64)
    s = x @ w.T + b
    mag = np.abs(x) @ np.abs(w).T + np.abs(b)
    out = np.where(s > 0, s, 0.0) if relu else s
    return out, 2 * (KPAD + 2) * U * mag + U * np.abs(out)


def grad(xb, dp, rows_per_group):
    """-> (dweight float64 [H, 447], its bound, dbias float64 [H], its bound)."""
    x = widen(xb)
    dw, dwm = dp.T @ x, np.abs(dp).T @ np.abs(x)
    db, dbm = dp.sum(0), np.abs(dp).sum(0)
    f = 2 * (rows_per_group + 2) * U
    return dw, f * dwm + U * np.abs(dw), db, f * dbm + U * np.abs(db)


def spans(H):
    return -(-H // 256)


def blocks_per_group(m, H):
    cap = max(1, MAX_WG // (KSPANS * spans(H)))
    return -(-(-(-m // ROWS)) // cap)


def groups(m, H):
    """The number of partials bg_extractor_rows_grad writes (include/balatro_mi355x.h): at most 256 / (3 ceil(H / 256)) groups of consecutive 128-row
    blocks."""
    return -(-(-(-m // ROWS)) // blocks_per_group(m, H))


def workspace_bytes(m, H):
    return groups(m, H) * PART_ROWS * H * 4


def grad_rows_per_group(m, H):
    return ROWS * blocks_per_group(m, H)


def smallest_m_with_two_blocks_per_group(H):
    """The smallest m at which a row group holds more than one 128-row block."""
    cap = max(1, MAX_WG // (KSPANS * spans(H)))
    return cap * ROWS + 1


# what the extractor layout divides by, per key (train_balatro_agent.py:102-113)
_DIVISORS = {"chips_scored": 10 ** 6, "chips_needed": 10 ** 5, "money": 100, "ante": 10, "round": 3, "hands_left": 10, "discards_left": 5, "hand_levels": 10,
             "phase": 3}


def int_quotient_obs(m, seed):
    """key -> [m, ...] records that encode, in the "extractor" layout, to multiples of 1/8 not above 12 that are exact in bfloat16: every integer field is
    in 0..12, each divided field multiplied by its divisor, progress_ratio a multiple of 1/8 below 2; `hand` is uniform in -1..51, row 0 all -1 and row 1
    [51, 51, 0, 0, 52, 127, -128, -1] (columns 51, 103, 104 and 156 and no others).  With integer weights of magnitude <= 4, an integer bias and integer
    dout in -4..4 every float32 sum is exact in any order."""
    from balatro_gym_amd import _native as nat
    rng = np.random.default_rng(seed)
    obs = {}
    for k in nat.OBS_KEYS:
        dt, shape = nat.OBS_SPEC[k]
        v = rng.integers(0, 13, (m,) + shape)
        if dt == "float32":
            obs[k] = (rng.integers(0, 16, (m,) + shape) / 8.0).astype(np.float32)
        else:
            obs[k] = (v * _DIVISORS.get(k, 1)).astype(dt)
            assert (obs[k].astype(np.int64) == v * _DIVISORS.get(k, 1)).all(), k
    hand = rng.integers(-1, 52, (m, 8)).astype(np.int8)
    hand[0] = -1
    if m > 1:
        hand[1] = np.array([51, 51, 0, 0, 52, 127, -128, -1], np.int8)
    obs["hand"] = hand
    return obs


def assert_exact_inputs(xb, wb, bias=None):
    """The condition under which every float32 sum is exact in any order: x * 8 is an integer, and sum |x| |w| + |b| < 2**21."""
    x = widen(xb)
    assert (x * 8 == np.round(x * 8)).all() and np.abs(x).max() <= 12
    mag = np.abs(x) @ np.abs(widen(np.asarray(wb)[:, :K])).T + (0 if bias is None else np.abs(np.asarray(bias, np.float64)))
    assert mag.max() < 2 ** 21
