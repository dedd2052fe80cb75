"""Shared by tests/test_linear_rows_host.py and tests/test_linear_rows.py: the float64 statement of bg_linear_rows / bg_linear_rows_grad and its bound.

The layer's input x is not restated here: it is the first 153 columns of the bfloat16 row of bg_encode_rows_ex, which tests/encode_ref.py
(`expected_bits`, `bf16_bits`) and tests/norm_ref.py (`obs_bits`) give as bit patterns and the encode tests hold to the kernel bit for bit.  Everything
else is float64 numpy over the WIDENED bfloat16 operands (a bfloat16 is a float32 whose low 16 bits are zero, so widening is exact).

The bound, for finite inputs.  Every bfloat16 x bfloat16 product has at most 16 significant bits: it is exact in float32, so only the accumulation
rounds.  A float32 sum of L terms in any order is within (L - 1) u S of the exact sum (u = 2**-24, S = the sum of the magnitudes, first order); the bias
add and the slack of the first-order statement make it (L + 2); the factor 2 is there because the matrix unit's internal rounding is not documented as
round-to-nearest (a truncating adder has twice the unit roundoff):
    |got - ref| <= 2 (L + 2) 2**-24 (sum |x w| + |b|)   + one rounding of the result to the output dtype (2**-24 relative for float32)
L = 160 forward (the padded reduction); for the gradient L = the rows one workgroup accumulates in float32 (`grad_rows_per_group`); the float64 sum
of the workgroups' partials adds 2**-53 terms that vanish beside it.  A bfloat16 output is not bounded but held exactly: it must be the
round-to-nearest-even of the float32 output of the same call (one rounding, behind the same float32 value)."""
import numpy as np

from tests import encode_ref as ref

K = 153
KPAD = 160
U = 2.0 ** -24
ROWS = 128        # BG_LIN_ROWS: rows of one block of the gradient
PART_ROWS = 161   # rows of a partial: 160 of dweight^T and one of dbias


def widen(bits16):
    """bfloat16 bit patterns -> their exact values as float64."""
    return (np.asarray(bits16, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def to_bf16_bits(f32):
    """float32 values -> bfloat16 bit patterns, round to nearest even (tests/encode_ref.py's rule)."""
    return ref.bf16_bits(np.ascontiguousarray(f32, np.float32).view(np.uint32))


def x_bits(bits32, index=None):
    """float32 bit patterns [store, >= 153] of the encoded rows -> the layer's input, bfloat16 bits [m, 153]: the rows at `index`, +0.0 where it is out of
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
    """-> (ref float64 [m, H], bound float64 [m, H] for a float32 output).  xb uint16 [m, 153]; wb uint16 [H, >= 153]; bias float32 [H] or None."""
    x, w = widen(xb), widen(np.asarray(wb)[:, :K])
    b = np.zeros(len(w)) if bias is None else np.asarray(bias, np.float64)
    s = x @ w.T + b
    mag = np.abs(x) @ np.abs(w).T + np.abs(b)
    out = np.where(s > 0, s, 0.0) if relu else s
    return out, 2 * (KPAD + 2) * U * mag + U * np.abs(out)


def dp_values(dout, out=None):
    """dp of bg_linear_rows_grad as float64: bfloat16(dout), +0.0 where the forward's output is not > 0 (out given = ReLU)."""
    dout = np.asarray(dout)
    dp = widen(dout) if dout.dtype == np.uint16 else widen(to_bf16_bits(dout))
    if out is not None:
        dp = np.where(np.asarray(out, np.float64) > 0, dp, 0.0)
    return dp


def grad(xb, dp, rows_per_group):
    """-> (dweight float64 [H, 153], its bound, dbias float64 [H], its bound)."""
    x = widen(xb)
    dw, dwm = dp.T @ x, np.abs(dp).T @ np.abs(x)
    db, dbm = dp.sum(0), np.abs(dp).sum(0)
    f = 2 * (rows_per_group + 2) * U
    return dw, f * dwm + U * np.abs(dw), db, f * dbm + U * np.abs(db)


def groups(m, H):
    """The number of partials bg_linear_rows_grad writes (include/balatro_mi355x.h): at most 256 / ceil(H / 256) groups of consecutive 128-row blocks."""
    blocks = -(-m // ROWS)
    cap = max(1, 256 // -(-H // 256))
    per = -(-blocks // cap)
    return -(-blocks // per)


def workspace_bytes(m, H):
    return groups(m, H) * PART_ROWS * H * 4


def grad_rows_per_group(m, H):
    blocks = -(-m // ROWS)
    return ROWS * -(-blocks // groups(m, H))


def check_close(got, want, bound, what):
    """Prints the worst ratio of the error to the bound, then asserts."""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert np.isfinite(got).all() and np.isfinite(want).all(), f"{what}: not finite"
    err = np.abs(got - want)
    ratio = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"{what}: worst error / bound = {ratio[at]:.4g} at {tuple(int(i) for i in at)} (error {err[at]:.4g}, bound {bound[at]:.4g})")
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} of {err.size} elements beyond the bound, worst ratio {ratio[at]:.4g} at {at}"


def small_int_obs(m, seed):
    """key -> [m, ...] records whose fields are integers in 0..15 and progress_ratio a multiple of 1/8 below 2: exact in bfloat16, and every sum of 153
    products with integer weights of magnitude <= 4 stays far below 2**24, so float32 accumulation is exact in ANY order."""
    from balatro_gym_amd import _native as nat
    rng = np.random.default_rng(seed)
    obs = {}
    for k in nat.OBS_KEYS:
        dt, shape = nat.OBS_SPEC[k]
        v = rng.integers(0, 16, (m,) + shape)
        obs[k] = (v / 8.0).astype(np.float32) if dt == "float32" else v.astype(dt)
    return obs


def finite_obs(m, seed):
    """key -> [m, ...] random records with every field within +-2**15 (progress_ratio uniform in [-4, 4)): finite, of mixed sign and magnitude."""
    from balatro_gym_amd import _native as nat
    rng = np.random.default_rng(seed)
    obs = {}
    for k in nat.OBS_KEYS:
        dt, shape = nat.OBS_SPEC[k]
        if dt == "float32":
            obs[k] = rng.uniform(-4, 4, (m,) + shape).astype(np.float32)
        else:
            hi = min(int(np.iinfo(dt).max), 2 ** 15)
            obs[k] = rng.integers(-hi, hi, (m,) + shape, endpoint=True).astype(dt)
    return obs


def int_weight(H, cols=K):
    """w[n, k] = ((3 n + 5 k) mod 9) - 4 as bfloat16 bits: asymmetric, so a row / column swap cannot pass."""
    n, k = np.arange(H)[:, None], np.arange(cols)[None, :]
    return to_bf16_bits((((3 * n + 5 * k) % 9) - 4).astype(np.float32))
