"""The masked categorical policy head (bg_sample_actions / bg_evaluate_actions; csrc/bg_head.h) restated in numpy, in float64: the reference of
tests/test_policy_head_host.py (the header compiled with g++) and tests/test_policy_head.py (the kernel).

The contract computes in float32, so it is held to this reference by BOUNDS, not bit for bit:
  * a row is DECIDABLE when no prefix sum lies within DELTA = 2**-16 (relative to S) of the threshold u * S; on decidable rows the drawn action must be
    the reference's.  A float32 prefix of at most 60 terms carries a relative error of at most 60 * 2**-24; a few ulp more for expf and the subtraction
    make about 4e-6, and DELTA is four times that.  At most 60 boundaries each exclude 2 * DELTA of u: at most 0.18 % of rows in expectation, and
    UNDECIDABLE_CAP = 0.5 % of a test set's rows is what a test set may hold (the generators below stay far inside it);
  * on EVERY row the drawn action is valid under the mask and  P[action - 1] - DELTA * S <= u * S <= P[action] + DELTA * S;
  * log_prob is within 2**-17 + 2**-22 * |d[action]| of float64, entropy within 2**-17 * (1 + sum p_j |d_j|): both from the operation counts
    (expf / logf / the 60-term sums each within a few float32 ulp of values of magnitude <= log 60 + |d|).
"""
from __future__ import annotations

import numpy as np

ACTIONS = 60
DELTA = 2.0 ** -16
UNDECIDABLE_CAP = 0.005
QNAN_BITS = 0x7FC00000
SIGMAS = (0.1, 1.0, 3.0, 10.0)
MASKED_SHARE = 0.4

_M64 = (1 << 64) - 1


def policy_hash(seed: int, index, t: int) -> np.ndarray:
    """bg_policy_hash / bg_head_hash over an array of env indices: the splitmix64 finaliser, high 32 bits."""
    idx = np.asarray(index, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = np.uint64(seed & _M64) + np.uint64(0x9E3779B97F4A7C15) * (idx + np.uint64(1)) + np.uint64((0xD1B54A32D192ED03 * ((t + 1) & _M64)) & _M64)
        x ^= x >> np.uint64(30); x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27); x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (x >> np.uint64(32)).astype(np.uint32)


def policy_hash_scalar(seed: int, index: int, t: int) -> int:
    """The same in Python integers (an independent restatement for the bit-for-bit check)."""
    x = (seed + 0x9E3779B97F4A7C15 * (index + 1) + 0xD1B54A32D192ED03 * (t + 1)) & _M64
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & _M64
    x ^= x >> 31
    return x >> 32


def uniform(h) -> np.ndarray:
    """u = float(h >> 8) * 2**-24, exact in float32 and so in float64."""
    return (np.asarray(h, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def bf16_bits(x32: np.ndarray) -> np.ndarray:
    """float32 -> bfloat16 bits, round to nearest even (finite inputs and infinities)."""
    u = np.ascontiguousarray(x32, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def widen_bf16(b16: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(b16, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def synthetic(seed: int, m: int, sigma: float, masked: bool):
    """N(0, sigma^2) float32 logits [m, 60] and (masked) an int8 mask that hides each action with probability MASKED_SHARE."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((m, ACTIONS)) * sigma).astype(np.float32)
    mask = (rng.random((m, ACTIONS)) >= MASKED_SHARE).astype(np.int8) if masked else None
    return logits, mask


class Reference:
    """Everything the contract defines, per row, in float64, from float32-valued logits [m, 60] and a mask [m, 60] (non-zero = valid) or None."""

    def __init__(self, logits, mask=None, seed: int = 0, index0: int = 0, t: int = 0):
        l = np.asarray(logits, dtype=np.float64)
        assert l.ndim == 2 and l.shape[1] == ACTIONS
        self.m = m = l.shape[0]
        self.valid = valid = np.ones((m, ACTIONS), bool) if mask is None else np.asarray(mask).reshape(m, ACTIONS) != 0
        with np.errstate(all="ignore"):
            lv = np.where(valid, l, -np.inf)
            mx = lv.max(axis=1) if m else np.zeros(0)
            bad = (valid & (np.isnan(l) | (l == np.inf))).any(axis=1)
            self.degenerate = deg = bad | ~np.isfinite(mx) | np.isnan(mx)
            mx = np.where(deg, 0.0, mx)
            self.d = d = np.where(valid & ~deg[:, None], l - mx[:, None], -np.inf)
            self.e = e = np.exp(d)                       # 0 for invalid j and for every j of a degenerate row
            self.P = P = np.cumsum(e, axis=1)
            self.S = S = P[:, -1] if m else np.zeros(0)
            self.u = u = uniform(policy_hash(seed, np.uint64(index0 & _M64) + np.arange(m, dtype=np.uint64), t))
            self.thr = thr = u * S
            pos = e > 0
            hit = pos & (P > thr[:, None])
            self.action = np.where(deg, -1, np.where(hit.any(axis=1), hit.argmax(axis=1), ACTIONS - 1 - pos[:, ::-1].argmax(axis=1))).astype(np.int32)
            self.mode = np.where(deg, -1, (valid & (lv == lv.max(axis=1, keepdims=True))).argmax(axis=1)).astype(np.int32)
            self.margin = np.where(pos, np.abs(P - thr[:, None]) / np.where(deg, 1.0, S)[:, None], np.inf).min(axis=1)
            self.decidable = deg | (self.margin > DELTA)
            self.logS = np.log(np.where(deg, 1.0, S))
            p = e / np.where(deg, 1.0, S)[:, None]
            ed = np.where(pos, e * np.where(pos, d, 0.0), 0.0)
            self.entropy = np.where(deg, np.nan, self.logS - ed.sum(axis=1) / np.where(deg, 1.0, S))
            self.spread = np.where(pos, p * np.abs(np.where(pos, d, 0.0)), 0.0).sum(axis=1)   # sum p_j |d_j|

    def log_prob(self, actions) -> np.ndarray:
        """float64 log-probability of given actions: NaN for a degenerate row or an action outside [0, 60), -inf for a masked one."""
        a = np.asarray(actions, dtype=np.int64)
        inr = (a >= 0) & (a < ACTIONS)
        ac = np.where(inr, a, 0)
        rows = np.arange(self.m)
        with np.errstate(all="ignore"):
            lp = self.d[rows, ac] - self.logS
        lp = np.where(self.valid[rows, ac], lp, -np.inf)
        return np.where(self.degenerate | ~inr, np.nan, lp)

    # ---- the assertions of the issue, shared by the host and the GPU test; each returns the largest observed share of its bound ----
    def check_sampled(self, actions, what: str, cap: bool = True) -> float:
        """cap=False: these rows are a slice of a test set whose share of undecidable rows is checked on the whole set."""
        a = np.asarray(actions, dtype=np.int64)
        assert a.shape == (self.m,), what
        und = ~self.decidable
        assert not cap or und.sum() <= UNDECIDABLE_CAP * self.m, f"{what}: {und.sum()} of {self.m} rows undecidable: the test set is unfit"
        assert np.array_equal(a[self.degenerate], np.full(int(self.degenerate.sum()), -1)), f"{what}: a degenerate row must give action -1"
        live = ~self.degenerate
        rows = np.arange(self.m)[live]
        al = a[live]
        assert ((al >= 0) & (al < ACTIONS)).all(), f"{what}: action out of range"
        assert self.valid[rows, al].all(), f"{what}: a masked action was returned"
        dec = self.decidable & live
        wrong = np.flatnonzero(dec & (a != self.action))
        assert wrong.size == 0, f"{what}: {wrong.size} decidable rows differ, first row {wrong[0]}: got {a[wrong[0]]}, want {self.action[wrong[0]]} (margin {self.margin[wrong[0]]:.3g})"
        S, thr = self.S[live], self.thr[live]
        hi = self.P[rows, al]
        lo = np.where(al > 0, self.P[rows, np.maximum(al - 1, 0)], 0.0)
        ok = (lo - DELTA * S <= thr) & (thr <= hi + DELTA * S)
        assert ok.all(), f"{what}: row {rows[np.flatnonzero(~ok)[0]]}: the action's interval does not hold u * S within DELTA * S"
        return float(und.mean()) if self.m else 0.0

    def check_stats(self, actions, log_prob, entropy, what: str) -> tuple:
        """log_prob / entropy (float32 arrays) of `actions` against float64; returns the largest share of each bound that was used."""
        lp, en = np.asarray(log_prob, np.float32), np.asarray(entropy, np.float32)
        want = self.log_prob(actions)
        nanw = np.isnan(want)
        assert np.array_equal(lp.view(np.uint32)[nanw], np.full(int(nanw.sum()), QNAN_BITS, np.uint32)), f"{what}: log_prob must be the quiet NaN {QNAN_BITS:#x}"
        infw = np.isneginf(want)
        assert np.array_equal(np.isneginf(lp), infw) and not np.isnan(lp[~nanw]).any(), f"{what}: log_prob -inf / NaN pattern"
        fin = ~nanw & ~infw
        a = np.asarray(actions, np.int64)
        dabs = np.abs(self.d[np.arange(self.m)[fin], a[fin]])
        bound = 2.0 ** -17 + 2.0 ** -22 * dabs
        err = np.abs(lp[fin].astype(np.float64) - want[fin])
        share_lp = float((err / bound).max()) if fin.any() else 0.0
        assert share_lp <= 1.0, f"{what}: log_prob off by {share_lp:.3f} of its bound"
        deg = self.degenerate
        assert np.array_equal(en.view(np.uint32)[deg], np.full(int(deg.sum()), QNAN_BITS, np.uint32)), f"{what}: entropy of a degenerate row must be the quiet NaN"
        live = ~deg
        eb = 2.0 ** -17 * (1.0 + self.spread[live])
        ee = np.abs(en[live].astype(np.float64) - self.entropy[live])
        assert not np.isnan(en[live]).any(), f"{what}: entropy NaN on a live row"
        share_en = float((ee / eb).max()) if live.any() else 0.0
        assert share_en <= 1.0, f"{what}: entropy off by {share_en:.3f} of its bound"
        return share_lp, share_en

    def check_mode(self, actions, what: str):
        assert np.array_equal(np.asarray(actions, np.int32), self.mode), f"{what}: deterministic action"
