"""Shared by tests/test_actor_rows_host.py and tests/test_actor_rows.py: the float64 statement of the actor calls' products (bg_actor_sample /
bg_actor_evaluate / bg_actor_ppo_loss) and their bounds.  The head and the loss behind the logits are not restated: they are held bit for bit to
sample_actions / evaluate_actions / ppo_loss on the same logits, which tests/head_ref.py and tests/ppo_ref.py hold to float64.

Everything is float64 numpy over the WIDENED bfloat16 operands (tests/linear_ref.py: `widen`, `to_bf16_bits`).  The bounds are derived as there: a
bfloat16 x bfloat16 product is exact in float32, so only the accumulation rounds; a float32 sum of L terms in any order is within (L - 1) u S of the
exact sum (u = 2**-24, S the sum of the magnitudes), (L + 2) with the bias add and the slack of the first-order statement, and a factor 2 because the
matrix unit's internal adder is not documented as round-to-nearest:
    logits           |got - ref| <= 2 (Hin + 2) u (sum_k |h w| + |b|)  + one float32 rounding of the result
    dh (float32)     |got - ref| <= 2 (64 + 2) u sum_j |dp w|          + one float32 rounding     (the 60 units padded to 64)
    dweight, dbias   |got - ref| <= 2 (L + 2) u sum_i |dp h| (|dp|)    + one float32 rounding, L = the rows one group accumulates in float32
                     (bg_actor_ppo_loss_rows_per_group); the float64 sum over the groups adds 2**-53 terms that vanish beside it
A bfloat16 dh is not bounded but held exactly: the nearest-even rounding of the float32 dh of the same call made with a float32 output."""
import numpy as np

from tests.linear_ref import U, check_close, to_bf16_bits, widen  # noqa: F401

UNITS = 60
ROWS = 64          # BG_ACT_ROWS: rows of a block
SPAN = 256         # BG_ACT_SPAN: k of one workgroup of the loss
MAX_WG = 256       # BG_ACT_MAX_WG


def weight_bits(weight):
    """The weight as the kernel reads it: bfloat16 bits as they are (uint16), float32 values rounded to nearest even."""
    weight = np.asarray(weight)
    return weight if weight.dtype == np.uint16 else to_bf16_bits(weight)


def logits(hb, wb, bias=None):
    """-> (ref float64 [m, 60], bound).  hb uint16 [m, Hin]; wb uint16 [60, Hin]; bias float32 [60] or None."""
    h, w = widen(hb), widen(wb)
    b = np.zeros(len(w)) if bias is None else np.asarray(bias, np.float64)
    s = h @ w.T + b
    mag = np.abs(h) @ np.abs(w).T + np.abs(b)
    return s, 2 * (h.shape[1] + 2) * U * mag + U * np.abs(s)


def dp_values(dlogits):
    """dp as float64 [m, 60]: bfloat16(dlogits), dlogits the float32 gradient of the loss with respect to the logits."""
    return widen(to_bf16_bits(np.asarray(dlogits, np.float32)))


def dh(dp, wb):
    """-> (ref float64 [m, Hin], bound for a float32 dh)."""
    w = widen(wb)
    s = dp @ w
    return s, 2 * (64 + 2) * U * (np.abs(dp) @ np.abs(w)) + U * np.abs(s)


def dweight(dp, hb, rows_per_group):
    """-> (dweight float64 [60, Hin], its bound, dbias float64 [60], its bound)."""
    h = widen(hb)
    dw, dwm = dp.T @ h, np.abs(dp).T @ np.abs(h)
    db, dbm = dp.sum(0), np.abs(dp).sum(0)
    f = 2 * (rows_per_group + 2) * U
    return dw, f * dwm + U * np.abs(dw), db, f * dbm + U * np.abs(db)


def groups(m, Hin):
    """The partials bg_actor_ppo_loss writes: at most 256 / ceil(Hin / 256) groups of consecutive 64-row blocks (include/balatro_mi355x.h)."""
    blocks = -(-m // ROWS)
    cap = MAX_WG // -(-Hin // SPAN)
    per = -(-blocks // cap)
    return -(-blocks // per)


def rows_per_group(m, Hin):
    blocks = -(-m // ROWS)
    return ROWS * -(-blocks // groups(m, Hin))


def ppo_workspace_bytes(m):
    """bg_ppo_loss_workspace_bytes(m): 16 bytes, a 24-byte triple per 256 rows, six float64 per 64 rows."""
    return 16 + -(-m // 256) * 24 + -(-m // 64) * 48


def workspace_bytes(m, Hin):
    return -(-ppo_workspace_bytes(m) // 16) * 16 + groups(m, Hin) * (UNITS * Hin + 64) * 4


class Case:
    """One call's inputs as host arrays: hb uint16 [m, Hin]; weight float32 or uint16 (bfloat16 bits) [60, Hin]; bias float32 [60] or None; the stored
    arrays mask int8 [store, 60] (or None), actions, old_log_prob, advantages, returns [store]; values [m]; index int32 [m] or None."""

    def src(self):
        """-> (ok [m], the stored row of every minibatch row, 0 where its index is out of range)."""
        if self.index is None:
            return np.ones(self.m, bool), np.arange(self.m)
        ok = (self.index >= 0) & (self.index < self.store_rows)
        return ok, np.where(ok, self.index, 0).astype(np.int64)

    def takes_part(self):
        """The rows the loss does not exclude (every float input of a case is finite): index in range, a valid action left, the stored action in range
        and not masked."""
        ok, s = self.src()
        a = self.actions[s]
        inr = (a >= 0) & (a < UNITS)
        if self.mask is None:
            return ok & inr
        mk = self.mask[s] != 0
        return ok & inr & mk.any(1) & mk[np.arange(self.m), np.where(inr, a, 0)]


def make_case(seed, m, Hin, mask=None, with_index=False, f32_weight=True, with_bias=True, specials=True):
    """mask: int8 [>= store, 60] (store = 2 m with an index, else m) or None.  h ~ N(0, 1) and weight ~ N(0, 4 / Hin) rounded to bfloat16 (a float32
    weight keeps its low bits: the kernel rounds it), so the logits spread over a few units.  Stored actions are valid under their row's mask;
    old_log_prob = the float64 log-prob of the row's logits + N(0, 0.15**2).  specials (m >= 16): minibatch row 3 reads an all-masked row, row 5 a
    masked stored action, row 9 the action 60, and with an index row 7's index is out of range."""
    rng = np.random.default_rng(seed)
    c = Case()
    c.m, c.Hin = m, Hin
    c.store_rows = S = 2 * m if with_index else m
    c.hb = to_bf16_bits(rng.standard_normal((m, Hin)).astype(np.float32))
    w = (rng.standard_normal((UNITS, Hin)) * 2.0 / np.sqrt(Hin)).astype(np.float32)
    c.weight = w if f32_weight else to_bf16_bits(w)
    c.bias = rng.standard_normal(UNITS).astype(np.float32) if with_bias else None
    c.index = rng.permutation(S)[:m].astype(np.int32) if with_index else None
    c.mask = None if mask is None else np.ascontiguousarray(mask[:S], np.int8).copy()
    assert c.mask is None or c.mask.shape == (S, UNITS)
    _, s = c.src()
    special = specials and m >= 16
    if special and c.mask is not None:
        c.mask[s[3]] = 0
    valid = np.ones((S, UNITS), bool) if c.mask is None else c.mask != 0
    c.actions = np.array([rng.choice(np.flatnonzero(v)) if v.any() else 0 for v in valid], np.int32)
    ref, _ = logits(c.hb, weight_bits(c.weight), c.bias)
    z = np.where(valid[s], ref, -np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        lp = z - (np.log(np.exp(z - z.max(1, keepdims=True)).sum(1, keepdims=True)) + z.max(1, keepdims=True))
    lp_a = np.nan_to_num(lp[np.arange(m), c.actions[s]], nan=0.0, neginf=0.0)
    c.old_log_prob = np.zeros(S, np.float32)
    c.old_log_prob[s] = (lp_a + rng.standard_normal(m) * 0.15).astype(np.float32)
    c.advantages = rng.standard_normal(S).astype(np.float32)
    c.returns = rng.standard_normal(S).astype(np.float32)
    c.values = rng.standard_normal(m).astype(np.float32)
    if special:
        if c.mask is not None:
            v5 = np.flatnonzero(c.mask[s[5]])
            if len(v5) >= 2:   # keep the row alive: only the stored action is masked
                c.mask[s[5], c.actions[s[5]]] = 0
        c.actions[s[9]] = UNITS
        if with_index:
            c.index[7] = S
    return c
