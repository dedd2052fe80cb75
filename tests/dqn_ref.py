"""bg_dqn_loss and bg_sample_actions_eps (csrc/bg_dqn.h) restated: the reference of tests/test_dqn_loss_host.py (the header compiled with g++) and
tests/test_dqn_loss.py (the kernels).  The contract is stated twice.

(a) `Contract`: the per-row rule of the header in numpy float32, operation by operation (every numpy float32 operation rounds on its own, and nothing is
    fused).  The contract has no transcendental function and no undecidable row, so the product is held to (a) BIT FOR BIT on every row: dq, td, the
    excluded rows and their count.  The scalars are float64 sums of (a)'s float32 terms; the product's are within
        2**-24 * |ref| + 2**-50 * (sum of |terms|)
    of them: one final rounding to float32 (at most 2**-24 relative), plus a float64 accumulation of at most 2**20 float32 terms in any order.  The
    terms carry 24 significant bits each, so float64 partial sums of them are exact over 29 binades of dynamic range and round by 2**-53 of the
    partial sum beyond that; along the at most 6 + 8 + 1 levels of the tree and the slices that stays below 2**-50 of the sum of absolute terms, for
    the reference's own pairwise sum as for the product's fixed order.

(b) `sb3_statement`: SB3's `DQN.train` loss written literally in torch float64 under autograd on the host:
        F.smooth_l1_loss(q.gather(1, a), r + (1 - done) * gamma * q_next.max(1))        with the mask as masked_fill(-inf)
    (double DQN: q_next.gather(1, masked q_next_online.argmax(1))), summed over the rows (a) includes and divided by m, as the contract's divisor
    stays m.  One departure, which the contract states: a done row reads neither q_next matrix, so its q_next is replaced by zeros before the
    product with (1 - done) (SB3's 0 * NaN would be NaN).

(a) is held to (b) by a bound from the operation count.  With ulp = 2**-24 (the relative error of one float32 rounding) and
scale = |q[a]| + |r| + gamma * |n|:
    y       three roundings: float(r) from the record's float64, gamma * n, and the sum: each at most ulp * scale
    d       one more: |d32 - d64| <= 4 * ulp * scale  =: dd                 (td is held to this)
    term    Huber and MSE are continuously differentiable with |term'(d)| = |g(d)|, so the error of d moves the term by at most (|g| + 2 * dd) * dd (the
            slope anywhere on the segment is within 2 * dd of |g|); its own two roundings ((0.5 * d) * d, or one for |d| - 0.5 and d * d) add
            2 * ulp * |term|
    g       Huber: g = d or sign(d), which differ by at most dd where the two precisions take different branches at |d| = 1: |g32 - g64| <= dd;
            MSE: 2 * dd (the doubling is exact)
    dq      g / float(m): one more rounding: (|g32 - g64| + ulp * |g|) / m
The largest observed shares of these bounds are recorded in the docstrings of the two test modules.

The epsilon-greedy rule is restated in Python integers (`eps_actions`), bit for bit on every row.
"""
from __future__ import annotations

import numpy as np

from tests import head_ref

ACTIONS = 60
STATS = ("loss", "q_mean", "target_mean", "abs_td_mean", "abs_td_max", "done_share", "excluded", "m")
MASK_NEXT, MSE, TIMEOUT_EXCLUDE = 1, 2, 4
END_MAX_STEPS = 4
OFF_REWARD, OFF_ACTION, OFF_MASK, OFF_TERMINATED, OFF_END_FLAGS = 136, 172, 176, 342, 343
ROW_BYTES = 352
REWARDS = np.array([-50.0, -1.2, -1.0, 0.0, 1.0, 0.0, 1.0, -1.0, 12.5, 137.0, 2500.0])   # what the env produces, and a few large positive ones
DONE_SHARE = 0.05
ULP = 2.0 ** -24
EPS_SALT = 0x632BE59BD9B4E019
QNAN_BITS = 0x7FC00000
HAND_ROWS = 32   # hand-made rows appended to every set


def _to_bf16(x):
    return head_ref.widen_bf16(head_ref.bf16_bits(np.ascontiguousarray(x, np.float32)))


class Case:
    """One minibatch over one store.  q, q_next, q_online float32 [m, 60]; rows uint8 [store_rows, stride]; next_index int32 [m]; rewards float32
    [store_rows] (the alternative reward source)."""

    def __init__(self, q, q_next, q_online, rows, next_index, rewards):
        self.q, self.q_next, self.q_online, self.rows, self.next_index, self.rewards = q, q_next, q_online, rows, next_index, rewards
        self.m, self.store_rows, self.stride = q.shape[0], rows.shape[0], rows.shape[1]

    # the record fields as the store holds them
    def field(self, off, dt):
        n = np.dtype(dt).itemsize
        return np.ascontiguousarray(self.rows[:, off:off + n]).view(dt)[:, 0]


def _put(rows, i, off, value, dt):
    rows[i, off:off + np.dtype(dt).itemsize] = np.array([value], dtype=dt).view(np.uint8)


def synthetic(seed: int, m: int, sigma: float, *, bf16: bool = False, stride: int = 384, base_rows=None, hand_made: bool = True) -> Case:
    """m rows in all; the last HAND_ROWS are the hand-made ones (when m > HAND_ROWS and hand_made).  The store holds m + 3 records (three are never
    named); the named records are a permutation.  base_rows: records the product wrote ([>= 1, stride] uint8), repeated to fill the store: only the
    fields the loss reads are written over them."""
    rng = np.random.default_rng(seed)
    S = m + 3
    q = (rng.standard_normal((m, ACTIONS)) * sigma).astype(np.float32)
    qn = (rng.standard_normal((m, ACTIONS)) * sigma).astype(np.float32)
    qo = (qn + rng.standard_normal((m, ACTIONS)).astype(np.float32) * np.float32(0.5 * sigma)).astype(np.float32)
    if base_rows is None:
        rows = np.zeros((S, stride), np.uint8)
        rows[:, ROW_BYTES:] = 0
    else:
        base_rows = np.asarray(base_rows, np.uint8)
        assert base_rows.shape[1] == stride
        rows = np.ascontiguousarray(base_rows[np.arange(S) % base_rows.shape[0]])
    rows[:, OFF_MASK:OFF_MASK + ACTIONS] = (rng.random((S, ACTIONS)) >= head_ref.MASKED_SHARE).astype(np.uint8) * rng.integers(1, 4, (S, ACTIONS)).astype(np.uint8)
    rows[:, OFF_ACTION:OFF_ACTION + 4] = rng.integers(0, ACTIONS, S).astype(np.int32).view(np.uint8).reshape(S, 4)
    rows[:, OFF_REWARD:OFF_REWARD + 8] = REWARDS[rng.integers(0, len(REWARDS), S)].view(np.uint8).reshape(S, 8)
    done = rng.random(S) < DONE_SHARE
    rows[:, OFF_TERMINATED] = done
    rows[:, OFF_END_FLAGS] = np.where(done, np.array([1, 2, 4, 8, 5, 12], np.uint8)[rng.integers(0, 6, S)], 0)
    nx = rng.permutation(S)[:m].astype(np.int32)
    if hand_made and m > HAND_ROWS:
        h0 = m - HAND_ROWS
        one = np.float32(1.0)
        below, above = np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2))

        def rec(k, action=3, reward=0.0, term=0, flags=0, mask=None):
            i = int(nx[h0 + k])
            _put(rows, i, OFF_ACTION, action, np.int32)
            _put(rows, i, OFF_REWARD, reward, np.float64)
            rows[i, OFF_TERMINATED], rows[i, OFF_END_FLAGS] = term, flags
            if mask is not None:
                rows[i, OFF_MASK:OFF_MASK + ACTIONS] = mask
            return h0 + k
        # 0..5: |d| exactly 1, just below and just above, both signs (done rows: y = r = 0, d = q[a])
        for k, v in enumerate((one, below, above, -one, -below, -above)):
            q[rec(k, term=1, flags=1), 3] = v
        # 6: a tie in the plain max (and in the online max, at two valid j whose target values differ: the smaller j wins)
        i = rec(6, mask=np.ones(ACTIONS, np.uint8))
        qn[i] = np.float32(-2.0); qn[i, 7] = np.float32(1.5); qn[i, 41] = np.float32(1.5)
        qo[i] = np.float32(-1.0); qo[i, 11] = np.float32(2.0); qo[i, 30] = np.float32(2.0); qn[i, 11] = np.float32(0.25); qn[i, 30] = np.float32(0.75)
        # 7: the same tie with the first of the pair masked
        mk = np.ones(ACTIONS, np.uint8); mk[7] = 0; mk[11] = 0
        i = rec(7, mask=mk)
        qn[i] = qn[h0 + 6]; qo[i] = qo[h0 + 6]
        # 8: a done row whose q_next (and online) is all NaN: included
        i = rec(8, term=1, flags=1, reward=1.0)
        qn[i] = np.nan; qo[i] = np.nan
        # 9: an all-masked next row, not done: excluded with the mask, included without
        rec(9, mask=np.zeros(ACTIONS, np.uint8))
        # 10..12: actions outside [0, 60)
        for k, a in enumerate((-1, 60, 32770)):
            rec(10 + k, action=a)
        # 13, 14: next_index outside the store
        nx[h0 + 13], nx[h0 + 14] = -1, S
        # 15, 16: non-finite rewards
        rec(15, reward=np.inf); rec(16, reward=np.nan)
        # 17..19: end_flags 4, 5, 1 on done rows (with BG_DQN_TIMEOUT_EXCLUDE only the first is excluded)
        for k, f in enumerate((4, 5, 1)):
            rec(17 + k, term=1, flags=f, reward=-1.0)
        # 20: NaN at a valid next action, 21: NaN at a masked one only, 22: q[a] not finite, 23: the target's value +inf at the maximum
        mk = np.ones(ACTIONS, np.uint8); mk[5] = 0
        i = rec(20, mask=mk); qn[i, 6] = np.nan; qo[i, 6] = np.nan
        i = rec(21, mask=mk); qn[i, 5] = np.nan; qo[i, 5] = np.nan
        q[rec(22), 3] = np.inf
        i = rec(23, mask=np.ones(ACTIONS, np.uint8)); qn[i, 9] = np.inf
        # 24: every valid next value -inf; 25: one valid action only; 26: the online maximum where the target's value is NaN
        i = rec(24, mask=mk); qn[i] = -np.inf; qo[i] = -np.inf
        mk1 = np.zeros(ACTIONS, np.uint8); mk1[59] = 1
        rec(25, mask=mk1)
        i = rec(26, mask=np.ones(ACTIONS, np.uint8)); qo[i, 17] = np.float32(1e6); qn[i, 17] = np.nan
        # 27: a large reward and a not-done bootstrap; 28: gamma * n with n negative; 29..31: ordinary rows
        rec(27, reward=2500.0); rec(28, reward=-50.0)
    if bf16:
        q, qn, qo = _to_bf16(q), _to_bf16(qn), _to_bf16(qo)
    r64 = np.ascontiguousarray(rows[:, OFF_REWARD:OFF_REWARD + 8]).view(np.float64)[:, 0]
    with np.errstate(all="ignore"):
        rewards = (r64 * 0.125 + 0.5).astype(np.float32)   # a "normalised" reward: another value than the record's, non-finite where it is
    return Case(q, qn, qo, rows, nx, rewards)


class Contract:
    """(a): the per-row rule in numpy float32, and the float64 sums of its terms."""

    def __init__(self, c: Case, gamma: float, flags: int, double: bool, use_rewards: bool = False):
        self.c, self.flags, self.double = c, flags, double
        m, S = c.m, c.store_rows
        f32 = np.float32
        self.gamma32 = g32 = f32(gamma)
        nx = c.next_index.astype(np.int64)
        ok = (nx >= 0) & (nx < S)
        nxc = np.where(ok, nx, 0)
        a = c.field(OFF_ACTION, np.int32)[nxc]
        with np.errstate(all="ignore"):
            r = (c.rewards[nxc] if use_rewards else c.field(OFF_REWARD, np.float64)[nxc].astype(f32)).astype(f32)
        self.r64 = (c.rewards[nxc].astype(np.float64) if use_rewards else c.field(OFF_REWARD, np.float64)[nxc])
        done = c.rows[nxc, OFF_TERMINATED] != 0
        ef = c.rows[nxc, OFF_END_FLAGS]
        inr = ok & (a >= 0) & (a < ACTIONS)
        ac = np.where(inr, a, 0)
        rows_i = np.arange(m)
        qa = c.q[rows_i, ac]
        valid = (c.rows[nxc, OFF_MASK:OFF_MASK + ACTIONS] != 0) if flags & MASK_NEXT else np.ones((m, ACTIONS), bool)
        sel = c.q_online if double else c.q_next
        with np.errstate(all="ignore"):
            nanv = (valid & np.isnan(sel)).any(axis=1)
            empty = ~valid.any(axis=1)
            selv = np.where(valid & ~np.isnan(sel), sel, -np.inf)
            mx = selv.max(axis=1)
            arg = (valid & (selv == mx[:, None])).argmax(axis=1)   # the smallest valid j at the maximum (all -inf: the first valid j)
            n = c.q_next[rows_i, arg] if double else mx.astype(f32)
            excl = ~inr | ~np.isfinite(r) | ~np.isfinite(qa)
            excl |= ~done & (empty | nanv | ~np.isfinite(n))
            if flags & TIMEOUT_EXCLUDE:
                excl |= done & (ef == END_MAX_STEPS)
            gn = (g32 * n).astype(f32)
            y = np.where(done, r, (r + gn).astype(f32)).astype(f32)
            d = (qa - y).astype(f32)
            ad = np.abs(d)
            if flags & MSE:
                term, g = (d * d).astype(f32), (f32(2.0) * d).astype(f32)
            else:
                term = np.where(ad < f32(1.0), ((f32(0.5) * d).astype(f32) * d).astype(f32), (ad - f32(0.5)).astype(f32))
                g = np.where(ad < f32(1.0), d, np.copysign(f32(1.0), d)).astype(f32)
            dqa = (g / f32(m)).astype(f32)
        inc = ~excl
        self.excluded, self.included, self.done, self.a, self.arg, self.valid, self.ok = excl, inc, done & inc, ac, arg, valid, ok
        self.done_raw = done & ok
        self.n = np.where(done | excl, 0.0, n).astype(np.float64)
        self.qa, self.y, self.d, self.g, self.term = (np.where(inc, x, 0).astype(f32) for x in (qa, y, d, g, term))
        self.td = np.where(inc, d, np.uint32(QNAN_BITS).view(f32)).astype(f32)
        self.dq = np.zeros((m, ACTIONS), f32)
        self.dq[rows_i[inc], ac[inc]] = dqa[inc]
        f64 = np.float64
        sums = {"loss": self.term.astype(f64), "q_mean": self.qa.astype(f64), "target_mean": self.y.astype(f64), "abs_td_mean": np.abs(self.d).astype(f64),
                "done_share": self.done.astype(f64)}
        self.stats = {k: float(v.sum() / m) for k, v in sums.items()}
        self.stats_abs = {k: float(np.abs(v).sum() / m) for k, v in sums.items()}
        self.stats["abs_td_max"] = self.stats_abs["abs_td_max"] = float(np.abs(self.d).astype(f64).max()) if m else 0.0
        self.stats["excluded"] = self.stats_abs["excluded"] = float(excl.sum())
        self.stats["m"] = self.stats_abs["m"] = float(m)

    def check(self, dq, td, stats, what: str) -> float:
        """The product's outputs against (a): dq / td bit for bit on every row (so the excluded rows are exactly (a)'s), the scalars within the bound
        of the module docstring.  dq: float32 [m, 60]; td: float32 [m] or None; stats: float32 [8].  -> the largest share of a scalar bound."""
        bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)   # noqa: E731
        bad = np.flatnonzero((bits(dq) != bits(self.dq)).any(axis=1))
        assert bad.size == 0, f"{what}: {bad.size} dq rows differ from the contract, first row {bad[0]}: got {dq[bad[0]][self.a[bad[0]]]!r}, want {self.dq[bad[0]][self.a[bad[0]]]!r}"
        if td is not None:
            bad = np.flatnonzero(bits(td) != bits(self.td))
            assert bad.size == 0, f"{what}: {bad.size} td values differ, first row {bad[0]}: got {td[bad[0]]!r}, want {self.td[bad[0]]!r}"
            assert np.array_equal(np.isnan(td), self.excluded | np.isnan(self.td)), what
        worst = 0.0
        for k, name in enumerate(STATS):
            ref, got = self.stats[name], float(stats[k])
            if not np.isfinite(ref):
                assert (np.isnan(ref) and np.isnan(got)) or ref == got, f"{what}: {name} {got} want {ref}"
                continue
            bound = 2.0 ** -24 * abs(ref) + 2.0 ** -50 * self.stats_abs[name]
            err = abs(got - ref)
            assert err <= bound, f"{what}: {name} = {got!r}, reference {ref!r}: off by {err:.3g}, bound {bound:.3g}"
            worst = max(worst, err / bound if bound > 0 else 0.0)
        assert stats[6] == self.excluded.sum() and stats[7] == self.c.m, what
        return worst


def sb3_statement(c: Case, ct: Contract, gamma32, params=None):
    """(b): SB3's loss in torch float64 under autograd over the rows (a) includes, the divisor m.  -> (loss, dq [m, 60], td [m]) as float64 numpy; with
    params = a float64 torch tensor [m, 60] that requires grad through a network: (loss tensor, None, td)."""
    import torch
    import torch.nn.functional as F
    m = c.m
    inc = torch.from_numpy(ct.included)
    q = params if params is not None else torch.from_numpy(c.q.astype(np.float64)).requires_grad_(True)
    done = torch.from_numpy(ct.done_raw.astype(np.float64))
    keep = (done == 0)[:, None]
    qn = torch.where(keep, torch.from_numpy(np.nan_to_num(c.q_next.astype(np.float64), nan=0.0, posinf=0.0, neginf=-np.inf)), torch.zeros(()).double())
    qo = torch.where(keep, torch.from_numpy(np.nan_to_num(c.q_online.astype(np.float64), nan=0.0, posinf=0.0, neginf=-np.inf)), torch.zeros(()).double())
    valid = torch.from_numpy(ct.valid) | ~keep
    a = torch.from_numpy(ct.a.astype(np.int64))[:, None]
    r = torch.from_numpy(np.nan_to_num(ct.r64, nan=0.0, posinf=0.0, neginf=0.0))
    if ct.double:
        nxt = qn.gather(1, qo.masked_fill(~valid, -np.inf).argmax(1, keepdim=True))[:, 0]
    else:
        nxt = qn.masked_fill(~valid, -np.inf).max(1).values
    nxt = torch.where(torch.isfinite(nxt), nxt, torch.zeros(()).double())   # (rows (a) excludes; they are left out below)
    target = (r + (1.0 - done) * float(gamma32) * nxt).detach()
    cur = q.gather(1, a)[:, 0]
    cur = torch.where(inc, cur, target)    # an excluded row: no term, no gradient
    if ct.flags & MSE:
        loss = F.mse_loss(cur, target, reduction="sum") / m
    else:
        loss = F.smooth_l1_loss(cur, target, reduction="sum") / m
    td = np.where(ct.included, (cur - target).detach().numpy(), np.nan)
    if params is not None:
        return loss, None, td
    loss.backward()
    return float(loss.detach()), q.grad.numpy(), td


def check_contract_against_sb3(c: Case, ct: Contract, what: str) -> dict:
    """(a) within the derived bounds of (b) -> the largest observed share of each bound."""
    loss64, dq64, td64 = sb3_statement(c, ct, ct.gamma32)
    inc = ct.included
    m = c.m
    r = np.where(inc, np.nan_to_num(ct.r64, nan=0.0, posinf=0.0, neginf=0.0), 0.0)
    scale = np.abs(ct.qa.astype(np.float64)) + np.abs(r) + float(ct.gamma32) * np.abs(np.where(inc, ct.n, 0.0))
    dd = 4 * ULP * scale
    sh = {}
    err = np.abs(ct.td[inc].astype(np.float64) - td64[inc])
    assert (err <= dd[inc]).all(), f"{what}: td off by {np.max(err / np.maximum(dd[inc], 1e-300)):.3f} of its bound"
    sh["td"] = float((err / np.maximum(dd[inc], 1e-300)).max()) if inc.any() else 0.0
    g = np.abs(ct.g.astype(np.float64))
    gb = ((2.0 if ct.flags & MSE else 1.0) * dd + ULP * g) / m
    rows_i = np.arange(m)
    gerr = np.abs(ct.dq[rows_i, ct.a].astype(np.float64) - dq64[rows_i, ct.a])
    assert (gerr[inc] <= gb[inc] + 1e-300).all(), f"{what}: dq off by {np.max(gerr[inc] / np.maximum(gb[inc], 1e-300)):.3f} of its bound"
    sh["dq"] = float((gerr[inc] / np.maximum(gb[inc], 1e-300)).max()) if inc.any() else 0.0
    other = dq64.copy(); other[rows_i, ct.a] = 0.0
    assert (other == 0.0).all() and (dq64[~inc] == 0.0).all(), f"{what}: the float64 gradient has an entry off the action's column or on an excluded row"
    tb = ((g + 2 * dd) * dd + 2 * ULP * np.abs(ct.term.astype(np.float64)))[inc].sum() / m
    lerr = abs(ct.stats["loss"] - loss64)
    assert lerr <= tb + 1e-300, f"{what}: loss {ct.stats['loss']!r} against SB3's {loss64!r}: off by {lerr:.3g}, bound {tb:.3g}"
    sh["loss"] = lerr / tb if tb > 0 else 0.0
    return sh


# ---------------------------------------------------------------- epsilon-greedy

def eps_actions(logits, mask, seed: int, index0: int, t: int, epsilon: float):
    """bg_sample_actions_eps restated in Python integers, row by row -> (actions int32 [m], explored bool [m])."""
    l = np.asarray(logits, np.float32)
    m = l.shape[0]
    valid = np.ones((m, ACTIONS), bool) if mask is None else np.asarray(mask).reshape(m, ACTIONS) != 0
    eps32 = np.float32(epsilon)
    out, explored = np.empty(m, np.int32), np.zeros(m, bool)
    M64 = (1 << 64) - 1
    for i in range(m):
        js = [j for j in range(ACTIONS) if valid[i, j]]
        vals = [float(l[i, j]) for j in js]
        h = head_ref.policy_hash_scalar(seed & M64, (index0 + i) & M64, t)
        u = np.float32((h >> 8) * 2.0 ** -24)
        explored[i] = bool(u < eps32)
        if not js or any(v != v or v == float("inf") for v in vals) or max(vals) == float("-inf"):
            out[i] = -1
            continue
        if explored[i]:
            h2 = head_ref.policy_hash_scalar((seed + EPS_SALT) & M64, (index0 + i) & M64, t)
            out[i] = js[(h2 * len(js)) >> 32]
        else:
            out[i] = js[vals.index(max(vals))]
    return out, explored
