"""The reference of bg_ppo_loss (csrc/bg_ppo.h): PPO's clipped loss over the masked categorical head, its diagnostics and its gradient, in float64,
stated twice and never through the code under test:
  * `torch_statement`: SB3's `PPO.train` loss written literally in torch on the CPU (masked_fill with -inf, log_softmax, gather, exp, clamp, torch.min,
    mse_loss, the entropy with 0 * log 0 = 0), differentiated by torch's autograd;
  * `ClosedForm`: the formulas of the contract in numpy, on the quantities of tests/head_ref.py.
tests/test_ppo_loss_host.py holds the two to each other (ties and boundary rows included), then the header compiled with g++ to the closed form;
tests/test_ppo_loss.py does the same for the kernel.

The kernel computes in float32 and is held by BOUNDS:
  * log_prob / entropy: head_ref's bounds (check_stats);
  * a gradient element: EPS_i * (G_i * (1[j == a] + p_j) + ent_coef * p_j * (1 + |log p_j| + |H|)) / m plus one float32 ulp of the result, where EPS_i is
    four times head_ref's log-prob bound of the row (2**-17 + 2**-22 |d_a|): that bound enters once through ratio = exp(log_prob - old) and once more
    each through p_j and the entropy bracket, and four is the margin head_ref.DELTA takes.  G_i = |g| without normalisation.  With normalisation the
    float32 adv' = (adv - mean) / (std + 1e-8) carries an ABSOLUTE error the log-prob bound does not know: mean and std are float32 roundings (2**-24
    relative each), the subtraction and the division round once more, so |adv'_32 - adv'_64| <= DADV_i = 2**-22 * (|adv'| + (|adv| + |mean|) / std), and
    G_i = |g| + DADV_i * ratio  (g is adv' * ratio; for a row with adv' near 0 the first term alone would allow nothing);
  * a scalar: the mean of its rows' bounds (policy: EPS_i * max(|s1|, |s2|) + DADV_i * max(ratio, rc); kl: EPS_i * (ratio + 1); entropy: head_ref's;
    value: 2**-21 dv**2; clip_fraction: the share of undecidable rows) plus 2**-23 of the value for the final roundings.
The clip decision is discontinuous.  A row is DECIDABLE when the float64 ratio is farther than MARGIN = 2**-14 (relative) from lo and hi and the sign of
s1 - s2 is safe: s1 == s2, or the row is clipped with |adv'| > DADV_i.  Decidable rows must take the reference's branch; the others may take either
(g = adv' * ratio or g = 0).  A test set may hold at most UNDECIDABLE_CAP = 0.5 % of them (the generator gives about 0.06 %).
"""
from __future__ import annotations

import numpy as np

from tests import head_ref

ACTIONS = 60
MARGIN = 2.0 ** -14
UNDECIDABLE_CAP = 0.005
STATS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "adv_mean", "adv_std", "excluded", "m")
NOISE = 0.15   # old_log_prob = log_prob + N(0, NOISE^2): a good share of rows clips at 0.2 on both sides


class Case:
    """One call's inputs as host arrays.  Stored arrays (mask, actions, old_log_prob, advantages, returns) have store_rows rows; logits / values m rows."""

    def __init__(self, logits, mask, actions, old_log_prob, advantages, values, returns, index, store_rows):
        self.logits, self.mask, self.actions, self.old_log_prob, self.advantages = logits, mask, actions, old_log_prob, advantages
        self.values, self.returns, self.index, self.store_rows = values, returns, index, store_rows
        self.m = logits.shape[0]

    def gathered(self):
        """-> (ok [m], the stored arrays gathered to minibatch rows; rows with an index out of range hold placeholders)."""
        if self.index is None:
            return np.ones(self.m, bool), self.mask, self.actions, self.old_log_prob, self.advantages, self.returns
        ok = (self.index >= 0) & (self.index < self.store_rows)
        ix = np.where(ok, self.index, 0)
        mk = None if self.mask is None else np.where(ok[:, None], self.mask[ix], 0).astype(np.int8)
        return (ok, mk, np.where(ok, self.actions[ix], -1).astype(np.int32), np.where(ok, self.old_log_prob[ix], 0).astype(np.float32),
                np.where(ok, self.advantages[ix], 0).astype(np.float32), None if self.returns is None else np.where(ok, self.returns[ix], 0).astype(np.float32))

    def without(self, *, values=False, index=False):
        """The same case without the value term, or with the index resolved on the host (stored arrays gathered)."""
        c = Case(self.logits, self.mask, self.actions, self.old_log_prob, self.advantages, self.values, self.returns, self.index, self.store_rows)
        if index and c.index is not None:
            ok, mk, a, olp, adv, ret = self.gathered()
            assert ok.all()
            c.mask, c.actions, c.old_log_prob, c.advantages, c.returns, c.index, c.store_rows = mk, a, olp, adv, ret, None, c.m
        if values:
            c.values = c.returns = None
        return c


def synthetic(seed: int, m: int, sigma: float, masked: bool, *, index: str | None = None, hand_made: bool = True, bf16: bool = False, mask=None,
              store_rows: int | None = None) -> Case:
    """The shared generator: logits and masks as head_ref.synthetic, actions drawn by head_ref.Reference (so valid), old_log_prob = the reference's
    log-prob + N(0, NOISE^2), advantages, values, returns N(0, 1); then (hand_made, m >= 16) rows 1..9 are overwritten with the hand-made kinds.
    index: None, "perm" (a permutation of m stored rows) or "repeat" (store_rows, by default 2 m, stored rows; indices drawn with repetition).
    mask: an int8 [>= store_rows, 60] array to use instead of the generated one (masks of records the product wrote)."""
    rng = np.random.default_rng(seed + 1000003)
    store_rows = m if index is None or index == "perm" else (store_rows or 2 * m)
    ix = None
    if index == "perm":
        ix = rng.permutation(m).astype(np.int32)
    elif index == "repeat":
        ix = rng.integers(0, store_rows, m).astype(np.int32)
        if m > 3:
            ix[m // 2] = ix[m // 2 - 1]
    # the rollout's side: one logits row, mask row, drawn action and log-prob per STORED row; the learner's logits are those of the rows it reads (so
    # rows that read the same stored row agree), and old_log_prob is off by the noise
    base, smask = head_ref.synthetic(seed, store_rows, sigma, masked and mask is None)
    if mask is not None:
        smask = np.ascontiguousarray(mask[:store_rows], np.int8).copy()
        assert smask.shape == (store_rows, ACTIONS)
    if bf16:
        base = head_ref.widen_bf16(head_ref.bf16_bits(base))
    r = head_ref.Reference(base, smask, seed=seed, index0=0, t=3)
    actions = np.where(r.degenerate, 0, r.action).astype(np.int32)
    old_lp = (np.where(r.degenerate, 0.0, r.log_prob(actions)) + rng.standard_normal(store_rows) * NOISE).astype(np.float32)
    src = np.arange(m) if ix is None else ix.astype(np.int64)
    logits = base[src].copy()
    adv = rng.standard_normal(store_rows).astype(np.float32)
    ret = rng.standard_normal(store_rows).astype(np.float32)
    values = rng.standard_normal(m).astype(np.float32)
    c = Case(logits, smask, actions, old_lp, adv, values, ret, ix, store_rows)
    if hand_made and m >= 16:
        s = src
        if smask is not None:
            a1 = c.actions[s[1]]
            smask[s[1], a1] = 0                      # 1: masked action
            smask[s[4]] = 0                          # 4: degenerate mask
            one = int(np.argmax(logits[9]))
            smask[s[9]] = 0; smask[s[9], one] = 1    # 9: a single valid action
            c.actions[s[9]] = one
            c.old_log_prob[s[9]] = 0.05              #    (its log-prob is exactly 0)
        else:
            logits[4, 17] = np.nan                   # 4: degenerate without a mask
        c.actions[s[2]] = -1                         # 2, 3: action -1 and 60
        c.actions[s[3]] = 60
        c.old_log_prob[s[5]] = np.inf                # 5: a non-finite old_log_prob
        c.returns[s[6]] = -np.inf                    # 6: a non-finite return (excluded only with the value term)
        c.advantages[s[7]] = 0.0                     # 7: adv == 0
        if ix is not None:
            ix[8] = store_rows                       # 8: index out of range
            ix[10] = -1
    return c


def add_nan_advantage(c: Case, row: int = 11) -> Case:
    """A NaN advantage: without normalisation one excluded row; with it the statistics are NaN and every row is excluded."""
    src = row if c.index is None else int(c.index[row])
    c.advantages = c.advantages.copy()
    c.advantages[src] = np.nan
    return c


def _adv_stats(adv, ok, normalize):
    """float64 mean and unbiased std of the n advantages whose row has an index in range; apply = normalize and n > 1."""
    x = adv.astype(np.float64)[ok]
    n = x.size
    apply = bool(normalize) and n > 1
    with np.errstate(all="ignore"):
        mean = float(x.mean()) if n else 0.0
        std = float(x.std(ddof=1)) if n > 1 else 0.0
    return apply, mean, std


class ClosedForm:
    """The contract's formulas in numpy float64."""

    def __init__(self, c: Case, clip: float, ent_coef: float, vf_coef: float, normalize: bool, use_values: bool = True):
        self.c, self.m = c, c.m
        m = c.m
        self.clip32, self.ent, self.vf = np.float32(clip), float(np.float32(ent_coef)), float(np.float32(vf_coef))
        clipf = float(self.clip32)
        self.lo, self.hi = float(np.float32(1.0) - self.clip32), float(np.float32(1.0) + self.clip32)
        ok, mk, a, olp, adv, ret = c.gathered()
        self.src_ok, self.actions = ok, a
        self.has_v = use_values and c.values is not None
        self.head = r = head_ref.Reference(c.logits, mk)
        deg = r.degenerate | ~ok
        inr = (a >= 0) & (a < ACTIONS)
        ac = np.where(inr, a, 0)
        rows = np.arange(m)
        hidden = inr & ~r.valid[rows, ac]
        self.apply, mean, std = _adv_stats(adv, ok, normalize)
        self.adv_mean, self.adv_std = (mean, std if self.apply else 0.0) if normalize else (0.0, 0.0)
        adv64 = adv.astype(np.float64)
        with np.errstate(all="ignore"):
            advn = (adv64 - mean) / (std + float(np.float32(1e-8))) if self.apply else adv64
            self.dadv = 2.0 ** -22 * (np.abs(advn) + (np.abs(adv64) + abs(mean)) / std) if self.apply else np.zeros(m)
            bad = ~np.isfinite(olp.astype(np.float64)) | ~np.isfinite(adv64) | ~np.isfinite(advn)
            if self.has_v:
                bad |= ~np.isfinite(c.values.astype(np.float64)) | ~np.isfinite(ret.astype(np.float64))
            self.excluded = ex = deg | ~inr | hidden | bad
            live = ~ex
            self.dadv = np.where(live, self.dadv, 0.0)
            self.log_prob = lp = r.log_prob(a)
            lr = np.where(live, lp - olp, 0.0)
            self.ratio = ratio = np.exp(lr)
            rc = np.minimum(np.maximum(ratio, self.lo), self.hi)
            advn = np.where(live, advn, 0.0)
            self.advn = advn
            s1, s2 = advn * ratio, advn * rc
            self.s1, self.s2, self.rc = s1, s2, rc
            self.policy = np.where(live, -np.minimum(s1, s2), 0.0)
            inside = (self.lo <= ratio) & (ratio <= self.hi)
            self.g_pass = np.where(live, advn * ratio, 0.0)
            self.g = np.where(live & (inside | (s1 < s2)), self.g_pass, 0.0)
            self.kl = np.where(live, (ratio - 1.0) - lr, 0.0)
            self.clipped = live & (np.abs(ratio - 1.0) > clipf)
            near = (np.abs(ratio - self.lo) <= MARGIN * self.lo) | (np.abs(ratio - self.hi) <= MARGIN * self.hi)
            sign_safe = (s1 == s2) | (~inside & (np.abs(advn) > self.dadv))
            self.decidable = ex | (~near & sign_safe)
            dv = np.where(live, c.values.astype(np.float64) - ret, 0.0) if self.has_v else np.zeros(m)
            self.dv = dv
            self.value = dv * dv
            self.dvalues = self.vf * 2.0 * dv / m
            S = np.where(deg, 1.0, r.S)
            self.p = p = r.e / S[:, None]
            pos = r.e > 0
            self.logp = logp = np.where(pos, np.where(pos, r.d, 0.0) - r.logS[:, None], 0.0)
            self.H = H = np.where(live, r.entropy, 0.0)
            hit = (np.arange(ACTIONS)[None, :] == ac[:, None]).astype(np.float64)
            self.hit = hit
            self.ent_part = np.where(live[:, None], self.ent * p * (logp + H[:, None]), 0.0)
            self.dlogits = self.grad_with(self.g)
            self.dlogits_other = self.grad_with(np.where(self.g == 0.0, self.g_pass, 0.0))   # the other branch, for undecidable rows
            d_a = np.abs(np.where(live, r.d[rows, ac], 0.0))
            self.eps = eps = 4.0 * (2.0 ** -17 + 2.0 ** -22 * d_a)
            self.G = lambda g: np.abs(g) + self.dadv * ratio
            self.ent_bound = self.ent * p * (1.0 + np.abs(logp) + np.abs(H)[:, None])
        dm = float(m)
        n_ex = int(ex.sum())
        self.stats = {
            "policy_loss": self.policy.sum() / dm, "value_loss": self.value.sum() / dm, "entropy_loss": -H.sum() / dm, "approx_kl": self.kl.sum() / dm,
            "clip_fraction": self.clipped.sum() / dm, "adv_mean": self.adv_mean, "adv_std": self.adv_std, "excluded": float(n_ex), "m": dm}
        self.stats["loss"] = self.stats["policy_loss"] + self.ent * self.stats["entropy_loss"] + self.vf * self.stats["value_loss"]
        und = ~self.decidable
        live_f = live.astype(np.float64)
        sb = {"policy_loss": (eps * np.maximum(np.abs(s1), np.abs(s2)) + self.dadv * np.maximum(ratio, rc)) * live_f, "approx_kl": eps * (ratio + 1.0) * live_f,
              "entropy_loss": 2.0 ** -17 * (1.0 + np.where(live, r.spread, 0.0)) * live_f, "value_loss": 2.0 ** -21 * self.value, "clip_fraction": und.astype(np.float64)}
        self.stat_bounds = {k: v.sum() / dm + 2.0 ** -23 * abs(self.stats[k]) for k, v in sb.items()}
        self.stat_bounds["loss"] = (self.stat_bounds["policy_loss"] + abs(self.ent) * self.stat_bounds["entropy_loss"] + abs(self.vf) * self.stat_bounds["value_loss"]
                                    + 2.0 ** -23 * abs(self.stats["loss"]))
        self.stat_bounds["adv_mean"] = 2.0 ** -23 * abs(self.adv_mean) + 1e-30
        self.stat_bounds["adv_std"] = 2.0 ** -23 * abs(self.adv_std) + 1e-30
        self.stat_bounds["excluded"] = 0.0
        self.stat_bounds["m"] = 0.0

    def grad_with(self, g):
        live = ~self.excluded
        pol = -g[:, None] * (self.hit - self.p)
        out = np.where(live[:, None] & self.head.valid, (pol + self.ent_part) / float(self.m), 0.0)
        return out

    def grad_bound(self, g, got32):
        """The bound of every gradient element for branch gradient g, with one float32 ulp of the result."""
        ulp = np.spacing(np.abs(np.asarray(got32, np.float32)).astype(np.float32)).astype(np.float64)
        return self.eps[:, None] * (self.G(g)[:, None] * (self.hit + self.p) + self.ent_bound) / float(self.m) + ulp

    # ---- the assertions, shared by the host and the GPU test; returns the largest observed share of each bound ----
    def check(self, got_dlogits, got_dvalues, got_lp, got_en, got_stats, what: str, cap: bool = True) -> dict:
        m = self.m
        und = ~self.decidable
        assert not cap or und.sum() <= UNDECIDABLE_CAP * m, f"{what}: {und.sum()} of {m} rows undecidable: the test set is unfit"
        shares = {}
        gd = np.asarray(got_dlogits, np.float32)
        assert gd.shape == (m, ACTIONS), what
        # log_prob / entropy: head_ref's bounds; index-out-of-range rows are quiet NaN
        lp, en = np.asarray(got_lp, np.float32), np.asarray(got_en, np.float32)
        out = ~self.src_ok
        assert (lp.view(np.uint32)[out] == head_ref.QNAN_BITS).all() and (en.view(np.uint32)[out] == head_ref.QNAN_BITS).all(), f"{what}: out-of-range rows are NaN"
        en = np.where(out, self.head.entropy.astype(np.float32), en)   # (the head reference does not know about the index)
        shares["log_prob"], shares["entropy"] = self.head.check_stats(self.actions, lp, en, what)
        # excluded rows: +0.0 everywhere
        ex = self.excluded
        assert (gd[ex].view(np.uint32) == 0).all(), f"{what}: an excluded row's gradient must be +0.0"
        assert (gd.view(np.uint32)[~self.head.valid & self.src_ok[:, None]] == 0).all(), f"{what}: an invalid action's gradient must be +0.0"
        assert np.isfinite(gd).all(), f"{what}: non-finite gradient"
        g64 = gd.astype(np.float64)
        b_ref = self.grad_bound(self.g, gd)
        e_ref = np.abs(g64 - self.dlogits) / b_ref
        b_alt = self.grad_bound(np.where(self.g == 0.0, self.g_pass, 0.0), gd)
        e_alt = np.abs(g64 - self.dlogits_other) / b_alt
        row_ref, row_alt = e_ref.max(axis=1), e_alt.max(axis=1)
        bad_dec = np.flatnonzero(self.decidable & (row_ref > 1.0))
        assert bad_dec.size == 0, f"{what}: gradient of decidable row {bad_dec[0]} off by {row_ref[bad_dec[0]]:.3f} of its bound ({bad_dec.size} rows)"
        bad_und = np.flatnonzero(und & (np.minimum(row_ref, row_alt) > 1.0))
        assert bad_und.size == 0, f"{what}: gradient of undecidable row {bad_und[0]} matches neither branch"
        shares["dlogits"] = float(row_ref[self.decidable].max()) if self.decidable.any() else 0.0
        if self.has_v:
            dvg = np.asarray(got_dvalues, np.float32)
            assert (dvg.view(np.uint32)[ex] == 0).all(), f"{what}: an excluded row's dvalue must be +0.0"
            b = 2.0 ** -22 * np.abs(self.dvalues) + 1e-45
            shares["dvalues"] = float((np.abs(dvg.astype(np.float64) - self.dvalues)[~ex] / b[~ex]).max()) if (~ex).any() else 0.0
            assert shares["dvalues"] <= 1.0, f"{what}: dvalues off by {shares['dvalues']:.3f} of its bound"
        st = np.asarray(got_stats, np.float32)
        assert st.shape == (len(STATS),)
        for k, name in enumerate(STATS):
            want, bound = self.stats[name], self.stat_bounds[name]
            if np.isnan(want):
                assert np.isnan(st[k]), f"{what}: {name} must be NaN"
                continue
            err = abs(float(st[k]) - want)
            if bound == 0.0:
                assert err == 0.0, f"{what}: {name} = {st[k]}, want {want}"
            else:
                shares[name] = err / bound
                assert err <= bound, f"{what}: {name} = {st[k]!r}, want {want!r}: off by {err / bound:.3f} of its bound"
        return shares


def torch_statement(c: Case, clip: float, ent_coef: float, vf_coef: float, normalize: bool, included, use_values: bool = True, params=None):
    """SB3's PPO.train loss, literally, in float64 on the CPU over the rows `included` (bool [m]; the others add nothing and the divisor stays m), with
    autograd: -> (dict of scalars, dlogits [m, 60], dvalues [m] or None).  The coefficients are taken at their float32 values, as the C ABI receives
    them.  params: optional (logits tensor, values tensor) that already require grad (the MLP test), instead of leaves made here."""
    import torch
    import torch.nn.functional as F
    m = c.m
    ok, mk, a, olp, adv, ret = c.gathered()
    clip64, ent64, vf64 = float(np.float32(clip)), float(np.float32(ent_coef)), float(np.float32(vf_coef))
    lo, hi = float(np.float32(1.0) - np.float32(clip)), float(np.float32(1.0) + np.float32(clip))
    inc = torch.from_numpy(np.asarray(included, bool))
    if params is None:
        logits = torch.from_numpy(np.nan_to_num(c.logits.astype(np.float64), nan=0.0)).requires_grad_(True)
        values = torch.from_numpy(c.values.astype(np.float64)).requires_grad_(True) if use_values and c.values is not None else None
    else:
        logits, values = params
    valid = torch.ones((m, ACTIONS), dtype=torch.bool) if mk is None else torch.from_numpy(mk != 0)
    valid = valid | ~inc[:, None]   # (rows that take no part: keep the softmax finite; they are dropped below)
    advantages = torch.from_numpy(adv.astype(np.float64))
    apply, mean, std = _adv_stats(adv, ok, normalize)
    if apply:   # SB3: (advantages - advantages.mean()) / (advantages.std() + 1e-8) when len(advantages) > 1, over the call's advantages
        sel = advantages[torch.from_numpy(ok)]
        advantages = (advantages - sel.mean()) / (sel.std() + float(np.float32(1e-8)))
    actions = torch.from_numpy(np.where(included, a, 0).astype(np.int64))
    old_log_prob = torch.from_numpy(np.where(included, olp, 0.0).astype(np.float64))
    advantages = torch.where(inc, advantages, torch.zeros_like(advantages))
    masked_logits = logits.masked_fill(~valid, float("-inf"))
    logp_all = F.log_softmax(masked_logits, dim=-1)
    log_prob = logp_all.gather(1, actions[:, None])[:, 0]
    p_all = logp_all.exp()
    entropy = -(p_all * torch.where(p_all > 0, logp_all, torch.zeros_like(logp_all))).sum(-1)
    ratio = torch.exp(log_prob - old_log_prob)
    policy_loss_1 = advantages * ratio
    policy_loss_2 = advantages * torch.clamp(ratio, lo, hi)
    w = inc.to(torch.float64)
    policy_loss = (-torch.min(policy_loss_1, policy_loss_2) * w).sum() / m
    clip_fraction = ((torch.abs(ratio - 1) > clip64).to(torch.float64) * w).sum() / m
    entropy_loss = -(entropy * w).sum() / m
    if values is not None:
        returns = torch.from_numpy(np.where(included, ret, 0.0).astype(np.float64))
        value_loss = (F.mse_loss(returns, torch.where(inc, values, torch.zeros_like(values)), reduction="none")).sum() / m
    else:
        value_loss = torch.zeros((), dtype=torch.float64)
    loss = policy_loss + ent64 * entropy_loss + vf64 * value_loss
    log_ratio = log_prob - old_log_prob
    approx_kl = (((torch.exp(log_ratio) - 1) - log_ratio) * w).sum().item() / m
    scal = {"loss": loss.item(), "policy_loss": policy_loss.item(), "value_loss": value_loss.item(), "entropy_loss": entropy_loss.item(),
            "approx_kl": approx_kl, "clip_fraction": clip_fraction.item()}
    if params is not None:
        return scal, loss
    loss.backward()
    return scal, logits.grad.numpy(), None if values is None else values.grad.numpy()


def mlp_gradient_bounds(B, D, W1, W2, x, slack=2.0 ** -14, forward_abs=False):
    """Carries the output-gradient bounds of a two-layer MLP  x -> tanh(x W1^T + b1) -> h W2^T + b2  (60 logits + 1 value) into the bounds of its parameter
    gradients.  B float64 [m, 61]: the bound of every dlogits / dvalues element (ClosedForm.grad_bound and 2**-22 |dvalues| + 1e-45); D [m, 61]: |dout|,
    the reference's absolute output gradient; W1: the float64 twin's (W1, b1), W2 its second weight matrix; x float64 [m, cols].
    The bound goes through the absolute Jacobian (|h|, |W2|, |1 - h^2|, |x|); `slack` of the sum of absolute terms of each gradient element pays for the
    float32 passes of the network itself (the forward activations carry at most (153 + 64) * 2**-24 < 2**-16, the backward dots over 256 rows 2**-16, tanh
    and its derivative a few ulp: below 2**-14 together.  tests/test_ppo_iteration.py calls this with 1000-row minibatches, where a strictly sequential
    float32 dot could reach 1000 * 2**-24 = 2**-14.03 on its own; a rounding error that grows like sqrt(m) stays near 2**-19, and the test prints its share).
    forward_abs: `slack` takes the float32 error of h to be RELATIVE to |h|.  It is not: the pre-activation z = x W1^T + b1 carries an ABSOLUTE error of up to
    EZ = (cols + 1) * 2**-24 * (|x| |W1|^T + |b1|), and tanh' <= 1 hands it to h whatever |h| is.  Where a logit column has a gradient on one or two rows
    and |h| there is 1e-5, slack * |dout| |h| allows nothing while the error is |dout| EZ (a float32 network on the CPU fed the exactly rounded closed-form
    gradient misses the relative bound by two orders of magnitude on such an element).  With forward_abs=True the bounds also hold |dout|^T EZ (W2.grad)
    and, through 1 - h^2 (off by at most 2 |h| EZ), (|dout| |W2| * 2 |h| EZ)^T |x| (W1.grad) and its column sums (b1.grad).  The default is the bound as
    test_mlp_takes_one_sgd_step_through_ppo_loss has always used it, on features squashed into (-1, 1).
    -> [bound of W1.grad, b1.grad, W2.grad, b2.grad]"""
    W1, b1 = W1
    h = np.tanh(x @ W1.T + b1)
    bW2 = B.T @ np.abs(h) + slack * (D.T @ np.abs(h))
    bb2 = B.sum(0) + slack * D.sum(0)
    Bh, Dh = (B @ np.abs(W2)) * np.abs(1 - h * h), (D @ np.abs(W2)) * np.abs(1 - h * h)
    bW1 = Bh.T @ np.abs(x) + slack * (Dh.T @ np.abs(x))
    bb1 = Bh.sum(0) + slack * Dh.sum(0)
    if forward_abs:
        EZ = (x.shape[1] + 1) * 2.0 ** -24 * (np.abs(x) @ np.abs(W1).T + np.abs(b1))
        Eh = (D @ np.abs(W2)) * 2.0 * np.abs(h) * EZ
        bW2 = bW2 + D.T @ EZ
        bW1 = bW1 + Eh.T @ np.abs(x)
        bb1 = bb1 + Eh.sum(0)
    return [bW1, bb1, bW2, bb2]


def check_mlp_gradients(grads, want, bounds, what: str = "") -> float:
    """The parameter gradients [W1, b1, W2, b2] (float64 copies of the device's) against the twin's within `bounds`; an element whose bound is 0 must be
    exact.  Returns the largest share of a bound."""
    worst = 0.0
    for name, g, w, b in zip(("W1", "b1", "W2", "b2"), grads, want, bounds):
        err, live = np.abs(g - w), b > 0.0
        assert (err[~live] == 0.0).all(), f"{what}{name}: an element whose bound is 0 (a feature column that is 0 on every row) must be exact"
        share = float((err[live] / b[live]).max())
        worst = max(worst, share)
        assert share <= 1.0, f"{what}{name}: parameter gradient off by {share:.3f} of its propagated bound"
    return worst
