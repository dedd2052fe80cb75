"""The reference of bg_bc_loss (csrc/bg_bc.h): the weighted cross-entropy of stored actions over the masked categorical head, its accuracy and its
gradient, in float64, stated twice and never through the code under test:
  * `torch_statement`: the composite written literally in torch on the CPU (masked_fill with -inf, log_softmax, gather, the weighted mean, the entropy
    with 0 * log 0 = 0), differentiated by torch's autograd;
  * `ClosedForm`: the formulas of the contract in numpy, on the quantities of tests/head_ref.py.
tests/test_bc_loss_host.py holds the two to each other, then the header compiled with g++ to the closed form; tests/test_bc_loss.py does the same for
the kernel.

The kernel computes in float32 and is held by BOUNDS, derived the way tests/ppo_ref.py derives its own.  EPS_ij = 2**-17 + 2**-22 |d_j| is head_ref's
bound of a float32 log-probability log p_j = d_j - logS (row i); it also bounds the RELATIVE error of p_j = e_j / S as the kernel takes it: d_j rounds
once (2**-24 |d_j|), expf is good to a few ulp (2**-22), S is a sequential float32 sum of 60 positive terms (at most 59 * 2**-24 < 2**-18.1 relative)
and the division rounds once -- together below 2**-17.6 + 2**-24 |d_j|.
  * log_prob / entropy: head_ref's bounds (check_stats);
  * a gradient element  ((ent_coef * p_j) * (log p_j + H) - (1[j == a] - p_j)) * w / Wf:  the cross-entropy part carries the error of p_j, EPS_ij p_j;
    the entropy part carries the relative error of p_j on the whole bracket, the absolute errors of log p_j (EPS_ij) and of H (head_ref's
    2**-17 (1 + spread_i)):
        B_ij = (w_i / W) * (EPS_ij p_j + ent_coef p_j (EPS_ij (1 + |log p_j| + |H_i|) + 2**-17 (1 + spread_i)))
               + 2**-21 |dlogits_ij| + one float32 ulp of the result + 2**-126 w_i / W
    the 2**-21 pays for the seven roundings between p_j and the element (two products and the sum of the entropy part, the difference, the product
    with w, float(W), the division: 7 * 2**-24 < 2**-21), the last term for an e_j below the smallest normal float32, which may lose bits or be
    flushed.  There is NO branch in this loss (no clip, no min), so no row is undecidable and no extra margin is taken;
  * nll_loss: the weighted mean of the rows' log-prob bounds; entropy_loss: that of head_ref's entropy bounds; loss: their combination; each plus
    2**-23 of the value for the final roundings (the float64 sums themselves are exact to 2**-53 m);
  * accuracy, weight_sum: `hit` is an exact float32 comparison and w * hit, w are exact in float64, so only the rounding to float32 is left: 2**-23 of
    the value;  excluded and m: exact.
"""
from __future__ import annotations

import numpy as np

from tests import head_ref

ACTIONS = 60
STATS = ("loss", "nll_loss", "entropy_loss", "accuracy", "weight_sum", "excluded", "m")


class Case:
    """One call's inputs as host arrays.  Stored arrays (mask, actions, weights) have store_rows rows; logits m rows."""

    def __init__(self, logits, mask, actions, weights, index, store_rows):
        self.logits, self.mask, self.actions, self.weights, self.index, self.store_rows = logits, mask, actions, weights, index, store_rows
        self.m = logits.shape[0]

    def gathered(self):
        """-> (ok [m], mask, actions, weights gathered to minibatch rows; rows with an index out of range hold placeholders; weights float32, 1 without)."""
        ones = np.ones(self.store_rows, np.float32) if self.weights is None else self.weights
        if self.index is None:
            return np.ones(self.m, bool), self.mask, self.actions, ones
        ok = (self.index >= 0) & (self.index < self.store_rows)
        ix = np.where(ok, self.index, 0)
        mk = None if self.mask is None else np.where(ok[:, None], self.mask[ix], 0).astype(np.int8)
        return ok, mk, np.where(ok, self.actions[ix], -1).astype(np.int32), np.where(ok, ones[ix], 0).astype(np.float32)


def synthetic(seed: int, m: int, sigma: float, masked: bool, *, index: str | None = None, weights: str | None = None, hand_made: bool = True,
              bf16: bool = False, mask=None, store_rows: int | None = None) -> Case:
    """The shared generator: logits and masks as head_ref.synthetic; the demonstrated action is the reference's argmax on two rows of three (so the
    accuracy is neither 0 nor 1) and its sampled action on the others.  index: None, "perm" or "repeat" (as ppo_ref.synthetic; rows 8 and 10 then get
    indices out of range).  weights: None, "random" (exponential weights with zeros and, hand_made, one negative and one NaN), "filter" (0 / 1) or
    "zero" (all zero).  hand_made (m >= 16): row 1 the stored action masked (masked sets) / a NaN logit (unmasked), 2 and 3 actions -1 and 60, 4 every
    action masked / a +inf logit, 5 a tie of the maximum whose FIRST index is demonstrated, 6 the same tie with its second index demonstrated, 7 a
    single valid action, 9 a valid -inf logit at the demonstrated action."""
    rng = np.random.default_rng(seed + 2000003)
    store_rows = m if index is None or index == "perm" else (store_rows or 2 * m)
    ix = None
    if index == "perm":
        ix = rng.permutation(m).astype(np.int32)
    elif index == "repeat":
        ix = rng.integers(0, store_rows, m).astype(np.int32)
        if m > 3:
            ix[m // 2] = ix[m // 2 - 1]
    base, smask = head_ref.synthetic(seed, store_rows, sigma, masked and mask is None)
    if mask is not None:
        smask = np.ascontiguousarray(mask[:store_rows], np.int8).copy()
        assert smask.shape == (store_rows, ACTIONS)
    if bf16:
        base = head_ref.widen_bf16(head_ref.bf16_bits(base))
    r = head_ref.Reference(base, smask, seed=seed, index0=0, t=5)
    greedy = rng.random(store_rows) < 2.0 / 3.0
    actions = np.where(r.degenerate, 0, np.where(greedy, r.mode, r.action)).astype(np.int32)
    src = np.arange(m) if ix is None else ix.astype(np.int64)
    logits = base[src].copy()
    w = None
    if weights == "random":
        w = rng.exponential(1.0, store_rows).astype(np.float32)
        w[rng.random(store_rows) < 0.3] = 0.0
    elif weights == "filter":
        w = (rng.random(store_rows) < 0.4).astype(np.float32)
    elif weights == "zero":
        w = np.zeros(store_rows, np.float32)
    c = Case(logits, smask, actions, w, ix, store_rows)
    if hand_made and m >= 16:
        s = src
        taken = set()

        def fresh(i):   # (a repeated index may name a stored row twice: hand-made rows must not overwrite each other)
            assert s[i] not in taken or ix is not None
            taken.add(int(s[i]))
            return int(s[i])
        if smask is not None:
            smask[fresh(1), c.actions[s[1]]] = 0      # 1: the stored action masked
            smask[fresh(4)] = 0                       # 4: every action masked
            one = int(np.argmax(logits[7]))
            smask[fresh(7)] = 0; smask[s[7], one] = 1  # 7: a single valid action (log_prob and H exactly 0)
            c.actions[s[7]] = one
        else:
            logits[1, 17] = np.nan
            logits[4, 3] = np.inf
        c.actions[fresh(2)] = -1
        c.actions[fresh(3)] = 60
        for row, which in ((5, 0), (6, 1)):           # 5, 6: ties of the maximum
            j0, j1 = 11, 40
            if smask is not None:
                smask[fresh(row), [j0, j1]] = 1
            else:
                fresh(row)
            top = np.float32(np.abs(logits[row]).max() + 1.0)
            if bf16:   # (the tie stays representable, and above every other logit: the rounding moves it by less than 2**-8 of itself)
                top = head_ref.widen_bf16(head_ref.bf16_bits(np.array([top], np.float32)))[0]
            logits[row, j0] = logits[row, j1] = top
            c.actions[s[row]] = (j0, j1)[which]
        j9 = 23                                       # 9: a valid -inf logit at the demonstrated action
        if smask is not None:
            smask[fresh(9), j9] = 1
        else:
            fresh(9)
        logits[9, j9] = -np.inf
        c.actions[s[9]] = j9
        if ix is not None:
            ix[8] = store_rows
            ix[10] = -1
        if weights == "random":
            w[s[12]] = -0.5
            w[s[13]] = np.nan
            w[s[14]] = 0.0
            w[s[15]] = 2.5
            w[s[5]], w[s[6]] = 1.0, 0.75                # (the ties take part)
    return c


class ClosedForm:
    """The contract's formulas in numpy float64."""

    def __init__(self, c: Case, ent_coef: float):
        self.c, self.m = c, c.m
        m = c.m
        self.ent = float(np.float32(ent_coef))
        ok, mk, a, w32 = c.gathered()
        self.src_ok, self.actions = ok, a
        self.head = r = head_ref.Reference(c.logits, mk)
        deg = r.degenerate | ~ok
        inr = (a >= 0) & (a < ACTIONS)
        ac = np.where(inr, a, 0)
        rows = np.arange(m)
        hidden = inr & ~r.valid[rows, ac]
        w = w32.astype(np.float64)
        with np.errstate(all="ignore"):
            w_ok = ok & np.isfinite(w) & (w >= 0)
            self.W = W = float(np.where(w_ok, w, 0.0).sum())
            self.log_prob = lp = r.log_prob(a)
            self.excluded = ex = deg | ~inr | hidden | ~np.isfinite(lp) | ~w_ok
            live = ~ex
            wl = np.where(live, w, 0.0)
            self.w = wl
            self.nll = np.where(live, -lp, 0.0)
            self.H = H = np.where(live, r.entropy, 0.0)
            self.hit_row = np.where(live, (r.mode == a), False)
            S = np.where(deg, 1.0, r.S)
            self.p = p = r.e / S[:, None]
            pos = r.e > 0
            self.logp = logp = np.where(pos, np.where(pos, r.d, 0.0) - r.logS[:, None], 0.0)
            hit = (np.arange(ACTIONS)[None, :] == ac[:, None]).astype(np.float64)
            scale = (wl / W if W > 0 else np.zeros(m))[:, None]
            elem = self.ent * p * (logp + H[:, None]) - (hit - p)
            self.dlogits = np.where(live[:, None] & r.valid, elem * scale, 0.0)
            eps = 2.0 ** -17 + 2.0 ** -22 * np.abs(np.where(pos, r.d, 0.0))
            spread = np.where(live, r.spread, 0.0)
            self.bound = np.where(live[:, None] & r.valid, scale * (eps * p + self.ent * p * (eps * (1.0 + np.abs(logp) + np.abs(H)[:, None])
                                                                                              + 2.0 ** -17 * (1.0 + spread)[:, None]) + 2.0 ** -126), 0.0) \
                + 2.0 ** -21 * np.abs(self.dlogits)
            d_a = np.abs(np.where(live, r.d[rows, ac], 0.0))
            lp_bound = 2.0 ** -17 + 2.0 ** -22 * d_a
            en_bound = 2.0 ** -17 * (1.0 + spread)
        z = W == 0.0
        dv = 1.0 if z else W
        self.stats = {"nll_loss": 0.0 if z else (wl * self.nll).sum() / dv, "entropy_loss": 0.0 if z else -(wl * H).sum() / dv,
                      "accuracy": 0.0 if z else (wl * self.hit_row).sum() / dv, "weight_sum": W, "excluded": float(ex.sum()), "m": float(m)}
        self.stats["loss"] = self.stats["nll_loss"] + self.ent * self.stats["entropy_loss"]
        sb = {"nll_loss": 0.0 if z else (wl * lp_bound).sum() / dv, "entropy_loss": 0.0 if z else (wl * en_bound).sum() / dv}
        self.stat_bounds = {k: v + 2.0 ** -23 * abs(self.stats[k]) for k, v in sb.items()}
        self.stat_bounds["loss"] = self.stat_bounds["nll_loss"] + abs(self.ent) * self.stat_bounds["entropy_loss"] + 2.0 ** -23 * abs(self.stats["loss"])
        self.stat_bounds["accuracy"] = 2.0 ** -23 * abs(self.stats["accuracy"])
        self.stat_bounds["weight_sum"] = 2.0 ** -23 * abs(W)
        self.stat_bounds["excluded"] = 0.0
        self.stat_bounds["m"] = 0.0

    def grad_bound(self, got32):
        ulp = np.spacing(np.abs(np.asarray(got32, np.float32)).astype(np.float32)).astype(np.float64)
        return self.bound + ulp

    # ---- the assertions, shared by the host and the GPU test; returns the largest observed share of each bound ----
    def check(self, got_dlogits, got_lp, got_en, got_stats, what: str) -> dict:
        m = self.m
        shares = {}
        gd = np.asarray(got_dlogits, np.float32)
        assert gd.shape == (m, ACTIONS), what
        lp, en = np.asarray(got_lp, np.float32), np.asarray(got_en, np.float32)
        out = ~self.src_ok
        assert (lp.view(np.uint32)[out] == head_ref.QNAN_BITS).all() and (en.view(np.uint32)[out] == head_ref.QNAN_BITS).all(), f"{what}: out-of-range rows are NaN"
        en = np.where(out, self.head.entropy.astype(np.float32), en)   # (the head reference does not know about the index)
        shares["log_prob"], shares["entropy"] = self.head.check_stats(self.actions, lp, en, what)
        ex = self.excluded
        assert (gd[ex].view(np.uint32) == 0).all(), f"{what}: an excluded row's gradient must be +0.0"
        assert (gd.view(np.uint32)[~self.head.valid & self.src_ok[:, None]] == 0).all(), f"{what}: an invalid action's gradient must be +0.0"
        assert np.isfinite(gd).all(), f"{what}: non-finite gradient"
        if self.W == 0.0:
            assert (gd.view(np.uint32) == 0).all(), f"{what}: W == 0 gives an all-+0.0 gradient"
        share = np.abs(gd.astype(np.float64) - self.dlogits) / self.grad_bound(gd)
        worst = np.unravel_index(np.argmax(share), share.shape)
        assert share[worst] <= 1.0, f"{what}: gradient element {worst} off by {share[worst]:.3f} of its bound (got {gd[worst]!r}, want {self.dlogits[worst]!r})"
        shares["dlogits"] = float(share.max())
        st = np.asarray(got_stats, np.float32)
        assert st.shape == (len(STATS),)
        for k, name in enumerate(STATS):
            want, bound = self.stats[name], self.stat_bounds[name]
            err = abs(float(st[k]) - want)
            if bound == 0.0:
                assert err == 0.0, f"{what}: {name} = {st[k]}, want {want}"
            else:
                shares[name] = err / bound
                assert err <= bound, f"{what}: {name} = {st[k]!r}, want {want!r}: off by {err / bound:.3f} of its bound"
        return shares


def torch_statement(c: Case, ent_coef: float, included, W: float, params=None):
    """The composite, literally, in float64 on the CPU over the rows `included` (bool [m]; the others add nothing) with the divisor W, with autograd:
    -> (dict of scalars, dlogits [m, 60]).  params: an optional logits tensor that already requires grad (the MLP test) -> (scalars, loss tensor)."""
    import torch
    import torch.nn.functional as F
    m = c.m
    ok, mk, a, w32 = c.gathered()
    ent64 = float(np.float32(ent_coef))
    inc = torch.from_numpy(np.asarray(included, bool))
    logits = torch.from_numpy(np.nan_to_num(c.logits.astype(np.float64), nan=0.0, posinf=0.0, neginf=-np.inf)).requires_grad_(True) if params is None else params
    valid = torch.ones((m, ACTIONS), dtype=torch.bool) if mk is None else torch.from_numpy(mk != 0)
    valid = valid | ~inc[:, None]   # (rows that take no part: keep the softmax finite; they are dropped below)
    actions = torch.from_numpy(np.where(included, a, 0).astype(np.int64))
    wt = torch.from_numpy(np.where(included, w32.astype(np.float64), 0.0))
    masked_logits = logits.masked_fill(~valid, float("-inf"))
    logp_all = F.log_softmax(masked_logits, dim=-1)
    log_prob = logp_all.gather(1, actions[:, None])[:, 0]
    log_prob = torch.where(inc, log_prob, torch.zeros_like(log_prob))
    p_all = logp_all.exp()
    entropy = -(p_all * torch.where(p_all > 0, logp_all, torch.zeros_like(logp_all))).sum(-1)
    eq = masked_logits.detach() == masked_logits.detach().max(-1, keepdim=True).values
    first = torch.where(eq, torch.arange(ACTIONS)[None, :], torch.full((1, 1), ACTIONS)).min(-1).values   # the first maximum among the valid logits
    div = W if W > 0 else 1.0
    nll_loss = (-(log_prob) * wt).sum() / div
    entropy_loss = -(entropy * wt).sum() / div
    accuracy = ((first == actions).to(torch.float64) * wt).sum() / div
    loss = nll_loss + ent64 * entropy_loss
    scal = {"loss": loss.item(), "nll_loss": nll_loss.item(), "entropy_loss": entropy_loss.item(), "accuracy": accuracy.item()}
    if params is not None:
        return scal, loss
    if loss.requires_grad and W > 0 and bool(inc.any()):
        loss.backward()
        return scal, logits.grad.numpy()
    return scal, np.zeros((m, ACTIONS))
