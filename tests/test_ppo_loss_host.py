"""bg_ppo_loss on the CPU (no GPU).  First the reference is held to itself: tests/ppo_ref.py's two statements -- SB3's loss written literally in torch
float64 under autograd, and the contract's closed form in numpy float64 -- agree, ties and boundary rows included, and its test sets are fit.  Then
csrc/bg_ppo.h -- the per-row arithmetic the kernel runs and the serial twin of its launch sequence -- is compiled with g++ (-O1 -ffp-contract=off
-DBG_PPO_HOST) into a small shared object and held to the closed form by the bounds derived in ppo_ref: 16 384-row sets for sigma in {0.1, 1, 3, 10},
masked and unmasked, with and without normalisation, value term and index; the hand-made rows; log_prob / entropy bit-equal to the host bg_head_row.
Also: the header's declaration, the exports, build.DEPS, and the argument checks of the Python wrapper.

Largest observed shares of the bounds with g++ and glibc's expf / logf: dlogits 0.38, dvalues 0.25, policy_loss 0.0005, approx_kl 0.00002, entropy_loss
0.02, value_loss 0.10, loss 0.002, adv_mean 0.45, adv_std 0.40, log_prob 0.11, entropy 0.08; undecidable rows at most 0.06 % of a set.
At m = 16 449 and 65 793 (the twin's folds with per > 1): dlogits 0.051, dvalues 0.50, policy_loss 0.0005, approx_kl 0.00001, entropy_loss 0.004,
value_loss 0.079, loss 0.0013, adv_mean 0.43, adv_std 0.32, log_prob 0.094, entropy 0.048, clip_fraction 0.063; undecidable rows at most 0.033 %."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import head_ref, ppo_ref
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")
M = 16384

_PROGRAM = r"""
#define BG_PPO_HOST
#include <stdio.h>
#include <stdlib.h>
#include "balatro_mi355x.h"
#include "bg_ppo.h"
extern "C" void ppo_host(const void* logits, int bf16, uint64_t lstride, const int8_t* mask, uint64_t mstride, const int32_t* actions, const float* old_lp,
                         const float* adv, const float* values, const float* returns, const int32_t* index, int64_t store_rows, int64_t m, float clip,
                         float ent_coef, float vf_coef, uint32_t flags, int keep, void* dlogits, uint64_t dstride, float* dvalues, float* log_prob,
                         float* entropy, float* stats) {
  BgPpoArgs A = {};
  A.logits = logits; A.lstride = lstride; A.mask = mask; A.mstride = mstride; A.actions = actions; A.old_lp = old_lp; A.adv = adv; A.values = values;
  A.returns = returns; A.index = index; A.store_rows = store_rows; A.m = m;
  A.c.clip = clip; A.c.lo = 1.0f - clip; A.c.hi = 1.0f + clip; A.c.ent_coef = ent_coef; A.c.vf_coef = vf_coef; A.c.fm = (float)m;
  A.normalize = flags & BG_PPO_NORMALIZE_ADV ? 1 : 0;
  A.dlogits = dlogits; A.dstride = dstride; A.dvalues = dvalues; A.log_prob = log_prob; A.entropy = entropy;
  bg_ppo_host(A, bf16 != 0, keep != 0, stats);
}
extern "C" void head_evaluate(const float* logits, const int8_t* mask, const int32_t* actions, int64_t m, float* log_prob, float* entropy) {
  for (int64_t i = 0; i < m; i++) {
    float P[BG_HEAD_ACTIONS];
    uint32_t k[BG_HEAD_ACTIONS / 4] = {};
    if (mask) memcpy(k, mask + i * BG_HEAD_ACTIONS, BG_HEAD_ACTIONS);
    const BgHeadOut o = bg_head_row_host(BG_HEAD_EVALUATE, mask != nullptr, logits + i * BG_HEAD_ACTIONS, k, P, 0, 0, 0, actions[i]);
    log_prob[i] = o.log_prob; entropy[i] = o.entropy;
  }
}
"""


class Host:
    def __init__(self, lib):
        self.lib = lib
        vp, u64, i64, f = C.c_void_p, C.c_uint64, C.c_int64, C.c_float
        lib.ppo_host.argtypes = [vp, C.c_int, u64, vp, u64, vp, vp, vp, vp, vp, vp, i64, i64, f, f, f, C.c_uint32, C.c_int, vp, u64, vp, vp, vp, vp]
        lib.ppo_host.restype = None
        lib.head_evaluate.argtypes = [vp, vp, vp, i64, vp, vp]
        lib.head_evaluate.restype = None

    def run(self, c: ppo_ref.Case, clip, ent, vf, normalize, use_values=True, keep=False, bf16=False, dstride=60):
        """-> (dlogits float32 [m, 60] (bf16: uint16 bits), dvalues or None, log_prob, entropy, stats) with the padding of a strided dlogits checked."""
        m = c.m
        logits = head_ref.bf16_bits(c.logits) if bf16 else np.ascontiguousarray(c.logits, np.float32)
        dl = np.full((m, dstride), 0x7B7B if bf16 else -777.0, np.uint16 if bf16 else np.float32)
        has_v = use_values and c.values is not None
        dv = np.full(m, -777.0, np.float32) if has_v else None
        lp, en, st = np.empty(m, np.float32), np.empty(m, np.float32), np.empty(10, np.float32)
        keepalive = [np.ascontiguousarray(x) if x is not None else None for x in (c.mask, c.actions, c.old_log_prob, c.advantages, c.values if has_v else None,
                                                                                  c.returns if has_v else None, c.index)]
        ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
        self.lib.ppo_host(ptr(logits), int(bf16), 60, ptr(keepalive[0]), 60, ptr(keepalive[1]), ptr(keepalive[2]), ptr(keepalive[3]), ptr(keepalive[4]),
                          ptr(keepalive[5]), ptr(keepalive[6]), c.store_rows, m, clip, ent, vf, 1 if normalize else 0, int(keep), ptr(dl), dstride, ptr(dv),
                          ptr(lp), ptr(en), ptr(st))
        assert (dl[:, 60:] == (0x7B7B if bf16 else np.float32(-777.0))).all(), "padding columns were written"
        return dl[:, :60].copy(), dv, lp, en, st

    def head(self, logits, mask, actions):
        m = logits.shape[0]
        lp, en = np.empty(m, np.float32), np.empty(m, np.float32)
        lg, mk, a = np.ascontiguousarray(logits, np.float32), None if mask is None else np.ascontiguousarray(mask, np.int8), np.ascontiguousarray(actions, np.int32)
        self.lib.head_evaluate(lg.ctypes.data, None if mk is None else mk.ctypes.data, a.ctypes.data, m, lp.ctypes.data, en.ctypes.data)
        return lp, en


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile csrc/bg_ppo.h for the host"
    d = tmp_path_factory.mktemp("ppo_host")
    src = d / "ppo_host.cpp"
    src.write_text(_PROGRAM)
    so = d / "ppo_host.so"
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-I", os.path.dirname(HEADER), "-o", str(so), str(src)])
    return Host(C.CDLL(str(so)))


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


_shares: dict = {}


def _note(sh):
    for k, v in sh.items():
        _shares[k] = max(_shares.get(k, 0.0), v)


# ---------------------------------------------------------------- the reference alone

def boundary_case():
    """64 unmasked rows whose float64 ratio sits at 1 (the tie of torch.min), 1e-9 and 1e-3 (relative) inside and outside lo and hi, and far outside,
    with advantages of both signs and zero: old_log_prob is set in float64 so that the reference's own ratio lands there.  (A ratio EXACTLY on lo cannot
    be made through exp; there the contract's inclusive comparison is torch.clamp's backward, which passes the gradient on the boundary.)"""
    c = ppo_ref.synthetic(5, 64, 1.0, False, hand_made=False)
    r = head_ref.Reference(c.logits, None)
    lp = r.log_prob(c.actions)
    lo, hi = float(np.float32(1) - np.float32(0.2)), float(np.float32(1) + np.float32(0.2))
    targets = [lo * (1 + 1e-9), lo * (1 - 1e-9), hi * (1 + 1e-9), hi * (1 - 1e-9), 1.0, lo * (1 + 1e-3), lo * (1 - 1e-3), hi * (1 + 1e-3), hi * (1 - 1e-3), 0.5, 2.0]
    old = np.array([lp[i] - np.log(targets[i % len(targets)]) for i in range(64)])
    c.old_log_prob = old   # float64 on purpose: only the reference reads this case
    c.advantages = np.where(np.arange(64) % 3 == 0, 0.0, c.advantages).astype(np.float32)
    return c, targets


def test_the_two_statements_of_the_reference_agree():
    """torch float64 autograd against the numpy closed form: every scalar and every gradient element within 1e-12 (relative to the row's scale), on
    synthetic sets of every kind, on the hand-made rows and on rows whose ratio sits exactly on a boundary or on the tie."""
    cases = []
    for sigma in (0.1, 3.0, 10.0):
        for masked in (False, True):
            cases.append((f"sigma {sigma} masked {masked}", ppo_ref.synthetic(int(sigma * 10) + masked, 2000, sigma, masked, index="repeat" if masked else None)))
    cases.append(("perm", ppo_ref.synthetic(3, 300, 1.0, True, index="perm")))
    cases.append(("nan adv", ppo_ref.add_nan_advantage(ppo_ref.synthetic(4, 300, 1.0, True))))
    cases.append(("single row", ppo_ref.synthetic(6, 1, 1.0, False)))
    bc, targets = boundary_case()
    cases.append(("boundaries", bc))
    for name, c in cases:
        for normalize, ent, vf, use_v in ((False, 0.0, 0.5, True), (True, 0.01, 0.5, True), (True, 0.02, 0.5, False), (False, 0.01, 0.25, False)):
            cf = ppo_ref.ClosedForm(c, 0.2, ent, vf, normalize, use_v)
            scal, dl, dv = ppo_ref.torch_statement(c, 0.2, ent, vf, normalize, ~cf.excluded, use_v)
            for k, v in scal.items():
                assert abs(v - cf.stats[k]) <= 1e-12 * (1.0 + abs(v)), (name, normalize, k, v, cf.stats[k])
            scale = (np.abs(cf.g_pass)[:, None] + cf.ent + 1e-300) / c.m
            assert (np.abs(dl - cf.dlogits) <= 1e-11 * scale + 1e-300).all(), (name, normalize, "dlogits", np.abs(dl - cf.dlogits).max())
            if use_v:
                assert np.allclose(dv, cf.dvalues, rtol=1e-13, atol=0.0), (name, "dvalues")
            if name == "nan adv":
                assert cf.excluded.all() == normalize and cf.excluded[11]
            if name == "single row":
                assert not cf.apply and cf.excluded.sum() == 0
    # the boundary rows take the branches the contract states: on lo / hi exactly the gradient passes; outside it passes only when s1 < s2
    cf = ppo_ref.ClosedForm(bc, 0.2, 0.0, 0.5, False, False)
    for i in range(64):
        t, adv = targets[i % len(targets)], float(bc.advantages[i])
        assert abs(cf.ratio[i] - t) <= 1e-13 * t
    inside = [i for i in range(64) if cf.lo < targets[i % len(targets)] < cf.hi]
    assert len(inside) > 20 and all(cf.g[i] == cf.g_pass[i] for i in inside), "inside the range the gradient always passes"
    for i in range(64):
        t = targets[i % len(targets)]
        if not cf.lo < t < cf.hi:
            assert (cf.g[i] != 0.0) == ((bc.advantages[i] < 0) if t > cf.hi else (bc.advantages[i] > 0)), (i, t)
    out_hi = [i for i in range(64) if targets[i % len(targets)] == 2.0]
    assert all((cf.g[i] != 0.0) == (bc.advantages[i] < 0) for i in out_hi), "above hi the gradient passes only for a negative advantage"
    out_lo = [i for i in range(64) if targets[i % len(targets)] == 0.5]
    assert all((cf.g[i] != 0.0) == (bc.advantages[i] > 0) for i in out_lo), "below lo the gradient passes only for a positive advantage"


def _set(sigma, masked, index=None):
    return ppo_ref.synthetic(int(sigma * 10) + 2 * masked + (5 if index else 0), M, sigma, masked, index=index)


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("sigma", head_ref.SIGMAS)
def test_reference_sets_are_fit(sigma, masked):
    """At most 0.5 % undecidable rows in every set the host test uses (a property of the reference alone), a good share of rows clipped on both sides, and
    every hand-made kind present."""
    for index in (None, "repeat"):
        c = _set(sigma, masked, index)
        for normalize in (False, True):
            cf = ppo_ref.ClosedForm(c, 0.2, 0.01, 0.5, normalize)
            und = (~cf.decidable).mean()
            assert und <= ppo_ref.UNDECIDABLE_CAP, (sigma, masked, index, normalize, und)
            live = ~cf.excluded
            assert (cf.ratio[live] > cf.hi).mean() > 0.05 and (cf.ratio[live] < cf.lo).mean() > 0.05
            assert cf.excluded[[1, 2, 3, 4, 5, 6][1 - masked:]].all() and not cf.excluded[7] and (index is None or (cf.excluded[8] and cf.excluded[10]))
            assert not masked or (not cf.excluded[9] and cf.log_prob[9] == 0.0 and cf.H[9] == 0.0)


# ---------------------------------------------------------------- the header on the host

@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("sigma", head_ref.SIGMAS)
def test_synthetic_sets_hold_the_bounds(host, sigma, masked):
    for index in (None, "repeat"):
        c = _set(sigma, masked, index)
        for normalize, ent, vf, use_v in ((True, 0.01, 0.5, True), (False, 0.01, 0.5, True), (True, 0.02, 0.5, False), (False, 0.0, 0.5, False)):
            cf = ppo_ref.ClosedForm(c, 0.3 if ent == 0.02 else 0.2, ent, vf, normalize, use_v)
            dl, dv, lp, en, st = host.run(c, float(cf.clip32), ent, vf, normalize, use_v)
            sh = ppo_ref.ClosedForm.check(cf, dl, dv, lp, en, st, f"sigma {sigma} masked {masked} index {index} norm {normalize} values {use_v}")
            _note(sh)
            again = host.run(c, float(cf.clip32), ent, vf, normalize, use_v, keep=True)
            for x, y in zip((dl, dv, lp, en, st), again):
                assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y)), "keeping e[j] and calling expf again give the same bits"
        # log_prob / entropy are the host bg_head_row's, bit for bit
        ok, mk, a, _, _, _ = c.gathered()
        hlp, hen = host.head(c.logits, mk, a)
        assert np.array_equal(_bits(lp)[ok], _bits(hlp)[ok]) and np.array_equal(_bits(en)[ok], _bits(hen)[ok])
    print(f"sigma {sigma} masked {masked}: largest shares so far {_shares}")


@pytest.mark.parametrize("masked,index,normalize", [(True, "perm", True), (False, None, True), (True, "repeat", True), (True, "perm", False)],
                         ids=["masked-perm", "unmasked", "masked-repeat", "masked-perm-raw-adv"])
@pytest.mark.parametrize("m", [256 * 64 + 64 + 1, 256 * 256 + 256 + 1])
def test_the_twins_second_level_folds(host, m, masked, index, normalize):
    """per > 1 in the twin's own SLICES-THEN-TREE loops: m = 16 449 gives 258 row partials (per = 2 in the finish), m = 65 793 gives 258 advantage
    triples (per = 2 in the moments) and 1 029 row partials (per = 5, lane 205 folds four, the lanes above none).  The sets are held to the cap."""
    c = ppo_ref.synthetic(m % 1000 + 2 * masked + (5 if index else 0), m, 1.0, masked, index=index)
    what = f"m {m} masked {masked} index {index} norm {normalize}"
    cf = ppo_ref.ClosedForm(c, 0.2, 0.01, 0.5, normalize)
    first = host.run(c, 0.2, 0.01, 0.5, normalize)
    dl, dv, lp, en, st = first
    _note(cf.check(dl, dv, lp, en, st, what, cap=True))
    assert st[9] == m and st[8] == cf.excluded.sum() > 0 and cf.apply == normalize
    for x, y in zip(first, host.run(c, 0.2, 0.01, 0.5, normalize, keep=True)):
        assert np.array_equal(_bits(x), _bits(y)), what + ": two calls differ"
    ok, mk, a, _, _, _ = c.gathered()
    hlp, hen = host.head(c.logits, mk, a)
    assert np.array_equal(_bits(lp)[ok], _bits(hlp)[ok]) and np.array_equal(_bits(en)[ok], _bits(hen)[ok])
    print(f"{what}: undecidable {(~cf.decidable).mean():.5f}; largest shares so far {_shares}")


def test_hand_made_rows(host):
    for masked in (False, True):
        for index in (None, "perm", "repeat"):
            c = ppo_ref.synthetic(21 + masked, 300, 1.0, masked, index=index)
            for normalize in (False, True):
                cf = ppo_ref.ClosedForm(c, 0.2, 0.01, 0.5, normalize)
                dl, dv, lp, en, st = host.run(c, 0.2, 0.01, 0.5, normalize, dstride=64)
                cf.check(dl, dv, lp, en, st, f"hand-made masked {masked} index {index}", cap=False)
                want = {1, 2, 3, 4, 5, 6} - (set() if masked else {1}) | ({8, 10} if index else set())
                assert want <= set(np.flatnonzero(cf.excluded).tolist()) and st[8] == cf.excluded.sum() >= len(want) and st[9] == 300
                assert not cf.excluded[7] and c.gathered()[4][7] == 0.0
                if not normalize:   # adv == 0: only the entropy part is left
                    assert np.allclose(dl[7], cf.ent_part[7] / 300, rtol=1e-3, atol=1e-12)
            # without the value term the non-finite return does not exclude its row
            cf = ppo_ref.ClosedForm(c, 0.2, 0.01, 0.5, False, use_values=False)
            dl, dv, lp, en, st = host.run(c, 0.2, 0.01, 0.5, False, use_values=False)
            assert dv is None and not cf.excluded[6] and st[2] == 0.0
            cf.check(dl, dv, lp, en, st, "no value term", cap=False)
    # a NaN advantage: one excluded row without normalisation, every row with it (the statistics are over all m advantages)
    c = ppo_ref.add_nan_advantage(ppo_ref.synthetic(30, 300, 1.0, True))
    for normalize in (False, True):
        cf = ppo_ref.ClosedForm(c, 0.2, 0.01, 0.5, normalize)
        dl, dv, lp, en, st = host.run(c, 0.2, 0.01, 0.5, normalize)
        cf.check(dl, dv, lp, en, st, f"nan advantage norm {normalize}", cap=False)
        assert (st[8] == 300) == normalize and (not normalize or (np.isnan(st[6]) and st[0] == 0.0 and (dl == 0).all()))
    # m = 1 and m = 2: SB3's len > 1
    for m in (1, 2):
        c = ppo_ref.synthetic(40 + m, m, 1.0, False, hand_made=False)
        cf = ppo_ref.ClosedForm(c, 0.2, 0.01, 0.5, True)
        assert cf.apply == (m > 1)
        cf.check(*host.run(c, 0.2, 0.01, 0.5, True), f"m {m}", cap=False)


def test_ratio_one_and_bf16(host):
    """old_log_prob taken from the host head itself: ratio is exactly 1, so approx_kl == 0, clip_fraction == 0 and policy_loss is the float64 mean of
    -adv' rounded.  bf16: logits widened exactly, dlogits the float32 result rounded to nearest even, bit for bit."""
    c = ppo_ref.synthetic(50, 4133, 3.0, True, hand_made=False)
    lp, _ = host.head(c.logits, c.mask, c.actions)
    c.old_log_prob = lp.copy()
    dl, dv, lp2, en, st = host.run(c, 0.2, 0.01, 0.5, False)
    assert np.array_equal(_bits(lp2), _bits(lp)) and st[4] == 0.0 and st[5] == 0.0 and st[8] == 0.0
    assert st[1] == np.float32((-c.advantages.astype(np.float64)).sum() / 4133)
    dl, dv, _, _, st = host.run(c, 0.2, 0.01, 0.5, True)
    mean, std = np.float32(c.advantages.astype(np.float64).mean()), np.float32(c.advantages.astype(np.float64).std(ddof=1))
    assert st[6] == mean and st[7] == std
    advn = (c.advantages - mean) / (std + np.float32(1e-8))
    assert advn.dtype == np.float32 and st[1] == np.float32((-advn.astype(np.float64)).sum() / 4133) and st[4] == 0.0
    cb = ppo_ref.synthetic(51, 1000, 3.0, True, bf16=True)
    f32 = host.run(cb, 0.2, 0.01, 0.5, True)
    b16 = host.run(cb, 0.2, 0.01, 0.5, True, bf16=True, dstride=64)
    assert np.array_equal(b16[0], head_ref.bf16_bits(f32[0])) and b16[0].dtype == np.uint16
    for x, y in zip(f32[1:], b16[1:]):
        assert np.array_equal(_bits(x), _bits(y))


def test_header_declares_and_library_exports_ppo_loss():
    from balatro_gym_amd import _native as nat, build
    import balatro_gym_amd
    hdr = open(HEADER).read()
    m = re.search(r"\bint\s+bg_ppo_loss\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/balatro_mi355x.h does not declare bg_ppo_loss"
    params = [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", p).strip()) for p in m.group(1).split(",")]
    assert params == ["const void* logits_dev", "int logits_dtype", "uint64_t logits_stride_elems", "const int8_t* mask_dev", "uint64_t mask_stride_bytes",
                      "const int32_t* actions_dev", "const float* old_log_prob_dev", "const float* advantages_dev", "const float* values_dev",
                      "const float* returns_dev", "const int32_t* index_dev", "int64_t store_rows", "int64_t m", "float clip_range", "float ent_coef",
                      "float vf_coef", "uint32_t flags", "void* dlogits_dev", "uint64_t dlogits_stride_elems", "float* dvalues_dev", "float* log_prob_dev",
                      "float* entropy_dev", "float* stats_dev", "void* workspace_dev", "uint64_t workspace_bytes", "float* kernel_ms_out", "void* stream"], params
    assert re.search(r"uint64_t\s+bg_ppo_loss_workspace_bytes\s*\(\s*int64_t m\s*\)\s*;", hdr)
    for name, val in (("BG_PPO_STATS", "10"), ("BG_PPO_NORMALIZE_ADV", "1u")):
        assert re.search(rf"#define {name} {val}\b", hdr), name
    doc = hdr[:hdr.index("#define BG_PPO_STATS")].rsplit("\n/*", 1)[1]
    for cite in ("hpc_train.py:77-88", "train_progressive.py:161-176", "RolloutBuffer.get", "std + 1e-8f", "lo <= ratio <= hi", "(ratio - 1) - lr", "EXCLUDED",
                 "the divisor stays m", "same bits", "clip_range_vf", "bg_ppo_loss: "):
        assert cite in doc, cite
    assert nat.PPO_STATS == ppo_ref.STATS and nat.PPO_NORMALIZE_ADV == 1
    assert "bg_ppo_loss" in nat.EXPORTS and "bg_ppo_loss_workspace_bytes" in nat.EXPORTS
    assert os.path.join(CSRC, "bg_ppo.h") in build.DEPS
    assert "ppo_loss" in balatro_gym_amd.__all__
    if os.path.exists(build.LIB):
        L = C.CDLL(build.LIB)
        assert hasattr(L, "bg_ppo_loss") and hasattr(L, "bg_ppo_loss_workspace_bytes")
        L.bg_ppo_loss_workspace_bytes.restype = C.c_uint64
        L.bg_ppo_loss_workspace_bytes.argtypes = [C.c_int64]
        assert L.bg_ppo_loss_workspace_bytes(0) == 0 and L.bg_ppo_loss_workspace_bytes(65) == 16 + 24 + 2 * 48


def test_wrapper_refuses_bad_arguments_before_the_library():
    """ppo_loss on CPU tensors: every bad argument is a ValueError raised before anything is loaded."""
    import torch
    from balatro_gym_amd import ppo_loss
    N = 6
    lg = torch.zeros((N, 60))
    a, f = torch.zeros(N, dtype=torch.int32), torch.zeros(N)
    for bad in (lg.double(), torch.zeros((N, 59)), "logits", None):
        with pytest.raises(ValueError, match=r"float32 or bfloat16 tensor \[\.\.\., 60\]"):
            ppo_loss(bad, a, f, f)
    with pytest.raises(ValueError, match="dense over its row pitch"):
        ppo_loss(torch.zeros((N, 120))[:, ::2], a, f, f)
    for bad in (a.long(), torch.zeros(N + 1, dtype=torch.int32), None, [0] * N):
        with pytest.raises(ValueError, match="actions must be"):
            ppo_loss(lg, bad, f, f)
    for name in ("old_log_prob", "advantages"):
        for bad in (f.double(), torch.zeros(N + 1), torch.zeros(2 * N)[::2], None):
            args = {"old_log_prob": f, "advantages": f}
            args[name] = bad
            with pytest.raises(ValueError, match=f"{name} must be a contiguous"):
                ppo_loss(lg, a, args["old_log_prob"], args["advantages"])
    with pytest.raises(ValueError, match="both or neither"):
        ppo_loss(lg, a, f, f, values=f)
    with pytest.raises(ValueError, match="both or neither"):
        ppo_loss(lg, a, f, f, returns=f)
    with pytest.raises(ValueError, match="values must be a contiguous"):
        ppo_loss(lg, a, f, f, values=torch.zeros((N, 1)), returns=f)
    with pytest.raises(ValueError, match="returns must be a contiguous"):
        ppo_loss(lg, a, f, f, values=f, returns=f.double())
    for bad in (torch.zeros((N, 360), dtype=torch.uint8), torch.zeros((N, 60), dtype=torch.bool), torch.zeros((N + 1, 384), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="mask|packed records"):
            ppo_loss(lg, a, f, f, bad)
    for bad in (torch.zeros(N, dtype=torch.int64), torch.zeros(N + 1, dtype=torch.int32), "index"):
        with pytest.raises(ValueError, match="index must be a contiguous"):
            ppo_loss(lg, a, f, f, index=bad)
    for kw in ({"clip_range": 0.0}, {"clip_range": 1.0}, {"clip_range": -0.2}, {"clip_range": float("nan")}, {"ent_coef": float("inf")}, {"vf_coef": "x"}):
        with pytest.raises(ValueError, match="clip_range must be in|must be a finite number"):
            ppo_loss(lg, a, f, f, **kw)
    # everything right, index included (stored arrays of another length): what is left is that there is no CPU path
    S = 11
    sa, sf = torch.zeros(S, dtype=torch.int32), torch.zeros(S)
    ix = torch.zeros(N, dtype=torch.int32)
    for mask in (None, torch.zeros((S, 384), dtype=torch.uint8), torch.ones((S, 60), dtype=torch.int8)):
        with pytest.raises(ValueError, match="device tensor"):
            ppo_loss(lg, sa, sf, sf, mask, values=f, returns=sf, index=ix, clip_range=0.3, ent_coef=0.02)
    with pytest.raises(ValueError, match="device tensor"):
        ppo_loss(lg.to(torch.bfloat16), a, f, f, normalize_advantage=False)
