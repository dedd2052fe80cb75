"""bg_bc_loss on the CPU (no GPU).  First the reference is held to itself: tests/bc_ref.py's two statements -- the composite written literally in torch
float64 under autograd, and the contract's closed form in numpy float64 -- agree, hand-made rows and ties included.  Then csrc/bg_bc.h -- the per-row
arithmetic the kernel runs and the serial twin of its launch sequence -- is compiled with g++ (-O1 -ffp-contract=off -DBG_BC_HOST) into a small shared
object and held to the closed form by the bounds derived in bc_ref: m in {1, 63, 64, 65, 257, 16 449} (the last makes the finishing fold run with
per > 1), float32 and bfloat16, the mask from records, dense int8 and none, actions dense and in place in records, an index with out-of-range
entries, weights with zeros, one negative and one NaN, all weights zero, and the hand-made rows (every action masked, the stored action masked, ties
of the maximum); log_prob / entropy bit-equal to the host bg_head_row.  Also: the header's declaration, the exports, build.DEPS, and the argument
checks of the Python wrapper.

Largest observed shares of the bounds with g++ and glibc's expf / logf: dlogits 0.25, nll_loss 0.027, entropy_loss 0.020, loss 0.028, accuracy 0.43,
weight_sum 0.41, log_prob 0.126, entropy 0.093."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import bc_ref, head_ref
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")
SIZES = (1, 63, 64, 65, 257, 256 * 64 + 64 + 1)
REC, MASK_OFF, ACT_OFF = 384, 176, 172

_PROGRAM = r"""
#define BG_BC_HOST
#include <stdio.h>
#include <stdlib.h>
#include "balatro_mi355x.h"
#include "bg_bc.h"
extern "C" void bc_host(const void* logits, int bf16, uint64_t lstride, const int8_t* mask, uint64_t mstride, const int32_t* actions, uint64_t astride,
                        const float* weights, const int32_t* index, int64_t store_rows, int64_t m, float ent_coef, int keep, void* dlogits, uint64_t dstride,
                        float* log_prob, float* entropy, float* stats) {
  BgBcArgs A = {};
  A.logits = logits; A.lstride = lstride; A.mask = mask; A.mstride = mstride; A.actions = actions; A.astride = astride; A.weights = weights;
  A.index = index; A.store_rows = store_rows; A.m = m; A.ent_coef = ent_coef; A.fm = (float)m;
  A.dlogits = dlogits; A.dstride = dstride; A.log_prob = log_prob; A.entropy = entropy;
  bg_bc_host(A, bf16 != 0, keep != 0, stats);
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


def records_of(c: bc_ref.Case, seed: int = 1):
    """The case's masks and actions inside [store_rows, 384] records of random bytes -> uint8 array (mask at 176, action at 172)."""
    rows = np.random.default_rng(seed).integers(0, 256, (c.store_rows, REC), dtype=np.uint8)
    if c.mask is not None:
        rows[:, MASK_OFF:MASK_OFF + 60] = c.mask.view(np.uint8)
    rows[:, ACT_OFF:ACT_OFF + 4] = np.ascontiguousarray(c.actions).view(np.uint8).reshape(-1, 4)
    return rows


class Host:
    def __init__(self, lib):
        self.lib = lib
        vp, u64, i64, f = C.c_void_p, C.c_uint64, C.c_int64, C.c_float
        lib.bc_host.argtypes = [vp, C.c_int, u64, vp, u64, vp, u64, vp, vp, i64, i64, f, C.c_int, vp, u64, vp, vp, vp]
        lib.bc_host.restype = None
        lib.head_evaluate.argtypes = [vp, vp, vp, i64, vp, vp]
        lib.head_evaluate.restype = None

    def run(self, c: bc_ref.Case, ent, keep=False, bf16=False, dstride=60, in_records=False):
        """-> (dlogits float32 [m, 60] (bf16: uint16 bits), log_prob, entropy, stats) with the padding of a strided dlogits checked.
        in_records: the mask and the actions are read in place from 384-byte records."""
        m = c.m
        logits = head_ref.bf16_bits(c.logits) if bf16 else np.ascontiguousarray(c.logits, np.float32)
        dl = np.full((m, dstride), 0x7B7B if bf16 else -777.0, np.uint16 if bf16 else np.float32)
        lp, en, st = np.empty(m, np.float32), np.empty(m, np.float32), np.empty(7, np.float32)
        ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
        if in_records:
            rows = records_of(c)
            mask_p, ms, act_p, astr = (rows.ctypes.data + MASK_OFF if c.mask is not None else None), REC, rows.ctypes.data + ACT_OFF, REC
        else:
            mk, ac = (None if c.mask is None else np.ascontiguousarray(c.mask)), np.ascontiguousarray(c.actions)
            mask_p, ms, act_p, astr = ptr(mk), 60, ptr(ac), 4
        w, ix = (None if c.weights is None else np.ascontiguousarray(c.weights)), (None if c.index is None else np.ascontiguousarray(c.index))
        self.lib.bc_host(ptr(logits), int(bf16), 60, mask_p, ms, act_p, astr, ptr(w), ptr(ix), c.store_rows, m, ent, int(keep), ptr(dl), dstride, ptr(lp),
                         ptr(en), ptr(st))
        assert (dl[:, 60:] == (0x7B7B if bf16 else np.float32(-777.0))).all(), "padding columns were written"
        return dl[:, :60].copy(), lp, en, st

    def head(self, logits, mask, actions):
        m = logits.shape[0]
        lp, en = np.empty(m, np.float32), np.empty(m, np.float32)
        lg, mk, a = np.ascontiguousarray(logits, np.float32), None if mask is None else np.ascontiguousarray(mask, np.int8), np.ascontiguousarray(actions, np.int32)
        self.lib.head_evaluate(lg.ctypes.data, None if mk is None else mk.ctypes.data, a.ctypes.data, m, lp.ctypes.data, en.ctypes.data)
        return lp, en


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile csrc/bg_bc.h for the host"
    d = tmp_path_factory.mktemp("bc_host")
    src = d / "bc_host.cpp"
    src.write_text(_PROGRAM)
    so = d / "bc_host.so"
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-I", os.path.dirname(HEADER), "-o", str(so), str(src)])
    return Host(C.CDLL(str(so)))


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


_shares: dict = {}


def _note(sh):
    for k, v in sh.items():
        _shares[k] = max(_shares.get(k, 0.0), v)


# ---------------------------------------------------------------- the reference alone

def test_the_two_statements_of_the_reference_agree():
    """torch float64 autograd against the numpy closed form: every scalar and every gradient element within 1e-12 (relative to the row's scale), on
    synthetic sets of every kind and on the hand-made rows, ties of the maximum included."""
    cases = []
    for sigma in (0.1, 3.0, 10.0):
        for masked in (False, True):
            for weights in (None, "random"):
                cases.append((f"sigma {sigma} masked {masked} weights {weights}",
                              bc_ref.synthetic(int(sigma * 10) + masked, 2000, sigma, masked, index="repeat" if masked else None, weights=weights)))
    cases.append(("perm filter", bc_ref.synthetic(3, 300, 1.0, True, index="perm", weights="filter")))
    cases.append(("all zero", bc_ref.synthetic(4, 300, 1.0, True, weights="zero")))
    cases.append(("single row", bc_ref.synthetic(6, 1, 1.0, False)))
    for name, c in cases:
        for ent in (0.0, 0.01):
            cf = bc_ref.ClosedForm(c, ent)
            scal, dl = bc_ref.torch_statement(c, ent, ~cf.excluded, cf.W)
            for k, v in scal.items():
                assert abs(v - cf.stats[k]) <= 1e-12 * (1.0 + abs(v)), (name, ent, k, v, cf.stats[k])
            scale = (cf.w / cf.W if cf.W > 0 else np.zeros(c.m))[:, None] * (1.0 + cf.ent) + 1e-300
            assert (np.abs(dl - cf.dlogits) <= 1e-11 * scale).all(), (name, ent, "dlogits", np.abs(dl - cf.dlogits).max())
    # the hand-made rows take the branches the contract states
    for masked in (False, True):
        c = bc_ref.synthetic(21 + masked, 300, 1.0, masked, weights="random")
        cf = bc_ref.ClosedForm(c, 0.01)
        assert cf.excluded[[1, 2, 3, 4, 9, 12, 13]].all() and not cf.excluded[[5, 6, 7, 14, 15]].any()
        assert cf.hit_row[5] and not cf.hit_row[6], "of a tie of the maximum the FIRST index is the hit"
        assert cf.w[14] == 0.0 and (cf.dlogits[14] == 0.0).all() and cf.w[15] == 2.5
        assert not masked or (cf.log_prob[7] == 0.0 and cf.H[7] == 0.0)
        assert 0.3 < cf.stats["accuracy"] < 0.95


# ---------------------------------------------------------------- the header on the host

def _set(m, masked, index, weights, bf16=False):
    sigma = head_ref.SIGMAS[(m + 2 * masked + (index is not None)) % 4]
    return bc_ref.synthetic(m + 7 * masked + (5 if index else 0), m, sigma, masked, index=index, weights=weights, bf16=bf16)


@pytest.mark.parametrize("m", SIZES)
def test_sets_hold_the_bounds(host, m):
    for masked in (False, True):
        for index in (None, "repeat", "perm"):
            for weights in (None, "random", "filter", "zero"):
                c = _set(m, masked, index, weights)
                for ent in (0.0, 0.01):
                    what = f"m {m} masked {masked} index {index} weights {weights} ent {ent}"
                    cf = bc_ref.ClosedForm(c, ent)
                    first = host.run(c, ent)
                    _note(cf.check(*first, what))
                    st = first[3]
                    assert st[6] == m and st[5] == cf.excluded.sum()
                    if weights == "zero" or cf.W == 0.0:
                        assert (st[:5] == 0.0).all() and (first[0].view(np.uint32) == 0).all(), what + ": W == 0 gives loss 0 and an all-+0.0 gradient"
                    if weights is None and index is None:
                        assert st[4] == m
                    for x, y in zip(first, host.run(c, ent, keep=True)):
                        assert np.array_equal(_bits(x), _bits(y)), what + ": keeping e[j] and calling expf again give the same bits"
                    # the mask and the actions read in place from records: the same bits
                    for x, y in zip(first, host.run(c, ent, in_records=True, dstride=64)):
                        assert np.array_equal(_bits(x), _bits(y)), what + ": in place from records"
                # log_prob / entropy are the host bg_head_row's, bit for bit
                ok, mk, a, _ = c.gathered()
                hlp, hen = host.head(c.logits, mk, a)
                assert np.array_equal(_bits(first[1])[ok], _bits(hlp)[ok]) and np.array_equal(_bits(first[2])[ok], _bits(hen)[ok])
    print(f"m {m}: largest shares so far {_shares}")


def test_hand_made_rows(host):
    for masked in (False, True):
        for index in (None, "perm"):
            c = bc_ref.synthetic(21 + masked, 300, 1.0, masked, index=index, weights="random")
            cf = bc_ref.ClosedForm(c, 0.01)
            dl, lp, en, st = host.run(c, 0.01, dstride=64)
            cf.check(dl, lp, en, st, f"hand-made masked {masked} index {index}")
            want = {1, 2, 3, 4, 9, 12, 13} | ({8, 10} if index else set())
            assert want <= set(np.flatnonzero(cf.excluded).tolist()) and st[5] == cf.excluded.sum() >= len(want) and st[6] == 300
            assert (dl[sorted(want)].view(np.uint32) == 0).all()
            assert np.isneginf(lp[1]) == masked and np.isnan(lp[2]) and np.isnan(lp[3]) and np.isnan(lp[4]) and np.isneginf(lp[9])
            # the ties: row 5 demonstrates the first maximum (a hit), row 6 the second (no hit); both have p = 1/2 (+ the rest) on each
            a5, a6 = int(c.gathered()[2][5]), int(c.gathered()[2][6])
            assert (a5, a6) == (11, 40) and dl[5, 11] < 0 < dl[5, 40] and dl[6, 40] < 0 < dl[6, 11]
    # accuracy is exact: the weighted share of hits, rounded once
    c = bc_ref.synthetic(33, 1000, 3.0, True, weights="filter", hand_made=False)
    cf = bc_ref.ClosedForm(c, 0.0)
    st = host.run(c, 0.0)[3]
    assert st[3] == np.float32((cf.w * cf.hit_row).sum() / cf.W) and st[4] == np.float32(cf.W) == (c.weights > 0).sum()


def test_bf16(host):
    """bf16: logits widened exactly, dlogits the float32 result rounded to nearest even, bit for bit; everything else the same bits."""
    cb = bc_ref.synthetic(51, 1000, 3.0, True, bf16=True, weights="random")
    f32 = host.run(cb, 0.01)
    b16 = host.run(cb, 0.01, bf16=True, dstride=64)
    assert np.array_equal(b16[0], head_ref.bf16_bits(f32[0])) and b16[0].dtype == np.uint16
    for x, y in zip(f32[1:], b16[1:]):
        assert np.array_equal(_bits(x), _bits(y))
    bc_ref.ClosedForm(cb, 0.01).check(*f32, "bf16-valued logits")


def test_header_declares_and_library_exports_bc_loss():
    from balatro_gym_amd import _native as nat, build
    import balatro_gym_amd
    hdr = open(HEADER).read()
    m = re.search(r"\bint\s+bg_bc_loss\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/balatro_mi355x.h does not declare bg_bc_loss"
    params = [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", p).strip()) for p in m.group(1).split(",")]
    assert params == ["const void* logits_dev", "int logits_dtype", "uint64_t logits_stride_elems", "const int8_t* mask_dev", "uint64_t mask_stride_bytes",
                      "const int32_t* actions_dev", "uint64_t actions_stride_bytes", "const float* weights_dev", "const int32_t* index_dev",
                      "int64_t store_rows", "int64_t m", "float ent_coef", "void* dlogits_dev", "uint64_t dlogits_stride_elems", "float* log_prob_dev",
                      "float* entropy_dev", "float* stats_dev", "void* workspace_dev", "uint64_t workspace_bytes", "float* kernel_ms_out", "void* stream"], params
    assert re.search(r"uint64_t\s+bg_bc_loss_workspace_bytes\s*\(\s*int64_t m\s*\)\s*;", hdr)
    assert re.search(r"#define BG_BC_STATS 7\b", hdr)
    doc = hdr[:hdr.index("int bg_episode_outcome_rows")].rsplit("\n/*", 1)[1]
    for cite in ("train_balatro_agent.py:220-262", "TODO: Implement actual BC training loop", "actions_stride_bytes", "BG_ROW_ACTION in place", "EXCLUDED",
                 "W == 0", "first maximum among the valid logits", "same bits", "label smoothing", "bg_bc_loss: "):
        assert cite in doc, cite
    assert nat.BC_STATS == bc_ref.STATS
    assert "bg_bc_loss" in nat.EXPORTS and "bg_bc_loss_workspace_bytes" in nat.EXPORTS
    assert os.path.join(CSRC, "bg_bc.h") in build.DEPS
    assert "bc_loss" in balatro_gym_amd.__all__ and "BcStats" in balatro_gym_amd.__all__
    if os.path.exists(build.LIB):
        L = C.CDLL(build.LIB)
        assert hasattr(L, "bg_bc_loss") and hasattr(L, "bg_bc_loss_workspace_bytes")
        L.bg_bc_loss_workspace_bytes.restype = C.c_uint64
        L.bg_bc_loss_workspace_bytes.argtypes = [C.c_int64]
        assert L.bg_bc_loss_workspace_bytes(0) == 0 and L.bg_bc_loss_workspace_bytes(65) == 16 + 8 + 2 * 32


def test_wrapper_refuses_bad_arguments_before_the_library():
    """bc_loss on CPU tensors: every bad argument is a ValueError raised before anything is loaded."""
    import torch
    from balatro_gym_amd import bc_loss
    N = 6
    lg = torch.zeros((N, 60))
    a, f = torch.zeros(N, dtype=torch.int32), torch.zeros(N)
    for bad in (lg.double(), torch.zeros((N, 59)), "logits", None):
        with pytest.raises(ValueError, match=r"float32 or bfloat16 tensor \[\.\.\., 60\]"):
            bc_loss(bad, a)
    with pytest.raises(ValueError, match="dense over its row pitch"):
        bc_loss(torch.zeros((N, 120))[:, ::2], a)
    for bad in (a.long(), torch.zeros(N + 1, dtype=torch.int32), None, [0] * N):
        with pytest.raises(ValueError, match="actions must be"):
            bc_loss(lg, bad)
    with pytest.raises(ValueError, match="one fixed pitch apart"):
        bc_loss(torch.zeros((2, 3, 60)), torch.zeros((2, 8), dtype=torch.int32)[:, ::3])
    for bad in (f.double(), torch.zeros(N + 1), torch.zeros(2 * N)[::2]):
        with pytest.raises(ValueError, match="weights must be a contiguous"):
            bc_loss(lg, a, weights=bad)
    for bad in (torch.zeros((N, 360), dtype=torch.uint8), torch.zeros((N, 60), dtype=torch.bool), torch.zeros((N + 1, 384), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="mask|packed records"):
            bc_loss(lg, a, bad)
    for bad in (torch.zeros(N, dtype=torch.int64), torch.zeros(N + 1, dtype=torch.int32), "index"):
        with pytest.raises(ValueError, match="index must be a contiguous"):
            bc_loss(lg, a, index=bad)
    for bad in (float("inf"), float("nan"), "x", True):
        with pytest.raises(ValueError, match="ent_coef must be a finite number"):
            bc_loss(lg, a, ent_coef=bad)
    # everything right -- the strided action view of records and an index included: what is left is that there is no CPU path
    S = 11
    store = torch.zeros((S + 1, 384), dtype=torch.uint8)
    act = store[1:, 172:176].view(torch.int32)[:, 0]
    assert act.stride() == (96,) and tuple(act.shape) == (S,)
    ix = torch.zeros(N, dtype=torch.int32)
    for mask in (None, store[:S], torch.ones((S, 60), dtype=torch.int8)):
        with pytest.raises(ValueError, match="device tensor"):
            bc_loss(lg, act, mask, weights=torch.ones(S), index=ix, ent_coef=0.01)
    with pytest.raises(ValueError, match="device tensor"):
        bc_loss(lg.to(torch.bfloat16), a)
