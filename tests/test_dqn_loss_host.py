"""bg_dqn_loss, bg_sample_actions_eps and RowReplay on the CPU (no GPU).  First the reference is held to itself: tests/dqn_ref.py's contract in numpy
float32 (a) stays within the bounds derived there of SB3's loss in torch float64 under autograd (b).  Then csrc/bg_dqn.h -- the per-row arithmetic the
kernel runs and the serial twin of its launch sequence -- is compiled with g++ (-O1 -ffp-contract=off -DBG_DQN_HOST) and held to (a): dq, td, the
excluded rows and their count bit for bit on every row, the scalars within 2**-24 * |ref| + 2**-50 * (sum of |terms|); 16 384-row sets for sigma in
{0.1, 1, 3, 10}, float32 and bfloat16, masked and unmasked, plain and double, Huber and MSE, with and without `rewards`; a size at which the twin's fold
takes two partials per lane; the hand-made rows.  The epsilon-greedy row function is held bit for bit to a Python-integer restatement at epsilon 0,
0.05, 0.5 and 1, and the share of exploring rows to four binomial standard deviations.  RowReplay runs on CPU tensors.  Also: the header's
declarations, the exports, build.DEPS, __all__ and the wrappers' argument checks.

Largest observed shares of the bounds of (a) against (b): td 0.56, dq 0.45, loss 0.012.  Of the scalar bound against (a) with g++: 0.97 at 16 384 rows,
0.78 at 16 449 (the final rounding to float32 alone can use all of 2**-24 * |ref|)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import dqn_ref, head_ref
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")
M = 16384
M_FOLD = 256 * 64 + 64 + 1   # 258 workgroup partials: the twin's 256 lanes fold two each
GAMMA = 0.99

_PROGRAM = r"""
#define BG_DQN_HOST
#include <stdio.h>
#include <stdlib.h>
#include "balatro_mi355x.h"
#include "bg_dqn.h"
extern "C" void dqn_host(const void* q, uint64_t qstride, const void* qn, uint64_t nstride, const void* qo, uint64_t ostride, int bf16, const uint8_t* rows,
                         uint64_t rstride, int64_t store_rows, const int32_t* next_index, const float* rewards, int64_t m, float gamma, uint32_t flags,
                         void* dq, uint64_t dstride, float* td, float* stats) {
  BgDqnArgs A = {};
  A.q = q; A.qstride = qstride; A.qn = qn; A.nstride = nstride; A.qo = qo; A.ostride = ostride; A.rows = rows; A.rstride = rstride;
  A.store_rows = store_rows; A.next_index = next_index; A.rewards = rewards; A.m = m; A.gamma = gamma; A.fm = (float)m; A.flags = flags;
  A.dq = dq; A.dstride = dstride; A.td = td;
  bg_dqn_host(A, bf16 != 0, stats);
}
extern "C" void eps_host(const float* logits, const int8_t* mask, int64_t m, uint64_t seed, uint64_t index0, uint64_t t, float epsilon, int32_t* actions,
                         int32_t* greedy) {
  for (int64_t i = 0; i < m; i++) {
    float P[BG_HEAD_ACTIONS];
    uint32_t k[BG_HEAD_ACTIONS / 4] = {};
    if (mask) memcpy(k, mask + i * BG_HEAD_ACTIONS, BG_HEAD_ACTIONS);
    const float* l = logits + i * BG_HEAD_ACTIONS;
    const float u = bg_head_u(bg_head_hash(seed, index0 + (uint64_t)i, t));
    const uint32_t h2 = bg_head_hash(seed + BG_DQN_EPS_SALT, index0 + (uint64_t)i, t);
    actions[i] = mask ? bg_head_eps_row<true>(l, k, u, epsilon, h2) : bg_head_eps_row<false>(l, k, u, epsilon, h2);
    greedy[i] = bg_head_row_host(BG_HEAD_ARGMAX, mask != nullptr, l, k, P, 0, 0, 0, 0).action;
  }
}
"""


class Host:
    def __init__(self, lib):
        self.lib = lib
        vp, u64, i64 = C.c_void_p, C.c_uint64, C.c_int64
        lib.dqn_host.argtypes = [vp, u64, vp, u64, vp, u64, C.c_int, vp, u64, i64, vp, vp, i64, C.c_float, C.c_uint32, vp, u64, vp, vp]
        lib.dqn_host.restype = None
        lib.eps_host.argtypes = [vp, vp, i64, u64, u64, u64, C.c_float, vp, vp]
        lib.eps_host.restype = None

    def run(self, c: dqn_ref.Case, flags, double, use_rewards=False, bf16=False, stride=60, with_td=True):
        """-> (dq float32 [m, 60] (bf16: uint16 bits), td or None, stats); every matrix at `stride`, padding columns checked."""
        m = c.m

        def lay(x):
            buf = np.full((m, stride), 77.0, np.float32)
            buf[:, :60] = x
            return head_ref.bf16_bits(buf).reshape(m, stride) if bf16 else buf
        q, qn, qo = lay(c.q), lay(c.q_next), lay(c.q_online) if double else None
        fill = 0x7B7B if bf16 else np.float32(-777.0)
        dq = np.full((m, stride), fill, np.uint16 if bf16 else np.float32)
        td = np.full(m, -777.0, np.float32) if with_td else None
        st = np.full(8, -777.0, np.float32)
        rows, nx, rw = np.ascontiguousarray(c.rows), np.ascontiguousarray(c.next_index), np.ascontiguousarray(c.rewards)
        before = rows.copy()
        ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
        self.lib.dqn_host(ptr(q), stride, ptr(qn), stride, ptr(qo), stride, int(bf16), ptr(rows), c.stride, c.store_rows, ptr(nx), ptr(rw) if use_rewards else None,
                          m, GAMMA, flags, ptr(dq), stride, ptr(td), ptr(st))
        assert (dq[:, 60:] == fill).all(), "padding columns were written"
        assert np.array_equal(rows, before)
        return dq[:, :60].copy(), td, st

    def eps(self, logits, mask, seed, index0, t, epsilon):
        m = logits.shape[0]
        lg = np.ascontiguousarray(logits, np.float32)
        mk = None if mask is None else np.ascontiguousarray(mask, np.int8)
        a, g = np.empty(m, np.int32), np.empty(m, np.int32)
        self.lib.eps_host(lg.ctypes.data, None if mk is None else mk.ctypes.data, m, seed, index0, t, epsilon, a.ctypes.data, g.ctypes.data)
        return a, g


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile csrc/bg_dqn.h for the host"
    d = tmp_path_factory.mktemp("dqn_host")
    src = d / "dqn_host.cpp"
    src.write_text(_PROGRAM)
    so = d / "dqn_host.so"
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-I", os.path.dirname(HEADER), "-o", str(so), str(src)])
    return Host(C.CDLL(str(so)))


_sets: dict = {}
_shares: dict = {}


def _set(sigma, bf16, m=M):
    key = (sigma, bf16, m)
    if key not in _sets:
        _sets[key] = dqn_ref.synthetic(int(sigma * 10) + 100 * bf16 + m % 997, m, sigma, bf16=bf16)
    return _sets[key]


def _note(sh):
    for k, v in sh.items():
        _shares[k] = max(_shares.get(k, 0.0), float(v))


CONFIGS = [(flags_mask | flags_loss | dqn_ref.TIMEOUT_EXCLUDE * tmo, double, rew)
           for flags_mask in (0, dqn_ref.MASK_NEXT) for flags_loss in (0, dqn_ref.MSE) for double in (False, True)
           for tmo, rew in ((1, False), (0, True))]


# ---------------------------------------------------------------- the reference alone

@pytest.mark.parametrize("sigma", head_ref.SIGMAS)
def test_the_contract_is_within_its_bounds_of_sb3(sigma):
    """(a) against (b) on 4 096-row sets with the hand-made rows, every flag combination, plain and double, both reward sources."""
    c = _set(sigma, False, 4096)
    for flags, double, rew in CONFIGS:
        ct = dqn_ref.Contract(c, GAMMA, flags, double, rew)
        _note(dqn_ref.check_contract_against_sb3(c, ct, f"sigma {sigma} flags {flags} double {double} rewards {rew}"))
        assert 0.02 < ct.done.mean() < 0.09 and ct.excluded.sum() >= 8
    print(f"sigma {sigma}: largest shares of (a) against (b) so far {_shares}")


def test_hand_made_rows_of_the_reference():
    """The hand-made rows take the branches they were made for."""
    c = _set(1.0, False, 300)
    h0 = c.m - dqn_ref.HAND_ROWS
    hand = lambda ct: set((np.flatnonzero(ct.excluded[h0:])).tolist())   # noqa: E731
    full = dqn_ref.MASK_NEXT | dqn_ref.TIMEOUT_EXCLUDE
    ct = dqn_ref.Contract(c, GAMMA, full, False)
    assert hand(ct) == {9, 10, 11, 12, 13, 14, 15, 16, 17, 20, 22, 23, 24, 26}
    one = np.float32(1.0)
    assert [float(x) for x in ct.d[h0:h0 + 6]] == [1.0, float(np.nextafter(one, np.float32(0))), float(np.nextafter(one, np.float32(2))), -1.0,
                                                  -float(np.nextafter(one, np.float32(0))), -float(np.nextafter(one, np.float32(2)))]
    assert [float(x) for x in ct.g[h0:h0 + 6]] == [1.0, float(ct.d[h0 + 1]), 1.0, -1.0, float(ct.d[h0 + 4]), -1.0]
    assert ct.term[h0] == np.float32(0.5) and ct.term[h0 + 2] == ct.d[h0 + 2] - np.float32(0.5) and ct.term[h0 + 1] < np.float32(0.5)
    assert ct.n[h0 + 6] == 1.5 and ct.n[h0 + 7] == 1.5 and ct.included[h0 + 8] and ct.y[h0 + 8] == 1.0 and ct.included[h0 + 21] and ct.included[h0 + 25]
    assert ct.included[h0 + 18] and ct.included[h0 + 19] and ct.y[h0 + 18] == -1.0
    ctd = dqn_ref.Contract(c, GAMMA, full, True)
    assert ctd.arg[h0 + 6] == 11 and ctd.n[h0 + 6] == 0.25 and ctd.arg[h0 + 7] == 30 and ctd.n[h0 + 7] == 0.75 and ctd.excluded[h0 + 26] and ctd.excluded[h0 + 24]
    assert {9, 10, 11, 12, 13, 14, 15, 16, 17, 20, 22, 24, 26} <= hand(ctd)
    ct0 = dqn_ref.Contract(c, GAMMA, 0, False)
    assert hand(ct0) == {10, 11, 12, 13, 14, 15, 16, 20, 21, 22, 23, 24, 26} and ct0.y[h0 + 17] == -1.0
    ctm = dqn_ref.Contract(c, GAMMA, full | dqn_ref.MSE, False, True)
    assert hand(ctm) == hand(ct) and ctm.g[h0] == 2 * ctm.d[h0] and ctm.term[h0] == ctm.d[h0] * ctm.d[h0]
    assert np.isnan(ct.td[h0 + 9]) and ct.td.view(np.uint32)[h0 + 9] == dqn_ref.QNAN_BITS and (ct.dq[h0 + 9] == 0).all()


# ---------------------------------------------------------------- the header on the host

@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("sigma", head_ref.SIGMAS)
def test_synthetic_sets_are_the_contract_bit_for_bit(host, sigma, bf16):
    c = _set(sigma, bf16)
    worst = 0.0
    for flags, double, rew in CONFIGS:
        what = f"sigma {sigma} bf16 {bf16} flags {flags} double {double} rewards {rew}"
        ct = dqn_ref.Contract(c, GAMMA, flags, double, rew)
        dq, td, st = host.run(c, flags, double, rew, stride=64 if flags & dqn_ref.MSE else 60)
        worst = max(worst, ct.check(dq, td, st, what))
        if bf16:   # the same values through bfloat16 storage: the gradient is the float32 one rounded to nearest even, everything else the same bits
            dqb, tdb, stb = host.run(c, flags, double, rew, bf16=True, stride=64)
            assert dqb.dtype == np.uint16 and np.array_equal(dqb, head_ref.bf16_bits(dq)), what
            assert np.array_equal(tdb.view(np.uint32), td.view(np.uint32)) and np.array_equal(stb.view(np.uint32), st.view(np.uint32)), what
    _note({"scalars": worst})
    print(f"sigma {sigma} bf16 {bf16}: largest share of a scalar bound {worst:.3f}")


@pytest.mark.parametrize("flags,double,rew", [(5, False, False), (5, True, True), (2, False, True), (1, True, False)])
def test_the_twins_second_level_fold(host, flags, double, rew):
    """m = 16 449: 258 row partials, two per lane of the finishing fold.  Two runs give the same bits; td_dev may be NULL."""
    assert -(-M_FOLD // 64) == 258 and -(-258 // 256) == 2
    c = _set(3.0, False, M_FOLD)
    ct = dqn_ref.Contract(c, GAMMA, flags, double, rew)
    dq, td, st = host.run(c, flags, double, rew)
    share = ct.check(dq, td, st, f"fold flags {flags} double {double}")
    dq2, td2, st2 = host.run(c, flags, double, rew, with_td=False)
    assert td2 is None and np.array_equal(dq.view(np.uint32), dq2.view(np.uint32)) and np.array_equal(st.view(np.uint32), st2.view(np.uint32))
    assert st[7] == M_FOLD and st[6] == ct.excluded.sum() > 0
    print(f"fold: share {share:.3f}")


def test_hand_made_rows_on_the_host(host):
    for m in (33, 300):
        c = _set(1.0, False, m)
        for flags, double, rew in CONFIGS:
            ct = dqn_ref.Contract(c, GAMMA, flags, double, rew)
            dq, td, st = host.run(c, flags, double, rew)
            ct.check(dq, td, st, f"hand-made m {m} flags {flags} double {double} rewards {rew}")
            assert st[6] >= 8


# ---------------------------------------------------------------- epsilon-greedy

@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_epsilon_greedy_row_function(host, masked):
    """Bit for bit the Python-integer restatement on every row at epsilon 0, 0.05, 0.5, 1; epsilon 0 is the deterministic rule, epsilon 1 never takes
    the greedy branch, and the share of exploring rows is within four binomial standard deviations of epsilon."""
    logits, mask = head_ref.synthetic(17 + masked, M, 3.0, masked)
    logits[5, :] = np.nan
    logits[6, 3] = np.inf
    logits[7, :] = -np.inf
    if masked:
        mask[8, :] = 0
        mask[9, :] = 0; mask[9, 59] = 1
        mask[6, 3] = 0   # the +inf logit is masked: the row is live
    seed, index0, t = 0xC0FFEE12345, 1 << 40, 77
    for eps in (0.0, 0.05, 0.5, 1.0):
        a, greedy = host.eps(logits, mask, seed, index0, t, eps)
        want, explored = dqn_ref.eps_actions(logits, mask, seed, index0, t, eps)
        assert np.array_equal(a, want), (eps, np.flatnonzero(a != want)[:5])
        assert a[5] == -1 and a[7] == -1 and (a[6] == -1) == (not masked) and (not masked or (a[8] == -1 and a[9] == 59))
        live = a >= 0
        assert not masked or (mask[np.arange(M)[live], a[live]] != 0).all()
        if eps == 0.0:
            assert np.array_equal(a, greedy) and not explored.any()
        if eps == 1.0:
            assert explored.all()
            h2 = np.array([head_ref.policy_hash_scalar((seed + dqn_ref.EPS_SALT) & (2 ** 64 - 1), index0 + i, t) for i in range(M)], dtype=np.uint64)
            k = (mask != 0).sum(axis=1).astype(np.uint64) if masked else np.full(M, 60, np.uint64)
            pick = (h2 * k) >> np.uint64(32)
            order = np.cumsum(mask != 0, axis=1) - 1 if masked else np.tile(np.arange(60), (M, 1))
            assert (order[np.arange(M)[live], a[live]] == pick[live]).all(), "epsilon 1: every live row takes the pick-th valid action, never the greedy branch"
            assert (a[live] != greedy[live]).mean() > 0.9
        sd = np.sqrt(eps * (1 - eps) / M)
        assert abs(explored.mean() - eps) <= 4 * sd + 1e-12, (eps, explored.mean(), sd)
    # the row does not depend on the batch: a slice with index0 moved gives the same actions
    a, _ = host.eps(logits, mask, seed, index0, t, 0.5)
    b, _ = host.eps(logits[1000:1300], None if mask is None else mask[1000:1300], seed, index0 + 1000, t, 0.5)
    assert np.array_equal(a[1000:1300], b)


# ---------------------------------------------------------------- RowReplay

def _stamp(replay, step, n, stride):
    import torch
    r = torch.zeros((n, stride), dtype=torch.uint8)
    r[:, 0] = step % 251
    r[:, 1] = torch.arange(n, dtype=torch.uint8)
    r[:, 8:16] = torch.tensor([step], dtype=torch.int64).view(torch.uint8)
    return r


def test_row_replay_on_the_cpu():
    import torch
    from balatro_gym_amd import RowReplay
    Cn, N, stride = 5, 3, 352
    rp = RowReplay(Cn, N, "cpu", row_stride=stride)
    assert tuple(rp.store.shape) == (Cn, N, stride) and rp.store.dtype == torch.uint8 and rp.store.data_ptr() % 128 == 0 and rp.store.is_contiguous()
    assert len(rp) == 0
    with pytest.raises(ValueError, match="no transition"):
        rp.sample(4)
    with pytest.raises(ValueError, match="start"):
        rp.add(torch.zeros((1, N, stride), dtype=torch.uint8))
    step = 0
    rp.start(_stamp(rp, step, N, stride))
    assert len(rp) == 0
    with pytest.raises(ValueError, match="no transition"):
        rp.sample(4)

    def stamp_of(flat_index):
        rec = rp.store.view(-1, stride)[flat_index.long()]
        return rec[:, 8:16].contiguous().view(torch.int64)[:, 0], rec[:, 1].long()
    gen = torch.Generator().manual_seed(3)
    for K in (2, 1, 4, 3, 4, 1, 2):   # the ring wraps several times, at different heads
        rows = torch.stack([_stamp(rp, step + 1 + k, N, stride) for k in range(K)])
        rp.add(rows)
        step += K
        filled = min(step + 1, Cn)
        assert len(rp) == (filled - 1) * N
        idx, nxt = rp.sample(200_000 if K == 4 and step > 8 else 4000, generator=gen)
        assert idx.dtype == torch.int32 and nxt.dtype == torch.int32 and tuple(idx.shape) == tuple(nxt.shape)
        s0, e0 = stamp_of(idx)
        s1, e1 = stamp_of(nxt)
        assert bool((s1 == s0 + 1).all()) and bool((e0 == e1).all()), "a sampled pair is two consecutive steps of one env"
        assert bool((idx % N == e0).all()) and bool((nxt // N == (idx // N + 1) % Cn).all())
        head = (step + 1) % Cn
        assert int(s1.max()) == step and int(s0.min()) == step + 1 - filled, "the newest and the oldest record are both reached"
        assert not bool((nxt // N == head).any()), "the write head is never a successor"
        assert not bool(((idx // N) == (head - 1) % Cn).any()), "the newest record has no successor yet: the write head is never a successor"
        pairs = set(zip((idx // N).tolist(), (idx % N).tolist()))
        valid = {((head - 1 - j) % Cn if filled == Cn else filled - 1 - j, e) for j in range(1, filled) for e in range(N)}
        assert pairs <= valid
        if idx.numel() == 200_000:
            assert pairs == valid and len(valid) == (Cn - 1) * N, "over 200 000 draws every valid (slot, env) pair is drawn"
            counts = torch.bincount((idx // N) * N + idx % N, minlength=Cn * N).double()
            exp = 200_000 / len(valid)
            assert bool(((counts[counts > 0] - exp).abs() < 6 * np.sqrt(exp)).all()), "uniform over the valid pairs"
    with pytest.raises(ValueError, match="K = 5"):
        rp.add(torch.zeros((Cn, N, stride), dtype=torch.uint8))
    for bad in (torch.zeros((1, N + 1, stride), dtype=torch.uint8), torch.zeros((1, N, stride)), torch.zeros((N, stride), dtype=torch.uint8), "rows"):
        with pytest.raises(ValueError, match="rows_kn must be"):
            rp.add(bad)
    with pytest.raises(ValueError, match="obs_rows must be"):
        rp.start(torch.zeros((N, 384), dtype=torch.uint8))
    # state_dict round trip into a fresh ring: the same store, the same draws
    sd = rp.state_dict()
    other = RowReplay(Cn, N, "cpu", row_stride=stride)
    other.load_state_dict(sd)
    assert torch.equal(other.store, rp.store) and len(other) == len(rp)
    a = rp.sample(1000, generator=torch.Generator().manual_seed(9))
    b = other.sample(1000, generator=torch.Generator().manual_seed(9))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    sd["store"][0, 0, 0] += 1
    assert not torch.equal(sd["store"], rp.store), "state_dict holds a copy"
    with pytest.raises(ValueError, match="ring"):
        RowReplay(Cn + 1, N, "cpu", row_stride=stride).load_state_dict(sd)
    rp.clear()
    assert len(rp) == 0
    with pytest.raises(ValueError, match="no transition"):
        rp.sample(1)
    for kw in (dict(capacity_steps=1, n=3), dict(capacity_steps=4, n=0), dict(capacity_steps=4, n=3, row_stride=360), dict(capacity_steps=4, n=3, row_stride=336),
               dict(capacity_steps=2 ** 16, n=2 ** 15)):
        with pytest.raises(ValueError):
            RowReplay(device="cpu", **kw)


# ---------------------------------------------------------------- declarations and wrappers

def test_header_declares_and_library_exports_dqn():
    from balatro_gym_amd import _native as nat, build
    import balatro_gym_amd
    hdr = open(HEADER).read()
    m = re.search(r"\bint\s+bg_dqn_loss\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/balatro_mi355x.h does not declare bg_dqn_loss"
    params = [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", p).strip()) for p in m.group(1).split(",")]
    assert params == ["const void* q_dev", "uint64_t q_stride_elems", "const void* q_next_dev", "uint64_t q_next_stride_elems", "const void* q_next_online_dev",
                      "uint64_t q_next_online_stride_elems", "int q_dtype", "const uint8_t* rows_dev", "uint64_t row_stride_bytes", "int64_t store_rows",
                      "const int32_t* next_index_dev", "const float* rewards_dev", "int64_t m", "float gamma", "uint32_t flags", "void* dq_dev",
                      "uint64_t dq_stride_elems", "float* td_dev", "float* stats_dev", "void* workspace_dev", "uint64_t workspace_bytes", "float* kernel_ms_out",
                      "void* stream"], params
    assert len(params) == len(nat_argtypes_of("bg_dqn_loss"))
    m = re.search(r"\bint\s+bg_sample_actions_eps\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/balatro_mi355x.h does not declare bg_sample_actions_eps"
    eps_params = [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", p).strip()) for p in m.group(1).split(",")]
    m0 = re.search(r"\bint\s+bg_sample_actions\s*\(([^;]*)\)\s*;", hdr)
    base = [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", p).strip()) for p in m0.group(1).split(",")]
    assert eps_params == base[:10] + ["float epsilon"] + base[10:], "bg_sample_actions' arguments plus epsilon"
    assert re.search(r"uint64_t\s+bg_dqn_loss_workspace_bytes\s*\(\s*int64_t m\s*\)\s*;", hdr)
    for name, val in (("BG_DQN_STATS", "8"), ("BG_DQN_MASK_NEXT", "1u"), ("BG_DQN_MSE", "2u"), ("BG_DQN_TIMEOUT_EXCLUDE", "4u")):
        assert re.search(rf"#define {name} {val}\b", hdr), name
    doc = hdr[:hdr.index("#define BG_DQN_STATS")].rsplit("\n/*", 1)[1]
    for cite in ("train_balatro_agent.py:344-362", "smooth_l1", "copysign(1, d)", "EXCLUDED", "the divisor stays m", "same bits", "terminal_observation",
                 "bg_dqn_loss: ", "0x632BE59BD9B4E019", "per env", "out of scope"):
        assert cite in doc, cite
    assert nat.DQN_STATS == dqn_ref.STATS and (nat.DQN_MASK_NEXT, nat.DQN_MSE, nat.DQN_TIMEOUT_EXCLUDE) == (1, 2, 4)
    for e in ("bg_dqn_loss", "bg_dqn_loss_workspace_bytes", "bg_sample_actions_eps"):
        assert e in nat.EXPORTS
    assert os.path.join(CSRC, "bg_dqn.h") in build.DEPS
    assert '#include "bg_dqn.h"' in open(os.path.join(CSRC, "bg_lib.hip")).read()
    for name in ("dqn_loss", "RowReplay", "DqnStats"):
        assert name in balatro_gym_amd.__all__ and callable(getattr(balatro_gym_amd, name))
    if os.path.exists(build.LIB):
        L = C.CDLL(build.LIB)
        assert hasattr(L, "bg_dqn_loss") and hasattr(L, "bg_sample_actions_eps")
        L.bg_dqn_loss_workspace_bytes.restype = C.c_uint64
        L.bg_dqn_loss_workspace_bytes.argtypes = [C.c_int64]
        assert L.bg_dqn_loss_workspace_bytes(0) == 0 and L.bg_dqn_loss_workspace_bytes(64) == 56 and L.bg_dqn_loss_workspace_bytes(65) == 112


def nat_argtypes_of(name):
    """The ctypes argument list `_native` binds for `name`, read from its source (binding needs the built library)."""
    src = open(os.path.join(ROOT, "balatro_gym_amd", "_native.py")).read()
    m = re.search(rf"L\.{name}\.argtypes = \[(.*?)\]\n", src, re.S)
    assert m, name
    return [x for x in re.sub(r"C\.POINTER\(C\.c_float\)", "fp", m.group(1)).replace("\n", " ").split(",") if x.strip()]


def test_wrappers_refuse_bad_arguments_before_the_library():
    """dqn_loss and sample_actions(epsilon=) on CPU tensors: every bad argument is a ValueError raised before anything is loaded."""
    import torch
    from balatro_gym_amd import dqn_loss, sample_actions
    N, S = 6, 11
    q = torch.zeros((N, 60))
    rows = torch.zeros((S, 384), dtype=torch.uint8)
    nx = torch.zeros(N, dtype=torch.int32)
    for bad in (q.double(), torch.zeros((N, 59)), "q", None):
        with pytest.raises(ValueError, match=r"float32 or bfloat16 tensor \[\.\.\., 60\]"):
            dqn_loss(bad, q, rows, nx)
    with pytest.raises(ValueError, match="dense over its row pitch"):
        dqn_loss(torch.zeros((N, 120))[:, ::2], q, rows, nx)
    for bad in (q.to(torch.bfloat16), torch.zeros((N + 1, 60)), None, torch.zeros((N, 59))):
        with pytest.raises(ValueError, match="q_next must|float32 or bfloat16 tensor"):
            dqn_loss(q, bad, rows, nx)
        if bad is not None:
            with pytest.raises(ValueError, match="q_next_online must|float32 or bfloat16 tensor"):
                dqn_loss(q, q, rows, nx, q_next_online=bad)
    for bad in (torch.zeros((S, 360), dtype=torch.uint8), torch.zeros((S, 336), dtype=torch.uint8), torch.zeros((S, 384)), torch.zeros(384, dtype=torch.uint8),
                torch.zeros((S, 768), dtype=torch.uint8)[:, ::2], None):
        with pytest.raises(ValueError, match="rows must be|record stride"):
            dqn_loss(q, q, bad, nx)
    for bad in (nx.long(), torch.zeros(N + 1, dtype=torch.int32), torch.zeros(2 * N, dtype=torch.int32)[::2], "index", None):
        with pytest.raises(ValueError, match="next_index must be a contiguous"):
            dqn_loss(q, q, rows, bad)
    for bad in (torch.zeros(S, dtype=torch.float64), torch.zeros(S + 1), torch.zeros(N)):
        with pytest.raises(ValueError, match="rewards must be a contiguous"):
            dqn_loss(q, q, rows, nx, rewards=bad)
    for bad in (-0.1, 1.5, float("nan"), float("inf"), "g", True):
        with pytest.raises(ValueError, match="gamma must be"):
            dqn_loss(q, q, rows, nx, gamma=bad)
    with pytest.raises(ValueError, match="loss must be"):
        dqn_loss(q, q, rows, nx, loss="l1")
    with pytest.raises(ValueError, match="timeouts must be"):
        dqn_loss(q, q, rows, nx, timeouts="bootstrap")
    # everything right: what is left is that there is no CPU path
    for kw in ({}, dict(q_next_online=q, rewards=torch.zeros(S), gamma=0.5, mask_next=False, loss="mse", timeouts="terminal")):
        with pytest.raises(ValueError, match="device tensor"):
            dqn_loss(q, q, rows, nx, **kw)
    with pytest.raises(ValueError, match="device tensor"):
        dqn_loss(q.view(2, 3, 60), q.view(2, 3, 60), rows.view(1, S, 384), nx.view(2, 3), rewards=torch.zeros((1, S)))
    # epsilon
    for bad in (-0.01, 1.01, float("nan"), "e", True):
        with pytest.raises(ValueError, match="epsilon must be"):
            sample_actions(q, seed=1, t=0, epsilon=bad)
    with pytest.raises(ValueError, match="exclude each other"):
        sample_actions(q, seed=1, t=0, epsilon=0.1, deterministic=True)
    for kw in (dict(log_prob=torch.zeros(N)), dict(entropy=torch.zeros(N))):
        with pytest.raises(ValueError, match="no categorical log_prob"):
            sample_actions(q, seed=1, t=0, epsilon=0.1, **kw)
    with pytest.raises(ValueError, match="actions must be"):
        sample_actions(q, seed=1, t=0, epsilon=0.1, actions=torch.zeros(N))
    with pytest.raises(ValueError, match=r"seed must be an integer"):
        sample_actions(q, seed=-1, t=0, epsilon=0.1)
    for mask in (None, torch.zeros((N, 384), dtype=torch.uint8), torch.ones((N, 60), dtype=torch.int8)):
        with pytest.raises(ValueError, match="device tensor"):
            sample_actions(q, mask, seed=1, t=0, epsilon=0.1)
