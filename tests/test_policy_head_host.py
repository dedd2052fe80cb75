"""bg_sample_actions / bg_evaluate_actions on the CPU (no GPU): csrc/bg_head.h -- the per-row arithmetic of the policy head, the very text the kernel
runs -- is compiled with g++ (-O1 -ffp-contract=off -DBG_HEAD_HOST) into a small program that walks rows from a file, and held to the float64 numpy
restatement of tests/head_ref.py by the bounds derived there: the synthetic sets in all three modes, bf16 widening, every kind of degenerate row, the
evaluate mode's masked and out-of-range actions, the hash bit for bit, and the frequencies of 65 536 draws from one row.  Also: the header's declarations
and citations, the exports, build.DEPS, and the argument checks of the Python wrappers.

Largest observed shares of the bounds with g++ and glibc's expf / logf: log_prob 0.10, entropy 0.08; undecidable rows at most 0.18 % of a set."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import head_ref as ref
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")
SAMPLE, ARGMAX, EVALUATE = 0, 1, 2

_PROGRAM = r"""
#define BG_HEAD_HOST
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "balatro_mi355x.h"
#include "bg_head.h"
template <int MODE>
static BgHeadOut row(bool masked, const float* l, const uint8_t* bytes, float u, int32_t given) {
  float P[BG_HEAD_ACTIONS];
  uint32_t k[BG_HEAD_ACTIONS / 4] = {};
  if (masked) memcpy(k, bytes, BG_HEAD_ACTIONS);
  return masked ? bg_head_row<MODE, true>(l, k, P, u, given) : bg_head_row<MODE, false>(l, k, P, u, given);
}
int main(int argc, char** argv) {
  if (argc == 7 && !strcmp(argv[1], "hash")) {   // hash seed index0 t count out
    const uint64_t seed = strtoull(argv[2], 0, 10), i0 = strtoull(argv[3], 0, 10), t = strtoull(argv[4], 0, 10), n = strtoull(argv[5], 0, 10);
    FILE* out = fopen(argv[6], "wb");
    for (uint64_t i = 0; i < n; i++) { const uint32_t h = bg_head_hash(seed, i0 + i, t); fwrite(&h, 4, 1, out); }
    fclose(out);
    return 0;
  }
  if (argc != 10) return 2;   // mode bf16 masked m seed index0 t in out;  in = logits | mask bytes (masked) | int32 actions (evaluate)
  const int mode = atoi(argv[1]), bf16 = atoi(argv[2]), masked = atoi(argv[3]);
  const size_t m = strtoull(argv[4], 0, 10), W = BG_HEAD_ACTIONS;
  const uint64_t seed = strtoull(argv[5], 0, 10), i0 = strtoull(argv[6], 0, 10), t = strtoull(argv[7], 0, 10);
  const size_t lbytes = m * W * (bf16 ? 2 : 4), bytes = lbytes + (masked ? m * W : 0) + (mode == BG_HEAD_EVALUATE ? m * 4 : 0);
  uint8_t* in = (uint8_t*)malloc(bytes + 16);
  FILE* f = fopen(argv[8], "rb");
  if (!f || fread(in, 1, bytes, f) != bytes) return 4;
  fclose(f);
  const uint8_t* mask = in + lbytes;
  const uint8_t* given = mask + (masked ? m * W : 0);
  int32_t* act = (int32_t*)malloc(m * 4 + 4);
  float* lp = (float*)malloc(m * 4 + 4);
  float* en = (float*)malloc(m * 4 + 4);
  for (size_t i = 0; i < m; i++) {
    float l[BG_HEAD_ACTIONS];
    for (size_t j = 0; j < W; j++) {
      if (bf16) { uint16_t b; memcpy(&b, in + (i * W + j) * 2, 2); l[j] = bg_head_widen_bf16(b); }
      else memcpy(&l[j], in + (i * W + j) * 4, 4);
    }
    int32_t g = 0;
    if (mode == BG_HEAD_EVALUATE) memcpy(&g, given + i * 4, 4);
    const float u = bg_head_u(bg_head_hash(seed, i0 + i, t));
    const uint8_t* k = mask + i * W;
    const BgHeadOut o = mode == BG_HEAD_SAMPLE ? row<BG_HEAD_SAMPLE>(masked, l, k, u, g) : mode == BG_HEAD_ARGMAX ? row<BG_HEAD_ARGMAX>(masked, l, k, u, g)
                                                                                                                   : row<BG_HEAD_EVALUATE>(masked, l, k, u, g);
    act[i] = o.action; lp[i] = o.log_prob; en[i] = o.entropy;
  }
  FILE* out = fopen(argv[9], "wb");
  if (!out || fwrite(act, 4, m, out) != m || fwrite(lp, 4, m, out) != m || fwrite(en, 4, m, out) != m) return 5;
  fclose(out);
  return 0;
}
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile csrc/bg_head.h for the host"
    d = tmp_path_factory.mktemp("head_host")
    src = d / "head_host.cpp"
    src.write_text(_PROGRAM)
    exe = d / "head_host"
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-I", CSRC, "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])

    class Host:
        @staticmethod
        def run(mode, logits, mask=None, *, seed=0, index0=0, t=0, actions=None):
            """logits: float32 [m, 60], or uint16 bfloat16 bits.  Returns (actions int32, log_prob float32, entropy float32)."""
            logits = np.ascontiguousarray(logits)
            assert logits.dtype in (np.float32, np.uint16) and logits.shape[1] == 60
            m = logits.shape[0]
            blob = logits.tobytes()
            if mask is not None:
                blob += np.ascontiguousarray(mask, np.int8).tobytes()
            if mode == EVALUATE:
                blob += np.ascontiguousarray(actions, np.int32).tobytes()
            (d / "in.bin").write_bytes(blob)
            subprocess.check_call([str(exe), str(mode), str(int(logits.dtype == np.uint16)), str(int(mask is not None)), str(m), str(seed), str(index0), str(t),
                                   str(d / "in.bin"), str(d / "out.bin")])
            b = (d / "out.bin").read_bytes()
            return np.frombuffer(b[:4 * m], np.int32), np.frombuffer(b[4 * m:8 * m], np.float32), np.frombuffer(b[8 * m:], np.float32)

        @staticmethod
        def hash(seed, index0, t, n):
            subprocess.check_call([str(exe), "hash", str(seed), str(index0), str(t), str(n), str(d / "hash.bin")])
            return np.fromfile(str(d / "hash.bin"), np.uint32)
    return Host


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("sigma", ref.SIGMAS)
def test_synthetic_sets_in_all_three_modes(host, sigma, masked):
    m, seed, index0, t = 16384, 0x1234_5678_9ABC_DEF0, 3_000_000_000, 41
    logits, mask = ref.synthetic(int(sigma * 10) + masked, m, sigma, masked)
    r = ref.Reference(logits, mask, seed, index0, t)
    a, lp, en = host.run(SAMPLE, logits, mask, seed=seed, index0=index0, t=t)
    und = r.check_sampled(a, "sample")
    s_lp, s_en = r.check_stats(a, lp, en, "sample")
    print(f"sigma {sigma} masked {masked}: undecidable {und:.5f}, log_prob share {s_lp:.3f}, entropy share {s_en:.3f}")
    a1, lp1, en1 = host.run(ARGMAX, logits, mask)
    r.check_mode(a1, "deterministic")
    r.check_stats(a1, lp1, en1, "deterministic")
    assert np.array_equal(_bits(en1), _bits(en)), "the entropy does not depend on the mode"
    # evaluate: the sampled actions give the sampler's bits back; arbitrary actions (masked ones included) hold the bounds
    a2, lp2, en2 = host.run(EVALUATE, logits, mask, actions=a)
    assert np.array_equal(_bits(lp2), _bits(lp)) and np.array_equal(_bits(en2), _bits(en))
    given = np.random.default_rng(5).integers(0, 60, m).astype(np.int32)
    _, lp3, en3 = host.run(EVALUATE, logits, mask, actions=given)
    r.check_stats(given, lp3, en3, "evaluate")
    if masked:
        assert np.isneginf(lp3).sum() == (mask[np.arange(m), given] == 0).sum() > m // 4


def test_result_is_a_function_of_the_global_index(host):
    logits, mask = ref.synthetic(77, 500, 3.0, True)
    full = host.run(SAMPLE, logits, mask, seed=9, index0=100, t=7)
    part = host.run(SAMPLE, logits[123:381], mask[123:381], seed=9, index0=223, t=7)
    for f, p in zip(full, part):
        assert np.array_equal(f[123:381].view(np.uint32), p.view(np.uint32))
    other = host.run(SAMPLE, logits, mask, seed=9, index0=100, t=8)
    assert (other[0] != full[0]).mean() > 0.5


def test_bf16_logits_are_widened_exactly(host):
    logits, mask = ref.synthetic(3, 4096, 3.0, True)
    b = ref.bf16_bits(logits)
    wide = ref.widen_bf16(b)
    assert np.array_equal(ref.bf16_bits(wide), b) and not np.array_equal(wide, logits)
    got = host.run(SAMPLE, b, mask, seed=5, t=2)
    same = host.run(SAMPLE, wide, mask, seed=5, t=2)
    for g, s in zip(got, same):
        assert np.array_equal(g.view(np.uint32), s.view(np.uint32))
    r = ref.Reference(wide, mask, 5, 0, 2)
    r.check_sampled(got[0], "bf16")
    r.check_stats(*got, "bf16")


def degenerate_cases():
    """logits [9, 60], mask [9, 60]: rows 0-4 degenerate, rows 5-8 live with special values."""
    rng = np.random.default_rng(11)
    l = rng.standard_normal((9, 60)).astype(np.float32)
    k = (rng.random((9, 60)) >= 0.4).astype(np.int8)
    k[:, 7] = 1
    k[:, 9] = 0
    k[0] = 0                                   # no valid action
    l[1, 7] = np.nan                           # a valid NaN
    l[2, 7] = np.inf                           # a valid +inf
    l[3] = -np.inf                             # every valid logit -inf
    l[4] = np.where(k[4] != 0, -np.inf, 1.0)   # every VALID logit -inf, the masked ones finite
    l[5, 9] = np.nan                           # masked NaN: ignored
    l[6, 9] = np.inf                           # masked +inf: ignored
    l[7, 7] = -np.inf                          # a valid -inf beside finite logits: probability 0
    l[8] = -np.inf; l[8, 7] = -3.0e38          # one finite valid logit: it is certain
    return l, k


def test_degenerate_rows(host):
    l, k = degenerate_cases()
    r = ref.Reference(l, k, 1, 0, 0)
    assert r.degenerate.tolist() == [True] * 5 + [False] * 4
    for mode in (SAMPLE, ARGMAX, EVALUATE):
        for tt in range(50):
            a, lp, en = host.run(mode, l, k, seed=1, t=tt, actions=np.full(9, 7, np.int32))
            if mode != EVALUATE:
                assert a[:5].tolist() == [-1] * 5 and (a[5:] >= 0).all() and (k[np.arange(5, 9), a[5:]] != 0).all()
                assert a[7] != 7, "an action of probability 0 was drawn"
                assert a[8] == 7
            assert _bits(lp)[:5].tolist() == [ref.QNAN_BITS] * 5 == _bits(en)[:5].tolist()
            assert np.isfinite(en[5:]).all() and (np.isfinite(lp[5:]) | (mode == EVALUATE)).all()
            assert en[8] == 0.0 and (mode == EVALUATE or lp[8] == 0.0)
            if mode == EVALUATE:
                assert np.isneginf(lp[7]) and lp[8] == 0.0   # the valid -inf logit: log 0
    # all valid, one row of the unmasked path with a NaN
    l2 = l.copy()
    a, lp, en = host.run(SAMPLE, l2, None, seed=1)
    assert a[[1, 2, 3, 5, 6]].tolist() == [-1] * 5 and a[0] >= 0 and a[4] >= 0


def test_evaluate_masked_and_out_of_range_actions(host):
    logits, mask = ref.synthetic(21, 256, 1.0, True)
    r = ref.Reference(logits, mask)
    given = np.random.default_rng(2).integers(0, 60, 256).astype(np.int32)
    given[:8] = [-1, 60, 61, -2 ** 31, 2 ** 31 - 1, 255, -60, 1 << 20]
    _, lp, en = host.run(EVALUATE, logits, mask, actions=given)
    assert _bits(lp)[:8].tolist() == [ref.QNAN_BITS] * 8
    hidden = mask[np.arange(256), np.clip(given, 0, 59)] == 0
    hidden[:8] = False
    assert hidden.sum() > 50 and np.isneginf(lp[hidden]).all() and np.isfinite(lp[8:][~hidden[8:]]).all()
    r.check_stats(given, lp, en, "evaluate")
    assert np.array_equal(_bits(en), _bits(host.run(SAMPLE, logits, mask)[2])), "the entropy is unchanged by the given action"
    _, lp_u, _ = host.run(EVALUATE, logits, None, actions=given)
    assert np.isfinite(lp_u[8:]).all() and _bits(lp_u)[:8].tolist() == [ref.QNAN_BITS] * 8


def test_hash_matches_numpy_bit_for_bit(host):
    for seed, i0, t in ((0, 0, 0), (1, 2, 3), (2 ** 64 - 1, 2 ** 64 - 5, 2 ** 64 - 1), (0xDEADBEEF12345678, 1 << 40, 1 << 33)):
        got = host.hash(seed, i0, t, 4096)
        idx = (np.uint64(i0) + np.arange(4096, dtype=np.uint64))
        assert np.array_equal(got, ref.policy_hash(seed, idx, t))
        for i in (0, 1, 7, 4095):
            assert int(got[i]) == ref.policy_hash_scalar(seed, (i0 + i) & (2 ** 64 - 1), t)
    u = ref.uniform(got)
    assert u.min() >= 0.0 and u.max() < 1.0 and np.array_equal(u.astype(np.float32).astype(np.float64), u)


def test_frequencies_of_one_row(host):
    """One row replicated 65 536 times, index0 + i varying: every action with M p >= 5 is drawn within 6 sqrt(M p (1 - p)) + 1 of M p times, a masked
    one never.  Deterministic: it passes always or never (the numpy reference's own draws have max z = 1.9)."""
    M = 65536
    rng = np.random.default_rng(8)
    row = (rng.standard_normal(60) * 2.0).astype(np.float32)
    mk = (rng.random(60) >= 0.4).astype(np.int8)
    logits, mask = np.tile(row, (M, 1)), np.tile(mk, (M, 1))
    r = ref.Reference(logits, mask, 99, 12345, 6)
    a, _, _ = host.run(SAMPLE, logits, mask, seed=99, index0=12345, t=6)
    counts = np.bincount(a, minlength=60)
    p = r.e[0] / r.S[0]
    assert counts[mk == 0].sum() == 0
    big = M * p >= 5
    assert big.sum() >= 15
    dev = np.abs(counts - M * p)
    assert (dev[big] <= 6 * np.sqrt(M * p * (1 - p))[big] + 1).all(), (counts, M * p)


def test_header_declares_and_library_exports_the_head():
    from balatro_gym_amd import _native as nat, build
    import balatro_gym_amd
    hdr = open(HEADER).read()
    m = re.search(r"\bint\s+bg_sample_actions\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/balatro_mi355x.h does not declare bg_sample_actions"
    params = [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", p).strip()) for p in m.group(1).split(",")]
    assert params == ["const void* logits_dev", "int logits_dtype", "uint64_t logits_stride_elems", "const int8_t* mask_dev", "uint64_t mask_stride_bytes",
                      "int64_t m", "uint32_t flags", "uint64_t seed", "uint64_t index0", "uint64_t t", "int32_t* actions_dev", "float* log_prob_dev",
                      "float* entropy_dev", "float* kernel_ms_out", "void* stream"], params
    m = re.search(r"\bint\s+bg_evaluate_actions\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/balatro_mi355x.h does not declare bg_evaluate_actions"
    params = [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", p).strip()) for p in m.group(1).split(",")]
    assert params == ["const void* logits_dev", "int logits_dtype", "uint64_t logits_stride_elems", "const int8_t* mask_dev", "uint64_t mask_stride_bytes",
                      "int64_t m", "const int32_t* actions_dev", "float* log_prob_dev", "float* entropy_dev", "float* kernel_ms_out", "void* stream"], params
    for name, val in (("BG_HEAD_F32", "0"), ("BG_HEAD_BF16", "1"), ("BG_HEAD_DETERMINISTIC", "1u"), ("BG_ROW_ACTION_MASK", "176")):
        assert re.search(rf"#define {name} {val}\b", hdr), name
    doc = hdr[:hdr.index("#define BG_HEAD_F32")].rsplit("\n/*", 1)[1]
    for cite in ("hpc_train.py:77-86", "CategoricalDistribution.sample / log_prob / entropy / mode", "balatro_env_2.py:1841-1849", "balatro_env_2.py:625-627",
                 "train_balatro_fixed.py:228-283", "0x7fc00000", "bg_policy_hash", "2^-24", "smallest valid j", "must not alias", "AFTER", "NEXT action",
                 "index0 + i", "e[j] > 0"):
        assert cite in doc, cite
    assert (nat.HEAD_F32, nat.HEAD_BF16, nat.HEAD_DETERMINISTIC) == (0, 1, 1) and nat.ROW_OFFSETS["action_mask"] == 176
    assert "bg_sample_actions" in nat.EXPORTS and "bg_evaluate_actions" in nat.EXPORTS
    assert os.path.join(CSRC, "bg_head.h") in build.DEPS
    assert "sample_actions" in balatro_gym_amd.__all__ and "evaluate_actions" in balatro_gym_amd.__all__
    # the hash twin has the text of the engines' hash
    def body(path, name):
        return re.sub(r"\s+", " ", re.search(name + r"\(uint64_t policy_seed, uint64_t env_index, uint64_t t\) \{(.*?)\n\}", open(path).read(), re.S).group(1))
    assert body(os.path.join(CSRC, "bg_head.h"), "bg_head_hash") == body(os.path.join(CSRC, "bg_device.h"), "bg_policy_hash")
    if os.path.exists(build.LIB):
        L = C.CDLL(build.LIB)
        assert hasattr(L, "bg_sample_actions") and hasattr(L, "bg_evaluate_actions")


def test_wrappers_refuse_bad_arguments_before_the_library():
    """sample_actions / evaluate_actions / RowBuffers.sample on CPU tensors: every bad argument is a ValueError raised before anything is loaded."""
    import torch
    from balatro_gym_amd import evaluate_actions, sample_actions
    from balatro_gym_amd.vec_env import RowBuffers
    N = 6
    lg = torch.zeros((N, 60))
    for bad in (lg.double(), torch.zeros((N, 59)), torch.zeros((N, 61)), torch.zeros(()), "logits", None, lg.to(torch.float16)):
        with pytest.raises(ValueError, match=r"float32 or bfloat16 tensor \[\.\.\., 60\]"):
            sample_actions(bad, seed=0, t=0)
    for bad in (torch.zeros((60, N)).t(), torch.zeros((N, 120))[:, ::2], torch.zeros((2, N, 64))[:, :4, :60]):
        with pytest.raises(ValueError, match="dense over its row pitch"):
            sample_actions(bad, seed=0, t=0)
    with pytest.raises(TypeError):
        sample_actions(lg)   # seed and t are required
    for kw in ({"seed": -1, "t": 0}, {"seed": 0, "t": 2 ** 64}, {"seed": 0.5, "t": 0}, {"seed": 0, "t": 0, "index0": -3}):
        with pytest.raises(ValueError, match=r"must be an integer in \[0, 2\*\*64\)"):
            sample_actions(lg, **kw)
    rec = torch.zeros((N, 384), dtype=torch.uint8)
    for bad in (torch.zeros((N, 360), dtype=torch.uint8), torch.zeros((N, 336), dtype=torch.uint8), torch.zeros((N, 768), dtype=torch.uint8)[:, ::2]):
        with pytest.raises(ValueError, match="packed records"):
            sample_actions(lg, bad, seed=0, t=0)
    for bad in (torch.zeros((N, 60), dtype=torch.bool), torch.zeros((N, 60), dtype=torch.int32), torch.zeros((N, 61), dtype=torch.int8), "mask"):
        with pytest.raises(ValueError, match="mask must be a uint8 tensor"):
            sample_actions(lg, bad, seed=0, t=0)
    with pytest.raises(ValueError, match="multiple of 4"):
        sample_actions(lg, torch.zeros((N, 62), dtype=torch.int8)[:, :60], seed=0, t=0)
    for bad in (torch.zeros((N + 1, 384), dtype=torch.uint8), torch.zeros((1, N, 384), dtype=torch.uint8), torch.zeros((N - 1, 60), dtype=torch.int8)):
        with pytest.raises(ValueError, match="leading shape of logits"):
            sample_actions(lg, bad, seed=0, t=0)
    for name, dt in (("actions", torch.int32), ("log_prob", torch.float32), ("entropy", torch.float32)):
        for bad in (torch.zeros(N, dtype=torch.float64), torch.zeros(N + 1, dtype=dt), torch.zeros(2 * N, dtype=dt)[::2], torch.zeros((N, 1), dtype=dt)):
            with pytest.raises(ValueError, match=f"{name} must be a contiguous"):
                sample_actions(lg, rec, seed=0, t=0, **{name: bad})
    for bad in (torch.zeros(N, dtype=torch.int64), torch.zeros(N + 1, dtype=torch.int32), None, [0] * N):
        with pytest.raises(ValueError, match="actions must be"):
            evaluate_actions(lg, bad, rec)
    # everything right: what is left is that there is no CPU path
    a = torch.zeros(N, dtype=torch.int32)
    for mask in (None, rec, torch.ones((N, 60), dtype=torch.int8), torch.ones((N, 64), dtype=torch.int8)[:, :60]):
        with pytest.raises(ValueError, match="device tensor"):
            sample_actions(lg, mask, seed=1, t=2, index0=3, deterministic=True)
        with pytest.raises(ValueError, match="device tensor"):
            evaluate_actions(lg.to(torch.bfloat16), a, mask)
    with pytest.raises(ValueError, match="device tensor"):
        sample_actions(torch.zeros((2, 3, 64))[:, :, :60], torch.zeros((2, 3, 352), dtype=torch.uint8), seed=0, t=0)
    rb = RowBuffers(N, torch.device("cpu"), steps=3, row_stride=384)
    with pytest.raises(ValueError, match="device tensor"):
        rb.sample(lg, seed=0, t=0)
    with pytest.raises(ValueError, match="device tensor"):
        rb.sample(lg, 1, seed=0, t=0, deterministic=True)
    with pytest.raises(ValueError, match="leading shape of logits"):
        rb.sample(torch.zeros((N + 1, 60)), seed=0, t=0)
