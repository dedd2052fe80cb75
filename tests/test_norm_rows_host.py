"""bg_norm_obs_rows / bg_norm_reward_rows on the CPU (no GPU): csrc/bg_norm.h -- the moment merge, the RunningMeanStd update, the normalise-and-clip,
the return recurrence, the very text the kernels run -- is compiled with g++ (-O1 -ffp-contract=off -DBG_NORM_HOST) into a small program that walks
records from a file in the kernels' order of merging.  Its batch moments are held to exact rational arithmetic (fractions.Fraction) and to numpy within
the issue's bound (4 N 2**-53 relative to mean(|x|) / to the variance; exactly 0.0 for a constant column); everything behind the moments is held, bit for
bit over every element, to tests/norm_ref.py's `from_moments` fed those moments.  Also: the header's declarations and citations, the exports,
build.DEPS, and the argument checks of the Python wrappers.

tests/norm_ref.py also states the kernels' fixed tree of merges in numpy (tree_moments_obs / tree_moments_ret); here that statement is held to the
compiled twin bit for bit, on the synthetic set and on BIG_CASES, the shapes past one reduction level (N > 4 096: the finishing wave of the returns folds
two to sixteen parts per lane; 17 to 256 observation chunks).  Largest observed shares of the bound at BIG_CASES: mean 0.0002, variance 0.062."""
import ctypes as C
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import norm_ref as ref
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")

_PROGRAM = r"""
#define BG_NORM_HOST
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "balatro_mi355x.h"
#include "bg_norm.h"
static void* slurp(const char* path, size_t bytes) {
  void* p = aligned_alloc(16, (bytes + 31) / 16 * 16);
  FILE* in = fopen(path, "rb");
  if (!in || fread(p, 1, bytes, in) != bytes) exit(4);
  fclose(in);
  return p;
}
static const BgEncTable<BG_ENC_PRODUCED> TAB{};
// the wave's shuffle tree of the reward kernels: lane i takes lane i + off as its right operand
static BgMoments wave_tree(BgMoments* a) {
  for (int off = 1; off < 64; off <<= 1) {
    BgMoments b[64];
    for (int i = 0; i < 64; i++) b[i] = i + off < 64 ? a[i + off] : bg_norm_none();
    for (int i = 0; i < 64; i++) a[i] = bg_norm_merge(a[i], b[i]);
  }
  return a[0];
}
int main(int argc, char** argv) {
  if (argc < 7) return 2;
  const size_t stride = strtoull(argv[2], 0, 10), K = strtoull(argv[3], 0, 10), N = strtoull(argv[4], 0, 10);
  const uint8_t* rows = (const uint8_t*)slurp(argv[5], K * N * stride);
  FILE* out = fopen(argv[7], "wb");
  if (!out) return 5;
  if (!strcmp(argv[1], "obs") && argc == 11) {   // obs stride K N rows state(mean[153] var[153] count) out epsilon clip update
    const double* st = (const double*)slurp(argv[6], (2 * BG_NORM_COLS + 1) * 8);
    const double eps = strtod(argv[8], 0), clip = strtod(argv[9], 0);
    const int update = atoi(argv[10]);
    std::vector<double> mom(K * 2 * BG_NORM_COLS);
    std::vector<uint32_t> o32(K * N * BG_NORM_COLS);
    std::vector<uint16_t> o16(K * N * BG_NORM_COLS);
    BgRms s[BG_NORM_COLS];
    for (int c = 0; c < BG_NORM_COLS; c++) { s[c].mean = st[c]; s[c].var = st[BG_NORM_COLS + c]; s[c].count = st[2 * BG_NORM_COLS]; }
    for (size_t t = 0; t < K; t++) {
      for (int c = 0; c < BG_NORM_COLS; c++) {
        if (update) {   // chunks of 256 envs, each 8 tiles of 32 merged left to right; the chunks merged left to right
          BgMoments step = bg_norm_none();
          for (size_t e0 = 0; e0 < N; e0 += 256) {
            BgMoments acc = bg_norm_none();
            for (size_t r0 = e0; r0 < e0 + 256 && r0 < N; r0 += BG_NORM_TILE) {
              double v[BG_NORM_TILE] = {};
              int n = 0;
              for (; n < BG_NORM_TILE && r0 + n < N; n++) v[n] = bg_norm_value64(rows + (t * N + r0 + n) * stride, TAB.d[c]);
              acc = bg_norm_merge(acc, bg_norm_tile(v, n));
            }
            step = bg_norm_merge(step, acc);
          }
          mom[(t * 2) * BG_NORM_COLS + c] = step.mean;
          mom[(t * 2 + 1) * BG_NORM_COLS + c] = bg_norm_batch_var(step);
          s[c] = bg_norm_rms_update(s[c], step.mean, bg_norm_batch_var(step), (double)N);
        }
        const double denom = bg_norm_denom(s[c].var, eps);
        for (size_t e = 0; e < N; e++) {
          const uint32_t b = bg_norm_obs_bits(bg_norm_value64(rows + (t * N + e) * stride, TAB.d[c]), s[c].mean, denom, clip);
          o32[(t * N + e) * BG_NORM_COLS + c] = b;
          o16[(t * N + e) * BG_NORM_COLS + c] = bg_enc_bf16(b);
        }
      }
    }
    std::vector<double> fin(2 * BG_NORM_COLS + 1);
    for (int c = 0; c < BG_NORM_COLS; c++) { fin[c] = s[c].mean; fin[BG_NORM_COLS + c] = s[c].var; }
    fin[2 * BG_NORM_COLS] = s[0].count;
    fwrite(mom.data(), 8, mom.size(), out); fwrite(fin.data(), 8, fin.size(), out); fwrite(o32.data(), 4, o32.size(), out); fwrite(o16.data(), 2, o16.size(), out);
    fclose(out);
    return 0;
  }
  if (!strcmp(argv[1], "rew") && argc == 12) {   // rew stride K N rows state(ret_stats[3] carry[N]) out gamma epsilon clip update
    const double* st = (const double*)slurp(argv[6], (3 + N) * 8);
    const double gamma = strtod(argv[8], 0), eps = strtod(argv[9], 0), clip = strtod(argv[10], 0);
    const int update = atoi(argv[11]);
    BgRms s; s.mean = st[0]; s.var = st[1]; s.count = st[2];
    std::vector<double> ret(st + 3, st + 3 + N), mom(K * 2), rew(K * N);
    const size_t nch = (N + 63) / 64, per = (nch + 63) / 64;
    for (size_t t = 0; t < K; t++) {
      if (update) {
        std::vector<BgMoments> part(nch);
        for (size_t k = 0; k < nch; k++) {
          BgMoments a[64];
          for (size_t i = 0; i < 64; i++) {
            const size_t e = k * 64 + i;
            if (e < N) { ret[e] = bg_norm_ret_step(ret[e], gamma, bg_norm_reward64(rows + (t * N + e) * stride)); a[i] = bg_norm_one(ret[e]); }
            else a[i] = bg_norm_none();
          }
          part[k] = wave_tree(a);
          part[k].n = (double)(N - k * 64 < 64 ? N - k * 64 : 64);
        }
        BgMoments a[64];
        for (size_t i = 0; i < 64; i++) {
          a[i] = bg_norm_none();
          for (size_t k = i * per; k < (i + 1) * per && k < nch; k++) a[i] = bg_norm_merge(a[i], part[k]);
        }
        const BgMoments step = wave_tree(a);
        mom[t * 2] = step.mean; mom[t * 2 + 1] = bg_norm_batch_var(step);
        s = bg_norm_rms_update(s, step.mean, bg_norm_batch_var(step), (double)N);
      }
      const double denom = bg_norm_denom(s.var, eps);
      for (size_t e = 0; e < N; e++) {
        const uint8_t* rec = rows + (t * N + e) * stride;
        rew[t * N + e] = bg_norm_reward(bg_norm_reward64(rec), denom, clip);
        if (update) ret[e] = bg_norm_ret_done(ret[e], rec[BG_ROW_TERMINATED] != 0);
      }
    }
    const double fin[3] = {s.mean, s.var, s.count};
    fwrite(mom.data(), 8, mom.size(), out); fwrite(fin, 8, 3, out); fwrite(ret.data(), 8, N, out); fwrite(rew.data(), 8, rew.size(), out);
    fclose(out);
    return 0;
  }
  return 2;
}
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile csrc/bg_norm.h for the host"
    d = tmp_path_factory.mktemp("norm_host")
    src = d / "norm_host.cpp"
    src.write_text(_PROGRAM)
    exe = d / "norm_host"
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-I", CSRC, "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])

    class Host:
        @staticmethod
        def obs(rows, state, epsilon, clip, update=1):
            K, N, stride = rows.shape
            np.ascontiguousarray(rows).tofile(str(d / "rows.bin"))
            np.concatenate([state["obs_mean"], state["obs_var"], [state["obs_count"]]]).astype(np.float64).tofile(str(d / "state.bin"))
            subprocess.check_call([str(exe), "obs", str(stride), str(K), str(N), str(d / "rows.bin"), str(d / "state.bin"), str(d / "out.bin"),
                                   float(epsilon).hex(), float(clip).hex(), str(update)])
            b = open(str(d / "out.bin"), "rb").read()
            a = K * 2 * ref.COLS * 8
            c = a + (2 * ref.COLS + 1) * 8
            e = c + K * N * ref.COLS * 4
            fin = np.frombuffer(b[a:c], np.float64)
            return {"moments": np.frombuffer(b[:a], np.float64).reshape(K, 2, ref.COLS), "mean": fin[:ref.COLS], "var": fin[ref.COLS:2 * ref.COLS], "count": fin[-1],
                    "f32": np.frombuffer(b[c:e], np.uint32).reshape(K, N, ref.COLS), "bf16": np.frombuffer(b[e:], np.uint16).reshape(K, N, ref.COLS)}

        @staticmethod
        def rew(rows, state, gamma, epsilon, clip, update=1):
            K, N, stride = rows.shape
            np.ascontiguousarray(rows).tofile(str(d / "rows.bin"))
            np.concatenate([[state["ret_mean"], state["ret_var"], state["ret_count"]], state["returns"]]).astype(np.float64).tofile(str(d / "state.bin"))
            subprocess.check_call([str(exe), "rew", str(stride), str(K), str(N), str(d / "rows.bin"), str(d / "state.bin"), str(d / "out.bin"),
                                   float(gamma).hex(), float(epsilon).hex(), float(clip).hex(), str(update)])
            o = np.fromfile(str(d / "out.bin"), np.float64)
            return {"moments": o[:2 * K].reshape(K, 2), "stats": o[2 * K:2 * K + 3], "returns": o[2 * K + 3:2 * K + 3 + N], "reward": o[2 * K + 3 + N:].reshape(K, N)}
    return Host


def _same(got, want, bits, what):
    g, w = bits(got), bits(want)
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{what}: {len(bad)} of {w.size} elements differ, first {tuple(bad[0])}: {g[tuple(bad[0])]:#x} != {w[tuple(bad[0])]:#x}"


def _u(a):
    return np.ascontiguousarray(a)


def _exact_moments(col):
    """Exact mean and population variance of a float64 column as Fractions."""
    xs = [Fraction(float(v)) for v in col]
    n = len(xs)
    mean = sum(xs) / n
    return mean, sum((x - mean) ** 2 for x in xs) / n


def _check_case(host, rows, state, what, kw=ref.DEFAULTS):
    """One call of both entry points from `state`: moments within the bound of numpy's; everything else bit for bit from_moments."""
    K, N, _ = rows.shape
    o = host.obs(rows, state, kw["epsilon"], kw["clip_obs"])
    r = host.rew(rows, state, kw["gamma"], kw["epsilon"], kw["clip_reward"])
    x = ref.produced64(rows)
    worst = [0.0, 0.0]
    for t in range(K):
        a, b = ref.check_moments(o["moments"][t, 0], o["moments"][t, 1], x[t], f"{what} step {t} obs")
        worst = [max(worst[0], a), max(worst[1], b)]
    want = ref.from_moments(rows, {"obs": o["moments"], "ret": r["moments"]}, state, **kw)
    s = want["state"]
    _same(o["mean"], s["obs_mean"], ref.bits64, f"{what} obs mean")
    _same(o["var"], s["obs_var"], ref.bits64, f"{what} obs var")
    _same([o["count"]], [s["obs_count"]], ref.bits64, f"{what} obs count")
    _same(o["f32"], ref.obs_bits(want["obs"]), _u, f"{what} normalised float32")
    _same(o["bf16"], ref.obs_bits(want["obs"], dtype="bfloat16"), _u, f"{what} normalised bf16")
    _same(r["stats"], [s["ret_mean"], s["ret_var"], s["ret_count"]], ref.bits64, f"{what} ret_stats")
    _same(r["returns"], s["returns"], ref.bits64, f"{what} returns carry")
    _same(r["reward"], want["reward"], ref.bits64, f"{what} normalised reward")
    # the returns the reward moments are taken over follow from the recurrence alone: rebuild them and hold the moments to numpy's
    reward, done = ref.gae_ref.unpack_records(rows)
    ret = np.array(state["returns"], np.float64)
    for t in range(K):
        ret = ret * kw["gamma"] + reward[t]
        a, b = ref.check_moments(r["moments"][t, 0], r["moments"][t, 1], ret, f"{what} step {t} returns")
        worst = [max(worst[0], a), max(worst[1], b)]
        ret[done[t]] = 0
    print(f"{what}: worst |dmean| / bound {worst[0]:.4f}, worst |dvar| / bound {worst[1]:.4f}")
    return o, r, want


@pytest.mark.parametrize("K", ref.SYN_K)
def test_synthetic(host, K):
    """From the initial state (count = 1e-4): every N, both strides; then a second call from the state the first one left (carry across calls)."""
    for _, N, stride, seed in [c for c in ref.synthetic_cases() if c[0] == K]:
        rows = ref.synthetic_rows(2 * K, N, stride, seed)
        s0 = ref.new_state(N)
        what = f"K {K} N {N} stride {stride}"
        o1, r1, w1 = _check_case(host, rows[:K], s0, what + " first call")
        o2, r2, w2 = _check_case(host, rows[K:], w1["state"], what + " second call")
        # 2 K steps in one call give the same bits as two calls of K
        o, r, w = _check_case(host, rows, s0, what + " one call of 2 K")
        _same(o["f32"], np.concatenate([o1["f32"], o2["f32"]]), _u, what + ": two calls differ from one (obs)")
        _same(r["reward"], np.concatenate([r1["reward"], r2["reward"]]), ref.bits64, what + ": two calls differ from one (reward)")
        _same(o["mean"], o2["mean"], ref.bits64, what + ": final mean")
        _same(o["var"], o2["var"], ref.bits64, what + ": final var")
        _same(r["stats"], r2["stats"], ref.bits64, what + ": final ret_stats")
        _same(r["returns"], r2["returns"], ref.bits64, what + ": final carry")


def _tree_is_the_twin(o, r, rows, state, what):
    """tests/norm_ref.py's numpy statement of the fixed tree gives the compiled twin's batch moments bit for bit: every step, every column, the returns."""
    tree = ref.tree_moments(rows, state)
    _same(o["moments"], tree["obs"], ref.bits64, f"{what}: observation moments, numpy tree against the twin")
    _same(r["moments"], tree["ret"], ref.bits64, f"{what}: return moments, numpy tree against the twin")


def test_numpy_tree_is_the_host_twin_on_the_synthetic_set(host):
    for K, N, stride, seed in ref.synthetic_cases():
        rows = ref.synthetic_rows(K, N, stride, seed)
        s0 = ref.new_state(N)
        _tree_is_the_twin(host.obs(rows, s0, 1e-8, 10.0), host.rew(rows, s0, 0.99, 1e-8, 10.0), rows, s0, f"K {K} N {N}")
    # from a state with a carry: the returns the moments are taken over start there
    K, N = 5, 300
    rows = ref.synthetic_rows(2 * K, N, 384, 77)
    s1 = ref.vecnormalize(rows[:K], ref.new_state(N))["state"]
    assert s1["returns"].any()
    _tree_is_the_twin(host.obs(rows[K:], s1, 1e-8, 10.0), host.rew(rows[K:], s1, 0.99, 1e-8, 10.0), rows[K:], s1, "second call")


@pytest.mark.parametrize("case", ref.BIG_CASES, ids=lambda c: f"K{c[0]}-N{c[1]}")
def test_past_one_reduction_level(host, case):
    """N > 4 096: the finishing wave of the returns folds per = ceil(waves / 64) >= 2 parts per lane, and the observation chunks are 17 to 256.  The twin
    holds the bound and the bit-for-bit checks behind the moments, and the numpy tree gives its moments bit for bit."""
    K, N, stride, seed = case
    assert -(-(-(-N // 64)) // 64) >= 2 and -(-N // 256) > 2
    rows = ref.synthetic_rows(K, N, stride, seed)
    s0 = ref.new_state(N)
    o, r, _ = _check_case(host, rows, s0, f"K {K} N {N} stride {stride}")
    _tree_is_the_twin(o, r, rows, s0, f"K {K} N {N}")


def test_big_cases_reach_what_they_claim():
    """The shapes' own arithmetic: waves, per, the lanes that hold fewer parts, chunks and the last chunk's tiles."""
    got = []
    for K, N, stride, _ in ref.BIG_CASES:
        nw, nch = -(-N // 64), -(-N // 256)
        per = -(-nw // 64)
        got.append((K, N, stride, nw, N - (nw - 1) * 64, per, nw // per, nw % per, nch, N - (nch - 1) * 256))
    assert got == [(2, 4097, 352, 65, 1, 2, 32, 1, 17, 1), (3, 8519, 384, 134, 7, 3, 44, 2, 34, 71), (17, 4160, 352, 65, 64, 2, 32, 1, 17, 64),
                   (1, 65536, 384, 1024, 64, 16, 64, 0, 256, 256)]


def test_frozen_statistics(host):
    """update = 0: the normalisation alone, on the statistics as given."""
    K, N = 5, 65
    rows = ref.synthetic_rows(K, N, 384, 99)
    state = ref.vecnormalize(ref.synthetic_rows(9, N, 384, 98), ref.new_state(N))["state"]
    want = ref.from_moments(rows, None, state, training=False, **ref.DEFAULTS)
    o = host.obs(rows, state, 1e-8, 10.0, update=0)
    r = host.rew(rows, state, 0.99, 1e-8, 10.0, update=0)
    _same(o["f32"], ref.obs_bits(want["obs"]), _u, "frozen float32")
    _same(o["bf16"], ref.obs_bits(want["obs"], dtype="bfloat16"), _u, "frozen bf16")
    _same(r["reward"], want["reward"], ref.bits64, "frozen reward")
    _same(o["mean"], state["obs_mean"], ref.bits64, "frozen mean")
    _same(r["stats"], [state["ret_mean"], state["ret_var"], state["ret_count"]], ref.bits64, "frozen ret_stats")
    _same(r["returns"], state["returns"], ref.bits64, "frozen carry")


def _column_of(key):
    """The first PRODUCED column of an observation key."""
    from balatro_gym_amd import _native as nat
    at = 0
    for k in ref.OBS_KEYS:
        if k == key:
            return at
        at += int(np.prod(nat.OBS_SPEC[k][1], dtype=np.int64))
    raise KeyError(key)


def test_merged_moments_against_exact_rationals(host):
    """The tree of merges against fractions.Fraction: N = 300 (two chunks, a ragged tile) and N = 1000 (four chunks; 16 waves), every column and the
    returns, within 4 N 2**-53 of the exact mean (relative to mean(|x|)) and of the exact variance; constant columns exactly.  N = 4 097 (17 chunks,
    65 waves: the finishing wave's lanes fold two parts each) on the returns, chips_scored, money, progress_ratio and the constant mult."""
    for N, seed, keys in ((300, 41, None), (1000, 42, None), (4097, 43, ("chips_scored", "money", "progress_ratio", "mult"))):
        rows = ref.synthetic_rows(1, N, 352, seed)
        o = host.obs(rows, ref.new_state(N), 1e-8, 10.0)
        r = host.rew(rows, ref.new_state(N), 0.99, 1e-8, 10.0)
        x = ref.produced64(rows)[0]
        reward, _ = ref.gae_ref.unpack_records(rows)
        which = range(ref.COLS) if keys is None else [_column_of(k) for k in keys]
        assert keys is None or bool(np.all(x[:, _column_of("mult")] == 1.0))
        cols = [(x[:, c], o["moments"][0, 0, c], o["moments"][0, 1, c]) for c in which] + [(reward[0], r["moments"][0, 0], r["moments"][0, 1])]
        f = Fraction(4 * N, 2 ** 53)
        for c, (col, gm, gv) in enumerate(cols):
            mean, var = _exact_moments(col)
            mabs = sum(Fraction(float(abs(v))) for v in col) / N
            assert abs(Fraction(float(gm)) - mean) <= f * mabs, (N, c, "mean")
            assert abs(Fraction(float(gv)) - var) <= f * var, (N, c, "var")
            if var == 0:
                assert gv == 0.0 and gm == col[0]


def test_synthetic_set_covers_what_it_claims():
    rows = ref.synthetic_rows(33, 300, 384, 7)
    x = ref.produced64(rows)
    obs = ref.encode_ref.unpack_records(rows.reshape(-1, 384))
    assert np.array_equal(ref.bits32(x.astype(np.float32)).reshape(-1, ref.COLS), ref.encode_ref.expected_bits("produced", obs)), "produced64 is encode_ref's matrix before the float32 conversion"
    chips = obs["chips_scored"].reshape(-1)
    assert (np.abs(chips) > 2 ** 24).any() and np.abs(chips).max() == 2 ** 53 - 1 and (chips.astype(np.float64).astype(np.int64) == chips).all()
    assert (chips.astype(np.float32).astype(np.float64) != chips).any(), "no chips_scored that float32 cannot hold"
    assert (obs["money"] < 0).any() and (obs["hand"] == -1).any() and (obs["mult"] == 1).all()
    const = np.all(x.reshape(-1, ref.COLS) == x[0, 0], axis=0)
    assert const.sum() >= 4
    reward, done = ref.gae_ref.unpack_records(rows)
    assert (reward > 0).any() and (reward < 0).any() and 0.05 < done.mean() < 0.4 and (rows[:, :, ref.gae_ref.ROW_TERMINATED] > 1).any()
    w = ref.vecnormalize(rows, ref.new_state(300))
    assert (w["obs"] == 10.0).any() and (w["obs"] == -10.0).any(), "no observation clips on both sides"
    assert (w["reward"] == 10.0).any() and (w["reward"] == -10.0).any(), "no reward clips on both sides"
    cv = w["state"]["obs_var"][const]   # what is left is the initial state's share: count 1e-4 of 9 900 samples, at distance x from mean 0
    assert (cv >= 0.0).all() and (cv <= 1e-6 * np.maximum(1.0, x[0, 0][const] ** 2)).all(), "constant columns: var -> 0"
    assert (w["state"]["returns"] == 0.0).any() and (w["state"]["returns"] != 0.0).any()
    assert {c[2] for c in ref.synthetic_cases()} == {352, 384} and {(c[0], c[1]) for c in ref.synthetic_cases()} == {(k, n) for k in ref.SYN_K for n in ref.SYN_N}


def test_vecnormalize_and_from_moments_agree_on_numpys_own_moments():
    rows = ref.synthetic_rows(6, 65, 352, 3)
    s0 = ref.new_state(65)
    a = ref.vecnormalize(rows, s0)
    b = ref.from_moments(rows, ref.numpy_moments(rows, s0), s0)
    assert np.array_equal(ref.bits32(a["obs"]), ref.bits32(b["obs"])) and np.array_equal(ref.bits64(a["reward"]), ref.bits64(b["reward"]))
    assert s0["obs_count"] == 1e-4 and not s0["returns"].any(), "the caller's state is not modified"
    assert a["state"]["obs_count"] == 6 * 65 + 1e-4


def test_header_declares_and_library_exports_the_normaliser():
    from balatro_gym_amd import _native as nat, build
    hdr = open(HEADER).read()

    def params(name, ret="int"):
        m = re.search(rf"\b{ret}\s+{name}\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"include/balatro_mi355x.h does not declare {name}"
        return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params("bg_norm_workspace_bytes", "uint64_t") == ["int K", "int64_t N"]
    assert params("bg_norm_obs_rows") == ["const uint8_t* rows_dev", "uint64_t row_stride_bytes", "int K", "int64_t N", "int layout", "int out_dtype", "double* mean_dev",
                                          "double* var_dev", "double* count_dev", "int update", "double epsilon", "double clip_obs", "void* out_dev",
                                          "uint64_t out_stride_elems", "double* moments_dev", "void* workspace_dev", "uint64_t workspace_bytes", "float* kernel_ms_out",
                                          "void* stream"]
    assert params("bg_norm_reward_rows") == ["const uint8_t* rows_dev", "uint64_t row_stride_bytes", "int K", "int64_t N", "double* returns_carry_dev", "double* ret_stats_dev",
                                             "int update", "double gamma", "double epsilon", "double clip_reward", "double* rewards_dev", "double* moments_dev",
                                             "void* workspace_dev", "uint64_t workspace_bytes", "float* kernel_ms_out", "void* stream"]
    assert params("bg_gae_rows_ex") == ["const uint8_t* rows_dev", "uint64_t row_stride_bytes", "int K", "int64_t N", "const float* values_dev", "const float* last_values_dev",
                                        "double gamma", "double gae_lambda", "float* advantages_dev", "float* returns_dev", "const double* rewards_dev", "float* kernel_ms_out",
                                        "void* stream"]
    assert int(re.search(r"#define BG_NORM_COLS (\d+)", hdr).group(1)) == ref.COLS == nat.NORM_COLS == nat.ENC_COLS[nat.ENC_PRODUCED]
    doc = hdr[:hdr.index("#define BG_NORM_COLS")].rsplit("/*", 1)[1]
    for cite in ("hpc_train.py:68,72", "train_balatro_agent.py:319,323", "hpc_train.py:101-107,151-152", "VecNormalize", "Replaces:", "progress_ratio",
                 "must not alias", "new_mean = mean + delta * n / tot"):
        assert cite in doc, cite
    for name in ("bg_norm_workspace_bytes", "bg_norm_obs_rows", "bg_norm_reward_rows", "bg_gae_rows_ex"):
        assert name in nat.EXPORTS
    assert os.path.join(CSRC, "bg_norm.h") in build.DEPS
    assert '#include "bg_norm.h"' in open(os.path.join(CSRC, "bg_lib.hip")).read()
    assert "progress_ratio" in open(os.path.join(CSRC, "bg_norm.h")).read().split("#ifndef BG_NORM_H")[0], "the header comment states the deviation"
    if os.path.exists(build.LIB):
        L = C.CDLL(build.LIB)
        assert all(hasattr(L, n) for n in ("bg_norm_workspace_bytes", "bg_norm_obs_rows", "bg_norm_reward_rows", "bg_gae_rows_ex"))


def test_wrappers_refuse_bad_arguments_before_the_library():
    """RowNormalizer / gae_rows(rewards=) on CPU tensors: every bad argument is a ValueError raised before anything is loaded; the state round trip."""
    import torch
    import balatro_gym_amd
    from balatro_gym_amd import RowNormalizer, gae_rows
    from balatro_gym_amd.vec_env import RowBuffers
    assert "RowNormalizer" in balatro_gym_amd.__all__
    K, N = 3, 5
    rows = torch.zeros((K, N, 384), dtype=torch.uint8)
    nm = RowNormalizer(N, "cpu")
    assert nm.obs_mean.dtype == torch.float64 and tuple(nm.obs_mean.shape) == (153,) == tuple(nm.obs_var.shape) and nm.obs_count.tolist() == [1e-4]
    assert nm.ret_stats.tolist() == [0.0, 1.0, 1e-4] and tuple(nm.returns.shape) == (N,) and not nm.returns.any() and bool((nm.obs_var == 1.0).all())
    assert (nm.gamma, nm.epsilon, nm.clip_obs, nm.clip_reward, nm.norm_obs, nm.norm_reward, nm.training) == (0.99, 1e-8, 10.0, 10.0, True, True, True)
    for bad in (rows.to(torch.int8), rows[:, :, :352][:, ::2], "rows", rows.view(1, K, N, 384)):
        with pytest.raises(ValueError, match=r"contiguous uint8 tensor \[K, N, stride\]"):
            nm.normalize_obs(bad)
        with pytest.raises(ValueError, match=r"contiguous uint8 tensor \[K, N, stride\]"):
            nm.normalize_reward(bad)
    for stride in (336, 360):
        with pytest.raises(ValueError, match="record stride"):
            nm.normalize_obs(torch.zeros((K, N, stride), dtype=torch.uint8))
    with pytest.raises(ValueError, match="records of 5 envs"):
        nm.normalize_obs(torch.zeros((K, N + 1, 384), dtype=torch.uint8))
    with pytest.raises(ValueError, match="layout must be 'produced' or 'fixed'"):
        nm.normalize_obs(rows, layout="extractor")
    with pytest.raises(ValueError, match="dtype must be"):
        nm.normalize_obs(rows, dtype=torch.float16)
    with pytest.raises(ValueError, match="out must be"):
        nm.normalize_obs(rows, out=torch.zeros((K, N, 628)))
    with pytest.raises(ValueError, match="out must be"):
        nm.normalize_obs(rows[0], out=torch.zeros((1, N, 153)))
    with pytest.raises(ValueError, match="out must be"):
        nm.normalize_reward(rows, out=torch.zeros((K, N)))
    for call in (lambda: nm.normalize_obs(rows), lambda: nm.normalize_obs(rows[0], "fixed", torch.bfloat16), lambda: nm.normalize_reward(rows),
                 lambda: RowBuffers(N, torch.device("cpu"), steps=K).normalize(nm), lambda: RowBuffers(N, torch.device("cpu"), steps=K).normalize_reward(nm)):
        with pytest.raises(ValueError, match="device tensor"):
            call()
    with pytest.raises(ValueError, match="norm_obs=False"):
        RowNormalizer(N, "cpu", norm_obs=False).normalize_obs(rows)
    with pytest.raises(ValueError, match="norm_reward=False"):
        RowNormalizer(N, "cpu", norm_reward=False).normalize_reward(rows)
    with pytest.raises(ValueError, match="finite"):
        RowNormalizer(N, "cpu", gamma=float("inf"))
    # gae_rows(rewards=)
    v, lv = torch.zeros((K, N)), torch.zeros(N)
    for bad in (torch.zeros((K, N)), torch.zeros((K, N + 1), dtype=torch.float64), torch.zeros((N, K), dtype=torch.float64).t()):
        with pytest.raises(ValueError, match="rewards must be a contiguous torch.float64 tensor"):
            gae_rows(rows, v, lv, rewards=bad)
    with pytest.raises(ValueError, match="device tensor"):
        RowBuffers(N, torch.device("cpu"), steps=K, row_stride=384).gae(v, lv, rewards=torch.zeros((K, N), dtype=torch.float64))
    # the state: an exact round trip through host tensors; reset_returns
    nm.obs_mean += torch.arange(153, dtype=torch.float64) / 7
    nm.obs_var *= 1.0 / 3
    nm.obs_count += 41
    nm.ret_stats += 0.1
    nm.returns += torch.arange(N, dtype=torch.float64) / 3
    sd = nm.state_dict()
    assert all(not t.is_cuda for t in sd.values() if isinstance(t, torch.Tensor))
    other = RowNormalizer(N, "cpu", gamma=0.5, training=False)
    other.load_state_dict(sd)
    for name in ("obs_mean", "obs_var", "obs_count", "ret_stats", "returns"):
        assert torch.equal(getattr(other, name).view(torch.int64), getattr(nm, name).view(torch.int64)), name
    assert other.gamma == 0.99 and other.training is True
    nm.obs_mean.zero_()
    assert sd["obs_mean"].any(), "state_dict holds copies"
    with pytest.raises(ValueError, match="returns must be a torch.float64 tensor"):
        other.load_state_dict(dict(sd, returns=torch.zeros(N + 1, dtype=torch.float64)))
    other.reset_returns(torch.tensor([True, False, False, True, False]))
    assert other.returns.tolist() == [0.0, 1 / 3, 2 / 3, 0.0, 4 / 3]
    with pytest.raises(ValueError, match="mask must have shape"):
        other.reset_returns(torch.zeros(N + 1, dtype=torch.bool))
    other.reset_returns()
    assert not other.returns.any()
