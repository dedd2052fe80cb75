"""bg_gae_rows / bg_episode_stats_rows on the CPU (no GPU): csrc/bg_gae.h -- the per-step arithmetic of both scans, the very text the kernels run -- is
compiled with g++ (-O1 -ffp-contract=off -DBG_GAE_HOST) into a small program that walks records from a file, and held, bit for bit over every element, to
the numpy restatement of tests/gae_ref.py (SB3's compute_returns_and_advantage verbatim; a forward float64 scan): rewards of the C oracle's real episodes
and synthetic rewards at the limits of the float32 rounding.  Also: the header's declarations and citations, the exports, build.DEPS, and the argument
checks of the Python wrappers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import gae_ref as ref
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")

_PROGRAM = r"""
#define BG_GAE_HOST
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "balatro_mi355x.h"
#include "bg_gae.h"
static void* slurp(const char* path, size_t bytes) {
  void* p = aligned_alloc(16, (bytes + 31) / 16 * 16);
  FILE* in = fopen(path, "rb");
  if (!in || fread(p, 1, bytes, in) != bytes) exit(4);
  fclose(in);
  return p;
}
int main(int argc, char** argv) {
  if (argc < 7) return 2;
  const size_t stride = strtoull(argv[2], 0, 10), K = strtoull(argv[3], 0, 10), N = strtoull(argv[4], 0, 10);
  const uint8_t* rows = (const uint8_t*)slurp(argv[5], K * N * stride);
  if (!strcmp(argv[1], "gae") && argc == 10) {   // gae stride K N rows values(K*N + N floats) out gamma lambda
    const float* values = (const float*)slurp(argv[6], (K * N + N) * 4);
    const float* last_values = values + K * N;
    const float g = bg_gae_g(strtod(argv[8], 0)), gl = bg_gae_gl(strtod(argv[8], 0), strtod(argv[9], 0));
    float* adv = (float*)malloc(K * N * 4 + 4);
    float* ret = (float*)malloc(K * N * 4 + 4);
    for (size_t e = 0; e < N; e++) {
      float last = 0.0f, nv = last_values[e];
      for (size_t t = K; t-- > 0;) {
        const uint8_t* rec = rows + (t * N + e) * stride;
        const float v = values[t * N + e];
        last = bg_gae_step(bg_gae_reward32(bg_gae_reward64(rec)), bg_gae_nnt(bg_gae_done(rec)), v, nv, g, gl, last);
        nv = v;
        adv[t * N + e] = last;
        ret[t * N + e] = bg_gae_return(last, v);
      }
    }
    FILE* out = fopen(argv[7], "wb");
    if (!out || fwrite(adv, 4, K * N, out) != K * N || fwrite(ret, 4, K * N, out) != K * N) return 5;
    fclose(out);
    return 0;
  }
  if (!strcmp(argv[1], "eps") && argc == 8) {   // eps stride K N rows carries(N doubles, N int32) out
    const uint8_t* c = (const uint8_t*)slurp(argv[6], N * 12);
    double* cr = (double*)malloc(N * 8 + 8);
    int32_t* cl = (int32_t*)malloc(N * 4 + 4);
    memcpy(cr, c, N * 8); memcpy(cl, c + N * 8, N * 4);
    double* er = (double*)malloc(K * N * 8 + 8);
    int32_t* el = (int32_t*)malloc(K * N * 4 + 4);
    for (size_t e = 0; e < N; e++)
      for (size_t t = 0; t < K; t++) {
        const uint8_t* rec = rows + (t * N + e) * stride;
        const BgEpsStep o = bg_eps_step(bg_gae_reward64(rec), bg_gae_done(rec), cr[e], cl[e]);
        cr[e] = o.carry_return; cl[e] = o.carry_len;
        er[t * N + e] = o.ep_return; el[t * N + e] = o.ep_len;
      }
    FILE* out = fopen(argv[7], "wb");
    if (!out || fwrite(er, 8, K * N, out) != K * N || fwrite(el, 4, K * N, out) != K * N || fwrite(cr, 8, N, out) != N || fwrite(cl, 4, N, out) != N) return 5;
    fclose(out);
    return 0;
  }
  return 2;
}
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile csrc/bg_gae.h for the host"
    d = tmp_path_factory.mktemp("gae_host")
    src = d / "gae_host.cpp"
    src.write_text(_PROGRAM)
    exe = d / "gae_host"
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-I", CSRC, "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])

    class Host:
        @staticmethod
        def gae(rows, values, last_values, gamma, gae_lambda):
            K, N, stride = rows.shape
            np.ascontiguousarray(rows).tofile(str(d / "rows.bin"))
            np.concatenate([np.ascontiguousarray(values, np.float32).reshape(-1), np.ascontiguousarray(last_values, np.float32)]).tofile(str(d / "values.bin"))
            subprocess.check_call([str(exe), "gae", str(stride), str(K), str(N), str(d / "rows.bin"), str(d / "values.bin"), str(d / "out.bin"),
                                   float(gamma).hex(), float(gae_lambda).hex()])
            o = np.fromfile(str(d / "out.bin"), np.float32)
            return o[:K * N].reshape(K, N), o[K * N:].reshape(K, N)

        @staticmethod
        def eps(rows, carry_return=None, carry_len=None):
            K, N, stride = rows.shape
            cr = np.zeros(N, np.float64) if carry_return is None else np.ascontiguousarray(carry_return, np.float64)
            cl = np.zeros(N, np.int32) if carry_len is None else np.ascontiguousarray(carry_len, np.int32)
            np.ascontiguousarray(rows).tofile(str(d / "rows.bin"))
            with open(str(d / "carry.bin"), "wb") as f:
                f.write(cr.tobytes() + cl.tobytes())
            subprocess.check_call([str(exe), "eps", str(stride), str(K), str(N), str(d / "rows.bin"), str(d / "carry.bin"), str(d / "out.bin")])
            b = open(str(d / "out.bin"), "rb").read()
            a, c, e = K * N * 8, K * N * 12, K * N * 12 + N * 8
            return (np.frombuffer(b[:a], np.float64).reshape(K, N), np.frombuffer(b[a:c], np.int32).reshape(K, N),
                    np.frombuffer(b[c:e], np.float64), np.frombuffer(b[e:], np.int32))
    return Host


def _assert_bits(got, want, bits, what):
    g, w = bits(got), bits(want)
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{what}: {len(bad)} of {w.size} elements differ, first (t, env) {tuple(bad[0])}: {g[tuple(bad[0])]:#x} != {w[tuple(bad[0])]:#x}"


def _check_gae(host, reward, done, values, last_values, gamma, lam, stride, what):
    rows = ref.pack_records(reward, done, stride)
    r2, d2 = ref.unpack_records(rows)
    assert np.array_equal(ref.bits64(r2), ref.bits64(reward)) and np.array_equal(d2, np.asarray(done) != 0)
    want_a, want_r = ref.gae(reward, done, values, last_values, gamma, lam)
    got_a, got_r = host.gae(rows, values, last_values, gamma, lam)
    _assert_bits(got_a, want_a, ref.bits32, f"{what} advantages")
    _assert_bits(got_r, want_r, ref.bits32, f"{what} returns")


def _check_eps(host, reward, done, stride, what):
    """One call over all K steps against the numpy scan; two calls of K / 2 with the carries passed on give the same; the step count is conserved."""
    rows = ref.pack_records(reward, done, stride)
    K, N = reward.shape
    want = ref.episode_stats(reward, done)
    got = host.eps(rows)
    for g, w, bits, name in zip(got, want, (ref.bits64, lambda a: np.asarray(a, np.int32), ref.bits64, lambda a: np.asarray(a, np.int32)),
                                ("ep_return", "ep_len", "carry_return", "carry_len")):
        _assert_bits(np.atleast_2d(g), np.atleast_2d(w), bits, f"{what} {name}")
    assert int(got[1].sum()) + int(got[3].sum()) == K * N
    assert np.count_nonzero(got[1]) == np.count_nonzero(done)
    if K >= 2:
        h = K // 2
        a = host.eps(rows[:h])
        b = host.eps(rows[h:], a[2], a[3])
        assert np.array_equal(ref.bits64(np.concatenate([a[0], b[0]])), ref.bits64(got[0])), f"{what}: two calls differ from one (ep_return)"
        assert np.array_equal(np.concatenate([a[1], b[1]]), got[1]), f"{what}: two calls differ from one (ep_len)"
        assert np.array_equal(ref.bits64(b[2]), ref.bits64(got[2])) and np.array_equal(b[3], got[3]), f"{what}: final carries differ"


@pytest.fixture(scope="module")
def oracle_window():
    """64 envs of the C oracle under the uniform policy for 128 steps, reset() first and again on done: (reward float64 [128, 64], done uint8 [128, 64])."""
    from oracle import pyoracle as po
    N, K = 64, 128
    envs = [po.OracleEnv(900 + e, scorer_jokers=True) for e in range(N)]
    reward, done = np.zeros((K, N), np.float64), np.zeros((K, N), np.uint8)
    for e, env in enumerate(envs):
        env.reset()
        for t in range(K):
            _, r, term, _, _ = env.step(env.policy_action(po.POLICY_UNIFORM, 11, e, t))
            reward[t, e], done[t, e] = r, term
            if term:
                env.reset()
    return reward, done


def test_oracle_rewards(host, oracle_window):
    """Real rewards: enough episodes end inside the window and enough rewards are not float32 values for the rounding to matter (asserted, not assumed)."""
    reward, done = oracle_window
    assert int(done.sum()) >= 32, f"only {int(done.sum())} terminated steps in the window"
    inexact = float(np.mean(reward.astype(np.float32).astype(np.float64) != reward))
    assert inexact >= 0.01, f"only {inexact:.2%} of the rewards are not float32-representable"
    K, N = reward.shape
    for i, (gamma, lam) in enumerate(ref.GAMMA_LAMBDA):
        values, last_values = ref.synthetic_values(K, N, 50 + i)
        for stride in (384, 352):
            _check_gae(host, reward, done, values, last_values, gamma, lam, stride, f"oracle gamma {gamma} lambda {lam} stride {stride}")
    zeros = np.zeros((K, N), np.float32)
    _check_gae(host, reward, done, zeros, zeros[0], 0.99, 0.95, 384, "oracle, zero values")
    for stride in (384, 352):
        _check_eps(host, reward, done, stride, f"oracle stride {stride}")


def test_a_discount_pair_pins_how_gl_is_rounded():
    """gl = float32(gamma * gae_lambda), the product taken in float64: at least one pair of the set tells it from float32(gamma) * float32(gae_lambda)
    ((0.95, 0.9) does; (0.99, 0.95) happens to give the same float32 either way)."""
    differs = [(g, l) for g, l in ref.GAMMA_LAMBDA if np.float32(g * l) != np.float32(g) * np.float32(l)]
    assert (0.95, 0.9) in differs, differs


@pytest.mark.parametrize("K", ref.SYN_K)
def test_synthetic(host, K):
    """Terminated at t = K - 1, at t = 0, on every step, never, at random; every N; rewards on float32 ties, subnormal after rounding, +-1e30; values up
    to 1e6; the five discount pairs; both strides."""
    cases = [c for c in ref.synthetic_cases() if c[0] == K]
    assert {c[1] for c in cases} == set(ref.SYN_N) and {c[2] for c in cases} == set(ref.DONE_PATTERNS)
    for _, N, pattern, (gamma, lam), stride, seed in cases:
        reward = ref.synthetic_rewards(K, N, seed)
        done = ref.synthetic_done(K, N, pattern, seed)
        values, last_values = ref.synthetic_values(K, N, seed)
        what = f"K {K} N {N} {pattern} gamma {gamma} lambda {lam} stride {stride}"
        _check_gae(host, reward, done, values, last_values, gamma, lam, stride, what)
        _check_eps(host, reward, done, stride, what)


def test_synthetic_set_covers_what_it_claims():
    used = ref.synthetic_cases()
    assert {c[3] for c in used} == set(ref.GAMMA_LAMBDA) and {c[4] for c in used} == {384, 352}
    for K in ref.SYN_K:
        assert {c[3] for c in used if c[0] == K} == set(ref.GAMMA_LAMBDA)
    r = ref.synthetic_rewards(17, 1000, 3)
    f = r.astype(np.float32)
    f64 = f.astype(np.float64)
    below = np.where(f64 < r, f, np.nextafter(f, np.float32(-np.inf))).astype(np.float64)   # the float32 neighbours of an inexact reward
    above = np.where(f64 > r, f, np.nextafter(f, np.float32(np.inf))).astype(np.float64)
    ties = (f64 != r) & (r - below == above - r)
    assert ties.sum() > 100, "no float32 ties among the synthetic rewards"
    up = f.astype(np.float64)[ties] > r[ties]
    assert up.any() and (~up).any(), "ties to even must round both ways"
    sub = np.abs(f) == np.float32(2.0 ** -140)
    assert sub.sum() > 100 and (f[sub] > 0).any() and (f[sub] < 0).any()
    assert (f == np.float32(1e30)).any() and (f == np.float32(-1e30)).any() and (r == -1.0).any() and (r == -50.0).any()
    v, lv = ref.synthetic_values(17, 1000, 3)
    assert np.abs(v).max() > 1e5 and np.isfinite(v).all() and np.isfinite(lv).all()


def test_header_declares_and_library_exports_both_scans():
    from balatro_gym_amd import _native as nat, build
    hdr = open(HEADER).read()
    m = re.search(r"\bint\s+bg_gae_rows\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/balatro_mi355x.h does not declare bg_gae_rows"
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == ["const uint8_t* rows_dev", "uint64_t row_stride_bytes", "int K", "int64_t N", "const float* values_dev", "const float* last_values_dev",
                      "double gamma", "double gae_lambda", "float* advantages_dev", "float* returns_dev", "float* kernel_ms_out", "void* stream"], params
    m = re.search(r"\bint\s+bg_episode_stats_rows\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/balatro_mi355x.h does not declare bg_episode_stats_rows"
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == ["const uint8_t* rows_dev", "uint64_t row_stride_bytes", "int K", "int64_t N", "double* ep_return_carry_dev", "int32_t* ep_len_carry_dev",
                      "double* ep_return_dev", "int32_t* ep_len_dev", "float* kernel_ms_out", "void* stream"], params
    doc = hdr[:hdr.index("int bg_gae_rows")].rsplit("/*", 1)[1]
    for cite in ("hpc_train.py:77-86", "train_balatro_fixed.py:346-355", "train_balatro_agent.py:329-335", "train_progressive.py:164-171",
                 "robust_training.py:143-149", "compute_returns_and_advantage", "hpc_train.py:26", "train_balatro_fixed.py:290", "Monitor",
                 "must not alias", "plain float64 sum in step order"):
        assert cite in doc, cite
    assert (ref.ROW_BYTES, ref.ROW_REWARD, ref.ROW_TERMINATED) == tuple(int(re.search(rf"#define {n} (\d+)", hdr).group(1)) for n in ("BG_ROW_BYTES", "BG_ROW_REWARD", "BG_ROW_TERMINATED"))
    assert (ref.ROW_REWARD, ref.ROW_TERMINATED) == (nat.ROW_EXTRA["reward"][0], nat.ROW_EXTRA["terminated"][0])
    assert "bg_gae_rows" in nat.EXPORTS and "bg_episode_stats_rows" in nat.EXPORTS
    assert os.path.join(CSRC, "bg_gae.h") in build.DEPS
    if os.path.exists(build.LIB):
        L = C.CDLL(build.LIB)
        assert hasattr(L, "bg_gae_rows") and hasattr(L, "bg_episode_stats_rows")


def test_wrappers_refuse_bad_arguments_before_the_library():
    """gae_rows / RowBuffers.gae / EpisodeStats on CPU tensors: every bad argument is a ValueError raised before anything is loaded."""
    import torch
    from balatro_gym_amd import EpisodeStats, gae_rows
    from balatro_gym_amd.vec_env import RowBuffers
    K, N = 3, 5
    rows = torch.zeros((K, N, 384), dtype=torch.uint8)
    v, lv = torch.zeros((K, N)), torch.zeros(N)
    for bad in (rows.to(torch.int8), rows.view(K * N, 384), rows[:, :, :352][:, ::2], "rows"):
        with pytest.raises(ValueError, match=r"contiguous uint8 tensor \[K, N, stride\]"):
            gae_rows(bad, v, lv)
    for stride in (336, 360):
        with pytest.raises(ValueError, match="record stride"):
            gae_rows(torch.zeros((K, N, stride), dtype=torch.uint8), v, lv)
        with pytest.raises(ValueError, match="record stride"):
            EpisodeStats(N, "cpu").update(torch.zeros((K, N, stride), dtype=torch.uint8))
    for bv in (v.double(), torch.zeros((K, N + 1)), torch.zeros((N, K)).t(), torch.zeros((K * N,)), None):
        with pytest.raises(ValueError, match="values must be a contiguous torch.float32 tensor"):
            gae_rows(rows, bv, lv)
    for blv in (lv.double(), torch.zeros(N + 1), torch.zeros((1, N)), torch.zeros(2 * N)[::2]):
        with pytest.raises(ValueError, match="last_values must be a contiguous torch.float32 tensor"):
            gae_rows(rows, v, blv)
    with pytest.raises(ValueError, match="advantages must be"):
        gae_rows(rows, v, lv, advantages=torch.zeros((K, N), dtype=torch.float64))
    with pytest.raises(ValueError, match="returns must be"):
        gae_rows(rows, v, lv, returns=torch.zeros((K + 1, N)))
    with pytest.raises(ValueError, match="finite"):
        gae_rows(rows, v, lv, gamma=float("nan"))
    # everything right: what is left is that there is no CPU path
    with pytest.raises(ValueError, match="device tensor"):
        gae_rows(rows, v, lv, advantages=torch.zeros((K, N)), returns=torch.zeros((K, N)))
    with pytest.raises(ValueError, match="device tensor"):
        RowBuffers(N, torch.device("cpu"), steps=K, row_stride=352).gae(v, lv, 0.99, 0.95)
    st = EpisodeStats(N, "cpu")
    assert st.ep_return_carry.dtype == torch.float64 and st.ep_len_carry.dtype == torch.int32 and tuple(st.ep_return_carry.shape) == (N,) == tuple(st.ep_len_carry.shape)
    with pytest.raises(ValueError, match=r"contiguous uint8 tensor \[K, N, stride\]"):
        st.update(rows[0])
    with pytest.raises(ValueError, match="records of 5 envs"):
        st.update(torch.zeros((K, N + 1, 384), dtype=torch.uint8))
    with pytest.raises(ValueError, match="ep_return must be"):
        st.update(rows, ep_return=torch.zeros((K, N)))
    with pytest.raises(ValueError, match="ep_len must be"):
        st.update(rows, ep_len=torch.zeros((K, N), dtype=torch.int64))
    with pytest.raises(ValueError, match="device tensor"):
        st.update(rows)
    with pytest.raises(ValueError, match="device tensor"):
        RowBuffers(N, torch.device("cpu"), steps=K, row_stride=384).episode_stats(st)
    # reset: all carries, or the masked ones
    st.ep_return_carry += 2.5
    st.ep_len_carry += 7
    st.reset(torch.tensor([True, False, False, True, False]))
    assert st.ep_return_carry.tolist() == [0.0, 2.5, 2.5, 0.0, 2.5] and st.ep_len_carry.tolist() == [0, 7, 7, 0, 7]
    with pytest.raises(ValueError, match="mask must have shape"):
        st.reset(torch.zeros(N + 1, dtype=torch.bool))
    st.reset()
    assert not st.ep_return_carry.any() and not st.ep_len_carry.any()
