"""The episode summary and bg_episode_ends_rows on the CPU (no GPU): the header's constants and declarations against _native's, the argument
checks of the Python wrappers, the restatement tests/ends_ref.py against sb3_adapter.CurriculumTracker.update itself, and csrc/bg_ends.h's per-record
rule -- the text the kernel runs -- compiled with g++ (-DBG_ENDS_HOST) into a small program and held against the restatement."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import ends_ref as ref
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")

# in (one file): int64 K, N, stride, window, increment; float64 threshold; int64 with_cur; records [K, N, stride]; cap int32 [N]; hist int16 [window, N];
# count int64 [N]; at_level int32 [N].  out (the same file): report int64 [32]; cap; hist; count; at_level; raised uint8 [N].  The loops are the
# kernel's: lane = env, forwards in t, the tail of a record as four little-endian words.
_PROGRAM = r"""
#define BG_ENDS_HOST
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "balatro_mi355x.h"
#include "bg_ends.h"
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* in = fopen(argv[1], "rb");
  int64_t hd[5]; double thr; int64_t with_cur;
  if (!in || fread(hd, 8, 5, in) != 5 || fread(&thr, 8, 1, in) != 1 || fread(&with_cur, 8, 1, in) != 1) return 4;
  const size_t K = (size_t)hd[0], N = (size_t)hd[1], stride = (size_t)hd[2], W = (size_t)hd[3];
  const int32_t inc = (int32_t)hd[4];
  uint8_t* rows = (uint8_t*)malloc(K * N * stride + 1);
  int32_t* cap = (int32_t*)malloc(N * 4 + 4);
  int16_t* hist = (int16_t*)malloc(W * N * 2 + 2);
  int64_t* count = (int64_t*)malloc(N * 8 + 8);
  int32_t* at = (int32_t*)malloc(N * 4 + 4);
  uint8_t* raised = (uint8_t*)calloc(N + 1, 1);
  if (fread(rows, 1, K * N * stride, in) != K * N * stride || fread(cap, 4, N, in) != N || fread(hist, 2, W * N, in) != W * N ||
      fread(count, 8, N, in) != N || fread(at, 4, N, in) != N) return 5;
  fclose(in);
  int64_t rep[BG_ENDS_WORDS];
  memset(rep, 0, sizeof(rep));
  for (size_t e = 0; e < N; e++) {
    BgEndsAcc acc; bg_ends_acc_init(acc);
    BgCurEnv c; c.cap = cap[e]; c.count = count[e]; c.at_level = at[e]; c.raised = false;
    for (size_t t = 0; t < K; t++) {
      uint32_t w[4];
      memcpy(w, rows + (t * N + e) * stride + BG_ENDS_TAIL, 16);
      const BgEndRec r = bg_ends_record(w[1], w[2], w[3]);
      if (r.ended != (rows[(t * N + e) * stride + BG_ROW_TERMINATED] != 0) || r.flags != rows[(t * N + e) * stride + BG_ROW_END_FLAGS]) return 6;
      if (!r.ended) continue;
      const int32_t bin = bg_ends_count(acc, r);
      if (bin < 0) continue;
      rep[BG_ENDS_W_HIST + bin] += 1;
      if (with_cur) bg_ends_curriculum(c, hist + e, N, r.ante, (int32_t)W, inc, thr);
    }
    cap[e] = c.cap; count[e] = c.count; at[e] = c.at_level; raised[e] = c.raised ? 1 : 0;
    rep[BG_ENDS_W_RAISED] += c.raised ? 1 : 0;
    rep[BG_ENDS_W_ENDED] += acc.ended; rep[BG_ENDS_W_GAME] += acc.game; rep[BG_ENDS_W_INVALID] += acc.invalid; rep[BG_ENDS_W_MAX_STEPS] += acc.max_steps;
    rep[BG_ENDS_W_NO_SUMMARY] += acc.no_summary; rep[BG_ENDS_W_ANTE_SUM] += (int64_t)acc.ante_sum; rep[BG_ENDS_W_CHIPS_SUM] += (int64_t)acc.chips_sum;
    if ((int64_t)acc.ante_max > rep[BG_ENDS_W_ANTE_MAX]) rep[BG_ENDS_W_ANTE_MAX] = acc.ante_max;
    if ((int64_t)acc.chips_max > rep[BG_ENDS_W_CHIPS_MAX]) rep[BG_ENDS_W_CHIPS_MAX] = acc.chips_max;
  }
  FILE* out = fopen(argv[1], "wb");
  if (!out || fwrite(rep, 8, BG_ENDS_WORDS, out) != BG_ENDS_WORDS || fwrite(cap, 4, N, out) != N || fwrite(hist, 2, W * N, out) != W * N ||
      fwrite(count, 8, N, out) != N || fwrite(at, 4, N, out) != N || fwrite(raised, 1, N, out) != N) return 7;
  fclose(out);
  free(rows); free(cap); free(hist); free(count); free(at); free(raised);
  return 0;
}
"""


def synthetic_rows(rng, K, N, stride, p_end=0.2, max_ante=20):
    """Records [K, N, stride] of random bytes whose five ending fields are drawn as the GPU test draws them: terminated with p_end, end antes
    0..max_ante (0 = made without the summary), flags from {1, 2, 4, 6}, chips up to 2**32 - 1 (the extremes included)."""
    rows = rng.integers(0, 256, (K, N, stride), dtype=np.uint8)
    term = (rng.random((K, N)) < p_end).astype(np.uint8)
    ante = rng.integers(0, max_ante + 1, (K, N)).astype(np.int16)
    flags = rng.choice(np.array([1, 2, 4, 6], np.uint8), (K, N))
    chips = rng.integers(0, 2 ** 32, (K, N), dtype=np.uint64).astype(np.uint32)
    chips[rng.random((K, N)) < 0.05] = 2 ** 32 - 1
    ref.put_fields(rows, term, flags, ante, rng.integers(1, 4, (K, N)).astype(np.int8), chips)
    return rows


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile csrc/bg_ends.h for the host"
    d = tmp_path_factory.mktemp("ends_host")
    src = d / "ends_host.cpp"
    src.write_text(_PROGRAM)
    out = d / "ends_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-I", os.path.dirname(HEADER), "-o", str(out), str(src)])
    return out


def _run(exe, rows, cur, with_cur=True):
    """Records and an ends_ref.Curriculum (read, not modified) through the compiled rule: (report, cap, hist, count, at_level, raised)."""
    K, N, stride = rows.shape
    W = cur.window
    path = exe.parent / "io.bin"
    with open(path, "wb") as f:
        f.write(np.array([K, N, stride, W, cur.inc], np.int64).tobytes())
        f.write(np.array([cur.thr], np.float64).tobytes())
        f.write(np.array([1 if with_cur else 0], np.int64).tobytes())
        for a in (rows, cur.cap, cur.hist, cur.count, cur.at_level):
            f.write(np.ascontiguousarray(a).tobytes())
    subprocess.check_call([str(exe), str(path)])
    raw = path.read_bytes()
    sizes = [(np.int64, (32,)), (np.int32, (N,)), (np.int16, (W, N)), (np.int64, (N,)), (np.int32, (N,)), (np.uint8, (N,))]
    out, at = [], 0
    for dt, shape in sizes:
        nb = int(np.prod(shape)) * np.dtype(dt).itemsize
        out.append(np.frombuffer(raw[at:at + nb], dt).reshape(shape))
        at += nb
    assert at == len(raw)
    return out


# ---------------------------------------------------------------------------------------------------------------- constants and declarations
def test_header_constants_exports_and_build():
    from balatro_gym_amd import _native as nat, build
    import balatro_gym_amd
    hdr = open(HEADER).read()
    for name, val in (("BG_ROW_END_ANTE", 344), ("BG_ROW_END_ROUND", 346), ("BG_ROW_END_CHIPS", 348), ("BG_ENDS_WORDS", 32)):
        assert re.search(rf"#define {name}\s+{val}\b", hdr), name
    assert (nat.ROW_END_ANTE, nat.ROW_END_ROUND, nat.ROW_END_CHIPS, nat.ENDS_WORDS) == (344, 346, 348, 32)
    assert (ref.R_END_ANTE, ref.R_END_ROUND, ref.R_END_CHIPS, ref.ENDS_WORDS) == (344, 346, 348, 32)
    assert nat.ROW_EXTRA["end_ante"] == (344, "int16") and nat.ROW_EXTRA["end_round"] == (346, "int8") and nat.ROW_EXTRA["end_chips"] == (348, "uint32")
    assert nat.ROW_END_CHIPS + 4 == nat.ROW_BYTES and ref.CAP_MAX == nat.CURRICULUM_CAP_MAX == 255
    # the report's words: the header of the scan, _native and the restatement name the same ones
    ends_h = open(os.path.join(CSRC, "bg_ends.h")).read()
    words = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define BG_ENDS_W_([A-Z_]+) (\d+)", ends_h)}
    assert words.pop("hist") == nat.ENDS_HIST == 16 and words == nat.ENDS_REPORT
    assert "BG_ENDS_HOST" in ends_h and int(re.search(r"#define BG_ENDS_TAIL (\d+)", ends_h).group(1)) == 336
    assert int(re.search(r"#define BG_ENDS_CAP_MAX (\d+)", ends_h).group(1)) == 255
    # the declarations
    assert re.search(r"\bint\s+bg_set_episode_summary\s*\(\s*bg_handle\* h,\s*int enable\s*\)\s*;", hdr)
    m = re.search(r"typedef struct bg_curriculum \{(.*?)\} bg_curriculum;", hdr, re.S)
    assert m, "include/balatro_mi355x.h does not declare bg_curriculum"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.sub(r"\s+", " ", f.strip()) for f in body.split(";") if f.strip()]
    assert fields == ["int32_t* cap_dev", "int16_t* hist_dev", "int64_t* count_dev", "int32_t* at_level_dev", "uint8_t* raised_dev",
                      "int32_t window, increment", "double threshold"], fields
    assert [f[0] for f in nat.Curriculum._fields_] == ["cap_dev", "hist_dev", "count_dev", "at_level_dev", "raised_dev", "window", "increment", "threshold"]
    assert C.sizeof(nat.Curriculum) == 56 and nat.Curriculum.window.offset == 40 and nat.Curriculum.threshold.offset == 48
    m = re.search(r"\bint\s+bg_episode_ends_rows\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/balatro_mi355x.h does not declare bg_episode_ends_rows"
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == ["const uint8_t* rows_dev", "uint64_t row_stride_bytes", "int K", "int64_t N", "int64_t* report_dev", "const bg_curriculum* cur",
                      "float* kernel_ms_out", "void* stream"], params
    assert "bg_set_episode_summary" in nat.EXPORTS and "bg_episode_ends_rows" in nat.EXPORTS
    assert os.path.join(CSRC, "bg_ends.h") in build.DEPS
    eng = open(os.path.join(CSRC, "bg_engine3.h")).read()
    assert "a.safe.summary" in eng and "BG_ROW_END_ANTE" in eng
    if os.path.exists(build.LIB):   # (the GPU tests load the library, and loading checks every name of EXPORTS)
        L = C.CDLL(build.LIB)
        assert hasattr(L, "bg_set_episode_summary") and hasattr(L, "bg_episode_ends_rows")
    assert "RowCurriculum" in balatro_gym_amd.__all__ and "episode_ends" in balatro_gym_amd.__all__


# ---------------------------------------------------------------------------------------------------------------- the Python wrappers
class _StandIn:
    """What CurriculumTracker and RowCurriculum ask of an env: num_envs, a device, set_max_ante."""

    def __init__(self, n):
        self.num_envs, self.device, self.calls = n, "cpu", []

    def set_max_ante(self, max_ante, mask=None):
        self.calls.append((np.array(max_ante).copy(), None if mask is None else np.array(mask).copy()))


def test_wrappers_refuse_bad_arguments_before_the_library():
    import torch
    from balatro_gym_amd import EpisodeLimits, RowCurriculum, episode_ends
    from balatro_gym_amd.vec_env import RowBuffers
    N, K = 5, 6
    assert EpisodeLimits(N, "cpu").summary is False and EpisodeLimits(N, "cpu", summary=True).summary is True
    assert "summary" not in EpisodeLimits(N, "cpu", summary=True).state_dict()   # the switch is no carried state
    with pytest.raises(ValueError, match="summary must be a bool"):
        EpisodeLimits(N, "cpu", summary=1)
    rb = RowBuffers(N, torch.device("cpu"), steps=K, row_stride=384)
    assert rb.end_ante.dtype == torch.int16 and rb.end_round.dtype == torch.int8 and rb.end_chips.dtype == torch.uint32
    assert tuple(rb.end_ante.shape) == tuple(rb.end_round.shape) == tuple(rb.end_chips.shape) == (K, N)
    rows = synthetic_rows(np.random.default_rng(2), K, N, 384)
    rb.rows.copy_(torch.from_numpy(rows))
    _, _, ante, rnd, chips = ref.fields(rows)
    assert np.array_equal(rb.end_ante.numpy(), ante) and np.array_equal(rb.end_round.numpy(), rnd) and np.array_equal(rb.end_chips.numpy(), chips)
    # the scan's wrappers
    env = _StandIn(N)
    cur = RowCurriculum(env, initial_max_ante=2, ante_increment=1, success_threshold=0.8, window=4)
    assert len(env.calls) == 1 and int(env.calls[0][0]) == 2 and env.calls[0][1] is None
    assert (cur.cap.dtype, cur.hist.dtype, cur.count.dtype, cur.at_level.dtype, cur.raised.dtype) == (torch.int32, torch.int16, torch.int64, torch.int32, torch.uint8)
    assert tuple(cur.hist.shape) == (4, N) and cur.cap.tolist() == [2] * N
    s = cur._struct()
    assert (s.cap_dev, s.hist_dev, s.window, s.increment, s.threshold) == (cur.cap.data_ptr(), cur.hist.data_ptr(), 4, 1, 0.8)
    for bad in ({"initial_max_ante": 0}, {"initial_max_ante": 256}, {"ante_increment": 0}, {"ante_increment": 256}):
        with pytest.raises(ValueError, match=r"1\.\.255"):
            RowCurriculum(env, **bad)
    with pytest.raises(ValueError, match="window"):
        RowCurriculum(env, window=0)
    with pytest.raises(ValueError, match="finite"):
        RowCurriculum(env, success_threshold=float("nan"))
    for call in (episode_ends, cur.update):
        with pytest.raises(ValueError, match="contiguous uint8"):
            call(rb.rows[:, :, :352])
        with pytest.raises(ValueError, match="contiguous uint8"):
            call(rb.rows.to(torch.int8))
        with pytest.raises(ValueError, match="record stride"):
            call(torch.zeros((K, N, 360), dtype=torch.uint8))
        with pytest.raises(ValueError, match="device tensor"):
            call(rb.rows)
    with pytest.raises(ValueError, match=f"records of {N} envs"):
        cur.update(torch.zeros((K, N + 1, 384), dtype=torch.uint8))
    # the state dict
    cur.cap[:] = torch.tensor([2, 3, 2, 4, 2], dtype=torch.int32)
    cur.count[:] = 7
    cur.hist[1, 2] = 9
    sd = cur.state_dict()
    other = RowCurriculum(_StandIn(N), initial_max_ante=1, window=4)
    other.load_state_dict(sd)
    assert other.cap.tolist() == [2, 3, 2, 4, 2] and other.count.tolist() == [7] * N and int(other.hist[1, 2]) == 9
    assert other.env.calls[-1][0].tolist() == [2, 3, 2, 4, 2]
    with pytest.raises(ValueError, match="another window"):
        RowCurriculum(_StandIn(N), window=5).load_state_dict(sd)
    sd["cap"] = sd["cap"][:-1]
    with pytest.raises(ValueError, match="cap must have shape"):
        other.load_state_dict(sd)


# ---------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("window", [1, 2, 100])
@pytest.mark.parametrize("threshold", [0.0, 0.8, 1.0])
def test_restatement_is_curriculum_tracker(window, threshold):
    """ends_ref.Curriculum.episode against sb3_adapter.CurriculumTracker.update ITSELF, on a stand-in env: random episode streams of 24 envs (each
    env finishes an episode in a step with its own probability, its final ante drawn around its cap), every step's caps, histories, counts, levels
    and raised masks equal, and every set_max_ante the tracker makes is the restatement's caps under the restatement's mask."""
    from balatro_gym_amd.sb3_adapter import CurriculumTracker
    n, steps = 24, 12 if window == 1 else (40 if window == 2 else 900)
    rng = np.random.default_rng(1000 * window + int(10 * threshold))
    env = _StandIn(n)
    trk = CurriculumTracker(env, initial_max_ante=2, ante_increment=1 + window % 2, success_threshold=threshold, window=window)
    cur = ref.Curriculum(n, 2, 1 + window % 2, threshold, window)
    p_done = rng.uniform(0.2, 1.0, n)
    raises = 0
    for t in range(steps):
        done = rng.random(n) < p_done
        # around the cap: env e reaches its cap with a probability of its own, so that some envs sit just below and some just above the threshold
        ante = np.where(rng.random(n) < np.linspace(0.6, 1.0, n), cur.cap + rng.integers(0, 2, n), rng.integers(1, 3, n)).astype(np.int64)
        ncalls = len(env.calls)
        want = trk.update(done, ante)
        got = np.array([cur.episode(e, int(ante[e])) if done[e] else False for e in range(n)])
        assert np.array_equal(got, want), t
        assert np.array_equal(cur.cap, trk.cap) and np.array_equal(cur.count, trk.count) and np.array_equal(cur.at_level, trk.at_level), t
        assert np.array_equal(cur.hist.T, trk.hist), t
        if want.any():
            assert len(env.calls) == ncalls + 1 and np.array_equal(env.calls[-1][0], cur.cap) and np.array_equal(env.calls[-1][1], got)
        raises += int(want.sum())
    assert int(cur.count.min()) >= (window if window < 100 else 150)
    if threshold < 1.0:
        assert raises >= n, raises
    if window == 100:
        assert 0 < raises and (cur.at_level >= window).any() == (threshold > 0.0)   # at 0.8 / 1.0 some env sits at its level past the window


@pytest.mark.parametrize("window", [1, 4, 100])
def test_compiled_rule_is_the_restatement(exe, window):
    """csrc/bg_ends.h compiled for the host (under AddressSanitizer + UBSan) on synthetic records -- N = 77, K = 53 twice, stride 352 and 384, end
    antes 0..20, flags {1, 2, 4, 6}, chips to 2**32 - 1 --: the report and the curriculum's state equal ends_ref's after each call, with and without
    the curriculum."""
    rng = np.random.default_rng(window)
    N, K = 77, 53
    cur = ref.Curriculum(N, 3, 2, 0.8 if window > 1 else 1.0, window)
    cur.cap[:] = rng.integers(1, 12 if window < 100 else 5, N)
    cur.cap[::13] = 0      # no cap: never raised
    cur.cap[5::13] = 254   # the clamp at 255 (these envs end at antes 250..300 below)
    if window == 100:      # a job well under way: full and partly filled histories, envs close to and past a whole window at their level
        cur.hist[:] = rng.integers(1, 7, (window, N))
        cur.count[:] = rng.integers(0, 300, N)
        cur.at_level[:] = np.minimum(cur.count, rng.integers(80, 130, N))
    raises = 0
    for stride in (352, 384):
        rows = synthetic_rows(rng, K, N, stride, max_ante=20 if window < 100 else 6)
        high = np.ascontiguousarray(rng.integers(250, 301, (K, len(range(5, N, 13)), 1)).astype(np.int16)).view(np.uint8)
        rows[:, 5::13, ref.R_END_ANTE:ref.R_END_ANTE + 2] = high
        rep0, cap0, *_ = _run(exe, rows, cur, with_cur=False)
        assert np.array_equal(rep0, ref.report(rows)) and np.array_equal(cap0, cur.cap)
        rep, cap, hist, count, at_level, raised = _run(exe, rows, cur)
        want_raised = cur.update(rows)
        assert np.array_equal(rep, ref.report(rows, int(want_raised.sum())))
        assert np.array_equal(raised != 0, want_raised)
        assert np.array_equal(cap, cur.cap) and np.array_equal(hist, cur.hist) and np.array_equal(count, cur.count) and np.array_equal(at_level, cur.at_level)
        assert rep[9] > 0 and rep[16] == 0 and rep[31] > 0 or window == 100
        raises += int(want_raised.sum())
    # (window 100: a history of low antes does not turn over in 2 x 53 steps, so only the short windows see the clamp at work)
    assert raises > 0 and (cur.cap[::13] == 0).all() and cur.cap.max() == (255 if window < 100 else 254)
