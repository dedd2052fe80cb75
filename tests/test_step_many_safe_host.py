"""bg_step_many_rows_ex on the CPU (no GPU): csrc/bg_safe.h -- SafeBalatroEnv's rule of one step, the very text the owner lanes of bg_engine3.h's SAFE
instantiation run -- is compiled with g++ (-DBG_SAFE_HOST) into a small program and held, on every element, to the reference's OWN wrapper output
(tests/golden/sb3_fixed.npz: SafeBalatroEnv(BalatroEnvFixed(seed + rank), 5, 40), 24 envs x 120 steps); so is the Python restatement tests/safe_ref.py,
the oracle-side wrapper of the GPU tests.  The same program runs once under AddressSanitizer + UBSan.  Also: the header's declarations and constants,
the exports, build.DEPS, and the argument checks of the Python wrappers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import safe_ref as ref
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")

# in: T, N, the two limits, then per step t and env e (step-major) a float64 reward and a uint8 env-terminated; out: float64 reward [T, N], uint8 flags
# [T, N], int32 counters [N, 2] behind the last step; `slots K a b` prints bg_safe_slots
_PROGRAM = r"""
#define BG_SAFE_HOST
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "balatro_mi355x.h"
#include "bg_safe.h"
int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "slots")) { printf("%d\n", (int)bg_safe_slots(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]))); return 0; }
  if (argc != 7 || strcmp(argv[1], "run")) return 2;
  const size_t T = strtoull(argv[2], 0, 10), N = strtoull(argv[3], 0, 10);
  const int32_t max_invalid = atoi(argv[4]), max_steps = atoi(argv[5]);
  double* rw = (double*)malloc(T * N * 8 + 8);
  uint8_t* et = (uint8_t*)malloc(T * N + 1);
  FILE* in = fopen(argv[6], "rb");
  if (!in || fread(rw, 8, T * N, in) != T * N || fread(et, 1, T * N, in) != T * N) return 4;
  fclose(in);
  uint8_t* fl = (uint8_t*)malloc(T * N + 1);
  int32_t* cn = (int32_t*)calloc(2 * N + 1, 4);
  for (size_t t = 0; t < T; t++)
    for (size_t e = 0; e < N; e++) {
      const BgSafeStep o = bg_safe_step(rw[t * N + e], et[t * N + e] != 0, cn[2 * e], cn[2 * e + 1], max_invalid, max_steps);
      cn[2 * e] = o.episode_steps; cn[2 * e + 1] = o.consecutive_invalid;
      rw[t * N + e] = o.reward; fl[t * N + e] = (uint8_t)o.flags;
      if (bg_safe_wrapper_ending(o.flags) != (o.flags != 0 && !(o.flags & BG_END_GAME))) return 6;
    }
  FILE* out = fopen(argv[6], "wb");
  if (!out || fwrite(rw, 8, T * N, out) != T * N || fwrite(fl, 1, T * N, out) != T * N || fwrite(cn, 4, 2 * N, out) != 2 * N) return 5;
  fclose(out);
  free(rw); free(et); free(fl); free(cn);
  return 0;
}
"""


def _compile(d, name, extra):
    assert shutil.which("g++"), "g++ is needed to compile csrc/bg_safe.h for the host"
    src = d / "safe_host.cpp"
    src.write_text(_PROGRAM)
    exe = d / name
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", *extra, "-I", CSRC, "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    return exe


def _run(exe, d, reward, env_term, max_invalid, max_steps):
    """reward float64 / env_term bool [T, N] through the compiled rule: (reward, flags, counters [N, 2])."""
    T, N = reward.shape
    path = d / "io.bin"
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(reward, np.float64).tobytes())
        f.write(np.ascontiguousarray(env_term, np.uint8).tobytes())
    subprocess.check_call([str(exe), "run", str(T), str(N), str(max_invalid), str(max_steps), str(path)])
    raw = path.read_bytes()
    rw = np.frombuffer(raw[:T * N * 8], np.float64).reshape(T, N)
    fl = np.frombuffer(raw[T * N * 8:T * N * 9], np.uint8).reshape(T, N)
    cn = np.frombuffer(raw[T * N * 9:], np.int32).reshape(N, 2)
    return rw, fl, cn


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("safe_host")


@pytest.fixture(scope="module")
def exe(workdir):
    return _compile(workdir, "safe_host", [])


@pytest.fixture(scope="module")
def golden():
    return ref.load_golden()


def _assert_golden(g, reward, flags):
    """Wrapped rewards / flags [env, step] against everything the golden recorded of the wrapper."""
    kill, mx, game = flags & ref.END_INVALID != 0, flags & ref.END_MAX_STEPS != 0, flags & ref.END_GAME != 0
    assert np.array_equal(reward.astype(np.float32).view(np.uint32), g["rewards"].view(np.uint32))
    assert np.array_equal(flags != 0, g["dones"] != 0)
    assert np.array_equal(kill, g["invalid_action_termination"] != 0)
    assert np.array_equal(mx, g["max_steps_reached"] != 0)
    assert np.array_equal(mx, g["truncated"] != 0)
    assert np.array_equal(game | kill, g["terminated"] != 0)
    # what the fixture holds: a changed fixture must not hollow the test out
    counts = (int(kill.sum()), int((mx & ~kill & ~game).sum()), int(game.sum()), int((game & mx).sum()))   # kills, time limit alone, game overs, of which on the limit's step
    assert counts == (144, 30, 25, 2), counts


def test_rule_reproduces_the_reference_wrapper(exe, workdir, golden):
    """bg_safe.h, compiled for the host, on the golden's inner signals (reward with -50 -> -1, env terminated = terminated & ~kill): rewards, dones,
    invalid_action_termination, max_steps_reached and truncated of every one of the 24 x 120 steps."""
    g = golden
    reward, env_term, want_flags = ref.golden_inner(g)
    rw, fl, cn = _run(exe, workdir, reward.T, env_term.T, int(g["max_invalid_actions"]), int(g["max_episode_steps"]))
    _assert_golden(g, rw.T, fl.T)
    assert np.array_equal(fl.T, want_flags)
    # the counters behind the last step, from the golden alone: steps since the env's last done, -1.0 rewards at the end of that stretch
    for e in range(reward.shape[0]):
        done = np.flatnonzero(g["dones"][e])
        tail = reward[e, (done[-1] + 1 if done.size else 0):]
        run = 0
        for r in tail[::-1]:
            if r != -1.0:
                break
            run += 1
        assert tuple(cn[e]) == (tail.size, run), (e, cn[e], tail.size, run)


def test_python_restatement_reproduces_the_reference_wrapper(golden):
    """tests/safe_ref.py's SafeCounters, the wrapper the GPU tests put around the oracle's envs, on the same signals."""
    g = golden
    reward, env_term, _ = ref.golden_inner(g)
    S, T = reward.shape
    rw, fl = np.zeros((S, T)), np.zeros((S, T), np.uint8)
    for e in range(S):
        c = ref.SafeCounters(int(g["max_invalid_actions"]), int(g["max_episode_steps"]))
        for t in range(T):
            rw[e, t], fl[e, t] = c.step(reward[e, t], bool(env_term[e, t]))
            assert ref.wrapper_ending(int(fl[e, t])) == bool(g["dones"][e, t] and not env_term[e, t])
    _assert_golden(g, rw, fl)


def test_rule_at_its_edges(exe, workdir):
    """Rewards next to -1.0 do not count; a terminated -1.0 step does not count and zeroes the run; a kill and the step limit on one step; limits
    of 2**30 never fire: compiled rule == Python restatement on synthetic signals."""
    rng = np.random.default_rng(5)
    T, N = 200, 16
    reward = rng.choice([-1.0, np.nextafter(-1.0, 0.0), np.nextafter(-1.0, -2.0), 0.0, -0.0, 1.5, -50.0, np.float64(np.float32(-1.0))], size=(T, N), p=[.65, .02, .02, .1, .02, .1, .02, .07])
    env_term = rng.random((T, N)) < 0.03
    for lim in ((3, 3), (3, 17), (4, 8), (6, 6), (2 ** 30, 2 ** 30)):
        rw, fl, cn = _run(exe, workdir, reward, env_term, *lim)
        seen = set()
        for e in range(N):
            c = ref.SafeCounters(*lim)
            for t in range(T):
                r, f = c.step(reward[t, e], bool(env_term[t, e]))
                assert (r, f) == (rw[t, e], fl[t, e]), (lim, t, e)
                seen.add(f)
            assert (c.episode_steps, c.consecutive_invalid) == tuple(cn[e])
        if lim == (6, 6):
            assert 6 in seen   # kill and step limit together
        if lim[0] == 2 ** 30:
            assert seen == {0, 1} and np.array_equal(rw, reward)


def test_rule_under_sanitizers(workdir, golden):
    """The same program built with -fsanitize=address,undefined runs the golden clean (a stand-alone CPU program; nothing of it touches a GPU)."""
    exe = _compile(workdir, "safe_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    reward, env_term, want_flags = ref.golden_inner(golden)
    _, fl, _ = _run(exe, workdir, reward.T, env_term.T, int(golden["max_invalid_actions"]), int(golden["max_episode_steps"]))
    assert np.array_equal(fl.T, want_flags)


def test_terminal_slots(exe):
    """bg_safe_slots = K / min(limits) + 1 (header, program and Python restatement agree), and the library's bg_safe_terminal_slots refuses limits < 3."""
    for K, a, b in ((1, 3, 3), (2, 3, 17), (3, 3, 17), (48, 3, 17), (48, 5, 40), (120, 5, 40), (144, 17, 3), (100, 50, 1000), (2048, 50, 1000), (49, 50, 1000), (50, 50, 1000)):
        got = int(subprocess.check_output([str(exe), "slots", str(K), str(a), str(b)]))
        assert got == K // min(a, b) + 1 == ref.terminal_slots(K, a, b), (K, a, b, got)
    from balatro_gym_amd import build
    if os.path.exists(build.LIB):   # (a tree without a built library checks nothing here: tests/test_step_many_safe.py repeats it on the library it loads)
        L = C.CDLL(build.LIB)
        L.bg_safe_terminal_slots.argtypes = [C.c_int, C.c_int, C.c_int]
        assert L.bg_safe_terminal_slots(48, 3, 17) == 17 and L.bg_safe_terminal_slots(100, 50, 1000) == 3 and L.bg_safe_terminal_slots(0, 3, 3) == 1
        assert L.bg_safe_terminal_slots(48, 2, 17) == -1 and L.bg_safe_terminal_slots(48, 17, 2) == -1 and L.bg_safe_terminal_slots(-1, 3, 3) == -1


def test_header_exports_and_build():
    from balatro_gym_amd import _native as nat, build
    hdr = open(HEADER).read()
    for name, val in (("BG_ROW_END_FLAGS", "343"), ("BG_END_GAME", "1u"), ("BG_END_INVALID", "2u"), ("BG_END_MAX_STEPS", "4u")):
        assert re.search(rf"#define {name} {val}\b", hdr), name
    assert (nat.ROW_END_FLAGS, nat.END_GAME, nat.END_INVALID, nat.END_MAX_STEPS) == (343, 1, 2, 4) == (343, ref.END_GAME, ref.END_INVALID, ref.END_MAX_STEPS)
    assert nat.ROW_EXTRA["terminated"][0] + 1 == nat.ROW_END_FLAGS < nat.ROW_BYTES
    m = re.search(r"typedef struct bg_safe_limits \{(.*?)\} bg_safe_limits;", hdr, re.S)
    assert m, "include/balatro_mi355x.h does not declare bg_safe_limits"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.sub(r"\s+", " ", f.strip()) for f in body.split(";") if f.strip()]
    assert fields == ["int32_t max_invalid_actions, max_episode_steps", "int32_t* counters_dev", "uint8_t* terminal_rows_dev", "uint64_t terminal_stride_bytes",
                      "int32_t* terminal_step_dev", "int32_t terminal_slots"], fields
    # the ctypes mirror: same order, same sizes
    assert [f[0] for f in nat.SafeLimits._fields_] == ["max_invalid_actions", "max_episode_steps", "counters_dev", "terminal_rows_dev", "terminal_stride_bytes",
                                                      "terminal_step_dev", "terminal_slots"]
    assert C.sizeof(nat.SafeLimits) == 48 and nat.SafeLimits.counters_dev.offset == 8 and nat.SafeLimits.terminal_slots.offset == 40
    m = re.search(r"\bint\s+bg_step_many_rows_ex\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/balatro_mi355x.h does not declare bg_step_many_rows_ex"
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == ["bg_handle* h", "int K", "const int32_t* actions_dev", "uint8_t* rows_dev", "uint64_t row_stride_bytes", "int rows_stride_steps",
                      "const bg_safe_limits* limits", "bg_rollout_stats* stats_dev", "void* stream"], params
    assert re.search(r"\bint\s+bg_safe_terminal_slots\s*\(\s*int K,\s*int max_invalid_actions,\s*int max_episode_steps\s*\)\s*;", hdr)
    doc = hdr[:hdr.index("#define BG_ROW_END_FLAGS")].rsplit("/*", 1)[1]
    for cite in ("train_balatro_fixed.py:228-277", "robust_training.py:35", "SafeBalatroEnv", "terminal_observation", "BG_FLAG_AUTORESET", "-50.0", "TimeLimit.truncated"):
        assert cite in doc, cite
    assert "bg_step_many_rows_ex" in nat.EXPORTS and "bg_safe_terminal_slots" in nat.EXPORTS
    assert os.path.join(CSRC, "bg_safe.h") in build.DEPS
    safe_h = open(os.path.join(CSRC, "bg_safe.h")).read()
    assert "BG_SAFE_HOST" in safe_h and int(re.search(r"#define BG_SAFE_MIN_LIMIT (\d+)", safe_h).group(1)) == nat.SAFE_MIN_LIMIT == 3
    eng = open(os.path.join(CSRC, "bg_engine3.h")).read()
    assert "bool ACT = false, bool SAFE = false>" in eng and "bg_safe_step(" in eng
    if os.path.exists(build.LIB):   # (as above: the GPU tests load the library, and loading checks every name of EXPORTS)
        L = C.CDLL(build.LIB)
        assert hasattr(L, "bg_step_many_rows_ex") and hasattr(L, "bg_safe_terminal_slots")
    import balatro_gym_amd
    assert "EpisodeLimits" in balatro_gym_amd.__all__


def test_wrappers_refuse_bad_arguments_before_the_library():
    """EpisodeLimits / RowBuffers.bootstrap_rewards on CPU tensors: sizes, the limits' floor, masks, state dicts, the bootstrap's arithmetic."""
    import torch
    from balatro_gym_amd import EpisodeLimits
    from balatro_gym_amd.vec_env import RowBuffers
    N, K = 5, 12
    lim = EpisodeLimits(N, "cpu", max_invalid_actions=5, max_episode_steps=40, steps=K, row_stride=384)
    assert lim.slots == K // 5 + 1 == 3
    assert lim.counters.dtype == torch.int32 and tuple(lim.counters.shape) == (N, 4)
    assert lim.terminal_rows.dtype == torch.uint8 and tuple(lim.terminal_rows.shape) == (3, N, 384)
    assert lim.terminal_step.dtype == torch.int32 and tuple(lim.terminal_step.shape) == (3, N) and bool((lim.terminal_step == -1).all())
    assert EpisodeLimits(N, "cpu").slots == 1 and EpisodeLimits(N, "cpu", steps=2048).slots == 2048 // 50 + 1
    for bad in ({"max_invalid_actions": 2}, {"max_episode_steps": 2}, {"max_invalid_actions": 0}, {"max_episode_steps": 2 ** 31}):
        with pytest.raises(ValueError, match=">= 3"):
            EpisodeLimits(N, "cpu", **bad)
    with pytest.raises(ValueError, match="row_stride"):
        EpisodeLimits(N, "cpu", row_stride=360)
    with pytest.raises(ValueError, match="steps >= 1"):
        EpisodeLimits(N, "cpu", steps=0)
    s = lim._struct()
    assert (s.max_invalid_actions, s.max_episode_steps, s.counters_dev, s.terminal_stride_bytes, s.terminal_slots) == (5, 40, lim.counters.data_ptr(), 384, 3)
    # reset / state dict
    lim.counters[:, 0] = 7
    lim.counters[:, 1] = 2
    sd = lim.state_dict()
    lim.reset(torch.tensor([True, False, False, True, False]))
    assert lim.counters[:, 0].tolist() == [0, 7, 7, 0, 7] and lim.counters[:, 1].tolist() == [0, 2, 2, 0, 2]
    with pytest.raises(ValueError, match="mask must have shape"):
        lim.reset(torch.zeros(N + 1, dtype=torch.bool))
    lim.reset()
    assert not lim.counters.any()
    lim.load_state_dict(sd)
    assert lim.counters[:, 0].tolist() == [7] * N
    with pytest.raises(ValueError, match="other limits"):
        EpisodeLimits(N, "cpu", 6, 40).load_state_dict(sd)
    with pytest.raises(ValueError, match="counters must have shape"):
        EpisodeLimits(N + 1, "cpu", 5, 40).load_state_dict(sd)
    # terminal(): ascending t * N + e whatever the slot; bootstrap_rewards adds only where the flags are exactly END_MAX_STEPS
    rb = RowBuffers(N, torch.device("cpu"), steps=K, row_stride=384)
    assert rb.end_flags.dtype == torch.uint8 and tuple(rb.end_flags.shape) == (K, N)
    rb.rows[3, 1, 343] = 9
    assert int(rb.end_flags[3, 1]) == 9
    rb.rows[3, 1, 343] = 0
    ends = [(0, 4, 7, 4), (1, 4, 11, 2), (0, 2, 0, 6), (0, 0, 5, 4)]   # slot, env, step, flags
    for j, e, t, f in ends:
        lim.terminal_step[j, e] = t
        lim.terminal_rows[j, e, :] = 10 * j + e
        rb.end_flags[t, e] = f
        rb.terminated[t, e] = 1
    rb.reward[:] = 1.0
    index, recs = lim.terminal()
    assert index.dtype == torch.int32 and index.tolist() == [0 * N + 2, 5 * N + 0, 7 * N + 4, 11 * N + 4]
    assert recs.dtype == torch.uint8 and tuple(recs.shape) == (4, 384) and recs[:, 0].tolist() == [2, 0, 4, 14]
    tv = torch.tensor([100.0, 200.0, 300.0, 400.0])
    out = rb.bootstrap_rewards(lim, tv, gamma=0.5)
    want = np.ones((K, N))
    want[5, 0] += 0.5 * 200.0
    want[7, 4] += 0.5 * 300.0
    assert out.dtype == torch.float64 and np.array_equal(out.numpy(), want)
    assert np.array_equal(out.numpy(), ref.bootstrap(np.ones((K, N)), rb.end_flags.numpy(), index.numpy(), tv.numpy(), 0.5))
    given = torch.full((K, N), 2.0, dtype=torch.float64)
    out2 = rb.bootstrap_rewards(lim, tv, gamma=0.5, rewards=given)
    assert np.array_equal(out2.numpy(), want + 1.0) and bool((given == 2.0).all())
    with pytest.raises(ValueError, match="terminal_values must have shape"):
        rb.bootstrap_rewards(lim, tv[:3])
    with pytest.raises(ValueError, match="rewards must be"):
        rb.bootstrap_rewards(lim, tv, rewards=given.float())
    with pytest.raises(ValueError, match="do not hold"):
        RowBuffers(N, torch.device("cpu"), steps=K - 1, row_stride=384).bootstrap_rewards(lim, tv)
