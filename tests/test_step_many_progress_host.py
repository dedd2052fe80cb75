"""bg_step_many_rows_progress on the CPU (no GPU): csrc/bg_progress.h -- ProgressionRewardWrapper's rule of one step, the very text the owner lanes of
bg_engine3.h's PROG instantiation run -- is compiled with g++ (-DBG_PROGRESS_HOST -DBG_SAFE_HOST) into a small program that composes it with bg_safe.h
as the engine does, and held, on every element, to the reference's OWN wrapper stack (tests/golden/progression.npz, made by tools/gen_progress_golden.py:
SafeBalatroEnv(ProgressionRewardWrapper(BalatroEnvFixed(seed + rank)), 50, 610), 8 scripted envs x 640 steps); so is the Python restatement
tests/progress_ref.py, the oracle-side wrapper of the GPU tests.  Rewards are compared as float64 bit patterns.  The same program runs once under
AddressSanitizer + UBSan.  Also: the packing of the carry, the header's declarations, constants and citations, the exports, build.DEPS, and the
argument checks of the Python wrappers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import progress_ref as ref
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")

# `run T N max_invalid max_steps file`: in: per step t and env e (step-major) float64 reward, then uint8 env-terminated, int32 ante, int32 round; out:
# float64 reward [T, N], uint8 flags [T, N], int32 packed carry [T, N, 4] behind every step, int32 limits' counters [N, 2] behind the last step.
# `slots K a b` prints bg_progress_slots; `pack a b c d e` prints the four packed words and what unpacking them gives.
_PROGRAM = r"""
#define BG_SAFE_HOST
#define BG_PROGRESS_HOST
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "balatro_mi355x.h"
#include "bg_safe.h"
#include "bg_progress.h"
int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "slots")) { printf("%d\n", (int)bg_progress_slots(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]))); return 0; }
  if (argc == 7 && !strcmp(argv[1], "pack")) {
    BgProgressCarry c = {atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6])};
    const BgProgressPacked p = bg_progress_pack(c);
    const BgProgressCarry u = bg_progress_unpack(p);
    printf("%d %d %d %d %d %d %d %d %d\n", p.w[0], p.w[1], p.w[2], p.w[3], u.total_steps, u.steps_on_current_ante, u.last_ante, u.last_round, u.max_ante_reached);
    return 0;
  }
  if (argc != 7 || strcmp(argv[1], "run")) return 2;
  const size_t T = strtoull(argv[2], 0, 10), N = strtoull(argv[3], 0, 10);
  const int32_t max_invalid = atoi(argv[4]), max_steps = atoi(argv[5]);
  double* rw = (double*)malloc(T * N * 8 + 8);
  uint8_t* et = (uint8_t*)malloc(T * N + 1);
  int32_t* an = (int32_t*)malloc(T * N * 4 + 4);
  int32_t* rd = (int32_t*)malloc(T * N * 4 + 4);
  FILE* in = fopen(argv[6], "rb");
  if (!in || fread(rw, 8, T * N, in) != T * N || fread(et, 1, T * N, in) != T * N || fread(an, 4, T * N, in) != T * N || fread(rd, 4, T * N, in) != T * N) return 4;
  fclose(in);
  uint8_t* fl = (uint8_t*)malloc(T * N + 1);
  int32_t* cy = (int32_t*)malloc(T * N * 16 + 4);
  int32_t* cn = (int32_t*)calloc(2 * N + 1, 4);
  BgProgressPacked* pk = (BgProgressPacked*)calloc(N + 1, sizeof(BgProgressPacked));   // all-zero rows: the state after reset()
  for (size_t t = 0; t < T; t++)
    for (size_t e = 0; e < N; e++) {
      // the composition of bg_engine3.h's PROG instantiation
      const bool env_term = et[t * N + e] != 0;
      const BgProgressStep po = bg_progress_step(rw[t * N + e], an[t * N + e], rd[t * N + e], bg_progress_unpack(pk[e]));
      pk[e] = bg_progress_pack(po.carry);
      BgSafeStep so = bg_safe_step(po.reward, env_term || po.stuck, cn[2 * e], cn[2 * e + 1], max_invalid, max_steps);
      so.flags = (so.flags & ~BG_SAFE_END_GAME) | (env_term ? BG_SAFE_END_GAME : 0u) | (po.stuck ? BG_PROGRESS_END_STUCK : 0u);
      if (so.flags) memset(&pk[e], 0, sizeof(pk[e]));
      cn[2 * e] = so.episode_steps; cn[2 * e + 1] = so.consecutive_invalid;
      rw[t * N + e] = so.reward; fl[t * N + e] = (uint8_t)so.flags;
      memcpy(cy + 4 * (t * N + e), pk[e].w, 16);
      if (BG_PROGRESS_END_STUCK != BG_END_STUCK) return 6;
    }
  FILE* out = fopen(argv[6], "wb");
  if (!out || fwrite(rw, 8, T * N, out) != T * N || fwrite(fl, 1, T * N, out) != T * N || fwrite(cy, 16, T * N, out) != T * N || fwrite(cn, 4, 2 * N, out) != 2 * N) return 5;
  fclose(out);
  free(rw); free(et); free(an); free(rd); free(fl); free(cy); free(cn); free(pk);
  return 0;
}
"""


def _compile(d, name, extra):
    assert shutil.which("g++"), "g++ is needed to compile csrc/bg_progress.h for the host"
    src = d / "progress_host.cpp"
    src.write_text(_PROGRAM)
    exe = d / name
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", *extra, "-I", CSRC, "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    return exe


def _run(exe, d, reward, env_term, ante, round_, max_invalid, max_steps):
    """[T, N] signals through the compiled rule: (reward, flags, packed carry [T, N, 4], limits' counters [N, 2])."""
    T, N = reward.shape
    path = d / "io.bin"
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(reward, np.float64).tobytes())
        f.write(np.ascontiguousarray(env_term, np.uint8).tobytes())
        f.write(np.ascontiguousarray(ante, np.int32).tobytes())
        f.write(np.ascontiguousarray(round_, np.int32).tobytes())
    subprocess.check_call([str(exe), "run", str(T), str(N), str(max_invalid), str(max_steps), str(path)])
    raw = path.read_bytes()
    n = T * N
    rw = np.frombuffer(raw[:n * 8], np.float64).reshape(T, N)
    fl = np.frombuffer(raw[n * 8:n * 9], np.uint8).reshape(T, N)
    cy = np.frombuffer(raw[n * 9:n * 25], np.int32).reshape(T, N, 4)
    cn = np.frombuffer(raw[n * 25:], np.int32).reshape(N, 2)
    return rw, fl, cy, cn


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("progress_host")


@pytest.fixture(scope="module")
def exe(workdir):
    return _compile(workdir, "progress_host", [])


@pytest.fixture(scope="module")
def golden():
    return ref.load_golden()


def _python_rule(g):
    """tests/progress_ref.py over the golden's inner signals: (reward, flags, packed carry) [env, step]."""
    S, T = g["actions"].shape
    rw, fl, cy = np.zeros((S, T)), np.zeros((S, T), np.uint8), np.zeros((S, T, 4), np.int32)
    for e in range(S):
        w = ref.ProgressSafe(int(g["max_invalid_actions"]), int(g["max_episode_steps"]))
        for t in range(T):
            rw[e, t], fl[e, t] = w.step(g["inner_reward"][e, t], bool(g["inner_terminated"][e, t]), g["ante"][e, t], g["round"][e, t])
            cy[e, t] = w.prog.pack()
    return rw, fl, cy


def _assert_golden(g, reward, flags):
    """Shaped rewards / flags [env, step] against everything the golden recorded of the wrapper stack."""
    stuck, kill, mx, game = (flags & b != 0 for b in (ref.END_STUCK, ref.END_INVALID, ref.END_MAX_STEPS, ref.END_GAME))
    assert np.array_equal(reward.view(np.uint64), g["reward"].view(np.uint64)), np.argwhere(reward.view(np.uint64) != g["reward"].view(np.uint64))[:4]
    assert np.array_equal(stuck, g["stuck_on_ante_1"] != 0)
    assert np.array_equal(kill, g["invalid_action_termination"] != 0)
    assert np.array_equal(mx, g["max_steps_reached"] != 0) and np.array_equal(mx, g["truncated"] != 0)
    assert np.array_equal(game, g["inner_terminated"] != 0)
    assert np.array_equal(game | kill | stuck, g["terminated"] != 0)
    assert np.array_equal(flags != 0, (g["terminated"] != 0) | (g["truncated"] != 0))


def test_golden_holds_every_branch(golden):
    """What the fixture must contain, from the golden and the rule's inputs alone (a changed fixture must not hollow the tests out): an ante bonus, a
    round bonus, a personal-best bonus, the ante-1 penalty, a stuck ending, each of the three tiers, the efficiency bonus, an invalid-action kill, a
    step-limit ending, and a run of >= max_invalid_actions invalid actions that is not counted because the shaped reward is not -1.0."""
    g = golden
    S, T = g["actions"].shape
    seen = dict.fromkeys(("ante_bonus", "round_bonus", "best_bonus", "ante1_penalty", "tier2", "tier3", "tier4", "efficiency", "uncounted_run"), 0)
    mi = int(g["max_invalid_actions"])
    for e in range(S):
        c, run = ref.ProgressCarry(), 0
        for t in range(T):
            a, r = int(g["ante"][e, t]), int(g["round"][e, t])
            la, lr, mx = c.last_ante, c.last_round, c.max_ante_reached
            c.step(g["inner_reward"][e, t], a, r)
            seen["ante_bonus"] += a > la
            seen["round_bonus"] += r > lr and a == max(a, la)
            seen["best_bonus"] += a > mx
            seen["ante1_penalty"] += a == 1 and c.steps_on_current_ante > 150
            tier = 2 if c.total_steps > 200 and a < 2 else 3 if c.total_steps > 400 and a < 3 else 4 if c.total_steps > 600 and a < 4 else 0
            if tier:
                seen[f"tier{tier}"] += 1
            seen["efficiency"] += a >= 3 and c.total_steps < 300
            done = bool(g["terminated"][e, t] or g["truncated"][e, t])
            run = run + 1 if g["inner_reward"][e, t] == -1.0 and not done and g["reward"][e, t] != -1.0 else 0
            seen["uncounted_run"] += run == mi
            if done:
                c.reset()
    assert all(v > 0 for v in seen.values()), seen
    counts = tuple(int(g[k].sum()) for k in ("stuck_on_ante_1", "invalid_action_termination", "max_steps_reached"))
    assert counts == (3, 18, 5), counts
    assert str(g["roles"][4]) == "invalid_late" and not g["invalid_action_termination"][4, :301].any() and (g["actions"][4, 205:301] == 59).all()


def test_rule_reproduces_the_reference_wrapper(exe, workdir, golden):
    """bg_progress.h + bg_safe.h, compiled for the host and composed as in the engine, on the golden's inner signals: the stack's float64 rewards bit
    for bit, terminated, truncated and the three info flags of every one of the 8 x 640 steps; the carries equal the Python restatement's."""
    g = golden
    rw, fl, cy, cn = _run(exe, workdir, g["inner_reward"].T, g["inner_terminated"].T, g["ante"].T, g["round"].T, int(g["max_invalid_actions"]), int(g["max_episode_steps"]))
    _assert_golden(g, np.ascontiguousarray(rw.T), fl.T)
    prw, pfl, pcy = _python_rule(g)
    assert np.array_equal(fl.T, pfl) and np.array_equal(cy.transpose(1, 0, 2), pcy)
    assert np.array_equal(np.ascontiguousarray(rw.T).view(np.uint64), prw.view(np.uint64))
    # the limits' counters behind the last step: steps since the env's last done
    for e in range(g["actions"].shape[0]):
        done = np.flatnonzero((g["terminated"][e] != 0) | (g["truncated"][e] != 0))
        assert cn[e, 0] == g["actions"].shape[1] - (done[-1] + 1 if done.size else 0)


def test_python_restatement_reproduces_the_reference_wrapper(golden):
    """tests/progress_ref.py's ProgressSafe, the wrapper the GPU tests put around the oracle's envs, on the same signals."""
    rw, fl, _ = _python_rule(golden)
    _assert_golden(golden, rw, fl)
    for f in np.unique(fl):
        assert ref.wrapper_ending(int(f)) == bool(f != 0 and not f & ref.END_GAME)


def test_rule_on_synthetic_signals(exe, workdir):
    """Antes that jump, fall and repeat, rounds 0..4, env endings anywhere, rewards next to -1.0, small limits: compiled rule == Python restatement on
    every reward bit, flag and carry word (the reference's line 117-118 included: an ante below last_ante copies the round)."""
    rng = np.random.default_rng(9)
    T, N = 700, 24
    reward = rng.choice([-1.0, 0.0, 0.1, 1.5, 89.2, -0.8, np.nextafter(-1.0, 0.0)], size=(T, N), p=[.3, .3, .1, .1, .1, .05, .05])
    ante = np.ones((T, N), np.int32)
    for e in range(N):
        if e % 3:
            ante[:, e] = np.maximum(1, np.cumsum(rng.choice([0, 0, 0, 1, 2, -1], size=T, p=[.9, .05, .02, .02, .005, .005]))).astype(np.int32) % 9 + (e % 3 == 2)
    round_ = rng.integers(0, 5, size=(T, N)).astype(np.int32)
    env_term = rng.random((T, N)) < 0.002
    for lim in ((50, 1000), (3, 3), (7, 320), (2 ** 30, 2 ** 30)):
        rw, fl, cy, cn = _run(exe, workdir, reward, env_term, ante, round_, *lim)
        seen = set()
        for e in range(N):
            w = ref.ProgressSafe(*lim)
            for t in range(T):
                r, f = w.step(reward[t, e], bool(env_term[t, e]), ante[t, e], round_[t, e])
                assert (np.float64(r).view(np.uint64), f) == (rw[t, e].view(np.uint64), fl[t, e]), (lim, t, e, r, rw[t, e], f, fl[t, e])
                assert np.array_equal(w.prog.pack(), cy[t, e]), (lim, t, e)
                seen.add(f)
            assert (w.safe.episode_steps, w.safe.consecutive_invalid) == tuple(cn[e])
        if lim[0] == 2 ** 30:
            assert ref.END_STUCK in seen and seen <= {0, ref.END_GAME, ref.END_STUCK, ref.END_GAME | ref.END_STUCK}, seen


def test_rule_under_sanitizers(workdir, golden):
    """The same program built with -fsanitize=address,undefined runs the golden clean (a stand-alone CPU program; nothing of it touches a GPU)."""
    g = golden
    exe = _compile(workdir, "progress_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    rw, fl, _, _ = _run(exe, workdir, g["inner_reward"].T, g["inner_terminated"].T, g["ante"].T, g["round"].T, int(g["max_invalid_actions"]), int(g["max_episode_steps"]))
    _assert_golden(g, np.ascontiguousarray(rw.T), fl.T)


def test_zero_carry_is_the_reset_state_and_packing_round_trips(exe):
    """Four zero words unpack to reset()'s state (train_progressive.py:33-41); the packing round-trips at the ends of its stated ranges: steps up to
    2**31 - 1, last_ante / max_ante_reached 1 .. 65536 (the engine's state.ante is one byte), last_round the whole int32 range minus one."""
    def pack(*c):
        out = [int(x) for x in subprocess.check_output([str(exe), "pack", *map(str, c)]).split()]
        return out[:4], tuple(out[4:])
    assert ref.ProgressCarry.unpack([0, 0, 0, 0]).values() == (0, 0, 1, 1, 1) == ref.ProgressCarry().values()
    assert not ref.ProgressCarry().pack().any()
    assert pack(0, 0, 1, 1, 1) == ([0, 0, 0, 0], (0, 0, 1, 1, 1))
    for c in ((2 ** 31 - 1, 2 ** 31 - 1, 65536, 2 ** 31 - 1, 65536), (1, 0, 1, -(2 ** 31) + 1, 65536), (1000, 301, 255, 3, 255), (5, 5, 101, 0, 102), (7, 0, 65536, 1, 1),
              (610, 0, 2, 1, 3)):
        words, back = pack(*c)
        assert back == c, (c, words, back)
        assert words == ref.ProgressCarry(*c).pack().tolist() and ref.ProgressCarry.unpack(words).values() == c
    # the engine's ranges lie inside: state.ante and state.round are bytes of chunk 3 (bg_pack), the game ends above ante 100
    dev = open(os.path.join(CSRC, "bg_device.h")).read()
    assert "bg_p4(e.ante, e.round, e.phase, e.hands_left)" in dev


def test_terminal_slots(exe):
    """bg_progress_slots = K / min(limits, 301) + 1 (header, program, Python restatement and EpisodeLimits(progression=True) agree)."""
    from balatro_gym_amd import EpisodeLimits, build
    for K, a, b in ((1, 3, 3), (48, 3, 17), (100, 50, 1000), (320, 1000, 1000), (300, 1000, 1000), (301, 400, 1000), (620, 2 ** 30, 610), (903, 2 ** 30, 2 ** 30), (2048, 50, 1000)):
        got = int(subprocess.check_output([str(exe), "slots", str(K), str(a), str(b)]))
        assert got == K // min(a, b, 301) + 1 == ref.terminal_slots(K, a, b), (K, a, b, got)
        assert EpisodeLimits(2, "cpu", a, b, steps=K, progression=True).slots == got
        assert EpisodeLimits(2, "cpu", a, b, steps=K).slots == K // min(a, b) + 1
    if os.path.exists(build.LIB):   # (a tree without a built library checks nothing here: tests/test_step_many_progress.py repeats it on the library it loads)
        L = C.CDLL(build.LIB)
        L.bg_progress_terminal_slots.argtypes = [C.c_int, C.c_int, C.c_int]
        assert L.bg_progress_terminal_slots(903, 2 ** 30, 2 ** 30) == 4 and L.bg_progress_terminal_slots(100, 50, 1000) == 3 and L.bg_progress_terminal_slots(0, 3, 3) == 1
        assert L.bg_progress_terminal_slots(48, 2, 17) == -1 and L.bg_progress_terminal_slots(48, 17, 2) == -1 and L.bg_progress_terminal_slots(-1, 3, 3) == -1


def test_header_exports_and_build():
    from balatro_gym_amd import _native as nat, build
    hdr = open(HEADER).read()
    assert re.search(r"#define BG_END_STUCK 8u\b", hdr)
    for name, val in (("BG_END_GAME", "1u"), ("BG_END_INVALID", "2u"), ("BG_END_MAX_STEPS", "4u")):   # unchanged
        assert re.search(rf"#define {name} {val}\b", hdr), name
    assert (nat.END_GAME, nat.END_INVALID, nat.END_MAX_STEPS, nat.END_STUCK) == (1, 2, 4, 8) == (ref.END_GAME, ref.END_INVALID, ref.END_MAX_STEPS, ref.END_STUCK)
    m = re.search(r"typedef struct bg_progress_rewards \{(.*?)\} bg_progress_rewards;", hdr, re.S)
    assert m, "include/balatro_mi355x.h does not declare bg_progress_rewards"
    fields = [re.sub(r"\s+", " ", f.strip()) for f in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";") if f.strip()]
    assert fields == ["int32_t* counters_dev"], fields
    assert [f[0] for f in nat.ProgressRewards._fields_] == ["counters_dev"] and C.sizeof(nat.ProgressRewards) == 8
    m = re.search(r"\bint\s+bg_step_many_rows_progress\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/balatro_mi355x.h does not declare bg_step_many_rows_progress"
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == ["bg_handle* h", "int K", "const int32_t* actions_dev", "uint8_t* rows_dev", "uint64_t row_stride_bytes", "int rows_stride_steps",
                      "const bg_safe_limits* limits", "const bg_progress_rewards* progress", "bg_rollout_stats* stats_dev", "void* stream"], params
    # bg_step_many_rows_ex keeps its signature
    m = re.search(r"\bint\s+bg_step_many_rows_ex\s*\(([^;]*)\)\s*;", hdr)
    assert [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")][6:] == ["const bg_safe_limits* limits", "bg_rollout_stats* stats_dev", "void* stream"]
    assert re.search(r"\bint\s+bg_progress_terminal_slots\s*\(\s*int K,\s*int max_invalid_actions,\s*int max_episode_steps\s*\)\s*;", hdr)
    # the header's entry states the rule in the reference's order, with its lines
    doc = hdr[:hdr.index("#define BG_END_STUCK")].rsplit("/*", 1)[1]
    cites = ("train_progressive.py:123-131", "train_progressive.py:21-120", "(:45)", "(:60-63)", "(:66-72)", "(:75-78)", "(:81-86)", "(:91-93)", "(:96-99)", "(:103-108)",
             "(:111-114)", "(:117-118)", "(:33-41)", "ProgressionRewardWrapper", "SafeBalatroEnv", "BG_END_STUCK", "bg_progress_terminal_slots", "-1.2")
    for cite in cites:
        assert cite in doc, cite
    order = [doc.index(c) for c in cites[2:12]]
    assert order == sorted(order), "the rule is not stated in the reference's order"
    # the rule's own header: its citations, the host switch, the constants
    ph = open(os.path.join(CSRC, "bg_progress.h")).read()
    for cite in ("train_progressive.py:21-120", "train_progressive.py:123-131", "// :45", "// :60-61", "// :66", "// :68-69", "// :72", "// :75", "// :78", "// :81", "// :84-85", "// :91",
                 "// :92-93", "// :96", "// :97", "// :98", "// :103-104", "// :105-106", "// :107-108", "// :111-113", "// :117-118", ":33-41"):
        assert cite in ph, cite
    assert "BG_PROGRESS_HOST" in ph and re.search(r"#define BG_PROGRESS_END_STUCK 8u\b", ph)
    assert int(re.search(r"#define BG_PROGRESS_STUCK_STEPS (\d+)", ph).group(1)) == nat.PROGRESS_STUCK_STEPS == ref.STUCK_STEPS == 300
    for const in ("200 *", "20.0", "100.0", "> 150", "-0.5 *", "50.0", "0.2", "0.3", "0.4", "> 200", "> 400", "> 600", "< 300"):
        assert const in ph, const
    assert "bg_step_many_rows_progress" in nat.EXPORTS and "bg_progress_terminal_slots" in nat.EXPORTS
    assert os.path.join(CSRC, "bg_progress.h") in build.DEPS
    eng = open(os.path.join(CSRC, "bg_engine3.h")).read()
    assert "bool PROG" in eng and "bg_progress_step(" in eng and "bg_safe_step(" in eng
    lib = open(os.path.join(CSRC, "bg_lib.hip")).read()
    assert '#include "bg_progress.h"' in lib and "BG_PROGRESS_END_STUCK == BG_END_STUCK" in lib
    if os.path.exists(build.LIB):   # (as above: the GPU tests load the library, and loading checks every name of EXPORTS)
        L = C.CDLL(build.LIB)
        assert hasattr(L, "bg_step_many_rows_progress") and hasattr(L, "bg_progress_terminal_slots")
    import balatro_gym_amd
    assert "ProgressionRewards" in balatro_gym_amd.__all__ and balatro_gym_amd.ProgressionRewards is not None


def test_wrappers_refuse_bad_arguments_before_the_library():
    """ProgressionRewards / EpisodeLimits(progression=) on CPU tensors: sizes, masks, state dicts; existing constructions give what they gave."""
    import torch
    from balatro_gym_amd import EpisodeLimits, ProgressionRewards
    N = 5
    prog = ProgressionRewards(N, "cpu")
    assert prog.counters.dtype == torch.int32 and tuple(prog.counters.shape) == (N, 4) and not prog.counters.any()
    assert prog._struct().counters_dev == prog.counters.data_ptr()
    with pytest.raises(ValueError, match="n must be"):
        ProgressionRewards(-1, "cpu")
    prog.counters[:] = torch.tensor([250, 100, 0x00020001, 2], dtype=torch.int32)
    sd = prog.state_dict()
    prog.reset(torch.tensor([True, False, False, True, False]))
    assert prog.counters[:, 0].tolist() == [0, 250, 250, 0, 250] and prog.counters[:, 2].tolist() == [0, 0x20001, 0x20001, 0, 0x20001]
    with pytest.raises(ValueError, match="mask must have shape"):
        prog.reset(torch.zeros(N + 1, dtype=torch.bool))
    prog.reset()
    assert not prog.counters.any()
    prog.load_state_dict(sd)
    assert prog.counters[:, 1].tolist() == [100] * N and ref.ProgressCarry.unpack(prog.counters[0].tolist()).values() == (250, 100, 2, 3, 3)
    with pytest.raises(ValueError, match="counters must have shape"):
        ProgressionRewards(N + 1, "cpu").load_state_dict(sd)
    # EpisodeLimits: the keyword, and nothing else, changes the slot count
    assert EpisodeLimits(N, "cpu", steps=620).slots == 620 // 50 + 1 == EpisodeLimits(N, "cpu", steps=620, progression=True).slots
    a, b = EpisodeLimits(N, "cpu", 1000, 1000, steps=620), EpisodeLimits(N, "cpu", 1000, 1000, steps=620, progression=True)
    assert (a.slots, b.slots) == (1, 3) and tuple(b.terminal_rows.shape) == (3, N, 384) and tuple(b.terminal_step.shape) == (3, N)
    assert a.progression is False and b.progression is True
    with pytest.raises(ValueError, match="progression must be a bool"):
        EpisodeLimits(N, "cpu", progression=1)
