"""bg_expert_actions on the CPU (no GPU): csrc/bg_expert.h -- the per-record rule, the very text the kernel runs -- is compiled with g++
(-DBG_EXPERT_HOST) into a small program that walks records from a file, and held action for action and detail for detail to the restatement of
tests/expert_ref.py: on the synthetic set (every phase, holes in the hand, face-down cards, the nine forced hand types, the level clamp, value ties
of equal and of different size, the play / discard threshold at, below and above equality, a zero mask, a masked intention, stale selections) and on
the records of a closed-loop run of the C oracle driven by the restatement.  That run also asserts what the rule promises (every action valid, no
invalid-action penalty, at most 13 card toggles in a row) and that the expert beats more blinds than a uniform policy over the valid actions.  Also: the
header's declaration, the exports, build.DEPS, the twins' text against bg_device.h, and the argument checks of the Python wrappers.

Measured here (32 seeds, max_ante 3, 600 steps; profiles/expert_rows.txt has the end-ante histograms): the expert beats 1194 blinds, the uniform policy 71."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import expert_ref as ref
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")
SEEDS, MAX_ANTE, STEPS = 32, 3, 600
BO_ERR_INVALID_ACTION = 1   # oracle/balatro_oracle.h: the error of the invalid-action penalty (its reward, -1.0, is also that of a play a boss blind refuses)

_PROGRAM = r"""
#define BG_EXPERT_HOST
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "balatro_mi355x.h"
#include "bg_expert.h"
int main(int argc, char** argv) {
  if (argc != 7) return 2;   // n stride m has_index in out;  in = n records | int32 index [m] (has_index)
  const size_t n = strtoull(argv[1], 0, 10), stride = strtoull(argv[2], 0, 10), m = strtoull(argv[3], 0, 10);
  const int has_index = atoi(argv[4]);
  uint8_t* rows = (uint8_t*)aligned_alloc(16, n * stride + 16);
  int32_t* index = (int32_t*)malloc(m * 4 + 4);
  FILE* f = fopen(argv[5], "rb");
  if (!f || fread(rows, 1, n * stride, f) != n * stride) return 4;
  if (has_index && fread(index, 4, m, f) != m) return 4;
  fclose(f);
  int32_t* act = (int32_t*)malloc(m * 4 + 4);
  int32_t* det = (int32_t*)malloc(m * 4 + 4);
  bg_expert_actions_host(rows, stride, (int64_t)m, has_index ? index : 0, (int64_t)n, act, det);
  FILE* out = fopen(argv[6], "wb");
  if (!out || fwrite(act, 4, m, out) != m || fwrite(det, 4, m, out) != m) return 5;
  fclose(out);
  return 0;
}
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile csrc/bg_expert.h for the host"
    d = tmp_path_factory.mktemp("expert_host")
    src = d / "expert_host.cpp"
    src.write_text(_PROGRAM)
    exe = d / "expert_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])

    def run(rows, index=None):
        rows = np.ascontiguousarray(rows, np.uint8)
        n, stride = rows.shape
        m = n if index is None else len(index)
        blob = rows.tobytes() + (b"" if index is None else np.ascontiguousarray(index, np.int32).tobytes())
        (d / "in.bin").write_bytes(blob)
        subprocess.check_call([str(exe), str(n), str(stride), str(m), str(int(index is not None)), str(d / "in.bin"), str(d / "out.bin")])
        b = np.fromfile(str(d / "out.bin"), np.int32)
        return b[:m], b[m:]
    return run


def _assert_same(names, got, want, what):
    for g, w, field in zip(got, want, ("action", "detail")):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{what}: {field} differs on {len(bad)} records, first {names[bad[0]]}: got {g[bad[0]]:#x} want {w[bad[0]]:#x}"


@pytest.mark.parametrize("stride", [352, 384])
def test_synthetic_set_matches_the_restatement(host, stride):
    names, rows, want = ref.synthetic_rows(stride)
    _assert_same(names, host(rows), want, f"stride {stride}")
    # the restatement on the records (unpacked) is the restatement on the observations they were packed from
    _assert_same(names, ref.expert_rows(rows), want, "unpacked records")


def test_synthetic_set_covers_what_it_is_meant_to():
    """Each listed case does what its name says under the restatement, so that a kernel with a wrong tie-break, clamp or deselect order differs."""
    names, obs = ref.synthetic_obs()
    a, d = ref.expert_obs(obs)
    by = {n: (int(a[i]), int(d[i]), {k: obs[k][i] for k in obs}) for i, n in enumerate(names)}
    assert [by[f"phase2_{j}"][0] for j in range(5)] == [45, 46, 47, 31, -1]
    assert by["phase2_3"][1] == ref.FELLBACK and by["phase2_0"][1] == 0
    assert by["shop_cheapest_joker"][0] == 29 and by["shop_cheapest_masked_tie_to_lower_slot"][0] == 22 and by["shop_every_joker_masked"][0] == 31
    assert by["shop_no_joker"][0] == 31 and by["shop_no_joker_31_masked"][0] == 20 and by["shop_negative_cost"][0] == 24
    assert by["pack_55"] [:2] == (55, 0) and by["pack_55_masked"][:2] == (12, ref.FELLBACK)
    assert all(by[f"phase_other_{p}"][:2] == (0, ref.FELLBACK) for p in (4, 5, -1, 100, -128, 127))
    assert by["live_0"][:2] == (0, ref.FELLBACK) and by["all_zero_mask"][0] == -1 and by["all_zero_mask"][1] & ref.FELLBACK
    for ht in range(9):
        assert (by[f"forced_ht{ht}_0"][1] >> 8) & 15 == ht, ht
    types = {(d[i] >> 8) & 15 for i in range(len(names)) if obs["phase"][i] == 0}
    assert types == set(range(9))
    # the clamp: levels 0 and 1 value alike, 15 and 16 alike, 1 and 15 do not
    v = {L: by[f"level_{L}"][1] >> 16 for L in (0, 1, 15, 16, -3, 127)}
    assert v[0] == v[1] == v[-3] and v[15] == v[16] == v[127] and v[1] < v[15]
    # ties: the best value is reached twice, and the rule's order picks among them
    for j in range(3):
        for kind in ("equal", "different"):
            rec = by[f"tie_{kind}_size_{j}"][2]
            ss = ref.subsets(rec)
            top = max(s[0] for s in ss)
            tied = [s for s in ss if s[0] == top]
            assert len(tied) >= 2 and (len({s[1] for s in tied}) == 1) == (kind == "equal")
    # the threshold: play at and below equality, discard one above
    modes = [bool(by[f"remaining_{s}"][1] & ref.DISCARD_MODE) for s in ("-1", "+0", "+1")]
    assert modes == [False, False, True]
    assert not by["needed_below_scored"][1] & ref.DISCARD_MODE and by["needed_int32_extremes"][1] & ref.DISCARD_MODE
    assert by["discard_mode"][1] & ref.DISCARD_MODE and not by["no_discards"][1] & ref.DISCARD_MODE and not by["last_hand"][1] & ref.DISCARD_MODE
    assert not by["every_live_card_in_P"][1] & ref.DISCARD_MODE
    assert bin(by["discard_mode"][1] & 255).count("1") == 3 and bin(by["discard_fewer_than_five_left"][1] & 255).count("1") == 2
    five = by["discard_five_of_six"][1]
    assert five & ref.DISCARD_MODE and five & 255 == 0b01101110, "the five cheapest of six by (chips, slot): the 2s of slots 1-3, then the 3s of slots 5-6"
    assert by["intended_toggle_masked"][1] & ref.FELLBACK and by["play_masked_when_selected"][1] & ref.FELLBACK
    assert by["play_when_selected"][:1] == (0,) and by["discard_mode_stale"][0] >= 2
    # a stale selection is deselected before anything is selected
    a_stale, d_stale, rec = by["stale_selection_outside_T"]
    T = d_stale & 255
    assert a_stale >= 2 and not (T >> (a_stale - 2)) & 1 and rec["selected_cards"][a_stale - 2] != 0
    a_e, d_e, rec = by["selection_on_an_empty_slot"]
    assert a_e == 2 + 1 and not (d_e & 255) >> 1 & 1


# ---------------------------------------------------------------------------------------------------------------- the closed loop
def _run_closed_loop(policy):
    """32 oracle envs, STEPS steps of `policy(obs) -> actions`.  -> dict of what the run saw."""
    from oracle import pyoracle
    from tests.ppo_iter_ref import OracleVec, make_oracles

    class Vec(OracleVec):
        """OracleVec's step, keeping each step's info flags and the ante an episode ended at."""
        def __init__(self, envs):
            super().__init__(envs)
            self.flags, self.errors, self.end_antes = [], [], []

        def step(self, actions):
            rew, done, fl, er = np.zeros(len(self.envs), np.float64), np.zeros(len(self.envs), bool), np.zeros(len(self.envs), np.int64), np.zeros(len(self.envs), np.int64)
            for i, e in enumerate(self.envs):
                ante = int(self._obs[-1]["ante"][i])
                _, rew[i], done[i], _, info = e.step(int(actions[i]))
                fl[i], er[i] = info.flags, info.error
                if done[i]:
                    self.end_antes.append(ante)
                    e.reset()
            self._obs.append(self.observe()); self._rew.append(rew); self._done.append(done); self.flags.append(fl); self.errors.append(er)
            return self._obs[-1], rew, done

    vec = Vec(make_oracles(range(7000, 7000 + SEEDS), scorer_jokers=True, max_ante=MAX_ANTE))
    obs = vec._obs[0]
    taken, masks = [], []
    for _ in range(STEPS):
        a = policy(obs)
        taken.append(a); masks.append(obs["action_mask"].copy())
        obs, _, _ = vec.step(a)
    tr = vec.transitions()
    flags = np.array(vec.flags)
    return {"tr": tr, "actions": np.array(taken), "masks": np.array(masks), "flags": flags, "errors": np.array(vec.errors), "beaten": int((flags & pyoracle_beat()).astype(bool).sum()),
            "end_antes": np.bincount(np.array(vec.end_antes, np.int64), minlength=MAX_ANTE + 2), "episodes": len(vec.end_antes)}


def pyoracle_beat():
    return 1   # BO_INFO_BEAT_BLIND


@pytest.fixture(scope="module")
def closed_loop():
    return _run_closed_loop(lambda obs: ref.expert_obs(obs)[0])


def test_closed_loop_actions_are_valid_and_toggles_bounded(closed_loop):
    run = closed_loop
    a, masks, errors = run["actions"], run["masks"], run["errors"]
    K, N = a.shape
    assert (a >= 0).all() and (a < 60).all()
    assert (np.take_along_axis(masks, a[:, :, None].astype(np.int64), axis=2)[:, :, 0] != 0).all(), "an action outside the observation's mask"
    assert (errors != BO_ERR_INVALID_ACTION).all(), "a step was answered with the invalid-action penalty"
    print(f"closed loop: steps the env refused for another reason (a full joker row, a boss blind's rule), by error code: {np.bincount(errors.reshape(-1))[1:].tolist()}")
    toggle = (a >= 2) & (a <= 9)
    longest = 0
    for i in range(N):
        runlen = 0
        for t in range(K):
            runlen = runlen + 1 if toggle[t, i] else 0
            longest = max(longest, runlen)
    print(f"closed loop: {K} x {N} steps, {run['episodes']} episodes, longest toggle run {longest}, blinds beaten {run['beaten']}, end antes {run['end_antes'].tolist()}")
    assert 1 <= longest <= 13
    # the run reaches what the parity test below relies on: every phase the rule knows, both modes
    phases = set(np.unique(run["tr"]["obs"]["phase"]).tolist())
    assert {0, 1, 2} <= phases and (a == 0).any() and (a == 1).any() and ((a >= 20) & (a < 30)).any()


def test_closed_loop_records_match_the_restatement(host, closed_loop):
    from tests import ppo_iter_ref
    tr, a = closed_loop["tr"], closed_loop["actions"]
    K, N = a.shape
    rows = ppo_iter_ref.records(tr, a, stride=384)[:K].reshape(K * N, 384)
    want = ref.expert_rows(rows)
    assert np.array_equal(want[0].reshape(K, N), a), "the records give the restatement the actions it took on the observations"
    _assert_same([f"t{i // N}_env{i % N}" for i in range(K * N)], host(rows), want, "closed loop")
    # through an index: out-of-range, negative and repeated entries
    index = np.concatenate([np.arange(K * N - 1, -1, -7), [-1, K * N, 2 ** 31 - 1, -2 ** 31, 5, 5, 5]]).astype(np.int32)
    _assert_same([str(i) for i in index], host(rows, index), ref.expert_rows(rows, index), "closed loop, indexed")
    assert host(rows, index)[0][-7:-3].tolist() == [-1] * 4 and host(rows, index)[1][-7:-3].tolist() == [0] * 4


def test_expert_beats_more_blinds_than_a_uniform_policy(closed_loop):
    rng = np.random.default_rng(3)

    def uniform(obs):
        m = obs["action_mask"] != 0
        return np.array([rng.choice(np.flatnonzero(r)) for r in m], np.int64)

    uni = _run_closed_loop(uniform)
    print(f"blinds beaten: expert {closed_loop['beaten']} (end antes {closed_loop['end_antes'].tolist()}), uniform {uni['beaten']} (end antes {uni['end_antes'].tolist()})")
    assert closed_loop["beaten"] > uni["beaten"]


# ---------------------------------------------------------------------------------------------------------------- the interface
def _params(hdr, name):
    m = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"include/balatro_mi355x.h does not declare {name}"
    return [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", p).strip()) for p in m.group(1).split(",")]


def test_header_declares_and_library_exports_the_expert():
    from balatro_gym_amd import _native as nat, build
    import balatro_gym_amd
    hdr = open(HEADER).read()
    base = ["const void* rows_dev", "int64_t row_stride_bytes", "int64_t m", "const int32_t* index_dev", "int64_t store_rows", "int32_t* actions_dev",
            "int32_t* detail_dev"]
    assert _params(hdr, "bg_expert_actions") == base + ["void* stream"]
    assert _params(hdr, "bg_expert_actions_ex") == base + ["int lanes_per_record", "float* kernel_ms_out", "void* stream"]
    doc = hdr[:hdr.index("int bg_expert_actions(")].rsplit("\n/*", 1)[1]
    for cite in ("expert_agent.py", "scoring_engine.py:103-122", "45, 46, 47, 31, 55, 0, 1..59", "FELLBACK", "at most 13 card toggles", "bits 16-31", "Out of scope"):
        assert cite in doc, cite
    assert "bg_expert_actions" in nat.EXPORTS and "bg_expert_actions_ex" in nat.EXPORTS
    assert os.path.join(CSRC, "bg_expert.h") in build.DEPS
    assert "expert_actions" in balatro_gym_amd.__all__
    # the three notes that deferred the expert now point at it
    for path, old in ((HEADER, "the expert policy itself"), (os.path.join(CSRC, "bg_bc.h"), "the expert policy itself"), (os.path.join(ROOT, "INTEGRATION.md"), "the expert policy itself")):
        assert old not in open(path).read(), path
    assert "bg_expert_actions" in open(os.path.join(CSRC, "bg_bc.h")).read() and "bg_expert_actions" in open(os.path.join(CSRC, "bg_demo.h")).read()
    assert "expert_act" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    if os.path.exists(build.LIB):
        L = C.CDLL(build.LIB)
        assert hasattr(L, "bg_expert_actions") and hasattr(L, "bg_expert_actions_ex")


def test_twins_have_the_text_of_the_engines_game_functions():
    """bg_expert.h restates bg_card_chips, bg_hand_base and bg_classify where g++ can compile them: the same text, but for the intrinsics' names."""
    dev, exp = open(os.path.join(CSRC, "bg_device.h")).read(), open(os.path.join(CSRC, "bg_expert.h")).read()

    def norm(s):
        s = re.sub(r"//[^\n]*", "", s)
        s = s.replace("__popcll", "__builtin_popcountll").replace("__popc(", "__builtin_popcount(").replace("#pragma unroll", "")
        return re.sub(r"\s+", " ", s).strip()

    def body(text, sig):
        i = text.index(sig)
        return text[text.index("{", i) + 1:text.index("\n}", i)]
    assert norm(body(dev, "int bg_card_chips(int code)")) == norm(body(exp, "int bg_expert_card_chips(int code)"))
    assert norm(body(dev, "void bg_hand_base(int ht, int level, int& chips, int& mult)")) == norm(body(exp, "void bg_expert_hand_base(int ht, int level, int& chips, int& mult)"))
    whole = norm(body(dev, "int bg_classify(uint64_t cards, int n)"))
    head = norm(body(exp, "int bg_expert_classify(uint64_t cards, int n)"))
    tail = norm(body(exp, "int bg_expert_classify_hist(uint64_t hist, uint32_t suits, int n)"))
    call = "return bg_expert_classify_hist(hist, suits, n);"
    assert head.endswith(call) and norm(head[:-len(call)] + " " + tail) == whole


def test_wrappers_refuse_bad_arguments_before_the_library():
    """expert_actions / RowBuffers.expert / BalatroVecEnv.expert_act on CPU tensors: every bad argument is a ValueError raised before anything is loaded."""
    import torch
    from balatro_gym_amd import expert_actions
    from balatro_gym_amd.vec_env import RowBuffers
    N = 6
    rec = torch.zeros((N, 384), dtype=torch.uint8)
    for bad in (torch.zeros((N, 360), dtype=torch.uint8), torch.zeros((N, 336), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="record stride"):
            expert_actions(bad)
    for bad in (torch.zeros((N, 768), dtype=torch.uint8)[:, ::2], torch.zeros((N, 384), dtype=torch.int8), torch.zeros(384, dtype=torch.uint8), torch.zeros((2, 2, N, 384), dtype=torch.uint8), "rows", None):
        with pytest.raises(ValueError, match="packed records"):
            expert_actions(bad)
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros((3, 1), dtype=torch.int32), torch.zeros(6, dtype=torch.int32)[::2], [0, 1]):
        with pytest.raises(ValueError, match="index must be a contiguous torch.int32"):
            expert_actions(rec, index=bad)
    for name in ("out", "detail"):
        for bad in (torch.zeros(N, dtype=torch.int64), torch.zeros(N + 1, dtype=torch.int32), torch.zeros(2 * N, dtype=torch.int32)[::2], torch.zeros((N, 1), dtype=torch.int32)):
            with pytest.raises(ValueError, match=f"{name} must be a contiguous int32"):
                expert_actions(rec, **{name: bad})
    with pytest.raises(ValueError, match="out must be a contiguous int32"):
        expert_actions(rec, index=torch.zeros(3, dtype=torch.int32), out=torch.zeros(N, dtype=torch.int32))
    with pytest.raises(ValueError, match="detail must be"):
        expert_actions(rec, detail=1)
    # everything right: what is left is that there is no CPU path
    for kw in ({}, {"index": torch.zeros(3, dtype=torch.int32)}, {"out": torch.zeros(N, dtype=torch.int32), "detail": True}):
        with pytest.raises(ValueError, match="device tensor"):
            expert_actions(rec, **kw)
    with pytest.raises(ValueError, match="device tensor"):
        expert_actions(torch.zeros((3, N, 352), dtype=torch.uint8), detail=torch.zeros((3, N), dtype=torch.int32))
    rb = RowBuffers(N, torch.device("cpu"), steps=3, row_stride=384)
    with pytest.raises(ValueError, match="device tensor"):
        rb.expert()
    with pytest.raises(ValueError, match="device tensor"):
        rb.expert(1, detail=True)
