"""bg_episode_outcome_rows on the CPU (no GPU).  csrc/bg_outcome.h -- the per-step arithmetic the kernel runs and the serial twin of its launch -- is
compiled with g++ (-O1 -ffp-contract=off -DBG_OUTCOME_HOST) into a small shared object and held BIT FOR BIT to the numpy loop of tests/outcome_ref.py:
synthetic records of random bytes at strides 352 and 384, K in {1, 15, 16, 17, 33}, N in {1, 63, 64, 65, 130}, with and without tails and dense rewards,
gamma 1.0 and 0.99, an env that never ends, one that ends on every step, an ending at t = 0 and one at t = K - 1; chunked calls chained through the
tail equal one call over the whole store.  Also: the header's declaration, the exports, build.DEPS and the refusals of the Python wrapper."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import outcome_ref as ref
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")
KS, NS, STRIDES = (1, 15, 16, 17, 33), (1, 63, 64, 65, 130), (352, 384)

_PROGRAM = r"""
#define BG_OUTCOME_HOST
#include <stddef.h>
#include "balatro_mi355x.h"
#include "bg_outcome.h"
extern "C" void outcome_host(const uint8_t* rows, uint64_t stride, int K, int64_t N, double gamma, const double* rewards, const int32_t* ts, const int32_t* ta,
                             const uint8_t* tf, const double* tr, int32_t* steps, int32_t* ante, uint8_t* flags, double* returns) {
  bg_outcome_host(rows, stride, K, (long long)N, gamma, rewards, ts, ta, tf, tr, steps, ante, flags, returns);
}
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile csrc/bg_outcome.h for the host"
    d = tmp_path_factory.mktemp("outcome_host")
    src = d / "outcome_host.cpp"
    src.write_text(_PROGRAM)
    so = d / "outcome_host.so"
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-I", os.path.dirname(HEADER), "-o", str(so), str(src)])
    lib = C.CDLL(str(so))
    vp = C.c_void_p
    lib.outcome_host.argtypes = [vp, C.c_uint64, C.c_int, C.c_int64, C.c_double] + [vp] * 9
    lib.outcome_host.restype = None

    def run(rows, gamma=1.0, rewards=None, tail=None, want=ref.FIELDS):
        K, N, stride = rows.shape
        rows = np.ascontiguousarray(rows)
        tail = {f: np.ascontiguousarray(v, ref.DTYPES[f]) for f, v in (tail or {}).items()}
        outs = {f: np.full((K, N), 99, ref.DTYPES[f]) for f in want}
        rw = None if rewards is None else np.ascontiguousarray(rewards, np.float64)
        p = lambda x: None if x is None else x.ctypes.data   # noqa: E731
        lib.outcome_host(p(rows), stride, K, N, gamma, p(rw), *(p(tail.get(f)) for f in ref.FIELDS), *(p(outs.get(f)) for f in ref.FIELDS))
        return outs
    return run


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("K", KS)
def test_twin_is_the_numpy_loop(host, K, stride):
    for N in NS:
        kinds = (None,) if N >= 4 else ref.KINDS
        for kind0 in kinds:
            rows = ref.synthetic_rows(K * 1000 + N + stride, K, N, stride, kind0)
            _, done, _, _ = ref.fields_of(rows)
            if N >= 4:
                assert not done[:, 0].any() and done[:, 1].all() and done[0, 2] and done[K - 1, 3]
            rewards = np.random.default_rng(K + N).standard_normal((K, N)) * 3.0
            for gamma in (1.0, 0.99):
                for tail in (None, ref.synthetic_tail(K + N, N)):
                    for rw in (None, rewards):
                        what = f"K {K} N {N} stride {stride} kind0 {kind0} gamma {gamma} tail {tail is not None} rewards {rw is not None}"
                        want = ref.outcome_loop(rows, gamma, rw, tail)
                        ref.assert_equal_bits(host(rows, gamma, rw, tail), want, what)
            # the properties the loop itself must have: an env that never ends is open throughout without a tail; an ending step is 0
            want = ref.outcome_loop(rows, 1.0)
            if N >= 4:
                assert (want["steps_to_end"][:, 0] == -1).all() and (want["end_ante"][:, 0] == -1).all() and (want["end_flags"][:, 0] == 0).all()
                assert (want["steps_to_end"][:, 1] == 0).all()
                assert np.array_equal(want["returns"][:, 0], np.cumsum(ref.fields_of(rows)[0][::-1, 0])[::-1])
            assert (want["steps_to_end"][done] == 0).all()
            # a subset of the outputs: the others are not touched (NULL), the ones asked for are the same
            sub = host(rows, 0.99, None, None, want=("end_ante",))
            ref.assert_equal_bits(sub, ref.outcome_loop(rows, 0.99), "end_ante alone", fields=("end_ante",))


@pytest.mark.parametrize("cuts", [(5,), (1, 16, 17), (32,)])
def test_chunks_chained_through_the_tail_equal_one_call(host, cuts):
    K, N = 33, 65
    rows = ref.synthetic_rows(91, K, N, 384, p_end=0.08)
    whole = host(rows, 0.99)
    ref.assert_equal_bits(whole, ref.outcome_loop(rows, 0.99), "whole")
    bounds = [0, *cuts, K]
    tail, parts = None, []
    for a, b in reversed(list(zip(bounds[:-1], bounds[1:]))):
        got = host(rows[a:b], 0.99, None, tail)
        tail = {f: got[f][0].copy() for f in ref.FIELDS}   # EpisodeOutcomes.tail(): row 0 of every field
        parts.insert(0, got)
    ref.assert_equal_bits({f: np.concatenate([p[f] for p in parts]) for f in ref.FIELDS}, whole, f"chunks at {cuts}")


def test_header_declares_and_library_exports_episode_outcome_rows():
    from balatro_gym_amd import _native as nat, build
    import balatro_gym_amd
    hdr = open(HEADER).read()
    m = re.search(r"\bint\s+bg_episode_outcome_rows\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/balatro_mi355x.h does not declare bg_episode_outcome_rows"
    params = [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", p).strip()) for p in m.group(1).split(",")]
    assert params == ["const uint8_t* rows_dev", "uint64_t row_stride_bytes", "int K", "int64_t N", "double gamma", "const double* rewards_dev",
                      "const int32_t* tail_steps_dev", "const int32_t* tail_ante_dev", "const uint8_t* tail_flags_dev", "const double* tail_return_dev",
                      "int32_t* steps_to_end_dev", "int32_t* end_ante_dev", "uint8_t* end_flags_dev", "double* returns_dev", "float* kernel_ms_out",
                      "void* stream"], params
    doc = hdr[:hdr.index("int bg_episode_outcome_rows")].rsplit("\n/*", 1)[1]
    for cite in ("train_balatro_agent.py:220-262", "BG_ROW_END_ANTE", "next.steps < 0 ? -1", "r + gamma * next.ret", "OPEN", "a tail without its output is refused",
                 "bg_episode_outcome_rows: "):
        assert cite in doc, cite
    assert (nat.ROW_EXTRA["terminated"][0], nat.ROW_EXTRA["end_flags"][0], nat.ROW_EXTRA["end_ante"][0]) == (342, 343, 344)
    assert "bg_episode_outcome_rows" in nat.EXPORTS
    assert os.path.join(CSRC, "bg_outcome.h") in build.DEPS
    assert "episode_outcomes" in balatro_gym_amd.__all__ and "EpisodeOutcomes" in balatro_gym_amd.__all__
    from balatro_gym_amd.vec_env import RowBuffers
    assert callable(RowBuffers.outcomes)
    if os.path.exists(build.LIB):
        assert hasattr(C.CDLL(build.LIB), "bg_episode_outcome_rows")


def test_wrapper_refuses_bad_arguments_before_the_library():
    """episode_outcomes on CPU tensors: every bad argument is a ValueError raised before anything is loaded."""
    import torch
    from balatro_gym_amd import EpisodeOutcomes, episode_outcomes
    K, N = 3, 5
    rows = torch.zeros((K, N, 384), dtype=torch.uint8)
    for bad in (rows[0], rows.to(torch.int8), torch.zeros((K, N, 360), dtype=torch.uint8), torch.zeros((K, N, 768), dtype=torch.uint8)[:, :, :384], None):
        with pytest.raises(ValueError, match="rows must be a contiguous uint8|record stride"):
            episode_outcomes(bad)
    for bad in ((), ("steps",), ("returns", "returns"), ("end_ante", "x")):
        with pytest.raises(ValueError, match="want must name"):
            episode_outcomes(rows, want=bad)
    for bad in (torch.zeros((K, N)), torch.zeros((K, N + 1), dtype=torch.float64), torch.zeros((N, K), dtype=torch.float64).t()):
        with pytest.raises(ValueError, match="rewards must be a contiguous"):
            episode_outcomes(rows, rewards=bad)
    with pytest.raises(ValueError, match="rewards are read only for 'returns'"):
        episode_outcomes(rows, rewards=torch.zeros((K, N), dtype=torch.float64), want=("end_ante",))
    with pytest.raises(ValueError, match="tail must be a dict"):
        episode_outcomes(rows, tail=[1])
    with pytest.raises(ValueError, match="tail must be a dict"):
        episode_outcomes(rows, tail={"ante": torch.zeros(N, dtype=torch.int32)})
    with pytest.raises(ValueError, match="without its output"):
        episode_outcomes(rows, tail={"returns": torch.zeros(N, dtype=torch.float64)}, want=("end_ante",))
    for f, bad in (("steps_to_end", torch.zeros(N, dtype=torch.int64)), ("end_flags", torch.zeros(N, dtype=torch.int8)), ("returns", torch.zeros(N)),
                   ("end_ante", torch.zeros(N + 1, dtype=torch.int32))):
        with pytest.raises(ValueError, match=r"tail\['%s'\] must be a contiguous" % f):
            episode_outcomes(rows, tail={f: bad})
    with pytest.raises(ValueError, match="gamma must not be NaN"):
        episode_outcomes(rows, float("nan"))
    # everything right: what is left is that there is no CPU path
    tail = {"steps_to_end": torch.zeros(N, dtype=torch.int32), "returns": torch.zeros(N, dtype=torch.float64)}
    with pytest.raises(ValueError, match="device tensor"):
        episode_outcomes(rows, 0.99, rewards=torch.zeros((K, N), dtype=torch.float64), tail=tail)
    # the tail of a result: row 0 of the computed fields
    o = EpisodeOutcomes(end_ante=torch.arange(K * N, dtype=torch.int32).view(K, N), returns=torch.ones((K, N), dtype=torch.float64))
    t = o.tail()
    assert sorted(t) == ["end_ante", "returns"] and t["end_ante"].tolist() == list(range(N)) and t["returns"].is_contiguous()
