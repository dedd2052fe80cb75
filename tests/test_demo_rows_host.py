"""bg_demo_append_rows / bg_demo_sample on the CPU (no GPU).  csrc/bg_demo.h -- the per-row functions the kernels run (the keep test, the slot rule,
the record blend) and the serial twin of the three launches -- is compiled with g++ (-O1 -DBG_DEMO_HOST) into a small shared object and held BYTE
FOR BYTE to tests/demo_ref.py over the whole ring, demo_weight, demo_source and cursor: records of random bytes (so every byte's origin shows, the
bytes above 352 of store and ring included), strides 352 and 384 for store and ring independently, returns given and not, every special weight, kept
= 0 and kept = all, three chained calls that wrap the ring, kept > capacity, kept == capacity and capacity == 1.  Also: the header's declarations, the
exports, build.DEPS and the refusals of the Python wrapper."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import demo_ref as ref
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")

_PROGRAM = r"""
#define BG_DEMO_HOST
#include <stddef.h>
#include "balatro_mi355x.h"
#include "bg_demo.h"
extern "C" uint64_t demo_ws_bytes(int64_t store_rows) { return bg_demo_ws_bytes(store_rows); }
extern "C" void demo_append_host(const uint8_t* rows, uint64_t stride, int K, int64_t N, const float* weights, const double* returns, uint8_t* demo,
                                 uint64_t dstride, int64_t capacity, float* demo_weight, int32_t* demo_source, int64_t* cursor, void* workspace) {
  bg_demo_append_host(rows, stride, K, N, weights, returns, demo, dstride, capacity, demo_weight, demo_source, cursor, workspace);
}
extern "C" void demo_sample_host(const int64_t* cursor, int64_t capacity, uint64_t seed, uint64_t index0, uint64_t t, int32_t* index, int64_t m) {
  bg_demo_sample_host(cursor, capacity, seed, index0, t, index, m);
}
extern "C" int demo_keep(uint32_t bits) { return bg_demo_keep(bits) ? 1 : 0; }
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile csrc/bg_demo.h for the host"
    d = tmp_path_factory.mktemp("demo_host")
    src = d / "demo_host.cpp"
    src.write_text(_PROGRAM)
    so = d / "demo_host.so"
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-I", os.path.dirname(HEADER), "-o", str(so), str(src)])
    L = C.CDLL(str(so))
    vp = C.c_void_p
    L.demo_ws_bytes.restype = C.c_uint64
    L.demo_ws_bytes.argtypes = [C.c_int64]
    L.demo_append_host.restype = None
    L.demo_append_host.argtypes = [vp, C.c_uint64, C.c_int, C.c_int64, vp, vp, vp, C.c_uint64, C.c_int64, vp, vp, vp, vp]
    L.demo_sample_host.restype = None
    L.demo_sample_host.argtypes = [vp, C.c_int64, C.c_uint64, C.c_uint64, C.c_uint64, vp, C.c_int64]
    L.demo_keep.argtypes = [C.c_uint32]
    return L


def _append(L, store, weights, returns, ring, dw, ds, cursor):
    """The twin on copies of the ring's arrays -> the dict tests/demo_ref.append returns (without `written`)."""
    K1, N, stride = store.shape
    K = K1 - 1
    store, w = np.ascontiguousarray(store), np.ascontiguousarray(weights, np.float32)
    rt = None if returns is None else np.ascontiguousarray(returns, np.float64)
    ring, dw, cursor = ring.copy(), dw.copy(), cursor.copy()
    ds = None if ds is None else ds.copy()
    need = int(L.demo_ws_bytes(K * N))
    assert need == (0 if K * N == 0 else 16 + (4 * ((K * N + 1023) // 1024) + 15) // 16 * 16)
    ws = np.full(need + 16, 0xA5, np.uint8)
    p = lambda x: None if x is None else x.ctypes.data   # noqa: E731
    L.demo_append_host(p(store), stride, K, N, p(w), p(rt), p(ring), ring.shape[1], ring.shape[0], p(dw), p(ds), p(cursor), p(ws))
    assert (ws[need:] == 0xA5).all(), "the twin wrote past bg_demo_workspace_bytes"
    return {"ring": ring, "weight": dw, "source": ds, "cursor": cursor}


def _case(L, seed, K, N, C_, stride, dstride, share, with_returns, with_source=True, T0=0, special=True):
    store = ref.synthetic_store(seed, K, N, stride)
    w = ref.synthetic_weights(seed, K, N, share, special)
    returns = np.random.default_rng(seed + 3).standard_normal((K, N)) * 7.0 if with_returns else None
    ring, dw, ds, cursor = ref.fresh_ring(seed, C_, dstride)
    cursor[0] = T0
    want = ref.append(store, w, returns, ring, dw, ds if with_source else None, cursor)
    got = _append(L, store, w, returns, ring, dw, ds if with_source else None, cursor)
    ref.assert_same(got, want, f"seed {seed} K {K} N {N} C {C_} strides {stride}/{dstride} share {share} returns {with_returns} T0 {T0}")
    return store, w, ring, want


@pytest.mark.parametrize("with_returns", [False, True])
@pytest.mark.parametrize("dstride", [352, 384])
@pytest.mark.parametrize("stride", [352, 384])
def test_twin_is_the_reference_at_every_stride_pair(lib, stride, dstride, with_returns):
    for seed, (K, N) in enumerate([(5, 7), (13, 96), (2, 1100)]):
        store, w, ring, want = _case(lib, 10 + seed, K, N, 4096, stride, dstride, 0.5, with_returns)
        kept = int(want["cursor"][1])
        assert 0 < kept < K * N and want["written"] == list(range(kept))
        # bytes 352 and above: never copied from the store, never written in the ring; the slots behind the kept ones are untouched
        assert np.array_equal(want["ring"][:, ref.ROW:], ring[:, ref.ROW:]) and np.array_equal(want["ring"][kept:], ring[kept:])
        # every byte's origin in the first kept record
        i = int(np.flatnonzero(ref.keep(w))[0])
        flat = store.reshape(-1, stride)
        rec = want["ring"][0]
        assert np.array_equal(rec[:136], flat[i, :136]) and np.array_equal(rec[144:172], flat[i, 144:172]) and np.array_equal(rec[176:342], flat[i, 176:342])
        assert np.array_equal(rec[172:176], flat[i + N, 172:176]) and np.array_equal(rec[342:352], flat[i + N, 342:352])
        if not with_returns:
            assert np.array_equal(rec[136:144], flat[i + N, 136:144])


def test_without_a_source_array_and_from_a_negative_count(lib):
    """demo_source_dev NULL: ring, weights and cursor are the reference's.  cursor[0] < 0 is taken as an empty ring (slot 0 onwards, count = kept)."""
    for K, N, C_, share in ((5, 7, 64, 0.5), (13, 96, 100, 0.7), (2, 1100, 4096, 0.5)):
        _case(lib, 20 + K, K, N, C_, 384, 352, share, True, with_source=False)
        store, w, ring, want = _case(lib, 21 + K, K, N, C_, 352, 384, share, False, T0=-5)
        kept = int(want["cursor"][1])
        assert int(want["cursor"][0]) == kept and want["written"][0] == max(kept - C_, 0) % C_


def test_special_weights(lib):
    """+0.0, -0.0, negatives, NaN, the infinities are not kept; denormals, float32's smallest normal and its largest value are."""
    assert np.array_equal(ref.keep(ref.SPECIAL_WEIGHTS), ref.SPECIAL_KEPT)
    for bits, k in zip(ref.SPECIAL_WEIGHTS.view(np.uint32), ref.SPECIAL_KEPT):
        assert bool(lib.demo_keep(int(bits))) == bool(k), hex(int(bits))
    for bits in (0x7FC00000, 0xFFC00000, 0x7F800001, 0x80000001, 0x7F7FFFFF, 0x00000001):
        assert bool(lib.demo_keep(bits)) == bool(ref.keep(np.array([bits], np.uint32).view(np.float32))[0]), hex(bits)
    K, N = 3, ref.SPECIAL_WEIGHTS.size
    store = ref.synthetic_store(5, K, N, 384)
    w = np.stack([ref.SPECIAL_WEIGHTS, ref.SPECIAL_WEIGHTS[::-1], np.roll(ref.SPECIAL_WEIGHTS, 5)])
    ring, dw, ds, cursor = ref.fresh_ring(5, 64, 384)
    want = ref.append(store, w, None, ring, dw, ds, cursor)
    assert int(want["cursor"][1]) == 3 * int(ref.SPECIAL_KEPT.sum())
    ref.assert_same(_append(lib, store, w, None, ring, dw, ds, cursor), want, "special weights")


@pytest.mark.parametrize("share", [0.0, 1.0])
def test_nothing_kept_and_everything_kept(lib, share):
    K, N = 13, 96
    store, w, ring, want = _case(lib, 30, K, N, 2000, 384, 384, share, True, T0=17, special=share == 0.0)
    kept = int(want["cursor"][1])
    assert kept == (0 if share == 0.0 else K * N) and int(want["cursor"][0]) == 17 + kept
    if share == 0.0:
        assert np.array_equal(want["ring"], ring) and (want["weight"] == -7.0).all() and (want["source"] == -9).all()
    else:
        assert np.array_equal(want["source"][17:17 + kept], np.arange(kept))


def test_three_chained_calls_wrap_the_ring(lib):
    C_ = 700
    ring, dw, ds, cursor = ref.fresh_ring(40, C_, 384)
    g = {"ring": ring, "weight": dw, "source": ds, "cursor": cursor}
    wn = dict(g)
    total = 0
    for call, (K, N) in enumerate([(5, 97), (3, 130), (4, 101)]):
        store = ref.synthetic_store(41 + call, K, N, 352)
        w = ref.synthetic_weights(41 + call, K, N, 0.6)
        wn = ref.append(store, w, None, wn["ring"], wn["weight"], wn["source"], wn["cursor"])
        g = _append(lib, store, w, None, g["ring"], g["weight"], g["source"], g["cursor"])
        ref.assert_same(g, wn, f"call {call}")
        total += int(wn["cursor"][1])
        assert int(wn["cursor"][0]) == total
    assert total > C_, "the three calls must wrap the ring"


@pytest.mark.parametrize("C_,K,N,share", [(100, 5, 97, 0.7), (1, 5, 7, 0.5), (1, 2, 3, 1.0), (1248, 13, 96, 1.0), (37, 2, 1100, 1.0)])
def test_more_kept_rows_than_slots(lib, C_, K, N, share):
    """kept > capacity: exactly the last `capacity` ranks are present, no slot is written twice; kept == capacity fills the ring exactly."""
    for T0 in (0, 5, 3 * C_ + 2):
        store, w, ring, want = _case(lib, 50 + C_, K, N, C_, 384, 352, share, False, T0=T0, special=share < 1.0)
        kept_rows = np.flatnonzero(ref.keep(w))
        kept = kept_rows.size
        assert kept >= C_ and int(want["cursor"][1]) == kept
        assert sorted(want["written"]) == list(range(C_))
        survivors = kept_rows[kept - C_:]
        assert np.array_equal(np.sort(want["source"]), survivors)
        assert np.array_equal(want["source"][(T0 + np.arange(kept - C_, kept)) % C_], survivors)


def test_sample_twin_is_the_reference(lib):
    for total, cap in ((0, 9), (1, 9), (5, 9), (9, 9), (1000, 9), (2 ** 31 - 1, 2 ** 31 - 1), (-3, 9)):
        cursor = np.array([total, 0], np.int64)
        for seed, index0, t, m in ((0, 0, 0, 1), (1234567, 10, 3, 257), (2 ** 64 - 1, 2 ** 40, 2 ** 63, 64)):
            got = np.full(m + 2, 77, np.int32)
            lib.demo_sample_host(cursor.ctypes.data, cap, seed, index0, t, got[1:].ctypes.data, m)
            want = ref.sample(total, cap, seed, index0, t, m)
            assert np.array_equal(got[1:-1], want) and got[0] == 77 and got[-1] == 77, (total, cap, seed)
            filled = min(max(total, 0), cap)
            assert ((want >= 0) & (want < filled)).all() if filled else (want == -1).all()
    # the same (seed, index0 + i, t) gives the same draw whatever m
    a, b = ref.sample(500, 1000, 9, 0, 4, 300), ref.sample(500, 1000, 9, 100, 4, 50)
    assert np.array_equal(a[100:150], b) and len(set(a.tolist())) > 100


def test_header_declares_and_library_exports_both_calls():
    from balatro_gym_amd import _native as nat, build
    import balatro_gym_amd
    hdr = open(HEADER).read()

    def params(name, ret):
        m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), hdr)
        assert m, f"include/balatro_mi355x.h does not declare {name}"
        return [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", p).strip()) for p in m.group(1).split(",")]
    assert params("bg_demo_workspace_bytes", "uint64_t") == ["int64_t store_rows"]
    assert params("bg_demo_append_rows", "int") == [
        "const uint8_t* rows_dev", "uint64_t row_stride_bytes", "int K", "int64_t N", "const float* weights_dev", "const double* returns_dev",
        "uint8_t* demo_dev", "uint64_t demo_stride_bytes", "int64_t capacity", "float* demo_weight_dev", "int32_t* demo_source_dev", "int64_t* cursor_dev",
        "void* workspace_dev", "uint64_t workspace_bytes", "float* kernel_ms_out", "void* stream"]
    assert params("bg_demo_sample", "int") == ["const int64_t* cursor_dev", "int64_t capacity", "uint64_t seed", "uint64_t index0", "uint64_t t",
                                               "int32_t* index_dev", "int64_t m", "float* kernel_ms_out", "void* stream"]
    doc = hdr[:hdr.index("uint64_t bg_demo_workspace_bytes")].rsplit("\n/*", 1)[1]
    for cite in ("train_balatro_agent.py:220-262", "(T0 + r) mod capacity", "kept - capacity", "bytes 340..341", "filled / 2**32", "bg_demo_append_rows: ",
                 "Out of scope"):
        assert cite in doc, cite
    for name in ("bg_demo_append_rows", "bg_demo_sample", "bg_demo_workspace_bytes"):
        assert name in nat.EXPORTS
    assert os.path.join(CSRC, "bg_demo.h") in build.DEPS
    assert "DemoBuffer" in balatro_gym_amd.__all__
    from balatro_gym_amd.vec_env import RowBuffers
    assert callable(RowBuffers.to_demo)
    if os.path.exists(build.LIB):   # (the GPU tests load the library, and loading checks every name of EXPORTS)
        L = C.CDLL(build.LIB)
        assert hasattr(L, "bg_demo_append_rows") and hasattr(L, "bg_demo_sample") and hasattr(L, "bg_demo_workspace_bytes")


def test_wrapper_refuses_bad_arguments_before_the_library():
    """DemoBuffer on CPU tensors: every bad argument is a ValueError raised before anything is loaded."""
    import torch
    from balatro_gym_amd import DemoBuffer
    for bad in (0, -1, 2 ** 31):
        with pytest.raises(ValueError, match="capacity must be in"):
            DemoBuffer(bad, "cpu")
    for bad in (344, 360, 0):
        with pytest.raises(ValueError, match="row_stride must be"):
            DemoBuffer(8, "cpu", row_stride=bad)
    demo = DemoBuffer(8, "cpu", row_stride=352)
    assert tuple(demo.rows.shape) == (8, 352) and demo.rows.data_ptr() % 128 == 0 and demo.weight.dtype == torch.float32 and demo.source.dtype == torch.int32
    assert demo.cursor.dtype == torch.int64 and tuple(demo.cursor.shape) == (2,) and len(demo) == 0 and demo.filled() == 0
    assert demo.actions.dtype == torch.int32 and tuple(demo.actions.shape) == (8,) and demo.actions.data_ptr() == demo.rows.data_ptr() + 172
    assert demo.returns.dtype == torch.float64 and tuple(demo.returns.shape) == (8,) and demo.returns.data_ptr() == demo.rows.data_ptr() + 136
    K, N = 3, 5
    store = torch.zeros((K + 1, N, 384), dtype=torch.uint8)
    w = torch.ones((K, N), dtype=torch.float32)
    for bad in (store[0], store.to(torch.int8), torch.zeros((K + 1, N, 360), dtype=torch.uint8), torch.zeros((K + 1, N, 768), dtype=torch.uint8)[:, :, :384], None):
        with pytest.raises(ValueError, match="rows must be a contiguous uint8|record stride"):
            demo.add(bad, w)
    with pytest.raises(ValueError, match="K >= 1"):
        demo.add(store[:1], w[:0])
    for bad in (w.double(), torch.ones((K + 1, N)), torch.ones((N, K)).t(), torch.ones(K * N), None):
        with pytest.raises(ValueError, match="weights must be a contiguous"):
            demo.add(store, bad)
    for bad in (torch.zeros((K, N)), torch.zeros((K, N + 1), dtype=torch.float64), torch.zeros((N, K), dtype=torch.float64).t()):
        with pytest.raises(ValueError, match="returns must be a contiguous"):
            demo.add(store, w, returns=bad)
    big = torch.empty((2 ** 20 + 1, 2 ** 11, 352), dtype=torch.uint8, device="meta")   # K * N = 2**31, with no memory behind it
    with pytest.raises(ValueError, match=r"below 2\*\*31"):
        demo.add(big, w)
    wide = DemoBuffer(24, "cpu", row_stride=384)
    with pytest.raises(ValueError, match="must not overlap the store"):
        wide.add(wide.rows[2:22].view(K + 1, N, 384), w)
    with pytest.raises(ValueError, match="must not share memory"):
        wide.add(store, wide.weight[:K * N].view(K, N))
    with pytest.raises(ValueError, match="the ring is on"):
        DemoBuffer(8, "meta").add(store, w)
    # everything right: what is left is that there is no CPU path
    with pytest.raises(ValueError, match="device tensor"):
        demo.add(store, w, returns=torch.zeros((K, N), dtype=torch.float64))
    with pytest.raises(ValueError, match="device tensor"):
        demo.sample(4, seed=1, t=0)
    for kw in (dict(seed=-1, t=0), dict(seed=1, t=2 ** 64), dict(seed=1.5, t=0), dict(seed=1, t=0, index0=-2)):
        with pytest.raises(ValueError, match="must be an integer in"):
            demo.sample(4, **kw)
    with pytest.raises(ValueError, match="m must be"):
        demo.sample(-1, seed=1, t=0)
    # the state of a ring: a round trip, and a ring of another shape is refused
    demo.cursor[0] = 3
    demo.rows[1, 7] = 9
    other = DemoBuffer(8, "cpu", row_stride=352)
    other.load_state_dict(demo.state_dict())
    assert other.filled() == 3 and int(other.rows[1, 7]) == 9
    demo.clear()
    assert len(demo) == 0 and other.filled() == 3
    with pytest.raises(ValueError, match="the state is of a ring"):
        DemoBuffer(9, "cpu", row_stride=352).load_state_dict(demo.state_dict())
    for bad in ([-1, 0], [3, 4], [3, -1]):
        state = dict(demo.state_dict(), cursor=torch.tensor(bad, dtype=torch.int64))
        with pytest.raises(ValueError, match="the state's cursor must hold"):
            other.load_state_dict(state)
    assert other.filled() == 3
