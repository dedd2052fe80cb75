"""The reference of bg_demo_append_rows / bg_demo_sample (csrc/bg_demo.h): the contract restated in numpy and Python integers.  The keep test is a
float comparison (`np.isfinite(w) & (w > 0)`), the kept rows come from `np.flatnonzero`, ranks / slots / the drop rule are Python integers, and the
record blend is byte slicing by `_native.ROW_OFFSETS` / `ROW_EXTRA` -- none of it shares a line with the C piece arithmetic.  All of the call is
integer work, so the kernel and the host twin are held to this BYTE FOR BYTE.  Also the generator of synthetic inputs the host and GPU tests share.
"""
from __future__ import annotations

import numpy as np

from balatro_gym_amd import _native as nat
from tests import head_ref

ROW = nat.ROW_BYTES
OFF_REWARD, OFF_ACTION, OFF_TERM = nat.ROW_EXTRA["reward"][0], nat.ROW_EXTRA["action"][0], nat.ROW_EXTRA["terminated"][0]
OFF_BOSS = nat.ROW_OFFSETS["boss_blind_active"]
# the fields of the step that FOLLOWED the observation: [first byte, one past the last)
NEXT_FIELDS = {"action": (OFF_ACTION, OFF_ACTION + 4), "ending": (OFF_TERM, nat.ROW_EXTRA["end_chips"][0] + 4)}
assert NEXT_FIELDS["ending"] == (342, ROW) and OFF_BOSS == 340 and nat.ROW_OFFSETS["boss_blind_type"] == 341


def keep(weights: np.ndarray) -> np.ndarray:
    """bool [M]: the weight is finite and > 0 (a denormal is; +0.0, -0.0, negatives, NaN and the infinities are not)."""
    w = np.asarray(weights, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        return np.isfinite(w) & (w > 0)


def demo_record(obs_rec: np.ndarray, next_rec: np.ndarray, ret=None) -> np.ndarray:
    """One demo record (uint8 [352]) from the observation record and the record of the step taken from it."""
    out = obs_rec[:ROW].copy()
    for a, b in NEXT_FIELDS.values():
        out[a:b] = next_rec[a:b]
    out[OFF_REWARD:OFF_REWARD + 8] = next_rec[OFF_REWARD:OFF_REWARD + 8] if ret is None else np.frombuffer(np.float64(ret).tobytes(), np.uint8)
    return out


def append(store: np.ndarray, weights, returns, ring: np.ndarray, demo_weight: np.ndarray, demo_source, cursor: np.ndarray) -> dict:
    """The call on copies: store uint8 [K + 1, N, stride], weights float32 [K, N], returns float64 [K, N] or None, ring uint8 [C, dstride], demo_weight
    float32 [C], demo_source int32 [C] or None, cursor int64 [2] -> dict(ring, weight, source, cursor, written): `written` lists the slots written, in
    rank order (no slot twice)."""
    K1, N, _ = store.shape
    K, C = K1 - 1, ring.shape[0]
    ring, demo_weight, cursor = ring.copy(), demo_weight.copy(), cursor.copy()
    demo_source = None if demo_source is None else demo_source.copy()
    w = np.asarray(weights, np.float32).reshape(-1)
    assert w.size == K * N
    flat = store.reshape(K1 * N, -1)
    kept_rows = [int(i) for i in np.flatnonzero(keep(w))]
    kept, T0 = len(kept_rows), max(int(cursor[0]), 0)   # (a negative count is not a state the call leaves: it is taken as an empty ring)
    drop = max(kept - C, 0)
    written = []
    for r, i in enumerate(kept_rows):
        if r < drop:
            continue
        slot = (T0 + r) % C
        ret = None if returns is None else np.asarray(returns, np.float64).reshape(-1)[i]
        ring[slot, :ROW] = demo_record(flat[i], flat[i + N], ret)
        demo_weight[slot] = w[i]
        if demo_source is not None:
            demo_source[slot] = i
        written.append(slot)
    assert len(set(written)) == len(written) == min(kept, C)
    if K * N > 0:
        cursor[0], cursor[1] = T0 + kept, kept
    return {"ring": ring, "weight": demo_weight, "source": demo_source, "cursor": cursor, "written": written}


def sample(total: int, capacity: int, seed: int, index0: int, t: int, m: int) -> np.ndarray:
    """int32 [m]: the multiply-high draw over filled = min(total, capacity) slots from the counter hash; -1 where the ring is empty."""
    filled = min(max(int(total), 0), int(capacity))
    if filled == 0:
        return np.full(m, -1, np.int32)
    h = head_ref.policy_hash(seed, np.arange(m, dtype=np.uint64) + np.uint64(index0), t)
    return np.array([(int(x) * filled) >> 32 for x in h], dtype=np.int32)


SPECIAL_WEIGHTS = np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1e-45, 1e-39, 1.0, 3.5, np.finfo(np.float32).max, np.finfo(np.float32).tiny],
                           dtype=np.float32)
SPECIAL_KEPT = np.array([0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1], dtype=bool)


def synthetic_store(seed: int, K: int, N: int, stride: int) -> np.ndarray:
    """uint8 [K + 1, N, stride] of random BYTES: every byte's origin shows, the bytes above 352 of a 384-byte record included."""
    return np.random.default_rng(seed).integers(0, 256, (K + 1, N, stride), dtype=np.uint8)


def synthetic_weights(seed: int, K: int, N: int, share: float, special: bool = True) -> np.ndarray:
    """float32 [K, N]: about `share` of the rows kept (exactly none at 0.0, all at 1.0) with varied positive weights; the rows not kept carry zeros and,
    with `special`, negatives, NaNs and infinities; the kept ones a few denormals."""
    rng = np.random.default_rng(seed + 1)
    k = rng.random((K, N)) < share
    w = np.where(k, rng.random((K, N)).astype(np.float32) + np.float32(0.25), np.float32(0.0)).astype(np.float32)
    if special and K * N >= 8:
        bad = np.array([-0.0, -2.0, np.nan, np.inf, -np.inf], np.float32)
        pick = rng.integers(0, bad.size, (K, N))
        w = np.where(~k & (rng.random((K, N)) < 0.5), bad[pick], w).astype(np.float32)
        w = np.where(k & (rng.random((K, N)) < 0.1), np.float32(1e-42), w).astype(np.float32)
    assert np.array_equal(keep(w), k.reshape(-1))
    return w


def fresh_ring(seed: int, C: int, dstride: int):
    """(ring, demo_weight, demo_source, cursor): random bytes / poison values, so a slot that is not written -- or the bytes above 352 -- show."""
    rng = np.random.default_rng(seed + 2)
    return (rng.integers(0, 256, (C, dstride), dtype=np.uint8), np.full(C, -7.0, np.float32), np.full(C, -9, np.int32), np.zeros(2, np.int64))


def assert_same(got: dict, want: dict, what: str) -> None:
    for f in ("cursor", "source", "weight", "ring"):
        g, w = got[f], want[f]
        if w is None:
            continue
        g = np.asarray(g)
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {f} is {g.dtype}{list(g.shape)}, want {w.dtype}{list(w.shape)}"
        same = g.view(np.uint32) == w.view(np.uint32) if f == "weight" else g == w
        assert same.all(), f"{what}: {f} differs at {np.argwhere(~same)[0].tolist()} ({int((~same).sum())} elements)"
