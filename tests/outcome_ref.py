"""The reference of bg_episode_outcome_rows (csrc/bg_outcome.h): the loop of the contract in numpy, one step of all envs at a time, backwards.
Every operation of the chain is elementwise float64 / int32, so numpy computes per env exactly what a scalar loop would: the kernel and the host twin
are held to it BIT FOR BIT.  Also the generator of synthetic records the host and the GPU test share.
"""
from __future__ import annotations

import numpy as np

from balatro_gym_amd import _native as nat

FIELDS = ("steps_to_end", "end_ante", "end_flags", "returns")
DTYPES = {"steps_to_end": np.int32, "end_ante": np.int32, "end_flags": np.uint8, "returns": np.float64}
DEFAULTS = {"steps_to_end": -1, "end_ante": -1, "end_flags": 0, "returns": 0.0}
OFF_REWARD, OFF_TERM, OFF_FLAGS, OFF_ANTE = nat.ROW_EXTRA["reward"][0], nat.ROW_EXTRA["terminated"][0], nat.ROW_EXTRA["end_flags"][0], nat.ROW_EXTRA["end_ante"][0]
KINDS = ("never", "every", "first", "last")   # an env that never ends, ends on every step, ends at t = 0 only, ends at t = K - 1 only


def fields_of(rows: np.ndarray):
    """rows uint8 [K, N, stride] -> (reward float64, terminated bool, end_flags uint8, end_ante int16), each [K, N]."""
    K, N, _ = rows.shape
    reward = np.ascontiguousarray(rows[:, :, OFF_REWARD:OFF_REWARD + 8]).view(np.float64).reshape(K, N)
    ante = np.ascontiguousarray(rows[:, :, OFF_ANTE:OFF_ANTE + 2]).view(np.int16).reshape(K, N)
    return reward, rows[:, :, OFF_TERM] != 0, rows[:, :, OFF_FLAGS].copy(), ante


def outcome_loop(rows: np.ndarray, gamma: float = 1.0, rewards=None, tail=None) -> dict:
    """The contract's loop.  tail: dict field -> [N] array (missing fields take the defaults).  -> dict field -> [K, N] array."""
    K, N, _ = rows.shape
    reward, done, flags, ante = fields_of(rows)
    if rewards is not None:
        reward = np.asarray(rewards, np.float64).reshape(K, N)
    tail = tail or {}
    nx = {f: np.full(N, DEFAULTS[f], DTYPES[f]) if tail.get(f) is None else np.asarray(tail[f], DTYPES[f]).copy() for f in FIELDS}
    out = {f: np.empty((K, N), DTYPES[f]) for f in FIELDS}
    g = np.float64(gamma)
    with np.errstate(all="ignore"):
        for t in range(K - 1, -1, -1):
            d = done[t]
            disc = g * nx["returns"]                      # rounds
            cont = reward[t] + disc                       # rounds
            nx = {"steps_to_end": np.where(d, 0, np.where(nx["steps_to_end"] < 0, -1, nx["steps_to_end"] + 1)).astype(np.int32),
                  "end_ante": np.where(d, ante[t].astype(np.int32), nx["end_ante"]).astype(np.int32),
                  "end_flags": np.where(d, flags[t], nx["end_flags"]).astype(np.uint8),
                  "returns": np.where(d, reward[t], cont)}
            for f in FIELDS:
                out[f][t] = nx[f]
    return out


def synthetic_rows(seed: int, K: int, N: int, stride: int, kind0: str | None = None, p_end: float = 0.15) -> np.ndarray:
    """uint8 [K, N, stride] records of random BYTES (so a decoder that reads a neighbouring byte is caught) with the four fields set: rewards N(0, 10^2)
    with a few exact zeros and huge values, a terminated byte set with probability p_end (any non-zero value), end flags and end antes (int16, negative
    and above 255 included) on EVERY record (only those of ended records may show).  With N >= 4 envs 0..3 are the four KINDS; kind0 makes env 0 that
    kind instead (for N < 4)."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 256, (K, N, stride), dtype=np.uint8)
    reward = rng.standard_normal((K, N)) * 10.0
    reward[rng.random((K, N)) < 0.05] = 0.0
    reward[rng.random((K, N)) < 0.02] *= 1e12
    done = rng.random((K, N)) < p_end
    kinds = {0: kind0} if kind0 is not None else ({i: k for i, k in enumerate(KINDS)} if N >= 4 else {})
    for e, kind in kinds.items():
        done[:, e] = kind == "every"
        if kind == "first":
            done[0, e] = True
        if kind == "last":
            done[K - 1, e] = True
    rows[:, :, OFF_REWARD:OFF_REWARD + 8] = reward.view(np.uint8).reshape(K, N, 8)
    rows[:, :, OFF_TERM] = np.where(done, rng.integers(1, 256, (K, N)), 0).astype(np.uint8)
    rows[:, :, OFF_FLAGS] = rng.integers(0, 256, (K, N)).astype(np.uint8)
    ante = rng.integers(-3, 400, (K, N)).astype(np.int16)
    rows[:, :, OFF_ANTE:OFF_ANTE + 2] = ante.view(np.uint8).reshape(K, N, 2)
    return rows


def synthetic_tail(seed: int, N: int) -> dict:
    """A tail of every field: open (-1) and closed envs mixed."""
    rng = np.random.default_rng(seed + 77)
    steps = np.where(rng.random(N) < 0.4, -1, rng.integers(0, 50, N)).astype(np.int32)
    return {"steps_to_end": steps, "end_ante": np.where(steps < 0, -1, rng.integers(1, 9, N)).astype(np.int32),
            "end_flags": np.where(steps < 0, 0, rng.integers(1, 8, N)).astype(np.uint8), "returns": rng.standard_normal(N) * 5.0}


def assert_equal_bits(got: dict, want: dict, what: str, fields=FIELDS) -> None:
    for f in fields:
        g, w = np.asarray(got[f]), want[f]
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {f} is {g.dtype}{list(g.shape)}, want {w.dtype}{list(w.shape)}"
        same = g.view(np.uint64) == w.view(np.uint64) if f == "returns" else g == w
        assert same.all(), f"{what}: {f} differs at {np.argwhere(~same)[0].tolist()} ({(~same).sum()} elements)"
