"""The observation checksum of a rollout (policy | BG_POLICY_HASH_OBS; BalatroVecEnv.stats()["obs_hash"]) restated in numpy uint64: bg_hash_image
(csrc/bg_step.h) over one 352-byte record, and the fold of the step engines (csrc/bg_engine3.h and csrc/bg_engine.h, `if (HASH) ohash ^= ...`) over
all records of a run.  All arithmetic is mod 2**64.  tests/test_engine3_instantiations.py applies it to records packed from the CPU oracle's arrays,
never to the device's own rows."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
MUL_LO, MUL_HI = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
# the step's own outputs are not part of the observation: reward (bytes 136..143), action (172..175), terminated (342)
EXCLUDED = tuple(range(136, 144)) + tuple(range(172, 176)) + (342,)


def hash_rows(rows):
    """H of every record: uint8 [..., >= 352] -> uint64 [...].  A record is 22 pieces of 16 bytes, each taken as two little-endian 64-bit words."""
    r = np.array(np.asarray(rows, np.uint8)[..., :352], order="C")   # (a copy: the caller's records are not modified)
    r[..., list(EXCLUDED)] = 0
    w = r.view("<u8")
    h = np.full(w.shape[:-1], GOLDEN, np.uint64)
    with np.errstate(over="ignore"):
        for k in range(22):
            h ^= w[..., 2 * k]; h *= MUL_LO; h ^= h >> np.uint64(29)
            h ^= w[..., 2 * k + 1]; h *= MUL_HI; h ^= h >> np.uint64(31)
    return h


def fold_terms(rows, t0=0, env_index0=0):
    """H(row) * (0x9E3779B97F4A7C15 + 2 * (t0 + t)) + (env_index0 + env) of every record of rows [T, N, >= 352]: uint64 [T, N]."""
    h = hash_rows(rows)
    T, N = h.shape
    with np.errstate(over="ignore"):
        f = GOLDEN + np.uint64(2) * (np.uint64(t0) + np.arange(T, dtype=np.uint64))
        return h * f[:, None] + (np.uint64(env_index0) + np.arange(N, dtype=np.uint64))[None, :]


def obs_hash(rows, t0=0, env_index0=0):
    """The folded checksum of rows [T, N, >= 352] as a Python int: the XOR of fold_terms over all (t, env)."""
    return int(np.bitwise_xor.reduce(fold_terms(rows, t0, env_index0).reshape(-1)))
