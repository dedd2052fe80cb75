"""Host tests of tests/hash_ref.py, the numpy restatement of the observation checksum (bg_hash_image and the engines' fold): that it covers what it
claims to cover.  tests/test_engine3_instantiations.py holds the device's checksum to it; these need no GPU."""
import numpy as np

from tests import hash_ref
from tests.helpers import OBS_KEYS
from tests.test_step_many_safe import _pack


def _oracle_records(n=3, steps=12):
    """Records [steps, n, 352] packed from the CPU oracle's observations: the uniform policy on fresh seeds."""
    from oracle import pyoracle as po
    orc = [po.OracleEnv(4100 + 7 * i, scorer_jokers=True) for i in range(n)]
    rows = []
    for t in range(steps):
        acts = [o.policy_action(0, 3, i, t) for i, o in enumerate(orc)]
        res = [o.step(int(a)) for o, a in zip(orc, acts)]
        obs = {k: np.stack([np.asarray(r[0][k]) for r in res]) for k in OBS_KEYS}
        rows.append(_pack(obs, np.array([r[1] for r in res]), np.array(acts, np.int32), np.zeros(n, np.uint8)))
    return np.stack(rows)


def test_every_bit_outside_the_excluded_fields_changes_the_hash():
    """On one oracle-made record: flipping any single bit of bytes 0..351 outside reward (136..143), action (172..175) and terminated (342) changes
    H, flipping one inside them does not -- and the record itself is left as it was."""
    rec = _oracle_records()[-1, 0]
    assert rec[:136].any() and rec[176:342].any()
    keep = rec.copy()
    flipped = np.repeat(rec[None], 352 * 8, axis=0)
    for b in range(352 * 8):
        flipped[b, b // 8] ^= 1 << (b % 8)
    changed = hash_ref.hash_rows(flipped) != hash_ref.hash_rows(rec)
    assert np.array_equal(rec, keep)
    excluded = np.zeros(352, bool)
    excluded[list(hash_ref.EXCLUDED)] = True
    assert excluded.sum() == 13
    want = np.repeat(~excluded, 8)
    bad = np.flatnonzero(changed != want)
    assert not len(bad), f"bit {bad[0] % 8} of byte {bad[0] // 8}: H {'changed' if changed[bad[0]] else 'did not change'} ({len(bad)} bits in all)"


def test_hash_is_the_c_arithmetic():
    """One record by hand in Python integers mod 2**64, piece by piece as bg_hash_image reads them (x, y, z, w of 22 uint4)."""
    rec = _oracle_records()[-1, 1]
    M = 2 ** 64 - 1
    w = rec.copy().view("<u4").astype(object)
    h = 0x9E3779B97F4A7C15
    for k in range(22):
        x, y, z, ww = (int(v) for v in w[4 * k:4 * k + 4])
        if k == 8:
            z = ww = 0
        if k == 10:
            ww = 0
        if k == 21:
            y &= 0xff00ffff
        h ^= (y << 32) | x; h = (h * 0xBF58476D1CE4E5B9) & M; h ^= h >> 29
        h ^= (ww << 32) | z; h = (h * 0x94D049BB133111EB) & M; h ^= h >> 31
    assert int(hash_ref.hash_rows(rec)) == h


def test_fold_depends_on_step_and_env_index():
    """The fold is the XOR of H * (0x9E3779B97F4A7C15 + 2 * (t0 + t)) + (env_index0 + env) in Python integers.  Swapping two records' steps changes
    the folded value, always; swapping two records' env indexes changes it in most cases but not in all (see below); t0 and env_index0 change it."""
    rows = _oracle_records(n=8)
    T, N = rows.shape[:2]
    base = hash_ref.obs_hash(rows, t0=48, env_index0=2)
    H = hash_ref.hash_rows(rows)
    by_hand = 0
    for t in range(T):
        for e in range(N):
            by_hand ^= (int(H[t, e]) * (0x9E3779B97F4A7C15 + 2 * (48 + t)) + 2 + e) & (2 ** 64 - 1)
    assert base == by_hand
    # the step enters as a factor: every swap of two different records of one env between two steps is seen
    seen = total = 0
    for e in range(N):
        for t1 in range(T):
            for t2 in range(t1 + 1, T):
                if H[t1, e] != H[t2, e]:
                    sw = rows.copy()
                    sw[[t1, t2], e] = rows[[t2, t1], e]
                    total += 1
                    seen += hash_ref.obs_hash(sw, t0=48, env_index0=2) != base
    assert total >= N * T and seen == total, (seen, total)
    # the env index enters by ADDITION only, so a swap of two envs' records of one step shows in the low bits of two sums alone, and the XOR of the
    # two can come out the same: about a quarter of such swaps are not seen (here 81 of 336).  A single swapped pair can escape the checksum;
    # records that go to the wrong env as a rule (a wrong lane or slot index: tens of pairs per step) cannot, short of 2**-40.  What is asserted
    # is that most single swaps are seen.
    seen = total = 0
    for t in range(T):
        for e1 in range(N):
            for e2 in range(e1 + 1, N):
                if H[t, e1] != H[t, e2]:
                    sw = rows.copy()
                    sw[t, [e1, e2]] = rows[t, [e2, e1]]
                    total += 1
                    seen += hash_ref.obs_hash(sw, t0=48, env_index0=2) != base
    print(f"swaps of two envs' records of one step seen by the fold: {seen} of {total}")
    assert total >= T * N and 2 * seen > total, (seen, total)
    assert hash_ref.obs_hash(rows, t0=49, env_index0=2) != base and hash_ref.obs_hash(rows, t0=48, env_index0=3) != base
    # two chunks folded one after the other are the whole run
    assert hash_ref.obs_hash(rows[:5], 48, 2) ^ hash_ref.obs_hash(rows[5:], 53, 2) == base
