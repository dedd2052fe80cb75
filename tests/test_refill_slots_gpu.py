"""Shop-stream ring slots as the refill seeds them (bg_refill_shop_kernel: built in registers, every 16-byte group stored once, never read by
the kernel that writes them) under the step engine that consumes them: every record byte of fused rollouts against the C oracle, over enough
steps that the envs visit shops out of slots that at least two different refills have re-seeded.

192 envs are three waves of work items, the last one partial as soon as the rings are partly full.  The shop ring runs at its default depth
(249 slots: a refill every 372 steps) and at the smallest depths the library takes (BG_KS = 3: one slot consumed, one re-seeded, a refill every
3 steps -- every slot is rewritten over and over; BG_KS = 2: no look-ahead left to overlap, the refill runs between the launches).  The refill
runs once WHOLE beside the launch that asks for it (a launch is a refill period of its own) and once IN PIECES beside the short launches that
follow (at most half a period each)."""
import random

import numpy as np
import pytest

from tests.helpers import OBS_KEYS
from tests.test_gpu_parity import SEED_OFFSET, _oracle_envs, _vec

pytestmark = pytest.mark.gpu

N = 192
POLICY, PSEED, ENV_INDEX0 = 0, 31, 2   # the uniform policy: it reaches shops


def _setup():
    from oracle.gen_golden import IMPLEMENTED
    seeds = [52_000 + SEED_OFFSET + 7 * i for i in range(N)]
    jokers = [random.Random(5200 + i).sample(IMPLEMENTED, 5) for i in range(N)]
    return seeds, jokers


_want = {}


def _oracle(T):
    """The oracle's SAME_STEP auto-reset rollout over T steps (what test_gpu_parity._oracle_rollout computes, whose environments, joker re-injection
    and statistics this follows), computed once per length and shared read-only.  The oracle writes every observation straight into one block of
    [T][N] structs that numpy then reads by field -- a dictionary of arrays per step and env would cost more than the run under test."""
    if T in _want:
        return _want[T]
    import ctypes as C
    from oracle import pyoracle as po
    L = po.lib()
    seeds, jokers = _setup()
    orc = _oracle_envs(N, seeds, True, 4, jokers)
    hs = [o.handle for o in orc]
    jk = [(C.c_int32 * len(j))(*j) for j in jokers]
    obs, info = ((po.Obs * N) * T)(), ((po.Info * N) * T)()
    rew, term, acts = np.zeros((T, N)), np.zeros((T, N), np.uint8), np.zeros((T, N), np.int32)
    r, tm = C.c_double(), C.c_uint8()
    for t in range(T):
        ot, it = obs[t], info[t]
        for i in range(N):
            h = hs[i]
            a = L.bo_policy_action(h, POLICY, PSEED, ENV_INDEX0 + i, t)
            L.bo_step(h, a, C.byref(r), C.byref(tm), C.byref(it[i]))
            if tm.value:
                L.bo_reset(h, 0, 0)
                L.bo_set_jokers(h, jk[i], len(jk[i]))
            L.bo_get_obs(h, C.byref(ot[i]))
            rew[t, i] = r.value; term[t, i] = tm.value; acts[t, i] = a
    o = np.frombuffer(obs, dtype=np.dtype(po.Obs)).reshape(T, N)
    f = np.frombuffer(info, dtype=np.dtype(po.Info)).reshape(T, N)
    wobs = {k: np.ascontiguousarray(o[k]).astype(po.OBS_DTYPES[k], copy=False) for k in OBS_KEYS}
    played = f["hand_type"] >= 0
    odd = (2 * np.arange(T, dtype=np.uint64) + np.uint64(1))[:, None]
    stats = {"steps": T * N, "episodes": int(term.sum()), "plays": int(played.sum()), "score_sum": int(f["final_score"][played].sum()),
             "reward_bits": int(np.bitwise_xor.reduce((rew.view(np.uint64) * odd).ravel()))}   # (uint64 products wrap, as the kernel's do)
    for arr in list(wobs.values()) + [rew, term, acts]:
        arr.setflags(write=False)
    _want[T] = (wobs, rew, term, acts, stats)
    return _want[T]


def _run_and_compare(monkeypatch, ks, sizes, T, periods):
    from balatro_gym_amd.vec_env import RowBuffers
    if ks is not None:
        monkeypatch.setenv("BG_KS", str(ks))
    seeds, jokers = _setup()
    env = _vec(N, seeds, scorer_jokers=True, autoreset=True, max_ante=4)
    env.inject(jokers=jokers, apply_now=True)
    period = env.max_fused_steps
    assert period == periods, (period, periods)   # the refill period the launch sizes below were chosen for
    rb = RowBuffers(N, env.device, steps=T)
    done, k = 0, 0
    while done < T:
        c = min(sizes[k % len(sizes)], T - done)
        part = RowBuffers.__new__(RowBuffers)
        part.n, part.steps, part.rows = N, c, rb.rows[done:done + c]
        env.rollout(c, policy=POLICY, policy_seed=PSEED, env_index0=ENV_INDEX0, t0=done, obs_buffers=part, zero_stats=(done == 0))
        done += c; k += 1
    env.check()
    got_stats = env.stats()
    wobs, wr, wt, wa, wstats = _oracle(T)
    # the run is long enough: the first period plays out of the reset's own slots, the next one out of the first refill's (a launch reads the refill
    # BEFORE the one beside it), so from the fourth period on every shop visit reads slots that a second or later refill seeded over consumed ones.
    # A uniform policy does not take EVERY env to a shop in a given stretch (an env that keeps losing its first blind never sees one): three in four
    # of them in the run's last quarter is what the test asks for.  (phase 1 = BO_PHASE_SHOP, oracle/balatro_oracle.h)
    late = wobs["phase"][max(3 * period, T - T // 4):]
    assert T >= 4 * period and int((late == 1).any(axis=0).sum()) * 4 >= 3 * N, "too few envs reach a shop out of slots of a later refill"
    assert np.array_equal(rb.action.cpu().numpy(), wa)
    assert np.array_equal(rb.terminated.cpu().numpy(), wt)
    assert np.array_equal(rb.reward.contiguous().cpu().numpy().view(np.uint64), wr.view(np.uint64))
    for key in OBS_KEYS:
        assert np.array_equal(rb.tensors[key].contiguous().cpu().numpy(), wobs[key]), f"record key {key} differs"
    for key in ("steps", "episodes", "plays", "score_sum", "reward_bits"):
        assert got_stats[key] == wstats[key], (key, got_stats[key], wstats[key])
    env.close()


@pytest.mark.parametrize("mode,sizes", [("whole", (372,)), ("pieces", (20, 13, 30, 7, 20, 20))])
def test_default_ring_slots_vs_oracle(monkeypatch, mode, sizes):
    """Default depth: 4 x 372 steps -- three refills, whole beside 372-step launches or in pieces beside launches of 7..30 steps."""
    _run_and_compare(monkeypatch, None, sizes, 4 * 372, 372)


@pytest.mark.parametrize("mode,ks,sizes", [("whole", 3, (3,)), ("pieces", 3, (1,)), ("between", 2, (3,))])
def test_smallest_ring_slots_vs_oracle(monkeypatch, mode, ks, sizes):
    """BG_KS = 3: the smallest ring whose refill still runs beside the launches (period 3: whole beside 3-step launches, in pieces beside 1-step ones);
    BG_KS = 2, the smallest the library takes: one slot of look-ahead, the refill between the launches.  240 steps = 80 refills of the same few slots."""
    _run_and_compare(monkeypatch, ks, sizes, 240, 3)
