"""The per-env state arrays (hot, cold, the live deck, the reset template, the ring of pre-shuffled decks) as every kernel reaches them through the
accessors of bg_device.h, under everything that reads and writes them: fused rollouts of the step engine (prologue, the service batch's loads and
stores, the owner's fetch-ahead of the next ring deck, resets), the refill's scan and deck kernels (whole and in pieces), state blobs between handles of
different sizes, deck injection, and the lane-equals-env kernels of the per-key step path.  Every record byte, reward bits, actions, terminated
flags and rollout statistics against the C oracle, as tests/test_refill_slots_gpu.py does it for the shop-stream ring.

200 envs are three full waves and a fourth with 8 live envs (one workgroup of 256 with 56 dead lanes).  The deck ring runs at its default depth
(248 slots, a refill every 372 steps) and at the smallest depths: BG_KD = 2 (with BG_KS = 3) is the smallest ring whose refill still runs beside
the launches, BG_KD = 1 the smallest the library takes -- both give a refill every 3 steps, so an env's one or two slots are written and consumed
over and over."""
import random

import numpy as np
import pytest

from tests.helpers import OBS_KEYS, assert_step_outputs, poison_env_outputs
from tests.test_gpu_parity import SEED_OFFSET, _assert_obs, _obs_np, _oracle_envs, _vec

pytestmark = pytest.mark.gpu

N = 200
POLICY, PSEED, ENV_INDEX0 = 0, 31, 2   # the uniform policy: it reaches shops and loses blinds (a reset consumes a ring deck)
T_DEFAULT = 4 * 372


def _setup():
    from oracle.gen_golden import IMPLEMENTED
    seeds = [61_000 + SEED_OFFSET + 7 * i for i in range(N)]
    jokers = [random.Random(6100 + i).sample(IMPLEMENTED, 5) for i in range(N)]
    return seeds, jokers


_full = []


def _oracle(T):
    """The oracle's SAME_STEP auto-reset rollout (tests/test_refill_slots_gpu._oracle, at this file's N): computed ONCE over the longest run and shared
    read-only; a shorter run is its prefix, with the statistics of that prefix."""
    if not _full:
        import ctypes as C
        from oracle import pyoracle as po
        L = po.lib()
        seeds, jokers = _setup()
        orc = _oracle_envs(N, seeds, True, 4, jokers)
        hs = [o.handle for o in orc]
        jk = [(C.c_int32 * len(j))(*j) for j in jokers]
        TT = T_DEFAULT
        obs, info = ((po.Obs * N) * TT)(), ((po.Info * N) * TT)()
        rew, term, acts = np.zeros((TT, N)), np.zeros((TT, N), np.uint8), np.zeros((TT, N), np.int32)
        r, tm = C.c_double(), C.c_uint8()
        for t in range(TT):
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
        o = np.frombuffer(obs, dtype=np.dtype(po.Obs)).reshape(TT, N)
        f = np.frombuffer(info, dtype=np.dtype(po.Info)).reshape(TT, N)
        wobs = {k: np.ascontiguousarray(o[k]).astype(po.OBS_DTYPES[k], copy=False) for k in OBS_KEYS}
        played, score = f["hand_type"] >= 0, np.ascontiguousarray(f["final_score"])
        for arr in list(wobs.values()) + [rew, term, acts, played, score]:
            arr.setflags(write=False)
        _full.append((wobs, rew, term, acts, played, score))
    wobs, rew, term, acts, played, score = _full[0]
    assert T <= rew.shape[0]
    odd = (2 * np.arange(T, dtype=np.uint64) + np.uint64(1))[:, None]
    stats = {"steps": T * N, "episodes": int(term[:T].sum()), "plays": int(played[:T].sum()), "score_sum": int(score[:T][played[:T]].sum()),
             "reward_bits": int(np.bitwise_xor.reduce((rew[:T].view(np.uint64) * odd).ravel()))}   # (uint64 products wrap, as the kernel's do)
    return {k: v[:T] for k, v in wobs.items()}, rew[:T], term[:T], acts[:T], stats


def _assert_records(rb, cols, want, rows, wcols, ctx):
    wobs, wr, wt, wa = want
    assert np.array_equal(rb.action[:, cols].cpu().numpy(), wa[rows, wcols]), f"{ctx}: actions"
    assert np.array_equal(rb.terminated[:, cols].cpu().numpy(), wt[rows, wcols]), f"{ctx}: terminated"
    assert np.array_equal(rb.reward[:, cols].contiguous().cpu().numpy().view(np.uint64), wr[rows, wcols].view(np.uint64)), f"{ctx}: reward bits"
    for key in OBS_KEYS:
        assert np.array_equal(rb.tensors[key][:, cols].contiguous().cpu().numpy(), wobs[key][rows, wcols]), f"{ctx}: record key {key} differs"


def _run_and_compare(monkeypatch, kd, ks, sizes, T, period):
    from balatro_gym_amd.vec_env import RowBuffers
    if kd is not None:
        monkeypatch.setenv("BG_KD", str(kd)); monkeypatch.setenv("BG_KS", str(ks))
    seeds, jokers = _setup()
    env = _vec(N, seeds, scorer_jokers=True, autoreset=True, max_ante=4)
    env.inject(jokers=jokers, apply_now=True)
    assert env.max_fused_steps == period, (env.max_fused_steps, period)   # the refill period the launch sizes were chosen for
    wobs, wr, wt, wa, wstats = _oracle(T)
    if kd is not None:
        # long enough, by the oracle alone: a reset consumes one ring deck, so an env that ended more than 2 * KD episodes has been through every
        # slot of its ring more than twice (written by a refill, consumed, written again)
        assert int((wt.sum(axis=0) > 2 * kd).sum()) * 4 >= 3 * N, "too few envs consume their deck ring several times over"
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
    _assert_records(rb, slice(None), (wobs, wr, wt, wa), slice(None), slice(None), f"KD {kd} sizes {sizes}")
    for key in ("steps", "episodes", "plays", "score_sum", "reward_bits"):
        assert got_stats[key] == wstats[key], (key, got_stats[key], wstats[key])
    env.close()


@pytest.mark.parametrize("mode,sizes", [("whole", (372,)), ("pieces", (20, 13, 30, 7, 20, 20))])
def test_default_ring_depths_vs_oracle(monkeypatch, mode, sizes):
    """Default depths: 4 x 372 steps -- three refills, whole beside 372-step launches or in pieces beside launches of 7..30 steps."""
    _run_and_compare(monkeypatch, None, None, sizes, T_DEFAULT, 372)


@pytest.mark.parametrize("mode,kd,ks,sizes,T", [("whole", 2, 3, (3,), 720), ("pieces", 2, 3, (1,), 720), ("between", 1, 3, (3,), 480)])
def test_smallest_deck_rings_vs_oracle(monkeypatch, mode, kd, ks, sizes, T):
    """BG_KD = 2: the smallest deck ring whose refill still runs beside the launches (period 3: whole beside 3-step launches, in pieces beside 1-step
    ones); BG_KD = 1, the smallest the library takes: no look-ahead left to overlap, the refill runs between the launches (the shop ring keeps its
    BG_KS = 3 there: with BG_KS = 2 these envs run out of shop streams by step 480 -- error word 8 -- in the library before this layout just the same,
    which is the shop ring's matter and not the deck ring's).  The lengths are the oracle's: under this policy and these
    jokers an env ends an episode every ~150 steps, and 165 of the 200 envs have ended more than four by step 720 (168 more than two by step 480)."""
    _run_and_compare(monkeypatch, kd, ks, sizes, T, 3)


def test_state_blob_between_handles_of_other_sizes_vs_oracle(monkeypatch):
    """bg_get_state of the LAST env of a 200-env handle into env 0 of a 70-env handle: the blob's bytes do not depend on where an env's chunks lie on
    the device.  Shallow rings and 5-step launches (a refill every fourth launch, issued in pieces beside the launches behind it -- bg_get_state has
    to issue what is pending); both handles then take the same 60 steps, and their records must agree with each other and with the oracle."""
    from balatro_gym_amd.vec_env import BalatroVecEnv, RowBuffers
    KG, KS, KD = 8, 13, 12
    monkeypatch.setenv("BG_KG", str(KG)); monkeypatch.setenv("BG_KS", str(KS)); monkeypatch.setenv("BG_KD", str(KD))
    monkeypatch.setenv("BG_REFILL_SLICED", "1")
    nB, src, dst, L, K, M = 70, N - 1, 0, 5, 4, 60
    seeds, jokers = _setup()
    A = _vec(N, seeds, scorer_jokers=True, autoreset=True, max_ante=4)
    assert L <= A.max_fused_steps // 2 and L * K > A.max_fused_steps, A.max_fused_steps   # short launches, and the K-th one asks for a refill
    A.inject(jokers=jokers, apply_now=True)
    rbA = RowBuffers(N, A.device, steps=L)
    for j in range(K):
        A.rollout(L, policy=POLICY, policy_seed=PSEED, env_index0=ENV_INDEX0, t0=L * j, obs_buffers=rbA, zero_stats=(j == 0))
    blob = A.get_state(src)
    # version 7 and its size: header, hot 128, deck 64, cold 112, template 32, ring decks, global blocks, shop slots, overflow + two lazy streams,
    # the ring of 128 pre-drawn shop seeds, its meta word, the producer word
    assert int(np.frombuffer(blob[:16], np.uint32)[1]) == 7
    assert len(blob) == 16 + 128 + 64 + 112 + 32 + KD * 64 + KG * 2560 + KS * 256 + 3 * 2560 + 128 * 4 + 4 + 4
    assert BalatroVecEnv.parse_state_blob(blob)["KD"] == KD
    B = _vec(nB, [9 + i for i in range(nB)], scorer_jokers=True, autoreset=True, max_ante=4)
    B.set_state(dst, blob)
    t0 = L * K
    rbA2, rbB = RowBuffers(N, A.device, steps=M), RowBuffers(nB, B.device, steps=M)
    A.rollout(M, policy=POLICY, policy_seed=PSEED, env_index0=ENV_INDEX0, t0=t0, obs_buffers=rbA2, zero_stats=True)
    B.rollout(M, policy=POLICY, policy_seed=PSEED, env_index0=ENV_INDEX0 + src - dst, t0=t0, obs_buffers=rbB, zero_stats=True)
    A.check(); B.check()
    wobs, wr, wt, wa, _ = _oracle(t0 + M)
    want = (wobs, wr, wt, wa)
    _assert_records(rbA2, slice(None), want, slice(t0, t0 + M), slice(None), "the 200-env handle")
    _assert_records(rbB, dst, want, slice(t0, t0 + M), src, "the restored env")
    assert np.array_equal(rbB.rows[:, dst].cpu().numpy(), rbA2.rows[:, src].cpu().numpy()), "the two handles' records differ"
    # a known deck, injected live: the blob's deck slice is that deck, in order, then its padding
    decks = np.stack([np.random.RandomState(700 + i).permutation(52) for i in range(nB)]).astype(np.uint8)
    B.inject_deck(decks)
    for i in (dst, nB - 1):
        b2 = np.frombuffer(B.get_state(i), np.uint8)
        assert np.array_equal(b2[16 + 128:16 + 128 + 52], decks[i]) and not b2[16 + 128 + 52:16 + 128 + 64].any(), f"deck slice of env {i}"
    A.close(); B.close()


def test_per_key_step_path_vs_oracle():
    """The lane-equals-env kernels (bg_step, bg_reset, bg_observe, the refill scan) at N = 200: 40 steps in lockstep with the oracle, every output
    word, with a reset of the envs that ended an episode after each step and of a fixed third of all envs in the middle."""
    import torch
    seeds, jokers = _setup()
    env = _vec(N, seeds, scorer_jokers=True, autoreset=False, max_ante=4)
    env.inject(jokers=jokers, apply_now=True)
    env.observe()
    orc = _oracle_envs(N, seeds, True, 4, jokers)
    _assert_obs(_obs_np(env), {k: np.stack([o.obs()[k] for o in orc]) for k in OBS_KEYS}, "initial")
    for t in range(40):
        acts = np.array([o.policy_action(POLICY, PSEED, ENV_INDEX0 + i, t) for i, o in enumerate(orc)], dtype=np.int32)
        res = [o.step(int(a)) for o, a in zip(orc, acts)]
        poison_env_outputs(env)
        ob, reward, term, trunc, info = env.step(torch.from_numpy(acts).to(env.device))
        assert_step_outputs(f"t {t}", res, reward, term, trunc, info, obs=ob)
        mask = np.array([r[2] for r in res], dtype=np.uint8)
        if t == 20:
            mask[::3] = 1
        if mask.any():
            for i in np.nonzero(mask)[0]:
                orc[i].reset(); orc[i].set_jokers(jokers[i])
            env.reset(mask=torch.from_numpy(mask).to(env.device))
            _assert_obs(_obs_np(env), {k: np.stack([o.obs()[k] for o in orc]) for k in OBS_KEYS}, f"reset behind t {t}")
    env.check()
    env.close()
