"""GPU tests that run the instantiations of bg_engine3.h no other test reaches.  bg_engine_launch (csrc/bg_lib.hip) ships the one body template 30
times: three workgroup shapes (113 / 213 / 413: 64, 128 and 256 envs per workgroup) x with and without card states x five modes (rollout, rollout
with the observation checksum, the caller's actions, those under the episode limits, those under the limits and the progression rewards).  A job of
300 envs runs shape 113 unless BG_E3_CFG says otherwise, so every case here creates its handle behind monkeypatch.setenv("BG_E3_CFG", ...); the
shape axis is 113, 113 with 64 live envs per workgroup (BG_E3_EPW), 213 and 413.  DESIGN.md has the table of all 30 with the test that runs each
against the CPU oracle.

 A. PROG in every shape, with and without card states: the "shapes" scenario of tests/test_step_many_progress.py, in which envs 64, 128 and 192
    apart never end their episodes alike (a slot of another owner wave read by accident holds a wrong value), and its "idle" scenario (stuck endings).
 B. ACT and SAFE with injected card states and consumables in every shape.
 C. The observation checksum against tests/hash_ref.py applied to records packed from the ORACLE's arrays."""
import functools
import random

import numpy as np
import pytest

from tests import hash_ref
from tests import progress_ref
from tests import safe_ref
from tests import test_step_many_progress as prog
from tests.helpers import OBS_KEYS, POISON, poison_
from tests.test_gpu_parity import (CARD_CHUNKS, CARD_INDEX0, CARD_N, CARD_PSEED, CARD_T, SEED_OFFSET, _card_state_env, _card_state_rollout,
                                   _oracle_rollout, _stats_of_steps, _vec)
from tests.test_step_many_safe import R_FLAGS, R_TERM, _diff, _first_masked, _pack, _shallow_rings, _terminal_sets

pytestmark = pytest.mark.gpu

SHAPES = [(113, None), (113, 64), (213, None), (413, None)]   # (BG_E3_CFG, BG_E3_EPW)
SHAPE_IDS = ["113", "113-epw64", "213", "413"]
STAT_KEYS = ("steps", "episodes", "plays", "score_sum", "reward_bits")


def _set_shape(monkeypatch, cfg, epw):
    """bg_create_ex reads both per handle: set them BEFORE the handle is made."""
    monkeypatch.setenv("BG_E3_CFG", str(cfg))
    if epw is not None:
        monkeypatch.setenv("BG_E3_EPW", str(epw))


# ---------------------------------------------------------------------------------------------------------------- A. PROG
def _shapes_conditions():
    """What the "shapes" scenario must contain, from the oracle side alone (bytes 343 and 344..351 of the expected records, summary on): for every
    env i and d in (64, 128, 192) the (step, final ante, final round) of the endings the ENV made differ between i and i + d, and every block of 64
    envs holds such an ending above ante 1."""
    _, calls = prog._scenario("shapes", True)
    want = np.concatenate([c[1] for c in calls])
    N = prog.N
    game = (want[:, :, R_FLAGS] & progress_ref.END_GAME) != 0
    ante = want[:, :, 344:346].copy().view(np.int16)[:, :, 0]
    rnd = want[:, :, 346].view(np.int8)
    ends = [[(int(t), int(ante[t, i]), int(rnd[t, i])) for t in np.flatnonzero(game[:, i])] for i in range(N)]
    alike = [(i, i + d) for i in range(N) for d in (64, 128, 192) if i + d < N and ends[i] == ends[i + d]]
    assert not alike, f"envs a multiple of 64 apart end their episodes alike: {alike[:8]}"
    for k in range(0, N, 64):
        assert (game[:, k:k + 64] & (ante[:, k:k + 64] > 1)).any(), f"envs {k}..{min(k + 64, N) - 1}: no ending by the env above ante 1"
    return ends


def _idle_conditions():
    """The "idle" scenario ends every env stuck at step 300 (a terminal record and a reset-only request each), and the carry starts again from zeros."""
    _, calls = prog._scenario("idle", False)
    fl = calls[0][1][:, :, R_FLAGS]
    assert (fl[300] == progress_ref.END_STUCK).all() and not fl[:300].any() and not fl[301:].any()
    assert len(calls[0][2]) == prog.N and (calls[0][4][:, 0] == 19).all() and (calls[1][4][:, 0] == 43).all()


@pytest.mark.parametrize("scenario", ["shapes", "idle"])
@pytest.mark.parametrize("cards", [False, True], ids=["plain", "cards"])
@pytest.mark.parametrize("cfg,epw", SHAPES, ids=SHAPE_IDS)
def test_progress_every_shape_vs_oracle(monkeypatch, cfg, epw, cards, scenario):
    """bg_engine3_progress_kernel in every workgroup shape, with and without card states, through test_step_many_progress._run: the shaped-reward bits,
    every byte 0..351 of every record and terminal record, the bytes behind, the counters, the progression carry, the stats and env.check().
    "shapes" (summary on, three calls of 32 steps on shallow rings: the carries cross launches) is where the owner lane reads back what a service
    wave's reset block left of the final state -- s_fin[l], l = (wave * KS + slice) * 64 + lane -- and in shape 113 l == lane; "idle" has the stuck
    endings.  With card states nothing is injected: the oracle side is the same, and what runs is the wrapper plumbing of the CARDS variant."""
    if scenario == "shapes":
        _shapes_conditions()
        env, _, _, _ = prog._run("shapes", monkeypatch, summary=True, shallow=True, cfg=cfg, epw=epw, cards=cards)
        assert env.max_fused_steps * 3 <= 32
    else:
        _idle_conditions()
        env, _, _, _ = prog._run("idle", monkeypatch, cfg=cfg, epw=epw, cards=cards)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- B. ACT with card states
@pytest.mark.parametrize("cfg,epw", SHAPES, ids=SHAPE_IDS)
def test_step_many_rows_card_states_every_shape_vs_oracle(monkeypatch, cfg, epw):
    """The action mode with card states in every shape: the actions of the oracle's card-state rollout (333 envs, 26 card states per deck, two
    consumables per env and episode, jokers from all 150 ids, cap 6) through step_many(..., obs_buffers=RowBuffers) on a twin handle with the same
    injections, in two calls of 48: every record key, the reward bits, terminated, the action word and the stats against the ORACLE's arrays."""
    import torch
    from balatro_gym_amd.vec_env import RowBuffers
    _set_shape(monkeypatch, cfg, epw)
    inputs, (wobs, wr, wt, wa, wstats) = _card_state_rollout()
    n, K = CARD_N, CARD_T
    assert wstats["plays"] > 0 and wstats["episodes"] > 0
    env = _card_state_env(n, inputs)
    rb = RowBuffers(n, env.device, steps=K + 1, row_stride=384)
    for c in range(CARD_CHUNKS):
        sl = slice(c * K, (c + 1) * K)
        ctx = f"cfg {cfg} epw {epw} call {c}"
        poison_(rb.rows)
        env.step_many(torch.from_numpy(np.array(wa[sl])).to(env.device), obs_buffers=rb)
        _diff(f"{ctx}: action word [step, env]", rb.action[:K].cpu().numpy(), wa[sl])
        _diff(f"{ctx}: terminated [step, env]", rb.terminated[:K].cpu().numpy(), wt[sl])
        _diff(f"{ctx}: reward bits [step, env]", rb.reward[:K].contiguous().cpu().numpy().view(np.uint64), wr[sl].view(np.uint64))
        for k in OBS_KEYS:
            _diff(f"{ctx}: record key {k}", rb.tensors[k][:K].contiguous().cpu().numpy(), wobs[k][sl])
        got = rb.rows.cpu().numpy()
        assert not got[:K, :, R_FLAGS:].any(), f"{ctx}: record bytes 343..383"
        assert (got[K:] == POISON).all(), f"{ctx}: rows past the call's last step were written"
        st, want = env.stats(), _stats_of_steps(wr, wt, wstats, c * K, (c + 1) * K)
        for key in STAT_KEYS:
            assert st[key] == want[key], (ctx, key, st[key], want[key])
    env.close()


# ---------------------------------------------------------------------------------------------------------------- B. SAFE with card states
SAFE_K, SAFE_CALLS, SAFE_LIMITS = 48, 2, (3, 40)
# tarot / spectral ids whose use, with a card selected, always edits that card's state (oracle/balatro_oracle.c use_consumable): the enhancements
# (Magician, Empress, Hierophant, Lovers, Chariot, Justice, Devil, Tower), Aura's edition and the four seals
EDITING = frozenset((2, 4, 6, 7, 8, 12, 16, 17, 53, 54, 61, 63, 64))


@functools.lru_cache(maxsize=None)
def _safe_cards_scenario():
    """The card-state job's inputs under limits 3 / 40, two calls of 48 steps on the oracle wrapped by safe_ref.  Actions by env index i: i % 4 == 0
    the oracle's uniform policy; 1: runs of an out-of-range action (60) between policy steps; 2: runs of an in-range masked action; 3: the policy,
    except that an env holding a card-editing consumable selects a card and uses it.  On EVERY ending the oracle env is reset() and its jokers, card
    states and consumables are applied again, as the device's reset template does.  Returns the inputs, per call (actions [K, n], expected records
    [K, n, 352], terminal records, counters), and edits [K * calls, n]: a consumable use that edited a card's state.  Computed once, never modified."""
    from oracle import pyoracle as po
    (seeds, jokers, cons, cards), _ = _card_state_rollout()
    n, K = CARD_N, SAFE_K

    def apply(o, i):
        o.set_jokers(jokers[i])
        for (idx, e_, d_, s_) in cards[i]:
            o.set_card_state(idx, e_, d_, s_)
        o.set_consumables(cons[i])
    orc = [po.OracleEnv(seeds[i], scorer_jokers=True, max_ante=6) for i in range(n)]
    for i, o in enumerate(orc):
        apply(o, i)
    cur = [o.obs() for o in orc]
    cnt = [safe_ref.SafeCounters(*SAFE_LIMITS) for _ in range(n)]
    edits = np.zeros((K * SAFE_CALLS, n), bool)
    calls = []
    for c in range(SAFE_CALLS):
        acts = np.zeros((K, n), np.int32)
        want = np.zeros((K, n, 352), np.uint8)
        terminal = []
        for j in range(K):
            t = c * K + j
            rew, flags = np.zeros(n), np.zeros(n, np.uint8)
            for i, o in enumerate(orc):
                before = cur[i]
                run, gap = 1 + (i // 4) % 4, 1 + (i // 16) % 3
                in_run = (t + i) % (run + gap) < run
                a = o.policy_action(0, CARD_PSEED, CARD_INDEX0 + i, t)
                if i % 4 == 1 and in_run:
                    a = 60
                elif i % 4 == 2 and in_run:
                    a = _first_masked(before["action_mask"])
                elif i % 4 == 3 and int(before["phase"]) == 0:
                    held = [s for s in range(int(before["consumable_count"])) if int(before["consumables"][s]) in EDITING]
                    if held:
                        a = 10 + held[0] if np.asarray(before["selected_cards"]).any() else 2 + i % 8
                acts[j, i] = a
                ob, r, term, _, _ = o.step(int(a))
                edits[t, i] = (10 <= a < 15 and int(before["consumables"][a - 10]) in EDITING and bool(np.asarray(before["selected_cards"]).any())
                               and r != -1.0 and int(before["phase"]) == 0)
                rew[i], flags[i] = cnt[i].step(r, bool(term))
                if safe_ref.wrapper_ending(int(flags[i])):
                    terminal.append((j, i, _pack({k: np.asarray(ob[k])[None] for k in OBS_KEYS}, rew[i:i + 1], acts[j, i:i + 1], flags[i:i + 1])[0]))
                if flags[i]:   # SAME_STEP reset, whoever ended the episode: the record shows the new one
                    o.reset(); apply(o, i)
                    ob = o.obs()
                cur[i] = ob
            want[j] = _pack({k: np.stack([np.asarray(w[k]) for w in cur]) for k in OBS_KEYS}, rew, acts[j], flags)
        counters = np.array([[x.episode_steps, x.consecutive_invalid] for x in cnt], np.int32)
        for arr in (acts, want, counters):
            arr.setflags(write=False)
        calls.append((acts, want, tuple(terminal), counters))
    edits.setflags(write=False)
    return (seeds, jokers, cons, cards), tuple(calls), edits


def _safe_cards_conditions():
    """What the scenario must contain, from the oracle side alone: a kill, a step-limit ending, a game over, and in every block of 64 envs a
    consumable use that edits a card's state."""
    _, calls, edits = _safe_cards_scenario()
    fl = np.concatenate([w[:, :, R_FLAGS] for _, w, _, _ in calls])
    kills, limit_only, game = int((fl & 2 != 0).sum()), int((fl == 4).sum()), int((fl & 1 != 0).sum())
    per_block = [int(edits[:, k:k + 64].sum()) for k in range(0, CARD_N, 64)]
    print(f"kills {kills}, step-limit endings {limit_only}, game overs {game}, card-editing consumable uses per 64-env block {per_block}")
    assert kills >= 1 and limit_only >= 1 and game >= 1, (kills, limit_only, game)
    assert all(per_block), per_block
    # an edit is only seen when the env goes on in the same episode, and a reset only when it follows an edit: some edited env is reset later
    assert any(fl[t + 1:, i].any() for t, i in np.argwhere(edits)), "no reset behind an edit"


@pytest.mark.parametrize("cfg", [213, 413])
def test_safe_card_states_vs_wrapped_oracle(monkeypatch, cfg):
    """The SAFE instantiation where the CARDS path has something to edit, at 128 and 256 envs per workgroup: injected card states and consumables,
    card-editing consumable uses in every 64-env block, kills, step-limit endings and game overs; every record byte 0..351 and every terminal record
    of two 48-step calls on shallow rings against pyoracle.OracleEnv + safe_ref.SafeCounters.  The oracle side applies jokers, card states and
    consumables again behind every reset, the wrapper's included: the device's reset template restores injected card states."""
    import torch
    from balatro_gym_amd import EpisodeLimits
    from balatro_gym_amd.vec_env import RowBuffers
    _safe_cards_conditions()
    _shallow_rings(monkeypatch)
    _set_shape(monkeypatch, cfg, None)
    inputs, calls, _ = _safe_cards_scenario()
    n, K = CARD_N, SAFE_K
    env = _card_state_env(n, inputs)
    rb = RowBuffers(n, env.device, steps=K + 2, row_stride=384)
    lim = EpisodeLimits(n, env.device, *SAFE_LIMITS, steps=K, row_stride=384)
    assert lim.slots == safe_ref.terminal_slots(K, *SAFE_LIMITS)
    env.set_profiling(True)
    for gi, (acts, want, term, counters) in enumerate(calls):
        terminal = {(t, e): rec for t, e, rec in term}
        poison_(rb.rows); poison_(lim.terminal_rows); poison_(lim.terminal_step)
        env.step_many(torch.from_numpy(np.array(acts)).to(env.device), obs_buffers=rb, limits=lim)
        ctx = f"cfg {cfg} call {gi}"
        assert env.get_profile()["rollout_launches"] >= 3, ctx
        got = rb.rows.cpu().numpy()
        _diff(f"{ctx}: records [step, env, byte]", got[:K, :, :352], want)
        assert not got[:K, :, 352:].any(), f"{ctx}: bytes 352..383 of a whole-line record are not zero"
        assert (got[K:] == POISON).all(), f"{ctx}: rows past the call's last step were written"
        sets, ts, trows = _terminal_sets(lim, n)
        assert set(sets) == set(terminal), (ctx, sorted(set(sets) ^ set(terminal))[:8])
        for key, rec in terminal.items():
            _diff(f"{ctx}: terminal record of (step, env) {key}", sets[key], rec)
        assert not trows[ts >= 0][:, 352:].any(), f"{ctx}: bytes 352..383 of a terminal record"
        assert (trows[ts < 0] == POISON).all(), f"{ctx}: a terminal slot that was not used was written"
        cn = lim.counters.cpu().numpy()
        _diff(f"{ctx}: counters", cn[:, :2], counters)
        _diff(f"{ctx}: wrapper endings counted per env", cn[:, 2], np.bincount([e for _, e in terminal], minlength=n).astype(np.int32))
        st = env.stats()
        assert st["steps"] == n * K and st["episodes"] == int((want[:, :, R_TERM] != 0).sum()), (ctx, st)
    env.check()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- C. the observation checksum
HASH_T, HASH_CHUNKS, HASH_INDEX0, HASH_PSEED = 24, 2, 2, 5


@functools.lru_cache(maxsize=None)
def _plain_rollout():
    """The inputs of test_packed_record_rollout_every_engine (333 envs, five scorer jokers, cap 4, uniform policy) on the oracle, 2 x 24 steps."""
    from oracle.gen_golden import IMPLEMENTED
    n = CARD_N
    seeds = [88_000 + SEED_OFFSET + 3 * i for i in range(n)]
    jokers = [random.Random(2600 + i).sample(IMPLEMENTED, 5) for i in range(n)]
    return (seeds, jokers), _oracle_rollout(n, seeds, HASH_T * HASH_CHUNKS, 0, HASH_PSEED, True, 4, jokers, env_index0=HASH_INDEX0)


def _oracle_records(wobs, wr, wt, wa, T):
    """Steps 0 .. T - 1 of an _oracle_rollout run as the records a rollout writes, [T, n, 352] (byte 343 and the bytes behind it: zeros)."""
    rows = np.stack([_pack({k: wobs[k][t] for k in OBS_KEYS}, wr[t], wa[t], wt[t]) for t in range(T)])
    rows[:, :, R_FLAGS] = 0   # (_pack writes the limits' flags there; a rollout has none)
    return rows


@functools.lru_cache(maxsize=None)
def _hash_expected(cards):
    """(inputs, the checksum of the oracle's records, the oracle's other five stats) of the 2 x 24 steps."""
    if cards:   # the first 48 steps of the card-state job (the same policy seed and env_index0)
        assert (CARD_PSEED, CARD_INDEX0) == (13, HASH_INDEX0) and HASH_T * HASH_CHUNKS <= CARD_T * CARD_CHUNKS
        inputs, (wobs, wr, wt, wa, wstats) = _card_state_rollout()
    else:
        inputs, (wobs, wr, wt, wa, wstats) = _plain_rollout()
    T = HASH_T * HASH_CHUNKS
    rows = _oracle_records(wobs, wr, wt, wa, T)
    return inputs, hash_ref.obs_hash(rows, t0=0, env_index0=HASH_INDEX0), _stats_of_steps(wr, wt, wstats, 0, T)


HASH_CASES = [(3, cfg, epw, cards, "rows") for cards in (False, True) for cfg, epw in SHAPES] + [(1, None, None, False, "rows"), (3, None, None, False, "keys")]
HASH_IDS = [f"e3-{s}-{'cards' if cards else 'plain'}" for cards in (False, True) for s in SHAPE_IDS] + ["e1-plain", "per-key-plain"]


@pytest.mark.parametrize("engine,cfg,epw,cards,out", HASH_CASES, ids=HASH_IDS)
def test_obs_hash_vs_oracle_records(monkeypatch, engine, cfg, epw, cards, out):
    """stats()["obs_hash"] of rollout(policy | BG_POLICY_HASH_OBS, env_index0=2, t0=c * 24) over 2 x 24 steps of 333 envs against tests/hash_ref.py
    applied to records packed from the ORACLE's observations -- the device's own rows are not read -- so the checksum the 65 536-env tests compare
    with itself is known to cover every byte of every record, the step and the env index.  Engine 3 in every shape with and without card states
    (the HASH instantiations), engine 1 once, and once the per-key path (no record buffers: bg_engine.h).  The other five stats equal the oracle's."""
    from balatro_gym_amd.vec_env import RowBuffers
    monkeypatch.setenv("BG_ENGINE", str(engine))
    if cfg is not None:
        _set_shape(monkeypatch, cfg, epw)
    inputs, want_hash, want_stats = _hash_expected(cards)
    n = CARD_N
    if cards:
        env, pseed = _card_state_env(n, inputs), CARD_PSEED
    else:
        env, pseed = _vec(n, inputs[0], scorer_jokers=True, autoreset=True, max_ante=4), HASH_PSEED
        env.inject(jokers=inputs[1], apply_now=True)
    rb = RowBuffers(n, env.device, steps=HASH_T, row_stride=384) if out == "rows" else None
    for c in range(HASH_CHUNKS):
        env.rollout(HASH_T, policy=0 | 0x100, policy_seed=pseed, env_index0=HASH_INDEX0, t0=c * HASH_T, obs_buffers=rb, zero_stats=(c == 0))
    st = env.stats()
    env.close()
    for key in STAT_KEYS:
        assert st[key] == want_stats[key], (key, st[key], want_stats[key])
    assert st["obs_hash"] == want_hash, f"obs_hash {st['obs_hash']:#018x}, hash_ref over the oracle's records {want_hash:#018x}"
