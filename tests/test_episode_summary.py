"""GPU tests of the episode summary (bg_set_episode_summary; EpisodeLimits(..., summary=True)): the record of every ended step of
bg_step_many_rows_ex with limits carries the ended episode's final ante, round and score in bytes 344..351, whoever ended the episode, and every
other record has zeros there.  Everything is compared bit for bit against the CPU oracle wrapped by tests/safe_ref.py; the expected summary is
taken from the observation the oracle's step returned BEFORE the test resets the env."""
import functools
import random

import numpy as np
import pytest

from tests import safe_ref as ref
from tests.helpers import OBS_KEYS, POISON, poison_
from tests.test_gpu_parity import SEED_OFFSET, _oracle_envs, _vec
from tests.test_step_many_safe import R_FLAGS, R_TERM, _diff, _pack, _shallow_rings, _terminal_sets

pytestmark = pytest.mark.gpu

R_END_ANTE, R_END_ROUND, R_END_CHIPS = 344, 346, 348   # BG_ROW_END_ANTE / BG_ROW_END_ROUND / BG_ROW_END_CHIPS
SC_N, SC_K, SC_CALLS, SC_LIMITS, SC_CAP = 200, 48, 3, (3, 60), 2


def _summary(ob):
    """Bytes 344..351 of the record of a step that ended an episode in the state `ob` shows."""
    out = np.zeros(8, np.uint8)
    out[0:2] = np.array([int(ob["ante"])], np.int16).view(np.uint8)
    out[2:3] = np.array([int(ob["round"])], np.int8).view(np.uint8)
    out[4:8] = np.array([min(max(int(ob["chips_scored"]), 0), 2 ** 32 - 1)], np.uint32).view(np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def _scenario():
    """200 envs (a partial last workgroup), cap 2, limits 3 / 60, scorer jokers, three calls of 48 steps on the oracle wrapped by safe_ref.  Actions
    by env index i: i % 4 == 0 the oracle's policy 2; 1: runs of an out-of-range action (60) between steps of policy 2, the run lengths 1..4 and the
    gaps 1..3 by i, so that runs of three end in a kill and runs of four send an invalid action directly behind it; 2: policy 1; 3: policy 0.
    Returns, per call: actions [K, n], the expected records [K, n, 352] with bytes 344..351, the terminal records [(t, e, record)] and the counters
    behind the call; and `stale`, the (t, e) of all 144 steps at which an invalid action directly follows an ended step.  Computed once, never modified."""
    from oracle.gen_golden import IMPLEMENTED
    n, K = SC_N, SC_K
    seeds = [752_000 + SEED_OFFSET + 7 * i for i in range(n)]
    jokers = [random.Random(7300 + i).sample(IMPLEMENTED, i % 6) for i in range(n)]
    orc = _oracle_envs(n, seeds, True, SC_CAP, jokers)
    cnt = [ref.SafeCounters(*SC_LIMITS) for _ in range(n)]
    ended_before = np.zeros(n, bool)
    calls, stale = [], []
    for c in range(SC_CALLS):
        acts = np.zeros((K, n), np.int32)
        want = np.zeros((K, n, 352), np.uint8)
        terminal = []
        for j in range(K):
            t = c * K + j
            rew, flags, obs, summ = np.zeros(n), np.zeros(n, np.uint8), [], np.zeros((n, 8), np.uint8)
            for i, o in enumerate(orc):
                run, gap = 1 + (i // 4) % 4, 1 + (i // 16) % 3
                if i % 4 == 1 and (t + i) % (run + gap) < run:
                    a = 60
                else:
                    a = o.policy_action((2, 2, 1, 0)[i % 4], 23, i, t)
                acts[j, i] = a
                ob, r, term, _, _ = o.step(int(a))
                rew[i], flags[i] = cnt[i].step(r, bool(term))
                if ended_before[i] and r == -1.0 and not term:
                    stale.append((t, i))
                if ref.wrapper_ending(int(flags[i])):
                    terminal.append((j, i, _pack({k: np.asarray(ob[k])[None] for k in OBS_KEYS}, rew[i:i + 1], acts[j, i:i + 1], flags[i:i + 1])[0]))
                if flags[i]:   # SAME_STEP reset, whoever ended the episode: the record shows the new one and the summary the old one's end
                    summ[i] = _summary(ob)
                    o.reset(); o.set_jokers(jokers[i])
                ended_before[i] = flags[i] != 0
                obs.append(o.obs())
            want[j] = _pack({k: np.stack([np.asarray(w[k]) for w in obs]) for k in OBS_KEYS}, rew, acts[j], flags)
            want[j, :, R_END_ANTE:R_END_ANTE + 8] = summ
        counters = np.array([[x.episode_steps, x.consecutive_invalid] for x in cnt], np.int32)
        for a in (acts, want, counters):
            a.setflags(write=False)
        calls.append((acts, want, tuple(terminal), counters))
    return seeds, jokers, tuple(calls), tuple(stale)


def _scenario_conditions():
    """What the scenario must contain, from the oracle side alone."""
    _, _, calls, stale = _scenario()
    want = np.concatenate([w for _, w, _, _ in calls])
    fl = want[:, :, R_FLAGS]
    ante = want[:, :, R_END_ANTE:R_END_ANTE + 2].copy().view(np.int16)[:, :, 0]
    game, cap, limit_only, kills = int((fl & 1 != 0).sum()), int(((fl & 1 != 0) & (ante == SC_CAP + 1)).sum()), fl == 4, int((fl & 2 != 0).sum())
    print(f"game overs {game}, of which at the cap {cap}; step-limit endings {int(limit_only.sum())} at antes {sorted(set(ante[limit_only].tolist()))}; "
          f"kills {kills}; invalid actions directly behind an ending {len(stale)}")
    assert game - cap >= 20 and cap >= 5, (game, cap)
    assert int(limit_only.sum()) >= 20 and len(set(ante[limit_only].tolist())) >= 2
    assert kills >= 10 and len(stale) >= 5
    # the summary sits on the ended records and nowhere else, and a summary's ante is at least 1
    assert (ante[fl != 0] >= 1).all() and not want[:, :, R_END_ANTE:R_END_ANTE + 8][fl == 0].any() and not want[:, :, R_END_ROUND + 1].any()
    for t, e in stale:   # the stale-image case: the record behind an ending is a patched image, and it must not carry the summary along
        assert fl[t - 1, e] != 0 and (fl[t, e] != 0 or not want[t, e, R_END_ANTE:R_END_ANTE + 8].any())


def _run_scenario(monkeypatch, cfg=None, cards=False, one_call=False, summary=True):
    """The scenario on the GPU, every byte checked (with summary=False: against the expected records with bytes 344..351 zeroed).  Returns the
    records of every call."""
    import torch
    from balatro_gym_amd import EpisodeLimits
    from balatro_gym_amd.vec_env import RowBuffers
    _shallow_rings(monkeypatch)
    if cfg is not None:
        monkeypatch.setenv("BG_E3_CFG", str(cfg))
    seeds, jokers, calls, _ = _scenario()
    n, K = SC_N, SC_K
    env = _vec(n, seeds, scorer_jokers=True, autoreset=True, max_ante=SC_CAP, card_states=cards)
    env.inject(jokers=jokers, apply_now=True)
    KK = K * len(calls) if one_call else K
    rb = RowBuffers(n, env.device, steps=KK + 2, row_stride=384)
    lim = EpisodeLimits(n, env.device, *SC_LIMITS, steps=KK, row_stride=384, summary=summary)
    env.set_profiling(True)
    groups = [calls] if one_call else [[c] for c in calls]
    outs = []
    for gi, group in enumerate(groups):
        acts = np.concatenate([c[0] for c in group])
        want = np.concatenate([c[1] for c in group])
        if not summary:
            want = want.copy()
            want[:, :, R_END_ANTE:R_END_ANTE + 8] = 0
        terminal = {(t + K * ci, e): rec for ci, c in enumerate(group) for t, e, rec in c[2]}
        poison_(rb.rows); poison_(lim.terminal_rows); poison_(lim.terminal_step)
        env.step_many(torch.from_numpy(acts).to(env.device), obs_buffers=rb, limits=lim)
        ctx = f"cfg {cfg} cards {cards} summary {summary} call {gi}"
        assert env.get_profile()["rollout_launches"] >= 3, ctx
        got = rb.rows.cpu().numpy()
        _diff(f"{ctx}: records [step, env, byte]", got[:KK, :, :352], want)
        assert not got[:KK, :, 352:].any(), f"{ctx}: bytes 352..383 of a whole-line record are not zero"
        assert (got[KK:] == POISON).all(), f"{ctx}: rows past the call's last step were written"
        # the strided views are those bytes
        _diff(f"{ctx}: rb.end_ante", rb.end_ante[:KK].cpu().numpy(), want[:, :, R_END_ANTE:R_END_ANTE + 2].copy().view(np.int16)[:, :, 0])
        _diff(f"{ctx}: rb.end_round", rb.end_round[:KK].cpu().numpy(), want[:, :, R_END_ROUND].view(np.int8))
        _diff(f"{ctx}: rb.end_chips", rb.end_chips[:KK].cpu().numpy(), want[:, :, R_END_CHIPS:R_END_CHIPS + 4].copy().view(np.uint32)[:, :, 0])
        # terminal records are written before the reset: their observation is the final state and bytes 344..351 stay zero
        sets, ts, trows = _terminal_sets(lim, n)
        assert set(sets) == set(terminal), (ctx, sorted(set(sets) ^ set(terminal))[:8])
        for key, rec in terminal.items():
            assert not rec[R_END_ANTE:].any()
            _diff(f"{ctx}: terminal record of (step, env) {key}", sets[key], rec)
        assert (trows[ts < 0] == POISON).all(), f"{ctx}: a terminal slot that was not used was written"
        _diff(f"{ctx}: counters", lim.counters.cpu().numpy()[:, :2], group[-1][3])
        st = env.stats()
        assert st["steps"] == n * KK and st["episodes"] == int((want[:, :, R_TERM] != 0).sum()), (ctx, st)
        outs.append(got[:KK, :, :352].copy())
    env.check()
    return env, rb, lim, outs


@pytest.mark.parametrize("cfg,cards", [(None, False), (213, False), (413, False), (None, True), (213, True), (413, True)],
                         ids=["113", "213", "413", "113-cards", "213-cards", "413-cards"])
def test_every_byte_vs_wrapped_oracle(monkeypatch, cfg, cards):
    """Every record byte 0..351 of three 48-step calls -- the summary's bytes 344..351 from the oracle's observation before the reset -- and every
    terminal record, under all three workgroup shapes, each also on a handle with card states."""
    _scenario_conditions()
    env, _, _, _ = _run_scenario(monkeypatch, cfg, cards)
    env.close()


def test_one_call_equals_three(monkeypatch):
    """The same 144 steps as ONE call on a twin handle: the same record bytes."""
    _scenario_conditions()
    env, _, _, _ = _run_scenario(monkeypatch, one_call=True)
    env.close()


def test_switch_off_twin_and_null_limits(monkeypatch):
    """A twin handle with the switch off gives the same bytes except 344..351, which are zero there (both held to the oracle).  Then, on the handle
    with the switch ON: limits = NULL is refused with its text and nothing is written, bg_step_many_rows is untouched by the switch (zeros in
    344..351 on ended records too), bg_set_episode_summary refuses values other than 0 / 1, and switching it off again lets limits = NULL through."""
    import ctypes as C
    import torch
    _scenario_conditions()
    off_env, _, _, off = _run_scenario(monkeypatch, summary=False)
    off_env.close()
    env, rb, lim, on = _run_scenario(monkeypatch)
    differ = 0
    for a, b in zip(on, off):
        _diff("switch on against switch off, bytes 0..343", a[:, :, :R_END_ANTE], b[:, :, :R_END_ANTE])
        assert not b[:, :, R_END_ANTE:].any()
        differ += int((a[:, :, R_END_ANTE:] != 0).any(axis=2).sum())
    assert differ >= 100   # (the conditions above: every ended record carries an ante >= 1)
    L, n, K = env._L, SC_N, SC_K
    acts = torch.from_numpy(np.array(_scenario()[2][0][0])).to(env.device)

    def ex(limits):
        return L.bg_step_many_rows_ex(env._h, K, C.c_void_p(acts.data_ptr()), C.c_void_p(rb.rows.data_ptr()), C.c_uint64(384), 1, limits,
                                      C.c_void_p(env._stats.data_ptr()), env._stream())
    poison_(rb.rows)
    assert ex(None) == -1
    err = L.bg_last_error(env._h).decode()
    assert err.startswith("bg_step_many_rows_ex: ") and "the episode summary needs limits" in err, err
    torch.cuda.synchronize()
    assert bool((rb.rows == POISON).all()), "a refused call wrote records"
    env.step_many(acts, obs_buffers=rb)   # bg_step_many_rows: the switch (still on) does not reach it
    plain = rb.rows.cpu().numpy()[:K]
    assert plain[:, :, R_TERM].any() and not plain[:, :, R_FLAGS:352].any()
    for bad in (2, -1):
        assert L.bg_set_episode_summary(env._h, bad) == -1 and "0 or 1" in L.bg_last_error(env._h).decode()
    assert L.bg_set_episode_summary(env._h, 0) == 0 and ex(None) == 0
    again = rb.rows.cpu().numpy()[:K]
    assert again[:, :, R_TERM].any() and not again[:, :, R_FLAGS:352].any()
    env.check()
    env.close()
