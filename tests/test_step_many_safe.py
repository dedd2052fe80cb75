"""GPU tests of bg_step_many_rows_ex (BalatroVecEnv.step_many(..., limits=EpisodeLimits)): SafeBalatroEnv's episode limits inside the packed-record
launch (bg_engine3.h's SAFE instantiation).  Everything is compared bit-exactly -- against the reference's own wrapper output (sb3_fixed.npz), against
the CPU oracle wrapped by tests/safe_ref.py, against the same steps in one call, against bg_step_many_rows, and against BalatroSB3VecEnv."""
import functools
import random

import numpy as np
import pytest

from tests import safe_ref as ref
from tests.helpers import OBS_KEYS, POISON, poison_
from tests.test_gpu_parity import SEED_OFFSET, _oracle_envs, _row_views, _vec

pytestmark = pytest.mark.gpu

R_REWARD, R_ACTION, R_TERM, R_FLAGS = 136, 172, 342, 343   # BG_ROW_REWARD / BG_ROW_ACTION / BG_ROW_TERMINATED / BG_ROW_END_FLAGS
_NPDT = {"int8": np.int8, "int16": np.int16, "int32": np.int32, "int64": np.int64, "float32": np.float32, "float64": np.float64}


def _shallow_rings(monkeypatch):
    """Look-ahead rings of a few steps (as tests/test_step_many_rows.py sets them): a 48-step call is many launches with refills between them."""
    monkeypatch.setenv("BG_KG", "4"); monkeypatch.setenv("BG_KS", "5"); monkeypatch.setenv("BG_KD", "4")


def _pack(obs, reward, action, flags):
    """Records [n, 352] from stacked per-key observations, float64 rewards, int32 actions and uint8 BG_END_* flags (terminated = flags != 0)."""
    from balatro_gym_amd import _native as nat
    n = len(reward)
    r = np.zeros((n, 352), np.uint8)
    for k in OBS_KEYS:
        dt, _ = nat.OBS_SPEC[k]
        v = np.ascontiguousarray(np.asarray(obs[k]).astype(_NPDT[dt]).reshape(n, -1)).view(np.uint8)
        r[:, nat.ROW_OFFSETS[k]:nat.ROW_OFFSETS[k] + v.shape[1]] = v
    r[:, R_REWARD:R_REWARD + 8] = np.ascontiguousarray(reward, np.float64).reshape(n, 1).view(np.uint8)
    r[:, R_ACTION:R_ACTION + 4] = np.ascontiguousarray(action, np.int32).reshape(n, 1).view(np.uint8)
    r[:, R_TERM] = np.asarray(flags) != 0
    r[:, R_FLAGS] = flags
    return r


def _diff(ctx, got, want):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)[0]
        raise AssertionError(f"{ctx}: first difference at {tuple(bad)}: got {got[tuple(bad)]} want {want[tuple(bad)]} ({int((got != want).sum())} in all)")


# ---------------------------------------------------------------------------------------------------------------- the oracle scenario
SC_N, SC_K, SC_CALLS, SC_LIMITS = 333, 48, 3, (3, 17)


def _first_masked(mask):
    """An in-range action the mask forbids."""
    return int(np.flatnonzero(np.asarray(mask) == 0)[0])


@functools.lru_cache(maxsize=None)
def _scenario():
    """333 envs (a partial last workgroup), limits 3 / 17, scorer jokers, three calls of 48 steps on the oracle wrapped by safe_ref.  Actions by env
    index i: i % 4 == 0 the oracle's uniform policy; 1: runs of an out-of-range action (60) between policy steps; 2: runs of an in-range masked
    action; 3: toggles only (behind the blind selection a fresh episode needs).  The run lengths 1..4 and the gaps between them depend on i, so
    that some runs reach the invalid-action limit and others end below it; every 16th env sends its run where it ends on the episode's 17th step.
    Returns, per call: actions [K, n], the expected records [K, n, 352], the expected terminal records [(t, e, record)], and the counters behind
    the call; computed once, never modified."""
    from oracle.gen_golden import IMPLEMENTED
    n, K = SC_N, SC_K
    seeds = [752_000 + SEED_OFFSET + 7 * i for i in range(n)]
    jokers = [random.Random(7300 + i).sample(IMPLEMENTED, i % 6) for i in range(n)]
    orc = _oracle_envs(n, seeds, True, 4, jokers)
    cnt = [ref.SafeCounters(*SC_LIMITS) for _ in range(n)]
    calls = []
    for c in range(SC_CALLS):
        acts = np.zeros((K, n), np.int32)
        want = np.zeros((K, n, 352), np.uint8)
        terminal = []
        for j in range(K):
            t = c * K + j
            rew, flags, obs = np.zeros(n), np.zeros(n, np.uint8), []
            for i, o in enumerate(orc):
                run, gap = 1 + (i // 4) % 4, 1 + (i // 16) % 3
                in_run = (t + i) % (run + gap) < run
                if i % 16 in (5, 6):   # the run that ends on the step limit's step
                    in_run = cnt[i].episode_steps >= SC_LIMITS[1] - SC_LIMITS[0]
                if i % 4 == 0:
                    a = o.policy_action(0, 23, i, t)
                elif i % 4 == 1:
                    a = 60 if in_run else o.policy_action(0, 23, i, t)
                elif i % 4 == 2:
                    a = _first_masked(o.obs()["action_mask"]) if in_run else o.policy_action(0, 23, i, t)
                else:
                    a = 45 if int(o.obs()["phase"]) == 2 else 2 + (t + i) % 8
                acts[j, i] = a
                ob, r, term, _, _ = o.step(int(a))
                rew[i], flags[i] = cnt[i].step(r, bool(term))
                if ref.wrapper_ending(int(flags[i])):
                    terminal.append((j, i, _pack({k: np.asarray(ob[k])[None] for k in OBS_KEYS}, rew[i:i + 1], acts[j, i:i + 1], flags[i:i + 1])[0]))
                if flags[i]:   # SAME_STEP reset, whoever ended the episode: the record shows the new one
                    o.reset(); o.set_jokers(jokers[i])
                obs.append(o.obs())
            want[j] = _pack({k: np.stack([np.asarray(w[k]) for w in obs]) for k in OBS_KEYS}, rew, acts[j], flags)
        counters = np.array([[x.episode_steps, x.consecutive_invalid] for x in cnt], np.int32)
        for a in (acts, want, counters):
            a.setflags(write=False)
        calls.append((acts, want, tuple(terminal), counters))
    return seeds, jokers, tuple(calls)


def _scenario_conditions():
    """What the scenario must contain, from the oracle side alone."""
    _, _, calls = _scenario()
    fl = np.concatenate([w[:, :, R_FLAGS] for _, w, _, _ in calls])
    kills, limit_only, game = int((fl & 2 != 0).sum()), int((fl == 4).sum()), int((fl & 1 != 0).sum())
    assert kills >= 20 and limit_only >= 20 and game >= 5, (kills, limit_only, game)
    assert int((fl == 6).sum()) >= 1, "no kill on the step limit's step"
    two = first = last = False
    for _, _, terminal, _ in calls:
        per_env = {}
        for t, e, _ in terminal:
            per_env[e] = per_env.get(e, 0) + 1
            first, last = first or t == 0, last or t == SC_K - 1
        two = two or max(per_env.values()) >= 2
    assert two and first and last, (two, first, last)
    return kills, limit_only, game


def _terminal_sets(lim, n):
    """{(t, e): record bytes 0..351} of the last call, and the slots check: env e's endings fill slots 0, 1, ... in step order, the rest is -1."""
    ts = lim.terminal_step.cpu().numpy()
    rows = lim.terminal_rows.cpu().numpy()
    out = {}
    for e in range(n):
        used = ts[:, e] >= 0
        k = int(used.sum())
        assert used[:k].all() and not used[k:].any(), f"env {e}: slots are not filled from 0 up"
        assert (np.diff(ts[:k, e]) > 0).all(), f"env {e}: slots are not in step order"
        for j in range(k):
            out[(int(ts[j, e]), e)] = rows[j, e, :352].copy()
    return out, ts, rows


def _run_scenario(monkeypatch, cfg=None, cards=False, one_call=False):
    import torch
    from balatro_gym_amd import EpisodeLimits
    from balatro_gym_amd.vec_env import RowBuffers
    _shallow_rings(monkeypatch)
    if cfg is not None:
        monkeypatch.setenv("BG_E3_CFG", str(cfg))
    seeds, jokers, calls = _scenario()
    n, K = SC_N, SC_K
    env = _vec(n, seeds, scorer_jokers=True, autoreset=True, max_ante=4, card_states=cards)
    env.inject(jokers=jokers, apply_now=True)
    KK = K * len(calls) if one_call else K
    rb = RowBuffers(n, env.device, steps=KK + 2, row_stride=384)
    lim = EpisodeLimits(n, env.device, *SC_LIMITS, steps=KK, row_stride=384)
    assert lim.slots == KK // 3 + 1
    assert env.max_fused_steps * 3 <= K
    env.set_profiling(True)
    groups = [calls] if one_call else [[c] for c in calls]
    for gi, group in enumerate(groups):
        acts = np.concatenate([c[0] for c in group])
        want = np.concatenate([c[1] for c in group])
        terminal = {(t + K * ci, e): rec for ci, c in enumerate(group) for t, e, rec in c[2]}
        poison_(rb.rows); poison_(lim.terminal_rows); poison_(lim.terminal_step)
        env.step_many(torch.from_numpy(acts).to(env.device), obs_buffers=rb, limits=lim)
        ctx = f"cfg {cfg} cards {cards} call {gi}"
        assert env.get_profile()["rollout_launches"] >= 3, ctx
        got = rb.rows.cpu().numpy()
        _diff(f"{ctx}: records [step, env, byte]", got[:KK, :, :352], want)
        assert not got[:KK, :, 352:].any(), f"{ctx}: bytes 352..383 of a whole-line record are not zero"
        assert (got[KK:] == POISON).all(), f"{ctx}: rows past the call's last step were written"
        sets, ts, trows = _terminal_sets(lim, n)
        assert set(sets) == set(terminal), (ctx, sorted(set(sets) ^ set(terminal))[:8])
        for key, rec in terminal.items():
            _diff(f"{ctx}: terminal record of (step, env) {key}", sets[key], rec)
        assert not trows[ts >= 0][:, 352:].any(), f"{ctx}: bytes 352..383 of a terminal record"
        assert (trows[ts < 0] == POISON).all(), f"{ctx}: a terminal slot that was not used was written"
        # EpisodeLimits.terminal(): ascending t * n + e, the records in that order
        index, recs = lim.terminal()
        keys = sorted(terminal)
        assert index.cpu().tolist() == [t * n + e for t, e in keys], ctx
        if keys:
            _diff(f"{ctx}: EpisodeLimits.terminal()", recs.cpu().numpy()[:, :352], np.stack([terminal[k] for k in keys]))
        cn = lim.counters.cpu().numpy()
        _diff(f"{ctx}: counters", cn[:, :2], group[-1][3])
        per_env = np.bincount([e for _, e in keys], minlength=n)
        _diff(f"{ctx}: wrapper endings counted per env", cn[:, 2], per_env.astype(np.int32))
        assert not cn[:, 3].any()
        st = env.stats()
        assert st["steps"] == n * KK and st["episodes"] == int((want[:, :, R_TERM] != 0).sum()), (ctx, st)
    env.check()
    return env, rb, lim


@pytest.mark.parametrize("cfg,cards", [(None, False), (213, False), (413, False), (None, True), (213, True), (413, True)],
                         ids=["113", "213", "413", "113-cards", "213-cards", "413-cards"])
def test_every_byte_vs_wrapped_oracle(monkeypatch, cfg, cards):
    """Every record byte 0..351 of three 48-step calls and every terminal record against pyoracle.OracleEnv + safe_ref (on a wrapper ending the
    oracle env is reset() and its jokers re-applied), under all three workgroup shapes, each also on a handle with card states (none injected:
    tests/test_engine3_instantiations.py has the case with injected ones); terminal slots that were not used keep their byte pattern, the counters
    and stats agree, env.check() is clean."""
    kills, limit_only, game = _scenario_conditions()
    env, _, _ = _run_scenario(monkeypatch, cfg, cards)
    env.close()
    assert kills and limit_only and game


def test_one_call_equals_three(monkeypatch):
    """The same 144 steps as ONE call on a twin handle: the same record bytes and final counters (both held to the oracle), the terminal records
    the same set, at slots counted per call."""
    _scenario_conditions()
    env, _, _ = _run_scenario(monkeypatch, one_call=True)
    env.close()


# ---------------------------------------------------------------------------------------------------------------- the reference's own wrapper
def test_golden_replay(monkeypatch):
    """sb3_fixed.npz (the reference's SafeBalatroEnv(BalatroEnvFixed(seed + rank), 5, 40), 24 envs x 120 steps) as calls of 48, 48 and 24 steps on
    shallow rings: the counters cross launch and call boundaries.  Every step: float32(reward) bit for bit, byte 342 = dones, byte 343 = the
    golden's three flags, every produced key = obs_*; every wrapper ending: the terminal record's keys = term_* and terminal_step names the step."""
    import torch
    from balatro_gym_amd import EpisodeLimits
    from balatro_gym_amd.vec_env import RowBuffers
    _shallow_rings(monkeypatch)
    g = ref.load_golden()
    _, env_term, want_flags = ref.golden_inner(g)
    S, T = g["actions"].shape
    mi, ms = int(g["max_invalid_actions"]), int(g["max_episode_steps"])
    env = _vec(S, [int(g["seed0"]) + r for r in range(S)], autoreset=True)
    env.reset()   # the VecEnv's reset() behind the constructor's: the golden's first episode is the env's second
    lim = EpisodeLimits(S, env.device, mi, ms, steps=48, row_stride=352)
    lim.reset()
    rb = RowBuffers(S, env.device, steps=48, row_stride=352)
    assert lim.slots == 48 // 5 + 1
    env.set_profiling(True)
    t0 = ends = 0
    for K in (48, 48, 24):
        acts = np.ascontiguousarray(g["actions"][:, t0:t0 + K].T)
        poison_(rb.rows); poison_(lim.terminal_rows); poison_(lim.terminal_step)
        env.step_many(torch.from_numpy(acts).to(env.device), obs_buffers=rb, limits=lim)
        assert env.get_profile()["rollout_launches"] >= 2
        got = rb.rows.cpu()
        gn = got.numpy()
        rew = gn[:K, :, R_REWARD:R_REWARD + 8].copy().view(np.float64)[:, :, 0].astype(np.float32)
        _diff(f"steps {t0}..: float32(reward) bits [step, env]", rew.view(np.uint32), g["rewards"][:, t0:t0 + K].T.view(np.uint32))
        _diff(f"steps {t0}..: byte 342 against dones", gn[:K, :, R_TERM], g["dones"][:, t0:t0 + K].T)
        _diff(f"steps {t0}..: byte 343 against the golden's flags", gn[:K, :, R_FLAGS], want_flags[:, t0:t0 + K].T)
        _diff(f"steps {t0}..: action word", gn[:K, :, R_ACTION:R_ACTION + 4].copy().view(np.int32)[:, :, 0], acts)
        assert not gn[:K, :, 344:].any()
        assert (gn[K:] == POISON).all()
        for j in range(K):
            v = _row_views(got[j])
            for k in OBS_KEYS:
                w = g["obs_" + k][:, t0 + j]
                assert np.array_equal(v[k].reshape(S, -1).astype(np.int64 if w.dtype.kind == "i" else w.dtype), w.reshape(S, -1)), (t0 + j, k)
        sets, ts, trows = _terminal_sets(lim, S)
        wend = (want_flags[:, t0:t0 + K] != 0) & ~env_term[:, t0:t0 + K]
        assert set(sets) == {(int(t), int(e)) for e, t in np.argwhere(wend)}
        assert (trows[ts < 0] == POISON).all(), "a terminal slot that was not used was written"
        for (t, e), rec in sets.items():
            ends += 1
            assert rec[R_TERM] == 1 and rec[R_FLAGS] == want_flags[e, t0 + t] and not rec[344:].any()
            assert rec[R_REWARD:R_REWARD + 8].view(np.float64)[0].astype(np.float32) == g["rewards"][e, t0 + t]
            assert rec[R_ACTION:R_ACTION + 4].view(np.int32)[0] == g["actions"][e, t0 + t]
            v = _row_views(torch.from_numpy(rec[None].copy()))
            for k in OBS_KEYS:
                w = g["term_" + k][e, t0 + t]
                assert np.array_equal(v[k].reshape(-1).astype(np.int64 if w.dtype.kind == "i" else w.dtype), w.reshape(-1)), (t0 + t, e, k)
        t0 += K
    assert ends == 144 + 30   # the fixture's kills and time-limit-only endings (tests/test_step_many_safe_host.py counts them)
    env.check()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- no existing behaviour changes
def test_limits_that_never_fire_and_null_limits(monkeypatch):
    """Limits of 2**30: the records are byte-identical to bg_step_many_rows on a twin handle except byte 343, which is 1 (BG_END_GAME) exactly where
    the game set byte 342; no terminal slot is used.  limits = NULL through bg_step_many_rows_ex: identical down to byte 343 = 0."""
    import ctypes as C
    import torch
    from balatro_gym_amd import EpisodeLimits
    from balatro_gym_amd.vec_env import RowBuffers
    _shallow_rings(monkeypatch)
    seeds, jokers, calls = _scenario()
    n, K = SC_N, SC_K
    acts = torch.from_numpy(np.array(calls[0][0])).to("cuda:0")
    outs = []
    for mode in ("plain", "never", "null"):
        env = _vec(n, seeds, scorer_jokers=True, autoreset=True, max_ante=4)
        env.inject(jokers=jokers, apply_now=True)
        rb = RowBuffers(n, env.device, steps=K, row_stride=384)
        poison_(rb.rows)
        for rep in range(2):   # (two calls: episodes of the random-policy envs end inside)
            if mode == "plain":
                env.step_many(acts, obs_buffers=rb)
            elif mode == "never":
                lim = EpisodeLimits(n, env.device, 2 ** 30, 2 ** 30, steps=K) if rep == 0 else lim
                env.step_many(acts, obs_buffers=rb, limits=lim)
                assert bool((lim.terminal_step == -1).all()) and lim.terminal()[0].numel() == 0
                assert lim.counters[:, 0].max() <= K * (rep + 1) and not lim.counters[:, 2:].any()
            else:
                rc = env._L.bg_step_many_rows_ex(env._h, K, C.c_void_p(acts.data_ptr()), C.c_void_p(rb.rows.data_ptr()), C.c_uint64(384), 1, None,
                                                 C.c_void_p(env._stats.data_ptr()), env._stream())
                assert rc == 0
            outs.append(rb.rows.cpu().numpy().copy())
        env.check()
        env.close()
    for rep in range(2):
        plain, never, null = outs[rep], outs[2 + rep], outs[4 + rep]
        _diff(f"call {rep}: limits = NULL against bg_step_many_rows", null, plain)
        assert not plain[:, :, R_FLAGS].any()
        _diff(f"call {rep}: byte 343 under limits that never fire", never[:, :, R_FLAGS], plain[:, :, R_TERM])
        never[:, :, R_FLAGS] = 0
        _diff(f"call {rep}: limits that never fire against bg_step_many_rows", never, plain)
    assert outs[0][:, :, R_TERM].any() or outs[1][:, :, R_TERM].any(), "no game over in the run"


# ---------------------------------------------------------------------------------------------------------------- against the one-step adapter
def test_against_the_one_step_adapter():
    """BalatroSB3VecEnv(64, seed=300, 5, 40, as_torch=True, features="produced") stepped 45 times with test_sb3_adapter_conventions' action rule
    (env 0 sends 59, the others toggle card 0 or take the first valid action); the same actions through ONE step_many(..., limits=) call on a
    second env: rewards and dones equal, encode_rows of every record = the adapter's matrix, the terminal records = its terminal_observations."""
    import torch
    from balatro_gym_amd import EpisodeLimits, _native as nat, encode_rows
    from balatro_gym_amd.sb3_adapter import BalatroSB3VecEnv
    from balatro_gym_amd.vec_env import RowBuffers
    n, T = 64, 45
    venv = BalatroSB3VecEnv(n, seed=300, max_invalid_actions=5, max_episode_steps=40, as_torch=True, features="produced")
    obs = venv.reset()
    c0 = [c for name, c, _ in nat.ENC_COLUMNS[nat.ENC_PRODUCED] if name == "action_mask"][0]
    acts, mats, rews, dones, terms = [], [], [], [], {}
    for t in range(T):
        mask = obs[:, c0:c0 + 60].cpu().numpy() != 0
        a = np.array([2 if mask[i, 2] else int(np.flatnonzero(mask[i])[0]) for i in range(n)], np.int32)
        a[0] = 59
        obs, rew, done, infos = venv.step(a)
        acts.append(a); mats.append(obs.cpu().numpy()); rews.append(rew.cpu().numpy()); dones.append(done.cpu().numpy())
        for i, inf in enumerate(infos):
            if "terminal_observation" in inf:
                terms[(t, i)] = np.asarray(inf["terminal_observation"])
    venv.close()
    env = _vec(n, [300 + r for r in range(n)], autoreset=True)
    env.reset()   # (venv.reset() above: the second reset of these seeds)
    rb = RowBuffers(n, env.device, steps=T, row_stride=384)
    lim = EpisodeLimits(n, env.device, 5, 40, steps=T)
    env.step_many(torch.from_numpy(np.stack(acts)).to(env.device), obs_buffers=rb, limits=lim)
    env.check()
    _diff("rewards [step, env] (float32 bits)", rb.reward.cpu().numpy().astype(np.float32).view(np.uint32), np.stack(rews).view(np.uint32))
    _diff("dones [step, env]", rb.terminated.cpu().numpy() != 0, np.stack(dones))
    _diff("encode_rows of the records against the adapter's matrices", encode_rows(rb.rows, "produced").cpu().numpy().view(np.uint32), np.stack(mats).view(np.uint32))
    index, recs = lim.terminal()
    assert index.cpu().tolist() == [t * n + e for t, e in sorted(terms)] and len(terms) >= 9 + 63
    _diff("terminal records against the adapter's terminal_observations", encode_rows(recs, "produced").cpu().numpy().view(np.uint32),
          np.stack([terms[k] for k in sorted(terms)]).view(np.uint32))
    fl = rb.end_flags.cpu().numpy()
    assert (fl[:, 0][fl[:, 0] != 0] == 2).all() and int((fl[:, 0] == 2).sum()) == 9 and (fl[39, 1:] == 4).all()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- downstream
def test_downstream_gae_with_bootstrap_and_episode_stats(monkeypatch):
    """On the scenario's records: bootstrap_rewards + rows.gae(rewards=) against SB3's loop (tests/gae_ref.py) with SB3's time-limit bootstrap added
    (tests/safe_ref.py), and episode_stats against a Monitor restatement that sees the -50s and the wrapper endings, carried across the calls."""
    import torch
    from balatro_gym_amd import EpisodeLimits, EpisodeStats
    from balatro_gym_amd.vec_env import RowBuffers
    from tests import gae_ref
    _shallow_rings(monkeypatch)
    seeds, jokers, calls = _scenario()
    n, K = SC_N, SC_K
    env = _vec(n, seeds, scorer_jokers=True, autoreset=True, max_ante=4)
    env.inject(jokers=jokers, apply_now=True)
    rb = RowBuffers(n, env.device, steps=K, row_stride=384)
    lim = EpisodeLimits(n, env.device, *SC_LIMITS, steps=K)
    stats = EpisodeStats(n, env.device)
    cr, cl = np.zeros(n, np.float64), np.zeros(n, np.int32)
    rng = np.random.default_rng(11)
    boots = 0
    for c, (acts, want, terminal, _) in enumerate(calls):
        env.step_many(torch.from_numpy(np.array(acts)).to(env.device), obs_buffers=rb, limits=lim)
        rewards = want[:, :, R_REWARD:R_REWARD + 8].copy().view(np.float64)[:, :, 0]
        flags, dones = want[:, :, R_FLAGS], want[:, :, R_TERM]
        index = np.array(sorted(t * n + e for t, e, _ in terminal), np.int64)
        tv = rng.standard_normal(len(index)).astype(np.float32)
        values, last_values = rng.standard_normal((K, n)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        assert lim.terminal()[0].cpu().tolist() == index.tolist()
        boosted = rb.bootstrap_rewards(lim, torch.from_numpy(tv).to(env.device), gamma=0.99)
        want_boost = ref.bootstrap(rewards, flags, index, tv, 0.99)
        boots += int((flags.reshape(-1)[index] == 4).sum())
        _diff(f"call {c}: bootstrap_rewards (float64 bits)", boosted.cpu().numpy().view(np.uint64), want_boost.view(np.uint64))
        adv, ret = rb.gae(torch.from_numpy(values).to(env.device), torch.from_numpy(last_values).to(env.device), 0.99, 0.95, rewards=boosted)
        wadv, wret = gae_ref.gae(want_boost.astype(np.float32), dones, values, last_values, 0.99, 0.95)
        _diff(f"call {c}: advantages", adv.cpu().numpy().view(np.uint32), wadv.view(np.uint32))
        _diff(f"call {c}: returns", ret.cpu().numpy().view(np.uint32), wret.view(np.uint32))
        er, el = rb.episode_stats(stats)
        wer, wel = ref.monitor(rewards, dones, cr, cl)
        _diff(f"call {c}: episode returns", er.cpu().numpy().view(np.uint64), wer.view(np.uint64))
        _diff(f"call {c}: episode lengths", el.cpu().numpy(), wel)
        assert wel.max() <= SC_LIMITS[1] and (wel[dones != 0] > 0).all() and not wel[dones == 0].any()
    assert boots >= 20
    env.check()
    env.close()


def test_documented_bootstrap_recipe_with_a_normaliser(monkeypatch):
    """INTEGRATION.md's lines, as written, on the scenario's first call: lim.terminal() -> encode_rows(term, "produced", norm=norm) -> a network's
    values -> normalize_reward -> bootstrap_rewards(rewards=) -> gae.  The encoded terminal records are VecNormalize in evaluation mode with the
    normaliser's statistics as they stand (tests/norm_ref.py, bit for bit) and leave them untouched; the bootstrap lands on the normalised rewards
    where the flags are exactly BG_END_MAX_STEPS.  Then the same lines with M = 0 (limits that never fire).  Also here, on the library the package
    loaded: bg_safe_terminal_slots' values and refusals."""
    import torch
    from balatro_gym_amd import EpisodeLimits, RowNormalizer, _native as nat, encode_rows
    from balatro_gym_amd.vec_env import RowBuffers
    from tests import gae_ref, norm_ref
    L = nat.load()
    assert L.bg_safe_terminal_slots(48, 3, 17) == 17 and L.bg_safe_terminal_slots(100, 50, 1000) == 3 and L.bg_safe_terminal_slots(0, 3, 3) == 1
    assert L.bg_safe_terminal_slots(48, 2, 17) == -1 and L.bg_safe_terminal_slots(48, 17, 2) == -1 and L.bg_safe_terminal_slots(-1, 3, 3) == -1
    _shallow_rings(monkeypatch)
    seeds, jokers, calls = _scenario()
    n, K = SC_N, SC_K
    acts, want, terminal, _ = calls[0]
    gen = torch.Generator(device="cpu").manual_seed(3)
    W = (torch.randn((153, 61), generator=gen) / 16).to("cuda:0")
    net = lambda x: x @ W   # noqa: E731  (60 logits and a value per row)
    for limits in (SC_LIMITS, (2 ** 30, 2 ** 30)):
        env = _vec(n, seeds, scorer_jokers=True, autoreset=True, max_ante=4)
        env.inject(jokers=jokers, apply_now=True)
        rows, lim = RowBuffers(n, env.device, steps=K, row_stride=384), EpisodeLimits(n, env.device, *limits, steps=K)
        norm = RowNormalizer(n, env.device)
        env.step_many(torch.from_numpy(np.array(acts)).to(env.device), obs_buffers=rows, limits=lim)
        norm.normalize_obs(rows.rows)   # statistics of real records (the collection loop's updates)
        before = {k: (v.numpy().tobytes() if hasattr(v, "numpy") else v) for k, v in norm.state_dict().items() if k.startswith("obs_")}
        # ---- the documented lines
        index, term = lim.terminal()
        x = encode_rows(term, "produced", norm=norm)
        tv = net(x)[:, 60]
        rn = rows.normalize_reward(norm)
        rew = rows.bootstrap_rewards(lim, tv, gamma=0.99, rewards=rn)
        values, last_values = torch.zeros((K, n), device=env.device), torch.zeros(n, device=env.device)
        adv, ret = rows.gae(values, last_values, rewards=rew)
        # ----
        M = int(index.numel())
        assert tuple(term.shape) == (M, 384) and tuple(x.shape) == (M, 153) and tuple(tv.shape) == (M,) and M != n
        after = {k: (v.numpy().tobytes() if hasattr(v, "numpy") else v) for k, v in norm.state_dict().items() if k.startswith("obs_")}
        assert before == after, "encode_rows(norm=) changed the statistics"
        flags = rows.end_flags.cpu().numpy()
        if limits == SC_LIMITS:
            assert M == len(terminal) > 100
            _diff("records against the oracle", rows.rows.cpu().numpy()[:, :, :352], want)
            sd = norm.state_dict()
            st = {"obs_mean": sd["obs_mean"].numpy(), "obs_var": sd["obs_var"].numpy(), "obs_count": sd["obs_count"].numpy()[0], "ret_mean": sd["ret_stats"].numpy()[0],
                  "ret_var": sd["ret_stats"].numpy()[1], "ret_count": sd["ret_stats"].numpy()[2], "returns": sd["returns"].numpy()}
            frozen = norm_ref.from_moments(term.cpu().numpy()[None], None, st, epsilon=norm.epsilon, clip_obs=norm.clip_obs, training=False)
            _diff("encode_rows(term, norm=norm) against VecNormalize in evaluation mode", x.cpu().numpy().view(np.uint32), norm_ref.obs_bits(frozen["obs"]).reshape(M, 153))
            assert int((flags.reshape(-1)[index.cpu().numpy()] == 4).sum()) >= 20
        else:
            assert M == 0 and not (flags & 6).any()
        want_rew = ref.bootstrap(rn.cpu().numpy(), flags, index.cpu().numpy(), tv.cpu().numpy(), 0.99)
        _diff(f"limits {limits}: bootstrap_rewards(rewards=rn) (float64 bits)", rew.cpu().numpy().view(np.uint64), want_rew.view(np.uint64))
        assert (want_rew != rn.cpu().numpy()).any() == (limits == SC_LIMITS)
        wadv, wret = gae_ref.gae(want_rew.astype(np.float32), rows.terminated.cpu().numpy(), values.cpu().numpy(), last_values.cpu().numpy(), 0.99, 0.95)
        _diff(f"limits {limits}: advantages", adv.cpu().numpy().view(np.uint32), wadv.view(np.uint32))
        _diff(f"limits {limits}: returns", ret.cpu().numpy().view(np.uint32), wret.view(np.uint32))
        env.check()
        env.close()


# ---------------------------------------------------------------------------------------------------------------- BG_E_ARG
def test_bad_arguments_are_refused_before_anything_is_launched(monkeypatch):
    """Every documented BG_E_ARG case returns BG_E_ARG with its text, leaves the rows buffer untouched, and a following valid call is correct."""
    import ctypes as C
    import torch
    from balatro_gym_amd import EpisodeLimits, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers
    seeds, jokers, calls = _scenario()
    n, K = SC_N, SC_K
    acts = torch.from_numpy(np.array(calls[0][0])).to("cuda:0")

    def call(env, rb, s):
        return env._L.bg_step_many_rows_ex(env._h, K, C.c_void_p(acts.data_ptr()), C.c_void_p(rb.rows.data_ptr()), C.c_uint64(rb.row_stride), 1,
                                           C.byref(s), C.c_void_p(env._stats.data_ptr()), env._stream())

    def refused(env, rb, s, text):
        poison_(rb.rows)
        assert call(env, rb, s) == -1, text
        err = env._L.bg_last_error(env._h).decode()
        assert err.startswith("bg_step_many_rows_ex: ") and text in err, (text, err)
        torch.cuda.synchronize()
        assert bool((rb.rows == POISON).all()), f"{text}: the rows buffer was written"

    env = _vec(n, seeds, scorer_jokers=True, autoreset=True, max_ante=4)
    env.inject(jokers=jokers, apply_now=True)
    rb = RowBuffers(n, env.device, steps=K, row_stride=384)
    lim = EpisodeLimits(n, env.device, *SC_LIMITS, steps=K)
    good = lim._struct()

    def variant(**kw):
        s = nat.SafeLimits.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    refused(env, rb, variant(max_invalid_actions=2), ">= 3")
    refused(env, rb, variant(max_episode_steps=2), ">= 3")
    refused(env, rb, variant(counters_dev=good.counters_dev + 4), "counters_dev")
    refused(env, rb, variant(counters_dev=None), "counters_dev")
    refused(env, rb, variant(terminal_rows_dev=good.terminal_rows_dev + 8), "terminal_rows_dev")
    refused(env, rb, variant(terminal_stride_bytes=360), "terminal_stride_bytes")
    refused(env, rb, variant(terminal_stride_bytes=336), "terminal_stride_bytes")
    refused(env, rb, variant(terminal_step_dev=good.terminal_step_dev + 2), "terminal_step_dev")
    refused(env, rb, variant(terminal_slots=K // 3), "terminal_slots")
    refused(env, rb, variant(terminal_rows_dev=None), "both")
    refused(env, rb, variant(terminal_step_dev=None), "both")
    for kw, text in (({"autoreset": False}, "BG_FLAG_AUTORESET"), ({"autoreset": True}, "BG_ENGINE=3")):
        if not kw["autoreset"]:
            other = _vec(n, seeds, scorer_jokers=True, max_ante=4, **kw)
        else:
            monkeypatch.setenv("BG_ENGINE", "1")
            other = _vec(n, seeds, scorer_jokers=True, max_ante=4, **kw)
            monkeypatch.delenv("BG_ENGINE")
        refused(other, rb, good, text)
        other.close()
    # the Python wrapper's own checks
    with pytest.raises(ValueError, match="EpisodeLimits of 333 envs"):
        env.step_many(acts, obs_buffers=rb, limits=EpisodeLimits(n + 1, env.device))
    with pytest.raises(ValueError, match="RowBuffers"):
        env.step_many(acts, limits=lim)
    with pytest.raises(nat.NativeError, match="terminal_slots"):
        env.step_many(acts, obs_buffers=rb, limits=EpisodeLimits(n, env.device, *SC_LIMITS, steps=K - 3))
    # ... and a valid call, with no terminal buffers at all (both NULL), is the scenario's first call
    poison_(rb.rows)
    assert call(env, rb, variant(terminal_rows_dev=None, terminal_step_dev=None, terminal_slots=0)) == 0
    _diff("the valid call behind the refused ones", rb.rows.cpu().numpy()[:, :, :352], calls[0][1])
    _diff("its counters", lim.counters.cpu().numpy()[:, :2], calls[0][3])
    env.check()
    env.close()
