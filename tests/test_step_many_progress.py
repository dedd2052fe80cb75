"""GPU tests of bg_step_many_rows_progress (BalatroVecEnv.step_many(..., limits=EpisodeLimits(progression=True), progression=ProgressionRewards)):
ProgressionRewardWrapper's reward shaping in front of SafeBalatroEnv's limits inside the packed-record launch (bg_engine3.h's PROG instantiation).
300 envs, which the library runs in its 64-env workgroup shape (113) with 16 live envs per workgroup; tests/test_engine3_instantiations.py runs the
scenarios here in every shape (`cfg` / `epw` / `cards` of _make and _run).  Every byte 0..351 of every record and terminal record, terminal_step, both carries
and the stats are compared against the CPU oracle stepped on the host under tests/progress_ref.py (which tests/test_step_many_progress_host.py holds
to the reference's own wrapper stack)."""
import functools

import numpy as np
import pytest

from tests import progress_ref as ref
from tests import safe_ref
from tests.helpers import OBS_KEYS, POISON, poison_
from tests.test_episode_summary import _summary
from tests.test_gpu_parity import SEED_OFFSET, _vec
from tests.test_step_many_safe import R_FLAGS, R_REWARD, R_TERM, _diff, _pack, _shallow_rings, _terminal_sets

pytestmark = pytest.mark.gpu

N = 300
# scenario: steps of each call, limits, curriculum cap, role of env i
SPECS = {
    # valid card toggles only: the ante-1 penalty from step 151, the 0.2 tier from step 201, stuck at step 301; a second call continues the new episode
    "idle": ((320, 24), (50, 1000), 0, lambda i: "idle"),
    # level-15 hands clear every blind: round, ante, best and efficiency bonuses; the cap ends episodes at ante 4 (the new episode's is 1 or 2);
    # every fourth env plays single cards without levels and loses on ante 1
    "progress": ((32, 32, 32), (50, 1000), 3, lambda i: ("play", "play_ante2", "play", "lose")[i % 4]),
    # injected at ante 2 / ante 3 and idle: the 0.3 tier from step 401, the 0.4 tier from step 601, the step limit at 610
    "long": ((620,), (50, 610), 0, lambda i: ("idle_ante2", "idle_ante3", "idle")[i % 3]),
    # a never-valid action from step 0: killed at 50 with -50; the same begun after step 200 on ante 1: shaped to -1.2 and below, never counted
    "invalid": ((320,), (50, 1000), 0, lambda i: ("invalid", "invalid_late")[i % 2]),
    # the progress scenario with role AND cap by the env's 64-env block as well as by i (tests/test_engine3_instantiations.py: envs 64, 128 and 192
    # apart -- the same lane of another owner wave or slice -- never end their episodes alike; _shapes_conditions states it from the oracle side)
    "shapes": ((32, 32, 32), (50, 1000), lambda i: 2 + i // 64, lambda i: ("play", "play_ante2", "play", "lose")[(i + i // 64) % 4]),
}


def _cap_of(name):
    """The curriculum cap of env i: a spec's cap entry is one int for every env or a function of i."""
    cap = SPECS[name][2]
    return cap if callable(cap) else (lambda i: cap)


def _ante0(role):
    return 2 if role.endswith("ante2") else 3 if role.endswith("ante3") else 0


def _leveled(role):
    return role.startswith("play")


def _action(role, i, t, ob):
    if role == "invalid" or (role == "invalid_late" and t >= 205):
        return 59   # in range, never valid
    phase = int(ob["phase"])
    if phase == 2:
        return 45
    if phase == 1:
        return 31
    if role.startswith("play") or role == "lose":
        return 0 if np.asarray(ob["selected_cards"]).any() else 2 + i % 8
    return 2 + i % 8


def _seeds(name):
    return [761_000 + SEED_OFFSET + 1000 * sorted(SPECS).index(name) + 3 * i for i in range(N)]


@functools.lru_cache(maxsize=None)
def _scenario(name, summary):
    """The scenario on the oracle under progress_ref.ProgressSafe.  Per call: actions [K, N], the expected records [K, N, 352], the expected terminal
    records [(t, e, record)], the limits' counters [N, 2] and the packed progression carry [N, 4] behind the call.  Computed once, never modified."""
    from oracle import pyoracle as po
    calls_k, limits, _, role_of = SPECS[name]
    roles = [role_of(i) for i in range(N)]
    orc = [po.OracleEnv(s, max_ante=_cap_of(name)(i)) for i, s in enumerate(_seeds(name))]

    def prep(o, role):
        if _ante0(role):
            o.set_ante(_ante0(role))
        if _leveled(role):
            for ht in range(12):
                o.set_hand_level(ht, 15)
    for o, r in zip(orc, roles):
        prep(o, r)
    cur = [o.obs() for o in orc]
    wr = [ref.ProgressSafe(*limits) for _ in range(N)]
    calls, t0 = [], 0
    for K in calls_k:
        acts = np.zeros((K, N), np.int32)
        want = np.zeros((K, N, 352), np.uint8)
        terminal = []
        for j in range(K):
            rew, flags = np.zeros(N), np.zeros(N, np.uint8)
            extra = {}
            for i, o in enumerate(orc):
                a = _action(roles[i], i, t0 + j, cur[i])
                acts[j, i] = a
                ob, r, term, _, _ = o.step(int(a))
                rew[i], flags[i] = wr[i].step(r, bool(term), int(ob["ante"]), int(ob["round"]))   # (`ob`: the final state when the game ended)
                if ref.wrapper_ending(int(flags[i])):
                    terminal.append((j, i, _pack({k: np.asarray(ob[k])[None] for k in OBS_KEYS}, rew[i:i + 1], acts[j, i:i + 1], flags[i:i + 1])[0]))
                if flags[i]:   # SAME_STEP reset, whoever ended the episode: the record shows the new one
                    if summary:
                        extra[i] = _summary(ob)
                    o.reset(); prep(o, roles[i])
                    ob = o.obs()
                cur[i] = ob
            want[j] = _pack({k: np.stack([np.asarray(w[k]) for w in cur]) for k in OBS_KEYS}, rew, acts[j], flags)
            for i, s in extra.items():
                want[j, i, 344:352] = s
        counters = np.array([[x.safe.episode_steps, x.safe.consecutive_invalid] for x in wr], np.int32)
        carry = np.stack([x.prog.pack() for x in wr])
        for a in (acts, want, counters, carry):
            a.setflags(write=False)
        calls.append((acts, want, tuple(terminal), counters, carry))
        t0 += K
    return tuple(roles), tuple(calls)


def _rewards(want):
    return want[:, :, R_REWARD:R_REWARD + 8].copy().view(np.float64)[:, :, 0]


def _make(name, monkeypatch=None, shallow=False, cfg=None, epw=None, cards=False):
    """The scenario's handle.  `cfg` / `epw`: BG_E3_CFG / BG_E3_EPW, which bg_create_ex reads per handle (the workgroup shape of bg_engine3.h);
    `cards`: a handle with card states (the CARDS instantiation; nothing is injected, so the oracle side is the same)."""
    _, limits, cap, role_of = SPECS[name]
    if shallow:
        _shallow_rings(monkeypatch)
    if cfg is not None:
        monkeypatch.setenv("BG_E3_CFG", str(cfg))
    if epw is not None:
        monkeypatch.setenv("BG_E3_EPW", str(epw))
    roles = [role_of(i) for i in range(N)]
    env = _vec(N, _seeds(name), autoreset=True, max_ante=0 if callable(cap) else cap, card_states=cards)
    if callable(cap):
        env.set_max_ante([cap(i) for i in range(N)])
    antes = [_ante0(r) for r in roles]
    levels = np.array([[15] * 12 if _leveled(r) else [0] * 12 for r in roles], np.uint8)
    if any(antes) or levels.any():
        env.inject(ante=antes if any(antes) else None, levels=levels if levels.any() else None, apply_now=True)
    return env


def _run(name, monkeypatch=None, summary=False, one_call=False, shallow=False, cfg=None, epw=None, cards=False):
    """The scenario on the device, call by call (or as one call), every output against the oracle's."""
    import torch
    from balatro_gym_amd import EpisodeLimits, ProgressionRewards
    from balatro_gym_amd.vec_env import RowBuffers
    calls_k, limits, _, _ = SPECS[name]
    _, calls = _scenario(name, summary)
    env = _make(name, monkeypatch, shallow, cfg, epw, cards)
    groups = [calls] if one_call else [[c] for c in calls]
    KK = max(sum(len(c[0]) for c in g) for g in groups)
    rb = RowBuffers(N, env.device, steps=KK + 1, row_stride=384)
    lim = EpisodeLimits(N, env.device, *limits, steps=KK, row_stride=384, summary=summary, progression=True)
    prog = ProgressionRewards(N, env.device)
    assert lim.slots == ref.terminal_slots(KK, *limits)
    env.set_profiling(True)
    for gi, group in enumerate(groups):
        acts = np.concatenate([c[0] for c in group])
        want = np.concatenate([c[1] for c in group])
        K, off, terminal = len(acts), 0, {}
        for c in group:
            terminal.update({(t + off, e): rec for t, e, rec in c[2]})
            off += len(c[0])
        poison_(rb.rows); poison_(lim.terminal_rows); poison_(lim.terminal_step)
        env.step_many(torch.from_numpy(acts).to(env.device), obs_buffers=rb, limits=lim, progression=prog)
        ctx = f"{name} summary {summary} call {gi}" + (f" cfg {cfg} epw {epw} cards {cards}" if cfg or epw or cards else "")
        if shallow:
            assert env.get_profile()["rollout_launches"] >= 3, ctx
        got = rb.rows.cpu().numpy()
        _diff(f"{ctx}: shaped rewards [step, env] (float64 bits)", _rewards(got[:K, :, :352]).view(np.uint64), _rewards(want).view(np.uint64))
        _diff(f"{ctx}: records [step, env, byte]", got[:K, :, :352], want)
        assert not got[:K, :, 352:].any(), f"{ctx}: bytes 352..383 of a whole-line record are not zero"
        assert (got[K:] == POISON).all(), f"{ctx}: rows past the call's last step were written"
        sets, ts, trows = _terminal_sets(lim, N)
        assert set(sets) == set(terminal), (ctx, sorted(set(sets) ^ set(terminal))[:8])
        for key, rec in terminal.items():
            _diff(f"{ctx}: terminal record of (step, env) {key}", sets[key], rec)
        assert not trows[ts >= 0][:, 352:].any(), f"{ctx}: bytes 352..383 of a terminal record"
        assert (trows[ts < 0] == POISON).all(), f"{ctx}: a terminal slot that was not used was written"
        cn = lim.counters.cpu().numpy()
        _diff(f"{ctx}: the limits' counters", cn[:, :2], group[-1][3])
        _diff(f"{ctx}: wrapper endings counted per env", cn[:, 2], np.bincount([e for _, e in terminal], minlength=N).astype(np.int32))
        assert not cn[:, 3].any()
        _diff(f"{ctx}: the progression carry", prog.counters.cpu().numpy(), group[-1][4])
        st = env.stats()
        assert st["steps"] == N * K and st["episodes"] == int((want[:, :, R_TERM] != 0).sum()), (ctx, st)
    env.check()
    return env, rb, lim, prog


def test_idle_scenario_penalty_tier_and_stuck_ending():
    """Valid toggles for 320 steps, then 24 more: -0.5 * (k - 150) from the 151st step on ante 1, -0.2 from the 201st, the stuck ending at the 301st with
    its terminal record (flags BG_END_STUCK, reward -0.5 * 151 - 50 - 0.2) and reset; the following call continues the new episode."""
    _, calls = _scenario("idle", False)
    want = calls[0][1]
    rew, fl = _rewards(want), want[:, :, R_FLAGS]
    assert (fl[300] == ref.END_STUCK).all() and not fl[:300].any() and not fl[301:].any()
    assert (rew[150] == -0.5).all() and (rew[199] == -25.0).all() and (rew[200] == -25.5 - 0.2).all() and (rew[300] == (-75.5 - 50.0) - 0.2).all()
    assert len(calls[0][2]) == N and all(t == 300 for t, _, _ in calls[0][2])
    assert (calls[0][4][:, 0] == 19).all() and (calls[1][4][:, 0] == 43).all()   # total_steps of the new episode
    env, _, lim, _ = _run("idle")
    assert (lim.counters[:, 0] == 43).all()
    env.close()


@pytest.mark.parametrize("summary", [False, True], ids=["summary-off", "summary-on"])
def test_progress_scenario_bonuses_and_game_overs(monkeypatch, summary):
    """Scripted plays with level-15 hands under cap 3, three calls of 32 steps on shallow rings: round, ante, best and efficiency bonuses; episodes the
    cap ends at ante 4 while the record already shows ante 1 or 2, and real game overs on ante 1.  With the episode summary off bytes 344..351 are
    zeros, with it on they hold the final state of every ended step -- and the rule reads the final ante and round either way."""
    roles, calls = _scenario("progress", summary)
    rew = np.concatenate([_rewards(c[1]) for c in calls])
    fl = np.concatenate([c[1][:, :, R_FLAGS] for c in calls])
    game = fl == ref.END_GAME
    assert game.any(axis=0)[[i for i, r in enumerate(roles) if r != "lose"]].all(), "an env never reached the cap"
    assert game.any(axis=0)[[i for i, r in enumerate(roles) if r == "lose"]].all(), "a single-card env never lost"
    assert (rew >= 200.0).sum() >= N and ((rew >= 20.0) & (rew < 200.0)).any() and not (fl & (0xff ^ ref.END_GAME)).any()
    # the step that ended at the cap: final ante 4 > last_ante 3 is worth 200 + 100 + 50 on top of the env's reward, which ante 1 / 2 would not give
    capped = game[:, 0]
    assert capped.any() and (rew[capped, 0] >= 350.0).all()
    if summary:
        want = np.concatenate([c[1] for c in calls])
        assert (want[:, :, 344][game] >= 1).all() and (want[:, 0, 344][capped] == 4).all() and not want[:, :, 344:352][~game].any()
    env, rb, _, _ = _run("progress", monkeypatch, summary=summary, shallow=True)
    if not summary:
        assert not rb.rows[:32, :, 344:352].any()
    env.close()


def test_long_scenario_tiers_and_step_limit():
    """620 steps in one call under limits 50 / 610: envs injected at ante 2 idle into the 0.3 tier (step 401), envs at ante 3 collect the efficiency
    bonus for 299 steps and reach the 0.4 tier (step 601), both end on the step limit at step 610 (flags exactly BG_END_MAX_STEPS: bootstrapped);
    ante-1 envs are stuck twice."""
    roles, calls = _scenario("long", False)
    want = calls[0][1]
    rew, fl = _rewards(want), want[:, :, R_FLAGS]
    a1, a2, a3 = 2, 0, 1   # an env of each role
    assert roles[a2] == "idle_ante2" and roles[a3] == "idle_ante3" and roles[a1] == "idle"
    assert rew[0, a2] == 300.0 and rew[399, a2] == 0.0 and rew[400, a2] == -0.3 and rew[609, a2] == -0.3
    assert rew[0, a3] == 550.0 and rew[298, a3] == 50.0 and rew[299, a3] == 0.0 and rew[599, a3] == 0.0 and rew[600, a3] == -0.4
    assert fl[609, a2] == fl[609, a3] == ref.END_MAX_STEPS and np.flatnonzero(fl[:, a1]).tolist() == [300, 601] and (fl[[300, 601], a1] == ref.END_STUCK).all()
    env, rb, lim, _ = _run("long")
    index, _ = lim.terminal()
    assert int((rb.end_flags.reshape(-1)[index.long()] == ref.END_MAX_STEPS).sum()) == sum(r != "idle" for r in roles)
    env.close()


def test_invalid_scenario_counted_and_uncounted_runs():
    """Action 59 from step 0: killed every 50 steps with -50.0 (the shaped reward of steps 1..200 is the env's -1.0).  The same begun at step 205 on
    ante 1: the shaped reward is -1.2 minus the ante-1 penalty, never -1.0, so 96 invalid actions in a row are not counted; the episode ends stuck."""
    roles, calls = _scenario("invalid", False)
    want = calls[0][1]
    rew, fl = _rewards(want), want[:, :, R_FLAGS]
    assert roles[0] == "invalid" and roles[1] == "invalid_late"
    assert np.flatnonzero(fl[:, 0]).tolist() == [49, 99, 149, 199, 249, 299] and (fl[fl[:, 0] != 0, 0] == ref.END_INVALID).all()
    assert (rew[fl[:, 0] != 0, 0] == -50.0).all() and (rew[fl[:, 0] == 0, 0] == -1.0).all()
    assert np.flatnonzero(fl[:, 1]).tolist() == [300] and fl[300, 1] == ref.END_STUCK and (want[205:300, 1, 172:176].copy().view(np.int32) == 59).all()
    assert rew[205, 1] == (-1.0 + -0.5 * 56) - 0.2 and (rew[301:, 1] == -1.0).all()
    env, _, _, _ = _run("invalid")
    env.close()


def test_one_call_equals_three(monkeypatch):
    """The progress scenario's 96 steps as ONE call on shallow rings (bg_max_fused_steps * 3 <= 32: every call is several launches, and the carries
    cross them): the same records, terminal records and carries as the three calls, all held to the oracle."""
    env, _, _, _ = _run("progress", monkeypatch, one_call=True, shallow=True)
    assert env.max_fused_steps * 3 <= 32
    env.close()


def test_null_progress_is_step_many_rows_ex():
    """progress = NULL through bg_step_many_rows_progress: the bytes of bg_step_many_rows_ex on a twin handle, records, terminal records and counters
    (limits = NULL too: bg_step_many_rows')."""
    import ctypes as C
    import torch
    from balatro_gym_amd import EpisodeLimits
    from balatro_gym_amd.vec_env import RowBuffers
    _, calls = _scenario("invalid", False)
    K = 120
    acts = torch.from_numpy(np.array(calls[0][0][:K])).to("cuda:0")
    outs = []
    for mode in ("ex", "progress-null", "plain", "both-null"):
        env = _make("invalid")
        rb = RowBuffers(N, env.device, steps=K, row_stride=384)
        lim = EpisodeLimits(N, env.device, 50, 1000, steps=K)
        poison_(rb.rows); poison_(lim.terminal_rows)
        args = (env._h, K, C.c_void_p(acts.data_ptr()), C.c_void_p(rb.rows.data_ptr()), C.c_uint64(384), 1)
        tail = (C.c_void_p(env._stats.data_ptr()), env._stream())
        if mode == "ex":
            rc = env._L.bg_step_many_rows_ex(*args, C.byref(lim._struct()), *tail)
        elif mode == "progress-null":
            rc = env._L.bg_step_many_rows_progress(*args, C.byref(lim._struct()), None, *tail)
        elif mode == "plain":
            rc = env._L.bg_step_many_rows(*args, *tail)
        else:
            rc = env._L.bg_step_many_rows_progress(*args, None, None, *tail)
        assert rc == 0, (mode, env._L.bg_last_error(env._h).decode())
        outs.append((rb.rows.cpu().numpy(), lim.terminal_rows.cpu().numpy(), lim.terminal_step.cpu().numpy(), lim.counters.cpu().numpy()))
        env.check()
        env.close()
    for a, b, what in ((0, 1, "progress = NULL against bg_step_many_rows_ex"), (2, 3, "limits = progress = NULL against bg_step_many_rows")):
        for x, y, part in zip(outs[a], outs[b], ("records", "terminal records", "terminal_step", "counters")):
            _diff(f"{what}: {part}", y, x)
    assert (outs[0][0][:, :, R_FLAGS] == ref.END_INVALID).sum() == 2 * (N // 2) and not (outs[0][0][:, :, R_FLAGS] & ref.END_STUCK).any()
    assert not outs[2][0][:, :, R_FLAGS].any()


def test_bad_arguments_are_refused_before_anything_is_launched(monkeypatch):
    """Every documented BG_E_ARG case returns BG_E_ARG with "bg_step_many_rows_progress: ...", leaves rows and carry untouched, and a following valid
    call is correct."""
    import ctypes as C
    import torch
    from balatro_gym_amd import EpisodeLimits, ProgressionRewards, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers
    _, calls = _scenario("invalid", False)
    K = 320
    acts = torch.from_numpy(np.array(calls[0][0])).to("cuda:0")
    L = nat.load()
    assert L.bg_progress_terminal_slots(903, 2 ** 30, 2 ** 30) == 4 and L.bg_progress_terminal_slots(100, 50, 1000) == 3 and L.bg_progress_terminal_slots(0, 3, 3) == 1
    assert L.bg_progress_terminal_slots(48, 2, 17) == -1 and L.bg_progress_terminal_slots(48, 17, 2) == -1 and L.bg_progress_terminal_slots(-1, 3, 3) == -1

    def call(env, rb, s, p):
        return env._L.bg_step_many_rows_progress(env._h, K, C.c_void_p(acts.data_ptr()), C.c_void_p(rb.rows.data_ptr()), C.c_uint64(rb.row_stride), 1,
                                                 None if s is None else C.byref(s), C.byref(p), C.c_void_p(env._stats.data_ptr()), env._stream())

    def refused(env, rb, s, p, text):
        poison_(rb.rows)
        assert call(env, rb, s, p) == -1, text
        err = env._L.bg_last_error(env._h).decode()
        assert err.startswith("bg_step_many_rows_progress: ") and text in err, (text, err)
        torch.cuda.synchronize()
        assert bool((rb.rows == POISON).all()), f"{text}: the rows buffer was written"
        assert not prog.counters.any(), f"{text}: the carry was written"

    env = _make("invalid")
    rb = RowBuffers(N, env.device, steps=K, row_stride=384)
    lim = EpisodeLimits(N, env.device, 1000, 1000, steps=K, progression=True)   # 2 slots; the limits alone would ask for 1
    prog = ProgressionRewards(N, env.device)
    good, gp = lim._struct(), prog._struct()

    def variant(**kw):
        s = nat.SafeLimits.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    refused(env, rb, None, gp, "needs limits")
    refused(env, rb, good, nat.ProgressRewards(gp.counters_dev + 4), "16-byte aligned")
    refused(env, rb, good, nat.ProgressRewards(None), "progress->counters_dev")
    refused(env, rb, good, nat.ProgressRewards(good.counters_dev), "must not be the limits' counters")
    assert lim.slots == 2 and EpisodeLimits(N, env.device, 1000, 1000, steps=K).slots == 1
    refused(env, rb, variant(terminal_slots=1), gp, "bg_progress_terminal_slots")
    refused(env, rb, variant(max_invalid_actions=2), gp, ">= 3")
    refused(env, rb, variant(max_episode_steps=2), gp, ">= 3")
    refused(env, rb, variant(counters_dev=good.counters_dev + 4), gp, "counters_dev")
    refused(env, rb, variant(terminal_stride_bytes=360), gp, "terminal_stride_bytes")
    refused(env, rb, variant(terminal_rows_dev=None), gp, "both")
    for kw, text in (({"autoreset": False}, "BG_FLAG_AUTORESET"), ({"autoreset": True}, "BG_ENGINE=3")):
        if kw["autoreset"]:
            monkeypatch.setenv("BG_ENGINE", "1")
        other = _vec(N, _seeds("invalid"), **kw)
        if kw["autoreset"]:
            monkeypatch.delenv("BG_ENGINE")
        refused(other, rb, good, gp, text)
        other.close()
    # the Python wrapper's own checks
    with pytest.raises(ValueError, match="ProgressionRewards of 300 envs"):
        env.step_many(acts, obs_buffers=rb, limits=lim, progression=ProgressionRewards(N + 1, env.device))
    with pytest.raises(ValueError, match="progression needs limits"):
        env.step_many(acts, obs_buffers=rb, progression=prog)
    with pytest.raises(ValueError, match="RowBuffers"):
        env.step_many(acts, progression=prog)
    with pytest.raises(nat.NativeError, match="bg_progress_terminal_slots"):
        env.step_many(acts, obs_buffers=rb, limits=EpisodeLimits(N, env.device, 1000, 1000, steps=K), progression=prog)
    # ... and a valid call behind them, under limits that never fire: the late-invalid envs end stuck, the others too (nothing counts their -1.0s away)
    poison_(rb.rows)
    env.step_many(acts, obs_buffers=rb, limits=lim, progression=prog)
    fl = rb.end_flags.cpu().numpy()
    assert (fl[300] == ref.END_STUCK).all() and not fl[:300].any() and not fl[301:].any()
    assert bool((lim.terminal_step[0] == 300).all()) and bool((lim.terminal_step[1] == -1).all())
    env.check()
    env.close()


def test_downstream_gae_episode_stats_and_reward_normalisation():
    """On the long scenario's records (stuck endings, step-limit endings, shaped rewards of 550 and of -0.3): rows.gae with the time-limit bootstrap
    against SB3's loop (tests/gae_ref.py), episode_stats against the Monitor restatement (safe_ref.monitor: Monitor sits outside both wrappers and sees
    the shaped rewards), normalize_reward against VecNormalize's reward half (tests/norm_ref.py), all fed the oracle's shaped rewards."""
    import torch
    from balatro_gym_amd import EpisodeStats, RowNormalizer
    from tests import gae_ref, norm_ref
    _, calls = _scenario("long", False)
    acts, want, terminal, _, _ = calls[0]
    K = len(acts)
    env, rb, lim, _ = _run("long")
    rewards, flags, dones = _rewards(want), want[:, :, R_FLAGS], want[:, :, R_TERM]
    rng = np.random.default_rng(13)
    index = np.array(sorted(t * N + e for t, e, _ in terminal), np.int64)
    tv = rng.standard_normal(len(index)).astype(np.float32)
    values, last_values = rng.standard_normal((K, N)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    assert lim.terminal()[0].cpu().tolist() == index.tolist()
    boosted = rb.bootstrap_rewards(lim, torch.from_numpy(tv).to(env.device), gamma=0.99)
    want_boost = safe_ref.bootstrap(rewards, flags, index, tv, 0.99)
    stuck_idx = index[flags.reshape(-1)[index] == ref.END_STUCK]
    assert len(stuck_idx) and (want_boost.reshape(-1)[stuck_idx] == rewards.reshape(-1)[stuck_idx]).all(), "a stuck ending was bootstrapped"
    assert (want_boost != rewards).sum() == int((flags == ref.END_MAX_STEPS).sum()) > 0
    _diff("bootstrap_rewards (float64 bits)", boosted[:K].cpu().numpy().view(np.uint64), want_boost.view(np.uint64))
    rows = RowBuffersView(rb, K)
    adv, ret = rows.gae(torch.from_numpy(values).to(env.device), torch.from_numpy(last_values).to(env.device), 0.99, 0.95, rewards=boosted[:K].contiguous())
    wadv, wret = gae_ref.gae(want_boost.astype(np.float32), dones, values, last_values, 0.99, 0.95)
    _diff("advantages", adv.cpu().numpy().view(np.uint32), wadv.view(np.uint32))
    _diff("returns", ret.cpu().numpy().view(np.uint32), wret.view(np.uint32))
    er, el = rows.episode_stats(EpisodeStats(N, env.device))
    wer, wel = safe_ref.monitor(rewards, dones)
    _diff("episode returns", er.cpu().numpy().view(np.uint64), wer.view(np.uint64))
    _diff("episode lengths", el.cpu().numpy(), wel)
    assert set(np.unique(wel[dones != 0]).tolist()) == {301, 610}
    nr = rows.normalize_reward(RowNormalizer(N, env.device))
    rets, _ = norm_ref.returns_of(rewards, dones != 0, np.zeros(N))
    wn = norm_ref.reward_from_moments(rewards, dones != 0, np.stack(norm_ref.tree_moments_ret(rets), axis=-1), norm_ref.new_state(N))
    _diff("normalize_reward (float64 bits)", nr.cpu().numpy().view(np.uint64), wn["reward"].view(np.uint64))
    env.close()


def RowBuffersView(rb, K):
    """A RowBuffers over the first K steps of `rb` (the scans take every row of their buffer)."""
    from balatro_gym_amd.vec_env import RowBuffers
    out = RowBuffers(rb.n, rb.rows.device, steps=K, row_stride=rb.row_stride)
    out.rows.copy_(rb.rows[:K])
    return out
