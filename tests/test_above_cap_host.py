"""What the scenario of tests/above_cap_ref.py contains, from the oracle side alone (no GPU): the conditions that keep the GPU tests of
tests/test_above_cap.py from being vacuous.  The counts are printed (pytest -s) and quoted in DESIGN.md section 7."""
import numpy as np
import pytest

from tests import above_cap_ref as ac


@pytest.mark.parametrize("mode,autoreset", [("caller", True), ("caller", False), ("policy", True)], ids=["caller-on", "caller-off", "policy"])
def test_scenario_conditions(mode, autoreset):
    sc = ac.scenario(mode, autoreset)
    c = ac.counts(sc)
    print(f"{mode} autoreset {autoreset}: {c}")
    W, N = ac.W, ac.N
    # the lowering leaves enough envs above their new cap, in both bg_engine.h workgroups and in every 64-env block of bg_engine3.h
    assert c["above_at_lowering"] >= 60 and c["of_them_env_256_up"] >= 10, c
    assert min(c["per_64_block"]) >= 5, c
    first = c["first_action"]
    if mode == "caller":
        # the first action behind the lowering: every cheap kind (what the owner / worker waves settle on the LDS image) and every service kind
        assert all(first[k] >= 8 for k in ac.CHEAP), first
        assert all(first[k] >= 5 for k in ac.SERVICE), first
    else:
        # the policy's own first actions: mostly toggles, and shop leaves
        assert first["toggle"] >= 8 and first["leave"] >= 8 and first["play"] >= 5, first
    # a blind selection is never on offer above a cap (above_cap_ref.DONE): the actions 45 that are sent count as invalid ones
    assert first["blind"] == 0 and not (sc.done == ac.DONE.index("blind")).any()
    # every step of an env above its cap is terminated with the curriculum flag, whatever the action
    assert (sc.terminated[sc.above] == 1).all() and ((sc.flags[sc.above] & 256) != 0).all()
    # the envs whose cap was not lowered do not end on the lowering step for cap reasons
    assert not (sc.flags[W, 3::4] & 256).any() and not sc.above[W, 3::4].any()
    assert not sc.above[:W].any() or not autoreset   # (with auto-reset nothing stands above a cap before the lowering)
    caps = ac.caps1()
    assert (caps[0::4] == 1).all() and (caps[1::4] == 1).all() and (caps[2::4] == 2).all() and (caps[3::4] == ac.caps0()[3::4]).all()
    if autoreset:
        # one ending per lowered env, then play continues below the cap
        assert c["steps_above_after_lowering"] == c["above_at_lowering"], c
        assert (sc.terminated[W][sc.above[W]] == 1).all() and not sc.above[W + 1:].any()
    else:
        # the env stays above its cap: at least 20 envs take at least 5 consecutive steps there (here: all K steps), every kind among them
        assert c["envs_5_steps_above"] >= 20, c
        later = np.bincount(sc.done[W + 1:][sc.above[W + 1:]], minlength=len(ac.DONE))
        print(f"steps above the cap behind the first, by kind {dict(zip(ac.DONE, later.tolist()))}")
        assert all(later[ac.DONE.index(k)] >= 8 for k in ac.CHEAP + ("play",)), later
        # ... and the other way above a cap: exceeded by PLAY behind the lowering (flag 256 on a step that did not start above), then stepped on
        crossed = ((sc.flags[W:] & 256) != 0) & ~sc.above[W:]
        stepped_on = int((crossed[:-1] & sc.above[W + 1:]).sum())
        print(f"caps exceeded by play behind the lowering {int(crossed.sum())}, stepped on afterwards {stepped_on}")
        assert stepped_on >= 5, (int(crossed.sum()), stepped_on)


@pytest.mark.parametrize("progress", [False, True], ids=["safe", "progress"])
def test_wrapped_scenario_conditions(progress):
    """The scenario under SafeBalatroEnv's limits (and ProgressionRewardWrapper): every env the lowering leaves above its cap ends on the lowering
    step as an ending of the ENV (BG_END_GAME) whose summary shows an ante above the new cap -- on cheap actions too -- and the run also holds
    kills and step-limit endings."""
    calls, cap_ended = ac.wrapped(progress)
    W = ac.W
    want = np.concatenate([c[1] for c in calls])
    fl = want[:, :, 343]
    ante = want[:, :, 344:346].copy().view(np.int16)[:, :, 0]
    ab = cap_ended[W]
    kills, limit_only = int((fl & 2 != 0).sum()), int((fl == 4).sum())
    print(f"progress {progress}: above their cap at the lowering {int(ab.sum())}, kills {kills}, step-limit endings {limit_only}, "
          f"wrapper endings with a terminal record {sum(len(c[2]) for c in calls)}")
    assert int(ab.sum()) >= 60 and int(ab[256:].sum()) >= 10
    assert (fl[W][ab] & 1 != 0).all() and (ante[W][ab] > ac.caps1()[ab]).all()
    assert (fl[cap_ended] & 1 != 0).all()
    assert kills >= 5 and limit_only >= 20, (kills, limit_only)
    counters = calls[1][3]
    assert (counters >= 0).all() and (counters[ab, 0] <= ac.K - 1).all()   # every lowered env's step counter started again behind its ending
    if progress:
        assert calls[1][4].shape == (ac.N, 4)


def test_records_and_stats_helpers():
    """Scenario.records packs what the GPU record tests compare (bytes 0..351; reward, action word, terminated in place) and Scenario.stats
    restates the rollout counters."""
    sc = ac.scenario("policy", True)
    rows = sc.records(ac.W, ac.W + 2)
    assert rows.shape == (2, ac.N, 352) and rows.dtype == np.uint8
    assert np.array_equal(rows[:, :, 136:144].copy().view(np.float64)[:, :, 0].view(np.uint64), sc.reward[ac.W:ac.W + 2].view(np.uint64))
    assert np.array_equal(rows[:, :, 172:176].copy().view(np.int32)[:, :, 0], sc.acts[ac.W:ac.W + 2])
    assert np.array_equal(rows[:, :, 342], sc.terminated[ac.W:ac.W + 2]) and not rows[:, :, 343:].any()
    st = sc.stats(ac.W, ac.W + ac.K, t0=ac.W)
    assert st["steps"] == ac.N * ac.K and st["episodes"] >= ac.counts(sc)["above_at_lowering"] and st["plays"] > 0
