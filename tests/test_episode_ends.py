"""GPU tests of bg_episode_ends_rows (episode_ends / RowCurriculum.update): the report over a [K, N] rollout of packed records and the curriculum's
state, exactly tests/ends_ref.py's (which tests/test_episode_ends_host.py holds to sb3_adapter.CurriculumTracker.update) on synthetic records;
and a whole curriculum job -- step_many with the episode summary, RowCurriculum.update after every call -- against the CPU oracle followed by
CurriculumTracker itself."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

from tests import ends_ref as ref
from tests import safe_ref
from tests.helpers import OBS_KEYS, POISON, poison_
from tests.test_episode_ends_host import _StandIn, synthetic_rows
from tests.test_episode_summary import R_END_ANTE, _summary
from tests.test_gpu_parity import SEED_OFFSET, _oracle_envs, _vec
from tests.test_step_many_safe import R_FLAGS, _diff, _pack, _shallow_rings

pytestmark = pytest.mark.gpu

SY_N, SY_K = 333, 37   # six workgroups, the last one partial; three batches of 16 steps, the last one partial


class _DevStandIn(_StandIn):
    def __init__(self, n):
        super().__init__(n)
        self.device = "cuda:0"


@functools.lru_cache(maxsize=None)
def _synthetic(stride):
    """Two rollouts [K, N, stride] of synthetic records: terminated with p = 0.2, end antes 0..20, flags from {1, 2, 4, 6}, chips to 2**32 - 1."""
    rng = np.random.default_rng(stride)
    rows = synthetic_rows(rng, 2 * SY_K, SY_N, stride)
    rows.setflags(write=False)
    return rows


def _state(cur):
    return cur.cap.cpu().numpy(), cur.hist.cpu().numpy(), cur.count.cpu().numpy(), cur.at_level.cpu().numpy()


def _assert_state(ctx, cur, want):
    cap, hist, count, at_level = _state(cur)
    _diff(f"{ctx}: cap", cap, want.cap)
    _diff(f"{ctx}: hist", hist, want.hist)
    _diff(f"{ctx}: count", count, want.count)
    _diff(f"{ctx}: at_level", at_level, want.at_level)


@pytest.mark.parametrize("stride", [352, 384])
@pytest.mark.parametrize("window", [1, 4, 100])
def test_report_and_curriculum_on_synthetic_records(stride, window):
    """The report and the curriculum's state after each of two calls of K = 37 exactly ends_ref's; the same 74 steps as ONE call on a second state
    give the same caps, history, counts and levels; without a curriculum the report alone (word 8 = 0); the report tensor is overwritten, the raised
    mask written for every env; set_max_ante gets exactly the raised caps, and only when a cap rose."""
    import torch
    from balatro_gym_amd import RowCurriculum, _native as nat, episode_ends
    both = _synthetic(stride)
    thr = 1.0 if window == 1 else 0.8
    env, env1 = _DevStandIn(SY_N), _DevStandIn(SY_N)
    cur, one = RowCurriculum(env, 3, 2, thr, window), RowCurriculum(env1, 3, 2, thr, window)
    want = ref.Curriculum(SY_N, 3, 2, thr, window)
    init = np.random.default_rng(window).integers(1, 12, SY_N).astype(np.int32)
    init[::13] = 0      # no cap: never raised (the clamp at 255 needs antes past 20: tests/test_episode_ends_host.py drives it)
    for c in (cur, one):
        c.cap.copy_(torch.from_numpy(init))
    want.cap[:] = init
    raises = 0
    for half in range(2):
        rows_np = both[half * SY_K:(half + 1) * SY_K]
        rows = torch.from_numpy(np.array(rows_np)).to("cuda:0")
        ctx = f"stride {stride} window {window} call {half}"
        rep0 = episode_ends(rows)
        assert rep0.dtype == torch.int64 and tuple(rep0.shape) == (32,) and rep0.is_cuda
        _diff(f"{ctx}: the report without a curriculum", rep0.cpu().numpy(), ref.report(rows_np))
        poison_(cur.raised)
        ncalls = len(env.calls)
        rep, ms = cur.update(rows, timing=True)
        want_raised = want.update(rows_np)
        _diff(f"{ctx}: the report", rep.cpu().numpy(), ref.report(rows_np, int(want_raised.sum())))
        _diff(f"{ctx}: raised", cur.raised.cpu().numpy(), want_raised.astype(np.uint8))
        _assert_state(ctx, cur, want)
        assert ms > 0.0
        if want_raised.any():
            assert len(env.calls) == ncalls + 1 and np.array_equal(env.calls[-1][0], want.cap) and np.array_equal(env.calls[-1][1] != 0, want_raised), ctx
        else:
            assert len(env.calls) == ncalls, ctx
        raises += int(want_raised.sum())
        r = rep.cpu().numpy()
        assert r[nat.ENDS_REPORT["no_summary"]] > 0 and r[nat.ENDS_HIST] == 0 and r[nat.ENDS_HIST + 15] > 0 and r[nat.ENDS_REPORT["chips_max"]] == 2 ** 32 - 1
    assert (raises > 0) == (window < 100)   # (window 100: no env has played a hundred episodes in 74 steps)
    rep1 = one.update(torch.from_numpy(np.array(both)).to("cuda:0"), apply=False)
    _assert_state(f"stride {stride} window {window}: one call of 2 K", one, want)
    assert len(env1.calls) == 1, "apply=False set caps"   # (the constructor's call)
    both_rep = ref.report(both, int(one.raised.sum().item()))
    _diff("the report of one call of 2 K", rep1.cpu().numpy(), both_rep)
    assert (want.cap[::13] == 0).all()


def test_smallest_and_empty_and_repeat():
    """N = 1, K = 1 (ended and not ended); K * N == 0 writes a zero report and a zero raised mask; two calls on the same records and state copies
    give the same values (integer atomics)."""
    import torch
    from balatro_gym_amd import RowCurriculum, _native as nat, episode_ends
    L = nat.load()
    for term in (0, 1):
        rows_np = np.zeros((1, 1, 352), np.uint8)
        ref.put_fields(rows_np, np.array([[term]], np.uint8), np.array([[4]], np.uint8), np.array([[7]], np.int16), np.array([[2]], np.int8), np.array([[123456]], np.uint32))
        rows = torch.from_numpy(rows_np).to("cuda:0")
        cur = RowCurriculum(_DevStandIn(1), 7, 1, 1.0, 1)
        rep = cur.update(rows).cpu().numpy()
        _diff(f"terminated {term}", rep, ref.report(rows_np, term))
        assert rep[nat.ENDS_HIST + 7] == term and rep[nat.ENDS_REPORT["max_steps"]] == term and rep[nat.ENDS_REPORT["chips_sum"]] == 123456 * term
        assert cur.cap.tolist() == [7 + term] and cur.count.tolist() == [term] and cur.raised.tolist() == [term]
    # K * N == 0 through the C call: the report is zeroed, the raised mask too, nothing else is touched
    rows = torch.from_numpy(np.array(_synthetic(384)[:SY_K])).to("cuda:0")
    cur = RowCurriculum(_DevStandIn(SY_N), 3, 1, 0.8, 4)
    report = torch.full((32,), 77, dtype=torch.int64, device="cuda:0")
    poison_(cur.raised)
    before = [x.copy() for x in _state(cur)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.bg_episode_ends_rows(C.c_void_p(rows.data_ptr()), C.c_uint64(384), 0, C.c_int64(SY_N), C.c_void_p(report.data_ptr()), C.byref(cur._struct()), None, st) == 0
    assert report.tolist() == [0] * 32 and not cur.raised.any()
    report.fill_(77)
    assert L.bg_episode_ends_rows(C.c_void_p(rows.data_ptr()), C.c_uint64(384), SY_K, C.c_int64(0), C.c_void_p(report.data_ptr()), None, None, st) == 0
    assert report.tolist() == [0] * 32
    for a, b in zip(before, _state(cur)):
        assert np.array_equal(a, b)
    assert episode_ends(rows[:0]).tolist() == [0] * 32 and cur.update(rows[:0]).tolist() == [0] * 32
    # the same call twice
    reps = []
    for _ in range(2):
        c2 = RowCurriculum(_DevStandIn(SY_N), 3, 1, 0.8, 4)
        reps.append((c2.update(rows).cpu().numpy(), *_state(c2)))
    for a, b in zip(*reps):
        assert np.array_equal(a, b)


def test_bad_arguments_are_refused_before_anything_is_launched():
    """Every documented BG_E_ARG case returns BG_E_ARG with its text and leaves the report and the curriculum's state untouched."""
    import torch
    from balatro_gym_amd import RowCurriculum, _native as nat
    L = nat.load()
    rows = torch.from_numpy(np.array(_synthetic(384)[:SY_K])).to("cuda:0")
    cur = RowCurriculum(_DevStandIn(SY_N), 3, 1, 0.8, 4)
    report = torch.full((32,), 77, dtype=torch.int64, device="cuda:0")
    poison_(cur.raised)
    before = [x.copy() for x in _state(cur)]
    good = cur._struct()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(rows_ptr=rows.data_ptr(), stride=384, K=SY_K, N=SY_N, rep=report.data_ptr(), s=good):
        return L.bg_episode_ends_rows(C.c_void_p(rows_ptr), C.c_uint64(stride), K, C.c_int64(N), C.c_void_p(rep), None if s is None else C.byref(s), None, st)

    def variant(**kw):
        s = nat.Curriculum.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    cases = [({"rows_ptr": None}, "rows_dev"), ({"rows_ptr": rows.data_ptr() + 8}, "rows_dev"), ({"stride": 336}, "row_stride_bytes"), ({"stride": 360}, "row_stride_bytes"),
             ({"K": -1}, "K / N"), ({"N": -1}, "K / N"), ({"rep": None}, "report_dev"), ({"rep": report.data_ptr() + 4}, "report_dev"),
             ({"rep": None, "s": None}, "report_dev")]
    for name in ("cap_dev", "hist_dev", "count_dev", "at_level_dev", "raised_dev"):
        cases.append(({"s": variant(**{name: None})}, "must all be device pointers"))
    cases += [({"s": variant(cap_dev=good.cap_dev + 2)}, "aligned"), ({"s": variant(at_level_dev=good.at_level_dev + 2)}, "aligned"),
              ({"s": variant(hist_dev=good.hist_dev + 1)}, "aligned"), ({"s": variant(count_dev=good.count_dev + 4)}, "aligned"),
              ({"s": variant(window=0)}, "window"), ({"s": variant(increment=0)}, "increment"), ({"s": variant(increment=256)}, "increment"),
              ({"s": variant(threshold=float("nan"))}, "threshold"), ({"s": variant(threshold=float("inf"))}, "threshold")]
    for kw, text in cases:
        assert call(**kw) == -1, (kw, text)
        err = L.bg_last_error(None).decode()
        assert err.startswith("bg_episode_ends_rows: ") and text in err, (text, err)
    torch.cuda.synchronize()
    assert report.tolist() == [77] * 32 and bool((cur.raised == POISON).all())
    for a, b in zip(before, _state(cur)):
        assert np.array_equal(a, b)
    assert call() == 0 and report[0].item() == int((_synthetic(384)[:SY_K, :, 342] != 0).sum())


# ---------------------------------------------------------------------------------------------------------------- a curriculum job
IN_N, IN_K, IN_CALLS, IN_LIMITS = 96, 48, 3, (3, 60)


@functools.lru_cache(maxsize=None)
def _job():
    """96 envs under the oracle's policy 2, scorer jokers, limits 3 / 60, initial cap 1, three calls of 48 steps.  The oracle side is followed by
    sb3_adapter.CurriculumTracker (window 2, threshold 0.8) fed every step from the oracle's own final observations; the caps it raises reach the
    oracle's envs at the call boundaries.  Per call: actions, expected records with bytes 344..351, and behind the call the tracker's caps, history,
    counts, levels and the mask of the envs it raised during the call."""
    from balatro_gym_amd.sb3_adapter import CurriculumTracker
    from oracle.gen_golden import IMPLEMENTED
    n, K = IN_N, IN_K
    seeds = [752_000 + SEED_OFFSET + 7 * i for i in range(n)]
    jokers = [random.Random(7300 + i).sample(IMPLEMENTED, i % 6) for i in range(n)]
    orc = _oracle_envs(n, seeds, True, 1, jokers)
    cnt = [safe_ref.SafeCounters(*IN_LIMITS) for _ in range(n)]
    trk = CurriculumTracker(_StandIn(n), initial_max_ante=1, ante_increment=1, success_threshold=0.8, window=2)
    calls = []
    for c in range(IN_CALLS):
        acts, want = np.zeros((K, n), np.int32), np.zeros((K, n, 352), np.uint8)
        raised = np.zeros(n, bool)
        for j in range(K):
            t = c * K + j
            rew, flags, obs, summ, end_ante = np.zeros(n), np.zeros(n, np.uint8), [], np.zeros((n, 8), np.uint8), np.zeros(n, np.int64)
            for i, o in enumerate(orc):
                a = o.policy_action(2, 23, i, t)
                acts[j, i] = a
                ob, r, term, _, _ = o.step(int(a))
                rew[i], flags[i] = cnt[i].step(r, bool(term))
                if flags[i]:
                    summ[i], end_ante[i] = _summary(ob), int(ob["ante"])
                    o.reset(); o.set_jokers(jokers[i])
                obs.append(o.obs())
            raised |= trk.update(flags != 0, end_ante)
            want[j] = _pack({k: np.stack([np.asarray(w[k]) for w in obs]) for k in OBS_KEYS}, rew, acts[j], flags)
            want[j, :, R_END_ANTE:R_END_ANTE + 8] = summ
        for i, o in enumerate(orc):   # the call boundary
            o.set_max_ante(int(trk.cap[i]))
        state = (trk.cap.copy(), trk.hist.T.astype(np.int16), trk.count.copy(), trk.at_level.astype(np.int32), raised)
        for a in (acts, want) + state:
            a.setflags(write=False)
        calls.append((acts, want, state))
    return seeds, jokers, tuple(calls)


def test_curriculum_job_vs_oracle_and_tracker(monkeypatch):
    """step_many(limits=EpisodeLimits(summary=True)) + RowCurriculum.update after each of three calls: the records bit for bit with bytes 344..351,
    and caps, history, counts, levels, raised mask and report exactly the tracker's.  The raised caps reach the library through
    BalatroVecEnv.set_max_ante, so the records of the later calls show antes above the first cap."""
    import torch
    from balatro_gym_amd import EpisodeLimits, RowCurriculum, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers
    _shallow_rings(monkeypatch)
    seeds, jokers, calls = _job()
    n, K = IN_N, IN_K
    # what the job must contain, from the oracle side alone
    ever = np.zeros(n, bool)
    for _, _, state in calls:
        ever |= state[4]
    later = np.concatenate([w for _, w, _ in calls[1:]])
    live_ante = later[:, :, 306:308].copy().view(np.int16)[:, :, 0]
    print(f"envs raised {int(ever.sum())}, reaching cap 3: {int((calls[-1][2][0] >= 3).sum())}, observations with ante >= 2 behind the first call {int((live_ante >= 2).sum())}")
    assert int(ever.sum()) >= 20 and int((live_ante >= 2).sum()) >= 5
    env = _vec(n, seeds, scorer_jokers=True, autoreset=True, max_ante=4)
    env.inject(jokers=jokers, apply_now=True)
    cur = RowCurriculum(env, initial_max_ante=1, ante_increment=1, success_threshold=0.8, window=2)
    rb = RowBuffers(n, env.device, steps=K, row_stride=384)
    lim = EpisodeLimits(n, env.device, *IN_LIMITS, steps=K, row_stride=384, summary=True)
    for c, (acts, want, (cap, hist, count, at_level, raised)) in enumerate(calls):
        poison_(rb.rows)
        env.step_many(torch.from_numpy(np.array(acts)).to(env.device), obs_buffers=rb, limits=lim)
        _diff(f"call {c}: records [step, env, byte]", rb.rows.cpu().numpy()[:, :, :352], want)
        rep = rb.episode_ends(cur)
        _diff(f"call {c}: the report", rep.cpu().numpy(), ref.report(want, int(raised.sum())))
        _diff(f"call {c}: raised", cur.raised.cpu().numpy() != 0, raised)
        got = _state(cur)
        for name, g, w in zip(("cap", "hist", "count", "at_level"), got, (cap, hist, count, at_level)):
            _diff(f"call {c}: {name}", g, w)
        assert rep[nat.ENDS_REPORT["no_summary"]].item() == 0 and rep[nat.ENDS_REPORT["ended"]].item() == int((want[:, :, R_FLAGS] != 0).sum())
    env.check()
    env.close()
