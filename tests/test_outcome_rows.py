"""bg_episode_outcome_rows on the MI355X, bit for bit against the numpy loop of tests/outcome_ref.py: the synthetic records of the host test (random
bytes, strides 352 and 384, K in {1, 15, 16, 17, 33}, N in {1, 63, 64, 65, 130}, with and without tails and dense rewards, gamma 1.0 and 0.99, an env
that never ends, one that ends on every step, endings at t = 0 and t = K - 1), every subset of the outputs through the C ABI between poisoned guards,
chunked calls chained through `.tail()`, two calls with the same bits, every refusal of the C checks, and one real rollout (N = 128, K = 64, step limit
20, episode summary on) whose records are copied back and run through the numpy loop."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import outcome_ref as ref

pytestmark = pytest.mark.gpu

KS, NS, STRIDES = (1, 15, 16, 17, 33), (1, 63, 64, 65, 130), (352, 384)
T_FIELDS = {"steps_to_end": "int32", "end_ante": "int32", "end_flags": "uint8", "returns": "float64"}


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _host(o):
    return {f: getattr(o, f).cpu().numpy() for f in ref.FIELDS if getattr(o, f) is not None}


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("K", KS)
def test_kernel_is_the_numpy_loop(K, stride):
    from balatro_gym_amd import episode_outcomes
    for N in NS:
        for kind0 in ((None,) if N >= 4 else ref.KINDS):
            rows = ref.synthetic_rows(K * 1000 + N + stride, K, N, stride, kind0)
            drows = _dev(rows)
            rewards = np.random.default_rng(K + N).standard_normal((K, N)) * 3.0
            for gamma, tail, rw in itertools.product((1.0, 0.99), (None, ref.synthetic_tail(K + N, N)), (None, rewards)):
                what = f"K {K} N {N} stride {stride} kind0 {kind0} gamma {gamma} tail {tail is not None} rewards {rw is not None}"
                got = episode_outcomes(drows, gamma, rewards=_dev(rw), tail=None if tail is None else {f: _dev(v) for f, v in tail.items()})
                ref.assert_equal_bits(_host(got), ref.outcome_loop(rows, gamma, rw, tail), what)
            assert np.array_equal(drows.cpu().numpy(), rows), "the records were written"


def test_every_subset_of_the_outputs_between_guards():
    """The C ABI with each non-empty subset of the four outputs (the others NULL), K = 33, N = 130: the outputs asked for are the loop's, the elements
    in front of and behind each stay poisoned, two calls give the same bits."""
    import torch
    from balatro_gym_amd import _native as nat
    L = nat.load()
    K, N, stride = 33, 130, 384
    rows = ref.synthetic_rows(5, K, N, stride)
    tail = ref.synthetic_tail(5, N)
    want = ref.outcome_loop(rows, 0.99, None, tail)
    drows = _dev(rows)
    dtail = {f: _dev(v) for f, v in tail.items()}
    vp = C.c_void_p
    for r in range(1, 5):
        for sub in itertools.combinations(ref.FIELDS, r):
            bufs = {f: torch.full((K * N + 16,), 77, dtype=getattr(torch, T_FIELDS[f]), device="cuda") for f in sub}
            ptr = lambda f, b: vp(b[f][8:].data_ptr()) if f in b else None   # noqa: E731
            for again in range(2):
                rc = L.bg_episode_outcome_rows(vp(drows.data_ptr()), C.c_uint64(stride), K, C.c_int64(N), C.c_double(0.99), None,
                                               *(vp(dtail[f].data_ptr()) if f in sub else None for f in ref.FIELDS), *(ptr(f, bufs) for f in ref.FIELDS),
                                               None, vp(torch.cuda.current_stream().cuda_stream))
                assert rc == 0, L.bg_last_error(None).decode()
                torch.cuda.synchronize()
                got = {f: bufs[f][8:8 + K * N].cpu().numpy().reshape(K, N) for f in sub}
                ref.assert_equal_bits(got, want, f"outputs {sub}", fields=sub)
                for f in sub:
                    edge = torch.cat([bufs[f][:8], bufs[f][8 + K * N:]]).cpu().numpy()
                    assert (edge == 77).all(), f"outputs {sub}: guard elements of {f} were written"


def test_chunks_chained_through_tail():
    from balatro_gym_amd import episode_outcomes
    K, N = 33, 65
    rows = ref.synthetic_rows(91, K, N, 384, p_end=0.08)
    drows = _dev(rows)
    whole = _host(episode_outcomes(drows, 0.99))
    ref.assert_equal_bits(whole, ref.outcome_loop(rows, 0.99), "whole")
    for cuts in ((5,), (1, 16, 17), (32,)):
        bounds = [0, *cuts, K]
        tail, parts = None, []
        for a, b in reversed(list(zip(bounds[:-1], bounds[1:]))):
            got = episode_outcomes(drows[a:b], 0.99, tail=tail)
            tail = got.tail()
            parts.insert(0, _host(got))
        ref.assert_equal_bits({f: np.concatenate([p[f] for p in parts]) for f in ref.FIELDS}, whole, f"chunks at {cuts}")
    # want= a subset, with timing; an empty shape launches nothing
    o = episode_outcomes(drows, 1.0, want=("end_ante", "steps_to_end"), timing=True)
    assert o.returns is None and o.end_flags is None and o.kernel_ms > 0.0 and sorted(o.tail()) == ["end_ante", "steps_to_end"]
    ref.assert_equal_bits(_host(o), ref.outcome_loop(rows, 1.0), "subset", fields=("end_ante", "steps_to_end"))
    e = episode_outcomes(drows[:0])
    assert tuple(e.returns.shape) == (0, N)


def test_c_checks_refuse_before_any_launch():
    import torch
    from balatro_gym_amd import _native as nat
    L = nat.load()
    K, N, stride = 4, 9, 384
    rows = _dev(ref.synthetic_rows(1, K, N, stride))
    i32 = torch.zeros(K * N + 4, dtype=torch.int32, device="cuda")
    i32b = torch.zeros(K * N + 4, dtype=torch.int32, device="cuda")
    u8 = torch.zeros(K * N + 4, dtype=torch.uint8, device="cuda")
    f64 = torch.full((K * N + 4,), 5.0, dtype=torch.float64, device="cuda")
    f64b = torch.zeros(K * N + 4, dtype=torch.float64, device="cuda")
    good = dict(rows=rows.data_ptr(), stride=stride, K=K, N=N, gamma=0.99, rewards=None, ts=None, ta=None, tf=None, tr=None, steps=i32.data_ptr(),
                ante=i32b.data_ptr(), flags=u8.data_ptr(), ret=f64.data_ptr())

    def call(**over):
        a = dict(good)
        a.update(over)
        vp = C.c_void_p
        return L.bg_episode_outcome_rows(vp(a["rows"]), C.c_uint64(a["stride"]), a["K"], C.c_int64(a["N"]), C.c_double(a["gamma"]), vp(a["rewards"]), vp(a["ts"]),
                                         vp(a["ta"]), vp(a["tf"]), vp(a["tr"]), vp(a["steps"]), vp(a["ante"]), vp(a["flags"]), vp(a["ret"]), None,
                                         vp(torch.cuda.current_stream().cuda_stream))
    assert call() == 0
    bad = [dict(rows=None), dict(rows=rows.data_ptr() + 8), dict(stride=344), dict(stride=360), dict(K=-1), dict(N=-1),
           dict(steps=None, ante=None, flags=None, ret=None), dict(steps=None, ts=i32b.data_ptr()), dict(ante=None, ta=i32.data_ptr()),
           dict(flags=None, tf=u8.data_ptr()), dict(ret=None, tr=f64b.data_ptr()), dict(ret=None, rewards=f64b.data_ptr()), dict(gamma=float("nan")),
           dict(steps=i32.data_ptr() + 2), dict(ta=i32.data_ptr() + 2), dict(ret=f64.data_ptr() + 4), dict(rewards=f64b.data_ptr() + 4),
           dict(tr=f64b.data_ptr() + 4), dict(ante=i32.data_ptr()), dict(rewards=f64.data_ptr()), dict(ts=i32.data_ptr()), dict(tr=f64.data_ptr())]
    f64.fill_(5.0)
    for over in bad:
        assert call(**over) == -1, over
        assert L.bg_last_error(None).decode().startswith("bg_episode_outcome_rows: "), over
    torch.cuda.synchronize()
    # K == 0 / N == 0: a no-op that writes nothing
    f64.fill_(5.0)
    assert call(K=0) == 0 and call(N=0) == 0
    torch.cuda.synchronize()
    assert (f64 == 5.0).all()


def test_real_rollout_has_open_and_closed_segments():
    """128 envs, 64 steps of random actions under EpisodeLimits(max_invalid_actions=50, max_episode_steps=20, summary=True): the step limit ends at
    least three episodes per env inside the call, the steps in front of the first ending and behind the last belong to segments open at one end.  The
    records are copied back and run through the numpy loop; RowBuffers.outcomes must give its bits, and the filter built from it is the reference's."""
    import torch
    from balatro_gym_amd import BalatroVecEnv, EpisodeLimits
    from balatro_gym_amd.vec_env import RowBuffers
    n, K = 128, 64
    env = BalatroVecEnv(n, [900 + i for i in range(n)], scorer_jokers=True, autoreset=True)
    rb = RowBuffers(n, env.device, steps=K, row_stride=384)
    lim = EpisodeLimits(n, env.device, max_invalid_actions=50, max_episode_steps=20, steps=K, row_stride=384, summary=True)
    acts = torch.from_numpy(np.random.default_rng(3).integers(0, 60, (K, n)).astype(np.int32)).to(env.device)
    env.step_many(acts, obs_buffers=rb, limits=lim)
    env.check()
    got = rb.outcomes(0.99)
    again = rb.outcomes(0.99)
    rows = rb.rows.cpu().numpy()
    env.close()
    want = ref.outcome_loop(rows, 0.99)
    ref.assert_equal_bits(_host(got), want, "real rollout")
    ref.assert_equal_bits(_host(again), _host(got), "two calls")
    done = rows[:, :, ref.OFF_TERM] != 0
    assert (done.sum(axis=0) >= 3).all(), "the step limit ends at least three episodes per env"
    steps = want["steps_to_end"]
    open_, closed = steps < 0, steps >= 0
    assert open_.any() and closed.any() and open_[-1].any() and closed[0].all()
    assert (want["end_ante"][closed] >= 1).all() and (want["end_flags"][closed] != 0).all(), "the summary and the end flags of ended records"
    assert (want["end_ante"][open_] == -1).all() and (want["end_flags"][open_] == 0).all()
    # a closed step's outcome is the record `steps_to_end` steps later
    t, e = np.nonzero(closed)
    end = t + steps[t, e]
    assert done[end, e].all() and np.array_equal(want["end_ante"][t, e], rb_end_ante(rows)[end, e])
    w = (got.end_ante >= 5).float()
    assert tuple(w.shape) == (K, n) and w.dtype == torch.float32


def rb_end_ante(rows):
    return ref.fields_of(rows)[3].astype(np.int32)
