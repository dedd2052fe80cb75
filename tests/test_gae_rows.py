"""bg_gae_rows / bg_episode_stats_rows on the MI355X: records the product writes (step_many at both strides, a fused rollout, three consecutive step_many
calls) and the synthetic set of tests/test_gae_rows_host.py; records and outputs are copied to the host and compared, bit for bit over every element, with
the numpy restatement of tests/gae_ref.py over the host copy of the same record bytes (never with torch arithmetic on the GPU).  Every output sits between
poisoned guard elements; bad arguments return BG_E_ARG and launch nothing."""
import ctypes as C

import numpy as np
import pytest

from tests import gae_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64
POISON32 = 0xA5A5A5A5 - (1 << 32)   # as int32
POISON64 = 0xA5A5A5A5A5A5A5A5 - (1 << 64)   # as int64


def _guarded(K, N, dtype):
    """A poisoned flat device buffer with GUARD elements before and after a contiguous [K, N] view of `dtype` -> (flat, view)."""
    import torch
    flat = torch.empty(K * N + 2 * GUARD, dtype=dtype, device="cuda")
    if dtype == torch.float64:
        flat.view(torch.int64).fill_(POISON64)
    else:
        flat.view(torch.int32).fill_(POISON32)
    return flat, flat[GUARD:GUARD + K * N].view(K, N)


def _ints(t):
    """float32 / int32 / float64 device tensor -> its bit patterns on the host."""
    import torch
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64).cpu().numpy().view(np.uint64)
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _guards_intact(flat, K, N):
    g = _ints(flat)
    p = np.uint64(0xA5A5A5A5A5A5A5A5) if g.dtype == np.uint64 else np.uint32(0xA5A5A5A5)
    return bool((g[:GUARD] == p).all() and (g[GUARD + K * N:] == p).all())


def _diff(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} elements differ, first (t, env) {tuple(bad[0])}: {got[tuple(bad[0])]:#x} != {want[tuple(bad[0])]:#x}"


def _check_gae(rows_dev, values, last_values, gamma, lam, what):
    """rows_dev uint8 [K, N, stride] on the device; values / last_values float32 numpy.  Advantages and returns against numpy over the host copy of the records."""
    import torch
    from balatro_gym_amd import gae_rows
    K, N, _ = rows_dev.shape
    reward, done = ref.unpack_records(rows_dev.cpu().numpy())
    want_a, want_r = ref.gae(reward, done, values, last_values, gamma, lam)
    fa, adv = _guarded(K, N, torch.float32)
    fr, ret = _guarded(K, N, torch.float32)
    v, lv = torch.from_numpy(values).cuda(), torch.from_numpy(last_values).cuda()
    ga, gr = gae_rows(rows_dev, v, lv, gamma, lam, advantages=adv, returns=ret)
    assert ga.data_ptr() == adv.data_ptr() and gr.data_ptr() == ret.data_ptr()
    _diff(_ints(adv), ref.bits32(want_a), f"{what} advantages")
    _diff(_ints(ret), ref.bits32(want_r), f"{what} returns")
    assert _guards_intact(fa, K, N) and _guards_intact(fr, K, N), f"{what}: guard elements were written"
    assert np.array_equal(_ints(v), ref.bits32(values)) and np.array_equal(_ints(lv), ref.bits32(last_values)), f"{what}: inputs were written"
    return reward, done


def _check_eps(rows_dev, what, split=None):
    """EpisodeStats over rows_dev in one call (or two, split at `split`) against the numpy scan; guards; the step count is conserved."""
    import torch
    from balatro_gym_amd import EpisodeStats
    K, N, _ = rows_dev.shape
    reward, done = ref.unpack_records(rows_dev.cpu().numpy())
    want_r, want_l, want_cr, want_cl = ref.episode_stats(reward, done)
    st = EpisodeStats(N, rows_dev.device)
    fr, er = _guarded(K, N, torch.float64)
    fl, el = _guarded(K, N, torch.int32)
    if split is None:
        st.update(rows_dev, ep_return=er, ep_len=el)
    else:
        st.update(rows_dev[:split], ep_return=er[:split], ep_len=el[:split])
        st.update(rows_dev[split:], ep_return=er[split:], ep_len=el[split:])
    _diff(_ints(er), ref.bits64(want_r), f"{what} ep_return")
    _diff(_ints(el).view(np.int32), want_l, f"{what} ep_len")
    assert np.array_equal(_ints(st.ep_return_carry), ref.bits64(want_cr)) and np.array_equal(st.ep_len_carry.cpu().numpy(), want_cl), f"{what}: carries"
    assert _guards_intact(fr, K, N) and _guards_intact(fl, K, N), f"{what}: guard elements were written"
    assert int(want_l.sum()) + int(want_cl.sum()) == K * N and int(el.sum()) + int(st.ep_len_carry.sum()) == K * N


def _env(n, **kw):
    from balatro_gym_amd import BalatroVecEnv
    return BalatroVecEnv(n, [900 + i for i in range(n)], scorer_jokers=True, autoreset=True, **kw)


def _warm(env, steps=400):
    """Run the envs `steps` steps under the uniform policy so that episodes end inside the windows that follow."""
    from balatro_gym_amd.vec_env import RowBuffers
    env.rollout(steps, policy=0, policy_seed=11, obs_buffers=RowBuffers(env.num_envs, env.device, steps=1))
    env.check()


def _values(K, N, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((K, N)).astype(np.float32) * 10.0, rng.standard_normal(N).astype(np.float32) * 10.0


def test_real_records_rollout_and_step_many():
    """4 096 envs, >= 400 steps in: a fused rollout of max_fused_steps, then its actions replayed through step_many (several launches) at both strides."""
    import torch
    from balatro_gym_amd.vec_env import RowBuffers
    n = 4096
    env = _env(n, fused_steps=8)
    _warm(env)
    T = env.max_fused_steps
    rb = RowBuffers(n, env.device, steps=T, row_stride=384)
    env.rollout(T, policy=0, policy_seed=12, obs_buffers=rb)
    env.check()
    v, lv = _values(T, n, 1)
    _, done = _check_gae(rb.rows, v, lv, 0.99, 0.95, "rollout")
    print(f"rollout window: {int(done.sum())} terminated steps of {done.size}")
    assert int(done.sum()) >= 32
    _check_eps(rb.rows, "rollout")
    # RowBuffers.gae / .episode_stats are the same calls
    from balatro_gym_amd import EpisodeStats, gae_rows
    tv, tlv = torch.from_numpy(v).cuda(), torch.from_numpy(lv).cuda()
    a1, r1 = rb.gae(tv, tlv, 0.95, 0.9)
    a2, r2, ms = gae_rows(rb.rows, tv, tlv, 0.95, 0.9, timing=True)
    assert torch.equal(a1.view(torch.int32), a2.view(torch.int32)) and torch.equal(r1.view(torch.int32), r2.view(torch.int32)) and ms > 0.0
    s1, s2 = EpisodeStats(n, env.device), EpisodeStats(n, env.device)
    e1, l1 = rb.episode_stats(s1)
    e2, l2, ms = s2.update(rb.rows, timing=True)
    assert torch.equal(e1.view(torch.int64), e2.view(torch.int64)) and torch.equal(l1, l2) and ms > 0.0
    s1.reset(torch.arange(n, device=env.device) % 2 == 0)
    assert not s1.ep_len_carry[0::2].any() and torch.equal(s1.ep_len_carry[1::2], s2.ep_len_carry[1::2])
    acts = torch.cat([rb.action, rb.action.flip(0), rb.action, rb.action[:5]]).contiguous()
    K = int(acts.shape[0])
    assert K > 3 * T
    for stride in (384, 352):
        rb2 = RowBuffers(n, env.device, steps=K, row_stride=stride)
        env.step_many(acts, obs_buffers=rb2)
        env.check()
        v, lv = _values(K, n, stride)
        _, done = _check_gae(rb2.rows, v, lv, 0.99, 0.95, f"step_many stride {stride}")
        print(f"step_many window, stride {stride}: {int(done.sum())} terminated steps of {done.size}")
        assert int(done.sum()) >= 32
        _check_eps(rb2.rows, f"step_many stride {stride}", split=K // 3)
    env.close()


def test_returns_null_leaves_the_buffer_untouched():
    import torch
    from balatro_gym_amd import _native as nat
    L = nat.load()
    K, N = 17, 130
    reward, done = ref.synthetic_rewards(K, N, 5), ref.synthetic_done(K, N, "random", 5)
    values, last_values = ref.synthetic_values(K, N, 5)
    rows = torch.from_numpy(ref.pack_records(reward, done, 352)).cuda()
    v, lv = torch.from_numpy(values).cuda(), torch.from_numpy(last_values).cuda()
    fa, adv = _guarded(K, N, torch.float32)
    fr, ret = _guarded(K, N, torch.float32)
    rc = L.bg_gae_rows(C.c_void_p(rows.data_ptr()), C.c_uint64(352), K, C.c_int64(N), C.c_void_p(v.data_ptr()), C.c_void_p(lv.data_ptr()), C.c_double(0.99),
                       C.c_double(0.95), C.c_void_p(adv.data_ptr()), None, None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    want_a, _ = ref.gae(reward, done, values, last_values, 0.99, 0.95)
    _diff(_ints(adv), ref.bits32(want_a), "returns_dev NULL: advantages")
    assert bool((fr.view(torch.int32) == POISON32).all()), "a NULL returns_dev still wrote somewhere near the old buffer"
    assert _guards_intact(fa, K, N)
    # the episode scan with one or both outputs NULL still moves the carries
    cr, cl = torch.zeros(N, dtype=torch.float64, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
    fl, el = _guarded(K, N, torch.int32)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.bg_episode_stats_rows(C.c_void_p(rows.data_ptr()), C.c_uint64(352), K, C.c_int64(N), C.c_void_p(cr.data_ptr()), C.c_void_p(cl.data_ptr()), None,
                                   C.c_void_p(el.data_ptr()), None, st) == 0
    torch.cuda.synchronize()
    want_r, want_l, want_cr, want_cl = ref.episode_stats(reward, done)
    assert np.array_equal(el.cpu().numpy(), want_l) and np.array_equal(_ints(cr), ref.bits64(want_cr)) and np.array_equal(cl.cpu().numpy(), want_cl)
    assert _guards_intact(fl, K, N)
    cr.zero_(); cl.zero_()
    assert L.bg_episode_stats_rows(C.c_void_p(rows.data_ptr()), C.c_uint64(352), K, C.c_int64(N), C.c_void_p(cr.data_ptr()), C.c_void_p(cl.data_ptr()), None, None,
                                   None, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_ints(cr), ref.bits64(want_cr)) and np.array_equal(cl.cpu().numpy(), want_cl)


@pytest.mark.parametrize("K", ref.SYN_K)
def test_synthetic(K):
    """The synthetic set of the host test on the device: N in {1, 63, 64, 65, 1000}, every done pattern, float32 ties, rewards that round to float32
    subnormals (the kernel must keep them), +-1e30, values up to 1e6, the five discount pairs, both strides."""
    import torch
    for _, N, pattern, (gamma, lam), stride, seed in [c for c in ref.synthetic_cases() if c[0] == K]:
        reward = ref.synthetic_rewards(K, N, seed)
        done = ref.synthetic_done(K, N, pattern, seed)
        values, last_values = ref.synthetic_values(K, N, seed)
        rows = torch.from_numpy(ref.pack_records(reward, done, stride)).cuda()
        what = f"K {K} N {N} {pattern} gamma {gamma} lambda {lam} stride {stride}"
        _check_gae(rows, values, last_values, gamma, lam, what)
        _check_eps(rows, what, split=None if K < 2 else K // 2)


def test_episode_stats_over_three_step_many_calls():
    """One EpisodeStats updated after each of three consecutive step_many calls equals the numpy scan over the concatenated records; the finished episodes
    it reports are as many as the engine itself counted (bg_rollout_stats.episodes of the three calls) and as the terminated bytes."""
    import torch
    from balatro_gym_amd import EpisodeStats
    from balatro_gym_amd.vec_env import RowBuffers
    n = 4096
    env = _env(n, fused_steps=16)
    _warm(env)
    stats = EpisodeStats(n, env.device)
    g = torch.Generator().manual_seed(7)
    got_r, got_l, recs, engine_episodes = [], [], [], 0
    for K in (16, 7, 40):
        acts = torch.randint(0, 60, (K, n), generator=g, dtype=torch.int32).to(env.device)
        rb = RowBuffers(n, env.device, steps=K, row_stride=384)
        env.step_many(acts, obs_buffers=rb)
        engine_episodes += env.stats()["episodes"]
        er, el = rb.episode_stats(stats)
        got_r.append(_ints(er)); got_l.append(el.cpu().numpy()); recs.append(rb.rows.cpu().numpy())
    env.close()
    reward, done = ref.unpack_records(np.concatenate(recs))
    want_r, want_l, want_cr, want_cl = ref.episode_stats(reward, done)
    got_r, got_l = np.concatenate(got_r), np.concatenate(got_l)
    _diff(got_r, ref.bits64(want_r), "three calls ep_return")
    _diff(got_l, want_l, "three calls ep_len")
    assert np.array_equal(_ints(stats.ep_return_carry), ref.bits64(want_cr)) and np.array_equal(stats.ep_len_carry.cpu().numpy(), want_cl)
    finished = int(np.count_nonzero(got_l))
    print(f"three step_many calls: {finished} finished episodes, the engine counted {engine_episodes}, {int(done.sum())} terminated bytes")
    assert finished == engine_episodes == int(done.sum()) and finished >= 32
    assert int(got_l.sum()) + int(want_cl.sum()) == 63 * n


def test_bad_arguments_launch_nothing():
    """K < 0, misaligned rows_dev, strides 360 and 336, NULL values_dev / advantages_dev / carries: BG_E_ARG with a text, outputs still poisoned."""
    import torch
    from balatro_gym_amd import _native as nat
    L = nat.load()
    K, N = 8, 100
    rows = torch.zeros((K * N + 1, 384), dtype=torch.uint8, device="cuda")
    v, lv = torch.zeros((K, N), device="cuda"), torch.zeros(N, device="cuda")
    fa, adv = _guarded(K, N, torch.float32)
    fr, ret = _guarded(K, N, torch.float32)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ms = C.c_float(-1.0)
    rp = rows.data_ptr()

    def gae(rows_p=rp, stride=384, k=K, n=N, v_p=v.data_ptr(), lv_p=lv.data_ptr(), a_p=adv.data_ptr(), r_p=ret.data_ptr()):
        return L.bg_gae_rows(C.c_void_p(rows_p), C.c_uint64(stride), k, C.c_int64(n), C.c_void_p(v_p), C.c_void_p(lv_p), C.c_double(0.99), C.c_double(0.95),
                             C.c_void_p(a_p), C.c_void_p(r_p), C.byref(ms), st)
    for kw in (dict(k=-1), dict(n=-1), dict(rows_p=rp + 8), dict(rows_p=None), dict(stride=360), dict(stride=336), dict(stride=0), dict(v_p=None), dict(lv_p=None),
               dict(a_p=None), dict(a_p=v.data_ptr()), dict(r_p=v.data_ptr()), dict(r_p=adv.data_ptr()), dict(a_p=adv.data_ptr() + 2)):
        assert gae(**kw) == -1, kw
        assert L.bg_last_error(None).decode().startswith("bg_gae_rows: "), kw
    torch.cuda.synchronize()
    assert bool((fa.view(torch.int32) == POISON32).all()) and bool((fr.view(torch.int32) == POISON32).all()) and ms.value == -1.0
    assert gae(k=0) == 0 and ms.value == 0.0 and gae(n=0) == 0
    torch.cuda.synchronize()
    assert bool((fa.view(torch.int32) == POISON32).all()) and bool((fr.view(torch.int32) == POISON32).all())

    cr, cl = torch.full((N,), 2.5, dtype=torch.float64, device="cuda"), torch.full((N,), 3, dtype=torch.int32, device="cuda")
    fe, er = _guarded(K, N, torch.float64)
    fl, el = _guarded(K, N, torch.int32)
    ms.value = -1.0

    def eps(rows_p=rp, stride=384, k=K, n=N, cr_p=cr.data_ptr(), cl_p=cl.data_ptr(), er_p=er.data_ptr(), el_p=el.data_ptr()):
        return L.bg_episode_stats_rows(C.c_void_p(rows_p), C.c_uint64(stride), k, C.c_int64(n), C.c_void_p(cr_p), C.c_void_p(cl_p), C.c_void_p(er_p), C.c_void_p(el_p),
                                       C.byref(ms), st)
    for kw in (dict(k=-1), dict(n=-1), dict(rows_p=rp + 8), dict(rows_p=None), dict(stride=360), dict(stride=336), dict(cr_p=None), dict(cl_p=None),
               dict(er_p=cr.data_ptr()), dict(el_p=cl.data_ptr()), dict(er_p=er.data_ptr() + 4), dict(cl_p=cl.data_ptr() + 2)):
        assert eps(**kw) == -1, kw
        assert L.bg_last_error(None).decode().startswith("bg_episode_stats_rows: "), kw
    torch.cuda.synchronize()

    def untouched():
        return (bool((fe.view(torch.int64) == POISON64).all()) and bool((fl.view(torch.int32) == POISON32).all()) and bool((cr == 2.5).all()) and bool((cl == 3).all()))
    assert untouched() and ms.value == -1.0
    assert eps(k=0) == 0 and ms.value == 0.0 and eps(n=0) == 0
    torch.cuda.synchronize()
    assert untouched()
    # and the good call: all-zero records are K unterminated steps of reward 0.0
    assert eps() == 0 and ms.value > 0.0
    torch.cuda.synchronize()
    assert bool((er == 0.0).all()) and bool((el == 0).all()) and bool((cr == 2.5).all()) and bool((cl == 3 + K).all())
    assert _guards_intact(fe, K, N) and _guards_intact(fl, K, N)
    assert gae() == 0 and ms.value > 0.0
    torch.cuda.synchronize()
    assert bool((adv == 0.0).all()) and bool((ret == 0.0).all()) and _guards_intact(fa, K, N) and _guards_intact(fr, K, N)
