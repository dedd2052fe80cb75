"""bg_demo_append_rows / bg_demo_sample on the MI355X, byte for byte against tests/demo_ref.py over the whole ring, demo_weight, demo_source and
cursor, at the smallest shapes at which each mechanism can go wrong: one partial chunk (5 x 7), a chunk boundary inside a wave's ballot (13 x 96 =
1 chunk + 224 rows), more chunks than one pass of the scan's 256 lanes holds (3 x 100 000 = 293 chunks; the scan takes ONE count per lane and pass),
keep shares 0 / 1 % / 50 % / 100 %, a wrap over three calls, kept > capacity, the stride pairs, weights that are not 16-byte aligned, two calls with
the same bytes, every refusal of the C checks, the draws of bg_demo_sample, and records of a real env through bc_loss."""
import ctypes as C

import numpy as np
import pytest

from tests import demo_ref as ref

pytestmark = pytest.mark.gpu


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _ring_on_device(ring, dw, ds, cursor):
    """A DemoBuffer whose arrays hold the given bytes."""
    import torch
    from balatro_gym_amd import DemoBuffer
    demo = DemoBuffer(ring.shape[0], torch.device("cuda", torch.cuda.current_device()), row_stride=ring.shape[1])
    assert demo.rows.data_ptr() % 128 == 0
    for t, a in ((demo.rows, ring), (demo.weight, dw), (demo.source, ds), (demo.cursor, cursor)):
        t.copy_(torch.from_numpy(a))
    return demo


def _host(demo):
    return {"ring": demo.rows.cpu().numpy(), "weight": demo.weight.cpu().numpy(), "source": demo.source.cpu().numpy(), "cursor": demo.cursor.cpu().numpy()}


def _case(seed, K, N, C_, stride, dstride, share, with_returns, T0=0, special=True, unaligned=False, with_source=True):
    import torch
    store = ref.synthetic_store(seed, K, N, stride)
    w = ref.synthetic_weights(seed, K, N, share, special)
    returns = np.random.default_rng(seed + 3).standard_normal((K, N)) * 7.0 if with_returns else None
    ring, dw, ds, cursor = ref.fresh_ring(seed, C_, dstride)
    cursor[0] = T0
    want = ref.append(store, w, returns, ring, dw, ds if with_source else None, cursor)
    dstore = _dev(store)
    if unaligned:   # the weights one float behind a 16-byte boundary: the kernels take single loads
        buf = torch.zeros(K * N + 1, dtype=torch.float32, device="cuda")
        dw_in = buf[1:].view(K, N)
        dw_in.copy_(torch.from_numpy(w))
        assert dw_in.data_ptr() % 16 == 4 and dw_in.is_contiguous()
    else:
        dw_in = _dev(w)
    what = f"seed {seed} K {K} N {N} C {C_} strides {stride}/{dstride} share {share} returns {with_returns} T0 {T0} unaligned {unaligned}"
    got = []
    for again in range(2):   # two calls on fresh copies of the same inputs: the same bytes
        demo = _ring_on_device(ring, dw, ds, cursor)
        if with_source:
            demo.add(dstore, dw_in, returns=_dev(returns))
        else:   # DemoBuffer always hands its source array over: the C ABI with demo_source_dev NULL
            from balatro_gym_amd import _native as nat
            L, vp, dret = nat.load(), C.c_void_p, _dev(returns)
            ws = torch.zeros(int(L.bg_demo_workspace_bytes(C.c_int64(K * N))), dtype=torch.uint8, device="cuda")
            rc = L.bg_demo_append_rows(vp(dstore.data_ptr()), C.c_uint64(stride), K, C.c_int64(N), vp(dw_in.data_ptr()), vp(None if dret is None else dret.data_ptr()),
                                       vp(demo.rows.data_ptr()), C.c_uint64(dstride), C.c_int64(C_), vp(demo.weight.data_ptr()), None, vp(demo.cursor.data_ptr()),
                                       vp(ws.data_ptr()), C.c_uint64(ws.numel()), None, vp(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, L.bg_last_error(None).decode()
            torch.cuda.synchronize()
        got.append(_host(demo))
        ref.assert_same(got[-1], want, f"{what} call {again}")
        assert with_source or np.array_equal(got[-1]["source"], ds), "a source array that was not handed over was written"
    assert np.array_equal(dstore.cpu().numpy(), store), "the store was written"
    return want


@pytest.mark.parametrize("K,N", [(5, 7), (13, 96)])
def test_small_shapes_at_every_stride_pair(K, N):
    for stride in (352, 384):
        for dstride in (352, 384):
            for with_returns in (False, True):
                want = _case(K + N, K, N, 2048, stride, dstride, 0.5, with_returns)
                assert 0 < int(want["cursor"][1]) < K * N
    _case(K + N + 1, K, N, 2048, 384, 384, 0.5, True, unaligned=True)


def test_without_a_source_array_and_from_a_negative_count():
    """demo_source_dev NULL: ring, weights and cursor are the reference's and the array is not touched.  cursor[0] < 0 is taken as an empty ring."""
    for K, N, C_, share in ((5, 7, 64, 0.5), (13, 96, 100, 0.7)):
        _case(20 + K, K, N, C_, 384, 352, share, True, with_source=False)
        want = _case(21 + K, K, N, C_, 352, 384, share, False, T0=-5)
        assert int(want["cursor"][0]) == int(want["cursor"][1])


@pytest.mark.parametrize("share", [0.0, 0.01, 0.5, 1.0])
def test_keep_shares(share):
    K, N = 13, 96
    want = _case(70, K, N, 2000, 384, 384, share, True, T0=17, special=share < 1.0)
    kept = int(want["cursor"][1])
    assert kept == 0 if share == 0.0 else kept == K * N if share == 1.0 else 0 < kept < K * N
    assert int(want["cursor"][0]) == 17 + kept


def test_more_chunks_than_one_scan_pass():
    """3 x 100 000 candidate rows = 293 chunks of 1 024: the scan workgroup takes one chunk count per lane, 256 per pass, so the second pass and its
    carry run.  About 2 % of the rows are kept (the reference loops over the kept rows in Python); a ring smaller than that also drops the first."""
    K, N = 3, 100_000
    assert (K * N + 1023) // 1024 == 293
    want = _case(80, K, N, 8192, 384, 384, 0.02, False)
    assert int(want["cursor"][1]) > 256 * 1024 // 50 // 2
    want = _case(81, K, N, 1000, 384, 352, 0.02, True, T0=999)
    assert int(want["cursor"][1]) > 1000 and sorted(want["written"]) == list(range(1000))


def test_three_chained_calls_wrap_the_ring():
    C_ = 700
    ring, dw, ds, cursor = ref.fresh_ring(40, C_, 384)
    demo = _ring_on_device(ring, dw, ds, cursor)
    wn = {"ring": ring, "weight": dw, "source": ds, "cursor": cursor}
    total = 0
    for call, (K, N) in enumerate([(5, 97), (3, 130), (4, 101)]):
        store = ref.synthetic_store(41 + call, K, N, 352)
        w = ref.synthetic_weights(41 + call, K, N, 0.6)
        wn = ref.append(store, w, None, wn["ring"], wn["weight"], wn["source"], wn["cursor"])
        ms = demo.add(_dev(store), _dev(w), timing=True)
        assert ms > 0.0
        ref.assert_same(_host(demo), wn, f"call {call}")
        total += int(wn["cursor"][1])
    assert total > C_ and len(demo) == C_ and demo.filled() == C_
    # an empty call is a no-op; clear() empties the ring
    before = _host(demo)
    assert demo.add(_dev(np.zeros((3, 0, 352), np.uint8)), _dev(np.zeros((2, 0), np.float32))) is None
    ref.assert_same(_host(demo), before, "empty call")
    demo.clear()
    assert len(demo) == 0


@pytest.mark.parametrize("C_,K,N,share", [(100, 5, 97, 0.7), (1, 5, 7, 0.5), (1248, 13, 96, 1.0), (37, 2, 1100, 1.0)])
def test_more_kept_rows_than_slots(C_, K, N, share):
    for T0 in (0, 3 * C_ + 2):
        want = _case(50 + C_, K, N, C_, 384, 352, share, False, T0=T0, special=share < 1.0)
        assert int(want["cursor"][1]) >= C_ and sorted(want["written"]) == list(range(C_))


def test_c_checks_refuse_before_any_launch():
    import torch
    from balatro_gym_amd import _native as nat
    L = nat.load()
    K, N, stride, cap = 4, 9, 384, 16
    store = _dev(ref.synthetic_store(1, K, N, stride))
    big = torch.zeros((K + 1) * N * stride + cap * stride + 64, dtype=torch.uint8, device="cuda")   # a store with a ring inside it, for the overlap
    w, w2 = _dev(ref.synthetic_weights(1, K, N, 0.5)), torch.zeros(K * N + 4, dtype=torch.float32, device="cuda")
    ret = torch.zeros(K * N + 2, dtype=torch.float64, device="cuda")
    ring = torch.full((cap * stride + 64,), 7, dtype=torch.uint8, device="cuda")
    dw, src = torch.full((cap + 4,), 5.0, dtype=torch.float32, device="cuda"), torch.zeros(cap + 4, dtype=torch.int32, device="cuda")
    cur = torch.zeros(4, dtype=torch.int64, device="cuda")
    need = int(L.bg_demo_workspace_bytes(C.c_int64(K * N)))
    assert need == 32 and int(L.bg_demo_workspace_bytes(C.c_int64(0))) == 0 and int(L.bg_demo_workspace_bytes(C.c_int64(300_000))) == 16 + 4 * 293 + 12
    ws = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    off = (-ring.data_ptr()) % 16
    good = dict(rows=store.data_ptr(), stride=stride, K=K, N=N, w=w.data_ptr(), ret=None, demo=ring.data_ptr() + off, dstride=stride, cap=cap, dw=dw.data_ptr(),
                src=src.data_ptr(), cur=cur.data_ptr(), ws=ws.data_ptr(), wsb=need)

    def call(**over):
        a = dict(good)
        a.update(over)
        vp = C.c_void_p
        return L.bg_demo_append_rows(vp(a["rows"]), C.c_uint64(a["stride"]), a["K"], C.c_int64(a["N"]), vp(a["w"]), vp(a["ret"]), vp(a["demo"]), C.c_uint64(a["dstride"]),
                                     C.c_int64(a["cap"]), vp(a["dw"]), vp(a["src"]), vp(a["cur"]), vp(a["ws"]), C.c_uint64(a["wsb"]), None,
                                     vp(torch.cuda.current_stream().cuda_stream))
    assert call() == 0 and call(src=None) == 0 and call(ret=ret.data_ptr()) == 0
    torch.cuda.synchronize()
    state = [t.clone() for t in (ring, dw, src, cur)]
    bad = [dict(K=0), dict(K=-1), dict(N=-1), dict(K=2 ** 20, N=2 ** 11), dict(cap=0), dict(cap=2 ** 31), dict(stride=344), dict(stride=360), dict(dstride=336),
           dict(dstride=360), dict(rows=store.data_ptr() + 8), dict(demo=ring.data_ptr() + off + 8), dict(rows=None), dict(w=None), dict(demo=None), dict(dw=None),
           dict(cur=None), dict(ws=None), dict(ws=ws.data_ptr() + 8), dict(wsb=need - 1), dict(w=w.data_ptr() + 2), dict(ret=ret.data_ptr() + 4),
           dict(cur=cur.data_ptr() + 4), dict(src=src.data_ptr() + 2), dict(dw=dw.data_ptr() + 2),
           dict(rows=big.data_ptr() + (-big.data_ptr()) % 16, demo=big.data_ptr() + (-big.data_ptr()) % 16 + 2 * stride),     # the ring inside the store
           dict(demo=store.data_ptr() + (K + 1) * N * stride - 16),                                                          # the ring begins in the store's last record
           dict(dw=w.data_ptr()), dict(src=w.data_ptr()), dict(cur=ret.data_ptr(), ret=ret.data_ptr()), dict(ws=cur.data_ptr()), dict(dw=src.data_ptr())]
    for over in bad:
        assert call(**over) == -1, over
        assert L.bg_last_error(None).decode().startswith("bg_demo_append_rows: "), over
    assert call(N=0) == 0 and call(N=0, K=0) == 0   # an empty shape: a no-op
    torch.cuda.synchronize()
    for t, s in zip((ring, dw, src, cur), state):
        assert torch.equal(t, s), "a refused or empty call wrote"
    # bg_demo_sample
    idx = torch.full((8,), 77, dtype=torch.int32, device="cuda")

    def sample(**over):
        a = dict(cur=cur.data_ptr(), cap=cap, idx=idx.data_ptr(), m=4)
        a.update(over)
        return L.bg_demo_sample(C.c_void_p(a["cur"]), C.c_int64(a["cap"]), C.c_uint64(1), C.c_uint64(0), C.c_uint64(0), C.c_void_p(a["idx"]), C.c_int64(a["m"]), None,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert sample() == 0
    for over in (dict(cur=None), dict(idx=None), dict(cap=0), dict(cap=2 ** 31), dict(m=-1), dict(cur=cur.data_ptr() + 4), dict(idx=idx.data_ptr() + 2),
                 dict(idx=cur.data_ptr())):
        assert sample(**over) == -1, over
        assert L.bg_last_error(None).decode().startswith("bg_demo_sample: "), over
    idx.fill_(77)
    assert sample(m=0) == 0
    torch.cuda.synchronize()
    assert (idx == 77).all()


def test_sample_is_the_reference():
    import torch
    from balatro_gym_amd import DemoBuffer
    cap = 1000
    demo = DemoBuffer(cap, torch.device("cuda", torch.cuda.current_device()))
    for total in (0, 1, 5, cap, 3 * cap + 1):
        demo.cursor[0] = total
        filled = min(total, cap)
        assert demo.filled() == filled and len(demo) == filled
        for seed, index0, t, m in ((0, 0, 0, 1), (1234567, 10, 3, 257), (2 ** 64 - 1, 2 ** 40, 2 ** 63, 1024)):
            got = demo.sample(m, seed=seed, t=t, index0=index0)
            assert got.dtype == torch.int32 and tuple(got.shape) == (m,)
            assert np.array_equal(got.cpu().numpy(), ref.sample(total, cap, seed, index0, t, m)), (total, seed)
        # the same (seed, index0 + i, t) gives the same draw whatever m
        a, (b, ms) = demo.sample(300, seed=9, t=4), demo.sample(50, seed=9, t=4, index0=100, timing=True)
        assert torch.equal(a[100:150], b) and ms > 0.0
    assert tuple(demo.sample(0, seed=1, t=0).shape) == (0,)
    # an empty ring's -1 is the index bc_loss excludes
    demo.clear()
    assert (demo.sample(64, seed=3, t=1) == -1).all()


def test_state_dict_round_trip():
    import torch
    from balatro_gym_amd import DemoBuffer
    dev = torch.device("cuda", torch.cuda.current_device())
    K, N = 5, 97
    a, b = DemoBuffer(300, dev), DemoBuffer(300, dev)
    a.add(_dev(ref.synthetic_store(3, K, N, 384)), _dev(ref.synthetic_weights(3, K, N, 0.5)))
    b.load_state_dict(a.state_dict())
    ref.assert_same(_host(b), _host(a), "state_dict")
    with pytest.raises(ValueError, match="the state is of a ring"):
        DemoBuffer(301, dev).load_state_dict(a.state_dict())


def test_real_records_through_bc_loss():
    """64 envs, 48 steps of masked uniform actions (sample_actions on zero logits under the record's mask) under EpisodeLimits(max_episode_steps=20, summary=True), one step per call,
    into a [K + 1, N] store.  Kept: the steps whose distance to their episode's end is a multiple of 3 (`steps_to_end[1:] % 3 == 0`; an open episode's -1
    is not).  Why that keeps between 10 % and 90 %: the step limit closes every episode within 20 steps, so at most the last 19 of the 48 steps of an env are
    open and at least 29 / 48 of the rows are closed; an episode of L steps keeps ceil(L / 3) of them, at least a third, so the share is >= 0.2; a game
    needs four played hands of at least two steps each to be lost, so L >= 8 and no episode keeps more than 3 / 8.
    bc_loss over the store (weights, index = the kept flat indices ascending) and over the demo ring (demo.weight, demo.actions, index = arange(kept))
    on the same logits walk the same rows in the same reduction order: every output is bit-identical."""
    import torch
    from balatro_gym_amd import BalatroVecEnv, DemoBuffer, EpisodeLimits, bc_loss, episode_outcomes, sample_actions
    from balatro_gym_amd.vec_env import RowBuffers
    n, K = 64, 48
    env = BalatroVecEnv(n, [4100 + i for i in range(n)], scorer_jokers=True, autoreset=True, obs_layout="rows")
    dev = env.device
    one = RowBuffers(n, dev, steps=1, row_stride=384)
    lim = EpisodeLimits(n, dev, max_invalid_actions=50, max_episode_steps=20, steps=1, row_stride=384, summary=True)
    store = torch.zeros((K + 1, n, 384), dtype=torch.uint8, device=dev)
    store[0].copy_(env.obs_rows)
    zeros = torch.zeros((n, 60), device=dev)
    for t in range(K):
        a = sample_actions(zeros, store[t], seed=11, t=t)[0]   # uniform over the actions the observation record's own mask allows
        env.step_many(a[None], obs_buffers=one, limits=lim)
        store[t + 1].copy_(one.rows[0])
    env.check()
    out = episode_outcomes(store, gamma=0.99)
    weights = (out.steps_to_end[1:] % 3 == 0).float() * 0.5 + (out.steps_to_end[1:] % 6 == 0).float()   # 0, 0.5 or 1.5
    returns = out.returns[1:].contiguous()
    kept_idx = torch.nonzero(weights.reshape(-1) > 0).reshape(-1).to(torch.int32)
    kept = int(kept_idx.numel())
    share = kept / (K * n)
    print(f"kept {kept} of {K * n} rows: share {share:.3f}")
    assert 0.10 <= share <= 0.90
    # what the docstring's bound rests on, checked on the records: no episode is shorter than 8 steps or longer than the limit's 20
    done = (store[1:, :, 342] != 0).cpu().numpy()
    lengths = np.concatenate([np.diff(np.concatenate([[-1], np.flatnonzero(done[:, e])])) for e in range(n)])
    print(f"{lengths.size} episodes end inside the rollout: {int(lengths.min())} to {int(lengths.max())} steps")
    assert lengths.size >= 2 * n and 8 <= int(lengths.min()) and int(lengths.max()) <= 20
    demo = DemoBuffer(K * n, dev)
    demo.add(store, weights, returns=returns)
    assert len(demo) == kept and int(demo.cursor[1]) == kept
    first = torch.zeros_like(store[0]).copy_(store[0])
    rb = RowBuffers(n, dev, steps=K, row_stride=384)
    rb.rows.copy_(store[1:])
    other = DemoBuffer(K * n, dev)
    rb.to_demo(other, first, weights, returns=returns)
    assert torch.equal(other.rows, demo.rows) and torch.equal(other.weight, demo.weight) and torch.equal(other.cursor, demo.cursor)
    # the ring against the reference, on the real records
    want = ref.append(store.cpu().numpy(), weights.cpu().numpy(), returns.cpu().numpy(), np.zeros((K * n, 384), np.uint8), np.zeros(K * n, np.float32),
                      np.full(K * n, -1, np.int32), np.zeros(2, np.int64))
    ref.assert_same({"ring": demo.rows.cpu().numpy(), "weight": demo.weight.cpu().numpy(), "source": demo.source.cpu().numpy(), "cursor": demo.cursor.cpu().numpy()},
                    want, "real records")
    assert torch.equal(demo.source[:kept], kept_idx) and torch.equal(demo.returns[:kept], returns.reshape(-1)[kept_idx.long()])
    actions = store[1:, :, 172:176].view(torch.int32)[:, :, 0]
    assert torch.equal(demo.actions[:kept], actions.reshape(-1)[kept_idx.long()])
    logits = torch.from_numpy(np.random.default_rng(5).standard_normal((kept, 60)).astype(np.float32) * 2.0).to(dev)
    loss_s, st_s = bc_loss(logits, actions, store[:K], weights=weights, index=kept_idx, ent_coef=0.01)
    loss_d, st_d = bc_loss(logits, demo.actions, demo.rows, weights=demo.weight, index=torch.arange(kept, dtype=torch.int32, device=dev), ent_coef=0.01)
    env.close()
    bits = lambda x: x.cpu().numpy().view(np.uint32)   # noqa: E731
    assert float(st_s.excluded) == 0.0 and float(st_d.excluded) == 0.0
    assert float(st_s.weight_sum) > 0.0 and np.isfinite(float(loss_s))
    for name in ("raw", "dlogits", "log_prob", "entropy"):
        assert np.array_equal(bits(getattr(st_s, name)), bits(getattr(st_d, name))), name
    assert np.array_equal(bits(loss_s.reshape(1)), bits(loss_d.reshape(1)))
