"""bg_encode_rows_ex on the MI355X: the network input of a shuffled minibatch straight from the stored records.  The store is 200 records (no multiple of the
32-record workgroup) at both strides: the synthetic records of tests/encode_ref.py (every dtype at its limits) for the plain encoding, those of
tests/norm_ref.py for the frozen VecNormalize statistics, and one real 64-env x 8-step rollout.  Outputs are copied to the host and compared there bit
pattern for bit pattern -- the feature adds no arithmetic, so there is no tolerance: with the numpy restatements taken at the index (zero rows where the
index is out of range) and with the existing contiguous calls on records gathered on the host."""
import ctypes as C

import numpy as np
import pytest

from tests import encode_ref as ref, norm_ref

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "bfloat16")
STORE = 200
MS = (1, 31, 32, 33, 97)
INT32_MAX = 2 ** 31 - 1
KW = norm_ref.DEFAULTS


def _bits(t):
    import torch
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _as(dt, bits32):
    return bits32 if dt == "float32" else ref.bf16_bits(bits32)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} elements differ, first (row, column) {tuple(bad[0])}: {got[tuple(bad[0])]:#x} != {want[tuple(bad[0])]:#x}"


def _indices(m, seed):
    """name -> int32 [m]: identity, reversed, random with repeats, one row m times, and a random one with -1 / STORE / INT32_MAX planted at the first and
    last position of a workgroup and at position m - 1."""
    rng = np.random.default_rng(seed)
    planted = rng.integers(0, STORE, m)
    for k, pos in enumerate(sorted({p for p in (0, 31, 32, 63, 64, m - 1) if p < m})):
        planted[pos] = (-1, STORE, INT32_MAX)[(k + m) % 3]
    if m >= 33:
        assert {-1, STORE, INT32_MAX} <= set(planted.tolist())
    return {"identity": np.arange(m), "reversed": STORE - 1 - np.arange(m), "random": rng.integers(0, STORE, m), "same": np.full(m, 137),
            "planted": planted}


def _take(want, idx):
    """Rows of the [STORE, D] reference at idx, zeros where idx is out of range."""
    ok = (idx >= 0) & (idx < len(want))
    out = np.zeros((len(idx), want.shape[1]), want.dtype)
    out[ok] = want[idx[ok]]
    return out


@pytest.fixture(scope="module")
def stores():
    """stride -> (records on the device [STORE, stride], their host copy, layout -> float32 bit patterns [STORE, D]): the reference is computed once."""
    import torch
    obs = ref.synthetic_obs(n_random=STORE - 17)
    assert len(obs["hand"]) == STORE
    want = {layout: ref.expected_bits(layout, obs) for layout in ref.LAYOUTS}
    out = {}
    for stride in (384, 352):
        host = ref.pack_records(obs, stride)
        out[stride] = (torch.from_numpy(host).cuda(), host, want)
    return out


@pytest.fixture(scope="module")
def rollout():
    """One real rollout: RowBuffers of 64 envs x 8 steps at stride 384."""
    from balatro_gym_amd import BalatroVecEnv
    from balatro_gym_amd.vec_env import RowBuffers
    n, K = 64, 8
    env = BalatroVecEnv(n, [900 + i for i in range(n)], scorer_jokers=True, autoreset=True, fused_steps=8)
    rb = RowBuffers(n, env.device, steps=K, row_stride=384)
    done = 0
    while done < K:
        T = min(env.max_fused_steps, K - done)
        part = RowBuffers(n, env.device, steps=T, row_stride=384)
        env.rollout(T, policy=0, policy_seed=11 + done, obs_buffers=part)
        rb.rows[done:done + T].copy_(part.rows)
        done += T
    env.check()
    env.close()
    return rb


@pytest.fixture(scope="module")
def normalizer():
    """(RowNormalizer of 25 envs after three real updates, records [8, 25, stride] per stride on the device and the host)."""
    import torch
    from balatro_gym_amd import RowNormalizer
    N = 25
    nm = RowNormalizer(N, "cuda")
    nm.normalize_obs(torch.from_numpy(norm_ref.synthetic_rows(3, N, 384, 41)).cuda())
    nm.normalize_reward(torch.from_numpy(norm_ref.synthetic_rows(3, N, 384, 41)).cuda())
    assert float(nm.obs_count) > 70 and bool((nm.obs_var != 1.0).any()) and bool((nm.obs_mean != 0.0).any())
    rows = {}
    for stride in (384, 352):
        host = norm_ref.synthetic_rows(STORE // N, N, stride, 42)
        rows[stride] = (torch.from_numpy(host).cuda(), host)
    return nm, rows


def _frozen_reference(nm, rows_host):
    """float32 bit patterns [K * N, 153] of VecNormalize in evaluation mode with the normaliser's statistics (tests/norm_ref.py)."""
    sd = nm.state_dict()
    st = {"obs_mean": sd["obs_mean"].numpy(), "obs_var": sd["obs_var"].numpy(), "obs_count": sd["obs_count"].numpy()[0], "ret_mean": sd["ret_stats"].numpy()[0],
          "ret_var": sd["ret_stats"].numpy()[1], "ret_count": sd["ret_stats"].numpy()[2], "returns": sd["returns"].numpy()}
    want = norm_ref.from_moments(rows_host, None, st, training=False, **KW)
    return norm_ref.obs_bits(want["obs"]).reshape(-1, 153)


def _state_bytes(nm):
    return {k: (v.numpy().tobytes() if hasattr(v, "numpy") else v) for k, v in nm.state_dict().items()}


@pytest.mark.parametrize("stride", [384, 352])
def test_gather_bit_for_bit(stores, stride):
    """Every m x index pattern x layout x dtype: the numpy restatement at the index (zeros where it is out of range), and the existing encode_rows on
    records gathered on the host."""
    import torch
    from balatro_gym_amd import encode_rows
    rows, host, want = stores[stride]
    for m in MS:
        for name, idx in _indices(m, 100 + m).items():
            index = torch.from_numpy(idx.astype(np.int32)).cuda()
            ok = (idx >= 0) & (idx < STORE)
            gathered = torch.from_numpy(host[np.where(ok, idx, 0)]).cuda()
            for layout in ref.LAYOUTS:
                for dt in DTYPES:
                    tdt = getattr(torch, dt)
                    got = encode_rows(rows, layout, tdt, index=index)
                    assert tuple(got.shape) == (m, ref.COLS[layout]) and got.dtype == tdt and got.is_contiguous()
                    g = _bits(got)
                    what = f"stride {stride} m {m} {name} {layout} {dt}"
                    _same(g, _as(dt, _take(want[layout], idx)), what)
                    old = _bits(encode_rows(gathered, layout, tdt))
                    _same(g[ok], old[ok], what + " against encode_rows of host-gathered records")
                    assert not g[~ok].any(), what + ": a row with an out-of-range index is not +0.0"


def test_real_rollout_and_3d_rows(rollout):
    """[K, N, stride] records of a real rollout: index t * N + e names record (t, e); RowBuffers.encode(index=) is the same call."""
    import torch
    from balatro_gym_amd import encode_rows
    rb = rollout
    host = rb.rows.cpu().numpy().reshape(-1, 384)
    rng = np.random.default_rng(3)
    idx = rng.permutation(len(host))[:97]
    index = torch.from_numpy(idx.astype(np.int32)).cuda()
    obs = ref.unpack_records(host[idx])
    for layout in ref.LAYOUTS:
        for dt in DTYPES:
            got = rb.encode(layout, getattr(torch, dt), index=index)
            _same(_bits(got), _as(dt, ref.expected_bits(layout, obs)), f"rollout {layout} {dt}")
            _same(_bits(encode_rows(rb.rows, layout, getattr(torch, dt), index=index)), _bits(got), "encode_rows == RowBuffers.encode")


def test_store_paths_and_untouched_memory(stores, normalizer):
    """The three store paths -- aligned rows, dense unaligned rows (bf16 x 153 among them), an output one element off a 16-byte boundary -- and an odd
    pitch, with and without statistics: the same values, and the sentinel still in the padding columns and in the rows at and beyond m."""
    import torch
    from balatro_gym_amd import encode_rows
    m, extra = 97, 3
    idx = _indices(m, 7)["planted"]
    index = torch.from_numpy(idx.astype(np.int32)).cuda()
    rows, _, want = stores[384]
    nm, nrows = normalizer
    nwant = _frozen_reference(nm, nrows[384][1])
    cases = [(layout, None, want[layout]) for layout in ref.LAYOUTS]
    cases += [("produced", nm, nwant), ("fixed", nm, np.concatenate([nwant, np.zeros((STORE, 628 - 153), np.uint32)], axis=1))]
    for layout, norm, w in cases:
        D = ref.COLS[layout]
        src = rows if norm is None else nrows[384][0]
        for dt in DTYPES:
            tdt = getattr(torch, dt)
            expect = _as(dt, _take(w, idx))
            es = 4 if dt == "float32" else 2
            aligned = (D + 16 + 7) // 8 * 8
            odd = D + 3 if (D + 3) * es % 16 else D + 5
            assert aligned * es % 16 == 0 and odd * es % 16 != 0
            sentinel = _bits(torch.full((1,), -7.0, dtype=tdt))[0]
            for pitch in (D, aligned, odd):
                full = torch.full((m + extra, pitch), -7.0, dtype=tdt, device="cuda")
                res = encode_rows(src, layout, tdt, out=full[:m], index=index, norm=norm)
                assert res.data_ptr() == full.data_ptr() and tuple(res.shape) == (m, D)
                got = _bits(full)
                what = f"{layout} {dt} pitch {pitch} norm {norm is not None}"
                _same(got[:m, :D], expect, what)
                assert (got[:m, D:] == sentinel).all(), what + ": padding columns were written"
                assert (got[m:] == sentinel).all(), what + ": rows at or beyond m were written"
            flat = torch.full((m * D + 8,), -7.0, dtype=tdt, device="cuda")
            encode_rows(src, layout, tdt, out=flat[1:1 + m * D].view(m, D), index=index, norm=norm)
            got = _bits(flat)
            _same(got[1:1 + m * D].reshape(m, D), expect, f"{layout} {dt} offset norm {norm is not None}")
            assert got[0] == sentinel and (got[1 + m * D:] == sentinel).all()
    _, ms = encode_rows(rows, "fixed", index=index, timing=True)
    assert ms > 0.0


@pytest.mark.parametrize("stride", [384, 352])
def test_frozen_statistics(normalizer, stride):
    """index + norm: VecNormalize in evaluation mode on the gathered records (tests/norm_ref.py), and the existing normalize_obs(update=False) of the
    whole store indexed on the host; the normaliser's state is byte for byte what it was."""
    import torch
    from balatro_gym_amd import encode_rows
    from balatro_gym_amd.vec_env import RowBuffers
    nm, rows = normalizer
    dev, host = rows[stride]
    K, N = host.shape[:2]
    want = _frozen_reference(nm, host)
    before = _state_bytes(nm)
    assert nm.training
    rb = RowBuffers(N, torch.device("cuda"), steps=K, row_stride=stride)
    rb.rows.copy_(dev)
    for layout in ("produced", "fixed"):
        w = want if layout == "produced" else np.concatenate([want, np.zeros((STORE, 628 - 153), np.uint32)], axis=1)
        for dt in DTYPES:
            tdt = getattr(torch, dt)
            whole = _bits(nm.normalize_obs(dev, layout, tdt, update=False)).reshape(STORE, -1)
            _same(whole, _as(dt, w), f"normalize_obs(update=False) {layout} {dt}")
            for m in MS:
                for name, idx in _indices(m, 300 + m).items():
                    index = torch.from_numpy(idx.astype(np.int32)).cuda()
                    what = f"stride {stride} m {m} {name} {layout} {dt}"
                    got = _bits(encode_rows(dev, layout, tdt, index=index, norm=nm))
                    _same(got, _as(dt, _take(w, idx)), what)
                    _same(got, _take(whole, idx), what + " against normalize_obs(update=False) indexed on the host")
            index = torch.from_numpy(_indices(97, 1)["planted"].astype(np.int32)).cuda()
            a = _bits(nm.normalize_obs(dev, layout, tdt, index=index))          # training is set: an index freezes the statistics
            b = _bits(rb.normalize(nm, layout, tdt, index=index))
            _same(a, _take(whole, _indices(97, 1)["planted"]), f"normalize_obs(index=) {layout} {dt}")
            _same(b, a, f"RowBuffers.normalize(index=) {layout} {dt}")
    assert _state_bytes(nm) == before, "the statistics were written"


def test_contiguous_path(stores, normalizer, rollout):
    """index=None: without norm it is bg_encode_rows; with norm the bits of normalize_obs(update=False), for [M, stride] and [K, N, stride] rows."""
    import torch
    from balatro_gym_amd import _native as nat, encode_rows
    rows, _, want = stores[384]
    nm, nrows = normalizer
    dev, host = nrows[352]
    before = _state_bytes(nm)
    for layout in ("produced", "fixed"):
        for dt in DTYPES:
            tdt = getattr(torch, dt)
            whole = nm.normalize_obs(dev, layout, tdt, update=False)
            got = encode_rows(dev, layout, tdt, norm=nm)
            assert tuple(got.shape) == tuple(whole.shape) == host.shape[:2] + (ref.COLS[layout],)
            _same(_bits(got), _bits(whole), f"norm without index {layout} {dt}")
            _same(_bits(encode_rows(dev.view(STORE, 352)[:33], layout, tdt, norm=nm)), _bits(whole).reshape(STORE, -1)[:33], f"norm without index, 33 rows {layout} {dt}")
    assert _state_bytes(nm) == before
    # the C entry without index and statistics is bg_encode_rows
    L = nat.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for layout in ref.LAYOUTS:
        for dt in DTYPES:
            tdt = getattr(torch, dt)
            out = torch.full((STORE, ref.COLS[layout]), -7.0, dtype=tdt, device="cuda")
            rc = L.bg_encode_rows_ex(C.c_void_p(rows.data_ptr()), C.c_uint64(384), C.c_int64(STORE), None, C.c_int64(STORE - 1), nat.ENC_LAYOUTS[layout],
                                     nat.ENC_F32 if dt == "float32" else nat.ENC_BF16, None, None, C.c_double(0.0), C.c_double(0.0), C.c_void_p(out.data_ptr()),
                                     C.c_uint64(ref.COLS[layout]), None, st)
            assert rc == 0, L.bg_last_error(None).decode()
            _same(_bits(out[:STORE - 1]), _bits(encode_rows(rows[:STORE - 1], layout, tdt)), f"bg_encode_rows_ex without index {layout} {dt}")
            assert bool((out[STORE - 1] == -7.0).all())
    _same(_bits(encode_rows(rollout.rows, "extractor", torch.bfloat16, index=None, norm=None)), _bits(rollout.encode("extractor", torch.bfloat16)), "index=None, norm=None")


def test_bad_arguments_launch_nothing(stores):
    """Every BG_E_ARG of the C entry, one by one: -1, a text that starts with the entry's name, and the sentinel-filled output as it was."""
    import torch
    from balatro_gym_amd import _native as nat
    L = nat.load()
    m = 64
    rows = stores[384][0]
    out = torch.full((m, 640), -7.0, device="cuda")
    index = torch.arange(m, dtype=torch.int32, device="cuda")
    mean = torch.zeros(154, dtype=torch.float64, device="cuda")
    var = torch.ones(154, dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rp, op, ip, mp, vp = rows.data_ptr(), out.data_ptr(), index.data_ptr(), mean.data_ptr(), var.data_ptr()
    ms = C.c_float(-1.0)
    inf, nan = float("inf"), float("nan")

    def call(rows_p=rp, stride=384, store=STORE, idx_p=ip, mm=m, layout=nat.ENC_FIXED, dt=nat.ENC_F32, mean_p=None, var_p=None, eps=1e-8, clip=10.0, out_p=op, pitch=640):
        return L.bg_encode_rows_ex(C.c_void_p(rows_p), C.c_uint64(stride), C.c_int64(store), C.c_void_p(idx_p), C.c_int64(mm), layout, dt, C.c_void_p(mean_p),
                                   C.c_void_p(var_p), C.c_double(eps), C.c_double(clip), C.c_void_p(out_p), C.c_uint64(pitch), C.byref(ms), st)
    stats = dict(mean_p=mp, var_p=vp)
    bad = [dict(layout=3), dict(layout=-1), dict(dt=2), dict(dt=-1), dict(stride=336), dict(stride=360), dict(stride=0), dict(rows_p=rp + 8), dict(rows_p=None),
           dict(out_p=None), dict(pitch=627), dict(pitch=0), dict(out_p=op + 2), dict(dt=nat.ENC_BF16, out_p=op + 1), dict(mm=-1),
           dict(layout=nat.ENC_PRODUCED, pitch=152), dict(layout=nat.ENC_EXTRACTOR, pitch=446),
           dict(store=-1), dict(store=2 ** 31), dict(store=2 ** 40), dict(idx_p=ip + 2), dict(idx_p=None, mm=STORE + 1),
           dict(mean_p=mp), dict(var_p=vp), dict(layout=nat.ENC_EXTRACTOR, **stats), dict(mean_p=mp + 4, var_p=vp), dict(mean_p=mp, var_p=vp + 4),
           dict(mean_p=mp, var_p=mp), dict(eps=-1e-8, **stats), dict(eps=inf, **stats), dict(eps=nan, **stats), dict(clip=-1.0, **stats), dict(clip=inf, **stats),
           dict(clip=nan, **stats), dict(out_p=rp), dict(out_p=ip), dict(out_p=mp, **stats), dict(out_p=vp, **stats)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert L.bg_last_error(None).decode().startswith("bg_encode_rows_ex: "), (kw, L.bg_last_error(None).decode())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and ms.value == -1.0
    assert bool((mean == 0.0).all()) and bool((var == 1.0).all()) and torch.equal(index, torch.arange(m, dtype=torch.int32, device="cuda"))
    # without statistics epsilon and clip_obs are not looked at; m == 0 is a no-op, with and without them
    assert call(mm=0) == 0 and ms.value == 0.0 and call(mm=0, **stats) == 0 and call(mm=0, idx_p=None) == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert call(eps=nan, clip=-1.0) == 0 and ms.value > 0.0
    assert call(store=2 ** 40, idx_p=None, layout=nat.ENC_PRODUCED) == 0      # store_rows beyond int32 is fine without an index
    assert call(**stats) == 0 and ms.value > 0.0
    torch.cuda.synchronize()
    assert bool((out[:, 628:] == -7.0).all()) and bool((out[:, 153:628] == 0).all())


def test_the_two_index_conventions_meet(rollout):
    """Over rollout.minibatches(64): the "produced" features of a minibatch carry, in their action_mask columns, the mask bytes of records index[i] as
    0.0 / 1.0; evaluate_actions with that mask (gathered by torch) gives the log_prob that ppo_loss(index=) reports for the same minibatch reading the
    records in place; the minibatches cover every record exactly once."""
    import torch
    from balatro_gym_amd import _native as nat, evaluate_actions, ppo_loss
    rb = rollout
    K, N = rb.steps, rb.n
    first, count = next((c0, n) for name, c0, n in nat.ENC_COLUMNS[nat.ENC_PRODUCED] if name == "action_mask")
    assert count == 60
    mask_all = rb.tensors["action_mask"].contiguous().view(K * N, 60)          # int8, the records' own bytes
    assert bool(mask_all.any(dim=1).all())
    g = torch.Generator().manual_seed(9)
    actions = torch.multinomial((mask_all != 0).float().cpu(), 1, generator=g).view(K, N).to(torch.int32).cuda()   # a valid action per record
    old_lp = (-torch.rand((K, N), generator=g)).cuda()
    adv = torch.randn((K, N), generator=g).cuda()
    seen = []
    batches = list(rb.minibatches(64, generator=torch.Generator().manual_seed(4)))
    assert len(batches) == K * N // 64
    for index in batches:
        assert index.dtype == torch.int32 and index.is_cuda and tuple(index.shape) == (64,)
        seen.append(index.cpu())
        feats = rb.encode("produced", index=index)
        mask = mask_all[index.long()]
        assert bool(((mask == 0) | (mask == 1)).all()) and torch.equal(feats[:, first:first + 60], mask.float()), "action_mask columns != the mask bytes of records index[i]"
        logits = torch.randn((64, 60), generator=g).cuda()
        lp, ent = evaluate_actions(logits, actions.view(-1)[index.long()].contiguous(), mask.contiguous())
        _, stats = ppo_loss(logits, actions, old_lp, adv, rb.rows, index=index)
        assert int(stats.excluded) == 0
        _same(_bits(stats.log_prob), _bits(lp), "ppo_loss(index=).log_prob against evaluate_actions on the gathered mask")
        _same(_bits(stats.entropy), _bits(ent), "entropy")
    assert torch.equal(torch.cat(seen).sort().values, torch.arange(K * N, dtype=torch.int32))
