"""bg_sample_actions / bg_evaluate_actions on the MI355X: every load path of the kernel (logits float32 / bfloat16, dense, at stride 64, from offset
pointers; masks from records the product writes at both strides, dense int8, stride 64, an offset pointer, none) at sizes on each side of the
workgroup's 64 rows, in all three modes.  Everything is copied to the host and held to the float64 numpy restatement of tests/head_ref.py by the bounds
derived there (never to torch arithmetic on the GPU): the drawn action exactly on decidable rows and inside its interval on every row, log_prob and
entropy within their bounds; outputs sit between poisoned guard elements, inputs stay unwritten, two calls give the same bits, a slice called with its
global index0 equals the slice of the full call, evaluating the drawn actions returns the sampler's bits, bad arguments are BG_E_ARG before any launch.
Then the closed loop: 200 steps of env.act + env.step never take an invalid action, and the same loop without the mask does.

Largest observed shares of the bounds on the MI355X (the device library's expf / logf): log_prob 0.11, entropy 0.09."""
import ctypes as C

import numpy as np
import pytest

from tests import head_ref as ref

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300, 4133)
M = max(SIZES)
SEED, INDEX0, T = 0xC0FFEE_0000_0001, 7_000_000_000, 12
POISON_I, POISON_F = -0x5A5A5A5B, -1234.5
LOGIT_LAYOUTS = ("f32", "f32_s64", "f32_off4", "bf16", "bf16_s64", "bf16_off4", "bf16_off2")
MASK_KINDS = ("rec352", "rec384", "dense", "s64", "dense_off4", None)

_cache = {}


def _logits_host(bf16):
    """[M, 60] float32 values (bf16: representable in bfloat16): sigma cycles over the rows so every size sees every scale."""
    key = ("logits", bf16)
    if key not in _cache:
        rng = np.random.default_rng(2024)
        sig = np.asarray(ref.SIGMAS, np.float64)[np.arange(M) % len(ref.SIGMAS)]
        x = (rng.standard_normal((M, 60)) * sig[:, None]).astype(np.float32)
        _cache[key] = ref.widen_bf16(ref.bf16_bits(x)) if bf16 else x
    return _cache[key]


def _records():
    """Records the product writes: 1 024 envs, 60 uniform-policy steps replayed through step_many into RowBuffers at strides 352 and 384; the last five
    steps' records are M rows whose masks come from play, shop and blind-select phases."""
    if "records" not in _cache:
        import torch
        from balatro_gym_amd import BalatroVecEnv
        from balatro_gym_amd.vec_env import RowBuffers
        n, K = 1024, 60
        seeds = [4000 + i for i in range(n)]
        src = BalatroVecEnv(n, seeds, scorer_jokers=True, autoreset=True, fused_steps=64)
        rb0 = RowBuffers(n, src.device, steps=K, row_stride=352)
        src.rollout(K, policy=0, policy_seed=3, obs_buffers=rb0)
        src.check()
        acts = rb0.action.contiguous()
        src.close()
        out = {}
        for stride in (352, 384):
            env = BalatroVecEnv(n, seeds, scorer_jokers=True, autoreset=True, fused_steps=64)
            rb = RowBuffers(n, env.device, steps=K, row_stride=stride)
            env.step_many(acts, obs_buffers=rb)
            env.check()
            env.close()
            rows = rb.rows[-5:].reshape(-1, stride)[:M].clone()
            phases = set(np.unique(rows[:, 339].cpu().numpy()).tolist())
            assert {0, 1, 2} <= phases, phases
            out[stride] = rows
        assert torch.equal(out[352][:, :352], out[384][:, :352])
        _cache["records"] = out
    return _cache["records"]


def _mask(kind):
    """-> (device tensor to pass as mask, host int8 [M, 60] or None)"""
    import torch
    key = ("mask", kind)
    if key not in _cache:
        if kind is None:
            _cache[key] = (None, None)
        elif kind.startswith("rec"):
            rows = _records()[int(kind[3:])]
            _cache[key] = (rows, rows.cpu().numpy()[:, 176:236].view(np.int8).copy())
        else:
            rng = np.random.default_rng(77)
            mk = (rng.random((M, 60)) >= ref.MASKED_SHARE).astype(np.int8) * rng.integers(1, 128, (M, 60)).astype(np.int8) * np.where(rng.random((M, 60)) < 0.5, -1, 1).astype(np.int8)
            mk[5] = 0   # a row with no valid action
            h = torch.from_numpy(mk)
            if kind == "dense":
                d = h.cuda()
            elif kind == "s64":
                d = torch.full((M, 64), 1, dtype=torch.int8).cuda()
                d[:, :60] = h.cuda()
                d = d[:, :60]
            else:   # dense rows from a pointer that is 4- but not 16-byte aligned
                flat = torch.zeros(M * 60 + 4, dtype=torch.int8).cuda()
                flat[4:] = h.cuda().reshape(-1)
                d = flat[4:].view(M, 60)
                assert d.data_ptr() % 16 == 4
            _cache[key] = (d, mk)
    return _cache[key]


def _logits(layout):
    """-> (device tensor [M, 60] laid out as `layout` says, host float32 values)"""
    import torch
    key = ("dev", layout)
    if key not in _cache:
        bf16 = layout.startswith("bf16")
        x = _logits_host(bf16)
        t = torch.from_numpy(x).cuda()
        if bf16:
            t = t.to(torch.bfloat16)
            assert np.array_equal(t.float().cpu().numpy(), x)
        kind = layout.split("_")[1] if "_" in layout else "dense"
        if kind == "s64":
            w = torch.full((M, 64), 50.0, dtype=t.dtype, device="cuda")
            w[:, :60] = t
            d = w[:, :60]
        elif kind.startswith("off"):
            off = int(kind[3:]) // t.element_size()
            flat = torch.zeros(M * 60 + off, dtype=t.dtype, device="cuda")
            flat[off:] = t.reshape(-1)
            d = flat[off:].view(M, 60)
            assert d.data_ptr() % 16 == int(kind[3:])
        else:
            d = t
            assert d.data_ptr() % 16 == 0
        _cache[key] = (d, x)
    return _cache[key]


def _reference(bf16, mkind, m, a0=0):
    key = ("ref", bf16, mkind, m, a0)
    if key not in _cache:
        mk = _mask(mkind)[1]
        _cache[key] = ref.Reference(_logits_host(bf16)[a0:a0 + m], None if mk is None else mk[a0:a0 + m], SEED, INDEX0 + a0, T)
    return _cache[key]


def _guarded(m, dtype, poison):
    import torch
    buf = torch.full((m + 2,), poison, dtype=dtype, device="cuda")
    return buf, buf[1:m + 1]


def _call(lg, mk, m, mode, a0=0, given=None):
    """One call on rows [a0, a0 + m) with guarded outputs -> host (actions, log_prob, entropy); checks guards and that the inputs are unwritten."""
    import torch
    from balatro_gym_amd import evaluate_actions, sample_actions
    lgs = lg[a0:a0 + m]
    mks = None if mk is None else mk[a0:a0 + m]
    before = (lgs.clone(), None if mks is None else mks.clone())
    ba, oa = _guarded(m, torch.int32, POISON_I)
    bl, ol = _guarded(m, torch.float32, POISON_F)
    be, oe = _guarded(m, torch.float32, POISON_F)
    if mode == "evaluate":
        res = evaluate_actions(lgs, given, mks, log_prob=ol, entropy=oe)
        assert res[0] is ol and res[1] is oe
    else:
        res = sample_actions(lgs, mks, seed=SEED, t=T, index0=INDEX0 + a0, deterministic=mode == "deterministic", actions=oa, log_prob=ol, entropy=oe)
        assert res[0] is oa and res[1] is ol and res[2] is oe
    torch.cuda.synchronize()
    assert torch.equal(lgs.view(torch.int16 if lgs.dtype == torch.bfloat16 else torch.int32), before[0].view(torch.int16 if lgs.dtype == torch.bfloat16 else torch.int32))
    assert mks is None or torch.equal(mks, before[1])
    for buf, poison, written in ((ba, POISON_I, mode != "evaluate"), (bl, POISON_F, True), (be, POISON_F, True)):
        h = buf.cpu().numpy()
        assert h[0] == poison and h[-1] == poison, "a guard element was written"
        assert written or (h == poison).all()
    return oa.cpu().numpy(), ol.cpu().numpy(), oe.cpu().numpy()


_shares = {"undecidable": 0.0, "log_prob": 0.0, "entropy": 0.0}


def _check_all_modes(layout, mkind, m, a0=0):
    import torch
    lg, _ = _logits(layout)
    mk, _ = _mask(mkind)
    r = _reference(layout.startswith("bf16"), mkind, m, a0)
    what = f"{layout} / mask {mkind} / m {m}"
    a, lp, en = _call(lg, mk, m, "sample", a0)
    # (the 0.5 % cap is a property of a test SET: test_reference_sets_are_fit holds the M-row sets to it; the smaller sizes are slices of them)
    und = r.check_sampled(a, what, cap=m == M)
    if m == M:
        _shares["undecidable"] = max(_shares["undecidable"], und)
    s = r.check_stats(a, lp, en, what + " sample")
    _shares["log_prob"], _shares["entropy"] = max(_shares["log_prob"], s[0]), max(_shares["entropy"], s[1])
    a1, lp1, en1 = _call(lg, mk, m, "deterministic", a0)
    r.check_mode(a1, what)
    r.check_stats(a1, lp1, en1, what + " deterministic")
    assert np.array_equal(en1.view(np.uint32), en.view(np.uint32))
    # evaluating the drawn actions returns the sampler's bits
    _, lp2, en2 = _call(lg, mk, m, "evaluate", a0, given=torch.from_numpy(a.copy()).cuda())
    assert np.array_equal(lp2.view(np.uint32), lp.view(np.uint32)) and np.array_equal(en2.view(np.uint32), en.view(np.uint32)), what
    # arbitrary given actions: masked ones are -inf, out-of-range ones NaN
    given = np.random.default_rng(m).integers(-2, 62, m).astype(np.int32)
    _, lp3, en3 = _call(lg, mk, m, "evaluate", a0, given=torch.from_numpy(given).cuda())
    r.check_stats(given, lp3, en3, what + " evaluate")
    return a, lp, en


def test_reference_sets_are_fit():
    """The M-row sets themselves hold at most 0.5 % undecidable rows (a property of the reference alone), and have degenerate rows in them."""
    for bf16 in (False, True):
        for mkind in MASK_KINDS:
            r = _reference(bf16, mkind, M)
            assert (~r.decidable).sum() <= ref.UNDECIDABLE_CAP * M, (bf16, mkind)
    assert _reference(False, "dense", M).degenerate[5]


@pytest.mark.parametrize("layout", LOGIT_LAYOUTS)
def test_every_load_path_size_and_mode(layout):
    for mkind in MASK_KINDS:
        for m in SIZES:
            _check_all_modes(layout, mkind, m)
    print(f"{layout}: largest shares so far {_shares}")


def test_same_bits_twice_and_slices_follow_the_global_index():
    lg, _ = _logits("bf16")
    mk, _ = _mask("rec384")
    full = _call(lg, mk, M, "sample")
    again = _call(lg, mk, M, "sample")
    for f, g in zip(full, again):
        assert np.array_equal(f.view(np.uint32), g.view(np.uint32))
    for layout, mkind, a0, b0 in (("bf16", "rec384", 64, 1000), ("f32", "dense", 37, 613), ("f32_s64", None, 4001, 4133), ("bf16_s64", "rec352", 1, 2)):
        lg, _ = _logits(layout)
        mk, _ = _mask(mkind)
        whole = _call(lg, mk, M, "sample")
        part = _check_all_modes(layout, mkind, b0 - a0, a0)
        for w, p in zip(whole, part):
            assert np.array_equal(w[a0:b0].view(np.uint32), p.view(np.uint32)), (layout, mkind, a0, b0)


def test_degenerate_rows_on_the_device():
    import torch
    from tests.test_policy_head_host import degenerate_cases
    l, k = degenerate_cases()
    r = ref.Reference(l, k, SEED, 0, T)
    from balatro_gym_amd import evaluate_actions, sample_actions
    for dt in (torch.float32, torch.bfloat16):
        lg, mk = torch.from_numpy(l).cuda().to(dt), torch.from_numpy(k).cuda()
        rr = r if dt == torch.float32 else ref.Reference(lg.float().cpu().numpy(), k, SEED, 0, T)
        assert rr.degenerate.tolist() == [True] * 5 + [False] * 4
        for det in (False, True):
            a, lp, en = (x.cpu().numpy() for x in sample_actions(lg, mk, seed=SEED, t=T, deterministic=det))
            assert a[:5].tolist() == [-1] * 5 and a[7] != 7 and a[8] == 7 and (k[np.arange(5, 9), a[5:]] != 0).all()
            rr.check_stats(a, lp, en, "degenerate")
            assert en[8] == 0.0 and lp[8] == 0.0
        lp, en = (x.cpu().numpy() for x in evaluate_actions(lg, torch.full((9,), 7, dtype=torch.int32, device="cuda"), mk))
        rr.check_stats(np.full(9, 7), lp, en, "degenerate evaluate")
        assert np.isneginf(lp[7])


def test_nullable_outputs_and_refused_arguments():
    """The C entry points: log_prob_dev / entropy_dev may be NULL; every bad argument is BG_E_ARG with a text, before any launch (poison untouched)."""
    import torch
    from balatro_gym_amd import _native as nat
    L = nat.load()
    m = 300
    lg, _ = _logits("f32")
    mk, _ = _mask("rec384")
    want = _call(lg, mk, m, "sample")
    vp = C.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream)

    def sample(logits=lg.data_ptr(), dt=0, ls=60, mask=mk.data_ptr() + 176, ms=384, mm=m, flags=0, acts=None, lp=None, en=None):
        return L.bg_sample_actions(vp(logits), dt, C.c_uint64(ls), vp(mask), C.c_uint64(ms), C.c_int64(mm), C.c_uint32(flags), C.c_uint64(SEED),
                                   C.c_uint64(INDEX0), C.c_uint64(T), vp(acts), vp(lp), vp(en), None, stream)

    def evaluate(logits=lg.data_ptr(), dt=0, ls=60, mask=mk.data_ptr() + 176, ms=384, mm=m, acts=None, lp=None, en=None):
        return L.bg_evaluate_actions(vp(logits), dt, C.c_uint64(ls), vp(mask), C.c_uint64(ms), C.c_int64(mm), vp(acts), vp(lp), vp(en), None, stream)

    for null_lp, null_en in ((True, True), (True, False), (False, True)):
        ba, oa = _guarded(m, torch.int32, POISON_I)
        bl, ol = _guarded(m, torch.float32, POISON_F)
        be, oe = _guarded(m, torch.float32, POISON_F)
        assert sample(acts=oa.data_ptr(), lp=None if null_lp else ol.data_ptr(), en=None if null_en else oe.data_ptr()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(oa.cpu().numpy(), want[0])
        assert (bl.cpu().numpy() == POISON_F).all() if null_lp else np.array_equal(ol.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
        assert (be.cpu().numpy() == POISON_F).all() if null_en else np.array_equal(oe.cpu().numpy().view(np.uint32), want[2].view(np.uint32))
        given = torch.from_numpy(want[0].copy()).cuda()
        assert evaluate(acts=given.data_ptr(), lp=None if null_lp else ol.data_ptr(), en=None if null_en else oe.data_ptr()) == 0
        torch.cuda.synchronize()
        assert null_lp or np.array_equal(ol.cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    # m == 0 is a no-op
    ba, oa = _guarded(m, torch.int32, POISON_I)
    assert sample(mm=0, acts=oa.data_ptr()) == 0
    # refused arguments
    bl, ol = _guarded(m, torch.float32, POISON_F)
    be, oe = _guarded(m, torch.float32, POISON_F)
    a, l, e = oa.data_ptr(), ol.data_ptr(), oe.data_ptr()
    bad = [dict(logits=0), dict(dt=2), dict(dt=-1), dict(ls=59), dict(logits=lg.data_ptr() + 2), dict(dt=1, logits=lg.data_ptr() + 1), dict(mm=-1),
           dict(mask=mk.data_ptr() + 177), dict(mask=mk.data_ptr() + 178), dict(ms=59), dict(ms=56), dict(ms=62), dict(flags=2), dict(flags=0x80000001),
           dict(acts=0), dict(acts=a + 1), dict(lp=l + 2), dict(en=e + 1), dict(lp=e), dict(lp=a), dict(en=a), dict(acts=lg.data_ptr()),
           dict(lp=lg.data_ptr()), dict(en=mk.data_ptr() + 176), dict(mm=64 * 0x7fffffff + 1)]
    for kw in bad:
        args = dict(acts=a, lp=l, en=e)
        args.update(kw)
        assert sample(**args) == -1, kw
        text = L.bg_last_error(None).decode()
        assert text.startswith("bg_sample_actions: "), (kw, text)
        if "flags" not in kw:
            args.pop("flags", None)
            assert evaluate(**args) == -1, kw
            assert L.bg_last_error(None).decode().startswith("bg_evaluate_actions: "), kw
    torch.cuda.synchronize()
    for buf, poison in ((ba, POISON_I), (bl, POISON_F), (be, POISON_F)):
        assert (buf.cpu().numpy() == poison).all(), "a refused call wrote an output"
    assert not lg[:m].isnan().any() and torch.equal(lg[:m].cpu(), torch.from_numpy(_logits_host(False)[:m]))


def test_row_buffers_sample_and_shapes():
    """RowBuffers.sample takes the mask of record row `step`; leading shapes [K, N] work; timing returns kernel milliseconds."""
    import torch
    from balatro_gym_amd import evaluate_actions, sample_actions
    from balatro_gym_amd.vec_env import RowBuffers
    n, K = 100, 3
    rows = _records()[384][:K * n].reshape(K, n, 384)
    rb = RowBuffers(n, rows.device, steps=K, row_stride=384)
    rb.rows.copy_(rows)
    lg, x = _logits("f32")
    for step in (-1, 0, 1):
        a, lp, en = rb.sample(lg[:n], step, seed=SEED, t=T, index0=INDEX0)
        r = ref.Reference(x[:n], rows[step].cpu().numpy()[:, 176:236], SEED, INDEX0, T)
        r.check_sampled(a.cpu().numpy(), f"RowBuffers.sample step {step}", cap=False)
        r.check_stats(a.cpu().numpy(), lp.cpu().numpy(), en.cpu().numpy(), "RowBuffers.sample")
    l3 = lg[:K * n].reshape(K, n, 60)
    a, lp, en, ms = sample_actions(l3, rb.rows, seed=SEED, t=T, index0=INDEX0, timing=True)
    assert tuple(a.shape) == (K, n) == tuple(lp.shape) == tuple(en.shape) and ms > 0.0
    flat = sample_actions(lg[:K * n], rows.reshape(K * n, 384), seed=SEED, t=T, index0=INDEX0)
    assert torch.equal(a.reshape(-1), flat[0]) and torch.equal(lp.reshape(-1).view(torch.int32), flat[1].view(torch.int32))
    lp2, en2 = evaluate_actions(l3, a, rb.rows)
    assert torch.equal(lp2.view(torch.int32), lp.view(torch.int32)) and torch.equal(en2.view(torch.int32), en.view(torch.int32))
    e = sample_actions(lg[:0], None, seed=0, t=0)
    assert tuple(e[0].shape) == (0,)


@pytest.mark.parametrize("obs_layout", ["rows", "keys"])
def test_closed_loop_never_takes_an_invalid_action(obs_layout):
    """256 envs, 200 steps of a = env.act(logits_t); env.step(a) with host-generated pseudo-random logits: info.error is never BG_ERR_INVALID_ACTION.
    The same loop drawing without the mask hits it, so the test can see one."""
    import torch
    from balatro_gym_amd import BalatroVecEnv, sample_actions
    n, steps, INVALID = 256, 200, 1
    g = torch.Generator().manual_seed(31)
    logits = (torch.randn((steps, n, 60), generator=g) * 2.0).cuda()
    for masked in (True, False):
        env = BalatroVecEnv(n, [70 + i for i in range(n)], scorer_jokers=True, autoreset=True, obs_layout=obs_layout)
        invalid = torch.zeros((), dtype=torch.int64, device=env.device)
        for t in range(steps):
            if masked:
                a = env.act(logits[t], seed=5, t=t)
                valid = env.obs["action_mask"].gather(1, a.long().clamp(min=0)[:, None])[:, 0] != 0
                assert bool(valid.all()) if t % 50 == 0 else True
            else:
                a = sample_actions(logits[t], None, seed=5, t=t)[0]
            _, _, _, _, info = env.step(a)
            invalid += (info["error"] == INVALID).sum()
        env.check()
        env.close()
        assert (int(invalid) == 0) == masked, f"masked {masked}: {int(invalid)} invalid actions in {steps * n} steps"
