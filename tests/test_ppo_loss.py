"""bg_ppo_loss on the MI355X: every load and store path of the kernel (logits and dlogits float32 / bfloat16, dense, at stride 64, from offset pointers;
masks from records the product wrote at both strides, dense int8, none; with and without an index, a permutation and repeated indices) at sizes on each
side of the workgroup's 64 rows and one with more workgroup partials than the finishing workgroup has lanes.  Everything is copied to the host and held
to the float64 closed form of tests/ppo_ref.py by the bounds derived there (never to torch arithmetic on the GPU): gradient elements, scalars, the
reference's clip branch on decidable rows, zero rows and the count for excluded rows; outputs sit between poisoned guards, padding columns and inputs
stay unwritten, two calls give the same bits, log_prob / entropy are bit for bit evaluate_actions', the bf16 gradient is the float32 call's rounded to
nearest even, a ratio of exactly 1 gives approx_kl == clip_fraction == 0, bad arguments are BG_E_ARG before any launch, m == 0 zeroes the stats.
Then autograd: logits.grad is dlogits, a scaled loss scales it, and a two-layer MLP on encode_rows output matches its float64 twin.

Largest observed shares of the bounds on the MI355X (the device library's expf / logf): dlogits 0.12, dvalues 0.49, policy_loss 0.011, approx_kl 0.001,
entropy_loss 0.034, value_loss 0.19, loss 0.043, adv_mean 0.43, adv_std 0.40, log_prob 0.12, entropy 0.08, clip_fraction 0.48 (its bound on a set without
undecidable rows is the final rounding alone).
At m = 65 793 (BIG2: two advantage triples per lane of bg_ppo_adv_combine, five row partials per lane of bg_ppo_finish): dlogits 0.12, dvalues 0.49,
policy_loss 0.0006, approx_kl 0.00004, entropy_loss 0.010, value_loss 0.089, loss 0.0014, adv_mean 0.24, adv_std 0.28, log_prob 0.12, entropy 0.066,
clip_fraction 0.071."""
import ctypes as C

import numpy as np
import pytest

from tests import head_ref, ppo_ref

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 257, 4133)
BIG = 256 * 64 + 64 + 1   # 258 workgroup partials: the finishing workgroup's lanes fold two each
LAYOUTS = ("f32", "f32_s64", "f32_off4", "bf16", "bf16_s64", "bf16_off4", "bf16_off2")
MASK_KINDS = ("rec352", "rec384", "dense", None)
INDEX_KINDS = (None, "perm", "repeat")
GUARD = 64
COEF = (0.2, 0.01, 0.5)

_cache: dict = {}
_shares: dict = {}


def _note(sh):
    for k, v in sh.items():
        _shares[k] = max(_shares.get(k, 0.0), float(v))


def _records(stride):
    from tests.test_policy_head import _records as head_records
    return head_records()[stride]


def _case(m, mkind, ikind, bf16):
    """-> (ppo_ref.Case, device mask tensor or None, mask pointer offset, mask stride)"""
    import torch
    key = ("case", m, mkind, ikind, bf16)
    if key not in _cache:
        sigma = head_ref.SIGMAS[(m + len(str(mkind))) % 4]
        seed = m * 7 + MASK_KINDS.index(mkind) * 3 + INDEX_KINDS.index(ikind)
        if mkind is not None and mkind.startswith("rec"):
            stride = int(mkind[3:])
            rows = _records(stride)
            store = min(rows.shape[0], 2 * m)
            host_mask = rows.cpu().numpy()[:, 176:236].view(np.int8)
            c = ppo_ref.synthetic(seed, m, sigma, True, index=ikind, bf16=bf16, mask=host_mask, store_rows=store)
            dev = rows[:c.store_rows].clone()   # the product's records; the hand-made rows' masks are written over theirs
            dev[:, 176:236] = torch.from_numpy(c.mask.view(np.uint8)).cuda()
            _cache[key] = (c, dev, 176, stride)
        else:
            c = ppo_ref.synthetic(seed, m, sigma, mkind == "dense", index=ikind, bf16=bf16)
            dev = torch.from_numpy(c.mask).cuda() if c.mask is not None else None
            _cache[key] = (c, dev, 0, 60)
    return _cache[key]


def _place(host, kind, bf16, poison=None):
    """A device matrix [m, 60] laid out as `kind` (dense / s64 / off4 / off2) inside a guarded flat buffer -> (flat, view, element offset, stride).
    host: float32 values to store (inputs), or None with `poison` (outputs)."""
    import torch
    m = host.shape[0] if host is not None else poison[1]
    dt = torch.bfloat16 if bf16 else torch.float32
    es = 2 if bf16 else 4
    stride = 64 if kind == "s64" else 60
    off = {"dense": 0, "s64": 0, "off4": 4 // es, "off2": 1}[kind]
    fill = 250.0 if poison is None else poison[0]
    flat = torch.full((GUARD + off + m * stride + GUARD,), fill, dtype=dt, device="cuda")
    view = flat[GUARD + off:GUARD + off + m * stride].view(m, stride)[:, :60]
    assert flat.data_ptr() % 16 == 0 and view.data_ptr() % 16 == (off * es) % 16
    if host is not None:
        view.copy_(torch.from_numpy(host).cuda().to(dt))
        assert np.array_equal(view.float().cpu().numpy(), host, equal_nan=True)
    return flat, view, GUARD + off, stride


def _outside_untouched(flat, view_off, m, stride, fill):
    import torch
    chk = flat.clone()
    chk[view_off:view_off + m * stride].view(m, stride)[:, :60] = fill
    return bool(torch.equal(chk, torch.full_like(chk, fill)))


class _Call:
    """One bg_ppo_loss call through the C ABI with every output between poisoned guards; `.run()` launches, `.fetch()` copies back and checks the guards
    and that no input was written."""

    def __init__(self, c, mask_dev, moff, mstride, layout, out_kind=None, clip=COEF[0], ent=COEF[1], vf=COEF[2], normalize=True, use_values=True,
                 null=()):
        import torch
        from balatro_gym_amd import _native as nat
        self.L = nat.load()
        self.c, self.m = c, c.m
        self.bf16 = layout.startswith("bf16")
        kind = layout.split("_")[1] if "_" in layout else "dense"
        self.lflat, self.lview, _, self.lstride = _place(c.logits, kind, self.bf16)
        self.dflat, self.dview, self.doff, self.dstride = _place(None, out_kind or kind, self.bf16, poison=(-1234.5 if not self.bf16 else -1232.0, c.m))
        self.dfill = -1234.5 if not self.bf16 else -1232.0
        dev = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
        self.mask, self.moff, self.mstride = mask_dev, moff, mstride
        self.has_v = use_values and c.values is not None
        self.ins = {"actions": dev(c.actions), "old": dev(c.old_log_prob), "adv": dev(c.advantages), "values": dev(c.values) if self.has_v else None,
                    "returns": dev(c.returns) if self.has_v else None, "index": dev(c.index)}
        self.before = {k: (None if v is None else v.clone()) for k, v in self.ins.items()}
        self.before["logits"] = self.lflat.clone()
        self.before["mask"] = None if mask_dev is None else mask_dev.clone()
        g = lambda n: torch.full((n + 2,), -1234.5, dtype=torch.float32, device="cuda")   # noqa: E731
        self.outs = {"dvalues": g(c.m) if self.has_v and "dvalues" not in null else None, "log_prob": g(c.m) if "log_prob" not in null else None,
                     "entropy": g(c.m) if "entropy" not in null else None, "stats": g(10)}
        need = int(self.L.bg_ppo_loss_workspace_bytes(C.c_int64(c.m)))
        self.ws = torch.zeros(need + 32, dtype=torch.uint8, device="cuda")
        self.args = dict(clip=clip, ent=ent, vf=vf, flags=1 if normalize else 0)

    def run(self, **over):
        import torch
        vp = C.c_void_p
        p = lambda t, o=0: None if t is None else t.data_ptr() + o   # noqa: E731
        a = dict(logits=p(self.lview), dt=1 if self.bf16 else 0, ls=self.lstride, mask=p(self.mask, self.moff), ms=self.mstride, actions=p(self.ins["actions"]),
                 old=p(self.ins["old"]), adv=p(self.ins["adv"]), values=p(self.ins["values"]), returns=p(self.ins["returns"]), index=p(self.ins["index"]),
                 store=self.c.store_rows, m=self.m, dlogits=p(self.dview), ds=self.dstride, dvalues=p(self.outs["dvalues"], 4), lp=p(self.outs["log_prob"], 4),
                 en=p(self.outs["entropy"], 4), stats=p(self.outs["stats"], 4), ws=p(self.ws), wsb=self.ws.numel() - 32, **self.args)
        a.update(over)
        return self.L.bg_ppo_loss(vp(a["logits"]), a["dt"], C.c_uint64(a["ls"]), vp(a["mask"]), C.c_uint64(a["ms"]), vp(a["actions"]), vp(a["old"]), vp(a["adv"]),
                                  vp(a["values"]), vp(a["returns"]), vp(a["index"]), C.c_int64(a["store"]), C.c_int64(a["m"]), C.c_float(a["clip"]),
                                  C.c_float(a["ent"]), C.c_float(a["vf"]), C.c_uint32(a["flags"]), vp(a["dlogits"]), C.c_uint64(a["ds"]), vp(a["dvalues"]),
                                  vp(a["lp"]), vp(a["en"]), vp(a["stats"]), vp(a["ws"]), C.c_uint64(a["wsb"]), None,
                                  vp(torch.cuda.current_stream().cuda_stream))

    def untouched(self):
        """Nothing was written: every output still holds its poison."""
        import torch
        torch.cuda.synchronize()
        ok = bool((self.dflat == self.dfill).all())
        for t in self.outs.values():
            ok = ok and (t is None or bool((t == -1234.5).all()))
        return ok

    def fetch(self):
        """-> (dlogits [m, 60] float32 or bf16 bits, dvalues, log_prob, entropy, stats) on the host"""
        import torch
        torch.cuda.synchronize()
        assert _outside_untouched(self.dflat, self.doff, self.m, self.dstride, self.dfill), "dlogits: a guard or a padding column was written"
        for k, t in self.outs.items():
            if t is not None:
                assert float(t[0]) == -1234.5 and float(t[-1]) == -1234.5, f"{k}: a guard element was written"
        for k, t in self.ins.items():
            assert t is None or torch.equal(t.view(torch.int32), self.before[k].view(torch.int32)), f"input {k} was written"
        assert torch.equal(self.lflat.view(torch.int16), self.before["logits"].view(torch.int16)), "the logits were written"
        assert self.mask is None or torch.equal(self.mask, self.before["mask"]), "the mask was written"
        dl = self.dview.contiguous()
        dl = dl.view(torch.int16).cpu().numpy().view(np.uint16) if self.bf16 else dl.cpu().numpy()
        h = lambda t: None if t is None else t[1:-1].cpu().numpy()   # noqa: E731
        return dl, h(self.outs["dvalues"]), h(self.outs["log_prob"]), h(self.outs["entropy"]), h(self.outs["stats"])


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _check_one(layout, mkind, ikind, m, normalize=True, use_values=True, twice=False):
    import torch
    from balatro_gym_amd import evaluate_actions
    bf16 = layout.startswith("bf16")
    c, mdev, moff, mstride = _case(m, mkind, ikind, bf16)
    what = f"{layout} / mask {mkind} / index {ikind} / m {m}"
    call = _Call(c, mdev, moff, mstride, layout, normalize=normalize, use_values=use_values)
    assert call.run() == 0, call.L.bg_last_error(None)
    first = call.fetch()
    dl, dv, lp, en, st = first
    if bf16:   # the float32 call on the same (bf16-representable) logits: its gradient rounded to nearest even is the bf16 call's, bit for bit
        f32 = _Call(c, mdev, moff, mstride, "f32" + layout[4:], normalize=normalize, use_values=use_values)
        assert f32.run() == 0
        dl32, dv32, lp32, en32, st32 = f32.fetch()
        assert np.array_equal(dl, head_ref.bf16_bits(dl32)), what + ": bf16 dlogits is not the rounding of the float32 call's"
        for x, y in ((dv, dv32), (lp, lp32), (en, en32), (st, st32)):
            assert (x is None and y is None) or np.array_equal(_bits(x), _bits(y)), what
        dl = dl32
    cf = ppo_ref.ClosedForm(c, COEF[0], COEF[1], COEF[2], normalize, use_values)
    _note(cf.check(dl, dv, lp, en, st, what, cap=m >= 4133))
    # log_prob / entropy: evaluate_actions' bits on the gathered rows
    ok, mk, a, _, _, _ = c.gathered()
    elp, een = evaluate_actions(torch.from_numpy(c.logits).cuda(), torch.from_numpy(a).cuda(), None if mk is None else torch.from_numpy(mk).cuda())
    assert np.array_equal(_bits(lp)[ok], _bits(elp.cpu().numpy())[ok]) and np.array_equal(_bits(en)[ok], _bits(een.cpu().numpy())[ok]), what
    if twice:
        again = _Call(c, mdev, moff, mstride, layout, normalize=normalize, use_values=use_values)
        assert again.run() == 0
        for x, y in zip(first, again.fetch()):
            assert (x is None and y is None) or np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), what + ": two calls differ"
    return cf, (dl, dv, lp, en, st)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_path_and_size(layout):
    """Every mask kind at every size, the index kind rotating so that every (mask, index) pair and every (size, index) pair occurs; normalisation and
    the value term alternate.  The 4 133-row calls run twice and must give equal bits."""
    n = 0
    for mi, mkind in enumerate(MASK_KINDS):
        for si, m in enumerate(SIZES):
            ikind = INDEX_KINDS[(mi + si + LAYOUTS.index(layout)) % 3]
            _check_one(layout, mkind, ikind, m, normalize=(n % 3) != 2, use_values=(n % 4) != 3, twice=m == 4133)
            n += 1
    print(f"{layout}: largest shares so far {_shares}")


@pytest.mark.parametrize("layout", ["f32", "bf16"])
def test_more_partials_than_the_finishing_workgroup_has_lanes(layout):
    for mkind, ikind in (("dense", "repeat"), (None, None)):
        cf, (dl, dv, lp, en, st) = _check_one(layout, mkind, ikind, BIG, twice=True)
        assert st[9] == BIG and st[8] == cf.excluded.sum() > 0
    print(f"{layout}: largest shares so far {_shares}")


BIG2 = 256 * 256 + 256 + 1   # 258 advantage triples: bg_ppo_adv_combine's lanes fold two each; 1 029 row partials: bg_ppo_finish's lanes fold five, lane 205 four
BIG2_CASES = (("dense", "perm", True), (None, None, True), ("rec384", "repeat", True), ("dense", "perm", False))


@pytest.mark.parametrize("mkind,ikind,normalize", BIG2_CASES, ids=["dense-perm", "none", "rec384-repeat", "dense-perm-raw-adv"])
@pytest.mark.parametrize("layout", ["f32", "bf16"])
def test_more_advantage_triples_than_the_statistics_workgroup_has_lanes(layout, mkind, ikind, normalize):
    """m = 65 793: per = 2 in bg_ppo_adv_combine (m > 65 536; 258 triples of 256 rows, the last of one row) and per = 5 in bg_ppo_finish.  The record
    masks are the product's 4 133 records read with repetition.  Twice, equal bits."""
    assert -(-BIG2 // 256) == 258 and -(-258 // 256) == 2 and -(-BIG2 // 64) == 1029 and -(-1029 // 256) == 5 and 1029 - 205 * 5 == 4
    cf, (dl, dv, lp, en, st) = _check_one(layout, mkind, ikind, BIG2, normalize=normalize, twice=True)
    assert st[9] == BIG2 and st[8] == cf.excluded.sum() > 0
    assert cf.apply == normalize
    print(f"{layout} {mkind} {ikind}: largest shares so far {_shares}")


def test_output_layout_is_independent_of_the_input_layout():
    """dlogits takes its own path: dense float32 logits into a strided and an offset gradient matrix and back; the values are the same bits."""
    c, mdev, moff, mstride = _case(257, "rec384", "perm", False)
    base = None
    for lin, lout in (("f32", "dense"), ("f32", "s64"), ("f32", "off4"), ("f32_s64", "dense"), ("f32_off4", "s64"), ("bf16", "off2"), ("bf16_off2", "dense"),
                      ("bf16", "s64"), ("bf16_s64", "off4")):
        cb = _case(257, "rec384", "perm", lin.startswith("bf16"))
        call = _Call(cb[0], cb[1], cb[2], cb[3], lin, out_kind=lout)
        assert call.run() == 0
        got = call.fetch()
        key = lin.startswith("bf16")
        if base is None or key not in base:
            base = dict(base or {})
            base[key] = got
        for x, y in zip(base[key], got):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (lin, lout)


def test_ratio_of_exactly_one():
    """old_log_prob taken from evaluate_actions: ratio == 1 on every row, so approx_kl == 0, clip_fraction == 0 and policy_loss is the float64 mean of
    -adv' rounded (adv' in float32 from the reported mean and std)."""
    import torch
    from balatro_gym_amd import evaluate_actions, ppo_loss
    m = 4133
    c = ppo_ref.synthetic(99, m, 3.0, True, hand_made=False)
    lg, a, mk = torch.from_numpy(c.logits).cuda(), torch.from_numpy(c.actions).cuda(), torch.from_numpy(c.mask).cuda()
    adv = torch.from_numpy(c.advantages).cuda()
    old, _ = evaluate_actions(lg, a, mk)
    for normalize in (False, True):
        loss, st = ppo_loss(lg, a, old, adv, mk, clip_range=0.2, ent_coef=0.01, normalize_advantage=normalize)
        raw = st.raw.cpu().numpy()
        assert raw[4] == 0.0 and raw[5] == 0.0 and raw[8] == 0.0 and raw[9] == m and raw[2] == 0.0
        assert torch.equal(st.log_prob.view(torch.int32), old.view(torch.int32))
        advn = c.advantages
        if normalize:
            mean, std = np.float32(c.advantages.astype(np.float64).mean()), np.float32(c.advantages.astype(np.float64).std(ddof=1))
            assert abs(float(raw[6]) - float(mean)) <= 2.0 ** -23 * abs(float(mean)) + 1e-30 and abs(float(raw[7]) - float(std)) <= 2.0 ** -23 * float(std)
            advn = (c.advantages - raw[6]) / (raw[7] + np.float32(1e-8))
            assert advn.dtype == np.float32
        assert raw[1] == np.float32((-advn.astype(np.float64)).sum() / m), (normalize, raw[1])
        assert float(loss) == float(raw[0]) and loss.dtype == torch.float32 and loss.dim() == 0 and not loss.requires_grad


def test_nullable_outputs_refused_arguments_and_m_zero():
    """dvalues_dev / log_prob_dev / entropy_dev may be NULL; every bad argument is BG_E_ARG with its text, before any launch (poison untouched);
    m == 0 writes zeros to stats and nothing else."""
    c, mdev, moff, mstride = _case(257, "rec384", "repeat", False)
    full = _Call(c, mdev, moff, mstride, "f32")
    assert full.run() == 0
    want = full.fetch()
    for null in (("dvalues",), ("log_prob", "entropy"), ("dvalues", "log_prob", "entropy")):
        call = _Call(c, mdev, moff, mstride, "f32", null=null)
        assert call.run() == 0
        got = call.fetch()
        for k, (x, y) in enumerate(zip(want, got)):
            assert y is None or np.array_equal(_bits(x), _bits(y)), (null, k)
        assert [g is None for g in got[1:4]] == [n in null for n in ("dvalues", "log_prob", "entropy")]
    # without the value term: values / returns NULL
    nov = _Call(c, mdev, moff, mstride, "f32", use_values=False)
    assert nov.run() == 0 and nov.fetch()[4][2] == 0.0
    call = _Call(c, mdev, moff, mstride, "f32")
    L = call.L
    p = lambda t, o=0: t.data_ptr() + o   # noqa: E731
    lgp, dlp, st, ws = p(call.lview), p(call.dview), p(call.outs["stats"], 4), p(call.ws)
    need = int(L.bg_ppo_loss_workspace_bytes(C.c_int64(c.m)))
    assert call.ws.numel() - 32 == need and dlp % 16 == 0
    bad = [dict(logits=0), dict(dt=2), dict(dt=-1), dict(ls=59), dict(ds=59), dict(logits=lgp + 2), dict(dlogits=dlp + 2), dict(dlogits=0), dict(m=-1),
           dict(dt=1, logits=lgp + 1), dict(dt=1, dlogits=dlp + 1), dict(mask=p(mdev, 177)), dict(mask=p(mdev, 178)), dict(ms=59), dict(ms=62),
           dict(actions=0), dict(old=0), dict(adv=0), dict(actions=p(call.ins["actions"], 2)), dict(old=p(call.ins["old"], 1)), dict(adv=p(call.ins["adv"], 3)),
           dict(returns=None), dict(values=None), dict(values=p(call.ins["values"], 2)), dict(index=p(call.ins["index"], 2)), dict(store=-1), dict(store=2 ** 31),
           dict(clip=0.0), dict(clip=1.0), dict(clip=-0.2), dict(clip=1.5), dict(clip=float("nan")), dict(ent=float("inf")), dict(ent=float("nan")),
           dict(vf=float("-inf")), dict(flags=2), dict(flags=0x80000001), dict(stats=0), dict(stats=st + 2), dict(ws=0), dict(ws=ws + 8), dict(wsb=need - 1),
           dict(wsb=0), dict(lp=p(call.outs["log_prob"], 6)), dict(en=p(call.outs["entropy"], 5)), dict(dvalues=p(call.outs["dvalues"], 3)),
           # aliasing: an output on an input, an output on another output
           dict(dlogits=lgp), dict(lp=p(call.ins["old"])), dict(en=p(call.ins["adv"])), dict(dvalues=p(call.ins["values"])), dict(stats=p(call.ins["returns"])),
           dict(dvalues=p(call.ins["actions"])), dict(lp=p(call.ins["index"])), dict(en=p(mdev, 176)), dict(lp=p(call.outs["entropy"], 4)),
           dict(dvalues=p(call.outs["log_prob"], 4)), dict(stats=p(call.outs["dvalues"], 4)), dict(ws=dlp), dict(m=64 * 0x7fffffff + 1)]
    for kw in bad:
        assert call.run(**kw) == -1, kw
        text = L.bg_last_error(None).decode()
        assert text.startswith("bg_ppo_loss: "), (kw, text)
    assert call.untouched(), "a refused call wrote an output"
    # dvalues without values is refused too
    nov = _Call(c, mdev, moff, mstride, "f32", use_values=False)
    assert nov.run(dvalues=p(call.outs["dvalues"], 4)) == -1 and "dvalues_dev" in L.bg_last_error(None).decode()
    # m == 0
    assert call.run(m=0, ws=0, wsb=0) == 0
    import torch
    torch.cuda.synchronize()
    assert (call.outs["stats"][1:-1] == 0).all() and float(call.outs["stats"][0]) == -1234.5 and float(call.outs["stats"][-1]) == -1234.5
    assert bool((call.dflat == call.dfill).all()) and bool((call.outs["log_prob"] == -1234.5).all())
    assert call.run() == 0
    for x, y in zip(want, call.fetch()):
        assert np.array_equal(_bits(x), _bits(y))


def test_python_surface_shapes_timing_and_workspace_cache():
    """ppo_loss: leading shapes [K, N], RowBuffers-style record masks, index over the stored rollout, timing, the cached workspace, an empty batch."""
    import torch
    from balatro_gym_amd import ppo_loss, vec_env
    K, n = 3, 100
    c, mdev, moff, mstride = _case(K * n, "rec384", None, False)
    t = lambda x: torch.from_numpy(x).cuda()   # noqa: E731
    flat, sf = ppo_loss(t(c.logits), t(c.actions), t(c.old_log_prob), t(c.advantages), mdev, values=t(c.values), returns=t(c.returns), ent_coef=0.01)
    l3, s3 = ppo_loss(t(c.logits).view(K, n, 60), t(c.actions).view(K, n), t(c.old_log_prob).view(K, n), t(c.advantages).view(K, n), mdev.view(K, n, 384),
                      values=t(c.values).view(K, n), returns=t(c.returns).view(K, n), ent_coef=0.01, timing=True)
    assert torch.equal(sf.raw.view(torch.int32), s3.raw.view(torch.int32)) and tuple(s3.dlogits.shape) == (K, n, 60) and tuple(s3.dvalues.shape) == (K, n)
    assert torch.equal(sf.dlogits.view(-1).view(torch.int32), s3.dlogits.view(-1).view(torch.int32)) and s3.kernel_ms > 0.0 and sf.kernel_ms is None
    cf = ppo_ref.ClosedForm(c, 0.2, 0.01, 0.5, True)
    cf.check(sf.dlogits.cpu().numpy(), sf.dvalues.cpu().numpy(), sf.log_prob.cpu().numpy(), sf.entropy.cpu().numpy(), sf.raw.cpu().numpy(), "python", cap=False)
    for k, name in enumerate(ppo_ref.STATS):
        assert getattr(sf, name).dim() == 0 and float(getattr(sf, name)) == float(sf.raw[k])
    assert float(flat) == float(sf.loss)
    # the index form: the stored arrays of the rollout, a minibatch of 64 rows; equal to the gathered call
    ci, mdi, _, _ = _case(64, "rec352", "repeat", False)
    ix = t(ci.index)
    li, si = ppo_loss(t(ci.logits), t(ci.actions), t(ci.old_log_prob), t(ci.advantages), mdi, values=t(ci.values), returns=t(ci.returns), index=ix, ent_coef=0.01)
    cfi = ppo_ref.ClosedForm(ci, 0.2, 0.01, 0.5, True)
    cfi.check(si.dlogits.cpu().numpy(), si.dvalues.cpu().numpy(), si.log_prob.cpu().numpy(), si.entropy.cpu().numpy(), si.raw.cpu().numpy(), "python index", cap=False)
    before = dict(vec_env._ppo_workspaces)
    ppo_loss(t(ci.logits), t(ci.actions), t(ci.old_log_prob), t(ci.advantages), mdi, index=ix)
    assert dict(vec_env._ppo_workspaces).keys() == before.keys() and all(vec_env._ppo_workspaces[k] is before[k] for k in before)
    e, se = ppo_loss(t(c.logits)[:0], t(c.actions)[:0], t(c.old_log_prob)[:0], t(c.advantages)[:0])
    assert float(e) == 0.0 and tuple(se.dlogits.shape) == (0, 60) and (se.raw == 0).all()


def test_autograd_leaf_and_scaled_loss():
    """logits as a leaf: loss.backward() leaves logits.grad equal to dlogits (values.grad to dvalues); (3 * loss).backward() scales them; without grad
    the loss carries no node; under no_grad neither."""
    import torch
    from balatro_gym_amd import ppo_loss
    for bf16 in (False, True):
        c, mdev, _, _ = _case(257, "rec384", None, bf16)
        t = lambda x: torch.from_numpy(x).cuda()   # noqa: E731
        dt = torch.bfloat16 if bf16 else torch.float32
        args = (t(c.actions), t(c.old_log_prob), t(c.advantages), mdev)
        kw = dict(returns=t(c.returns), ent_coef=0.01)
        lg = t(c.logits).to(dt).requires_grad_(True)
        v = t(c.values).requires_grad_(True)
        loss, st = ppo_loss(lg, *args, values=v, **kw)
        assert loss.requires_grad and loss.grad_fn is not None and loss.dim() == 0 and float(loss.detach()) == float(st.loss)
        loss.backward()
        assert lg.grad.dtype == dt and torch.equal(lg.grad.view(torch.int16 if bf16 else torch.int32), st.dlogits.view(torch.int16 if bf16 else torch.int32))
        assert torch.equal(v.grad.view(torch.int32), st.dvalues.view(torch.int32))
        assert float(st.dlogits.float().abs().sum()) > 0.0
        lg2 = t(c.logits).to(dt).requires_grad_(True)
        v2 = t(c.values).requires_grad_(True)
        loss2, st2 = ppo_loss(lg2, *args, values=v2, **kw)
        (3.0 * loss2).backward()
        want = (st2.dlogits.float() * 3.0).to(dt)
        assert torch.equal(lg2.grad.view(torch.int16 if bf16 else torch.int32), want.view(torch.int16 if bf16 else torch.int32))
        assert torch.equal(v2.grad, st2.dvalues * 3.0)
        # only the values require grad; nothing requires grad; no_grad
        v3 = t(c.values).requires_grad_(True)
        loss3, st3 = ppo_loss(t(c.logits).to(dt), *args, values=v3, **kw)
        loss3.backward()
        assert torch.equal(v3.grad.view(torch.int32), st3.dvalues.view(torch.int32))
        loss4, _ = ppo_loss(t(c.logits).to(dt), *args, values=t(c.values), **kw)
        assert not loss4.requires_grad and loss4.grad_fn is None
        with torch.no_grad():
            loss5, _ = ppo_loss(lg, *args, values=v, **kw)
        assert not loss5.requires_grad
        assert float(loss4) == float(loss.detach()) == float(loss5)


def test_mlp_takes_one_sgd_step_through_ppo_loss():
    """A two-layer MLP (153 -> 64 tanh -> 60 logits + 1 value) on 256 rows of encode_rows output, float32 on the GPU, takes one SGD step through
    ppo_loss.  Its twin runs in float64 on the CPU through ppo_ref.torch_statement, its logits and values pinned to the GPU's float32 values (straight
    through), so that the reference is taken where the kernel was.  The parameter gradients agree within the PROPAGATED bounds: ppo_ref's bound B of every
    dlogits / dvalues element carried through the absolute Jacobian (|h|, |W2|, |1 - h^2|, |x|), plus the float32 slack of the network's own passes:
    2**-14 of the sum of absolute terms of each gradient element (the forward activations carry at most (153 + 64) * 2**-24 < 2**-16, the backward dots
    over 256 rows 2**-16, tanh and its derivative a few ulp: below 2**-14 together)."""
    import torch
    from balatro_gym_amd import encode_rows, ppo_loss
    m = 256
    rows = _records(384)[:m].contiguous()
    x = encode_rows(rows, "produced", torch.float32)
    assert tuple(x.shape) == (m, 153)
    x = x / (1.0 + x.abs())   # (a fixed squashing of the raw features, the same on both sides)
    host_mask = rows.cpu().numpy()[:, 176:236].view(np.int8)
    torch.manual_seed(7)
    net = torch.nn.Sequential(torch.nn.Linear(153, 64), torch.nn.Tanh(), torch.nn.Linear(64, 61))
    twin = torch.nn.Sequential(torch.nn.Linear(153, 64), torch.nn.Tanh(), torch.nn.Linear(64, 61)).double()
    twin.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    net = net.cuda()
    out = net(x)
    logits, values = out[:, :60], out[:, 60]
    lg_host = logits.detach().cpu().numpy().copy()
    c = ppo_ref.synthetic(3, m, 1.0, True, hand_made=False, mask=host_mask)
    c.logits = lg_host                       # the learner's logits: the network's
    c.values = values.detach().cpu().numpy().copy()
    r = head_ref.Reference(lg_host, c.mask, seed=11, index0=0, t=0)
    c.actions = r.action.astype(np.int32)
    c.old_log_prob = (r.log_prob(c.actions) + np.random.default_rng(5).standard_normal(m) * ppo_ref.NOISE).astype(np.float32)
    t = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    before = [p.detach().clone() for p in net.parameters()]
    loss, st = ppo_loss(logits, t(c.actions), t(c.old_log_prob), t(c.advantages), rows, values=values.contiguous(), returns=t(c.returns), ent_coef=0.01)
    opt.zero_grad()
    loss.backward()
    grads = [p.grad.detach().cpu().numpy().astype(np.float64) for p in net.parameters()]
    opt.step()
    for p, b, g in zip(net.parameters(), before, grads):
        assert torch.allclose(p.detach(), b - 0.1 * p.grad, rtol=1e-6, atol=1e-8) and not torch.equal(p.detach(), b) and np.abs(g).sum() > 0.0
    # the float64 twin, pinned to the GPU's outputs
    cf = ppo_ref.ClosedForm(c, 0.2, 0.01, 0.5, True)
    assert cf.excluded.sum() == 0 and cf.decidable.all(), "the 256-row set must be decidable for this comparison"
    dl = st.dlogits.cpu().numpy()
    sh = cf.check(dl, st.dvalues.cpu().numpy(), st.log_prob.cpu().numpy(), st.entropy.cpu().numpy(), st.raw.cpu().numpy(), "mlp", cap=False)
    x64 = x.detach().cpu().double()
    out64 = twin(x64)
    pinned = out64 + (torch.from_numpy(np.concatenate([lg_host, c.values[:, None]], axis=1)).double() - out64).detach()
    scal, loss64 = ppo_ref.torch_statement(c, 0.2, 0.01, 0.5, True, ~cf.excluded, params=(pinned[:, :60], pinned[:, 60]))
    loss64.backward()
    want = [p.grad.numpy() for p in twin.parameters()]
    # the propagated bounds
    W1, b1, W2, b2 = (p.detach().numpy() for p in twin.parameters())
    B = np.concatenate([cf.grad_bound(cf.g, dl), (2.0 ** -22 * np.abs(cf.dvalues) + 1e-45)[:, None]], axis=1)          # [m, 61]
    D = np.abs(np.concatenate([cf.dlogits, cf.dvalues[:, None]], axis=1))                                              # |dout|
    worst = ppo_ref.check_mlp_gradients(grads, want, ppo_ref.mlp_gradient_bounds(B, D, (W1, b1), W2, x64.numpy()))
    assert abs(scal["loss"] - float(loss.detach())) <= cf.stat_bounds["loss"]
    print(f"mlp: largest share of a propagated bound {worst:.3f}; dlogits share {sh['dlogits']:.3f}")
