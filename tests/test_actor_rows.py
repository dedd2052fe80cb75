"""bg_actor_sample / bg_actor_evaluate / bg_actor_ppo_loss on the MI355X.  m in {1, 63, 64, 65, 130} (a partial block, exactly one, one past it, past two)
x Hin in {32, 96, 256} (the minimum, an odd count of 32s, the real width); over the fifteen shapes the other choices rotate so that each occurs with
every Hin: h dense and at a pitch wider than Hin, float32 and bfloat16 weights (dense, at a wider 16-byte aligned pitch and at an odd pitch: the vector and the element loads), with and without bias, masks read in place
from records a short step_many rollout wrote (tests/test_policy_head.py's) and one dense int8 mask per Hin.  The data holds an all-masked row, a masked
stored action, an out-of-range action and an out-of-range index (asserted on the CPU side before any launch, with the share of rows that take part).
  (a) logits_out is inside tests/actor_ref.py's bound of the float64 product;
  (b) actor_sample (both flags) and actor_evaluate are bit for bit sample_actions / evaluate_actions fed that logits_out, with and without logits_out;
  (c) actor_ppo_loss: every statistic, log_prob, entropy, dvalues and dlogits_out bit for bit ppo_loss fed logits_out, with and without index= and
      normalisation; dh, dweight, dbias inside their bounds; a bfloat16 dh is the exact rounding of the float32 one; an excluded row's dh is +0.0; two
      calls give the same bits;
  (d) RowActor: loss.backward() fills weight.grad, bias.grad and h.grad with the call's own outputs times the incoming scalar;
  (e) every refusal is BG_E_ARG with the call's name in the text, and nothing is written."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import actor_ref as ar

pytestmark = pytest.mark.gpu

MS = (1, 63, 64, 65, 130)
HINS = (32, 96, 256)
SHAPES = list(itertools.product(MS, HINS))
COEF = dict(clip_range=0.2, ent_coef=0.01, vf_coef=0.5)
BG_E_ARG = -1

_cache: dict = {}


def _variant(k):
    """The choices that rotate over the shapes: k = the shape's place in SHAPES (k % 3 is its Hin, so a period coprime to 3 meets every Hin)."""
    return dict(f32_weight=k % 2 == 0, with_bias=k % 4 != 1, wide_h=k % 2 == 1, wide_w=(3, 0, 8, 3)[k % 4], dense_mask=k % 5 == 4)


def _record_masks():
    """(records [rows, 384] uint8 on the device, their action masks int8 on the host): real records of a short step_many rollout."""
    if "records" not in _cache:
        from tests.test_policy_head import _records
        rows = _records()[384][:2 * max(MS)].clone()
        _cache["records"] = (rows, rows.cpu().numpy()[:, 176:236].view(np.int8).copy())
    return _cache["records"]


def _bf16(bits):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).cuda().view(torch.bfloat16)


def _bits(t):
    import torch
    t = t.contiguous()
    return (t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16)).cpu().numpy()


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {int((g != w).sum())} of {w.size} elements differ"


class Dev:
    """A case on the device, laid out as its variant says."""

    def __init__(self, c, v):
        import torch
        self.c = c
        dev = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
        hp = c.Hin + (8 if v["wide_h"] else 0)
        self.hbuf = torch.full((c.m, hp), float("nan"), dtype=torch.bfloat16, device="cuda")
        self.h = self.hbuf[:, :c.Hin]
        self.h.copy_(_bf16(c.hb))
        wp = c.Hin + v["wide_w"]
        wt = dev(c.weight) if c.weight.dtype == np.float32 else _bf16(c.weight)
        self.wbuf = torch.full((60, wp), float("nan"), dtype=wt.dtype, device="cuda")
        self.w = self.wbuf[:, :c.Hin]
        self.w.copy_(wt)
        self.b = dev(c.bias)
        if v["dense_mask"]:
            self.mask = dev(c.mask)
        else:
            self.mask = _record_masks()[0][:c.store_rows].clone()
            self.mask[:, 176:236] = dev(c.mask.view(np.uint8))
        self.actions, self.old, self.adv, self.ret, self.values, self.index = (dev(x) for x in (c.actions, c.old_log_prob, c.advantages, c.returns, c.values, c.index))


def _case(k, with_index):
    key = ("case", k, with_index)
    if key not in _cache:
        m, Hin = SHAPES[k]
        v = _variant(k)
        c = ar.make_case(100 * k + with_index, m, Hin, _record_masks()[1], with_index, v["f32_weight"], v["with_bias"])
        # the data is what the test says it is, before anything is launched
        part = c.takes_part()
        assert 2 * int(part.sum()) >= m, (m, Hin, int(part.sum()))
        if m >= 16:
            ok, s = c.src()
            assert (c.mask[s[3]] == 0).all(), "row 3 reads an all-masked record"
            a5 = c.actions[s[5]]
            assert c.mask[s[5], a5] == 0 and (c.mask[s[5]] != 0).any(), "row 5's stored action is masked, others are not"
            assert c.actions[s[9]] == 60, "row 9's stored action is out of range"
            assert not with_index or (not ok[7] and c.index[7] == c.store_rows), "row 7's index is out of range"
            assert not part[3] and not part[5] and not part[9] and (not with_index or not part[7])
        _cache[key] = (c, Dev(c, v))
    return _cache[key]


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=[f"m{m}-Hin{H}" for m, H in SHAPES])
def test_logits_and_head(k):
    import torch
    from balatro_gym_amd import actor_evaluate, actor_sample, evaluate_actions, sample_actions
    c, d = _case(k, False)
    m, what = c.m, f"m {c.m} Hin {c.Hin} {_variant(k)}"
    seed, t, index0 = 77 + k, 5 + k, 1000 * k
    lo = torch.full((m, 60), -777.0, device="cuda")
    a, lp, en = actor_sample(d.h, d.w, d.b, d.mask, seed=seed, t=t, index0=index0, logits_out=lo)
    # (a)
    ref, bound = ar.logits(c.hb, ar.weight_bits(c.weight), c.bias)
    got = lo.cpu().numpy()
    ar.check_close(got, ref, bound, what + ": logits_out")
    # (b) the head on these logits, bit for bit; the same without logits_out and at a wider logits_out
    ra, rlp, ren = sample_actions(lo, d.mask, seed=seed, t=t, index0=index0)
    for x, y, n in ((a, ra, "actions"), (lp, rlp, "log_prob"), (en, ren, "entropy")):
        _same(x, y, f"{what}: sample {n}")
    if m >= 16:
        assert int(a[3]) == -1 and bool(torch.isnan(lp[3])), "the all-masked row is degenerate"
    picked = a.cpu().numpy()
    live = picked >= 0
    assert (c.mask[np.flatnonzero(live), picked[live]] != 0).all(), "a masked action was drawn"
    a2, lp2, en2 = actor_sample(d.h, d.w, d.b, d.mask, seed=seed, t=t, index0=index0)
    wide = torch.full((m, 64), -777.0, device="cuda")
    a3, lp3, en3 = actor_sample(d.h, d.w, d.b, d.mask, seed=seed, t=t, index0=index0, logits_out=wide[:, :60])
    for x, y, z in ((a, a2, a3), (lp, lp2, lp3), (en, en2, en3)):
        _same(x, y, what + ": without logits_out")
        _same(x, z, what + ": wide logits_out")
    _same(wide[:, :60], lo, what + ": wide logits_out")
    assert bool((wide[:, 60:] == -777.0).all()), "a padding column of logits_out was written"
    da, dlp, den = actor_sample(d.h, d.w, d.b, d.mask, seed=seed, t=t, index0=index0, deterministic=True)
    rda, rdlp, rden = sample_actions(lo, d.mask, seed=seed, t=t, index0=index0, deterministic=True)
    for x, y, n in ((da, rda, "actions"), (dlp, rdlp, "log_prob"), (den, rden, "entropy")):
        _same(x, y, f"{what}: deterministic {n}")
    lo2 = torch.full((m, 60), -777.0, device="cuda")
    for given in (a, d.actions):   # the drawn actions (a -1 among them) and the stored ones (a masked one, a 60)
        elp, een = actor_evaluate(d.h, d.w, d.b, given, d.mask, logits_out=lo2)
        relp, reen = evaluate_actions(lo, given, d.mask)
        _same(elp, relp, what + ": evaluate log_prob")
        _same(een, reen, what + ": evaluate entropy")
        _same(lo2, lo, what + ": evaluate logits_out")
        elp2, een2 = actor_evaluate(d.h, d.w, d.b, given, d.mask)
        _same(elp2, elp, what + ": evaluate without logits_out")
        _same(een2, een, what + ": evaluate without logits_out")
    assert torch.equal(d.hbuf[:, c.Hin:].isnan(), torch.ones_like(d.hbuf[:, c.Hin:], dtype=torch.bool)), "h's padding was written"


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=[f"m{m}-Hin{H}" for m, H in SHAPES])
def test_ppo_loss(k):
    import torch
    from balatro_gym_amd import actor_evaluate, actor_ppo_loss, ppo_loss
    from balatro_gym_amd.rows import actor_rows_per_group
    for with_index in (False, True):
        c, d = _case(k, with_index)
        m, Hin = c.m, c.Hin
        wb = ar.weight_bits(c.weight)
        part = c.takes_part()
        L = actor_rows_per_group(m, Hin)
        assert L == ar.rows_per_group(m, Hin)
        for normalize in (True, False):
            what = f"m {m} Hin {Hin} index {with_index} normalize {normalize} {_variant(k)}"
            kw = dict(values=d.values, returns=d.ret, index=d.index, normalize_advantage=normalize, **COEF)
            lo, dlo = torch.full((m, 60), -777.0, device="cuda"), torch.full((m, 60), -777.0, device="cuda")
            loss, st = actor_ppo_loss(d.h, d.w, d.b, d.actions, d.old, d.adv, d.mask, dh_dtype=torch.float32, logits_out=lo, dlogits_out=dlo, **kw)
            ref, bound = ar.logits(c.hb, wb, c.bias)
            ar.check_close(lo.cpu().numpy(), ref, bound, what + ": logits_out")
            if not with_index and normalize:   # the head calls and the loss compute the same logits, bit for bit (a first epoch's ratio is exactly 1)
                lo_head = torch.full((m, 60), -777.0, device="cuda")
                actor_evaluate(d.h, d.w, d.b, d.actions, d.mask, logits_out=lo_head)
                _same(lo_head, lo, what + ": the head calls' logits")
            # (c) bit for bit ppo_loss on these logits
            rloss, rst = ppo_loss(lo, d.actions, d.old, d.adv, d.mask, **kw)
            _same(st.raw, rst.raw, what + ": stats")
            _same(loss, rloss, what + ": loss")
            for n in ("log_prob", "entropy", "dvalues"):
                _same(getattr(st, n), getattr(rst, n), f"{what}: {n}")
            _same(dlo, rst.dlogits, what + ": dlogits_out")
            assert st.dlogits is dlo and int(st.excluded) == m - int(part.sum()), what
            # the layer's gradients from dp = bfloat16(dlogits)
            dp = ar.dp_values(dlo.cpu().numpy())
            dh = st.dh.cpu().numpy()
            want, bound = ar.dh(dp, wb)
            ar.check_close(dh, want, bound, what + ": dh")
            assert (dh[~part].view(np.uint32) == 0).all(), what + ": an excluded row's dh is +0.0"
            dw, dwb, db, dbb = ar.dweight(dp, c.hb, L)
            ar.check_close(st.dweight.cpu().numpy(), dw, dwb, what + ": dweight")
            ar.check_close(st.dbias.cpu().numpy(), db, dbb, what + ": dbias")
            # a bfloat16 dh is the rounding of the float32 one; without the optional tiles and a second time: the same bits
            loss2, st2 = actor_ppo_loss(d.h, d.w, d.b, d.actions, d.old, d.adv, d.mask, dh_dtype=torch.bfloat16, **kw)
            assert np.array_equal(_bits(st2.dh).view(np.uint16), ar.to_bf16_bits(dh)), what + ": bfloat16 dh"
            assert st2.dlogits is None
            loss3, st3 = actor_ppo_loss(d.h, d.w, d.b, d.actions, d.old, d.adv, d.mask, dh_dtype=torch.float32, **kw)
            for x, y in ((st2, st), (st3, st)):
                for n in ("raw", "log_prob", "entropy", "dvalues", "dweight", "dbias"):
                    _same(getattr(x, n), getattr(y, n), f"{what}: {n} of a second call")
            _same(st3.dh, st.dh, what + ": dh of a second call")
        # without the value term
        loss4, st4 = actor_ppo_loss(d.h, d.w, d.b, d.actions, d.old, d.adv, d.mask, index=d.index, logits_out=lo, **COEF)
        rloss4, rst4 = ppo_loss(lo, d.actions, d.old, d.adv, d.mask, index=d.index, **COEF)
        _same(st4.raw, rst4.raw, "stats without the value term")
        assert st4.dvalues is None


@pytest.mark.parametrize("Hin,dtype", [(256, "bfloat16"), (96, "float32")])
def test_row_actor_backward(Hin, dtype):
    import torch
    from balatro_gym_amd import RowActor
    k = SHAPES.index((130, Hin))
    c, d = _case(k, True)
    torch.manual_seed(3)
    lin = torch.nn.Linear(Hin, 60).cuda()
    layer = RowActor.from_linear(lin, dtype=getattr(torch, dtype))
    back = layer.to_linear()
    assert torch.equal(back.weight, lin.weight) and torch.equal(back.bias, lin.bias) and back.weight.device == lin.weight.device
    h = d.h.clone().requires_grad_(True)
    values = d.values.clone().requires_grad_(True)
    loss, st = layer.ppo_loss(h, d.actions, d.old, d.adv, d.mask, values=values, returns=d.ret, index=d.index, **COEF)
    assert loss.requires_grad and st.dh.dtype == getattr(torch, dtype)
    scale = torch.tensor(3.0, device="cuda")
    (loss * scale).backward()
    _same(layer.weight.grad, st.dweight * scale, "weight.grad")
    _same(layer.bias.grad, st.dbias * scale, "bias.grad")
    _same(h.grad, (st.dh * scale).to(torch.bfloat16), "h.grad")
    _same(values.grad, st.dvalues * scale, "values.grad")
    assert h.grad.dtype == torch.bfloat16 and float(st.dweight.abs().sum()) > 0 and float(st.dh.float().abs().sum()) > 0
    # the same numbers as the functional call with these parameters; act / evaluate run and agree with each other
    from balatro_gym_amd import actor_ppo_loss
    _, st2 = actor_ppo_loss(d.h, layer.weight.detach(), layer.bias.detach(), d.actions, d.old, d.adv, d.mask, values=d.values, returns=d.ret, index=d.index,
                            dh_dtype=getattr(torch, dtype), **COEF)
    for n in ("raw", "dh", "dweight", "dbias"):
        _same(getattr(st2, n), getattr(st, n), n)
    c0, d0 = _case(k, False)
    a, lp, en = layer.act(d0.h, d0.mask, seed=9, t=1)
    elp, een = layer.evaluate(d0.h, a, d0.mask)
    _same(elp, lp, "evaluate(act) log_prob")
    _same(een, en, "evaluate(act) entropy")


class _Raw:
    """bg_actor_ppo_loss / bg_actor_sample / bg_actor_evaluate through the C ABI over one good argument set, every output poisoned."""

    def __init__(self):
        import torch
        from balatro_gym_amd import _native as nat
        self.L = nat.load()
        c, d = _case(SHAPES.index((65, 96)), True)
        self.c, self.d, m, Hin = c, d, c.m, c.Hin
        f = lambda *shape: torch.full(shape, -1234.5, dtype=torch.float32, device="cuda")   # noqa: E731
        self.out = dict(dh=f(m, Hin), dweight=f(60, Hin), dbias=f(64), dvalues=f(m), log_prob=f(m), entropy=f(m), stats=f(16), logits_out=f(m, 60),
                        dlogits_out=f(m, 60), actions=torch.full((m,), -99, dtype=torch.int32, device="cuda"))
        self.ws = torch.zeros(int(self.L.bg_actor_ppo_loss_workspace_bytes(C.c_int64(m), Hin)) + 32, dtype=torch.uint8, device="cuda")
        assert self.ws.numel() - 32 == ar.workspace_bytes(m, Hin)
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        o = self.out
        self.good = dict(h=p(d.h), hs=d.h.stride(0), Hin=Hin, w=p(d.w), wdt=0 if d.w.dtype == torch.float32 else 1, ws_=d.w.stride(0), b=p(d.b),
                         mask=d.mask.data_ptr() + 176, ms=384, actions=p(d.actions), old=p(d.old), adv=p(d.adv), values=p(d.values), returns=p(d.ret),
                         index=p(d.index), store=c.store_rows, m=m, clip=0.2, ent=0.01, vf=0.5, flags=1, dh=p(o["dh"]), dhdt=0, dhs=Hin, dweight=p(o["dweight"]),
                         dbias=p(o["dbias"]), dvalues=p(o["dvalues"]), lp=p(o["log_prob"]), en=p(o["entropy"]), stats=p(o["stats"]), lo=p(o["logits_out"]), los=60,
                         dlo=p(o["dlogits_out"]), dlos=60, wsp=p(self.ws), wsb=self.ws.numel() - 32, out_actions=p(o["actions"]), seed=1, index0=0, t=0, sflags=0)

    def _layer(self, a):
        vp, u64 = C.c_void_p, C.c_uint64
        return [vp(a["h"]), u64(a["hs"]), a["Hin"], vp(a["w"]), a["wdt"], u64(a["ws_"]), vp(a["b"]), vp(a["mask"]), u64(a["ms"])]

    def ppo(self, **over):
        import torch
        a = {**self.good, **over}
        vp, u64 = C.c_void_p, C.c_uint64
        return self.L.bg_actor_ppo_loss(*self._layer(a), vp(a["actions"]), vp(a["old"]), vp(a["adv"]), vp(a["values"]), vp(a["returns"]), vp(a["index"]),
                                        C.c_int64(a["store"]), C.c_int64(a["m"]), C.c_float(a["clip"]), C.c_float(a["ent"]), C.c_float(a["vf"]), C.c_uint32(a["flags"]),
                                        vp(a["dh"]), a["dhdt"], u64(a["dhs"]), vp(a["dweight"]), vp(a["dbias"]), vp(a["dvalues"]), vp(a["lp"]), vp(a["en"]),
                                        vp(a["stats"]), vp(a["lo"]), u64(a["los"]), vp(a["dlo"]), u64(a["dlos"]), vp(a["wsp"]), u64(a["wsb"]), None,
                                        vp(torch.cuda.current_stream().cuda_stream))

    def sample(self, **over):
        import torch
        a = {**self.good, "mask": self.good["mask"], **over}
        vp, u64 = C.c_void_p, C.c_uint64
        return self.L.bg_actor_sample(*self._layer(a), C.c_int64(a["m"]), C.c_uint32(a["sflags"]), u64(a["seed"]), u64(a["index0"]), u64(a["t"]),
                                      vp(a["out_actions"]), vp(a["lp"]), vp(a["en"]), vp(a["lo"]), u64(a["los"]), None, vp(torch.cuda.current_stream().cuda_stream))

    def evaluate(self, **over):
        import torch
        a = {**self.good, **over}
        vp, u64 = C.c_void_p, C.c_uint64
        return self.L.bg_actor_evaluate(*self._layer(a), C.c_int64(a["m"]), vp(a["actions"]), vp(a["lp"]), vp(a["en"]), vp(a["lo"]), u64(a["los"]), None,
                                        vp(torch.cuda.current_stream().cuda_stream))

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(bool((t == (-99 if t.dtype == torch.int32 else -1234.5)).all()) for t in self.out.values())

    def error(self):
        return self.L.bg_last_error(None).decode()


def test_refusals_launch_nothing():
    import torch
    r = _Raw()
    g = r.good
    a4 = lambda name: g[name] + 4   # noqa: E731
    common = [dict(Hin=0), dict(Hin=16), dict(Hin=48), dict(Hin=1056), dict(Hin=-32), dict(h=None), dict(h=g["h"] + 2), dict(h=g["h"] + 8), dict(hs=g["Hin"] - 8),
              dict(hs=g["Hin"] + 4), dict(w=None), dict(w=g["w"] + 1), dict(wdt=2), dict(ws_=g["Hin"] - 1), dict(b=g["b"] + 2), dict(mask=g["mask"] + 2), dict(ms=56),
              dict(ms=62), dict(m=-1), dict(lo=g["lo"] + 2), dict(los=59), dict(lp=g["en"]), dict(lo=g["lp"]), dict(lp=g["h"]), dict(en=g["b"])]
    ppo_only = [dict(flags=2), dict(clip=0.0), dict(clip=1.0), dict(clip=float("nan")), dict(ent=float("inf")), dict(vf=float("nan")), dict(actions=None), dict(old=None),
                dict(adv=a4("adv") - 2), dict(values=None), dict(returns=None), dict(values=None, returns=None), dict(index=g["index"] + 2), dict(store=-1), dict(store=2 ** 31),
                dict(dh=None), dict(dhdt=2), dict(dhdt=1, dh=g["dh"] + 1), dict(dhs=g["Hin"] - 1), dict(dweight=None), dict(dbias=None), dict(dweight=g["dweight"] + 2),
                dict(stats=None), dict(dlo=g["dlo"] + 2), dict(dlos=59), dict(wsp=None), dict(wsp=g["wsp"] + 8), dict(wsb=g["wsb"] - 1), dict(wsb=0),
                dict(dh=g["h"]), dict(dweight=g["w"]), dict(dbias=g["b"]), dict(dlo=g["lo"]), dict(dh=g["dweight"]), dict(dvalues=g["values"]), dict(lp=g["old"]),
                dict(stats=g["dbias"]), dict(wsp=g["dh"]), dict(lo=g["dh"]), dict(en=g["adv"])]
    for over in common + ppo_only:
        assert r.ppo(**over) == BG_E_ARG, over
        assert r.error().startswith("bg_actor_ppo_loss: "), (over, r.error())
    for over in common + [dict(sflags=2), dict(out_actions=None), dict(out_actions=g["out_actions"] + 2), dict(out_actions=g["lp"]), dict(lo=g["out_actions"])]:
        assert r.sample(**over) == BG_E_ARG, over
        assert r.error().startswith("bg_actor_sample: "), (over, r.error())
    for over in common + [dict(actions=None), dict(actions=g["actions"] + 2), dict(lp=g["actions"])]:
        assert r.evaluate(**over) == BG_E_ARG, over
        assert r.error().startswith("bg_actor_evaluate: "), (over, r.error())
    assert r.untouched(), "a refused call wrote to an output"
    # the same arguments unchanged are accepted, and an empty call zeroes what the loss would have summed
    assert r.sample() == 0 and r.evaluate() == 0 and r.ppo() == 0, r.error()
    torch.cuda.synchronize()
    assert float(r.out["stats"][9]) == r.c.m and float(r.out["stats"][10]) == -1234.5 and float(r.out["dbias"][60]) == -1234.5
    assert r.ppo(m=0) == 0, r.error()
    torch.cuda.synchronize()
    assert bool((r.out["stats"][:10] == 0).all()) and bool((r.out["dweight"] == 0).all()) and bool((r.out["dbias"][:60] == 0).all())
    assert float(r.out["stats"][10]) == -1234.5 and float(r.out["dbias"][60]) == -1234.5
    assert r.sample(m=0) == 0 and r.evaluate(m=0) == 0
    # the Python calls on an empty batch return empty tensors and zeros
    from balatro_gym_amd import actor_ppo_loss, actor_sample
    e = torch.zeros((0, 96), dtype=torch.bfloat16, device="cuda")
    z, zi = torch.zeros(0, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")
    a, lp, en = actor_sample(e, r.d.w, r.d.b, seed=1, t=0)
    assert a.shape == lp.shape == en.shape == (0,)
    loss, st = actor_ppo_loss(e, r.d.w, r.d.b, zi, z, z)
    assert float(loss) == 0.0 and st.dh.shape == (0, 96) and not bool(st.dweight.any()) and not bool(st.dbias.any())
