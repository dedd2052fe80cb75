"""bg_actor_sample / bg_actor_evaluate / bg_actor_ppo_loss on the CPU (no GPU): the header's declarations and the library's exports; csrc/bg_actor.h
compiled with g++ under BG_ACTOR_HOST -- the tile and fragment index functions the kernels use and the serial twin that drives them through a scalar model
of v_mfma_f32_32x32x16_bf16 -- held to tests/actor_ref.py: exactly on small integers (any accumulation order is exact there, so a wrong lane map cannot
pass), inside the derived bounds on random data for the logits, dp, dh, dweight and dbias; the twin's statistics bit for bit bg_ppo_host's on the twin's
logits; the split of the rows into groups and the workspace size against the statement; the argument checks of the Python wrappers on CPU stand-ins; and
RowActor's parameters to and from nn.Linear."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import actor_ref as ar
from tests.first_layer_helpers import _decl
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")

_PROGRAM = r"""
#define BG_ACTOR_HOST
#include <stdio.h>
#include <stdlib.h>
#include "balatro_mi355x.h"
#include "bg_actor.h"
static BgPpoArgs ppo_args(const int8_t* mask, uint64_t mstride, const int32_t* actions, const float* old_lp, const float* adv, const float* values,
                          const float* returns, const int32_t* index, int64_t store_rows, int64_t m, float clip, float ent_coef, float vf_coef, uint32_t flags,
                          float* logits, float* dlogits, float* dvalues, float* log_prob, float* entropy) {
  BgPpoArgs A = {};
  A.logits = logits; A.lstride = 60; A.mask = mask; A.mstride = mstride; A.actions = actions; A.old_lp = old_lp; A.adv = adv; A.values = values;
  A.returns = returns; A.index = index; A.store_rows = store_rows; A.m = m;
  A.c.clip = clip; A.c.lo = 1.0f - clip; A.c.hi = 1.0f + clip; A.c.ent_coef = ent_coef; A.c.vf_coef = vf_coef; A.c.fm = (float)m;
  A.normalize = flags & BG_PPO_NORMALIZE_ADV ? 1 : 0;
  A.dlogits = dlogits; A.dstride = 60; A.dvalues = dvalues; A.log_prob = log_prob; A.entropy = entropy;
  return A;
}
static BgActorArgs actor_args(const uint16_t* h, uint64_t hstride, int Hin, const void* weight, int w_bf16, uint64_t wstride, const float* bias) {
  BgActorArgs G = {};
  G.h = h; G.hstride = hstride; G.Hin = Hin; G.weight = weight; G.w_bf16 = w_bf16; G.wstride = wstride; G.bias = bias;
  return G;
}
extern "C" void actor_logits(const uint16_t* h, uint64_t hstride, int Hin, const void* weight, int w_bf16, uint64_t wstride, const float* bias, int64_t m,
                             float* logits) {
  bg_actor_host_logits(actor_args(h, hstride, Hin, weight, w_bf16, wstride, bias), m, logits);
}
extern "C" void actor_host(const uint16_t* h, uint64_t hstride, int Hin, const void* weight, int w_bf16, uint64_t wstride, const float* bias,
                           const int8_t* mask, uint64_t mstride, const int32_t* actions, const float* old_lp, const float* adv, const float* values,
                           const float* returns, const int32_t* index, int64_t store_rows, int64_t m, float clip, float ent_coef, float vf_coef,
                           uint32_t flags, float* logits, float* dlogits, uint16_t* dp, float* dh, float* dweight, float* dbias, float* dvalues,
                           float* log_prob, float* entropy, float* stats) {
  const BgPpoArgs A = ppo_args(mask, mstride, actions, old_lp, adv, values, returns, index, store_rows, m, clip, ent_coef, vf_coef, flags, logits, dlogits,
                               dvalues, log_prob, entropy);
  bg_actor_host(A, actor_args(h, hstride, Hin, weight, w_bf16, wstride, bias), stats, dp, dh, dweight, dbias);
}
extern "C" void ppo_host(const int8_t* mask, uint64_t mstride, const int32_t* actions, const float* old_lp, const float* adv, const float* values,
                         const float* returns, const int32_t* index, int64_t store_rows, int64_t m, float clip, float ent_coef, float vf_coef, uint32_t flags,
                         float* logits, float* dlogits, float* dvalues, float* log_prob, float* entropy, float* stats) {
  bg_ppo_host(ppo_args(mask, mstride, actions, old_lp, adv, values, returns, index, store_rows, m, clip, ent_coef, vf_coef, flags, logits, dlogits, dvalues,
                       log_prob, entropy), false, false, stats);
}
extern "C" void actor_split(int64_t m, int Hin, int64_t* out) {
  out[3] = (int64_t)bg_act_workspace_bytes(m, Hin); out[4] = bg_act_hin_ok(Hin);
  if (!out[4]) return;   // (the split is defined for a width the calls accept)
  out[0] = bg_act_groups(m, Hin); out[1] = bg_act_blocks_per_group(m, Hin); out[2] = bg_act_spans(Hin);
}
"""

COEF = (0.2, 0.01, 0.5)


class Host:
    def __init__(self, lib):
        self.lib = lib
        for f in (lib.actor_logits, lib.actor_host, lib.ppo_host, lib.actor_split):
            f.restype = None
        vp, u64, i64, f = C.c_void_p, C.c_uint64, C.c_int64, C.c_float
        self.layer = [vp, u64, C.c_int, vp, C.c_int, u64, vp]
        self.ppo = [vp, u64, vp, vp, vp, vp, vp, vp, i64, i64, f, f, f, C.c_uint32]
        lib.actor_logits.argtypes = self.layer + [i64, vp]
        lib.actor_host.argtypes = self.layer + self.ppo + [vp] * 10
        lib.ppo_host.argtypes = self.ppo + [vp] * 6
        lib.actor_split.argtypes = [i64, C.c_int, vp]

    @staticmethod
    def _layer(c, hpitch=None, wpitch=None):
        hp, wp = hpitch or c.Hin, wpitch or c.Hin
        h = np.full((c.m, hp), 0x7FC0, np.uint16)
        h[:, :c.Hin] = c.hb
        w = np.full((ar.UNITS, wp), np.nan if c.weight.dtype == np.float32 else 0x7FC0, c.weight.dtype)
        w[:, :c.Hin] = c.weight
        return h, w, [h.ctypes.data, hp, c.Hin, w.ctypes.data, int(c.weight.dtype == np.uint16), wp, None if c.bias is None else c.bias.ctypes.data]

    @staticmethod
    def _ppo(c, normalize, use_values):
        p = lambda x: None if x is None else x.ctypes.data   # noqa: E731
        return [p(c.mask), 60, p(c.actions), p(c.old_log_prob), p(c.advantages), p(c.values) if use_values else None, p(c.returns) if use_values else None,
                p(c.index), c.store_rows, c.m, COEF[0], COEF[1], COEF[2], 1 if normalize else 0]

    def logits(self, c, **pitch):
        h, w, layer = self._layer(c, **pitch)
        out = np.full((c.m, 60), -777.0, np.float32)
        self.lib.actor_logits(*layer, c.m, out.ctypes.data)
        return out

    def run(self, c, normalize=True, use_values=True, **pitch):
        h, w, layer = self._layer(c, **pitch)
        m = c.m
        o = dict(logits=np.full((m, 60), -777.0, np.float32), dlogits=np.full((m, 60), -777.0, np.float32), dp=np.full((m, 60), 0x7B7B, np.uint16),
                 dh=np.full((m, c.Hin), -777.0, np.float32), dweight=np.full((60, c.Hin), -777.0, np.float32), dbias=np.full(60, -777.0, np.float32),
                 dvalues=np.full(m, -777.0, np.float32) if use_values else None, log_prob=np.empty(m, np.float32), entropy=np.empty(m, np.float32),
                 stats=np.empty(10, np.float32))
        self.lib.actor_host(*layer, *self._ppo(c, normalize, use_values), *[None if v is None else v.ctypes.data for v in o.values()])
        return o

    def ppo_on(self, c, logits, normalize=True, use_values=True):
        m = c.m
        lg = np.ascontiguousarray(logits, np.float32).copy()
        o = dict(dlogits=np.empty((m, 60), np.float32), dvalues=np.empty(m, np.float32) if use_values else None, log_prob=np.empty(m, np.float32),
                 entropy=np.empty(m, np.float32), stats=np.empty(10, np.float32))
        self.lib.ppo_host(*self._ppo(c, normalize, use_values), lg.ctypes.data, *[None if v is None else v.ctypes.data for v in o.values()])
        return o

    def split(self, m, Hin):
        out = np.zeros(5, np.int64)
        self.lib.actor_split(m, Hin, out.ctypes.data)
        return [int(x) for x in out]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile csrc/bg_actor.h for the host"
    d = tmp_path_factory.mktemp("actor_host")
    src, so = d / "actor_host.cpp", d / "actor_host.so"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-Wall", "-fPIC", "-shared", "-I", CSRC, "-I", os.path.dirname(HEADER), "-o", str(so),
                           str(src)])
    return Host(C.CDLL(str(so)))


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _mask(seed, rows):
    return (np.random.default_rng(seed).random((rows, 60)) < 0.7).astype(np.int8)


def test_header_declares_and_library_exports():
    from balatro_gym_amd import _native as nat, build
    hdr = open(HEADER).read()
    layer = ["const void*", "uint64_t", "int", "const void*", "int", "uint64_t", "const float*", "const int8_t*", "uint64_t"]
    m, params = _decl(hdr, "int", "bg_actor_sample")
    want = layer + ["int64_t", "uint32_t", "uint64_t", "uint64_t", "uint64_t", "int32_t*", "float*", "float*", "float*", "uint64_t", "float*", "void*"]
    assert len(params) == len(want) and all(p.startswith(t) for p, t in zip(params, want)), params
    doc = hdr[:m.start()].rsplit("/*", 1)[1]
    for word in ("action_net", "nn.Linear(latent, 60)", "__builtin_amdgcn_mfma_f32_32x32x16_bf16", "bit for bit", "bg_ppo_loss", "bg_sample_actions", "NON-FINITE",
                 "BG_E_ARG", "float64", "Out of scope", "two calls give the same bits", "bg_actor_ppo_loss_rows_per_group", "nearest even", "LDS does not grow"):
        assert word in doc, word
    _, params = _decl(hdr, "int", "bg_actor_evaluate")
    want = layer + ["int64_t", "const int32_t*", "float*", "float*", "float*", "uint64_t", "float*", "void*"]
    assert len(params) == len(want) and all(p.startswith(t) for p, t in zip(params, want)), params
    for ret, name in (("uint64_t", "bg_actor_ppo_loss_workspace_bytes"), ("int64_t", "bg_actor_ppo_loss_rows_per_group")):
        _, params = _decl(hdr, ret, name)
        assert len(params) == 2 and params[0].startswith("int64_t") and params[1].startswith("int"), params
    _, params = _decl(hdr, "int", "bg_actor_ppo_loss")
    want = layer + ["const int32_t*", "const float*", "const float*", "const float*", "const float*", "const int32_t*", "int64_t", "int64_t", "float", "float",
                    "float", "uint32_t", "void*", "int", "uint64_t", "float*", "float*", "float*", "float*", "float*", "float*", "float*", "uint64_t", "float*",
                    "uint64_t", "void*", "uint64_t", "float*", "void*"]
    assert len(params) == len(want) and all(p.startswith(t) for p, t in zip(params, want)), params
    names = ("bg_actor_sample", "bg_actor_evaluate", "bg_actor_ppo_loss", "bg_actor_ppo_loss_workspace_bytes", "bg_actor_ppo_loss_rows_per_group")
    assert all(n in nat.EXPORTS for n in names)
    assert (nat.ACTOR_HIN_MIN, nat.ACTOR_HIN_MAX) == (32, 1024)
    assert any(d.endswith("bg_actor.h") for d in build.DEPS)
    if not os.path.exists(build.LIB):
        pytest.skip("library not built")
    L = C.CDLL(build.LIB)
    assert all(hasattr(L, n) for n in names)


def test_fragment_maps_are_exact_on_small_integers(host):
    """h in -5..5, weights in -4..4, integer bias: every partial sum is an integer far below 2**24, so float32 accumulation is exact in ANY order and the
    twin's logits must equal the integer product exactly -- at a partial block, past two blocks, at an odd count of 32s, with wide pitches, with both
    weight dtypes.  The asymmetric patterns make a swapped row / column / k index a mismatch."""
    for m, Hin, f32, bias in ((1, 32, True, False), (65, 96, False, True), (130, 256, True, True), (64, 160, False, False)):
        c = ar.Case()
        c.m, c.Hin = m, Hin
        i, k, j = np.arange(m)[:, None], np.arange(Hin)[None, :], np.arange(60)[:, None]
        c.hb = ar.to_bf16_bits(((7 * i + 3 * k) % 11 - 5).astype(np.float32))
        w = ((3 * j + 5 * k) % 9 - 4).astype(np.float32)
        c.weight = w if f32 else ar.to_bf16_bits(w)
        c.bias = ((np.arange(60) * 5) % 13 - 6).astype(np.float32) if bias else None
        want = ar.widen(c.hb) @ w.astype(np.float64).T + (0 if c.bias is None else c.bias.astype(np.float64))
        for pitch in ({}, {"hpitch": Hin + 8, "wpitch": Hin + 3}):
            got = host.logits(c, **pitch)
            assert np.array_equal(got.astype(np.float64), want), (m, Hin, f32, bias, pitch)


@pytest.mark.parametrize("m,Hin,masked,index,f32,bias", [(1, 32, True, False, True, True), (63, 96, True, True, False, True), (65, 256, False, False, True, False),
                                                           (130, 96, True, True, True, True), (300, 512, True, False, False, True)])
def test_twin_is_inside_the_bounds_and_its_statistics_are_the_ppo_twin_s(host, m, Hin, masked, index, f32, bias):
    c = ar.make_case(m * 3 + Hin, m, Hin, _mask(m, 2 * m) if masked else None, index, f32, bias)
    wb = ar.weight_bits(c.weight)
    for normalize, use_values in ((True, True), (False, False)):
        o = host.run(c, normalize, use_values, hpitch=Hin + 8 * (m % 2))
        what = f"m {m} Hin {Hin} normalize {normalize}"
        ref, bound = ar.logits(c.hb, wb, c.bias)
        ar.check_close(o["logits"], ref, bound, what + ": logits")
        # the statistics, log_prob, entropy, dvalues and dlogits: bg_ppo_host's on these logits, bit for bit
        p = host.ppo_on(c, o["logits"], normalize, use_values)
        for k in ("stats", "log_prob", "entropy", "dlogits") + (("dvalues",) if use_values else ()):
            assert np.array_equal(_bits(o[k]), _bits(p[k])), f"{what}: {k}"
        part = c.takes_part()
        assert int(o["stats"][8]) == m - int(part.sum()), what
        assert (o["dlogits"][~part] == 0).all() and not np.signbit(o["dlogits"][~part]).any()
        # dp is the nearest-even rounding of dlogits; dh, dweight and dbias are its products
        assert np.array_equal(o["dp"], ar.to_bf16_bits(o["dlogits"])), what + ": dp"
        dp = ar.dp_values(o["dlogits"])
        ref, bound = ar.dh(dp, wb)
        ar.check_close(o["dh"], ref, bound, what + ": dh")
        assert (_bits(o["dh"][~part]) == 0).all(), what + ": an excluded row's dh is +0.0"
        L = ar.rows_per_group(m, Hin)
        dw, dwb, db, dbb = ar.dweight(dp, c.hb, L)
        ar.check_close(o["dweight"], dw, dwb, what + ": dweight")
        ar.check_close(o["dbias"], db, dbb, what + ": dbias")


def test_split_and_workspace_match_the_statement(host):
    for m, Hin in ((1, 32), (64, 32), (65, 96), (4096, 256), (16385, 256), (65536, 256), (65536, 512), (65536, 1024), (10 ** 6, 768), (2 ** 24 + 1, 1024)):
        g, per, spans, ws, ok = host.split(m, Hin)
        assert ok == 1 and g == ar.groups(m, Hin) and per * 64 == ar.rows_per_group(m, Hin) and spans == -(-Hin // 256), (m, Hin)
        assert g * spans <= 256 and g * per >= -(-m // 64) > (g - 1) * per, (m, Hin)
        assert ws == ar.workspace_bytes(m, Hin), (m, Hin)
    assert ar.groups(65536, 512) == 128 and ar.rows_per_group(65536, 512) == 512
    for bad in (0, 16, 48, 1056, 2048, -32):
        assert host.split(64, bad)[3:] == [0, 0]
    assert host.split(0, 256)[3] == 0


def test_wrappers_refuse_bad_arguments_before_the_library():
    """actor_sample / actor_evaluate / actor_ppo_loss / RowActor on CPU stand-ins: every bad argument is a ValueError before anything is loaded; what is
    left of a good call is that there is no CPU path."""
    import torch
    from balatro_gym_amd import RowActor, actor_evaluate, actor_ppo_loss, actor_sample
    m, Hin = 6, 64
    h = torch.zeros((m, Hin), dtype=torch.bfloat16)
    w, b = torch.zeros((60, Hin)), torch.zeros(60)
    a, f = torch.zeros(m, dtype=torch.int32), torch.zeros(m)
    rows = torch.zeros((m, 384), dtype=torch.uint8)
    kw = dict(seed=1, t=0)
    for bad_h in (h.float(), torch.zeros((m, 48), dtype=torch.bfloat16), torch.zeros((m, 2048), dtype=torch.bfloat16), torch.zeros((m, 2 * Hin), dtype=torch.bfloat16)[:, ::2],
                  torch.zeros((m, Hin + 4), dtype=torch.bfloat16)[:, :Hin], "h"):
        with pytest.raises(ValueError, match="h must|Hin, the last dimension of h"):
            actor_sample(bad_h, w, b, **kw)
        with pytest.raises(ValueError, match="h must|Hin, the last dimension of h"):
            actor_ppo_loss(bad_h, w, b, a, f, f)
    for bad_w in (torch.zeros((64, Hin)), torch.zeros((60, Hin + 32)), w.double(), torch.zeros((60, 2 * Hin))[:, ::2], torch.zeros(60 * Hin), None):
        with pytest.raises(ValueError, match=r"weight must be a float32 / bfloat16 tensor \[60, 64\]"):
            actor_evaluate(h, bad_w, b, a)
    for bad_b in (torch.zeros(64), torch.zeros(60, dtype=torch.bfloat16), torch.zeros(120)[::2], [0.0] * 60):
        with pytest.raises(ValueError, match="bias must be a contiguous torch.float32"):
            actor_sample(h, w, bad_b, **kw)
    for name, bad in (("seed", -1), ("t", 2 ** 64), ("index0", 1.5), ("seed", True)):
        with pytest.raises(ValueError, match=name + " must be an integer"):
            actor_sample(h, w, b, **{**kw, name: bad})
    with pytest.raises(ValueError, match="mask must"):
        actor_sample(h, w, b, torch.zeros((m, 60)), **kw)
    with pytest.raises(ValueError, match="leading shape"):
        actor_sample(h, w, b, torch.zeros((m + 1, 60), dtype=torch.int8), **kw)
    for bad_lo in (torch.zeros((m, 59)), torch.zeros((m, 60), dtype=torch.bfloat16), torch.zeros((m + 1, 60)), torch.zeros((m, 120))[:, ::2]):
        with pytest.raises(ValueError, match="logits_out must be"):
            actor_sample(h, w, b, logits_out=bad_lo, **kw)
        with pytest.raises(ValueError, match="dlogits_out must be"):
            actor_ppo_loss(h, w, b, a, f, f, dlogits_out=bad_lo)
    with pytest.raises(ValueError, match="actions must be"):
        actor_evaluate(h, w, b, a.long())
    with pytest.raises(ValueError, match="actions must be"):
        actor_ppo_loss(h, w, b, a[:-1], f, f)
    with pytest.raises(ValueError, match="old_log_prob must be"):
        actor_ppo_loss(h, w, b, a, f.double(), f)
    with pytest.raises(ValueError, match="values and returns go together"):
        actor_ppo_loss(h, w, b, a, f, f, values=f)
    with pytest.raises(ValueError, match="index must be a contiguous torch.int32"):
        actor_ppo_loss(h, w, b, a, f, f, index=a.long())
    with pytest.raises(ValueError, match="clip_range must be in"):
        actor_ppo_loss(h, w, b, a, f, f, clip_range=1.0)
    with pytest.raises(ValueError, match="ent_coef must be a finite number"):
        actor_ppo_loss(h, w, b, a, f, f, ent_coef=float("nan"))
    with pytest.raises(ValueError, match="dh_dtype must be"):
        actor_ppo_loss(h, w, b, a, f, f, dh_dtype=torch.float16)
    for bad_in in (48, 0, 1056, 16):
        with pytest.raises(ValueError, match="multiple of 32"):
            RowActor(bad_in)
    with pytest.raises(ValueError, match="float32 or torch.bfloat16"):
        RowActor(Hin, dtype=torch.float16)
    layer = RowActor(Hin)
    for call in (lambda: actor_sample(h, w, b, rows, **kw), lambda: actor_sample(h, w.bfloat16(), None, torch.ones((m, 60), dtype=torch.int8), deterministic=True, **kw),
                 lambda: actor_evaluate(h, w, b, a, rows, logits_out=torch.zeros((m, 64))[:, :60]),
                 lambda: actor_ppo_loss(h, w, b, a, f, f, rows, values=f, returns=f), lambda: actor_ppo_loss(h, w, None, torch.zeros(9, dtype=torch.int32), torch.zeros(9), torch.zeros(9), index=a),
                 lambda: layer.act(h, rows, **kw), lambda: layer.evaluate(h, a, rows), lambda: layer.ppo_loss(h, a, f, f, rows)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()


def test_row_actor_parameters_round_trip():
    """RowActor is initialised as nn.Linear(in_features, 60) (same generator draws) and from_linear / to_linear move SB3's action_net exactly."""
    import torch
    from balatro_gym_amd import RowActor
    for Hin in (256, 512):
        torch.manual_seed(11)
        layer = RowActor(Hin)
        torch.manual_seed(11)
        twin = torch.nn.Linear(Hin, 60)
        assert layer.weight.shape == (60, Hin) and layer.bias.shape == (60,) and layer.weight.dtype == layer.bias.dtype == torch.float32
        assert torch.equal(layer.weight, twin.weight) and torch.equal(layer.bias, twin.bias)
        assert layer.weight.requires_grad and layer.bias.requires_grad and sorted(dict(layer.named_parameters())) == ["bias", "weight"]
        lin2 = layer.to_linear()
        assert isinstance(lin2, torch.nn.Linear) and (lin2.in_features, lin2.out_features) == (Hin, 60)
        assert torch.equal(lin2.weight, layer.weight) and torch.equal(lin2.bias, layer.bias) and lin2.weight.data_ptr() != layer.weight.data_ptr()
        back = RowActor.from_linear(lin2, dtype=torch.float32)
        assert back.dtype == torch.float32 and torch.equal(back.weight, layer.weight) and torch.equal(back.bias, layer.bias)
        lin2.load_state_dict(back.state_dict())
    for bad in (torch.nn.Linear(256, 64), torch.nn.Linear(256, 60, bias=False), torch.nn.Linear(100, 60), "linear"):
        with pytest.raises(ValueError):
            RowActor.from_linear(bad)
