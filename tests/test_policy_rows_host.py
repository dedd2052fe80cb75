"""bg_policy_forward on the CPU (no GPU): the header's declarations and the library's exports; csrc/bg_policy.h compiled with g++ under BG_POLICY_HOST --
the fragment, image and table index functions the kernel uses and the serial twin that drives them through a scalar model of
v_mfma_f32_32x32x16_bf16 -- held to tests/policy_ref.py: EQUAL on the exact cases (any accumulation order is exact there, so a wrong lane map, image
swap or layer order cannot pass), inside the derived per-layer intervals on the reference's topology, to the contract's bits on the activations'
special values (policy_ref.special_case) and on pitched weights; the envelope check; the argument checks of
RowDense / RowPolicy on CPU stand-ins; from_modules / to_modules; stack_blocks and its mask under an optimiser step; latent() against plain modules."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import policy_ref as pr
from tests.first_layer_helpers import _decl
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")

_PROGRAM = r"""
#define BG_POLICY_HOST
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include "balatro_mi355x.h"
#include "bg_policy.h"
static_assert(sizeof(BgPolicyNet) == sizeof(BgPolNet) && sizeof(BgPolicyLayer) == sizeof(BgPolLayer) && offsetof(BgPolicyNet, layer) == offsetof(BgPolNet, layer), "one table");
extern "C" const char* pol_check(const BgPolicyNet* n) { return bg_pol_check((const BgPolNet*)n); }
extern "C" int pol_tap_cols(const BgPolicyNet* n) { return bg_pol_tap_cols(*(const BgPolNet*)n); }
extern "C" void pol_host(const BgPolicyNet* n, int mode, const uint16_t* h, uint64_t hstride, const int8_t* mask, uint64_t mstride, int64_t m, uint64_t seed,
                         uint64_t index0, uint64_t t, int32_t* actions, float* log_prob, float* entropy, float* values, uint16_t* taps, float* logits) {
  bg_policy_host(*(const BgPolNet*)n, mode, h, hstride, mask, mstride, m, seed, index0, t, actions, log_prob, entropy, values, taps, logits);
}
extern "C" void pol_images(int ntrunk, int n, int* out) {
  out[0] = bg_pol_trunk_img(ntrunk);
  for (int q = 0; q < n; q++) { out[1 + 2 * q] = bg_pol_branch_in(ntrunk, q); out[2 + 2 * q] = bg_pol_branch_out(ntrunk, q); }
  out[1 + 2 * n] = bg_pol_branch_last(ntrunk, n);
}
"""
SAMPLE, ARGMAX, EVALUATE = 0, 1, 2


def table(net, wide=0):
    """A policy_ref.Net -> (the host table as the wrapper's own dtype builds it, the arrays it points to)."""
    from balatro_gym_amd.policy import _NET
    t = np.zeros(1, _NET)
    n, keep = t[0], []
    n["n_trunk"], n["n_pi"], n["n_vf"], n["has_value"], n["in0"] = len(net.trunk), len(net.pi), len(net.vf), int(net.value is not None), net.in0
    for k, l in enumerate(net.hidden() + [net.action] + ([net.value] if net.value is not None else [])):
        w = np.full((l.out, l.in_ + wide), 0x7FC0, np.uint16)   # the padding of a wide pitch is NaN: never read
        w[:, :l.in_] = l.wb
        storage = np.zeros(w.size + 8, np.uint16)
        off = (-storage.ctypes.data % 16) // 2
        wa = storage[off:off + w.size].reshape(w.shape)
        wa[:] = w
        keep += [storage, l.bias]
        e = n["layer"][k]
        e["weight"], e["bias"], e["pitch"], e["in"], e["out"], e["act"] = wa.ctypes.data, l.bias.ctypes.data, l.in_ + wide, l.in_, l.out, pr.ACT[l.act]
    return t, keep


class Host:
    def __init__(self, lib):
        self.lib = lib
        vp, u64, i64 = C.c_void_p, C.c_uint64, C.c_int64
        lib.pol_check.restype, lib.pol_check.argtypes = C.c_char_p, [vp]
        lib.pol_tap_cols.restype, lib.pol_tap_cols.argtypes = C.c_int, [vp]
        lib.pol_host.restype, lib.pol_host.argtypes = None, [vp, C.c_int, vp, u64, vp, u64, i64, u64, u64, u64, vp, vp, vp, vp, vp, vp]
        lib.pol_images.restype, lib.pol_images.argtypes = None, [C.c_int, C.c_int, vp]

    def check(self, t):
        r = self.lib.pol_check(t.ctypes.data)
        return None if r is None else r.decode()

    def run(self, net, hb, mode=SAMPLE, mask=None, actions=None, seed=3, index0=0, t=1, hpitch=None, wide=0, taps=True):
        tab, keep = table(net, wide)
        assert self.check(tab) is None, self.check(tab)
        m = len(hb)
        hp = hpitch or net.in0
        h = np.full((m, hp), 0x7FC0, np.uint16)
        h[:, :net.in0] = hb
        o = dict(actions=np.full(m, -7, np.int32) if actions is None else actions.copy(), log_prob=np.empty(m, np.float32), entropy=np.empty(m, np.float32),
                 values=np.full(m, -777.0, np.float32) if net.value is not None else None,
                 taps=np.full((m, net.tap_cols()), 0x7B7B, np.uint16) if taps else None, logits=np.full((m, 60), -777.0, np.float32) if taps else None)
        p = lambda x: None if x is None else x.ctypes.data   # noqa: E731
        self.lib.pol_host(tab.ctypes.data, mode, h.ctypes.data, hp, p(mask), 60, m, seed, index0, t, *[p(v) for v in o.values()])
        return o


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile csrc/bg_policy.h for the host"
    d = tmp_path_factory.mktemp("policy_host")
    src, so = d / "policy_host.cpp", d / "policy_host.so"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-Wall", "-fPIC", "-shared", "-I", CSRC, "-I", os.path.dirname(HEADER), "-o", str(so),
                           str(src)])
    return Host(C.CDLL(str(so)))


def test_header_declares_and_library_exports():
    from balatro_gym_amd import _native as nat, build
    hdr = open(HEADER).read()
    m, params = _decl(hdr, "int", "bg_policy_forward")
    want = ["const BgPolicyNet*", "const void*", "uint64_t", "const int8_t*", "uint64_t", "int64_t", "uint32_t", "uint64_t", "uint64_t", "uint64_t", "int32_t*",
            "float*", "float*", "float*", "void*", "uint64_t", "float*", "uint64_t", "float*", "void*"]
    assert len(params) == len(want) and all(p.startswith(t) for p, t in zip(params, want)), params
    doc = hdr[:m.start()].rsplit("/* ----", 1)[1]
    for word in ("mlp_extractor", "action_net", "value_net", "__builtin_amdgcn_mfma_f32_32x32x16_bf16", "bit for bit", "bg_sample_actions", "BG_E_ARG", "HOST memory",
                 "multiple of 32 in [32, 512]", "tanh(y) = sign(y) * (1 - 2 / (expf(2 |y|) + 1))", "Out of scope", "two calls give the same bits", "nearest-even",
                 "LDS does not grow", "changes no other output bit"):
        assert word in doc, word
    for name in ("bg_policy_check", "bg_policy_tap_cols"):
        _, params = _decl(hdr, "int", name)
        assert len(params) == 1 and params[0].startswith("const BgPolicyNet*"), params
    names = ("bg_policy_forward", "bg_policy_check", "bg_policy_tap_cols")
    assert all(n in nat.EXPORTS for n in names)
    assert (nat.POLICY_WIDTH_MIN, nat.POLICY_WIDTH_MAX, nat.POLICY_MAX_SECTION, nat.POLICY_MAX_LAYERS, nat.POLICY_EVALUATE) == (32, 512, 4, 14, 2)
    for macro, value in (("BG_POLICY_ACT_NONE", 0), ("BG_POLICY_ACT_RELU", 1), ("BG_POLICY_ACT_TANH", 2), ("BG_POLICY_MAX_LAYERS", 14), ("BG_POLICY_MAX_WIDTH", 512)):
        assert f"#define {macro} {value}" in hdr, macro
    assert nat.POLICY_ACTIVATIONS == {None: 0, "relu": 1, "tanh": 2}
    assert any(d.endswith("bg_policy.h") for d in build.DEPS)
    if not os.path.exists(build.LIB):
        pytest.skip("library not built")
    L = C.CDLL(build.LIB)
    assert all(hasattr(L, n) for n in names)


def test_images_never_collide(host):
    """A layer never writes the image it reads, a branch never writes the trunk's output, and a section's last output is where the next reader looks."""
    for nt in range(5):
        for n in range(5):
            out = np.zeros(2 * n + 2, np.int32)
            host.lib.pol_images(nt, n, out.ctypes.data)
            trunk = int(out[0])
            assert trunk == nt % 2
            prev = trunk
            for q in range(n):
                i, o = int(out[1 + 2 * q]), int(out[2 + 2 * q])
                assert i == prev and o != i and o != trunk and 0 <= o < 3, (nt, n, q, i, o)
                prev = o
            assert int(out[1 + 2 * n]) == prev


@pytest.mark.parametrize("name", list(pr.EXACT))
def test_twin_equals_the_integers_on_the_exact_cases(host, name):
    for m in pr.MS:
        net = pr.exact_net(pr.EXACT[name], 11)
        hb = pr.exact_h(m, net.in0, 5 + m)
        taps, logits, values = pr.exact_forward(net, hb)
        for kw in ({}, dict(hpitch=net.in0 + 8, wide=8)):
            o = host.run(net, hb, **kw)
            assert np.array_equal(o["taps"], taps), (name, m, kw)
            assert np.array_equal(o["logits"].astype(np.float64), logits), (name, m, kw)
            if values is not None:
                assert np.array_equal(o["values"].astype(np.float64), values), (name, m, kw)


@pytest.mark.parametrize("act", ["tanh", "relu", None])
def test_twin_activations_at_their_special_values(host, act):
    """policy_ref.special_case: +-0, the smallest normal, tanh's saturation, +-inf, NaN and a subnormal operand through an identity layer; the finite
    rows of the workgroup do not notice the non-finite ones beside them."""
    c = pr.special_case(act)
    o = host.run(c["net"], c["hb"], seed=3, t=1)
    pr.check_special(c, o["taps"], o["logits"], o["values"], o["actions"], o["log_prob"], f"twin, {act}")
    q = host.run(c["net"], c["hb_finite"], seed=3, t=1)
    keep = np.setdiff1d(np.arange(pr.SPECIAL_M), c["nonfinite"])
    for k in ("actions", "log_prob", "entropy", "values", "taps", "logits"):
        assert np.array_equal(o[k][keep].view(np.uint8), q[k][keep].view(np.uint8)), (act, k)
    assert np.isfinite(q["logits"]).all() and (q["actions"] >= 0).all()


def test_twin_reads_pitched_weights_and_equals_the_integers(host):
    """The case tests/test_policy_rows.py sends through the C ABI with pitched weights, taps and logits: the twin's taps and logits are dense by
    construction, so the weights' pitch (in + 8, NaN padding) and h's are what it can show."""
    from balatro_gym_amd.policy import _NET
    net, m = pr.exact_net(pr.EXACT["64-32|pi32|novf"], 11), 33
    hb = pr.exact_h(m, net.in0, 5 + m)
    taps, logits, values = pr.exact_forward(net, hb)
    assert values is None
    t = np.zeros(1, _NET)
    n, keep = t[0], []
    n["n_trunk"], n["n_pi"], n["n_vf"], n["has_value"], n["in0"] = 1, 1, 0, 0, net.in0
    for k, l in enumerate(net.hidden() + [net.action]):
        w, storage = pr.pitched(l.wb, l.in_ + 8, pr.QNAN)
        keep += [storage, l.bias]
        e = n["layer"][k]
        e["weight"], e["bias"], e["pitch"], e["in"], e["out"], e["act"] = w.ctypes.data, l.bias.ctypes.data, l.in_ + 8, l.in_, l.out, pr.ACT[l.act]
    assert host.check(t) is None
    h, hkeep = pr.pitched(hb, net.in0 + 8, pr.QNAN)
    got_t, got_l = np.full((m, net.tap_cols()), 0x7B7B, np.uint16), np.full((m, 60), -777.0, np.float32)
    a, lp, en = np.full(m, -7, np.int32), np.empty(m, np.float32), np.empty(m, np.float32)
    host.lib.pol_host(t.ctypes.data, SAMPLE, h.ctypes.data, net.in0 + 8, None, 60, m, 1, 0, m, a.ctypes.data, lp.ctypes.data, en.ctypes.data, None,
                      got_t.ctypes.data, got_l.ctypes.data)
    assert np.array_equal(got_t, taps) and np.array_equal(got_l.astype(np.float64), logits)
    assert ((a >= 0) & (a < 60)).all() and np.isfinite(lp).all()


def test_twin_is_inside_the_intervals_on_the_reference_topology(host):
    net = pr.random_net(pr.REFERENCE, 3)
    m = 70
    hb = pr.random_h(m, net.in0, 4)
    mask = (np.random.default_rng(9).random((m, 60)) < 0.6).astype(np.int8)
    mask[5] = 0
    o = host.run(net, hb, SAMPLE, mask, hpitch=net.in0 + 64, seed=21, index0=100, t=6)
    pr.check_taps(net, hb, o["taps"], o["logits"], o["values"], "twin, reference topology")
    # the test outputs change nothing else, and the head is a function of the logits
    q = host.run(net, hb, SAMPLE, mask, hpitch=net.in0 + 64, seed=21, index0=100, t=6, taps=False)
    for k in ("actions", "log_prob", "entropy", "values"):
        assert np.array_equal(o[k].view(np.uint32), q[k].view(np.uint32)), k
    a = o["actions"]
    assert a[5] == -1 and np.isnan(o["log_prob"][5])
    live = np.arange(m) != 5
    assert (mask[live, a[live]] != 0).all()
    d = host.run(net, hb, ARGMAX, mask)
    z = np.where(mask != 0, o["logits"], -np.inf)
    assert np.array_equal(d["actions"][live], z.argmax(1)[live]), "deterministic: the first valid maximum"
    e = host.run(net, hb, EVALUATE, mask, actions=a)
    assert np.array_equal(e["log_prob"][live].view(np.uint32), o["log_prob"][live].view(np.uint32))
    # rows do not depend on the rows around them
    part = host.run(net, hb[40:], SAMPLE, mask[40:], hpitch=net.in0 + 64, seed=21, index0=140, t=6)
    for k in ("actions", "log_prob", "entropy", "values", "taps", "logits"):
        assert np.array_equal(o[k][40:].view(np.uint8), part[k].view(np.uint8)), k


def test_the_envelope_is_checked(host):
    net = pr.random_net(pr.REFERENCE, 1)
    good, keep = table(net)
    assert host.check(good) is None and host.lib.pol_tap_cols(good.ctypes.data) == net.tap_cols() == 224 + 512 + 512 + 4 * 256

    def bad(change, text):
        t = good.copy()
        change(t[0])
        msg = host.check(t)
        assert msg is not None and text in msg, (text, msg)

    def setl(k, field, v):
        def f(n):
            n["layer"][k][field] = v
        return f
    bad(lambda n: n.__setitem__("n_trunk", 5), "at most 4 layers")
    bad(lambda n: n.__setitem__("has_value", 0), "vf layers need the value layer")
    bad(lambda n: n.__setitem__("in0", 440), "multiple of 32")
    bad(lambda n: n.__setitem__("in0", 544), "multiple of 32")
    bad(setl(0, "out", 240), "multiple of 32")
    bad(setl(1, "in", 256), "in_features must be the width of what it reads")
    bad(setl(3, "in", 256), "in_features must be the width of what it reads")   # pi[0] reads the trunk
    bad(setl(5, "in", 256), "in_features must be the width of what it reads")   # vf[0] reads the trunk, not pi
    bad(setl(7, "out", 64), "60 units")
    bad(setl(8, "out", 32), "1 unit")
    bad(setl(2, "act", 3), "activation must be")
    bad(setl(7, "act", 1), "take no activation")
    bad(setl(4, "weight", 0), "16-byte aligned")
    bad(setl(4, "weight", int(good[0]["layer"][4]["weight"]) + 2), "16-byte aligned")
    bad(setl(4, "pitch", 252), "multiple of 8")
    bad(setl(4, "pitch", 260), "multiple of 8")
    bad(setl(6, "bias", 0), "bias")
    assert host.lib.pol_check(None).decode().startswith("net must be")


def test_wrappers_refuse_bad_arguments_before_the_library():
    import torch
    from balatro_gym_amd import RowActor, RowDense, RowOptimizer, RowPolicy
    for i, o in ((48, 64), (64, 48), (544, 64), (64, 1024), (0, 32), (64, 16)):
        with pytest.raises(ValueError, match="multiple of 32"):
            RowDense(i, o)
    with pytest.raises(ValueError, match="activation must be"):
        RowDense(64, 64, "gelu")
    with pytest.raises(ValueError, match="mask must be"):
        RowDense(64, 32, None, mask=torch.ones(64, 32))
    d = lambda i, o, a="relu": RowDense(i, o, a)   # noqa: E731
    with pytest.raises(ValueError, match="at most 4"):
        RowPolicy([d(64, 64) for _ in range(5)], [], [], RowActor(64))
    with pytest.raises(ValueError, match="at most 4"):
        RowPolicy([], [d(64, 64) for _ in range(5)], [], RowActor(64))
    with pytest.raises(ValueError, match="vf given without value"):
        RowPolicy([], [], [d(64, 64)], RowActor(64))
    with pytest.raises(ValueError, match="reads 96 features"):
        RowPolicy([d(64, 64)], [d(96, 64)], [], RowActor(64))
    with pytest.raises(ValueError, match="action reads 128 features"):
        RowPolicy([d(64, 64)], [], [], RowActor(128))
    with pytest.raises(ValueError, match="value reads"):
        RowPolicy([d(64, 64)], [], [d(64, 32)], RowActor(64), RowDense(64, 1))
    with pytest.raises(ValueError, match="multiple of 32 in"):
        RowPolicy([], [], [], RowActor(1024))
    with pytest.raises(ValueError, match="value must be"):
        RowPolicy([], [], [], RowActor(64), d(64, 32))
    with pytest.raises(ValueError, match="must be a RowDense"):
        RowPolicy([torch.nn.Linear(64, 64)], [], [], RowActor(64))
    with pytest.raises(ValueError, match="action must be a RowActor"):
        RowPolicy([], [], [], torch.nn.Linear(64, 60))
    with pytest.raises(ValueError, match="pair"):
        RowPolicy.from_modules(trunk=[torch.nn.Linear(64, 64)], action_net=torch.nn.Linear(64, 60))
    with pytest.raises(ValueError, match="activation must be"):
        RowPolicy.from_modules(trunk=[(torch.nn.Linear(64, 64), "elu")], action_net=torch.nn.Linear(64, 60))
    policy = RowPolicy([d(64, 96)], [d(96, 64, "tanh")], [d(96, 32, "tanh")], RowActor(64), RowDense(32, 1))
    m = 6
    h = torch.zeros((m, 64), dtype=torch.bfloat16)
    kw = dict(seed=1, t=0)
    for bad_h in (h.float(), torch.zeros((m, 96), dtype=torch.bfloat16), torch.zeros((m, 128), dtype=torch.bfloat16)[:, ::2],
                  torch.zeros((m, 68), dtype=torch.bfloat16)[:, :64], "h"):
        with pytest.raises(ValueError, match="h must|last dimension of h"):
            policy.act(bad_h, **kw)
        with pytest.raises(ValueError, match="h must|last dimension of h"):
            policy.evaluate(bad_h, torch.zeros(m, dtype=torch.int32))
    with pytest.raises(ValueError, match="mask must"):
        policy.act(h, torch.zeros((m, 60)), **kw)
    with pytest.raises(ValueError, match="leading shape"):
        policy.act(h, torch.zeros((m + 1, 60), dtype=torch.int8), **kw)
    with pytest.raises(ValueError, match="a uint8 mask is"):
        policy.act(h, torch.zeros((m, 100), dtype=torch.uint8), **kw)
    for name, v in (("seed", -1), ("t", 2 ** 64), ("index0", 1.5), ("seed", True)):
        with pytest.raises(ValueError, match=name + " must be an integer"):
            policy.act(h, **{**kw, name: v})
    with pytest.raises(ValueError, match="actions must be"):
        policy.evaluate(h, torch.zeros(m, dtype=torch.int64))
    with pytest.raises(ValueError, match="actions must be"):
        policy.evaluate(h, [0] * m)
    for call in (lambda: policy.act(h, torch.zeros((m, 384), dtype=torch.uint8), **kw), lambda: policy.act(h, deterministic=True, taps=True, **kw),
                 lambda: policy.evaluate(h, torch.zeros(m, dtype=torch.int32), torch.ones((m, 60), dtype=torch.int8))):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()
    # RowOptimizer.attach takes the new layers (an additive change) and still refuses what it refused
    opt = RowOptimizer(list(policy.parameters()))
    with pytest.raises(ValueError, match="attach takes"):
        opt.attach(torch.nn.Linear(64, 64))
    with pytest.raises(ValueError, match="not one of this optimiser's parameters"):
        opt.attach(RowDense(64, 64))
    opt.attach(policy)
    for layer in policy.layers():
        assert layer.weight_bf16 is not None and layer.weight_bf16.dtype == torch.bfloat16 and layer._weight_bf16_version == layer.weight._version
        assert torch.equal(layer.weight_bf16, layer.weight.detach().bfloat16()) and layer.weight_bf16.stride(0) == layer.in_features


def _reference_modules(seed=0):
    import torch
    torch.manual_seed(seed)
    nn = torch.nn
    return dict(trunk=[(nn.Linear(448, 224), "relu"), (nn.Linear(224, 512), "relu"), (nn.Linear(512, 512), "relu")],
                pi=[(nn.Linear(512, 256), "tanh"), (nn.Linear(256, 256), "tanh")], vf=[(nn.Linear(512, 256), "tanh"), (nn.Linear(256, 256), "tanh")],
                action_net=nn.Linear(256, 60), value_net=nn.Linear(256, 1))


def test_from_modules_and_to_modules_round_trip_exactly():
    import torch
    from balatro_gym_amd import RowPolicy
    mods = _reference_modules()
    policy = RowPolicy.from_modules(**mods)
    assert (len(policy.trunk), len(policy.pi), len(policy.vf), policy.in_features, policy.tap_cols) == (3, 2, 2, 448, 224 + 512 + 512 + 4 * 256)
    back = policy.to_modules()
    for sec in ("trunk", "pi", "vf"):
        assert len(back[sec]) == len(mods[sec])
        for (a, act_a), (b, act_b) in zip(mods[sec], back[sec]):
            assert act_a == act_b and torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias) and a.weight.data_ptr() != b.weight.data_ptr()
    for k in ("action_net", "value_net"):
        assert torch.equal(mods[k].weight, back[k].weight) and torch.equal(mods[k].bias, back[k].bias)
    again = RowPolicy.from_modules(**back)
    assert all(torch.equal(p, q) for p, q in zip(policy.parameters(), again.parameters()))
    assert len(list(policy.parameters())) == 2 * 9 and all(p.dtype == torch.float32 and p.requires_grad for p in policy.parameters())
    no_value = RowPolicy.from_modules(pi=[(torch.nn.Linear(64, 32), "tanh")], action_net=torch.nn.Linear(32, 60))
    assert no_value.value is None and no_value.to_modules()["value_net"] is None and no_value.latent(torch.zeros((2, 64), dtype=torch.bfloat16))[1] is None
    # a RowDense is initialised as nn.Linear (same generator draws)
    from balatro_gym_amd import RowDense
    torch.manual_seed(4)
    a = RowDense(96, 64, "tanh")
    torch.manual_seed(4)
    b = torch.nn.Linear(96, 64)
    assert torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)


def test_stack_blocks_is_block_diagonal_and_stays_so():
    import torch
    from balatro_gym_amd import RowPolicy
    torch.manual_seed(2)
    parts = [torch.nn.Linear(256, 128), torch.nn.Linear(128, 64), torch.nn.Linear(64, 32)]
    layer = RowPolicy.stack_blocks(parts, "relu")
    assert (layer.in_features, layer.out_features, layer.activation) == (448, 224, "relu") and tuple(layer.block_mask.shape) == (224, 448)
    on = layer.block_mask != 0
    assert int(on.sum()) == 256 * 128 + 128 * 64 + 64 * 32 and (layer.weight[~on] == 0).all()
    assert torch.equal(layer.weight[:128, :256], parts[0].weight) and torch.equal(layer.weight[128:192, 256:384], parts[1].weight)
    assert torch.equal(layer.weight[192:, 384:], parts[2].weight) and torch.equal(layer.bias, torch.cat([p.bias for p in parts]))
    # the stacked layer computes the three layers side by side
    x = torch.randn(5, 448)
    want = torch.cat([torch.relu(p(x[:, c0:c1])) for p, (c0, c1) in zip(parts, ((0, 256), (256, 384), (384, 448)))], 1)
    assert torch.allclose(layer(x), want, atol=1e-5)
    before = layer.weight.detach().clone()
    for opt in (torch.optim.Adam(layer.parameters(), lr=1e-2), torch.optim.RMSprop(layer.parameters(), lr=1e-2)):
        for _ in range(3):
            opt.zero_grad()
            layer(torch.randn(16, 448)).square().sum().backward()
            assert (layer.weight.grad[~on] == 0).all()
            opt.step()
    assert (layer.weight[~on] == 0).all() and not torch.equal(layer.weight[on], before[on])
    with pytest.raises(ValueError, match="multiple of 32"):
        RowPolicy.stack_blocks([torch.nn.Linear(64, 48), torch.nn.Linear(64, 32)])


def test_latent_is_the_plain_modules_in_bfloat16():
    """latent() against nn.Sequential over copies of the same modules after .to(torch.bfloat16): bit for bit, values and gradients' presence."""
    import copy

    import torch
    from balatro_gym_amd import RowPolicy
    nn = torch.nn
    mods = _reference_modules(5)
    policy = RowPolicy.from_modules(**mods)
    acts = {"relu": nn.ReLU, "tanh": nn.Tanh}
    seq = lambda pairs: nn.Sequential(*[x for lin, a in pairs for x in (copy.deepcopy(lin), acts[a]())]).to(torch.bfloat16)   # noqa: E731
    trunk, pi, vf = seq(mods["trunk"]), seq(mods["pi"]), seq(mods["vf"])
    value_net = copy.deepcopy(mods["value_net"]).to(torch.bfloat16)
    h = torch.randn(37, 448).to(torch.bfloat16)
    with torch.no_grad():
        x = trunk(h)
        want_pi, want_v = pi(x), value_net(vf(x)).float().squeeze(-1)
    lat, values = policy.latent(h)
    assert lat.dtype == torch.bfloat16 and values.dtype == torch.float32 and tuple(values.shape) == (37,)
    assert torch.equal(lat.detach().view(torch.int16), want_pi.view(torch.int16)) and torch.equal(values.detach().view(torch.int32), want_v.view(torch.int32))
    (lat.float().sum() + values.sum()).backward()
    assert all(p.grad is not None and p.grad.dtype == torch.float32 for n, p in policy.named_parameters() if not n.startswith("action."))
