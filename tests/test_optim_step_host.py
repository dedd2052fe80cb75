"""bg_optim_step and RowOptimizer on the CPU (no GPU).
(i)   tests/optim_ref.py -- the contract in numpy float32 -- takes one step from a random state and stays inside the bound derived there of
      torch.optim.Adam on float64 tensors behind clip_grad_norm_, and of SB3's RMSpropTFLike restated in torch float64.  torch's float32 bits are NOT
      demanded: its vectorised CPU path differs from a one-rounding-per-operation restatement by ulps from about 1 000 elements on.
(ii)  csrc/bg_optim.h -- the element functions the kernels run and the serial twin of the launch sequence -- compiled with g++ (-O1 -ffp-contract=off
      -DBG_OPTIM_HOST) is held to optim_ref BIT FOR BIT on p, both states, shadows, targets, gradients, grad_norm, clip_coef and step: both algorithms,
      clip active and inactive, wd 0 and 0.01, zero_grad on and off, tau 0 / 0.005 / 1, three consecutive steps, and a table of 339 chunks so that a
      lane of the combining fold takes two partials; the skip on NaN and Inf; the shadow-only pass.
(iii) the bfloat16 rounding (the header's and optim_ref's) against x.to(torch.bfloat16) for all 65 536 high halves times five low halves.
(iv)  the header's declarations, the exports, build.DEPS, __all__, RowOptimizer's argument checks and attach's version rule on CPU tensors.

Largest observed shares of the one-step bound against float64 (i): Adam p 0.999, m 0.86, v 0.71; RMSpropTFLike p 0.997, sq 0.70 (the bound is tight where
it should be: u |v| is half an ulp of a value just above a power of two, and p's last addition alone can use all of it)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import optim_ref as R
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")
FOLD_SHAPES = R.BASE_SHAPES + [(300 * 1024 + 7,)]   # 38 + 301 = 339 chunks: the 256 lanes of the combine fold two partials each

_PROGRAM = r"""
#define BG_OPTIM_HOST
#include <stdio.h>
#include <stdlib.h>
#include "balatro_mi355x.h"
#include "bg_optim.h"
extern "C" void optim_host(const void* table, int ntensors, int64_t chunks, int algo, double lr, double beta1, double beta2, double eps, double wd,
                           double max_norm, double tau, uint32_t flags, void* carry, void* stats) {
  const BgOptHyper h = bg_optim_hyper(algo, lr, beta1, beta2, eps, wd, max_norm, tau, flags);
  bg_optim_host((const BgOptTensor*)table, ntensors, chunks, h, (BgOptCarry*)carry, (BgOptStats*)stats);
}
extern "C" void bf16_host(const float* x, uint16_t* out, int64_t n) { for (int64_t i = 0; i < n; i++) out[i] = bg_ppo_bf16(x[i]); }
extern "C" uint64_t ws_host(int64_t chunks) { return bg_optim_ws_bytes(chunks); }
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile csrc/bg_optim.h for the host"
    d = tmp_path_factory.mktemp("optim_host")
    src = d / "optim_host.cpp"
    src.write_text(_PROGRAM)
    so = d / "optim_host.so"
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-I", os.path.dirname(HEADER), "-o", str(so), str(src)])
    lib = C.CDLL(str(so))
    d_ = C.c_double
    lib.optim_host.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int, d_, d_, d_, d_, d_, d_, d_, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.optim_host.restype = None
    lib.bf16_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.bf16_host.restype = None
    lib.ws_host.argtypes = [C.c_int64]
    lib.ws_host.restype = C.c_uint64
    return lib


def _host_step(lib, tensors, h: R.Hyper, carry, flags=None):
    table, chunks = R.pack_table(tensors)
    stats = np.zeros(1, R.STATS)
    if flags is None:
        flags = R.ZERO_GRAD if h.zero_grad else 0
    lib.optim_host(table.ctypes.data, len(tensors), chunks, h.algo, h.lr, h.beta1, h.beta2, h.raw["eps"], h.raw["weight_decay"], h.raw["max_norm"], h.raw["tau"],
                   flags, carry.ctypes.data, stats.ctypes.data)
    return stats[0]


def _compare(dut, ref, st, want, carry, rc, what):
    for i, (a, b) in enumerate(zip(dut, ref)):
        for name in ("p", "g", "s1", "s2", "target", "shadow"):
            x, y = getattr(a, name), getattr(b, name)
            assert (x is None) == (y is None)
            if x is not None:
                assert R.same_bits(x, y), (what, i, name, int((x.view(np.uint8) != y.view(np.uint8)).sum()))
    for k in ("grad_norm", "clip_coef"):
        assert np.float32(st[k]).tobytes() == np.float32(want[k]).tobytes(), (what, k, st[k], want[k])
    assert (int(st["skipped"]), int(st["nonfinite"]), int(st["step"]), int(st["zero"])) == (want["skipped"], want["nonfinite"], want["step"], 0), (what, st, want)
    assert (int(carry["step"][0]), float(carry["b1pow"][0]), float(carry["b2pow"][0])) == (rc.step, rc.b1pow, rc.b2pow), what


def _new_grads(rng, dut, ref, scale=1.0):
    for a, b in zip(dut, ref):
        g = (rng.normal(0, 1, a.g.size) * scale).astype(np.float32)
        a.g[:] = g
        b.g[:] = g


def _carry_at(step, h):
    c = np.zeros(1, R.CARRY)
    rc = R.Carry.at(step, h.beta1, h.beta2) if h.algo == R.ADAM else R.Carry(step)
    c["step"], c["b1pow"], c["b2pow"] = rc.step, rc.b1pow, rc.b2pow
    return c, rc


CONFIGS = [(algo, max_norm, wd, zg, tau) for algo in (R.ADAM, R.RMSPROP_TF) for max_norm, wd, zg, tau in
           ((0.5, 0.0, True, 0.0), (0.0, 0.01, False, 0.005), (1e6, 0.01, True, 1.0), (0.5, 0.01, False, 1.0), (-1.0, 0.0, True, 0.005))]


# ---------------------------------------------------------------- (i) the reference against float64
def _torch_step64(h: R.Hyper, step_before, data):
    import torch
    ps = [torch.tensor(d["p"].astype(np.float64), requires_grad=True) for d in data]
    for p, d in zip(ps, data):
        p.grad = torch.tensor(d["g"].astype(np.float64))
    if h.raw["max_norm"] > 0:
        torch.nn.utils.clip_grad_norm_(ps, h.raw["max_norm"])
    if h.algo == R.ADAM:
        opt = torch.optim.Adam(ps, lr=h.lr, betas=(h.beta1, h.beta2), eps=h.raw["eps"], weight_decay=h.raw["weight_decay"])
        for p, d in zip(ps, data):
            opt.state[p] = {"step": torch.tensor(float(step_before)), "exp_avg": torch.tensor(d["s1"].astype(np.float64)),
                            "exp_avg_sq": torch.tensor(d["s2"].astype(np.float64))}
        opt.step()
        return [(p.detach().numpy(), opt.state[p]["exp_avg"].numpy(), opt.state[p]["exp_avg_sq"].numpy()) for p in ps]
    out = []
    with torch.no_grad():   # SB3's RMSpropTFLike.step, uncentred, without momentum
        for p, d in zip(ps, data):
            g, sq = p.grad, torch.tensor(d["s1"].astype(np.float64))
            if h.raw["weight_decay"] != 0:
                g = g.add(p, alpha=h.raw["weight_decay"])
            sq.mul_(h.beta1).addcmul_(g, g, value=1 - h.beta1)
            avg = sq.add(h.raw["eps"]).sqrt_()
            p.addcdiv_(g, avg, value=-h.lr)
            out.append((p.numpy(), sq.numpy(), None))
    return out


@pytest.mark.parametrize("algo,max_norm,wd,zg,tau", CONFIGS)
def test_the_contract_is_within_its_bound_of_float64(algo, max_norm, wd, zg, tau):
    h = R.Hyper(algo, lr=3e-4 if algo == R.ADAM else 7e-4, beta1=0.9 if algo == R.ADAM else 0.99, weight_decay=wd, max_norm=max_norm)
    shares = {}
    for seed, step_before, gscale in ((1, 0, 1.0), (2, 7, 1e-3), (3, 999, 30.0)):
        data = R.random_set(seed + 10 * algo, R.BASE_SHAPES, algo, gscale)
        want = _torch_step64(h, step_before, data)
        S, _ = R.grad_norm([d["g"] for d in data])
        carry = R.Carry.at(step_before, h.beta1, h.beta2) if algo == R.ADAM else R.Carry(step_before)
        _, _, _, stats = R.finish(S, 0, h, carry)
        tensors = [R.Tensor(d["p"].copy(), d["g"].copy(), d["s1"].copy(), d["s2"].copy() if algo == R.ADAM else None) for d in data]
        carry2 = R.Carry.at(step_before, h.beta1, h.beta2) if algo == R.ADAM else R.Carry(step_before)
        R.step(tensors, R.Hyper(algo, h.lr, h.beta1, h.beta2, h.raw["eps"], wd, max_norm, zero_grad=False), carry2)
        for d, t, (p64, s1_64, s2_64) in zip(data, tensors, want):
            P, S1, V = R.step_bound(h, carry, S, d["p"], d["g"], d["s1"], d["s2"] if algo == R.ADAM else None)
            assert R.same_bits(P.v, t.p) and R.same_bits(S1.v, t.s1), "the bound is made of the values of the step it bounds"
            ex = R.exact_step(h, carry.step, d["p"], d["g"], d["s1"], d["s2"], float(np.sqrt(S)))
            assert np.allclose(ex[0], p64, rtol=1e-11, atol=1e-13) and np.allclose(ex[1], s1_64, rtol=1e-11, atol=1e-13), "exact_step is torch on float64"
            for name, got, ref64, E in (("p", t.p, p64, P), ("s1", t.s1, s1_64, S1)) + ((("s2", t.s2, s2_64, V),) if algo == R.ADAM else ()):
                err = np.abs(got.astype(np.float64) - ref64)
                assert (err <= E.e).all(), (name, step_before, float((err / E.e).max()))
                shares[name] = max(shares.get(name, 0.0), float((err / E.e).max()))
    print(f"algo {algo} max_norm {max_norm} wd {wd}: largest shares of the one-step bound {shares}")
    assert all(0.0 < v <= 1.0 for v in shares.values())


# ---------------------------------------------------------------- (ii) the header on the host
@pytest.mark.parametrize("algo,max_norm,wd,zg,tau", CONFIGS)
def test_three_steps_are_the_contract_bit_for_bit(host, algo, max_norm, wd, zg, tau):
    h = R.Hyper(algo, lr=3e-4 if algo == R.ADAM else 7e-4, beta1=0.9 if algo == R.ADAM else 0.99, weight_decay=wd, max_norm=max_norm, tau=tau, zero_grad=zg)
    dut, ref = R.host_set(R.random_set(5 + algo, R.BASE_SHAPES, algo), algo)
    assert dut[R.OFFSET_TENSOR].p.ctypes.data % 16 == 4 and dut[0].p.ctypes.data % 16 == 0
    carry, rc = _carry_at(3, h)
    rng = np.random.default_rng(99)
    for k in range(3):
        if k:
            _new_grads(rng, dut, ref, 10.0 ** -k)
        st = _host_step(host, dut, h, carry)
        want = R.step(ref, h, rc)
        _compare(dut, ref, st, want, carry, rc, f"step {k}")
        assert want["skipped"] == 0 and want["step"] == 4 + k
        assert (float(want["clip_coef"]) < 1.0) == (max_norm == 0.5 and k == 0) or max_norm == 0.5
        for t in dut:
            assert (not zg) or not t.g.any()
        sh = dut[8].shadow.reshape(32, 448)
        assert (sh[:, 447] == 0x7B7B).all(), "the padding column of the pitch-448 shadow is not written"
        assert R.same_bits(sh[:, :447].ravel(), R.bf16_bits(dut[8].p))


@pytest.mark.parametrize("algo", [R.ADAM, R.RMSPROP_TF])
def test_the_twins_second_level_fold(host, algo):
    assert sum(R.chunks_of(np.prod(s)) for s in FOLD_SHAPES) == 339
    h = R.Hyper(algo, beta1=0.9 if algo == R.ADAM else 0.99, weight_decay=0.01, max_norm=0.5, tau=0.005)
    dut, ref = R.host_set(R.random_set(21 + algo, FOLD_SHAPES, algo), algo, targeted=(5, 10))
    carry, rc = _carry_at(0, h)
    st = _host_step(host, dut, h, carry)
    want = R.step(ref, h, rc)
    _compare(dut, ref, st, want, carry, rc, "fold")
    assert float(want["clip_coef"]) < 1e-2 and want["step"] == 1
    # the same inputs again: the same bits
    dut2, _ = R.host_set(R.random_set(21 + algo, FOLD_SHAPES, algo), algo, targeted=(5, 10))
    carry2, _ = _carry_at(0, h)
    st2 = _host_step(host, dut2, h, carry2)
    assert st2.tobytes() == st.tobytes() and all(R.same_bits(a.p, b.p) for a, b in zip(dut, dut2))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("zg", [True, False])
def test_a_non_finite_gradient_skips_the_step(host, bad, zg):
    h = R.Hyper(R.ADAM, weight_decay=0.01, max_norm=0.5, tau=1.0, zero_grad=zg)
    data = R.random_set(31, R.BASE_SHAPES, R.ADAM)
    dut, ref = R.host_set(data, R.ADAM)
    before, _ = R.host_set(data, R.ADAM)
    for ts in (dut, ref):
        ts[7].g[1024] = bad
        ts[2].g[0] = bad
    carry, rc = _carry_at(5, h)
    st = _host_step(host, dut, h, carry)
    want = R.step(ref, h, rc)
    _compare(dut, ref, st, want, carry, rc, "skip")
    assert want["skipped"] == 1 and want["nonfinite"] == 2 and want["step"] == 5 and int(carry["step"][0]) == 5
    for a, b in zip(dut, before):
        assert R.same_bits(a.p, b.p) and R.same_bits(a.s1, b.s1) and R.same_bits(a.s2, b.s2)
        assert a.shadow is None or (a.shadow == 0x7B7B).all()
        assert a.target is None or R.same_bits(a.target, b.target)
        assert not a.g.any() if zg else True
    if not zg:
        assert not np.isfinite(dut[7].g[1024])
    # the following finite step is the first step of a run that never saw the bad gradient
    fresh, fresh_ref = R.host_set(data, R.ADAM)
    rng = np.random.default_rng(7)
    _new_grads(rng, dut, fresh_ref)
    for a, b in zip(fresh, fresh_ref):
        a.g[:] = b.g
    fc, frc = _carry_at(5, h)
    st_a, st_b = _host_step(host, dut, h, carry), _host_step(host, fresh, h, fc)
    assert st_a.tobytes() == st_b.tobytes() and int(st_a["step"]) == 6 and int(st_a["skipped"]) == 0
    want = R.step(fresh_ref, h, frc)
    _compare(dut, fresh_ref, st_a, want, carry, frc, "the step behind the skip")


def test_shadow_only_writes_the_shadows_and_nothing_else(host):
    data = R.random_set(41, R.BASE_SHAPES, R.ADAM)
    dut, ref = R.host_set(data, R.ADAM)
    carry, _ = _carry_at(2, R.Hyper())
    c0 = carry.copy()
    _host_step(host, dut, R.Hyper(), carry, flags=R.SHADOW_ONLY)
    R.refresh(ref)
    for a, b in zip(dut, ref):
        for name in ("p", "g", "s1", "s2", "target", "shadow"):
            x = getattr(a, name)
            assert x is None or R.same_bits(x, getattr(b, name)), name
    assert carry.tobytes() == c0.tobytes() and (dut[9].shadow != 0x7B7B).any()
    assert host.ws_host(0) == 0 and host.ws_host(1) == 48 and host.ws_host(313) == 32 + 16 * 313


# ---------------------------------------------------------------- (iii) bfloat16
def test_bfloat16_rounding_against_torch(host):
    import torch
    hi = np.arange(65536, dtype=np.uint32) << 16
    for lo in (0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF):
        x = (hi | np.uint32(lo)).view(np.float32)
        want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        got = np.zeros(65536, np.uint16)
        host.bf16_host(x.ctypes.data, got.ctypes.data, 65536)
        nan = np.isnan(x)
        for mine in (got, R.bf16_bits(x)):
            assert np.array_equal(mine[~nan], want[~nan]), hex(lo)
            assert ((mine[nan] & 0x7F80) == 0x7F80).all() and ((mine[nan] & 0x007F) != 0).all(), "a NaN stays a NaN"
        assert ((want[nan] & 0x7F80) == 0x7F80).all() and ((want[nan] & 0x007F) != 0).all()


# ---------------------------------------------------------------- (iv) declarations and wrappers
def test_header_declares_and_library_exports_optim():
    from balatro_gym_amd import _native as nat, build
    import balatro_gym_amd
    hdr = open(HEADER).read()
    m = re.search(r"\bint\s+bg_optim_step\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/balatro_mi355x.h does not declare bg_optim_step"
    params = [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", p).strip()) for p in m.group(1).split(",")]
    assert params == ["const void* table_dev", "int ntensors", "int64_t chunks", "int algo", "double lr", "double beta1", "double beta2", "double eps",
                      "double weight_decay", "double max_norm", "double tau", "uint32_t flags", "void* carry_dev", "void* workspace_dev", "void* stats_dev",
                      "float* kernel_ms_out", "void* stream"], params
    src = open(os.path.join(ROOT, "balatro_gym_amd", "_native.py")).read()
    bound = re.search(r"L\.bg_optim_step\.argtypes = \[(.*?)\]\n", src, re.S).group(1)
    assert len(re.sub(r"C\.POINTER\(C\.c_float\)", "fp", bound).split(",")) == len(params)
    assert re.search(r"uint64_t\s+bg_optim_workspace_size\s*\(\s*int64_t chunks\s*\)\s*;", hdr)
    for name, val in (("BG_OPTIM_ADAM", "0"), ("BG_OPTIM_RMSPROP_TF", "1"), ("BG_OPTIM_ZERO_GRAD", "1u"), ("BG_OPTIM_SHADOW_ONLY", "2u"),
                      ("BG_OPTIM_MAX_TENSORS", "1024"), ("BG_OPTIM_CHUNK", "1024"), ("BG_OPTIM_STATS_BYTES", "32")):
        assert re.search(rf"#define {name} {val}\b", hdr), name
    assert (nat.OPTIM_ADAM, nat.OPTIM_RMSPROP_TF, nat.OPTIM_ZERO_GRAD, nat.OPTIM_SHADOW_ONLY) == (R.ADAM, R.RMSPROP_TF, R.ZERO_GRAD, R.SHADOW_ONLY)
    assert (nat.OPTIM_MAX_TENSORS, nat.OPTIM_CHUNK, nat.OPTIM_ENTRY_BYTES, nat.OPTIM_STATS_BYTES, nat.OPTIM_CARRY_BYTES) == (1024, R.CHUNK, R.ENTRY.itemsize, R.STATS.itemsize, R.CARRY.itemsize)
    assert nat.OPTIM_STATS == tuple(n for n in R.STATS.names if n != "zero")
    for e in ("bg_optim_step", "bg_optim_workspace_size"):
        assert e in nat.EXPORTS
    assert os.path.join(CSRC, "bg_optim.h") in build.DEPS
    api = open(os.path.join(CSRC, "bg_rows_api.h")).read()
    assert '#include "bg_optim.h"' in api and api.index('#include "bg_optim.h"') > api.index('#include "bg_actor.h"'), "read behind every other header"
    assert '#include "bg_rows_api.h"' in open(os.path.join(CSRC, "bg_lib.hip")).read()
    body = api[api.index("int bg_optim_step("):]
    assert "bg_op_begin(\"bg_optim_step: \"" in body and "bg_op_run(" in body
    for name in ("RowOptimizer", "OptimStats"):
        assert name in balatro_gym_amd.__all__ and callable(getattr(balatro_gym_amd, name))
    if os.path.exists(build.LIB):
        L = C.CDLL(build.LIB)
        assert hasattr(L, "bg_optim_step")
        L.bg_optim_workspace_size.restype = C.c_uint64
        L.bg_optim_workspace_size.argtypes = [C.c_int64]
        assert L.bg_optim_workspace_size(0) == 0 and L.bg_optim_workspace_size(1) == 48 and L.bg_optim_workspace_size(313) == 32 + 16 * 313


def test_row_optimizer_refuses_bad_arguments_before_the_library():
    import torch
    from balatro_gym_amd import RowOptimizer
    ok = [torch.zeros(4, 3, requires_grad=True), torch.zeros(5, requires_grad=True)]
    for bad, match in ((torch.zeros(3, dtype=torch.float64), "float32"), (torch.zeros(3, dtype=torch.bfloat16), "float32"), (torch.zeros(4, 6)[:, ::2], "contiguous"),
                       ("w", "float32"), (torch.zeros(0), "non-empty")):
        with pytest.raises(ValueError, match=match):
            RowOptimizer(ok + [bad])
    with pytest.raises(ValueError, match="one GPU"):
        RowOptimizer(ok + [torch.zeros(3, device="meta")])
    with pytest.raises(ValueError, match="at most 1024"):
        RowOptimizer([torch.zeros(1) for _ in range(1025)])
    with pytest.raises(ValueError, match="empty"):
        RowOptimizer([])
    with pytest.raises(ValueError, match="twice"):
        RowOptimizer([ok[0], ok[0]])
    with pytest.raises(ValueError, match="algorithm"):
        RowOptimizer(ok, algorithm="adamw")
    for kw in (dict(lr=-1.0), dict(lr=float("nan")), dict(eps=-1e-8), dict(betas=(0.9, 1.0)), dict(betas=(0.9,)), dict(alpha=1.0), dict(weight_decay=-0.1),
               dict(max_grad_norm="x"), dict(lr=True)):
        with pytest.raises(ValueError):
            RowOptimizer(ok, **kw)
    opt = RowOptimizer(ok, max_grad_norm=None)
    assert opt.max_grad_norm == 0.0 and opt.state1[0].shape == (4, 3) and not opt.state1[0].any()
    assert bool(RowOptimizer(ok, algorithm="rmsprop_tf").state1[1].eq(1).all()) and RowOptimizer(ok, algorithm="rmsprop_tf").state2 == [None, None]
    for kw in (dict(lr=-1.0), dict(target_tau=1.5), dict(target_tau=float("nan")), dict(lr="x")):
        with pytest.raises(ValueError, match="lr must|target_tau must"):
            opt.step(**kw)
    ok[0].grad = torch.zeros(3, 4).t()   # torch itself refuses a gradient of another dtype or shape; a transposed one it takes
    with pytest.raises(ValueError, match=r"params\[0\].grad must be a contiguous"):
        opt.step()
    ok[0].grad = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="device tensors"):   # everything right: what is left is that there is no CPU path
        opt.step()
    opt.zero_grad()
    assert ok[0].grad is not None and ok[1].grad is None
    with pytest.raises(ValueError, match="pair up"):
        opt.set_target(ok, ok[:1])
    with pytest.raises(ValueError, match="not one of"):
        opt.set_target([torch.zeros(5)], [torch.zeros(5)])
    with pytest.raises(ValueError, match="shape"):
        opt.set_target([ok[1]], [torch.zeros(6)])
    with pytest.raises(ValueError, match="its own parameter"):
        opt.set_target([ok[1]], [ok[1]])
    opt.set_target([ok[1]], [torch.zeros(5)])
    with pytest.raises(ValueError, match="attach takes"):
        opt.attach(torch.nn.Linear(3, 4))
    # checkpoints
    sd = opt.state_dict()
    assert sd["step"] == 0 and sd["algorithm"] == "adam"
    sd["step"], sd["lr"] = 12, 1e-3
    sd["state1"][0].fill_(0.5)
    opt.load_state_dict(sd)
    c = opt._carry.numpy()
    rc = R.Carry.at(12, 0.9, 0.999)
    assert int(c.view(np.int64)[0]) == 12 and c[1] == rc.b1pow and c[2] == rc.b2pow and opt.lr == 1e-3 and bool(opt.state1[0].eq(0.5).all())
    with pytest.raises(ValueError, match="not one of"):
        RowOptimizer(ok, algorithm="rmsprop_tf").load_state_dict(sd)
    adam = opt.to_torch()
    assert isinstance(adam, torch.optim.Adam) and float(adam.state[ok[0]]["step"]) == 12.0 and bool(adam.state[ok[0]]["exp_avg"].eq(0.5).all())
    assert adam.param_groups[0]["eps"] == 1e-5 and adam.param_groups[0]["lr"] == 1e-3
    back = RowOptimizer.from_torch(adam, max_grad_norm=0.5)
    assert back.state_dict()["step"] == 12 and bool(back.state1[0].eq(0.5).all()) and back.betas == (0.9, 0.999)
    assert back._carry.numpy().tobytes() == c.tobytes()
    with pytest.raises(ValueError, match="one parameter group"):
        RowOptimizer.from_torch(torch.optim.SGD(ok, lr=0.1))
    with pytest.raises(ValueError, match="RMSpropTFLike"):
        RowOptimizer(ok, algorithm="rmsprop_tf").to_torch()


def test_attach_uses_the_shadow_only_while_the_version_holds():
    import torch
    from balatro_gym_amd import RowActor, RowExtractor, RowLinear, RowOptimizer
    from balatro_gym_amd.rows import _live_shadow
    for layer, pitch in ((RowLinear(32, "produced"), 153), (RowExtractor(32), 448), (RowActor(64), 64)):
        assert layer.weight_bf16 is None and _live_shadow(layer) is None, "the default: every existing path is unchanged"
        opt = RowOptimizer(layer.parameters())
        with pytest.raises(ValueError, match="not one of"):
            RowOptimizer([layer.bias]).attach(layer)
        opt.attach(layer)
        wb = layer.weight_bf16
        assert wb.dtype == torch.bfloat16 and tuple(wb.shape) == tuple(layer.weight.shape) and wb.stride(0) == pitch and wb.stride(1) == 1
        assert torch.equal(wb, layer.weight.detach().to(torch.bfloat16)) and _live_shadow(layer) is wb
        with torch.no_grad():
            layer.weight.copy_(layer.weight * 2)   # any torch in-place write bumps the version
        assert _live_shadow(layer) is None and layer.weight_bf16 is wb, "stale: the module casts again"
        layer._weight_bf16_version = layer.weight._version   # what refresh() records behind its launch
        assert _live_shadow(layer) is wb
        layer.load_state_dict(layer.state_dict())
        assert _live_shadow(layer) is None
        with pytest.raises(ValueError, match="device tensors"):
            opt.refresh()
        v = layer.weight._version
        layer.weight.data.mul_(1.0)
        assert layer.weight._version == v, "a write through .data does not bump the version: refresh() is the documented remedy"
