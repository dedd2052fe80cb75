"""bg_linear_rows / bg_linear_rows_grad on the MI355X: the network's first layer and its weight gradient straight from packed records, against the float64
statement of tests/linear_ref.py.  The layer's input is the bfloat16 row of bg_encode_rows_ex, taken from the numpy restatements the encode tests hold to
the kernel bit for bit.  Integer data must come out bit for bit (every float32 sum is exact in any order, so only a wrong element, a swapped index or a
missed row can differ); real data is held to the derived bound, and a bfloat16 output to the round-to-nearest-even of the float32 output of the same call.

Largest observed shares of the bounds on the MI355X are printed by every bounded test (`check_close`)."""
import ctypes as C

import numpy as np
import pytest

from tests import encode_ref as ref, linear_ref as lin, norm_ref
from tests.first_layer_helpers import _bf16, _bits, _dev, _f32_bits, _int_indices, _same

pytestmark = pytest.mark.gpu

K = lin.K
STRIDE = 384
SENTINEL = -12288.0   # exact in bfloat16


@pytest.fixture(scope="module")
def ints():
    """300 small-integer records on the device, their float32 bit patterns [300, 153], the integer weight [1024, 628] and an integer bias [1024]."""
    obs = lin.small_int_obs(300, 31)
    rng = np.random.default_rng(32)
    return {"rows": _dev(ref.pack_records(obs, STRIDE)), "bits": ref.expected_bits("produced", obs), "w": lin.int_weight(1024, 628),
            "b": rng.integers(-9, 10, 1024).astype(np.float32)}


def _forward_exact(ints, m, H, index, relu, cols=K):
    """Both output dtypes of one integer call, bit for bit -> the float64 reference."""
    import torch
    from balatro_gym_amd import linear_rows
    xb = lin.x_bits(ints["bits"][:m] if index is None else ints["bits"], index)
    want, _ = lin.forward(xb, ints["w"][:H], ints["b"][:H], relu)
    assert np.abs(want).max() < 2 ** 24 and (np.abs(lin.widen(xb)) @ np.abs(lin.widen(ints["w"][:H, :K])).T).max() < 2 ** 22
    rows = ints["rows"][:m] if index is None else ints["rows"]
    idx = None if index is None else _dev(np.asarray(index, np.int32))
    w = _bf16(ints["w"][:H, :cols])
    got32 = linear_rows(rows, w, _dev(ints["b"][:H]), index=idx, activation="relu" if relu else None, dtype=torch.float32)
    got16 = linear_rows(rows, w, _dev(ints["b"][:H]), index=idx, activation="relu" if relu else None, dtype=torch.bfloat16)
    assert got32.shape == got16.shape == (m, H)
    _same(_bits(got32), _f32_bits(want), f"float32 out, m={m} H={H}")
    _same(_bits(got16), lin.to_bf16_bits(want), f"bfloat16 out, m={m} H={H}")
    return want


@pytest.mark.parametrize("which", ["none", "shuffled", "repeated"])
def test_exact_integers_forward(ints, which):
    """m = 200 (no multiple of any tile), H = 64, asymmetric integer weight, integer bias: the integer reference bit for bit, in both output dtypes, with
    and without ReLU; without an index, through a shuffled one and through one with repeats."""
    index = _int_indices(200, 300)[which]
    want = _forward_exact(ints, 200, 64, index, False)
    assert (want < 0).any() and (want > 0).any()
    _forward_exact(ints, 200, 64, index, True)


def test_identity_weight():
    """H = 160, w[n, k] = [n == k], no bias: columns 0..152 are the widened bfloat16 row of bg_encode_rows_ex bit for bit (checked against the kernel's own
    output too), columns 153..159 are +0.0; an out-of-range index gives a row of act(b).  Records: the type extremes of encode_ref.synthetic_obs, the
    rows whose bfloat16 image is finite."""
    import torch
    from balatro_gym_amd import encode_rows, linear_rows
    obs = ref.synthetic_obs(n_random=230)
    bits = ref.expected_bits("produced", obs)
    xb_all = ref.bf16_bits(bits)
    finite = np.flatnonzero(((xb_all & 0x7f80) != 0x7f80).all(axis=1))
    assert len(finite) > 150 and (xb_all[finite] == 0x8000).any()   # (a -0.0 input comes out as +0.0 + ... = +0.0 only if other terms are +0.0: see below)
    rows = _dev(ref.pack_records(obs, STRIDE))
    index = finite.copy()
    index[[0, 37, len(index) - 1]] = (-1, len(bits), 2 ** 31 - 1)
    idx = _dev(index.astype(np.int32))
    eye = np.zeros((160, K), np.float32)
    eye[np.arange(K), np.arange(K)] = 1.0
    w = _bf16(lin.to_bf16_bits(eye))
    got = linear_rows(rows, w, None, index=idx, dtype=torch.float32)
    xb = lin.x_bits(bits, index)
    want = np.zeros((len(index), 160), np.float64)
    want[:, :K] = lin.widen(xb)
    # a sum of one value and 159 signed zeros: the value itself; a -0.0 value alone among +0.0 products sums to +0.0
    want_bits = _f32_bits(want + 0.0)
    want_bits[want_bits == 0x80000000] = 0
    _same(_bits(got), want_bits, "identity weight")
    enc = encode_rows(rows, "fixed", torch.bfloat16, index=idx)[:, :K]
    kernel_x = (_bits(enc).astype(np.uint32) << 16)
    kernel_x[kernel_x == 0x80000000] = 0
    _same(_bits(got)[:, :K], kernel_x, "identity weight against bg_encode_rows_ex")
    assert not _bits(got)[[0, 37, len(index) - 1]].any()
    bias = np.arange(160, dtype=np.float32) - 80.5
    got_b = linear_rows(rows, w, _dev(bias), index=idx, activation="relu", dtype=torch.float32)
    _same(_bits(got_b)[[0, 37, len(index) - 1]], np.tile(_f32_bits(np.maximum(bias, 0)), (3, 1)), "out-of-range rows are act(b)")


def test_statistics():
    """norm_ref.synthetic_rows(3, 70) under a RowNormalizer's frozen statistics, H = 128, random bfloat16 weights, ReLU: within the bound, the bfloat16
    output the rounding of the float32 one, two calls bit-identical."""
    import torch
    from balatro_gym_amd import RowNormalizer, linear_rows
    st = norm_ref.vecnormalize(norm_ref.synthetic_rows(5, 70, STRIDE, 98), norm_ref.new_state(70))["state"]
    host = norm_ref.synthetic_rows(3, 70, STRIDE, 99)
    nm = RowNormalizer(70, "cuda", training=False)
    nm.obs_mean.copy_(torch.from_numpy(st["obs_mean"]))
    nm.obs_var.copy_(torch.from_numpy(st["obs_var"]))
    xbits = norm_ref.obs_bits(norm_ref.from_moments(host, None, st, training=False, **norm_ref.DEFAULTS)["obs"]).reshape(-1, K)
    rng = np.random.default_rng(5)
    wb = lin.to_bf16_bits(rng.standard_normal((128, 628)).astype(np.float32) * 0.1)
    bias = rng.standard_normal(128).astype(np.float32)
    index = rng.permutation(210)[:150]
    rows = _dev(host)
    for idx in (None, index):
        want, bound = lin.forward(lin.x_bits(xbits, idx), wb, bias, relu=True)
        args = dict(index=None if idx is None else _dev(idx.astype(np.int32)), norm=nm, activation="relu")
        got = linear_rows(rows, _bf16(wb), _dev(bias), dtype=torch.float32, **args)
        lin.check_close(got.cpu().numpy(), want, bound, f"statistics, {'index' if idx is not None else 'dense'}")
        assert (want == 0).any() and (want > 0).any()
        again = linear_rows(rows, _bf16(wb), _dev(bias), dtype=torch.float32, **args)
        _same(_bits(again), _bits(got), "two calls")
        got16 = linear_rows(rows, _bf16(wb), _dev(bias), dtype=torch.bfloat16, **args)
        _same(_bits(got16), lin.to_bf16_bits(got.cpu().numpy()), "bfloat16 out = the rounding of the float32 out")


def test_weight_stride_and_untouched_memory(ints):
    """A [H, 628] weight gives the bits of its [:, :153] copy, "produced" the bits of "fixed"; output columns at or beyond H and rows at or beyond m keep
    a sentinel (the out tensor is a window of a larger poisoned one)."""
    import torch
    from balatro_gym_amd import linear_rows
    m, H = 77, 96
    rows = ints["rows"][:m]
    rng = np.random.default_rng(8)
    wb = lin.to_bf16_bits(rng.standard_normal((H, 628)).astype(np.float32))
    bias = _dev(ints["b"][:H])
    for dt in (torch.float32, torch.bfloat16):
        base = linear_rows(rows, _bf16(wb), bias, dtype=dt)
        _same(_bits(linear_rows(rows, _bf16(wb[:, :K].copy()), bias, dtype=dt)), _bits(base), "[H, 153] copy of the weight")
        _same(_bits(linear_rows(rows, _bf16(wb), bias, dtype=dt, layout="produced")), _bits(base), "produced = fixed")
        big = torch.full((m + 40, H + 9), SENTINEL, dtype=dt, device="cuda")
        res = linear_rows(rows, _bf16(wb), bias, dtype=dt, out=big[:m])
        assert res.shape == (m, H) and res.data_ptr() == big.data_ptr()
        _same(_bits(big[:m, :H]), _bits(base), "strided out")
        assert bool((big[:m, H:] == SENTINEL).all()) and bool((big[m:] == SENTINEL).all()), "memory beyond H columns / m rows was written"


@pytest.mark.parametrize("H", [32, 1024])
def test_width_limits(ints, H):
    """The narrowest and a wide layer at m = 64 by the integer data (H = 1024 through the 628-wide weight)."""
    _forward_exact(ints, 64, H, None, False, cols=628)


def test_refusals_write_nothing(ints):
    """H = 48, 0, 4128 and the extractor layout: BG_E_ARG with the call's name, nothing written."""
    import torch
    from balatro_gym_amd import _native as nat
    L = nat.load()
    m = 64
    rows = ints["rows"][:m]
    w = _bf16(lin.int_weight(4128, 160))
    out = torch.full((m, 4200), SENTINEL, dtype=torch.float32, device="cuda")
    def call(H, layout):
        return L.bg_linear_rows(C.c_void_p(rows.data_ptr()), C.c_uint64(STRIDE), C.c_int64(m), None, C.c_int64(m), layout, None, None, C.c_double(0), C.c_double(0),
                                C.c_void_p(w.data_ptr()), C.c_uint64(160), None, H, nat.LIN_NONE, nat.ENC_F32, C.c_void_p(out.data_ptr()), C.c_uint64(4200), None, None)
    for H, layout in ((48, nat.ENC_FIXED), (0, nat.ENC_FIXED), (4128, nat.ENC_FIXED), (64, nat.ENC_EXTRACTOR)):
        assert call(H, layout) == -1
        assert L.bg_last_error(None).decode().startswith("bg_linear_rows: ")
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call(64, nat.ENC_FIXED) == 0
    torch.cuda.synchronize()
    assert bool((out[:, :64] != SENTINEL).all()) and bool((out[:, 64:] == SENTINEL).all())


def test_exact_integers_gradient(ints):
    """m = 300, H = 64, integer dout in -4..4 (float32 and bfloat16): dweight and dbias are bit for bit the integer sums; under ReLU the forward's output
    masks exactly the non-positive units; out-of-range index rows add nothing to dweight and their dout to dbias; dweight columns at or beyond 153 keep
    a sentinel."""
    import torch
    from balatro_gym_amd import linear_rows, linear_rows_grad
    m, H = 300, 64
    rng = np.random.default_rng(77)
    dout = rng.integers(-4, 5, (m, H)).astype(np.float32)
    index = rng.permutation(300)
    index[[3, 150, 299]] = (-1, 300, 2 ** 31 - 1)
    for idx in (None, index):
        xb = lin.x_bits(ints["bits"], idx)
        args = dict(index=None if idx is None else _dev(idx.astype(np.int32)))
        for relu in (False, True):
            out = None
            if relu:
                out = linear_rows(ints["rows"], _bf16(ints["w"][:H]), _dev(ints["b"][:H]), activation="relu", dtype=torch.float32, **args)
                _same(_bits(out), _f32_bits(lin.forward(xb, ints["w"][:H], ints["b"][:H], True)[0]), "the forward of the masked gradient")
            dp = lin.dp_values(dout, None if out is None else out.cpu().numpy())
            assert not relu or ((dp == 0) & (dout != 0)).any()
            dw, _, db, _ = lin.grad(xb, dp, 0)
            assert np.abs(dw).max() < 2 ** 24
            for d in (_dev(dout), _dev(dout).to(torch.bfloat16)):
                dweight = torch.full((H, 628), SENTINEL, dtype=torch.float32, device="cuda")
                gw, gb = linear_rows_grad(ints["rows"], d, out=out, activation="relu" if relu else None, dweight=dweight, **args)
                assert gw.data_ptr() == dweight.data_ptr()
                _same(_bits(gw[:, :K]), _f32_bits(dw), f"dweight relu={relu} {d.dtype}")
                _same(_bits(gb), _f32_bits(db), f"dbias relu={relu} {d.dtype}")
                assert bool((gw[:, K:] == SENTINEL).all()), "dweight columns at or beyond 153 were written"
        if idx is not None:   # the out-of-range rows: no input, but their dout is in `dp` and so in dbias
            assert (lin.widen(xb[[3, 150, 299]]) == 0).all() and (dout[[3, 150, 299]] != 0).any()


def test_more_than_one_reduction_level():
    """m = 20 000 random finite records through an index, H = 64: 157 partials reduced by the second launch; within the bound, two calls bit-identical;
    the workspace is exactly bg_linear_rows_workspace_bytes and one byte less is a BG_E_ARG."""
    import torch
    from balatro_gym_amd import _native as nat, linear_rows, linear_rows_grad
    m, H, store = 20000, 64, 5000
    obs = lin.finite_obs(store, 11)
    bits = ref.expected_bits("produced", obs)
    rows = _dev(ref.pack_records(obs, STRIDE))
    rng = np.random.default_rng(12)
    index = rng.integers(0, store, m)
    idx = _dev(index.astype(np.int32))
    wb = lin.to_bf16_bits(rng.standard_normal((H, K)).astype(np.float32) * 2.0 ** -10)
    bias = rng.standard_normal(H).astype(np.float32)
    xb = lin.x_bits(bits, index)
    want, bound = lin.forward(xb, wb, bias, relu=True)
    out = linear_rows(rows, _bf16(wb), _dev(bias), index=idx, activation="relu", dtype=torch.float32)
    lin.check_close(out.cpu().numpy(), want, bound, "forward m=20000")
    dout = rng.standard_normal((m, H)).astype(np.float32)
    L = nat.load()
    need = int(L.bg_linear_rows_workspace_bytes(C.c_int64(m), H))
    assert need == lin.workspace_bytes(m, H) == 157 * 161 * H * 4 and lin.groups(m, H) == 157
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    gw, gb = linear_rows_grad(rows, _dev(dout), out=out, index=idx, activation="relu", workspace=ws)
    dp = lin.dp_values(dout, out.cpu().numpy())
    dw, dwb, db, dbb = lin.grad(xb, dp, lin.grad_rows_per_group(m, H))
    assert gw.shape == (H, 628) and not bool(gw[:, K:].any())
    lin.check_close(gw[:, :K].cpu().numpy(), dw, dwb, "dweight m=20000")
    lin.check_close(gb.cpu().numpy(), db, dbb, "dbias m=20000")
    gw2, gb2 = linear_rows_grad(rows, _dev(dout), out=out, index=idx, activation="relu")
    _same(_bits(gw2), _bits(gw), "dweight, two calls")
    _same(_bits(gb2), _bits(gb), "dbias, two calls")
    keep = gw.clone()
    d = _dev(dout)
    rc = L.bg_linear_rows_grad(C.c_void_p(rows.data_ptr()), C.c_uint64(STRIDE), C.c_int64(store), C.c_void_p(idx.data_ptr()), C.c_int64(m), nat.ENC_FIXED, None, None,
                               C.c_double(0), C.c_double(0), C.c_void_p(d.data_ptr()), nat.ENC_F32, C.c_uint64(H), C.c_void_p(out.data_ptr()), nat.ENC_F32, C.c_uint64(H), H,
                               nat.LIN_RELU, C.c_void_p(gw.data_ptr()), C.c_uint64(628), C.c_void_p(gb.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_uint64(need - 1), None, None)
    assert rc == -1 and L.bg_last_error(None).decode().startswith("bg_linear_rows_grad: ")
    torch.cuda.synchronize()
    _same(_bits(gw), _bits(keep), "a refused call wrote dweight")
    # a longer call: more than one block per group (the cap of 256 partials)
    assert lin.groups(40000, H) == 157 and lin.grad_rows_per_group(40000, H) == 256 and lin.groups(2 ** 20, 512) == 128


def test_past_4_gib():
    """A store of 2**32 / 384 + 4096 records (torch.empty: never initialised, never read but for the 64 records written at its end, which the index
    names): forward and gradient equal the same 64 records in a small store, bit for bit."""
    import torch
    from balatro_gym_amd import linear_rows, linear_rows_grad
    R = 2 ** 32 // STRIDE + 4096
    assert (R - 64) * STRIDE > 2 ** 32
    try:
        torch.cuda.empty_cache()
        store = torch.empty((R, STRIDE), dtype=torch.uint8, device="cuda")
    except (RuntimeError, torch.cuda.OutOfMemoryError):
        pytest.skip("no room for a 4.3 GB store")
    obs = lin.finite_obs(64, 21)
    small = _dev(ref.pack_records(obs, STRIDE))
    store[R - 64:] = small
    rng = np.random.default_rng(22)
    order = rng.permutation(64)
    H = 64
    wb = _bf16(lin.to_bf16_bits(rng.standard_normal((H, K)).astype(np.float32) * 2.0 ** -10))
    bias = _dev(rng.standard_normal(H).astype(np.float32))
    dout = _dev(rng.standard_normal((64, H)).astype(np.float32))
    far, near = _dev((R - 64 + order).astype(np.int32)), _dev(order.astype(np.int32))
    a = linear_rows(store, wb, bias, index=far, dtype=torch.float32)
    b = linear_rows(small, wb, bias, index=near, dtype=torch.float32)
    assert bool(torch.isfinite(b).all()) and bool((b != 0).any())
    _same(_bits(a), _bits(b), "forward past 4 GiB")
    ga, gab = linear_rows_grad(store, dout, index=far)
    gb, gbb = linear_rows_grad(small, dout, index=near)
    assert bool((gb != 0).any())
    _same(_bits(ga), _bits(gb), "dweight past 4 GiB")
    _same(_bits(gab), _bits(gbb), "dbias past 4 GiB")
    del store
    torch.cuda.empty_cache()


def test_autograd():
    """RowLinear(64, "fixed", activation="relu") followed by a float32 Linear(64, 61) on m = 512 records through an index: loss.backward() fills
    weight.grad and bias.grad within the bound of the float64 statement (columns at or beyond 153 exactly zero), and the second layer's gradients equal
    those of the torch composite fed the same first-layer output."""
    import torch
    from balatro_gym_amd import RowBuffers, RowLinear
    torch.manual_seed(3)
    store, m = 700, 512
    obs = lin.finite_obs(store, 41)
    bits = ref.expected_bits("produced", obs)
    rb = RowBuffers(store, torch.device("cuda", torch.cuda.current_device()), steps=1, row_stride=STRIDE)
    rb.rows[0].copy_(_dev(ref.pack_records(obs, STRIDE)))
    index = np.random.default_rng(42).permutation(store)[:m]
    idx = _dev(index.astype(np.int32))
    layer = RowLinear(64, "fixed", activation="relu").cuda()
    with torch.no_grad():
        layer.weight.mul_(2.0 ** -8)   # records hold values up to 2**15
    head = torch.nn.Linear(64, 61).cuda()
    target = torch.randn(m, 61, device="cuda")
    h = rb.linear(layer, idx)
    assert h.dtype == torch.bfloat16 and h.shape == (m, 64) and h.requires_grad
    loss = ((head(h.float()) - target) ** 2).mean()
    loss.backward()
    # the torch composite behind the first layer, fed the same output
    h2 = h.detach().clone().requires_grad_(True)
    head2 = torch.nn.Linear(64, 61).cuda()
    head2.load_state_dict(head.state_dict())
    ((head2(h2.float()) - target) ** 2).mean().backward()
    assert torch.equal(head.weight.grad, head2.weight.grad) and torch.equal(head.bias.grad, head2.bias.grad)
    xb = lin.x_bits(bits, index)
    wbits = lin.to_bf16_bits(layer.weight.detach().cpu().numpy())
    want, bound = lin.forward(xb, wbits, layer.bias.detach().cpu().numpy(), relu=True)
    from balatro_gym_amd import linear_rows
    h32 = linear_rows(rb.rows, layer.weight.detach().to(torch.bfloat16), layer.bias.detach(), index=idx, activation="relu", dtype=torch.float32)
    lin.check_close(h32.cpu().numpy(), want, bound, "RowLinear forward as float32")
    _same(_bits(h.detach()), lin.to_bf16_bits(h32.cpu().numpy()), "RowLinear forward = the rounding of the float32 output")
    hf = h.detach().float().cpu().numpy()
    dp = lin.dp_values(_bits(h2.grad), hf)
    dw, dwb, db, dbb = lin.grad(xb, dp, lin.grad_rows_per_group(m, 64))
    assert layer.weight.grad.shape == (64, 628) and not bool(layer.weight.grad[:, K:].any())
    lin.check_close(layer.weight.grad[:, :K].cpu().numpy(), dw, dwb, "weight.grad")
    lin.check_close(layer.bias.grad.cpu().numpy(), db, dbb, "bias.grad")
    assert bool((layer.weight.grad[:, :K] != 0).any())
