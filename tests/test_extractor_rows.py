"""bg_extractor_rows / bg_extractor_rows_grad on the MI355X: the first layer behind BalatroFeaturesExtractor's 447-column input and its weight gradient
straight from packed records, against the float64 statement of tests/extractor_ref.py.  The layer's input is the bfloat16 row of bg_encode_rows_ex
("extractor"), taken from the numpy restatement the encode tests hold to the kernel bit for bit.  Integer-quotient data must come out bit for bit (every
float32 sum is exact in any order, so only a wrong element, a swapped index or a missed row can differ); real data is held to the derived bound, and a
bfloat16 output to the round-to-nearest-even of the float32 output of the same call.

Every bounded test prints its largest share of the bound (`check_close`)."""
import ctypes as C

import numpy as np
import pytest

from tests import encode_ref as ref, extractor_ref as ext, linear_ref as lin
from tests.first_layer_helpers import _bf16, _bits, _dev, _f32_bits, _int_indices, _same

pytestmark = pytest.mark.gpu

K = ext.K
STRIDE = 384
SENTINEL = -12288.0   # exact in bfloat16


def _redraw_hand(obs, seed):
    """finite_obs draws `hand` over the whole int8 range: almost never a card.  Redrawn in -1..51, so that the one-hot columns are exercised."""
    obs = dict(obs)
    obs["hand"] = np.random.default_rng(seed).integers(-1, 52, obs["hand"].shape).astype(np.int8)
    return obs


@pytest.fixture(scope="module")
def ints():
    """300 integer-quotient records on the device, their float32 bit patterns [300, 447], the integer weight [64, 447] and an integer bias [64]."""
    obs = ext.int_quotient_obs(300, 31)
    bits = ref.expected_bits("extractor", obs)
    xb = ext.x_bits(bits)
    hot1 = np.flatnonzero(xb[1, :416])
    assert hot1.tolist() == [51, 103, 104, 156] and not xb[0, :416].any() and (xb[:, :416] != 0).sum() > 6 * 300
    rng = np.random.default_rng(32)
    return {"rows": _dev(ref.pack_records(obs, STRIDE)), "bits": bits, "w": lin.int_weight(64, K), "b": rng.integers(-9, 10, 64).astype(np.float32)}


def _forward_exact(ints, m, H, index, relu):
    """Both output dtypes of one integer call, bit for bit -> the float64 reference."""
    import torch
    from balatro_gym_amd import extractor_rows
    xb = ext.x_bits(ints["bits"][:m] if index is None else ints["bits"], index)
    ext.assert_exact_inputs(xb, ints["w"][:H], ints["b"][:H])
    want, _ = ext.forward(xb, ints["w"][:H], ints["b"][:H], relu)
    rows = ints["rows"][:m] if index is None else ints["rows"]
    idx = None if index is None else _dev(np.asarray(index, np.int32))
    w = _bf16(ints["w"][:H])
    got32 = extractor_rows(rows, w, _dev(ints["b"][:H]), index=idx, activation="relu" if relu else None, dtype=torch.float32)
    got16 = extractor_rows(rows, w, _dev(ints["b"][:H]), index=idx, activation="relu" if relu else None, dtype=torch.bfloat16)
    assert got32.shape == got16.shape == (m, H)
    _same(_bits(got32), _f32_bits(want), f"float32 out, m={m} H={H}")
    _same(_bits(got16), ext.to_bf16_bits(want), f"bfloat16 out, m={m} H={H}")
    return want


@pytest.mark.parametrize("which", ["none", "shuffled", "repeated"])
def test_exact_forward(ints, which):
    """m = 200 (no multiple of any tile) of a store of 300, H = 64, asymmetric integer weight, integer bias: the reference bit for bit, in both output
    dtypes, with and without ReLU; without an index, through a shuffled one and through one with repeats."""
    index = _int_indices(200, 300)[which]
    want = _forward_exact(ints, 200, 64, index, False)
    assert (want < 0).any() and (want > 0).any()
    _forward_exact(ints, 200, 64, index, True)


def test_identity_weight():
    """H = 448, w[n, k] = [n == k], no bias: columns 0..446 are the widened bfloat16 row of bg_encode_rows_ex bit for bit (-0.0 read as +0.0), against the
    numpy restatement and against the kernel's own output; column 447 is +0.0; indices -1, len and 2**31 - 1 give act(b).  Records: the type extremes of
    encode_ref.synthetic_obs, the rows whose bfloat16 image is finite."""
    import torch
    from balatro_gym_amd import encode_rows, extractor_rows
    obs = ref.synthetic_obs(n_random=230)
    bits = ref.expected_bits("extractor", obs)
    xb_all = ref.bf16_bits(bits)
    finite = np.flatnonzero(((xb_all & 0x7f80) != 0x7f80).all(axis=1))
    assert len(finite) > 150 and (xb_all[finite][:, :416] == 0x3f80).any()
    rows = _dev(ref.pack_records(obs, STRIDE))
    index = finite.copy()
    index[[0, 37, len(index) - 1]] = (-1, len(bits), 2 ** 31 - 1)
    idx = _dev(index.astype(np.int32))
    eye = np.zeros((448, K), np.float32)
    eye[np.arange(K), np.arange(K)] = 1.0
    w = _bf16(ext.to_bf16_bits(eye))
    got = extractor_rows(rows, w, None, index=idx, dtype=torch.float32)
    xb = ext.x_bits(bits, index)
    want = np.zeros((len(index), 448), np.float64)
    want[:, :K] = ext.widen(xb)
    want_bits = _f32_bits(want + 0.0)
    want_bits[want_bits == 0x80000000] = 0   # a -0.0 value alone among +0.0 products sums to +0.0
    _same(_bits(got), want_bits, "identity weight")
    enc = encode_rows(rows, "extractor", torch.bfloat16, index=idx)
    kernel_x = (_bits(enc).astype(np.uint32) << 16)
    kernel_x[kernel_x == 0x80000000] = 0
    _same(_bits(got)[:, :K], kernel_x, "identity weight against bg_encode_rows_ex")
    assert not _bits(got)[:, K].any() and not _bits(got)[[0, 37, len(index) - 1]].any()
    bias = np.arange(448, dtype=np.float32) - 224.5
    got_b = extractor_rows(rows, w, _dev(bias), index=idx, activation="relu", dtype=torch.float32)
    _same(_bits(got_b)[[0, 37, len(index) - 1]], np.tile(_f32_bits(np.maximum(bias, 0)), (3, 1)), "out-of-range rows are act(b)")


def test_bounded_forward():
    """m = 333, H = 128, linear_ref.finite_obs with `hand` redrawn in -1..51, random bfloat16 weights, ReLU: within the bound, the bfloat16 output the
    rounding of the float32 one, two calls bit-identical, and a weight at a 2-byte-aligned odd offset with an odd pitch (and the 16-byte and 4-byte
    aligned stagings of the same values) gives the same bits."""
    import torch
    from balatro_gym_amd import extractor_rows
    m, H = 333, 128
    obs = _redraw_hand(lin.finite_obs(m, 51), 52)
    bits = ref.expected_bits("extractor", obs)
    xb = ext.x_bits(bits)
    assert ((xb & 0x7f80) != 0x7f80).all() and (xb[:, :416] == 0x3f80).sum() > 6 * m
    rows = _dev(ref.pack_records(obs, STRIDE))
    rng = np.random.default_rng(5)
    wbits = ext.to_bf16_bits(rng.standard_normal((H, K)).astype(np.float32) * 0.1)
    bias = rng.standard_normal(H).astype(np.float32)
    want, bound = ext.forward(xb, wbits, bias, relu=True)
    assert (want == 0).any() and (want > 0).any()
    got = extractor_rows(rows, _bf16(wbits), _dev(bias), activation="relu", dtype=torch.float32)
    ext.check_close(got.cpu().numpy(), want, bound, "bounded forward")
    again = extractor_rows(rows, _bf16(wbits), _dev(bias), activation="relu", dtype=torch.float32)
    _same(_bits(again), _bits(got), "two calls")
    got16 = extractor_rows(rows, _bf16(wbits), _dev(bias), activation="relu", dtype=torch.bfloat16)
    _same(_bits(got16), ext.to_bf16_bits(got.cpu().numpy()), "bfloat16 out = the rounding of the float32 out")
    for offset, pitch in ((1, 449), (2, 450), (8, 448), (0, 456)):   # by element; by word; by 16-byte piece (twice)
        flat = torch.zeros(offset + H * pitch + 8, dtype=torch.bfloat16, device="cuda")
        view = flat[offset:offset + H * pitch].view(H, pitch)[:, :K]
        view.copy_(_bf16(wbits))
        assert view.data_ptr() % 16 == (2 * offset) % 16 and view.stride(0) == pitch
        res = extractor_rows(rows, view, _dev(bias), activation="relu", dtype=torch.float32)
        _same(_bits(res), _bits(got), f"weight at element offset {offset}, pitch {pitch}")


def test_exact_gradient(ints):
    """m = 300, H = 64, integer dout in -4..4 (float32 and bfloat16): dweight and dbias are bit for bit the integer sums; under ReLU the forward's output
    masks exactly the non-positive units; the three out-of-range index rows add nothing to dweight and their dout to dbias; dweight has pitch 456 with a
    sentinel in columns 447..455 that survives."""
    import torch
    from balatro_gym_amd import extractor_rows, extractor_rows_grad
    m, H = 300, 64
    rng = np.random.default_rng(77)
    dout = rng.integers(-4, 5, (m, H)).astype(np.float32)
    index = rng.permutation(300)
    index[[3, 150, 299]] = (-1, 300, 2 ** 31 - 1)
    for idx in (None, index):
        xb = ext.x_bits(ints["bits"], idx)
        ext.assert_exact_inputs(xb, ints["w"], ints["b"])
        args = dict(index=None if idx is None else _dev(idx.astype(np.int32)))
        for relu in (False, True):
            out = None
            if relu:
                out = extractor_rows(ints["rows"], _bf16(ints["w"]), _dev(ints["b"]), activation="relu", dtype=torch.float32, **args)
                _same(_bits(out), _f32_bits(ext.forward(xb, ints["w"], ints["b"], True)[0]), "the forward of the masked gradient")
            dp = ext.dp_values(dout, None if out is None else out.cpu().numpy())
            assert not relu or ((dp == 0) & (dout != 0)).any()
            dw, _, db, _ = ext.grad(xb, dp, 0)
            assert (np.abs(dp).T @ np.abs(ext.widen(xb))).max() < 2 ** 21 and (dw * 8 == np.round(dw * 8)).all()
            for d in (_dev(dout), _dev(dout).to(torch.bfloat16)):
                dweight = torch.full((H, 456), SENTINEL, dtype=torch.float32, device="cuda")
                gw, gb = extractor_rows_grad(ints["rows"], d, out=out, activation="relu" if relu else None, dweight=dweight, **args)
                assert gw.data_ptr() == dweight.data_ptr()
                _same(_bits(gw[:, :K]), _f32_bits(dw), f"dweight relu={relu} {d.dtype}")
                _same(_bits(gb), _f32_bits(db), f"dbias relu={relu} {d.dtype}")
                assert bool((gw[:, K:] == SENTINEL).all()), "dweight columns at or beyond 447 were written"
        if idx is not None:   # the out-of-range rows: no input, but their dout is in `dp` and so in dbias
            assert (ext.widen(xb[[3, 150, 299]]) == 0).all() and (dout[[3, 150, 299]] != 0).any()


M_TWO_BLOCKS = ext.smallest_m_with_two_blocks_per_group(64)


@pytest.mark.parametrize("m,H", [(700, 288), (M_TWO_BLOCKS, 64)])
def test_bounded_gradient(m, H):
    """(700, 288): two unit spans, H no multiple of 64.  (10 881, 64): the smallest m at which the split gives a group more than one 128-row block at
    H = 64.  Random finite records through an index with repeats, ReLU: forward, dweight and dbias within the bound, two calls bit-identical."""
    import torch
    from balatro_gym_amd import _native as nat, extractor_rows, extractor_rows_grad
    assert M_TWO_BLOCKS == 10881 and ext.blocks_per_group(M_TWO_BLOCKS, 64) == 2 and ext.blocks_per_group(M_TWO_BLOCKS - 1, 64) == 1
    assert ext.spans(288) == 2 and 288 % 64
    store = 2000
    obs = _redraw_hand(lin.finite_obs(store, 11 + H), 12)
    bits = ref.expected_bits("extractor", obs)
    rows = _dev(ref.pack_records(obs, STRIDE))
    rng = np.random.default_rng(13 + H)
    index = rng.integers(0, store, m)
    idx = _dev(index.astype(np.int32))
    wbits = ext.to_bf16_bits(rng.standard_normal((H, K)).astype(np.float32) * 2.0 ** -10)
    bias = rng.standard_normal(H).astype(np.float32)
    xb = ext.x_bits(bits, index)
    want, bound = ext.forward(xb, wbits, bias, relu=True)
    out = extractor_rows(rows, _bf16(wbits), _dev(bias), index=idx, activation="relu", dtype=torch.float32)
    ext.check_close(out.cpu().numpy(), want, bound, f"forward m={m} H={H}")
    dout = rng.standard_normal((m, H)).astype(np.float32)
    need = int(nat.load().bg_extractor_rows_workspace_bytes(C.c_int64(m), H))
    assert need == ext.workspace_bytes(m, H) == ext.groups(m, H) * 449 * H * 4
    gw, gb = extractor_rows_grad(rows, _dev(dout), out=out, index=idx, activation="relu")
    dp = ext.dp_values(dout, out.cpu().numpy())
    dw, dwb, db, dbb = ext.grad(xb, dp, ext.grad_rows_per_group(m, H))
    assert gw.shape == (H, K) and (dp == 0).any() and (dw[:, :416] != 0).any()
    ext.check_close(gw.cpu().numpy(), dw, dwb, f"dweight m={m} H={H}")
    ext.check_close(gb.cpu().numpy(), db, dbb, f"dbias m={m} H={H}")
    gw2, gb2 = extractor_rows_grad(rows, _dev(dout), out=out, index=idx, activation="relu")
    _same(_bits(gw2), _bits(gw), "dweight, two calls")
    _same(_bits(gb2), _bits(gb), "dbias, two calls")


def test_refusals_write_nothing(ints):
    """Through the C ABI: H = 48, 0 and 4128, weight pitch 446, a misaligned output, a workspace that is too small: -1 with the call's name, nothing
    written."""
    import torch
    from balatro_gym_amd import _native as nat
    L = nat.load()
    m = 64
    rows = ints["rows"][:m]
    w = _bf16(lin.int_weight(4128, 448))
    out = torch.full((m, 4200), SENTINEL, dtype=torch.float32, device="cuda")

    def call(H, wpitch=448, out_ptr=None):
        return L.bg_extractor_rows(C.c_void_p(rows.data_ptr()), C.c_uint64(STRIDE), C.c_int64(m), None, C.c_int64(m), C.c_void_p(w.data_ptr()), C.c_uint64(wpitch), None,
                                   H, nat.LIN_NONE, nat.ENC_F32, C.c_void_p(out_ptr or out.data_ptr()), C.c_uint64(4200), None, None)
    for kw in (dict(H=48), dict(H=0), dict(H=4128), dict(H=64, wpitch=446), dict(H=64, out_ptr=out.data_ptr() + 2)):
        assert call(**kw) == -1, kw
        assert L.bg_last_error(None).decode().startswith("bg_extractor_rows: "), kw
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call(64) == 0
    torch.cuda.synchronize()
    assert bool((out[:, :64] != SENTINEL).all()) and bool((out[:, 64:] == SENTINEL).all())
    # the gradient: the same widths, a dweight pitch of 446 and a workspace one byte short
    H = 64
    need = int(L.bg_extractor_rows_workspace_bytes(C.c_int64(m), H))
    assert need == ext.workspace_bytes(m, H) > 0
    dout = torch.ones((m, 4200), dtype=torch.float32, device="cuda")
    dweight = torch.full((4128, 456), SENTINEL, dtype=torch.float32, device="cuda")
    dbias = torch.full((4128,), SENTINEL, dtype=torch.float32, device="cuda")
    ws = torch.full((need // 4,), SENTINEL, dtype=torch.float32, device="cuda")

    def grad(H=64, dwpitch=456, ws_bytes=need):
        return L.bg_extractor_rows_grad(C.c_void_p(rows.data_ptr()), C.c_uint64(STRIDE), C.c_int64(m), None, C.c_int64(m), C.c_void_p(dout.data_ptr()), nat.ENC_F32,
                                        C.c_uint64(4200), None, 0, C.c_uint64(0), H, nat.LIN_NONE, C.c_void_p(dweight.data_ptr()), C.c_uint64(dwpitch),
                                        C.c_void_p(dbias.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_uint64(ws_bytes), None, None)
    for kw in (dict(H=48), dict(H=0), dict(H=4128), dict(dwpitch=446), dict(ws_bytes=need - 1)):
        assert grad(**kw) == -1, kw
        assert L.bg_last_error(None).decode().startswith("bg_extractor_rows_grad: "), kw
    torch.cuda.synchronize()
    assert bool((dweight == SENTINEL).all()) and bool((dbias == SENTINEL).all()) and bool((ws == SENTINEL).all())
    assert grad() == 0
    torch.cuda.synchronize()
    assert bool((dweight[:64, :K] != SENTINEL).all()) and bool((dweight[:64, K:] == SENTINEL).all()) and bool((dweight[64:] == SENTINEL).all())
    assert bool((dbias[:64] == float(m)).all()) and bool((dbias[64:] == SENTINEL).all())


def test_row_extractor_autograd():
    """RowExtractor(64) on m = 512 records through an index: h.float().square().sum().backward() fills weight.grad and bias.grad within the bound of the
    same layer through encode_rows + F.linear on the widened operands in float64.  The bfloat16 forward is held to the float32 bound plus one rounding
    to bfloat16 (8 significant bits: unit roundoff 2**-8)."""
    import torch
    import torch.nn.functional as F
    from balatro_gym_amd import RowExtractor, encode_rows
    torch.manual_seed(3)
    store, m, H = 700, 512, 64
    obs = _redraw_hand(lin.finite_obs(store, 41), 43)
    rows = _dev(ref.pack_records(obs, STRIDE))
    index = np.random.default_rng(42).permutation(store)[:m]
    idx = _dev(index.astype(np.int32))
    layer = RowExtractor(H).cuda()
    with torch.no_grad():
        layer.weight.mul_(2.0 ** -8)   # records hold values up to 2**15
    h = layer(rows, idx)
    assert h.dtype == torch.bfloat16 and h.shape == (m, H) and h.requires_grad
    h.float().square().sum().backward()
    # the composite: the kernel's own encoded rows (held to the restatement bit for bit elsewhere), widened, through F.linear in float64
    x = encode_rows(rows, "extractor", torch.bfloat16, index=idx).double()
    w64 = layer.weight.detach().to(torch.bfloat16).double().requires_grad_(True)
    b64 = layer.bias.detach().double().requires_grad_(True)
    ref_lin = F.linear(x, w64, b64)
    ref_out = F.relu(ref_lin).detach().cpu().numpy()
    xb = _bits(encode_rows(rows, "extractor", torch.bfloat16, index=idx))
    _same(xb, ext.x_bits(ref.expected_bits("extractor", obs), index), "the composite's input")
    wbits = ext.to_bf16_bits(layer.weight.detach().cpu().numpy())
    want, bound = ext.forward(xb, wbits, layer.bias.detach().cpu().numpy(), relu=True)
    assert np.abs(want - ref_out).max() <= 1e-10 * np.abs(want).max()   # two float64 summation orders
    # the forward: bfloat16 = one rounding of a float32 value within the bound
    hf = h.detach().float().cpu().numpy().astype(np.float64)
    ext.check_close(hf, want, bound + 2.0 ** -8 * np.abs(want), "RowExtractor forward (bfloat16)")
    # the backward of the composite with the layer's own dp: dout = 2 h (exact in bfloat16) where the kernel's output is > 0
    dout = (2.0 * h.detach().float())
    dp = ext.dp_values(dout.cpu().numpy(), hf)
    ref_lin.backward(torch.from_numpy(dp).cuda())   # dp carries ReLU's mask already: the one the layer's backward takes from its own output
    dw, dwb, db, dbb = ext.grad(xb, dp, ext.grad_rows_per_group(m, H))
    assert np.abs(dw - w64.grad.cpu().numpy()).max() <= 1e-10 * np.abs(dw).max() and np.abs(db - b64.grad.cpu().numpy()).max() <= 1e-10 * np.abs(db).max()
    assert layer.weight.grad.shape == (H, K) and layer.bias.grad.shape == (H,)
    ext.check_close(layer.weight.grad.cpu().numpy(), dw, dwb, "weight.grad")
    ext.check_close(layer.bias.grad.cpu().numpy(), db, dbb, "bias.grad")
    assert bool((layer.weight.grad[:, :416] != 0).any()) and bool((layer.weight.grad[:, 416:] != 0).any())


def test_from_linears_block_structure():
    """from_linears(Linear(416, 32), Linear(10, 16), Linear(21, 16)): off-block weight.grad is exactly zero, the three blocks' gradients match the three
    sub-layers computed separately (float64, on their own column ranges) within the bound, and after one SGD step the off-block weights are still +0.0."""
    import torch
    from balatro_gym_amd import RowBuffers, RowExtractor
    torch.manual_seed(6)
    store, m = 400, 300
    obs = _redraw_hand(lin.finite_obs(store, 61), 62)
    bits = ref.expected_bits("extractor", obs)
    rb = RowBuffers(store, torch.device("cuda", torch.cuda.current_device()), steps=1, row_stride=STRIDE)
    rb.rows[0].copy_(_dev(ref.pack_records(obs, STRIDE)))
    index = np.random.default_rng(63).permutation(store)[:m]
    idx = _dev(index.astype(np.int32))
    subs = (torch.nn.Linear(416, 32), torch.nn.Linear(10, 16), torch.nn.Linear(21, 16))
    with torch.no_grad():
        subs[1].weight.mul_(2.0 ** -12)
        subs[2].weight.mul_(2.0 ** -8)
    layer = RowExtractor.from_linears(*subs).cuda()
    assert layer.splits == (32, 16, 16) and layer.block_mask.is_cuda
    h = rb.extractor(layer, idx)
    parts = h.split(layer.splits, dim=1)
    assert [p.shape[1] for p in parts] == [32, 16, 16]
    h.float().square().sum().backward()
    mask = layer.block_mask.cpu().numpy() != 0
    g = layer.weight.grad.cpu().numpy()
    assert (g[~mask] == 0).all(), "off-block weight.grad is not exactly zero"
    xb = ext.x_bits(bits, index)
    hf = h.detach().float().cpu().numpy().astype(np.float64)
    dp = ext.dp_values((2.0 * h.detach().float()).cpu().numpy(), hf)
    r = c = 0
    for lin_k, cols in zip(subs, (416, 10, 21)):
        width = lin_k.out_features
        xs = ext.widen(xb[:, c:c + cols])
        dps = dp[:, r:r + width]
        dw, mag = dps.T @ xs, np.abs(dps).T @ np.abs(xs)
        f = 2 * (ext.grad_rows_per_group(m, 64) + 2) * ext.U
        ext.check_close(g[r:r + width, c:c + cols], dw, f * mag + ext.U * np.abs(dw), f"block ({r}, {c}) of weight.grad")
        # the sub-layer's forward on its own columns
        wsub = ext.widen(ext.to_bf16_bits(lin_k.weight.detach().numpy()))
        s = xs @ wsub.T + lin_k.bias.detach().numpy().astype(np.float64)
        smag = np.abs(xs) @ np.abs(wsub).T + np.abs(lin_k.bias.detach().numpy().astype(np.float64))
        sub_out = np.where(s > 0, s, 0.0)
        ext.check_close(hf[:, r:r + width], sub_out, 2 * (ext.KPAD + 2) * ext.U * smag + (ext.U + 2.0 ** -8) * np.abs(sub_out), f"sub-network {r} forward")
        assert (dw != 0).any()
        r, c = r + width, c + cols
    opt = torch.optim.SGD(layer.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-2)
    before = layer.weight.detach().clone()
    opt.step()
    after = _bits(layer.weight.detach())
    assert not after[~mask].any(), "an off-block weight left +0.0"
    assert bool((layer.weight.detach() != before).any())


def test_row_buffers_extractor_equals_extractor_rows():
    import torch
    from balatro_gym_amd import RowBuffers, RowExtractor, extractor_rows
    torch.manual_seed(8)
    n, steps = 37, 3
    obs = _redraw_hand(lin.finite_obs(n * steps, 71), 72)
    rb = RowBuffers(n, torch.device("cuda", torch.cuda.current_device()), steps=steps, row_stride=STRIDE)
    rb.rows.view(-1, STRIDE).copy_(_dev(ref.pack_records(obs, STRIDE)))
    layer = RowExtractor(96, activation=None, dtype=torch.float32).cuda()
    idx = _dev(np.random.default_rng(73).permutation(n * steps)[:50].astype(np.int32))
    with torch.no_grad():
        for index in (None, idx):
            a = rb.extractor(layer, index)
            b = extractor_rows(rb.rows, layer.weight.detach().to(torch.bfloat16), layer.bias.detach(), index=index, activation=None, dtype=torch.float32)
            assert a.shape == (n * steps if index is None else 50, 96) and a.dtype == torch.float32
            _same(_bits(a), _bits(b), "RowBuffers.extractor")
