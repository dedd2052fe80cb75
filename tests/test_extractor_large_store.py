"""bg_extractor_rows / bg_extractor_rows_grad over the store of tests/test_large_store.py, which reaches past 2**31 and past 2**32 bytes: one
identity-weight forward and one gradient through `_gather_index`'s 131 indices -- the planted records around byte 2**31, around 2**32 and the last ones,
plus three indices out of range.  Every `(size_t)record * stride` of the two kernels (the hand bytes' own 16-byte read and the staged records) runs
here on such offsets; a truncated offset reads a zero record (or another planted one) and fails.  The forward is bit for bit the host copy's rows, the
gradient within tests/extractor_ref.py's bound; the planted records are unchanged afterwards.

The planted records are encode_ref's type extremes: `progress_ratio` holds random float32 bits, so column 428 of some rows is not finite.  Such a row
is all NaN behind an identity weight but for its own non-finite column (0 x inf); the forward holds the finite rows bit for bit and the others to that
pattern.  The gradient zeroes dout on those rows and leaves column 428 of dweight out (0 x inf again): the only column that can be affected."""
import numpy as np
import pytest

from tests import encode_ref, extractor_ref as ext
from tests.test_large_store import R, STRIDE, _gather_index, _unchanged, big  # noqa: F401

pytestmark = pytest.mark.gpu

K = ext.K
RATIO_COLUMN = 416 + 10 + 2   # progress_ratio: the float32 field, copied bit for bit


def _inputs(big):
    import torch
    idx, src = _gather_index(17)
    ok = src >= 0
    assert len(idx) == 131 and (~ok).sum() == 3 and (idx[ok] * STRIDE > 2 ** 32).sum() > 40 and (idx[ok] * STRIDE > 2 ** 31).sum() > 70
    rows_host = big["host"][np.where(ok, src, 0)]
    bits = encode_ref.expected_bits("extractor", encode_ref.unpack_records(rows_host))
    xb = np.where(ok[:, None], encode_ref.bf16_bits(bits), np.uint16(0))
    finite_el = (xb & 0x7f80) != 0x7f80
    assert finite_el[:, np.arange(K) != RATIO_COLUMN].all(), "only progress_ratio can be non-finite"
    return torch.from_numpy(idx.astype(np.int32)).cuda(), xb, finite_el.all(axis=1)


def _bf16(bits):
    import torch
    return torch.from_numpy(np.asarray(bits, np.uint16).view(np.int16)).cuda().view(torch.bfloat16)


def test_identity_forward_across_the_boundaries(big):
    import torch
    from balatro_gym_amd import extractor_rows
    index, xb, finite = _inputs(big)
    assert finite.sum() > 100
    eye = np.zeros((448, K), np.float32)
    eye[np.arange(K), np.arange(K)] = 1.0
    got = extractor_rows(big["store"], _bf16(ext.to_bf16_bits(eye)), None, index=index, dtype=torch.float32)
    torch.cuda.synchronize()
    got = got.view(torch.int32).cpu().numpy().view(np.uint32)
    want = np.zeros((len(xb), 448), np.uint32)
    want[:, :K] = xb.astype(np.uint32) << 16
    want[want == 0x80000000] = 0   # a -0.0 value alone among +0.0 products sums to +0.0
    bad = np.argwhere(got[finite] != want[finite])
    assert bad.size == 0, f"{len(bad)} elements differ, first (finite row, column) {tuple(bad[0])}"
    assert (want[finite][:, :416] == 0x3f800000).any() and (want[finite][:, 416:K] != 0).any()
    if (~finite).any():
        assert np.isnan(got[~finite].view(np.float32)).mean() > 0.9   # NaN but for the column itself
    _unchanged(big)


def test_gradient_across_the_boundaries(big):
    import torch
    from balatro_gym_amd import extractor_rows_grad
    index, xb, finite = _inputs(big)
    m, H = len(xb), 64
    rng = np.random.default_rng(18)
    dout = rng.standard_normal((m, H)).astype(np.float32)
    dout[~finite] = 0.0
    gw, gb = extractor_rows_grad(big["store"], torch.from_numpy(dout).cuda(), index=index)
    torch.cuda.synchronize()
    keep = np.arange(K) != RATIO_COLUMN
    xk = np.where(((xb & 0x7f80) != 0x7f80), xb, np.uint16(0))   # (only column 428 differs, and it is left out)
    dp = ext.dp_values(dout)
    dw, dwb, db, dbb = ext.grad(xk, dp, ext.grad_rows_per_group(m, H))
    ext.check_close(gw.cpu().numpy()[:, keep], dw[:, keep], dwb[:, keep], "dweight across the boundaries")
    ext.check_close(gb.cpu().numpy(), db, dbb, "dbias across the boundaries")
    assert (dw[:, :416] != 0).any() and (dw[:, 416:][:, keep[416:]] != 0).any()
    _unchanged(big)
