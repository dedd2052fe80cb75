"""What the tests of the two first layers share (test_linear_rows*.py, test_extractor_rows*.py): device tensors and bit patterns, the index sets of
the integer cases, and, for the host tests, the scalar model of v_mfma_f32_32x32x16_bf16 as C text and the parser of the header's declarations."""
import re

import numpy as np


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bf16(bits):
    """bfloat16 bit patterns (uint16) -> a torch.bfloat16 device tensor."""
    import torch
    return _dev(np.asarray(bits, np.uint16).view(np.int16)).view(torch.bfloat16)


def _bits(t):
    import torch
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _f32_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} elements differ, first {tuple(bad[0])}: {got[tuple(bad[0])]:#x} != {want[tuple(bad[0])]:#x}"


def _int_indices(m, store):
    rng = np.random.default_rng(m)
    rep = rng.integers(0, store, m)
    rep[1::3] = rep[0]   # one record many times
    return {"none": None, "shuffled": rng.permutation(store)[:m], "repeated": rep}


# The model: lane l of 64 holds A[row l & 31][k = 8 (l >> 5) + j] and B[k = 8 (l >> 5) + j][column l & 31] in element j = 0..7 of its fragments;
# accumulator register g of lane l is D[row (g & 3) + 8 (g >> 2) + 4 (l >> 5)][column l & 31].  Written from the documented lane maps, not from the
# headers under test; a host program places it behind its includes.
MODEL_MFMA = r"""
typedef long long i64;
static void model_mfma(const i64 a[64][8], const i64 b[64][8], i64 c[64][16]) {
  i64 A[32][16], B[16][32];
  for (int l = 0; l < 64; l++)
    for (int j = 0; j < 8; j++) { A[l & 31][8 * (l >> 5) + j] = a[l][j]; B[8 * (l >> 5) + j][l & 31] = b[l][j]; }
  for (int l = 0; l < 64; l++)
    for (int g = 0; g < 16; g++) {
      const int row = (g & 3) + 8 * (g >> 2) + 4 * (l >> 5), col = l & 31;
      for (int k = 0; k < 16; k++) c[l][g] += A[row][k] * B[k][col];
    }
}
"""


def _decl(hdr, ret, name):
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"include/balatro_mi355x.h does not declare {name}"
    return m, [re.sub(r"/\*.*?\*/", "", p).strip() for p in m.group(1).replace("\n", " ").split(",")]
