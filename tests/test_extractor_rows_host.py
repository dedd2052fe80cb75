"""bg_extractor_rows / bg_extractor_rows_grad on the CPU (no GPU): the header's declarations and the library's exports; the index functions of
csrc/bg_extractor.h compiled with g++ under BG_EXT_HOST and driven through a scalar model of v_mfma_f32_32x32x16_bf16 -- tests/first_layer_helpers.py,
written from the documented lane maps, not from the header -- over a one-hot-plus-integer input, in the forward's and in the gradient's orientation; the gradient's split
of rows, units and k against tests/extractor_ref.py; the argument checks of `extractor_rows` / `extractor_rows_grad` / `RowExtractor` on CPU stand-ins;
`from_linear` / `to_linear` / `from_linears` / `to_linears`."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from tests import extractor_ref as ext
from tests.first_layer_helpers import MODEL_MFMA, _decl
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")

# The input: hand bytes [128][8] with every kind of byte (cards, -1, 52, 127, -128, the same card twice), 31 dense integer columns.
_PROGRAM = r"""
#define BG_EXT_HOST
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "bg_extractor.h"
""" + MODEL_MFMA + r"""static i64 one(uint16_t bits) { return bits == 0x3f80 ? 1 : bits == 0 ? 0 : 1000000; }   // bfloat16 1.0 / +0.0 as integers; anything else is loud
int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "groups")) {
    const i64 m = atoll(argv[2]); const int H = atoi(argv[3]);
    printf("%lld %lld %lld %llu\n", (i64)bg_ext_groups(m, H), (i64)bg_ext_blocks_per_group(m, H), (i64)bg_lin_spans(H), (unsigned long long)bg_ext_workspace_bytes(m, H));
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "ws")) { printf("%llu\n", (unsigned long long)bg_ext_workspace_bytes(atoll(argv[2]), atoi(argv[3]))); return 0; }
  if (argc == 2 && !strcmp(argv[1], "spans")) {
    for (int z = 0; z < BG_EXT_KSPANS; z++) printf("%d %d ", bg_ext_span_tile0(z), bg_ext_span_tiles(z));
    printf("%d %d %d %d %d\n", BG_EXT_K, BG_EXT_KPAD, BG_EXT_HOT, BG_EXT_PART_ROWS, BG_EXT_KTILES);
    return 0;
  }
  const int M = BG_LIN_ROWS, H = 64, K = BG_EXT_K, KP = BG_EXT_KPAD;
  std::vector<int> hand(M * 8);
  std::vector<i64> X(M * KP, 0), W(H * KP, 0), DP(M * H);
  for (int i = 0; i < M; i++)
    for (int s = 0; s < 8; s++) {
      int b = (i * 7 + s * 13 + i * s) % 56 - 2;   // -2 .. 53
      if (b == -2) b = -128;
      if (b == 53) b = 127;
      if (i == 0) b = -1;
      if (i == 1) { const int r1[8] = {51, 51, 0, 0, 52, 127, -128, -1}; b = r1[s]; }
      hand[i * 8 + s] = b;
    }
  int hot = 0;
  for (int i = 0; i < M; i++) {
    for (int k = 0; k < BG_EXT_HOT; k++) { X[i * KP + k] = hand[i * 8 + k / 52] == k % 52; hot += (int)X[i * KP + k]; }
    for (int k = BG_EXT_HOT; k < K; k++) X[i * KP + k] = (7 * i + 3 * k) % 11 - 5;
  }
  for (int k : {51, 103, 104, 156}) if (X[1 * KP + k] != 1) { printf("row 1 column %d\n", k); return 1; }
  int row1 = 0; for (int k = 0; k < BG_EXT_HOT; k++) row1 += (int)X[1 * KP + k];
  if (row1 != 4 || hot < 6 * M) { printf("input: row 1 has %d, all %d\n", row1, hot); return 1; }
  for (int n = 0; n < H; n++) for (int k = 0; k < K; k++) W[n * KP + k] = (3 * n + 5 * k) % 9 - 4;
  for (int i = 0; i < M; i++) for (int n = 0; n < H; n++) DP[i * H + n] = (5 * i + 2 * n) % 7 - 3;
  int bad = 0;
  // forward: out[i][n] = sum_k X[i][k] W[n][k]; wave w = rows 32w.., tile t = units 32t..; one-hot A fragments by bg_ext_hot_q / bg_ext_hot_elem from the
  // lane's row's bytes, the two dense ones from an image [row][32], B from an image [unit][448]
  for (int w = 0; w < M / BG_LIN_TILE; w++)
    for (int t = 0; t < H / BG_LIN_TILE; t++) {
      i64 c[64][16] = {};
      for (int s = 0; s < BG_EXT_STEPS; s++) {
        i64 a[64][8], b[64][8];
        for (int l = 0; l < 64; l++) {
          const int row = w * BG_LIN_TILE + bg_lin_frag_rc(l);
          int q[BG_EXT_SLOTS];
          for (int sl = 0; sl < BG_EXT_SLOTS; sl++) q[sl] = bg_ext_hot_q(sl, hand[row * 8 + sl], l);
          for (int j = 0; j < 8; j++) {
            a[l][j] = s < BG_EXT_HOT_STEPS ? one(bg_ext_hot_elem(q, s, j)) : X[row * KP + BG_EXT_HOT + bg_lin_frag_k(l, s - BG_EXT_HOT_STEPS, j)];
            b[l][j] = W[t * BG_LIN_TILE * KP + bg_lin_frag_off(l, s, KP) + j];
          }
        }
        model_mfma(a, b, c);
      }
      for (int l = 0; l < 64; l++)
        for (int g = 0; g < 16; g++) {
          const int i = w * BG_LIN_TILE + bg_lin_acc_row(l, g), n = t * BG_LIN_TILE + bg_lin_acc_col(l);
          i64 want = 0;
          for (int k = 0; k < K; k++) want += X[i * KP + k] * W[n * KP + k];
          if (c[l][g] != want && bad++ < 5) printf("forward (%d, %d): %lld != %lld\n", i, n, c[l][g], want);
        }
    }
  // gradient: D[k][n] = sum_i X[i][k] DP[i][n] over the k spans: a one-hot tile's A fragment is 8 records' bytes of slot(k) against card(k) (bg_ext_hot),
  // the dense tile's from the transposed image; B from DP directly
  int tiles_seen = 0;
  for (int z = 0; z < BG_EXT_KSPANS; z++)
    for (int kt = 0; kt < bg_ext_span_tiles(z); kt++, tiles_seen++)
      for (int t = 0; t < H / BG_LIN_TILE; t++) {
        const int tile = bg_ext_span_tile0(z) + kt;
        i64 c[64][16] = {};
        for (int s = 0; s < M / BG_LIN_KSTEP; s++) {
          i64 a[64][8], b[64][8];
          for (int l = 0; l < 64; l++)
            for (int j = 0; j < 8; j++) {
              const int k = bg_ext_tile_k(tile, l), i = bg_lin_frag_k(l, s, j);
              a[l][j] = tile < BG_EXT_HOT_TILES ? one(bg_ext_hot(hand[i * 8 + bg_ext_slot(k)] & 0xff, k)) : X[i * KP + k];
              b[l][j] = DP[i * H + t * BG_LIN_TILE + bg_lin_frag_rc(l)];
            }
          model_mfma(a, b, c);
        }
        for (int l = 0; l < 64; l++)
          for (int g = 0; g < 16; g++) {
            const int k = tile * BG_LIN_TILE + bg_lin_acc_row(l, g), n = t * BG_LIN_TILE + bg_lin_acc_col(l);
            i64 want = 0;
            if (k < K) for (int i = 0; i < M; i++) want += X[i * KP + k] * DP[i * H + n];
            if (c[l][g] != want && bad++ < 5) printf("gradient (%d, %d): %lld != %lld\n", k, n, c[l][g], want);
          }
      }
  if (tiles_seen != BG_EXT_KTILES) { printf("the k spans cover %d tiles\n", tiles_seen); return 1; }
  printf(bad ? "MISMATCHES %d\n" : "OK %d\n", bad);
  return bad != 0;
}
"""


def test_header_declares_and_library_exports():
    import balatro_gym_amd
    from balatro_gym_amd import _native as nat, build
    hdr = open(HEADER).read()
    rows_args = ["const uint8_t*", "uint64_t", "int64_t", "const int32_t*", "int64_t"]
    m, params = _decl(hdr, "int", "bg_extractor_rows")
    want = rows_args + ["const void*", "uint64_t", "const float*", "int", "int", "int", "void*", "uint64_t", "float*", "void*"]
    assert len(params) == len(want) and all(p.startswith(t) for p, t in zip(params, want)), params
    doc = hdr[:m.start()].rsplit("/*", 1)[1]
    for word in ("BalatroFeaturesExtractor", "train_balatro_agent.py:84-119", "hand_net", "joker_net", "game_state_net", "bg_encode_rows_ex", "BG_ENC_EXTRACTOR",
                 "52 slot + card", "-1, 52..127", "two slots", "VecNormalize", "BG_E_ARG", "float64", "groups * 449 * H * 4", "Out of scope", "combined_net",
                 "two calls give the same bits", "no atomics", "__builtin_amdgcn_mfma_f32_32x32x16_bf16", "64-bit", "BG_LIN_RELU"):
        assert word in doc, word
    _, params = _decl(hdr, "uint64_t", "bg_extractor_rows_workspace_bytes")
    assert len(params) == 2 and params[0].startswith("int64_t") and params[1].startswith("int"), params
    _, params = _decl(hdr, "int", "bg_extractor_rows_grad")
    want = rows_args + ["const void*", "int", "uint64_t", "const void*", "int", "uint64_t", "int", "int", "float*", "uint64_t", "float*", "void*", "uint64_t",
                        "float*", "void*"]
    assert len(params) == len(want) and all(p.startswith(t) for p, t in zip(params, want)), params
    # bg_linear_rows keeps its words about the layout it refuses
    lin_doc = hdr[:_decl(hdr, "int", "bg_linear_rows")[0].start()].rsplit("/*", 1)[1]
    assert "BG_ENC_EXTRACTOR is a BG_E_ARG (its 416 one-hot columns want an embedding gather)" in lin_doc
    assert (nat.EXT_K, nat.EXT_SPLITS) == (447, (416, 10, 21)) and nat.EXT_K == nat.ENC_COLS[nat.ENC_EXTRACTOR]
    names = ("bg_extractor_rows", "bg_extractor_rows_workspace_bytes", "bg_extractor_rows_grad")
    assert all(n in nat.EXPORTS for n in names)
    assert any(d.endswith("bg_extractor.h") for d in build.DEPS)
    assert '#include "bg_rows_api.h"' in open(os.path.join(CSRC, "bg_lib.hip")).read() and '#include "bg_extractor.h"' in open(os.path.join(CSRC, "bg_rows_api.h")).read()
    for name in ("extractor_rows", "extractor_rows_grad", "RowExtractor"):
        assert name in balatro_gym_amd.__all__ and callable(getattr(balatro_gym_amd, name))
    if not os.path.exists(build.LIB):
        pytest.skip("library not built")
    L = C.CDLL(build.LIB)
    assert all(hasattr(L, n) for n in names)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("extractor_host")
    src, exe = d / "frag.cpp", d / "frag"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-o", str(exe), str(src)])
    return str(exe)


def test_fragment_rules_reproduce_the_products(program):
    """128 x 447 input (one-hot from hand bytes of every kind, 31 integer columns), 64 x 447 weight, 128 x 64 dout: the header's one-hot rules, k spans and
    fragment offsets, through the model of the instruction, give X W^T (forward) and X^T dout (gradient) exactly, row 447 of the gradient zero."""
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK 0"), r.stdout[-2000:]
    out = subprocess.check_output([program, "spans"], text=True).split()
    assert [int(x) for x in out] == [0, 5, 5, 5, 10, 4, ext.K, ext.KPAD, 416, ext.PART_ROWS, 14]


def test_gradient_split_matches_the_statement(program):
    for m, H in ((1, 32), (128, 32), (129, 64), (20000, 64), (40000, 64), (32768, 256), (65536, 512), (65536, 1024), (2 ** 20, 512), (10 ** 7, 4096), (300, 288)):
        g, per, spans, ws = (int(x) for x in subprocess.check_output([program, "groups", str(m), str(H)], text=True).split())
        assert g == ext.groups(m, H) and per == ext.blocks_per_group(m, H) and per * 128 == ext.grad_rows_per_group(m, H) and spans == -(-H // 256), (m, H)
        assert g * spans * ext.KSPANS <= 256 and g * per >= -(-m // 128) > (g - 1) * per, (m, H)
        assert ws == ext.workspace_bytes(m, H) == g * 449 * H * 4 <= 40 * 10 ** 6   # tens of MB
    assert ext.workspace_bytes(65536, 1024) == 21 * 449 * 1024 * 4 < 40 * 2 ** 20   # tens of MB at H = 1024
    assert max(ext.workspace_bytes(10 ** 7, H) for H in range(32, 4097, 32)) <= 40 * 10 ** 6
    for m, H in ((0, 64), (-1, 64), (100, 48), (100, 0), (100, 4128)):
        assert int(subprocess.check_output([program, "ws", str(m), str(H)], text=True)) == 0
    m2 = ext.smallest_m_with_two_blocks_per_group(64)
    assert m2 == 85 * 128 + 1 and ext.blocks_per_group(m2, 64) == 2 and ext.blocks_per_group(m2 - 1, 64) == 1


def test_wrappers_refuse_bad_arguments_before_the_library():
    """extractor_rows / extractor_rows_grad / RowExtractor / RowBuffers.extractor on CPU stand-ins: every bad argument is a ValueError before anything is
    loaded; what is left of a good call is that there is no CPU path."""
    import torch
    from balatro_gym_amd import RowExtractor, extractor_rows, extractor_rows_grad
    from balatro_gym_amd.vec_env import RowBuffers
    K, N, H = 3, 5, 64
    rows = torch.zeros((K, N, 384), dtype=torch.uint8)
    idx = torch.tensor([0, 14, 7, 7], dtype=torch.int32)
    w = torch.zeros((H, 447), dtype=torch.bfloat16)
    b = torch.zeros(H)
    for bad in (idx.long(), idx.view(2, 2), [0, 1]):
        with pytest.raises(ValueError, match="index must be a contiguous torch.int32"):
            extractor_rows(rows, w, b, index=bad)
        with pytest.raises(ValueError, match="index must be a contiguous torch.int32"):
            extractor_rows_grad(rows, torch.zeros((4, H)), index=bad)
    for bad_w in (w.float(), torch.zeros((H, 448), dtype=torch.bfloat16), torch.zeros((H, 628), dtype=torch.bfloat16), torch.zeros((H, 153), dtype=torch.bfloat16),
                  torch.zeros(H * 447, dtype=torch.bfloat16), torch.zeros((H, 894), dtype=torch.bfloat16)[:, ::2], "w"):
        with pytest.raises(ValueError, match=r"weight must be a torch.bfloat16 tensor \[H, 447\]"):
            extractor_rows(rows, bad_w, None)
    for bad_h in (48, 0, 4128, 16):
        with pytest.raises(ValueError, match="multiple of 32"):
            extractor_rows(rows, torch.zeros((bad_h, 447), dtype=torch.bfloat16))
        with pytest.raises(ValueError, match="multiple of 32"):
            RowExtractor(bad_h)
        with pytest.raises(ValueError, match="multiple of 32"):
            extractor_rows_grad(rows, torch.zeros((K * N, bad_h)))
    for bad_b in (torch.zeros(H + 1), torch.zeros(H, dtype=torch.bfloat16), torch.zeros((1, H)), torch.zeros(2 * H)[::2], [0.0] * H):
        with pytest.raises(ValueError, match="bias must be a contiguous torch.float32"):
            extractor_rows(rows, w, bad_b)
    for act in ("tanh", "gelu", 1):
        with pytest.raises(ValueError, match="activation must be None or 'relu'"):
            extractor_rows(rows, w, b, activation=act)
        with pytest.raises(ValueError, match="activation must be None or 'relu'"):
            extractor_rows_grad(rows, torch.zeros((K * N, H)), activation=act)
        with pytest.raises(ValueError, match="activation must be None or 'relu'"):
            RowExtractor(H, activation=act)
    with pytest.raises(ValueError, match="float32 or torch.bfloat16"):
        extractor_rows(rows, w, b, dtype=torch.float16)
    with pytest.raises(ValueError, match="float32 or torch.bfloat16"):
        RowExtractor(H, dtype=torch.float16)
    with pytest.raises(TypeError):
        extractor_rows(rows, w, b, norm=None)   # there are no statistics for this layout: the call does not take them
    for bad_rows in (rows.to(torch.int8), rows[:, :, :352][:, ::2], "rows"):
        with pytest.raises(ValueError, match="contiguous uint8 tensor"):
            extractor_rows(bad_rows, w, b)
    with pytest.raises(ValueError, match="record stride"):
        extractor_rows(torch.zeros((4, 360), dtype=torch.uint8), w, b)
    for out in (torch.zeros((3, H), dtype=torch.bfloat16), torch.zeros((4, H - 1), dtype=torch.bfloat16), torch.zeros((4, H)), torch.zeros((4, 2 * H), dtype=torch.bfloat16)[:, ::2],
                torch.zeros(4 * H, dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="out must be"):
            extractor_rows(rows, w, b, index=idx, out=out)
    for bad_d in (torch.zeros((3, H)), torch.zeros((4, H), dtype=torch.float64), torch.zeros((4, 2 * H))[:, ::2], torch.zeros(4 * H)):
        with pytest.raises(ValueError, match="dout must be"):
            extractor_rows_grad(rows, bad_d, index=idx)
    with pytest.raises(ValueError, match="out .* is required with activation='relu'"):
        extractor_rows_grad(rows, torch.zeros((4, H)), index=idx, activation="relu")
    with pytest.raises(ValueError, match="must be None without it"):
        extractor_rows_grad(rows, torch.zeros((4, H)), index=idx, out=torch.zeros((4, H)))
    for bad_dw in (torch.zeros((H, 446)), torch.zeros((H, 447), dtype=torch.bfloat16), torch.zeros((H, 894))[:, ::2]):
        with pytest.raises(ValueError, match="dweight must be a torch.float32"):
            extractor_rows_grad(rows, torch.zeros((4, H)), index=idx, dweight=bad_dw)
    for bad_db in (torch.zeros(H + 1), torch.zeros(H, dtype=torch.float64), torch.zeros(2 * H)[::2]):
        with pytest.raises(ValueError, match="dbias must be a contiguous torch.float32"):
            extractor_rows_grad(rows, torch.zeros((4, H)), index=idx, dbias=bad_db)
    # good arguments: only the device is missing
    rb = RowBuffers(N, torch.device("cpu"), steps=K, row_stride=384)
    layer = RowExtractor(H)
    wide = torch.zeros((H, 448), dtype=torch.bfloat16)[:, :447]   # a [H, 447] view with a wider pitch passes
    for call in (lambda: extractor_rows(rows, w, b), lambda: extractor_rows(rows, wide, None, index=idx, activation="relu"),
                 lambda: extractor_rows(rows, w, b, index=idx, out=torch.zeros((4, H + 3), dtype=torch.bfloat16)),
                 lambda: extractor_rows_grad(rows, torch.zeros((4, H)), index=idx),
                 lambda: extractor_rows_grad(rows, torch.zeros((4, H)), out=torch.zeros((4, H)), index=idx, activation="relu", dweight=torch.zeros((H, 456))[:, :450],
                                             dbias=torch.zeros(H)),
                 lambda: layer(rows), lambda: rb.extractor(layer, idx)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()


def test_row_extractor_parameters_round_trip():
    """RowExtractor is initialised as nn.Linear(447, H) (same shapes, same generator draws), and from_linear / to_linear move the parameters exactly."""
    import torch
    from balatro_gym_amd import RowExtractor
    torch.manual_seed(9)
    layer = RowExtractor(96)
    torch.manual_seed(9)
    twin = torch.nn.Linear(447, 96)
    assert layer.weight.shape == (96, 447) and layer.bias.shape == (96,) and layer.weight.dtype == layer.bias.dtype == torch.float32
    assert torch.equal(layer.weight, twin.weight) and torch.equal(layer.bias, twin.bias)
    assert layer.activation == "relu" and layer.dtype == torch.bfloat16 and layer.splits == (96,) and layer.block_mask is None
    assert layer.weight.requires_grad and layer.bias.requires_grad and sorted(dict(layer.named_parameters())) == ["bias", "weight"]
    lin2 = layer.to_linear()
    assert isinstance(lin2, torch.nn.Linear) and (lin2.in_features, lin2.out_features) == (447, 96)
    assert torch.equal(lin2.weight, layer.weight) and torch.equal(lin2.bias, layer.bias) and lin2.weight.data_ptr() != layer.weight.data_ptr()
    back = RowExtractor.from_linear(lin2, activation=None)
    assert back.activation is None and torch.equal(back.weight, layer.weight) and torch.equal(back.bias, layer.bias)
    lin2.load_state_dict(back.state_dict())
    back.load_state_dict(torch.nn.Linear(447, 96).state_dict())
    for bad in (torch.nn.Linear(153, 64), torch.nn.Linear(628, 64), torch.nn.Linear(447, 64, bias=False)):
        with pytest.raises(ValueError, match="447 inputs"):
            RowExtractor.from_linear(bad)
    with pytest.raises(ValueError, match="from_linears"):
        layer.to_linears()


def test_from_linears_round_trip():
    """The reference's three first layers (256 + 128 + 64 = 448 units over 416, 10 and 21 inputs) as one block-structured weight and back, bit for bit;
    wrong in_features and a sum of out_features that is no multiple of 32 are refused."""
    import torch
    from balatro_gym_amd import RowExtractor
    torch.manual_seed(4)
    hand, joker, state = torch.nn.Linear(416, 256), torch.nn.Linear(10, 128), torch.nn.Linear(21, 64)
    layer = RowExtractor.from_linears(hand, joker, state)
    assert layer.splits == (256, 128, 64) and layer.out_features == 448 and layer.weight.shape == (448, 447) and layer.activation == "relu"
    assert "block_mask" in dict(layer.named_buffers()) and "block_mask" not in dict(layer.named_parameters())
    mask = layer.block_mask
    assert mask.shape == (448, 447) and mask.dtype == torch.float32 and int(mask.sum()) == 256 * 416 + 128 * 10 + 64 * 21
    assert bool(mask[:256, :416].all()) and bool(mask[256:384, 416:426].all()) and bool(mask[384:, 426:].all())
    w = layer.weight.detach()
    assert torch.equal(w[:256, :416], hand.weight) and torch.equal(w[256:384, 416:426], joker.weight) and torch.equal(w[384:, 426:], state.weight)
    assert not bool(w[mask == 0].any()) and not bool(torch.signbit(w[mask == 0]).any())   # off-block: +0.0
    assert torch.equal(layer.bias.detach(), torch.cat([hand.bias, joker.bias, state.bias]))
    out = torch.arange(2 * 448.0).view(2, 448)
    a, b, c = out.split(layer.splits, dim=1)
    assert a.shape == (2, 256) and b.shape == (2, 128) and c.shape == (2, 64)
    for got, src in zip(layer.to_linears(), (hand, joker, state)):
        assert isinstance(got, torch.nn.Linear) and (got.in_features, got.out_features) == (src.in_features, src.out_features)
        assert torch.equal(got.weight, src.weight) and torch.equal(got.bias, src.bias) and got.weight.data_ptr() != src.weight.data_ptr()
    again = RowExtractor.from_linears(*layer.to_linears(), activation=None)
    assert again.activation is None and torch.equal(again.weight, layer.weight) and torch.equal(again.block_mask, mask)
    whole = RowExtractor.from_linear(layer.to_linear())
    assert torch.equal(whole.weight, layer.weight) and whole.splits == (448,) and whole.block_mask is None
    clone = RowExtractor.from_linears(torch.nn.Linear(416, 256), torch.nn.Linear(10, 128), torch.nn.Linear(21, 64))
    clone.load_state_dict(layer.state_dict())
    assert torch.equal(clone.weight, layer.weight) and torch.equal(clone.block_mask, mask)
    for bad in ((torch.nn.Linear(416, 256), torch.nn.Linear(160, 128), torch.nn.Linear(21, 64)),    # the constructor's declared joker_dim
                (torch.nn.Linear(416, 256), torch.nn.Linear(10, 128), torch.nn.Linear(32, 64)),     # the constructor's declared game_state_dim
                (torch.nn.Linear(415, 256), torch.nn.Linear(10, 128), torch.nn.Linear(21, 64)),
                (torch.nn.Linear(416, 256, bias=False), torch.nn.Linear(10, 128), torch.nn.Linear(21, 64))):
        with pytest.raises(ValueError, match="in_features"):
            RowExtractor.from_linears(*bad)
    with pytest.raises(ValueError, match="multiple of 32"):
        RowExtractor.from_linears(torch.nn.Linear(416, 256), torch.nn.Linear(10, 128), torch.nn.Linear(21, 60))
