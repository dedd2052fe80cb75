"""bg_linear_rows / bg_linear_rows_grad on the CPU (no GPU): the header's declarations and the library's exports; the fragment index functions of
csrc/bg_linear.h compiled with g++ under BG_LIN_HOST and driven through a scalar model of v_mfma_f32_32x32x16_bf16 -- tests/first_layer_helpers.py, written from the
documented lane maps, not from the header -- over asymmetric integer matrices, in the forward's and in the gradient's orientation; the gradient's split of the rows
against tests/linear_ref.py; the argument checks of `linear_rows` / `linear_rows_grad` / `RowLinear` on CPU stand-ins; `from_linear` / `to_linear`."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from tests import linear_ref as lin
from tests.first_layer_helpers import MODEL_MFMA, _decl
from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")

_PROGRAM = r"""
#define BG_LIN_HOST
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "bg_linear.h"
""" + MODEL_MFMA + r"""int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "groups")) {
    const i64 m = atoll(argv[2]); const int H = atoi(argv[3]);
    printf("%lld %lld %lld\n", (i64)bg_lin_groups(m, H), (i64)bg_lin_blocks_per_group(m, H), (i64)bg_lin_spans(H));
    return 0;
  }
  const int M = BG_LIN_ROWS, H = 64, K = BG_LIN_K, P = 168, TP = BG_LIN_ROWS + 8;
  std::vector<i64> X(M * K), W(H * K), DP(M * H);
  for (int i = 0; i < M; i++) for (int k = 0; k < K; k++) X[i * K + k] = (7 * i + 3 * k) % 11 - 5;
  for (int n = 0; n < H; n++) for (int k = 0; k < K; k++) W[n * K + k] = (3 * n + 5 * k) % 9 - 4;
  for (int i = 0; i < M; i++) for (int n = 0; n < H; n++) DP[i * H + n] = (5 * i + 2 * n) % 7 - 3;
  // the LDS images as the kernels lay them out: [row][k] of pitch P (forward), [k][row] of pitch TP (gradient), the reduction padded with zeros
  std::vector<i64> xa(M * P, 0), wb(H * P, 0), xt(BG_LIN_KPAD * TP, 0);
  for (int i = 0; i < M; i++) for (int k = 0; k < K; k++) { xa[i * P + k] = X[i * K + k]; xt[k * TP + i] = X[i * K + k]; }
  for (int n = 0; n < H; n++) for (int k = 0; k < K; k++) wb[n * P + k] = W[n * K + k];
  int bad = 0;
  // forward: out[i][n] = sum_k X[i][k] W[n][k]; wave w = rows 32w.., tile t = units 32t..
  for (int w = 0; w < M / BG_LIN_TILE; w++)
    for (int t = 0; t < H / BG_LIN_TILE; t++) {
      i64 c[64][16] = {};
      for (int s = 0; s < BG_LIN_KPAD / BG_LIN_KSTEP; s++) {
        i64 a[64][8], b[64][8];
        for (int l = 0; l < 64; l++)
          for (int j = 0; j < 8; j++) {
            a[l][j] = xa[w * BG_LIN_TILE * P + bg_lin_frag_off(l, s, P) + j];
            b[l][j] = wb[t * BG_LIN_TILE * P + bg_lin_frag_off(l, s, P) + j];
          }
        model_mfma(a, b, c);
      }
      for (int l = 0; l < 64; l++)
        for (int g = 0; g < 16; g++) {
          const int i = w * BG_LIN_TILE + bg_lin_acc_row(l, g), n = t * BG_LIN_TILE + bg_lin_acc_col(l);
          i64 want = 0;
          for (int k = 0; k < K; k++) want += X[i * K + k] * W[n * K + k];
          if (c[l][g] != want && bad++ < 5) printf("forward (%d, %d): %lld != %lld\n", i, n, c[l][g], want);
        }
    }
  // gradient: D[k][n] = sum_i X[i][k] DP[i][n]; the B fragment is read from DP directly: element j is row bg_lin_frag_k of unit bg_lin_frag_rc
  for (int kt = 0; kt < BG_LIN_KPAD / BG_LIN_TILE; kt++)
    for (int t = 0; t < H / BG_LIN_TILE; t++) {
      i64 c[64][16] = {};
      for (int s = 0; s < M / BG_LIN_KSTEP; s++) {
        i64 a[64][8], b[64][8];
        for (int l = 0; l < 64; l++)
          for (int j = 0; j < 8; j++) {
            a[l][j] = xt[kt * BG_LIN_TILE * TP + bg_lin_frag_off(l, s, TP) + j];
            b[l][j] = DP[bg_lin_frag_k(l, s, j) * H + t * BG_LIN_TILE + bg_lin_frag_rc(l)];
          }
        model_mfma(a, b, c);
      }
      for (int l = 0; l < 64; l++)
        for (int g = 0; g < 16; g++) {
          const int k = kt * BG_LIN_TILE + bg_lin_acc_row(l, g), n = t * BG_LIN_TILE + bg_lin_acc_col(l);
          i64 want = 0;
          if (k < K) for (int i = 0; i < M; i++) want += X[i * K + k] * DP[i * H + n];
          if (c[l][g] != want && bad++ < 5) printf("gradient (%d, %d): %lld != %lld\n", k, n, c[l][g], want);
        }
    }
  printf("relu %g %g %g %d\n", bg_lin_relu(-1.5f), bg_lin_relu(2.5f), bg_lin_relu(-0.0f), bg_lin_relu(__builtin_nanf("")) != bg_lin_relu(__builtin_nanf("")));
  printf(bad ? "MISMATCHES %d\n" : "OK %d\n", bad);
  return bad != 0;
}
"""


def test_header_declares_and_library_exports():
    from balatro_gym_amd import _native as nat, build
    hdr = open(HEADER).read()
    rows_args = ["const uint8_t*", "uint64_t", "int64_t", "const int32_t*", "int64_t", "int", "const double*", "const double*", "double", "double"]
    m, params = _decl(hdr, "int", "bg_linear_rows")
    want = rows_args + ["const void*", "uint64_t", "const float*", "int", "int", "int", "void*", "uint64_t", "float*", "void*"]
    assert len(params) == len(want) and all(p.startswith(t) for p, t in zip(params, want)), params
    doc = hdr[:m.start()].rsplit("/*", 1)[1]
    for word in ("CombinedExtractor", "nn.Linear", "mlp_extractor", 'PPO("MultiInputPolicy", ...)', "autograd backward", "hpc_train.py:92-93",
                 "train_balatro_fixed.py:361-363", "bg_encode_rows_ex", "BG_ENC_EXTRACTOR", "BG_E_ARG", "float64", "Out of scope", "two calls give the same bits",
                 "__builtin_amdgcn_mfma_f32_32x32x16_bf16", "64-bit"):
        assert word in doc, word
    _, params = _decl(hdr, "uint64_t", "bg_linear_rows_workspace_bytes")
    assert len(params) == 2 and params[0].startswith("int64_t") and params[1].startswith("int"), params
    _, params = _decl(hdr, "int", "bg_linear_rows_grad")
    want = rows_args + ["const void*", "int", "uint64_t", "const void*", "int", "uint64_t", "int", "int", "float*", "uint64_t", "float*", "void*", "uint64_t",
                        "float*", "void*"]
    assert len(params) == len(want) and all(p.startswith(t) for p, t in zip(params, want)), params
    assert re.search(r"#define\s+BG_LIN_NONE\s+0\b", hdr) and re.search(r"#define\s+BG_LIN_RELU\s+1\b", hdr)
    assert (nat.LIN_NONE, nat.LIN_RELU, nat.LIN_K) == (0, 1, 153)
    names = ("bg_linear_rows", "bg_linear_rows_workspace_bytes", "bg_linear_rows_grad")
    assert all(n in nat.EXPORTS for n in names)
    assert any(d.endswith("bg_linear.h") for d in build.DEPS)
    if not os.path.exists(build.LIB):
        pytest.skip("library not built")
    L = C.CDLL(build.LIB)
    assert all(hasattr(L, n) for n in names)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("linear_host")
    src, exe = d / "frag.cpp", d / "frag"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-o", str(exe), str(src)])
    return str(exe)


def test_fragment_maps_reproduce_the_products(program):
    """128 x 153 input, 64 x 153 weight, 128 x 64 dout, all asymmetric integers: the header's fragment offsets and accumulator coordinates, through the
    model of the instruction, give X W^T (forward) and X^T dout (gradient) exactly, rows 153..159 of the gradient zero."""
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK 0"), r.stdout[-2000:]
    assert "relu 0 2.5 0 1" in r.stdout, r.stdout   # max(v, +0.0), a NaN kept


def test_gradient_split_matches_the_statement(program):
    for m, H in ((1, 32), (128, 32), (129, 64), (20000, 64), (40000, 64), (32768, 256), (65536, 512), (65536, 1024), (2 ** 20, 512), (10 ** 7, 4096), (300, 288)):
        g, per, spans = (int(x) for x in subprocess.check_output([program, "groups", str(m), str(H)], text=True).split())
        assert g == lin.groups(m, H) and per * 128 == lin.grad_rows_per_group(m, H) and spans == -(-H // 256), (m, H)
        assert g * spans <= 256 and g * per >= -(-m // 128) > (g - 1) * per, (m, H)
        assert lin.workspace_bytes(m, H) <= 256 * 161 * 256 * 4   # 42 MB at the most
    assert lin.workspace_bytes(65536, 1024) == 64 * 161 * 1024 * 4 < 48 * 2 ** 20   # tens of MB at H = 1024


def test_wrappers_refuse_bad_arguments_before_the_library():
    """linear_rows / linear_rows_grad / RowLinear / RowBuffers.linear on CPU stand-ins: every bad argument is a ValueError before anything is loaded; what
    is left of a good call is that there is no CPU path."""
    import torch
    from balatro_gym_amd import RowLinear, RowNormalizer, linear_rows, linear_rows_grad
    from balatro_gym_amd.vec_env import RowBuffers
    K, N, H = 3, 5, 64
    cpu = torch.device("cpu")
    rows = torch.zeros((K, N, 384), dtype=torch.uint8)
    idx = torch.tensor([0, 14, 7, 7], dtype=torch.int32)
    w = torch.zeros((H, 628), dtype=torch.bfloat16)
    b = torch.zeros(H)
    nm = RowNormalizer(N, cpu)
    for bad in (idx.long(), idx.view(2, 2), [0, 1]):
        with pytest.raises(ValueError, match="index must be a contiguous torch.int32"):
            linear_rows(rows, w, b, index=bad)
        with pytest.raises(ValueError, match="index must be a contiguous torch.int32"):
            linear_rows_grad(rows, torch.zeros((4, H)), index=bad)
    for bad_w in (w.float(), torch.zeros((H, 447), dtype=torch.bfloat16), torch.zeros((H, 152), dtype=torch.bfloat16), torch.zeros(H * 153, dtype=torch.bfloat16),
                  torch.zeros((H, 1256), dtype=torch.bfloat16)[:, ::2], "w"):
        with pytest.raises(ValueError, match=r"weight must be a contiguous torch.bfloat16 tensor \[H, 153\] or \[H, 628\]"):
            linear_rows(rows, bad_w, None)
    for bad_h in (48, 0, 4128, 16):
        with pytest.raises(ValueError, match="multiple of 32"):
            linear_rows(rows, torch.zeros((bad_h, 153), dtype=torch.bfloat16))
        with pytest.raises(ValueError, match="multiple of 32"):
            RowLinear(bad_h)
        with pytest.raises(ValueError, match="multiple of 32"):
            linear_rows_grad(rows, torch.zeros((K * N, bad_h)))
    for bad_b in (torch.zeros(H + 1), torch.zeros(H, dtype=torch.bfloat16), torch.zeros((1, H)), torch.zeros(2 * H)[::2], [0.0] * H):
        with pytest.raises(ValueError, match="bias must be a contiguous torch.float32"):
            linear_rows(rows, w, bad_b)
    with pytest.raises(ValueError, match="layout must be 'produced' or 'fixed'"):
        linear_rows(rows, w, b, layout="extractor")
    with pytest.raises(ValueError, match="in_layout must be 'produced' or 'fixed'"):
        RowLinear(H, "extractor")
    for act in ("tanh", "gelu", 1):
        with pytest.raises(ValueError, match="activation must be None or 'relu'"):
            linear_rows(rows, w, b, activation=act)
        with pytest.raises(ValueError, match="activation must be None or 'relu'"):
            RowLinear(H, activation=act)
    with pytest.raises(ValueError, match="float32 or torch.bfloat16"):
        linear_rows(rows, w, b, dtype=torch.float16)
    with pytest.raises(ValueError, match="float32 or torch.bfloat16"):
        RowLinear(H, dtype=torch.float16)
    with pytest.raises(ValueError, match="norm must be a RowNormalizer"):
        linear_rows(rows, w, b, norm=object())
    with pytest.raises(ValueError, match="norm_obs=False"):
        linear_rows(rows, w, b, norm=RowNormalizer(N, cpu, norm_obs=False))
    for bad_rows in (rows.to(torch.int8), rows[:, :, :352][:, ::2], "rows"):
        with pytest.raises(ValueError, match="contiguous uint8 tensor"):
            linear_rows(bad_rows, w, b)
    with pytest.raises(ValueError, match="record stride"):
        linear_rows(torch.zeros((4, 360), dtype=torch.uint8), w, b)
    for out in (torch.zeros((3, H), dtype=torch.bfloat16), torch.zeros((4, H - 1), dtype=torch.bfloat16), torch.zeros((4, H)), torch.zeros((4, 2 * H), dtype=torch.bfloat16)[:, ::2],
                torch.zeros(4 * H, dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="out must be"):
            linear_rows(rows, w, b, index=idx, out=out)
    # the gradient: dout / out / dweight
    for bad_d in (torch.zeros((3, H)), torch.zeros((4, H), dtype=torch.float64), torch.zeros((4, 2 * H))[:, ::2], torch.zeros(4 * H)):
        with pytest.raises(ValueError, match="dout must be"):
            linear_rows_grad(rows, bad_d, index=idx)
    with pytest.raises(ValueError, match="out .* is required with activation='relu'"):
        linear_rows_grad(rows, torch.zeros((4, H)), index=idx, activation="relu")
    with pytest.raises(ValueError, match="must be None without it"):
        linear_rows_grad(rows, torch.zeros((4, H)), index=idx, out=torch.zeros((4, H)))
    for bad_dw in (torch.zeros((H, 152)), torch.zeros((H, 628), dtype=torch.bfloat16), torch.zeros((H, 1256))[:, ::2]):
        with pytest.raises(ValueError, match="dweight must be a contiguous torch.float32"):
            linear_rows_grad(rows, torch.zeros((4, H)), index=idx, dweight=bad_dw)
    # good arguments: only the device is missing
    rb = RowBuffers(N, cpu, steps=K, row_stride=384)
    layer = RowLinear(H, "fixed", activation="relu")
    for call in (lambda: linear_rows(rows, w, b), lambda: linear_rows(rows, w[:, :153].contiguous(), None, index=idx, norm=nm, layout="produced", activation="relu"),
                 lambda: linear_rows(rows, w, b, index=idx, out=torch.zeros((4, H + 3), dtype=torch.bfloat16)),
                 lambda: linear_rows_grad(rows, torch.zeros((4, H)), index=idx), lambda: linear_rows_grad(rows, torch.zeros((4, H)), out=torch.zeros((4, H)), index=idx, activation="relu"),
                 lambda: layer(rows), lambda: rb.linear(layer, idx, nm)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            call()


def test_row_linear_parameters_round_trip():
    """RowLinear is initialised as nn.Linear (same shapes, same generator draws), and from_linear / to_linear move the parameters exactly, so a state dict
    passes between it and the nn.Linear SB3 builds."""
    import torch
    from balatro_gym_amd import RowLinear
    for layout, cols in (("fixed", 628), ("produced", 153)):
        torch.manual_seed(9)
        layer = RowLinear(96, layout, activation="relu")
        torch.manual_seed(9)
        twin = torch.nn.Linear(cols, 96)
        assert layer.weight.shape == (96, cols) and layer.bias.shape == (96,) and layer.weight.dtype == layer.bias.dtype == torch.float32
        assert torch.equal(layer.weight, twin.weight) and torch.equal(layer.bias, twin.bias)
        assert layer.weight.requires_grad and layer.bias.requires_grad and sorted(dict(layer.named_parameters())) == ["bias", "weight"]
        lin2 = layer.to_linear()
        assert isinstance(lin2, torch.nn.Linear) and (lin2.in_features, lin2.out_features) == (cols, 96)
        assert torch.equal(lin2.weight, layer.weight) and torch.equal(lin2.bias, layer.bias) and lin2.weight.data_ptr() != layer.weight.data_ptr()
        back = RowLinear.from_linear(lin2, activation="relu")
        assert back.in_layout == layout and back.activation == "relu" and torch.equal(back.weight, layer.weight) and torch.equal(back.bias, layer.bias)
        lin2.load_state_dict(back.state_dict())
        back.load_state_dict(torch.nn.Linear(cols, 96).state_dict())
    with pytest.raises(ValueError, match="153 .* or 628"):
        RowLinear.from_linear(torch.nn.Linear(447, 64))
    with pytest.raises(ValueError, match="153 .* or 628"):
        RowLinear.from_linear(torch.nn.Linear(628, 64, bias=False))
