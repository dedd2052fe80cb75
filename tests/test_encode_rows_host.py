"""bg_encode_rows on the CPU (no GPU): csrc/bg_encode.h -- the column tables, the per-element conversion and the bf16 rounding, the very text the kernel
runs -- is compiled with g++ into a small program that encodes records from a file, and held, bit for bit over every element, to the numpy restatement
of tests/encode_ref.py: the reference's own wrapper observations (sb3_fixed.npz, all 628 columns), late-game traces, and synthetic records at the
limits of every field's dtype.  Also: _native.ENC_COLUMNS against the header's tables and BG_ROW_* offsets, the exports, and the argument checks of the
Python wrappers."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from tests import encode_ref as ref
from tests.helpers import OBS_KEYS, ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")
LAYOUT_ID = {"produced": 0, "fixed": 1, "extractor": 2}

_PROGRAM = r"""
#define BG_ENC_HOST
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "balatro_mi355x.h"
#include "bg_encode.h"
template <int L>
static int run(int bf16, size_t stride, size_t m, const uint8_t* rows, FILE* out) {
  const int D = bg_enc_cols(L);
  for (size_t r = 0; r < m; r++)
    for (int c = 0; c < D; c++) {
      const uint32_t u = bg_enc_element<L>(rows + r * stride, BgEncTab<L>::t.d[c]);
      const uint16_t h = bg_enc_bf16(u);
      if (fwrite(bf16 ? (const void*)&h : (const void*)&u, bf16 ? 2 : 4, 1, out) != 1) return 3;
    }
  return 0;
}
template <int L>
static void table() {
  for (int c = 0; c < bg_enc_cols(L); c++) {
    const uint32_t d = BgEncTab<L>::t.d[c];
    printf("col %d %d %u %u %u %u\n", L, c, BG_ENC_OFF(d), BG_ENC_TYPE(d), BG_ENC_OP(d), BG_ENC_PAR(d));
  }
}
int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "table")) {
#define P(k, o, t, n) printf("produced %s %d %d %d\n", #k, (int)(o), (int)(t), (int)(n));
    BG_ENC_PRODUCED_KEYS(P)
#define Z(k, n) printf("zero %s %d\n", #k, (int)(n));
    BG_ENC_ZERO_KEYS(Z)
#define S(k, o, t, n, dv) printf("state %s %d %d %d %.9g\n", #k, (int)(o), (int)(t), (int)(n), (dv) >= 0 ? (double)bg_enc_divisor((dv) >= 0 ? (dv) : 0) : 0.0);
    BG_ENC_EXTRACTOR_STATE(S)
    printf("cols %d %d %d\n", bg_enc_cols(0), bg_enc_cols(1), bg_enc_cols(2));
    table<0>(); table<1>(); table<2>();
    return 0;
  }
  if (argc != 7) return 2;
  const int layout = atoi(argv[1]), bf16 = atoi(argv[2]);
  const size_t stride = strtoull(argv[3], 0, 10), m = strtoull(argv[4], 0, 10);
  uint8_t* rows = (uint8_t*)aligned_alloc(16, m * stride + 16);
  FILE* in = fopen(argv[5], "rb");
  if (!in || fread(rows, 1, m * stride, in) != m * stride) return 4;
  fclose(in);
  FILE* out = fopen(argv[6], "wb");
  if (!out) return 5;
  const int rc = layout == 0 ? run<0>(bf16, stride, m, rows, out) : layout == 1 ? run<1>(bf16, stride, m, rows, out) : run<2>(bf16, stride, m, rows, out);
  fclose(out);
  return rc;
}
"""


@pytest.fixture(scope="module")
def encoder(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("encode_host")
    src = d / "encode_host.cpp"
    src.write_text(_PROGRAM)
    exe = d / "encode_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", CSRC, "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])

    def encode(rows, layout, bf16):
        """rows: uint8 [m, stride] -> the encoded bit patterns, uint32 (f32) or uint16 (bf16) [m, D]."""
        rows = np.ascontiguousarray(rows)
        m, stride = rows.shape
        fin, fout = d / "rows.bin", d / "out.bin"
        rows.tofile(str(fin))
        subprocess.check_call([str(exe), str(LAYOUT_ID[layout]), str(int(bf16)), str(stride), str(m), str(fin), str(fout)])
        return np.fromfile(str(fout), np.uint16 if bf16 else np.uint32).reshape(m, ref.COLS[layout])
    encode.exe = str(exe)
    return encode


def _check_all(encode, obs, stride, what):
    rows = ref.pack_records(obs, stride)
    for layout in ref.LAYOUTS:
        want = ref.expected_bits(layout, obs)
        assert want.shape == (len(rows), ref.COLS[layout])
        got = encode(rows, layout, False)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{what} {layout} f32: {len(bad)} elements differ, first (record, column) {tuple(bad[0])}: {got[tuple(bad[0])]:#x} != {want[tuple(bad[0])]:#x}"
        got = encode(rows, layout, True)
        bad = np.argwhere(got != ref.bf16_bits(want))
        assert bad.size == 0, f"{what} {layout} bf16: {len(bad)} elements differ, first (record, column) {tuple(bad[0])}"


def test_sb3_fixture_all_628_columns(encoder):
    """All 24 x (1 + 120) fixed observations of the reference's wrappers -> records -> FIXED equals the 51 keys `.astype(float32)` flattened and
    concatenated in `keys` order (zeros included); PRODUCED is its first 153 columns."""
    from balatro_gym_amd import _native as nat
    g = ref.sb3_fixture()
    assert [str(k) for k in g["keys"][:31]] == nat.OBS_KEYS == OBS_KEYS and [str(k) for k in g["keys"][31:]] == [k for k, _ in ref.ZERO_KEYS]
    S, T = g["actions"].shape
    for prefix, lead in (("obs0_", (S,)), ("obs_", (S, T))):
        m = int(np.prod(lead))
        want = ref.sb3_fixed_bits(g, prefix, lead)
        assert want.shape == (m, 628) and not want[:, 153:].any()
        obs = {k: g[prefix + k].reshape((m,) + g[prefix + k].shape[len(lead):]) for k in OBS_KEYS}
        for stride in (384, 352):
            rows = ref.pack_records(obs, stride)
            assert np.array_equal(encoder(rows, "fixed", False), want), (prefix, stride)
            assert np.array_equal(encoder(rows, "produced", False), want[:, :153]), (prefix, stride)
            assert np.array_equal(encoder(rows, "fixed", True), ref.bf16_bits(want)), (prefix, stride)
        # and the restatement used everywhere else agrees with the fixture
        unpacked = ref.unpack_records(rows)
        assert np.array_equal(ref.expected_bits("fixed", unpacked), want)


@pytest.mark.parametrize("trace", ["c5_uniform_rich", "consumables_scorer"])
def test_late_game_traces_all_layouts(encoder, trace):
    """Late antes, jokers, consumables, shops (sb3_fixed.npz stays at ante 1): every 31-key observation of the trace through all three layouts."""
    obs = ref.trace_obs(trace)
    assert obs["ante"].max() > 1 and obs["joker_ids"].max() > 0
    _check_all(encoder, obs, 384, trace)


def test_synthetic_records_at_the_limits(encoder):
    """Every field at its dtype's minimum, maximum, 0 and -1; chips_scored at +-(2**24 + 1), 2**31, 2**53 + 1, int64 min / max; special float32 patterns in
    progress_ratio; 10 000 records of random bytes with hand in -1..51.  f32 and bf16, both record strides."""
    obs = ref.synthetic_obs()
    assert len(obs["hand"]) > 10000
    _check_all(encoder, obs, 384, "synthetic")
    _check_all(encoder, {k: v[:64] for k, v in obs.items()}, 352, "synthetic, stride 352")
    ref.check_bf16_against_torch(ref.expected_bits("extractor", obs))
    ref.check_bf16_against_torch(ref.expected_bits("produced", obs))
    # bytes of a record outside the observation fields (reward, action, terminated, padding) are in no layout
    rows = ref.pack_records(obs, 384)[:256].copy()
    noise = rows.copy()
    covered = np.zeros(384, bool)
    from balatro_gym_amd import _native as nat
    for k in OBS_KEYS:
        dt, shape = nat.OBS_SPEC[k]
        covered[nat.ROW_OFFSETS[k]:nat.ROW_OFFSETS[k] + np.dtype(dt).itemsize * int(np.prod(shape, dtype=np.int64))] = True
    noise[:, ~covered] = 0xa5
    for layout in ref.LAYOUTS:
        assert np.array_equal(encoder(noise, layout, False), encoder(rows, layout, False))


def test_enc_columns_match_the_header_tables(encoder):
    """_native.ENC_COLUMNS / ENC_COLS against the X-macro lists of csrc/bg_encode.h (printed by the host build), the BG_ROW_* offsets of the public header
    and -- when the library is built -- bg_encode_cols."""
    from balatro_gym_amd import _native as nat, build
    from balatro_gym_amd.sb3_adapter import _NEVER_PRODUCED
    hdr = open(HEADER).read()
    row_off = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define BG_ROW_([A-Z_]+) (\d+)", hdr)}
    enc_def = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (BG_ENC_[A-Z0-9]+) (\d+)", hdr)}
    assert (enc_def["BG_ENC_PRODUCED"], enc_def["BG_ENC_FIXED"], enc_def["BG_ENC_EXTRACTOR"]) == (nat.ENC_PRODUCED, nat.ENC_FIXED, nat.ENC_EXTRACTOR)
    assert (enc_def["BG_ENC_F32"], enc_def["BG_ENC_BF16"]) == (nat.ENC_F32, nat.ENC_BF16)
    lines = [l.split() for l in subprocess.check_output([encoder.exe, "table"], text=True).splitlines()]
    types_ = {0: "int8", 1: "int16", 2: "int32", 3: "int64", 4: "float32"}
    produced = [(l[1], int(l[2]), types_[int(l[3])], int(l[4])) for l in lines if l[0] == "produced"]
    zero = [(l[1], int(l[2])) for l in lines if l[0] == "zero"]
    state = [(l[1], int(l[2]), types_[int(l[3])], int(l[4]), float(l[5])) for l in lines if l[0] == "state"]
    cols = [int(x) for x in next(l for l in lines if l[0] == "cols")[1:]]
    assert cols == [153, 628, 447] == [nat.ENC_COLS[i] for i in range(3)]
    # the produced keys: reference order, the record's offsets and dtypes
    assert [p[0] for p in produced] == nat.OBS_KEYS
    for name, off, dt, n in produced:
        assert off == row_off[name] == nat.ROW_OFFSETS[name] and dt == nat.OBS_SPEC[name][0] and n == int(np.prod(nat.OBS_SPEC[name][1], dtype=np.int64)), name
    assert zero == nat.ENC_ZERO_KEYS == ref.ZERO_KEYS
    assert [(k, int(np.prod(s, dtype=np.int64))) for k, (_, s) in _NEVER_PRODUCED.items()] == zero
    for name, off, dt, n, dv in state:
        assert off == row_off[name] and dt == nat.OBS_SPEC[name][0], name
    assert [(s[0], s[0], s[3], s[4] or None) for s in state] == [tuple(p) for p in nat.ENC_EXTRACTOR_PARTS[2:]]
    # ENC_COLUMNS = the running sums of those lists
    def run(parts):
        out, c = [], 0
        for name, n in parts:
            out.append((name, c, n))
            c += n
        return out
    pk = [(p[0], p[3]) for p in produced]
    assert nat.ENC_COLUMNS[nat.ENC_PRODUCED] == run(pk)
    assert nat.ENC_COLUMNS[nat.ENC_FIXED] == run(pk + zero)
    assert nat.ENC_COLUMNS[nat.ENC_EXTRACTOR] == run([("hand_one_hot", 416), ("joker_ids", 10)] + [(s[0], s[3]) for s in state])
    # the per-column descriptors the kernel indexes: every column reads inside its key's bytes of the record
    col = {(int(l[1]), int(l[2])): tuple(int(x) for x in l[3:]) for l in lines if l[0] == "col"}
    assert len(col) == 153 + 628 + 447
    for layout in (nat.ENC_PRODUCED, nat.ENC_FIXED):
        for name, first, n in nat.ENC_COLUMNS[layout]:
            for i in range(n):
                off, ty, op, par = col[(layout, first + i)]
                if name in nat.ROW_OFFSETS and first < 153:
                    assert (off, types_[ty], op) == (nat.ROW_OFFSETS[name] + i * np.dtype(nat.OBS_SPEC[name][0]).itemsize, nat.OBS_SPEC[name][0], 0), (name, i)
                else:
                    assert op == 3, (name, i)
    for c in range(416):
        assert col[(2, c)] == (nat.ROW_OFFSETS["hand"] + c // 52, 0, 2, c % 52)
    for c in range(10):
        assert col[(2, 416 + c)] == (nat.ROW_OFFSETS["joker_ids"] + 2 * c, 1, 0, 0)
    if os.path.exists(build.LIB):
        L = C.CDLL(build.LIB)
        assert [L.bg_encode_cols(i) for i in range(3)] == cols and L.bg_encode_cols(3) == -1 and L.bg_encode_cols(-1) == -1


def test_header_declares_and_library_exports_encode():
    from balatro_gym_amd import _native as nat, build
    hdr = open(HEADER).read()
    assert re.search(r"\bint\s+bg_encode_cols\s*\(\s*int\s+layout\s*\)\s*;", hdr)
    m = re.search(r"\bint\s+bg_encode_rows\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/balatro_mi355x.h does not declare bg_encode_rows"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 9 and "const uint8_t*" in params[0] and "uint64_t" in params[1] and "int64_t" in params[2] and "float*" in params[7], params
    doc = hdr[:hdr.index("#define BG_ENC_PRODUCED")].rsplit("/*", 1)[1]
    for cite in ("train_balatro_agent.py:84-119", "train_balatro_fixed.py:125-207", "hpc_train.py:77", "bg_encode_cols", "32 inputs"):
        assert cite in doc, cite
    assert "bg_encode_cols" in nat.EXPORTS and "bg_encode_rows" in nat.EXPORTS
    assert os.path.join(CSRC, "bg_encode.h") in build.DEPS
    if not os.path.exists(build.LIB):
        pytest.skip("library not built")
    L = C.CDLL(build.LIB)
    assert hasattr(L, "bg_encode_cols") and hasattr(L, "bg_encode_rows")


def test_wrappers_refuse_bad_arguments_before_the_library():
    """encode_rows / RowBuffers.encode / BalatroVecEnv.features on CPU stand-ins: every bad argument is a ValueError raised before anything is loaded."""
    import torch
    from balatro_gym_amd import encode_rows
    from balatro_gym_amd.sb3_adapter import BalatroSB3VecEnv
    from balatro_gym_amd.vec_env import BalatroVecEnv, RowBuffers
    rows = torch.zeros((3, 5, 384), dtype=torch.uint8)
    with pytest.raises(ValueError, match="layout must be one of"):
        encode_rows(rows, "dict")
    with pytest.raises(ValueError, match="float32 or torch.bfloat16"):
        encode_rows(rows, "fixed", torch.float16)
    for bad in (rows.to(torch.int8), rows[:, :, :352][:, ::2], torch.zeros((), dtype=torch.uint8), "rows"):
        with pytest.raises(ValueError, match="contiguous uint8 tensor"):
            encode_rows(bad, "fixed")
    for stride in (336, 360):
        with pytest.raises(ValueError, match="record stride"):
            encode_rows(torch.zeros((4, stride), dtype=torch.uint8), "produced")
    for out in (torch.zeros((3, 5, 152)), torch.zeros((3, 4, 153)), torch.zeros((15, 153)), torch.zeros((3, 5, 153), dtype=torch.bfloat16)):
        with pytest.raises(ValueError, match="out must"):
            encode_rows(rows, "produced", out=out)
    with pytest.raises(ValueError, match="dense over its row pitch"):
        encode_rows(rows, "produced", out=torch.zeros((3, 5, 306))[:, :, ::2])
    with pytest.raises(ValueError, match="dense over its row pitch"):
        encode_rows(rows, "produced", out=torch.zeros((3, 6, 160))[:, :5])
    # a column slice of a wider matrix is fine as far as the argument checks go: what is left is that there is no CPU path
    for out in (None, torch.zeros((3, 5, 153)), torch.zeros((3, 5, 200))[:, :, 8:170]):
        with pytest.raises(ValueError, match="device tensor"):
            encode_rows(rows, "produced", out=out)
    with pytest.raises(ValueError, match="device tensor"):
        RowBuffers(5, torch.device("cpu"), steps=3, row_stride=384).encode("extractor", torch.bfloat16)
    with pytest.raises(ValueError, match="obs_layout='rows'"):
        BalatroVecEnv.features(types.SimpleNamespace(_rowbuf=None), "fixed")
    with pytest.raises(ValueError, match="features must be None or one of"):
        BalatroSB3VecEnv(4, features="dict")
