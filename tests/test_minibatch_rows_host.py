"""bg_encode_rows_ex on the CPU (no GPU): the header's declaration and the library's export, the index resolution of csrc/bg_encode.h compiled with g++
(the very function phase 1 of the gathered kernels calls), the argument checks of the Python wrappers on CPU stand-ins, and `RowBuffers.minibatches`
-- SB3's `RolloutBuffer.get` permutation as int32 tensors."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

_PROGRAM = r"""
#define BG_ENC_HOST
#include <stdio.h>
#include <stdlib.h>
#include "balatro_mi355x.h"
#include "bg_encode.h"
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const long long store_rows = atoll(argv[1]);
  for (int i = 2; i < argc; i++) printf("%lld\n", (long long)bg_enc_source_row((int32_t)atoll(argv[i]), (int64_t)store_rows));
  return 0;
}
"""


def test_header_declares_and_library_exports_encode_rows_ex():
    from balatro_gym_amd import _native as nat, build
    hdr = open(HEADER).read()
    m = re.search(r"\bint\s+bg_encode_rows_ex\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/balatro_mi355x.h does not declare bg_encode_rows_ex"
    params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 15, params
    for i, ty in ((0, "const uint8_t*"), (1, "uint64_t"), (2, "int64_t"), (3, "const int32_t*"), (4, "int64_t"), (5, "int"), (6, "int"), (7, "const double*"),
                  (8, "const double*"), (9, "double"), (10, "double"), (11, "void*"), (12, "uint64_t"), (13, "float*"), (14, "void*")):
        assert params[i].startswith(ty), (i, params[i])
    doc = hdr[:m.start()].rsplit("/*", 1)[1]
    for word in ("RolloutBuffer.get", "bg_ppo_loss", "store_rows", "+0.0", "bg_norm_obs_rows(update = 0)", "BG_E_ARG", "Out of scope", "int64 indices", "bg_norm_reward_rows"):
        assert word in doc, word
    assert "bg_encode_rows_ex" in nat.EXPORTS
    if not os.path.exists(build.LIB):
        pytest.skip("library not built")
    L = C.CDLL(build.LIB)
    assert hasattr(L, "bg_encode_rows_ex")


def test_index_resolution_host_build(tmp_path):
    """bg_enc_source_row: the index value itself inside [0, store_rows), -1 ("none") outside -- at both ends of the store and of int32."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    src, exe = tmp_path / "source_row.cpp", tmp_path / "source_row"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    for store_rows in (200, 1, 0, INT32_MAX, 2 ** 40):
        values = [-1, 0, store_rows - 1, store_rows, INT32_MIN, INT32_MAX]
        values = [v for v in values if INT32_MIN <= v <= INT32_MAX]
        got = [int(x) for x in subprocess.check_output([str(exe), str(store_rows)] + [str(v) for v in values], text=True).split()]
        assert got == [v if 0 <= v < store_rows else -1 for v in values], (store_rows, values, got)


def test_wrappers_refuse_bad_arguments_before_the_library():
    """encode_rows(index=, norm=) / RowBuffers.encode / normalize / RowNormalizer.normalize_obs on CPU stand-ins: every bad argument is a ValueError raised
    before anything is loaded; what is left of a good call is that there is no CPU path."""
    import torch
    from balatro_gym_amd import RowNormalizer, encode_rows
    from balatro_gym_amd.vec_env import RowBuffers
    K, N = 3, 5
    rows = torch.zeros((K, N, 384), dtype=torch.uint8)
    idx = torch.tensor([0, 14, 7, 7], dtype=torch.int32)
    cpu = torch.device("cpu")
    nm = RowNormalizer(N, cpu)
    rb = RowBuffers(N, cpu, steps=K, row_stride=384)
    # the index: ppo_loss' rule and ppo_loss' message
    for bad in (idx.long(), idx.float(), idx.view(2, 2), torch.zeros((), dtype=torch.int32), torch.zeros(8, dtype=torch.int32)[::2], [0, 1], idx.to("meta")):
        for call in (lambda: encode_rows(rows, "produced", index=bad), lambda: rb.encode(index=bad), lambda: rb.normalize(nm, index=bad),
                     lambda: nm.normalize_obs(rows, index=bad), lambda: encode_rows(rows, "fixed", index=bad, norm=nm)):
            with pytest.raises(ValueError, match=r"index must be a contiguous torch.int32 tensor of shape \[m\] on cpu"):
                call()
    # the same helper serves ppo_loss: its message is the one it had
    from balatro_gym_amd.vec_env import ppo_loss
    z = torch.zeros(4)
    with pytest.raises(ValueError, match=r"index must be a contiguous torch.int32 tensor of shape \[4\] on cpu"):
        ppo_loss(torch.zeros((4, 60)), torch.zeros(4, dtype=torch.int32), z, z, index=idx.long())
    # statistics: not with the extractor's tensors, not from another device, not updated over a minibatch
    with pytest.raises(ValueError, match="layout must be 'produced' or 'fixed'"):
        encode_rows(rows, "extractor", norm=nm)
    with pytest.raises(ValueError, match="layout must be 'produced' or 'fixed'"):
        encode_rows(rows, "extractor", index=idx, norm=nm)
    with pytest.raises(ValueError, match="layout must be 'produced' or 'fixed'"):
        nm.normalize_obs(rows, "extractor", index=idx)
    with pytest.raises(ValueError, match="norm must be a RowNormalizer"):
        encode_rows(rows, "produced", norm=object())
    with pytest.raises(ValueError, match="norm_obs=False"):
        encode_rows(rows, "produced", index=idx, norm=RowNormalizer(N, cpu, norm_obs=False))
    with pytest.raises(ValueError, match="update=True with an index"):
        nm.normalize_obs(rows, index=idx, update=True)
    with pytest.raises(ValueError, match="update=True with an index"):
        nm.normalize_obs(rows, index=idx.long(), update=True)   # refused before the index is even looked at
    # out: [m, >= D] of the right dtype
    for out in (torch.zeros((3, 153)), torch.zeros((5, 153)), torch.zeros((4, 152)), torch.zeros((K, N, 153)), torch.zeros((4, 153), dtype=torch.bfloat16), torch.zeros(4 * 153)):
        with pytest.raises(ValueError, match="out must"):
            encode_rows(rows, "produced", out=out, index=idx)
        with pytest.raises(ValueError, match="out must"):
            nm.normalize_obs(rows, out=out, index=idx)
    with pytest.raises(ValueError, match="dense over its row pitch"):
        encode_rows(rows, "produced", out=torch.zeros((4, 306))[:, ::2], index=idx)
    for bad_rows in (rows.to(torch.int8), rows[:, :, :352][:, ::2], "rows"):
        with pytest.raises(ValueError, match="contiguous uint8 tensor"):
            encode_rows(bad_rows, "fixed", index=idx)
    with pytest.raises(ValueError, match="record stride"):
        encode_rows(torch.zeros((4, 360), dtype=torch.uint8), "produced", index=idx)
    with pytest.raises(ValueError, match="layout must be one of"):
        encode_rows(rows, "dict", index=idx)
    with pytest.raises(ValueError, match="float32 or torch.bfloat16"):
        encode_rows(rows, "fixed", torch.float16, index=idx)
    # good arguments: only the device is missing
    for call in (lambda: encode_rows(rows, "extractor", index=idx), lambda: encode_rows(rows.view(K * N, 384), "fixed", torch.bfloat16, index=idx, norm=nm),
                 lambda: encode_rows(rows, "produced", norm=nm), lambda: encode_rows(rows, "produced", out=torch.zeros((4, 160)), index=idx),
                 lambda: rb.encode("fixed", index=idx), lambda: rb.normalize(nm, index=idx), lambda: nm.normalize_obs(rows, index=idx, update=False),
                 lambda: nm.normalize_obs(rows, index=idx)):
        with pytest.raises(ValueError, match="device tensor"):
            call()


def test_minibatches_are_one_permutation_in_int32():
    """Consecutive slices of ONE randperm(K * N): together a permutation of 0 .. K*N-1, reproducible from the generator's seed, the last one shorter
    (or, with drop_last, left out) when K * N is no multiple of the batch size, int32 on the records' device."""
    import torch
    from balatro_gym_amd.vec_env import RowBuffers
    K, N = 7, 13   # 91 records
    rb = RowBuffers(N, torch.device("cpu"), steps=K, row_stride=384)

    def batches(bs, seed, **kw):
        return list(rb.minibatches(bs, generator=torch.Generator().manual_seed(seed), **kw))
    for bs, sizes in ((32, [32, 32, 27]), (13, [13] * 7), (91, [91]), (200, [91]), (1, [1] * 91)):
        got = batches(bs, 5)
        assert [len(b) for b in got] == sizes, bs
        for b in got:
            assert b.dtype == torch.int32 and b.dim() == 1 and b.is_contiguous() and b.device == rb.rows.device
        whole = torch.cat(got)
        assert torch.equal(whole.sort().values, torch.arange(K * N, dtype=torch.int32)), bs
        assert torch.equal(whole.long(), torch.randperm(K * N, generator=torch.Generator().manual_seed(5))), "slices of ONE torch.randperm"
        again = batches(bs, 5)
        assert all(torch.equal(a, b) for a, b in zip(got, again))
    assert not torch.equal(torch.cat(batches(32, 5)), torch.cat(batches(32, 6)))
    assert [len(b) for b in batches(32, 5, drop_last=True)] == [32, 32]
    assert [len(b) for b in batches(13, 5, drop_last=True)] == [13] * 7
    assert batches(200, 5, drop_last=True) == []
    assert all(torch.equal(a, b) for a, b in zip(batches(32, 5, drop_last=True), batches(32, 5)))
    # without a generator: torch's global one
    torch.manual_seed(11)
    a = torch.cat(list(rb.minibatches(40)))
    torch.manual_seed(11)
    assert torch.equal(a, torch.cat(list(rb.minibatches(40)))) and torch.equal(a.sort().values, torch.arange(K * N, dtype=torch.int32))
    with pytest.raises(ValueError, match="batch_size must be >= 1"):
        list(rb.minibatches(0))
