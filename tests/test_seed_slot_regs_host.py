"""The register-only slot seeding against CPython's `random` -- on the CPU, over a few thousand keys.  `bg_mt_seed_impl<true>`
(balatro_gym_amd/csrc/bg_lib.hip) builds a shop-stream ring slot without ever reading the slot it writes: the near words S[k], S[k+1] come from a
delayed second copy of the two seeding recurrences that meets S[k+397] in registers.  As in test_seed_slot_host.py the very text the GPU runs is
compiled with g++ (its device-only store flavour sits behind a compile-time switch whose host side is plain C++) and the WHOLE 64-word slot is held
to CPython: 56 `getrandbits(32)` words of `random.Random(key)`, the six packed top-byte words, the key, a zero.  The full-state mode
(`bg_mt_seed_impl<false>`: bg_seed_kernel, the operators) runs on the same keys against `getstate()`.  The slot mode runs a second time as a
stand-alone program under AddressSanitizer + UBSan, on heap blocks of exactly the slot's size that are filled with a poison pattern before every
call -- with two different patterns: a function that looked at `p` before writing it could not give the same slots for both."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")

EDGE_KEYS = [0, 1, 7, 42, 382, 12345, 2 ** 31 - 1, 2 ** 31, 4000000000, 2 ** 32 - 1, 1650520237]   # test_seed_slot_host.KEYS (0 and 2**32 - 1 among them)
_rng = random.Random(20261019)
KEYS = EDGE_KEYS + [_rng.getrandbits(32) for _ in range(2048)] + [_rng.getrandbits(31) for _ in range(256)]   # (shop seeds are < 2**31)
SLOT_WORDS, STATE_WORDS = 64, 624


def _between(text, a, b):
    i = text.index(a)
    return text[i:text.index(b, i)]


def _source():
    lib = open(os.path.join(CSRC, "bg_lib.hip")).read()
    dev = open(os.path.join(CSRC, "bg_device.h")).read()
    body = _between(lib, "struct alignas(64) BgG16", "__device__ void bg_mt_seed(uint32_t* __restrict__ p")
    temper = _between(dev, "__device__ __forceinline__ uint32_t bg_temper", "// One word / one random() of a lazy MT19937 stream")
    defs = _between(dev, "#define BG_SW_T ", "#define BG_BF_SHOP_OVF")
    return """#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#define __device__
#define __forceinline__ inline
#define BG_MT_N 624
#define BG_MT_M 397
struct uint4 { uint32_t x, y, z, w; }; struct uint2 { uint32_t x, y; };
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return uint4{a, b, c, d}; }
static inline uint2 make_uint2(uint32_t a, uint32_t b) { return uint2{a, b}; }
""" + defs + temper + body + """
// seed_host <s|f> <file of uint32 keys> <poison byte>: every key's slot / state, raw uint32, on stdout.  The block is exactly as large as
// the mode writes, fresh from the heap for every key (redzones on both sides under ASan), and poisoned before the call.
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const bool slot = argv[1][0] == 's';
  const size_t words = slot ? BG_SLOT_WORDS : 624;
  FILE* f = fopen(argv[2], "rb");
  if (!f) return 3;
  const int poison = (int)strtoul(argv[3], 0, 0);
  uint32_t key;
  while (fread(&key, 4, 1, f) == 1) {
    uint32_t* p = (uint32_t*)aligned_alloc(64, words * 4);
    if (!p) return 4;
    memset(p, poison, words * 4);
    if (slot) bg_mt_seed_impl<true>(p, key); else bg_mt_seed_impl<false>(p, key);
    if (fwrite(p, 4, words, stdout) != words) return 5;
    free(p);
  }
  fclose(f);
  return 0;
}
"""


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("seed_regs_host")
    (d / "seed_host.cpp").write_text(_source())
    np.array(KEYS, dtype="<u4").tofile(str(d / "keys.bin"))
    return d


def _build(d, name, extra):
    exe = d / name
    subprocess.check_call(["g++", "-O1", "-std=c++17"] + extra + ["-o", str(exe), str(d / "seed_host.cpp")])
    return str(exe)


def _run(exe, d, mode, poison, words):
    out = subprocess.check_output([exe, mode, str(d / "keys.bin"), str(poison)])
    got = np.frombuffer(out, dtype="<u4")
    assert got.size == len(KEYS) * words
    return got.reshape(len(KEYS), words)


@pytest.fixture(scope="module")
def want_slots():
    want = np.zeros((len(KEYS), SLOT_WORDS), dtype=np.uint32)
    for i, key in enumerate(KEYS):
        r = random.Random(key)
        words = [r.getrandbits(32) for _ in range(56)]
        pk = [0] * 6
        for k in range(24):
            pk[k >> 2] |= (words[k] >> 24) << (8 * (k & 3))
        want[i] = words + pk + [key, 0]
    want.setflags(write=False)
    return want


def _assert_rows(got, want, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    if bad.size:
        i = int(bad[0]); w = int(np.nonzero(got[i] != want[i])[0][0])
        raise AssertionError(f"{what}: {bad.size} of {len(KEYS)} keys differ; first key {KEYS[i]} at word {w}: got {int(got[i, w])}, want {int(want[i, w])}")


def test_keys_cover_the_edges():
    assert len(KEYS) >= 2000 and set(EDGE_KEYS) <= set(KEYS) and 0 in KEYS and 2 ** 32 - 1 in KEYS


def test_whole_slot_is_cpythons(workdir, want_slots):
    exe = _build(workdir, "seed_host", [])
    _assert_rows(_run(exe, workdir, "s", 0x00, SLOT_WORDS), want_slots, "slot")
    _assert_rows(_run(exe, workdir, "s", 0xA5, SLOT_WORDS), want_slots, "slot over poison 0xa5")


def test_full_state_is_cpythons(workdir):
    exe = _build(workdir, "seed_host", [])
    want = np.array([random.Random(key).getstate()[1][:624] for key in KEYS], dtype=np.uint32)   # what init_by_array([key]) leaves, before the first twist
    _assert_rows(_run(exe, workdir, "f", 0x5A, STATE_WORDS), want, "full state")


def test_slot_mode_under_sanitizers_never_depends_on_the_slot(workdir, want_slots):
    # (the sanitizer runtimes are linked INTO the program: it runs as it is, whatever else the process environment loads)
    exe = _build(workdir, "seed_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                                            "-static-libasan", "-static-libubsan"])
    for poison in (0xFF, 0x3C):
        _assert_rows(_run(exe, workdir, "s", poison, SLOT_WORDS), want_slots, f"slot under ASan/UBSan over poison {poison:#x}")
