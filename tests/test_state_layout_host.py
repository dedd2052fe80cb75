"""The per-env array layout of balatro_gym_amd/csrc/bg_device.h (bg_hot_at / bg_cold_at / bg_deck_at / bg_tmpl_at / bg_ndeck_at and the chunk
counts the arrays are allocated with) -- on the CPU.  The layout block of the header is plain C++: its very text is compiled with g++ into a
stand-alone program that, for one (N, KD), lays every array out in a heap block of exactly the allocated size and prints the byte offset of every
(env, chunk) and (env, slot, chunk).  The test holds them to what the kernels rely on: 16-byte pieces inside the allocation that never overlap,
every live deck and every ring slot in one aligned 64-byte sector, an env's ring contiguous.  (`hot`, `cold` and the template ship structure-of-arrays:
one 128-byte line per env was measured and did not gain, so there is no per-env block of theirs to hold to a line boundary.)  The program
also writes a tag through every address and reads all of them back (two addresses that met would lose one), over blocks filled with a poison
pattern; it runs a second time under AddressSanitizer + UBSan, where a piece that left its allocation would stop it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")

NS, KDS = (1, 70, 200), (1, 2, 248)
NHOT, NDECK, NCOLD, NTMPL = 8, 4, 7, 2


def _between(text, a, b):
    i = text.index(a)
    return text[i:text.index(b, i)]


def _source():
    dev = open(os.path.join(CSRC, "bg_device.h")).read()
    consts = _between(dev, "#define BG_NHOT ", "#define BG_MT_N")
    block = _between(dev, "// ---- per-env array layout", "// ---- end of the per-env array layout")
    return """#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#define BG_HD static inline
""" + consts + block + """
struct Piece { uint64_t tag[2]; };   // 16 bytes
static int fail(const char* what) { fprintf(stderr, "layout_host: %s\\n", what); return 1; }
// one array: a block of exactly `chunks` pieces (redzones on both sides under ASan), poisoned; every address written, then every address read back
template <class At>
static int run(const char* name, size_t chunks, size_t n_addr, int poison, At at) {
  Piece* base = nullptr;   // (hipMalloc aligns to 256 bytes and more)
  if (posix_memalign((void**)&base, 128, chunks * sizeof(Piece)) != 0 || !base) return fail("alloc");
  memset(base, poison, chunks * sizeof(Piece));
  for (size_t i = 0; i < n_addr; i++) { const size_t c = at(i); base[c].tag[0] = i; base[c].tag[1] = ~(uint64_t)i; }
  for (size_t i = 0; i < n_addr; i++) { const size_t c = at(i); if (base[c].tag[0] != i || base[c].tag[1] != ~(uint64_t)i) { free(base); return fail(name); } }
  // the report: name, allocated bytes, the block's address modulo 128, then the byte offset of every address in order
  printf("%s %zu %zu", name, chunks * sizeof(Piece), (size_t)((uintptr_t)base % 128));
  for (size_t i = 0; i < n_addr; i++) printf(" %zu", at(i) * sizeof(Piece));
  printf("\\n");
  free(base);
  return 0;
}
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const size_t N = strtoul(argv[1], 0, 0), KD = strtoul(argv[2], 0, 0);
  const int poison = (int)strtoul(argv[3], 0, 0);
  int rc = 0;
  rc |= run("hot", bg_hot_chunks(N), N * BG_NHOT, poison, [&](size_t i) { return bg_hot_at(N, i / BG_NHOT, (int)(i % BG_NHOT)); });
  rc |= run("deck", bg_deck_chunks(N), N * BG_NDECK, poison, [&](size_t i) { return bg_deck_at(N, i / BG_NDECK, (int)(i % BG_NDECK)); });
  rc |= run("cold", bg_cold_chunks(N), N * BG_NCOLD, poison, [&](size_t i) { return bg_cold_at(N, i / BG_NCOLD, (int)(i % BG_NCOLD)); });
  rc |= run("tmpl", bg_tmpl_chunks(N), N * BG_NTMPL, poison, [&](size_t i) { return bg_tmpl_at(N, i / BG_NTMPL, (int)(i % BG_NTMPL)); });
  rc |= run("ndeck", bg_ndeck_chunks(N, KD), N * KD * BG_NDECK, poison,
            [&](size_t i) { return bg_ndeck_at(N, KD, i / (KD * BG_NDECK), (i / BG_NDECK) % KD, (int)(i % BG_NDECK)); });
  return rc;
}
"""


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("state_layout_host")
    (d / "layout_host.cpp").write_text(_source())
    return d


def _build(d, name, extra):
    exe = d / name
    subprocess.check_call(["g++", "-O1", "-std=c++17"] + extra + ["-o", str(exe), str(d / "layout_host.cpp")])
    return str(exe)


def _report(exe, n, kd, poison):
    out = subprocess.check_output([exe, str(n), str(kd), str(poison)]).decode()
    rep = {}
    for line in out.splitlines():
        f = line.split()
        rep[f[0]] = (int(f[1]), int(f[2]), np.array(f[3:], dtype=np.int64))
    assert set(rep) == {"hot", "deck", "cold", "tmpl", "ndeck"}
    return rep


def _check(rep, n, kd):
    shapes = {"hot": (n, NHOT), "deck": (n, NDECK), "cold": (n, NCOLD), "tmpl": (n, NTMPL), "ndeck": (n * kd, NDECK)}   # (blocks, chunks per block)
    for name, (nbytes, base_mod, off) in rep.items():
        ctx = f"{name} at N={n} KD={kd}"
        blocks, per = shapes[name]
        assert base_mod == 0, ctx
        assert off.size == blocks * per, ctx
        assert (off % 16 == 0).all(), f"{ctx}: a piece off its 16-byte boundary"
        assert off.min() >= 0 and off.max() + 16 <= nbytes, f"{ctx}: a piece outside the allocation of {nbytes} bytes"
        assert np.unique(off).size == off.size, f"{ctx}: two pieces at one address"
        if name in ("deck", "ndeck"):
            # what the sparse lanes of the engine and of the deck kernel rely on: a deck's four chunks are back to back, in chunk order, in one
            # aligned 64-byte sector (the live deck, every ring slot: two consecutive slots share a line)
            blk = off.reshape(blocks, per)
            assert (np.diff(blk, axis=1) == 16).all(), f"{ctx}: a deck's chunks are not back to back"
            assert (blk[:, 0] % 64 == 0).all(), f"{ctx}: a deck off its 64-byte sector"
    # an env's ring is contiguous: slot s + 1 follows slot s
    ring = rep["ndeck"][2].reshape(n, kd, NDECK)[:, :, 0]
    if kd > 1:
        assert (np.diff(ring, axis=1) == 64).all(), f"ring slots at N={n} KD={kd} are not consecutive sectors"


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kd", KDS)
def test_every_address_is_aligned_inside_and_distinct(workdir, n, kd):
    exe = _build(workdir, "layout_host", [])
    _check(_report(exe, n, kd, 0xA5), n, kd)


def test_layout_under_sanitizers_over_poisoned_blocks(workdir):
    # (the sanitizer runtimes are linked INTO the program: it runs as it is, whatever else the process environment loads)
    exe = _build(workdir, "layout_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                                              "-static-libasan", "-static-libubsan"])
    for n, kd, poison in ((200, 248, 0xFF), (70, 2, 0x3C), (1, 1, 0x00)):
        _check(_report(exe, n, kd, poison), n, kd)
