"""bg_get_states / bg_set_states / bg_copy_states on the CPU (no GPU): the piece plan, the unit addresses and the index checks of csrc/bg_snapshot.h
compiled with g++ under BG_SNAP_HOST, and a scalar model of the kernel's loop over (pair, tile, lane, unit) -- restated here from the header's
description -- run on host memory that is laid out with the real accessors of bg_device.h (bg_hot_at, bg_ndeck_at, ...).  Held against a restatement
of what bg_get_state / bg_set_state do, one 2-D copy per slice: blob bytes equal, header included; set after get is the identity; poisoned padding
and poisoned other envs untouched; the producer word in both buffers; a copy between two handles' arrays equals get + set; the blob size is the
formula tests/test_state_layout_gpu.py asserts.  Then every refused index list and the accepted edge cases."""
import os
import shutil
import subprocess

import pytest

from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "balatro_gym_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "balatro_mi355x.h")


def _between(text, a, b):
    i = text.index(a)
    return text[i:text.index(b, i)]


def _source():
    dev = open(os.path.join(CSRC, "bg_device.h")).read()
    consts = _between(dev, "#define BG_NHOT ", "#define BG_MT_N")
    block = _between(dev, "// ---- per-env array layout", "// ---- end of the per-env array layout")
    return r"""#define BG_SNAP_HOST
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#define BG_HD static inline
""" + consts + block + r"""
#include "bg_snapshot.h"
#define MTS 640
#define SLOT_WORDS 64
#define SSEED 128
#define NCST 7
typedef std::vector<uint8_t> Bytes;
static int bad = 0;
static void fail(const char* what, long a = 0, long b = 0) { if (bad++ < 8) printf("FAIL %s %ld %ld\n", what, a, b); }

// one handle's arrays: the slices of bg_slices (bg_lib.hip), restated with the accessors; every array in a block of exactly its size
struct Arrays {
  size_t N, KG, KS, KD; bool cards;
  std::vector<Bytes> mem;   // hot deck cold tmpl ndeck gblk sblk sovf deckmt shopgenmt sseed smeta prod [cstate ctmpl cardmt sealmt], then prod_other
  BgSnapTable t;
  int prod_slice;
  uint8_t* al(size_t bytes, int fill) { mem.push_back(Bytes(bytes + 16, (uint8_t)fill)); uint8_t* p = mem.back().data(); return p + ((16 - ((uintptr_t)p & 15)) & 15); }
  Arrays(size_t n, size_t kg, size_t ks, size_t kd, bool c, int fill, unsigned seed) : N(n), KG(kg), KS(ks), KD(kd), cards(c) {
    mem.reserve(32);
    int j = 0;
    auto chunked = [&](size_t chunks, size_t rows, size_t env_stride, size_t row_stride) { t.s[j++] = {al(chunks * 16, fill), 16 * env_stride, 16 * row_stride, 16u, (uint32_t)rows}; };
    auto flat = [&](size_t bytes) { t.s[j++] = {al(bytes * N, fill), bytes, bytes, (uint32_t)bytes, 1u}; };
    chunked(bg_hot_chunks(N), BG_NHOT, bg_hot_at(N, 1, 0) - bg_hot_at(N, 0, 0), bg_hot_at(N, 0, 1) - bg_hot_at(N, 0, 0));
    chunked(bg_deck_chunks(N), BG_NDECK, bg_deck_at(N, 1, 0) - bg_deck_at(N, 0, 0), bg_deck_at(N, 0, 1) - bg_deck_at(N, 0, 0));
    chunked(bg_cold_chunks(N), BG_NCOLD, bg_cold_at(N, 1, 0) - bg_cold_at(N, 0, 0), bg_cold_at(N, 0, 1) - bg_cold_at(N, 0, 0));
    chunked(bg_tmpl_chunks(N), BG_NTMPL, bg_tmpl_at(N, 1, 0) - bg_tmpl_at(N, 0, 0), bg_tmpl_at(N, 0, 1) - bg_tmpl_at(N, 0, 0));
    chunked(bg_ndeck_chunks(N, KD), KD * BG_NDECK, bg_ndeck_at(N, KD, 1, 0, 0) - bg_ndeck_at(N, KD, 0, 0, 0), bg_ndeck_at(N, KD, 0, 0, 1) - bg_ndeck_at(N, KD, 0, 0, 0));
    flat(KG * MTS * 4); flat(KS * SLOT_WORDS * 4); flat(MTS * 4); flat(MTS * 4); flat(MTS * 4); flat(SSEED * 4); flat(4);
    prod_slice = j; flat(4);
    if (cards) { chunked(NCST * N, NCST, 1, N); chunked(NCST * N, NCST, 1, N); flat(MTS * 4); flat(MTS * 4); }
    t.n = j;
    if (seed) for (int k = 0; k < j; k++) { uint8_t* p = t.s[k].base; const size_t nb = mem[k].size() - 16; for (size_t i = 0; i < nb; i++) { seed = seed * 1664525u + 1013904223u; p[i] = (uint8_t)(seed >> 24); } }
    other = (uint32_t*)al(4 * N, fill);
  }
  uint32_t* other;
  bool same_bytes(const Arrays& o) const { for (size_t k = 0; k < mem.size(); k++) if (mem[k] != o.mem[k]) return false; return true; }
};
static const uint32_t HDR[4] = {0x42474d58u, 7u, 0, 0};

// the restatement: hipMemcpy2D(dst, dpitch, src, spitch, width, height) per slice, as bg_get_state / bg_set_state call it
static void copy2d(uint8_t* d, size_t dp, const uint8_t* s, size_t sp, size_t w, size_t h) { for (size_t r = 0; r < h; r++) memcpy(d + r * dp, s + r * sp, w); }
static void ref_get(const Arrays& A, size_t env, uint8_t* out, const uint32_t* hdr) {
  memcpy(out, hdr, 16); out += 16;
  for (int k = 0; k < A.t.n; k++) { const BgSnapSlice& s = A.t.s[k]; copy2d(out, s.elem, s.base + env * s.env_stride, s.row_stride, s.elem, s.rows); out += (size_t)s.rows * s.elem; }
}
static void ref_set(Arrays& A, size_t env, const uint8_t* in) {
  in += 16;
  for (int k = 0; k < A.t.n; k++) { const BgSnapSlice& s = A.t.s[k]; copy2d(s.base + env * s.env_stride, s.row_stride, in, s.elem, s.elem, s.rows); in += (size_t)s.rows * s.elem; }
  memcpy(&A.other[env], A.t.s[A.prod_slice].base + 4 * env, 4);
}

// the kernel's loop, scalar: m * tiles workgroups of BG_SNAP_BLOCK lanes, BG_SNAP_PER_LANE units per lane, unit `units` = the header
struct Args { BgSnapTable src, dst; BgSnapPlan plan; const int32_t* src_idx; const int32_t* dst_idx; uint8_t* hdr_base; uint64_t hdr_stride; const uint32_t* hdr; int prod_slice; uint32_t* prod_other; };
static int model(Args& a, int m) {
  if (bg_snap_plan(a.src, a.dst, a.plan)) return 1;
  const uint32_t tiles = (a.plan.units + 1u + BG_SNAP_TILE - 1u) / BG_SNAP_TILE;
  for (uint32_t blk = 0; blk < tiles * (uint32_t)m; blk++) {
    const uint32_t pair = blk / tiles, tile = blk - pair * tiles;
    const uint64_t se = a.src_idx ? (uint64_t)a.src_idx[pair] : pair, de = a.dst_idx ? (uint64_t)a.dst_idx[pair] : pair;
    if (a.src_idx && a.dst_idx && se == de && a.src.s[0].base == a.dst.s[0].base) continue;
    for (uint32_t lane = 0; lane < BG_SNAP_BLOCK; lane++)
      for (int q = 0; q < BG_SNAP_PER_LANE; q++) {
        const uint32_t u = tile * BG_SNAP_TILE + lane + q * BG_SNAP_BLOCK;
        if (u < a.plan.units) {
          const int j = bg_snap_find(a.plan, u);
          const uint8_t* from = bg_snap_addr(a.src, a.plan, j, u, se);
          uint8_t* to = bg_snap_addr(a.dst, a.plan, j, u, de);
          const uint32_t w = a.plan.width[j];
          if (((uintptr_t)from | (uintptr_t)to) & (w - 1)) fail("a misaligned unit", j, u);
          memmove(to, from, w);
          if (j == a.prod_slice) { if (w != 4) fail("producer word width", w); memcpy(&a.prod_other[de], from, 4); }
        } else if (u == a.plan.units && a.hdr_base) memcpy(a.hdr_base + de * a.hdr_stride, a.hdr, 16);
      }
  }
  return 0;
}

static int run_moves(size_t N, size_t KG, size_t KS, size_t KD, bool cards, size_t extra) {
  Arrays A(N, KG, KS, KD, cards, 0, 12345u + (unsigned)N);
  const uint64_t blob = BG_SNAP_HEADER_BYTES + bg_snap_bytes(A.t), stride = ((blob + 15) & ~(uint64_t)15) + extra;
  uint32_t hdr[4] = {HDR[0], HDR[1], (uint32_t)KG | (cards ? 0x10000u : 0u), (uint32_t)KS | ((uint32_t)KD << 16)};
  // get: the last env, the first, the middle ones, one twice
  std::vector<int32_t> envs = {(int32_t)N - 1, 0, (int32_t)(N / 3), (int32_t)(N / 2), (int32_t)N - 1};
  const int m = (int)envs.size();
  Bytes want(stride * m + 16, 0xA5), got(stride * m + 16, 0xA5);
  uint8_t* wb = want.data() + ((16 - ((uintptr_t)want.data() & 15)) & 15); uint8_t* gb = got.data() + ((16 - ((uintptr_t)got.data() & 15)) & 15);
  for (int i = 0; i < m; i++) ref_get(A, envs[i], wb + i * stride, hdr);
  Args g; memset(&g, 0, sizeof(g));
  g.src = A.t; g.dst = bg_snap_blob_table(A.t, gb, stride); g.src_idx = envs.data(); g.hdr_base = gb; g.hdr_stride = stride; g.hdr = hdr; g.prod_slice = -1;
  if (model(g, m)) fail("plan (get)");
  if (memcmp(wb, gb, stride * m)) fail("get: blob bytes or padding differ");
  printf("blob %llu stride %llu units %u widths", (unsigned long long)blob, (unsigned long long)stride, g.plan.units);
  for (int j = 0; j < g.plan.n; j++) printf(" %d", g.plan.width[j]);
  printf("\n");
  // set with fan-out into a handle of another size whose memory is poisoned: blob 0 to two envs, blob 2 and 3 to one each
  const size_t NB = N < 3 ? N + 4 : N / 2 + 2;
  Arrays B(NB, KG, KS, KD, cards, 0x5A, 0), R(NB, KG, KS, KD, cards, 0x5A, 0);
  std::vector<int32_t> to = {0, (int32_t)NB - 1, 2, 1}, from = {0, 0, 2, 3};
  for (size_t i = 0; i < to.size(); i++) ref_set(R, to[i], wb + from[i] * stride);
  Args s; memset(&s, 0, sizeof(s));
  s.dst = B.t; s.src = bg_snap_blob_table(B.t, gb, stride); s.src_idx = from.data(); s.dst_idx = to.data(); s.prod_slice = B.prod_slice; s.prod_other = B.other;
  if (model(s, (int)to.size())) fail("plan (set)");
  if (!B.same_bytes(R)) fail("set: the arrays differ from bg_set_state's (restored envs, or poisoned other envs touched)");
  if (memcmp(wb, gb, stride * m)) fail("set: the blobs were written");
  // round trip: get of the restored envs = the blobs they came from
  Bytes back(stride * to.size() + 16, 0xA5);
  uint8_t* bb = back.data() + ((16 - ((uintptr_t)back.data() & 15)) & 15);
  Args g2; memset(&g2, 0, sizeof(g2));
  g2.src = B.t; g2.dst = bg_snap_blob_table(B.t, bb, stride); g2.src_idx = to.data(); g2.hdr_base = bb; g2.hdr_stride = stride; g2.hdr = hdr; g2.prod_slice = -1;
  if (model(g2, (int)to.size())) fail("plan (get 2)");
  for (size_t i = 0; i < to.size(); i++) if (memcmp(bb + i * stride, wb + from[i] * stride, stride)) fail("round trip", (long)i);
  // copy A -> C (another handle) = get + set; every slice but the two words moves in 16-byte units
  Arrays C(NB, KG, KS, KD, cards, 0x5A, 0);
  std::vector<int32_t> csrc = {envs[0], envs[0], envs[2], envs[3]};
  Args c; memset(&c, 0, sizeof(c));
  c.src = A.t; c.dst = C.t; c.src_idx = csrc.data(); c.dst_idx = to.data(); c.prod_slice = C.prod_slice; c.prod_other = C.other;
  if (model(c, (int)to.size())) fail("plan (copy)");
  if (!C.same_bytes(R)) fail("copy between handles differs from get + set");
  for (int j = 0; j < c.plan.n; j++) if (c.plan.width[j] != (A.t.s[j].elem == 4 ? 4 : 16)) fail("copy: unit width", j, c.plan.width[j]);
  // copy inside one handle: the first half onto the second, one pair onto itself; the sources and every other env keep their bytes
  if (N >= 4) {
    Arrays D(N, KG, KS, KD, cards, 0, 777u), E(N, KG, KS, KD, cards, 0, 777u);
    std::vector<int32_t> ds, ss;
    for (size_t i = 0; i < N / 2; i++) { ds.push_back((int32_t)(N / 2 + i)); ss.push_back((int32_t)i); }
    ds.push_back(0); ss.push_back(0);
    Bytes one(stride + 16);
    for (size_t i = 0; i + 1 < ds.size(); i++) { ref_get(E, ss[i], one.data(), hdr); ref_set(E, ds[i], one.data()); }
    Args d; memset(&d, 0, sizeof(d));
    d.src = D.t; d.dst = D.t; d.src_idx = ss.data(); d.dst_idx = ds.data(); d.prod_slice = D.prod_slice; d.prod_other = D.other;
    if (model(d, (int)ds.size())) fail("plan (copy inside)");
    if (!D.same_bytes(E)) fail("copy inside one handle differs from get + set");
  }
  return 0;
}

static int check(const std::vector<int32_t>* src, long n_src, const std::vector<int32_t>* dst, long n_dst, int m, bool ns, bool nd, bool distinct, bool same) {
  std::vector<uint8_t> seen(n_dst > 0 ? n_dst : 1);
  int pair = -2;
  const int code = bg_snap_check_indices(src ? src->data() : nullptr, n_src, dst ? dst->data() : nullptr, n_dst, m, ns, nd, distinct, same, seen.data(), &pair);
  if ((code == BG_SNAP_OK) != (pair == -1) && !(code == BG_SNAP_E_M || code == BG_SNAP_E_NULL)) fail("bad_pair does not go with the code", code, pair);
  return code;
}
static void run_indices() {
  typedef std::vector<int32_t> V;
  const V a = {199, 0, 64, 63, 199}, low = {0, -1}, high = {0, 200}, d4 = {0, 69, 5, 64}, b4 = {0, 0, 2, 3}, bhigh = {0, 0, 2, 4}, twice = {0, 5, 0, 7};
  printf("get_repeats %d\n", check(&a, 200, nullptr, 5, 5, false, false, false, false));
  printf("get_all %d\n", check(nullptr, 200, nullptr, 200, 200, false, false, false, false));
  printf("get_all_too_many %d\n", check(nullptr, 200, nullptr, 201, 201, false, false, false, false));
  printf("get_negative %d\n", check(&low, 200, nullptr, 2, 2, false, false, false, false));
  printf("get_high %d\n", check(&high, 200, nullptr, 2, 2, false, false, false, false));
  printf("m_negative %d\n", check(&a, 200, nullptr, 5, -1, false, false, false, false));
  printf("m_zero %d\n", check(nullptr, 200, nullptr, 70, 0, true, true, true, true));
  printf("set_fanout %d\n", check(&b4, 4, &d4, 70, 4, false, true, true, false));
  printf("set_identity_blobs %d\n", check(nullptr, 4, &d4, 70, 4, false, true, true, false));
  printf("set_null_envs %d\n", check(&b4, 4, nullptr, 70, 4, false, true, true, false));
  printf("set_blob_high %d\n", check(&bhigh, 4, &d4, 70, 4, false, true, true, false));
  printf("set_too_few_blobs %d\n", check(nullptr, 3, &d4, 70, 4, false, true, true, false));
  printf("set_env_high %d\n", check(&b4, 4, &d4, 69, 4, false, true, true, false));
  printf("set_env_twice %d\n", check(&b4, 4, &twice, 70, 4, false, true, true, false));
  const V s1 = {1, 1, 1}, dd = {2, 3, 4}, chain_s = {0, 1}, chain_d = {1, 2}, self_s = {5, 5, 9}, self_d = {5, 6, 9}, swap_s = {0, 1}, swap_d = {1, 0};
  printf("copy_fork %d\n", check(&s1, 10, &dd, 10, 3, true, true, true, true));
  printf("copy_chain %d\n", check(&chain_s, 10, &chain_d, 10, 2, true, true, true, true));
  printf("copy_chain_other_handle %d\n", check(&chain_s, 10, &chain_d, 10, 2, true, true, true, false));
  printf("copy_self %d\n", check(&self_s, 10, &self_d, 10, 3, true, true, true, true));
  printf("copy_swap %d\n", check(&swap_s, 10, &swap_d, 10, 2, true, true, true, true));
  printf("copy_null_src %d\n", check(nullptr, 10, &dd, 10, 3, true, true, true, true));
  printf("copy_null_dst %d\n", check(&s1, 10, nullptr, 10, 3, true, true, true, true));
  printf("copy_dst_twice %d\n", check(&s1, 10, &twice, 10, 3, true, true, true, true));
  printf("copy_src_high %d\n", check(&dd, 4, &dd, 10, 3, true, true, true, false));
  printf("codes %d %d %d %d %d %d %d\n", BG_SNAP_OK, BG_SNAP_E_M, BG_SNAP_E_NULL, BG_SNAP_E_SRC_RANGE, BG_SNAP_E_DST_RANGE, BG_SNAP_E_DST_TWICE, BG_SNAP_E_OVERLAP);
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "indices")) run_indices();
  else if (argc == 7) run_moves(atol(argv[1]), atol(argv[2]), atol(argv[3]), atol(argv[4]), atoi(argv[5]) != 0, atol(argv[6]));
  else return 2;
  printf(bad ? "MISMATCHES %d\n" : "OK %d\n", bad);
  return bad != 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("state_batch_host")
    (d / "snap_host.cpp").write_text(_source())
    out = d / "snap_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-o", str(out), str(d / "snap_host.cpp")])
    return str(out)


def _blob_bytes(kg, ks, kd, cards):
    # tests/test_state_layout_gpu.py's formula; the card-state slices add two 112-byte chunk sets and two lazy streams
    return 16 + 128 + 64 + 112 + 32 + kd * 64 + kg * 2560 + ks * 256 + 3 * 2560 + 128 * 4 + 4 + 4 + (2 * 112 + 2 * 2560 if cards else 0)


@pytest.mark.parametrize("n", (1, 70, 200))
@pytest.mark.parametrize("depths", ((1, 3, 1), (12, 13, 8)), ids=("KD1_KS3_KG1", "KD12_KS13_KG8"))
@pytest.mark.parametrize("cards", (False, True), ids=("plain", "cards"))
@pytest.mark.parametrize("extra", (0, 128), ids=("tight", "one_line_more"))
def test_get_set_copy_against_slice_copies(exe, n, depths, cards, extra):
    kd, ks, kg = depths
    r = subprocess.run([exe, str(n), str(kg), str(ks), str(kd), str(int(cards)), str(extra)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "OK 0", r.stdout + r.stderr
    f = next(l for l in r.stdout.splitlines() if l.startswith("blob ")).split()
    blob, stride, units, widths = int(f[1]), int(f[3]), int(f[5]), [int(w) for w in f[7:]]
    assert blob == _blob_bytes(kg, ks, kd, cards)
    assert stride == (blob + 15) // 16 * 16 + extra and stride % 16 == 0
    # to a blob: 16-byte units everywhere but the two words; the card-state slices lie behind those 8 bytes, so they move 8 at a time
    assert widths == [16] * 11 + [4, 4] + ([8] * 4 if cards else [])
    assert units == (blob - 16 - 8 - (5344 if cards else 0)) // 16 + 2 + (5344 // 8 if cards else 0)


def test_index_lists(exe):
    r = subprocess.run([exe, "indices"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in r.stdout.splitlines() if not l.startswith(("OK", "FAIL"))}
    ok, e_m, e_null, e_src, e_dst, e_twice, e_overlap = got.pop("codes")
    want = {"get_repeats": ok, "get_all": ok, "get_all_too_many": e_src, "get_negative": e_src, "get_high": e_src, "m_negative": e_m, "m_zero": ok,
            "set_fanout": ok, "set_identity_blobs": ok, "set_null_envs": e_null, "set_blob_high": e_src, "set_too_few_blobs": e_src, "set_env_high": e_dst,
            "set_env_twice": e_twice, "copy_fork": ok, "copy_chain": e_overlap, "copy_chain_other_handle": ok, "copy_self": ok, "copy_swap": e_overlap,
            "copy_null_src": e_null, "copy_null_dst": e_null, "copy_dst_twice": e_twice, "copy_src_high": e_src}
    assert {k: v[0] for k, v in got.items()} == want
    assert len({ok, e_m, e_null, e_src, e_dst, e_twice, e_overlap}) == 7 and ok == 0


def test_header_declares_and_library_exports():
    import re
    from balatro_gym_amd import _native as nat, build
    hdr = open(HEADER).read()
    for name in ("bg_get_states", "bg_set_states", "bg_copy_states"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in nat.EXPORTS
    doc = hdr[:hdr.index("int bg_get_states")].rsplit("/*", 1)[1]
    for word in ("save_state()", "load_state()", "BG_E_ARG", "EVENT", "SYNCHRONISES", "never written", "m == 0", "RowNormalizer"):
        assert word in doc, word
    assert os.path.join(CSRC, "bg_snapshot.h") in build.DEPS
