// bg_snapshot.h -- many envs' state at once: bg_get_states / bg_set_states / bg_copy_states (gfx950).
//
// An env's state is one slice of every per-env array (bg_slices in bg_lib.hip: `rows` pieces of `elem` bytes, row r of env i at
// base + i * env_stride + r * row_stride).  ONE kernel moves m envs between two SLICE TABLES that list the same slices in the same order: the
// handle's arrays on one side and dense blobs on the other (a blob is a table whose env stride is the blob stride and whose rows are packed), or
// the arrays of two handles.  One launch moves every slice of every pair, writes the blobs' 16-byte headers (bg_get_states) and puts the
// producer word into the second producer buffer as well (on the way in).
//
// The PLAN cuts an env's state into UNITS, slice after slice: a unit is the widest power of two of bytes (16 at most) that divides the slice's
// row and both tables' addresses of it -- 16 everywhere but for the two 4-byte words (shop-seed meta, producer word), and 8 for the card-state
// slices when one side is a blob (they lie behind those two words: at 8 modulo 16).  Unit u of a pair is one lane's load and store; consecutive
// lanes take consecutive units, so the contiguous runs (an env's rings and MT blocks: 2.5 KB and more) move as whole lines.  A workgroup of 256
// lanes moves BG_SNAP_TILE consecutive units of one pair, all loads in flight before the first store.  Plain stores: the engine reads this next.
//
// The plan, the address of a unit and the index checks are plain C++ behind BG_SNAP_FN, so tests/test_state_batch_host.py compiles them with g++
// (define BG_SNAP_HOST before including) and drives them through a scalar model of the kernel's loop.
#ifndef BG_SNAPSHOT_H
#define BG_SNAPSHOT_H
#include <stddef.h>
#include <stdint.h>

#ifdef BG_SNAP_HOST
#define BG_SNAP_FN static inline
#else
#define BG_SNAP_FN __host__ __device__ __forceinline__
#endif

#define BG_SNAP_MAX_SLICES 20
#define BG_SNAP_BLOCK 256
#define BG_SNAP_PER_LANE 4
#define BG_SNAP_TILE (BG_SNAP_BLOCK * BG_SNAP_PER_LANE)   // units of one pair per workgroup
#define BG_SNAP_HEADER_BYTES 16

struct BgSnapSlice { uint8_t* base; uint64_t env_stride, row_stride; uint32_t elem, rows; };
struct BgSnapTable { BgSnapSlice s[BG_SNAP_MAX_SLICES]; int n; };
// slice j: units [first[j], first[j + 1]) of `width[j]` bytes; a row holds 1 << row_shift[j] units (slices of one row: the whole slice)
struct BgSnapPlan { uint32_t first[BG_SNAP_MAX_SLICES + 1]; uint8_t width[BG_SNAP_MAX_SLICES], row_shift[BG_SNAP_MAX_SLICES]; int n; uint32_t units; };

BG_SNAP_FN uint64_t bg_snap_bytes(const BgSnapTable& t) {   // an env's bytes behind the header
  uint64_t b = 0;
  for (int j = 0; j < t.n; j++) b += (uint64_t)t.s[j].rows * t.s[j].elem;
  return b;
}

// The blobs as a table: slice j packed (row stride = elem) at its offset behind the header, blob i at blobs + i * stride
BG_SNAP_FN BgSnapTable bg_snap_blob_table(const BgSnapTable& dev, void* blobs, uint64_t stride) {
  BgSnapTable t;
  t.n = dev.n;
  uint64_t off = BG_SNAP_HEADER_BYTES;
  for (int j = 0; j < dev.n; j++) {
    t.s[j].base = (uint8_t*)blobs + off; t.s[j].env_stride = stride; t.s[j].row_stride = dev.s[j].elem; t.s[j].elem = dev.s[j].elem; t.s[j].rows = dev.s[j].rows;
    off += (uint64_t)dev.s[j].rows * dev.s[j].elem;
  }
  return t;
}

BG_SNAP_FN uint32_t bg_snap_align(const BgSnapSlice& s) {   // the widest move every row of every env of the slice allows on this side
  uint64_t bits = (uint64_t)(uintptr_t)s.base | s.env_stride | s.elem | 16u;
  if (s.rows > 1) bits |= s.row_stride;
  return (uint32_t)(bits & (~bits + 1u));
}

// 0, or what is wrong: 1 the tables differ in their slices, 2 a slice that is no multiple of 4 bytes or not 4-byte aligned, 3 a row of several
// units whose count is no power of two (no slice of the library's: a unit's row would need a division)
BG_SNAP_FN int bg_snap_plan(const BgSnapTable& a, const BgSnapTable& b, BgSnapPlan& p) {
  if (a.n != b.n || a.n > BG_SNAP_MAX_SLICES) return 1;
  p.n = a.n;
  uint32_t u = 0;
  for (int j = 0; j < a.n; j++) {
    if (a.s[j].elem != b.s[j].elem || a.s[j].rows != b.s[j].rows) return 1;
    const uint32_t wa = bg_snap_align(a.s[j]), wb = bg_snap_align(b.s[j]), w = wa < wb ? wa : wb;
    if (w < 4) return 2;
    const uint32_t per_row = a.s[j].elem / w;
    uint32_t sh = 0;
    while ((1u << sh) < per_row) sh++;
    if (a.s[j].rows > 1 && (1u << sh) != per_row) return 3;
    p.first[j] = u; p.width[j] = (uint8_t)w; p.row_shift[j] = (uint8_t)sh;
    u += a.s[j].rows * per_row;
  }
  p.first[a.n] = u; p.units = u;
  return 0;
}

// the slice of unit u (u < p.units): the number of slices that start at or below u, less one.  No loop whose next load waits for the last compare: on the
// device the starts are read with constant indexes (scalar loads, once per wave) and the lanes only compare
BG_SNAP_FN int bg_snap_find(const BgSnapPlan& p, uint32_t u) {
  int j = 0;
#pragma unroll
  for (int k = 1; k < BG_SNAP_MAX_SLICES; k++) j += (k < p.n && u >= p.first[k]) ? 1 : 0;
  return j;
}
// where unit u (of slice j) of env `env` lies in table t
BG_SNAP_FN uint8_t* bg_snap_addr(const BgSnapTable& t, const BgSnapPlan& p, int j, uint32_t u, uint64_t env) {
  const uint32_t k = u - p.first[j];
  const BgSnapSlice& s = t.s[j];
  if (s.rows == 1) return s.base + env * s.env_stride + (uint64_t)k * p.width[j];
  const uint32_t row = k >> p.row_shift[j], col = k & ((1u << p.row_shift[j]) - 1u);
  return s.base + env * s.env_stride + (uint64_t)row * s.row_stride + (uint64_t)col * p.width[j];
}

// The index lists of a call, checked on the host before anything is launched.  src / dst: m indexes each (NULL = 0..m-1); n_src / n_dst: what they
// index; distinct_dst: a dst may occur once; same: src and dst index the SAME envs (bg_copy_states on one handle) -- a pair with dst == src moves
// nothing, and no dst of another pair may be a src.  `seen` is scratch of n_dst bytes.
enum { BG_SNAP_OK = 0, BG_SNAP_E_M = 1, BG_SNAP_E_NULL = 2, BG_SNAP_E_SRC_RANGE = 3, BG_SNAP_E_DST_RANGE = 4, BG_SNAP_E_DST_TWICE = 5, BG_SNAP_E_OVERLAP = 6 };
BG_SNAP_FN int bg_snap_check_indices(const int32_t* src, int64_t n_src, const int32_t* dst, int64_t n_dst, int m, bool need_src, bool need_dst,
                                     bool distinct_dst, bool same, uint8_t* seen, int* bad_pair) {
  *bad_pair = -1;
  if (m < 0) return BG_SNAP_E_M;
  if (m == 0) return BG_SNAP_OK;
  if ((need_src && !src) || (need_dst && !dst)) return BG_SNAP_E_NULL;
  for (int i = 0; i < m; i++) {
    const int64_t se = src ? src[i] : i, de = dst ? dst[i] : i;
    *bad_pair = i;
    if (se < 0 || se >= n_src) return BG_SNAP_E_SRC_RANGE;
    if (de < 0 || de >= n_dst) return BG_SNAP_E_DST_RANGE;
  }
  if (distinct_dst) {
    for (int64_t e = 0; e < n_dst; e++) seen[e] = 0;
    for (int i = 0; i < m; i++) {
      const int64_t de = dst ? dst[i] : i;
      *bad_pair = i;
      if (seen[de]) return BG_SNAP_E_DST_TWICE;
      seen[de] = 1;
    }
    if (same) {   // seen: 1 = a dst that is written (its pair has another src)
      for (int i = 0; i < m; i++) { const int64_t se = src ? src[i] : i, de = dst ? dst[i] : i; if (se == de) seen[de] = 0; }
      for (int i = 0; i < m; i++) {
        const int64_t se = src ? src[i] : i, de = dst ? dst[i] : i;
        *bad_pair = i;
        if (se != de && seen[se]) return BG_SNAP_E_OVERLAP;
      }
    }
  }
  *bad_pair = -1;
  return BG_SNAP_OK;
}

#ifndef BG_SNAP_HOST
struct BgSnapArgs {
  BgSnapTable src, dst;
  BgSnapPlan plan;
  const int32_t* src_idx;   // [m] on the device, null = the pair's number
  const int32_t* dst_idx;
  uint32_t tiles;           // workgroups per pair: ceil((units + header) / BG_SNAP_TILE)
  uint8_t* hdr_base;        // bg_get_states: blob i's header at hdr_base + i * hdr_stride (null otherwise); it is unit `plan.units`
  uint64_t hdr_stride;
  uint4 hdr;
  int prod_slice;           // on the way in: the slice of the producer word, which also goes to prod_other[dst env] (-1: nowhere else)
  uint32_t* prod_other;
};

// grid = m * tiles workgroups of BG_SNAP_BLOCK lanes
__global__ __launch_bounds__(BG_SNAP_BLOCK) void bg_snapshot_kernel(const BgSnapArgs a) {
  const uint32_t pair = blockIdx.x / a.tiles, tile = blockIdx.x - pair * a.tiles;
  const uint64_t se = a.src_idx ? (uint64_t)a.src_idx[pair] : pair, de = a.dst_idx ? (uint64_t)a.dst_idx[pair] : pair;
  if (a.src_idx && a.dst_idx && se == de && a.src.s[0].base == a.dst.s[0].base) return;   // a pair onto itself
  const uint32_t u0 = tile * BG_SNAP_TILE + threadIdx.x;
  uint4 v[BG_SNAP_PER_LANE];
  uint8_t* to[BG_SNAP_PER_LANE];
  uint32_t w[BG_SNAP_PER_LANE];
#pragma unroll
  for (int q = 0; q < BG_SNAP_PER_LANE; q++) {
    const uint32_t u = u0 + q * BG_SNAP_BLOCK;
    w[q] = 0; to[q] = nullptr; v[q] = make_uint4(0, 0, 0, 0);
    if (u < a.plan.units) {
      // a wave's 64 consecutive units nearly always lie in ONE slice: its table entries are then read with a scalar index (scalar loads of the kernel
      // arguments) instead of per lane
      const int j = bg_snap_find(a.plan, u), ju = __builtin_amdgcn_readfirstlane(j);
      const uint8_t* from;
      if (__ballot(j != ju) == 0ull) { from = bg_snap_addr(a.src, a.plan, ju, u, se); to[q] = bg_snap_addr(a.dst, a.plan, ju, u, de); w[q] = a.plan.width[ju]; }
      else { from = bg_snap_addr(a.src, a.plan, j, u, se); to[q] = bg_snap_addr(a.dst, a.plan, j, u, de); w[q] = a.plan.width[j]; }
      if (w[q] == 16) v[q] = *(const uint4*)from;
      else if (w[q] == 8) { const uint2 t = *(const uint2*)from; v[q].x = t.x; v[q].y = t.y; }
      else v[q].x = *(const uint32_t*)from;
      if (j == a.prod_slice) w[q] |= 0x100u;
    } else if (u == a.plan.units && a.hdr_base) {
      to[q] = a.hdr_base + de * a.hdr_stride; w[q] = 16; v[q] = a.hdr;
    }
  }
#pragma unroll
  for (int q = 0; q < BG_SNAP_PER_LANE; q++) {
    const uint32_t wq = w[q] & 0xffu;
    if (wq == 16) *(uint4*)to[q] = v[q];
    else if (wq == 8) *(uint2*)to[q] = make_uint2(v[q].x, v[q].y);
    else if (wq == 4) { *(uint32_t*)to[q] = v[q].x; if (w[q] & 0x100u) a.prod_other[de] = v[q].x; }
  }
}

// What bg_set_states needs on the host of every pair's blob before it writes: the header, hot chunk 7 (the curriculum cap) and the two template
// chunks -- 64 bytes per pair, read back in one copy.  Slices 0 and 3 are the hot and template chunks (bg_slices).
__global__ __launch_bounds__(64) void bg_snapshot_meta_kernel(const uint8_t* __restrict__ blobs, uint64_t stride, const int32_t* __restrict__ blob_idx, int m,
                                                              uint32_t hot7_off, uint32_t tmpl_off, uint4* __restrict__ out) {
  const int i = blockIdx.x * 16 + (threadIdx.x >> 2), part = threadIdx.x & 3;
  if (i >= m) return;
  const uint8_t* b = blobs + (uint64_t)(blob_idx ? blob_idx[i] : i) * stride;
  const uint32_t off = part == 0 ? 0u : part == 1 ? hot7_off : tmpl_off + (uint32_t)(part - 2) * 16u;
  out[(size_t)i * 4 + part] = *(const uint4*)(b + off);
}
#endif  // BG_SNAP_HOST
#endif
