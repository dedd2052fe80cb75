// bg_extractor.h -- bg_extractor_rows / bg_extractor_rows_grad: the first layer behind BalatroFeaturesExtractor's input, forward and weight gradient,
// straight from packed records.
//
// The layer's input is the 447-column bfloat16 row bg_encode_rows_ex writes for BG_ENC_EXTRACTOR: 416 one-hot hand columns (52 slot + card), 10 joker ids
// and 21 scaled state features.  The product runs over 447 columns padded to 448 = 28 k-steps of the matrix cores' 32x32x16 bfloat16 instruction; the
// 416 one-hot columns are exactly 26 of them (13 accumulator tiles of the gradient), the 31 dense columns and the padding the last two (one tile).
// The one-hot part never exists as an image: a row's 8 hand bytes decide every one of its 416 elements, so a lane builds its fragment elements from the
// bytes (forward: the lane owns a row; gradient: the lane owns a column and compares it with 8 rows' bytes of one slot).  Only the 31 dense columns go
// through phases 1-2 of the records-to-tile pipeline (bg_encode.h: bg_enc_stage_gather, bg_enc_fill_tile with BgEncConvert<BG_ENC_EXTRACTOR>, the
// converter of bg_encode_gather_kernel) and are rounded to bfloat16 (bg_enc_bf16) into a 32-column operand image.
//
// The index arithmetic is plain C++ behind BG_EXT_FN, so tests/test_extractor_rows_host.py compiles it with g++ (define BG_EXT_HOST before including)
// and drives it through a scalar model of the instruction.  The fragment maps of the instruction itself are bg_linear.h's (bg_lin_frag_*, bg_lin_acc_*).
#ifndef BG_EXTRACTOR_H
#define BG_EXTRACTOR_H
#include <stdint.h>

#ifdef BG_EXT_HOST
#ifndef BG_LIN_HOST
#define BG_LIN_HOST
#endif
#define BG_EXT_FN static inline
#else
#define BG_EXT_FN __host__ __device__ __forceinline__
#endif
#include "bg_linear.h"

#define BG_EXT_K 447      /* columns of the input: BG_ENC_EXTRACTOR_COLS */
#define BG_EXT_KPAD 448   /* the reduction the matrix cores run: one column of zeros */
#define BG_EXT_HOT 416    /* the one-hot columns: 8 slots x 52 cards */
#define BG_EXT_CARDS 52
#define BG_EXT_SLOTS 8
#define BG_EXT_DENSE 31   /* joker ids and state features: columns 416..446 */
#define BG_EXT_HOT_STEPS (BG_EXT_HOT / BG_LIN_KSTEP)   /* 26 k-steps of the forward are one-hot */
#define BG_EXT_STEPS (BG_EXT_KPAD / BG_LIN_KSTEP)      /* 28 */
#define BG_EXT_KTILES (BG_EXT_KPAD / BG_LIN_TILE)      /* 14 accumulator tiles of k in the gradient: 13 one-hot, then the dense one */
#define BG_EXT_HOT_TILES (BG_EXT_HOT / BG_LIN_TILE)    /* 13 */
#define BG_EXT_SPAN_TILES 5 /* k-tiles of one workgroup of the gradient: the wave shape of bg_linear_rows_grad_kernel (2 x 5 accumulator tiles) */
#define BG_EXT_KSPANS 3     /* spans of k over the gradient's grid: tiles 0..4, 5..9, 10..13 */
#define BG_EXT_PART_ROWS (BG_EXT_KPAD + 1) /* rows of a gradient partial: [448][H] of dweight^T, then [H] of dbias */

// ---- the one-hot columns ----
BG_EXT_FN int bg_ext_slot(int k) { return k / BG_EXT_CARDS; }   // one-hot column k = 52 slot + card
BG_EXT_FN int bg_ext_card(int k) { return k % BG_EXT_CARDS; }
// x[i][k] for k < 416 from the row's hand byte of slot(k): bfloat16 bits of 1.0 / +0.0.  The bytes -1, 52..127 and negative values equal no card.
BG_EXT_FN uint16_t bg_ext_hot(int byte, int k) { return byte == bg_ext_card(k) ? (uint16_t)0x3f80u : (uint16_t)0; }
// FORWARD: lane l holds, in k-step s, the columns 16 s + 8 (l >> 5) + j of its row.  q[slot] is the hot column of a slot relative to the lane's half,
// 52 slot + byte - 8 (l >> 5), or a negative number no column equals when the byte names no card; element j of step s is 1.0 exactly when the slot
// its column lies in has q == 16 s + j.  Columns 16 s .. 16 s + 15 lie in at most two slots, known at compile time: no indexed register access.
BG_EXT_FN int bg_ext_hot_q(int slot, int byte, int lane) { return byte >= 0 && byte < BG_EXT_CARDS ? BG_EXT_CARDS * slot + byte - 8 * (lane >> 5) : -1024; }
BG_EXT_FN uint16_t bg_ext_hot_elem(const int* q, int step, int j) {
  const int a = bg_ext_slot(BG_LIN_KSTEP * step), b = bg_ext_slot(BG_LIN_KSTEP * step + BG_LIN_KSTEP - 1), t = BG_LIN_KSTEP * step + j;
  return q[a] == t || q[b] == t ? (uint16_t)0x3f80u : (uint16_t)0;
}
// GRADIENT: lane l holds, in k-tile `tile`, row k = 32 tile + (l & 31) of x^T: 8 consecutive records' hand bytes of slot(k) compared with card(k)
BG_EXT_FN int bg_ext_tile_k(int tile, int lane) { return BG_LIN_TILE * tile + bg_lin_frag_rc(lane); }

// ---- the gradient's split: m rows into blocks of 128, `per` consecutive blocks per row group; H into spans of 256 units; k into 3 spans of tiles ----
BG_EXT_FN int bg_ext_span_tile0(int z) { return BG_EXT_SPAN_TILES * z; }
BG_EXT_FN int bg_ext_span_tiles(int z) { return BG_EXT_KTILES - bg_ext_span_tile0(z) < BG_EXT_SPAN_TILES ? BG_EXT_KTILES - bg_ext_span_tile0(z) : BG_EXT_SPAN_TILES; }
// bg_linear.h's split with BG_EXT_KSPANS workgroups per unit span
BG_EXT_FN int64_t bg_ext_blocks_per_group(int64_t m, int H) { return bg_lin_blocks_per_group(m, H, BG_EXT_KSPANS); }
BG_EXT_FN int64_t bg_ext_groups(int64_t m, int H) { return bg_lin_groups(m, H, BG_EXT_KSPANS); }
// bg_extractor_rows_workspace_bytes: groups partials of [449][H] float32
BG_EXT_FN uint64_t bg_ext_workspace_bytes(int64_t m, int H) { return bg_lin_workspace_bytes(m, H, BG_EXT_KSPANS, BG_EXT_PART_ROWS); }

#ifndef BG_EXT_HOST
// ---- the kernels ----
// FORWARD, grid (ceil(m / 128), ysplit), 256 lanes = 4 waves, wave w = rows 32 w .. 32 w + 31 of the workgroup's 128:
//   1  the 128 rows' hand bytes (one 16-byte read of the record per row, through the index; no source or a row at or beyond m: 0xff) into LDS;
//   2  four times phases 1-2 of the encode kernels for 32 records with the EXTRACTOR converter, each followed by the rounding of the 32 x 31 float32
//      tile to bfloat16 into XD[128][40] (column 31 = the padding column 447: zero; 80-byte lines: 16-byte aligned fragments);
//   3  a lane builds the 26 one-hot A fragments of its row from the 8 bytes (bg_ext_hot_elem) and reads the two dense ones from XD: 112 registers, once;
//   4  for every chunk of 64 output units (chunks y, y + ysplit, ...): the 64 x 447 weights go to WB[64][456] (bg_ext_stage_w: 16-byte pieces when the
//      matrix is 16-byte aligned with a pitch that is a multiple of 8, words when 4-byte aligned with an even pitch, else elements -- 2-byte alignment is
//      all that is asked; all loads of a batch in flight before its first LDS store), over the LDS of phase 2 which is dead by then; per 32 units a
//      wave runs 28 instructions, adds the bias, applies the activation and stores its 32 x 32 tile as bg_linear_rows_kernel does.
// LDS 69.9 KB: two workgroups per CU.
// GRADIENT, grid (groups, ceil(H / 256), 3): a workgroup walks `per` blocks of 128 rows for the k-tiles of its span z.  Per block the rows' hand bytes go
// to LDS slot-major (HB[8][128]); span 2 also runs phase 2 above into the TRANSPOSE XT[32][136] of the dense tile.  D'[k][n] = sum_i x[i][k] dp[i][n]:
// the A fragment of a one-hot tile is ONE 8-byte LDS read (8 records' bytes of the lane's slot) compared with the lane's card; of the dense tile a
// 16-byte read of XT.  The B fragment is bg_linear_rows_grad_kernel's: 8 rows of one unit of dout, from HBM, masked and rounded -- but all 16 fragments
// of a block are loaded before its staging, unconditionally and with the element types compile-time constants (bg_ext_raw / bg_ext_dp: six instantiations of the
// kernel), 16 to 32 loads at a time -- with run-time types every load sat behind a branch and a wait of its own.  A wave keeps
// 2 x 5 accumulator tiles and the float32 sum of its dp values.  Partial g = [449][H] float32 (span z writes rows 160 z ..; span 0 the dbias row);
// bg_extractor_reduce_kernel sums the partials in index order in float64.  No atomics: two calls give the same bits.
// Every kernel here is a template (the reduce kernel on KCOLS = BG_EXT_K, where nothing else varies) and the header is read at the end of the library (bg_rows_api.h): instantiations
// are emitted behind every other function, so adding them leaves the other kernels' text, label numbers included, as it was.
#define BG_EXT_WPITCH 456  /* bf16 elements of a line of WB: 912 bytes */
#define BG_EXT_DPITCH 40   /* bf16 elements of a line of XD */
#define BG_EXT_STAGE_WORDS (BG_ENC_RECS * BG_ENC_REC_PITCH / 4 + BG_ENC_RECS * BG_EXT_DENSE)
static_assert(BG_EXT_K == BG_ENC_EXTRACTOR_COLS && BG_EXT_HOT == BG_ENC_ONEHOT_COLS && BG_EXT_DENSE == bg_enc_dense_cols(BG_ENC_EXTRACTOR), "the layout of bg_encode.h");
static_assert(BG_EXT_HOT % BG_LIN_TILE == 0 && BG_EXT_KPAD - BG_EXT_HOT == BG_LIN_TILE, "13 one-hot tiles and one dense tile");
static_assert(BG_EXT_KSPANS * BG_EXT_SPAN_TILES >= BG_EXT_KTILES && (BG_EXT_KSPANS - 1) * BG_EXT_SPAN_TILES <= BG_EXT_HOT_TILES, "the dense tile is in the last span alone");
static_assert(BG_EXT_WPITCH % 8 == 0 && BG_EXT_DPITCH % 8 == 0 && BG_EXT_WPITCH >= BG_EXT_KPAD, "fragments are 16-byte reads");
static_assert(BG_LIN_WCHUNK * BG_EXT_WPITCH * 2 >= BG_EXT_STAGE_WORDS * 4, "the staging area fits the weight chunk that reuses it");
static_assert((BG_ROW_HAND & ~15) + 16 >= BG_ROW_HAND + BG_EXT_SLOTS && BG_ROW_HAND % 16 == 6, "the hand bytes lie in one 16-byte piece of the record, from its byte 6");

// the hand bytes of the BG_LIN_ROWS rows from rec0 as two words per row: hw[2 row] (slots 0..3), hw[2 row + 1] (slots 4..7), or slot-major bytes
// hb[128 slot + row] (TRANSPOSED).  No barrier.
template <bool TRANSPOSED>
__device__ __forceinline__ void bg_ext_load_hands(const uint8_t* __restrict__ rows, uint64_t row_stride, const int32_t* __restrict__ index, long long store_rows,
                                                  long long m, long long rec0, uint32_t* hw) {
  if (threadIdx.x >= BG_LIN_ROWS) return;
  const long long i = rec0 + threadIdx.x;
  const long long at = i >= m ? -1 : index ? bg_enc_source_row(index[i], store_rows) : i;
  uint32_t lo = ~0u, hi = ~0u;
  if (at >= 0) {
    const uint4 v = *reinterpret_cast<const uint4*>(rows + (size_t)at * row_stride + (BG_ROW_HAND & ~15));
    lo = v.y >> 16 | v.z << 16;
    hi = v.z >> 16 | v.w << 16;
  }
  if (TRANSPOSED) {
    uint8_t* const hb = reinterpret_cast<uint8_t*>(hw);
#pragma unroll
    for (int s = 0; s < BG_EXT_SLOTS; s++) hb[s * BG_LIN_ROWS + threadIdx.x] = (uint8_t)((s < 4 ? lo : hi) >> (8 * (s & 3)));
  } else {
    hw[2 * threadIdx.x] = lo;
    hw[2 * threadIdx.x + 1] = hi;
  }
}

// the 31 dense columns of the BG_LIN_ROWS records from rec0 as bfloat16 into `x`: [row][c] of BG_EXT_DPITCH (TRANSPOSED false) or [c][row] of
// BG_LIN_TPITCH; rows at or beyond m and column 31 are +0.0.  Ends behind a barrier.  (The twin of bg_lin_build_x, bg_linear.h: one function over the
// converter, the columns and the pitch moved a kernel's text -- DESIGN.md, "Source-only changes to the engines".)
template <bool TRANSPOSED>
__device__ __forceinline__ void bg_ext_build_dense(const uint8_t* __restrict__ rows, uint64_t row_stride, const int32_t* __restrict__ index, long long store_rows,
                                                   long long m, long long rec0, long long* src, uint32_t* stage, uint16_t* x) {
  uint32_t* const recs32 = stage;
  uint32_t* const tile = stage + BG_ENC_RECS * BG_ENC_REC_PITCH / 4;
  for (int sub = 0; sub < BG_LIN_ROWS / BG_ENC_RECS; sub++) {
    const long long r0 = rec0 + sub * BG_ENC_RECS;
    const int nrec = (int)(m - r0 < BG_ENC_RECS ? m - r0 : BG_ENC_RECS);
    if (nrec > 0) {   // (uniform over the workgroup)
      bg_enc_stage_gather(rows, row_stride, index, store_rows, r0, nrec, src, recs32);
      __syncthreads();
      bg_enc_fill_tile<BG_EXT_DENSE, true>(recs32, tile, r0, nrec, src, BgEncConvert<BG_ENC_EXTRACTOR>{});
      __syncthreads();
    }
    for (int e = threadIdx.x; e < BG_ENC_RECS * BG_LIN_TILE; e += BG_LIN_BLOCK) {
      int r, c;
      if (TRANSPOSED) { c = e / BG_ENC_RECS; r = e - c * BG_ENC_RECS; }
      else { r = e / BG_LIN_TILE; c = e - r * BG_LIN_TILE; }
      const uint16_t v = r < nrec && c < BG_EXT_DENSE ? bg_enc_bf16(tile[r * BG_EXT_DENSE + c]) : (uint16_t)0;
      if (TRANSPOSED) x[c * BG_LIN_TPITCH + sub * BG_ENC_RECS + r] = v;
      else x[(sub * BG_ENC_RECS + r) * BG_EXT_DPITCH + c] = v;
    }
    __syncthreads();
  }
}

// A chunk of BG_LIN_WCHUNK units of the weight -> WB, element 447 of every line zero (units at or beyond H: zeros).  V elements per load: 8 (the matrix
// 16-byte aligned, its pitch a multiple of 8), 2 (4-byte aligned, even pitch) or 1.  The whole pieces in front of a line's last one go in batches, every
// load unconditional -- a line at or beyond H reads the chunk's first piece instead and is replaced by zero; the last piece holds element 447, which a
// [H, 447] matrix does not have: its elements below 447 are read one by one, by the first BG_LIN_WCHUNK lanes.
template <int V> struct BgExtPiece { typedef uint16_t T; };
template <> struct BgExtPiece<2> { typedef uint32_t T; };
template <> struct BgExtPiece<8> { typedef bg_lin_u4 T; };
template <int V>
__device__ __forceinline__ void bg_ext_stage_w(const uint16_t* __restrict__ weight, uint32_t wstride, int n0, int H, uint16_t* wb) {
  typedef typename BgExtPiece<V>::T T;
  const uint16_t* const base = weight + (size_t)n0 * wstride;   // uniform; a lane's offsets below fit 32 bits (wstride <= 2**24: bg_extractor_rows)
  constexpr int MAIN = BG_EXT_KPAD / V - 1, ITEMS = BG_LIN_WCHUNK * MAIN, PER = (ITEMS + BG_LIN_BLOCK - 1) / BG_LIN_BLOCK, BATCH = V == 8 ? 7 : 14;   // 28 / 14 / 14 registers of loads in flight beside the 112 of the A fragments
  static_assert(PER % BATCH == 0 && BG_EXT_KPAD % V == 0, "whole batches per lane");
#pragma unroll 1
  for (int b0 = 0; b0 < PER; b0 += BATCH) {
    T v[BATCH];
#pragma unroll
    for (int i = 0; i < BATCH; i++) {
      const int e = threadIdx.x + (b0 + i) * BG_LIN_BLOCK, n = e / MAIN, j = e - n * MAIN;
      const bool ok = e < ITEMS && n0 + n < H;
      const T w = *reinterpret_cast<const T*>(__builtin_assume_aligned(base + (ok ? (uint32_t)n * wstride + (uint32_t)(j * V) : 0u), 2 * V));
      v[i] = ok ? w : T(0);
    }
#pragma unroll
    for (int i = 0; i < BATCH; i++) {
      const int e = threadIdx.x + (b0 + i) * BG_LIN_BLOCK, n = e / MAIN, j = e - n * MAIN;
      if (e < ITEMS) *reinterpret_cast<T*>(wb + n * BG_EXT_WPITCH + j * V) = v[i];
    }
  }
  if (threadIdx.x < BG_LIN_WCHUNK) {   // the last piece: elements MAIN * V .. 446 and the zero of 447
    const bool ok = n0 + (int)threadIdx.x < H;
    uint16_t t[V];
#pragma unroll
    for (int k = 0; k < V - 1; k++) {
      const uint16_t w = base[ok ? threadIdx.x * wstride + (uint32_t)(MAIN * V + k) : 0u];
      t[k] = ok ? w : (uint16_t)0;
    }
    t[V - 1] = 0;
#pragma unroll
    for (int k = 0; k < V; k++) wb[threadIdx.x * BG_EXT_WPITCH + MAIN * V + k] = t[k];
  }
}

template <int ODT>
__global__ __launch_bounds__(BG_LIN_BLOCK, 2) void bg_extractor_rows_kernel(const uint8_t* __restrict__ rows, uint64_t row_stride, const int32_t* __restrict__ index,
                                                                         long long store_rows, long long m, const uint16_t* __restrict__ weight, uint64_t wstride,
                                                                         const float* __restrict__ bias, int H, int relu, void* __restrict__ out, uint64_t ostride) {
  __shared__ __attribute__((aligned(16))) uint16_t wb[BG_LIN_WCHUNK * BG_EXT_WPITCH];   // phase 2's staging area first
  __shared__ __attribute__((aligned(16))) uint16_t xd[BG_LIN_ROWS * BG_EXT_DPITCH];
  __shared__ uint32_t hw[BG_LIN_ROWS * 2];
  __shared__ long long src[BG_ENC_RECS];
  const long long rec0 = (long long)blockIdx.x * BG_LIN_ROWS;
  bg_ext_load_hands<false>(rows, row_stride, index, store_rows, m, rec0, hw);
  bg_ext_build_dense<false>(rows, row_stride, index, store_rows, m, rec0, src, reinterpret_cast<uint32_t*>(wb), xd);   // (its barriers are behind hw's stores)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = wave * BG_LIN_TILE + bg_lin_frag_rc(lane);
  bg_lin_ab a[BG_EXT_STEPS];
  {
    const uint32_t lo = hw[2 * row], hi = hw[2 * row + 1];
    int q[BG_EXT_SLOTS];
#pragma unroll
    for (int s = 0; s < BG_EXT_SLOTS; s++) q[s] = bg_ext_hot_q(s, (int)(int8_t)((s < 4 ? lo : hi) >> (8 * (s & 3))), lane);
#pragma unroll
    for (int s = 0; s < BG_EXT_HOT_STEPS; s++) {
      bg_lin_u4 p;
#pragma unroll
      for (int j = 0; j < 8; j += 2) p[j / 2] = (uint32_t)bg_ext_hot_elem(q, s, j) | (uint32_t)bg_ext_hot_elem(q, s, j + 1) << 16;
      a[s] = __builtin_bit_cast(bg_lin_ab, p);
    }
#pragma unroll
    for (int s = BG_EXT_HOT_STEPS; s < BG_EXT_STEPS; s++) a[s] = bg_lin_ld_frag(xd + row * BG_EXT_DPITCH + bg_lin_frag_k(lane, s - BG_EXT_HOT_STEPS, 0));
  }
  const int vec = ((uintptr_t)weight & 15) == 0 && (wstride & 7) == 0 ? 8 : ((uintptr_t)weight & 3) == 0 && (wstride & 1) == 0 ? 2 : 1;
  const int nchunks = (H + BG_LIN_WCHUNK - 1) / BG_LIN_WCHUNK;
  const long long row_base = rec0 + wave * BG_LIN_TILE;
  for (int chunk = blockIdx.y; chunk < nchunks; chunk += gridDim.y) {
    const int n0 = chunk * BG_LIN_WCHUNK;
    const int nn = H - n0 < BG_LIN_WCHUNK ? H - n0 : BG_LIN_WCHUNK;   // 32 or 64
    __syncthreads();   // the previous chunk's fragments (the first time: the staging area and XD) are read
    if (vec == 8) bg_ext_stage_w<8>(weight, (uint32_t)wstride, n0, H, wb);
    else if (vec == 2) bg_ext_stage_w<2>(weight, (uint32_t)wstride, n0, H, wb);
    else bg_ext_stage_w<1>(weight, (uint32_t)wstride, n0, H, wb);
    __syncthreads();
    for (int t = 0; t < nn / BG_LIN_TILE; t++) {
      bg_lin_c16 acc;
#pragma unroll
      for (int g = 0; g < 16; g++) acc[g] = 0.f;
#pragma unroll
      for (int s = 0; s < BG_EXT_STEPS; s++) {
        const bg_lin_ab b = bg_lin_ld_frag(wb + t * BG_LIN_TILE * BG_EXT_WPITCH + bg_lin_frag_off(lane, s, BG_EXT_WPITCH));
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s], b, acc, 0, 0, 0);
        if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // four B fragments in flight, not 28: the A fragments leave no room for more
      }
      const int col = n0 + t * BG_LIN_TILE + bg_lin_acc_col(lane);
      const float bv = bias ? bias[col] : 0.f;
#pragma unroll
      for (int g = 0; g < 16; g++) {
        const long long r = row_base + bg_lin_acc_row(lane, g);
        if (r < m) bg_lin_emit<ODT>(out, (size_t)r * ostride + (size_t)col, bias ? acc[g] + bv : acc[g], relu);
      }
    }
  }
}

// dp, as bg_lin_dp gives it, in two steps with the element types compile-time constants (DBF16: dout is bfloat16, else float32; OUTK: 0 no ReLU, 1 the
// forward's output is float32, 2 bfloat16): the raw element of dout or out at (row i, unit n) by an unconditional load -- a row at or beyond m reads row
// `safe` (< m) instead --, then the value: rounded, +0.0 for such a row and where the output is not > 0.  Nothing branches, so a group of loads is issued
// back to back (the kernel fences the groups with sched_barrier: left alone, the scheduler waits for every load before it issues the next).
template <bool BF16>
__device__ __forceinline__ uint32_t bg_ext_raw(const void* __restrict__ p, uint64_t stride, long long i, int n, long long m, long long safe) {
  const size_t at = (size_t)(i < m ? i : safe) * stride + (size_t)n;
  return BF16 ? (uint32_t)reinterpret_cast<const uint16_t*>(p)[at] : reinterpret_cast<const uint32_t*>(p)[at];
}
template <bool DBF16, int OUTK>
__device__ __forceinline__ uint16_t bg_ext_dp(uint32_t raw_dout, uint32_t raw_out, bool in_range) {
  bool keep = in_range;
  if (OUTK != 0) keep = keep && (OUTK == 2 ? bg_lin_widen((uint16_t)raw_out) : __uint_as_float(raw_out)) > 0.f;
  const uint16_t v = DBF16 ? (uint16_t)raw_dout : bg_enc_bf16(raw_dout);
  return keep ? v : (uint16_t)0;
}

template <bool DBF16, int OUTK>
__global__ __launch_bounds__(BG_LIN_BLOCK) void bg_extractor_rows_grad_kernel(const uint8_t* __restrict__ rows, uint64_t row_stride, const int32_t* __restrict__ index,
                                                                              long long store_rows, long long m, const void* __restrict__ dout, uint64_t dstride,
                                                                              const void* __restrict__ out, uint64_t ostride, int H, long long per,
                                                                              float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) uint32_t stage[BG_EXT_STAGE_WORDS];
  __shared__ __attribute__((aligned(16))) uint16_t xt[BG_LIN_TILE * BG_LIN_TPITCH];
  __shared__ __attribute__((aligned(16))) uint32_t hw[BG_LIN_ROWS * 2];   // HB[8][128] bytes
  __shared__ long long src[BG_ENC_RECS];
  const uint8_t* const hb = reinterpret_cast<const uint8_t*>(hw);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int KT = BG_EXT_SPAN_TILES, NT = BG_LIN_NSPAN / BG_LIN_TILE / (BG_LIN_BLOCK / 64);   // 5 tiles of k; 2 unit tiles per wave
  const int tile0 = bg_ext_span_tile0(blockIdx.z), ntile = bg_ext_span_tiles(blockIdx.z);
  const bool dense = tile0 + ntile > BG_EXT_HOT_TILES;   // this span holds the dense tile (its last)
  // (ncol / acc / dbsum, the block range and the write-out of the partial are bg_linear_rows_grad_kernel's: shared helpers moved both kernels' text)
  int ncol[NT];      // the lane's unit in tile t, or -1: the tile is beyond H (uniform over the wave)
  int card[KT], hoff[KT];   // the card of the lane's column in k-tile kt and where its slot's bytes of the lane's 8 records start in HB
  bg_lin_c16 acc[NT][KT];
  float dbsum[NT];
#pragma unroll
  for (int kt = 0; kt < KT; kt++) {
    const int k = bg_ext_tile_k(tile0 + kt, lane);
    const bool hot = k < BG_EXT_HOT;
    card[kt] = hot ? bg_ext_card(k) : 0;
    hoff[kt] = (hot ? bg_ext_slot(k) : 0) * BG_LIN_ROWS + 8 * (lane >> 5);
  }
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const int tile_index = blockIdx.y * (BG_LIN_NSPAN / BG_LIN_TILE) + t * (BG_LIN_BLOCK / 64) + wave;
    ncol[t] = tile_index * BG_LIN_TILE < H ? tile_index * BG_LIN_TILE + bg_lin_frag_rc(lane) : -1;
    dbsum[t] = 0.f;
#pragma unroll
    for (int kt = 0; kt < KT; kt++)
#pragma unroll
      for (int g = 0; g < 16; g++) acc[t][kt][g] = 0.f;
  }
  const long long nblk = bg_lin_blocks(m);
  const long long b0 = (long long)blockIdx.x * per, b1 = b0 + per < nblk ? b0 + per : nblk;
  for (long long b = b0; b < b1; b++) {
    const long long rec0 = b * BG_LIN_ROWS;
    // every dp element of the block first, in groups of two k-steps of one unit tile: 16 to 32 loads in flight, then their values
    uint32_t dpw[NT][BG_LIN_ROWS / BG_LIN_KSTEP][4];
#pragma unroll
    for (int t = 0; t < NT; t++) {
      if (ncol[t] < 0) continue;
#pragma unroll
      for (int s2 = 0; s2 < BG_LIN_ROWS / BG_LIN_KSTEP; s2 += 2) {
        uint32_t rd[16], ro[16];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 16; e++) {
          const long long i = rec0 + bg_lin_frag_k(lane, s2 + (e >> 3), e & 7);
          rd[e] = bg_ext_raw<DBF16>(dout, dstride, i, ncol[t], m, rec0);
          ro[e] = OUTK != 0 ? bg_ext_raw<OUTK == 2>(out, ostride, i, ncol[t], m, rec0) : 0u;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
          const long long i = rec0 + bg_lin_frag_k(lane, s2 + (e >> 3), e & 7);
          const uint16_t lo = bg_ext_dp<DBF16, OUTK>(rd[e], ro[e], i < m), hi = bg_ext_dp<DBF16, OUTK>(rd[e + 1], ro[e + 1], i + 1 < m);
          dpw[t][s2 + (e >> 3)][(e & 7) / 2] = (uint32_t)lo | (uint32_t)hi << 16;
        }
      }
    }
    bg_ext_load_hands<true>(rows, row_stride, index, store_rows, m, rec0, hw);
    if (dense) bg_ext_build_dense<true>(rows, row_stride, index, store_rows, m, rec0, src, stage, xt);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < BG_LIN_ROWS / BG_LIN_KSTEP; s++) {
      bg_lin_ab af[KT];
#pragma unroll
      for (int kt = 0; kt < KT; kt++) {
        if (kt >= ntile) continue;
        if (tile0 + kt >= BG_EXT_HOT_TILES) { af[kt] = bg_lin_ld_frag(xt + bg_lin_frag_off(lane, s, BG_LIN_TPITCH)); continue; }
        const uint2 by = *reinterpret_cast<const uint2*>(__builtin_assume_aligned(hb + hoff[kt] + BG_LIN_KSTEP * s, 8));
        bg_lin_u4 p;
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          const uint32_t w = j < 4 ? by.x : by.y;
          const uint32_t lo = (w >> (8 * (j & 3))) & 0xffu, hi = (w >> (8 * ((j + 1) & 3))) & 0xffu;
          p[j / 2] = (lo == (uint32_t)card[kt] ? 0x3f80u : 0u) | (hi == (uint32_t)card[kt] ? 0x3f800000u : 0u);
        }
        af[kt] = __builtin_bit_cast(bg_lin_ab, p);
      }
#pragma unroll
      for (int t = 0; t < NT; t++) {
        if (ncol[t] < 0) continue;
        bg_lin_u4 pv;
#pragma unroll
        for (int w = 0; w < 4; w++) {
          pv[w] = dpw[t][s][w];
          dbsum[t] = dbsum[t] + bg_lin_widen((uint16_t)dpw[t][s][w]);   // (the order of bg_linear_rows_grad_kernel: k-step by k-step, element by element)
          dbsum[t] = dbsum[t] + bg_lin_widen((uint16_t)(dpw[t][s][w] >> 16));
        }
        const bg_lin_ab bf = __builtin_bit_cast(bg_lin_ab, pv);
#pragma unroll
        for (int kt = 0; kt < KT; kt++)
          if (kt < ntile) acc[t][kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[kt], bf, acc[t][kt], 0, 0, 0);
      }
    }
    __syncthreads();   // HB and XT are read before the next block overwrites them
  }
  float* const mine = part + (size_t)blockIdx.x * BG_EXT_PART_ROWS * (size_t)H;
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const float other = __shfl_xor(dbsum[t], 32);
    if (ncol[t] < 0) continue;
    const int n = ncol[t] - bg_lin_frag_rc(lane) + bg_lin_acc_col(lane);
#pragma unroll
    for (int kt = 0; kt < KT; kt++) {
      if (kt >= ntile) continue;
#pragma unroll
      for (int g = 0; g < 16; g++) mine[(size_t)((tile0 + kt) * BG_LIN_TILE + bg_lin_acc_row(lane, g)) * H + n] = acc[t][kt][g];
    }
    if (blockIdx.z == 0 && lane < 32) mine[(size_t)BG_EXT_KPAD * H + n] = dbsum[t] + other;
  }
}

// bg_linear.h's reduce over partials of [449][H] (a template, as every kernel here: see above)
template <int KCOLS>
__global__ __launch_bounds__(256) void bg_extractor_reduce_kernel(const float* __restrict__ part, long long groups, int H, float* __restrict__ dweight, uint64_t dwstride,
                                                                  float* __restrict__ dbias) {
  bg_lin_reduce<KCOLS, BG_EXT_KPAD>(part, groups, H, dweight, dwstride, dbias);
}
#endif  // BG_EXT_HOST
#endif
