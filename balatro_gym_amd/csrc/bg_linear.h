// bg_linear.h -- bg_linear_rows / bg_linear_rows_grad: the network's first layer, forward and weight gradient, straight from packed records.
//
// The layer's input is the row bg_encode_rows_ex writes as bfloat16 ("produced" / "fixed", with or without frozen statistics).  Of its 628 columns
// only the first 153 can be non-zero, so the product runs over 153 columns padded to 160 = ten k-steps of the matrix cores' 32x32x16 bfloat16
// instruction; the feature matrix never exists in HBM.  Phases 1-2 of the records-to-tile pipeline (bg_encode.h: bg_enc_stage_gather, bg_enc_fill_tile
// with the converter of bg_encode_gather_kernel / bg_norm_obs_gather_kernel) give a float32 tile of finished column values for 32 records; the tile is
// rounded to bfloat16 (bg_enc_bf16, the rounding of bg_encode_rows_ex) into the operand image the matrix cores read.
//
// The index arithmetic of the fragments is plain C++ behind BG_LIN_FN, so tests/test_linear_rows_host.py compiles it with g++ (define BG_LIN_HOST
// before including) and drives it through a scalar model of the instruction.
#ifndef BG_LINEAR_H
#define BG_LINEAR_H
#include <stdint.h>

#ifdef BG_LIN_HOST
#define BG_LIN_FN static inline
#else
#define BG_LIN_FN __host__ __device__ __forceinline__
#endif

#define BG_LIN_K 153    /* columns that can be non-zero: BG_ENC_PRODUCED_COLS */
#define BG_LIN_KPAD 160 /* the reduction the matrix cores run: padded with zeros */
#define BG_LIN_TILE 32  /* edge of an accumulator tile */
#define BG_LIN_KSTEP 16 /* reduction length of one instruction */
#define BG_LIN_ROWS 128 /* records of one pass of a workgroup: four sub-tiles of 32, as bg_encode_kernel stages them */
#define BG_LIN_NSPAN 256 /* output units of one workgroup of the gradient: two accumulator tiles per wave */
#define BG_LIN_PART_ROWS (BG_LIN_KPAD + 1) /* rows of a gradient partial: [160][H] of dweight^T, then [H] of dbias */
#define BG_LIN_MAX_WG 256 /* bound on the workgroups of a gradient (row groups x unit spans x, in bg_extractor.h, k spans): one per CU */

// ---- v_mfma_f32_32x32x16_bf16: D[32][32] += A[32][16] * B[16][32], one wave of 64 lanes ----
// Lane l holds 8 consecutive k of ONE row of A and of ONE column of B; its 16 accumulator registers are 16 rows of ONE column of D.
BG_LIN_FN int bg_lin_frag_rc(int lane) { return lane & 31; }                                        // row of A = column of B of the lane's fragment
BG_LIN_FN int bg_lin_frag_k(int lane, int step, int j) { return BG_LIN_KSTEP * step + 8 * (lane >> 5) + j; }   // reduction index of fragment element j, k-step `step`
BG_LIN_FN int bg_lin_acc_row(int lane, int reg) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }
BG_LIN_FN int bg_lin_acc_col(int lane) { return lane & 31; }
// element offset of the lane's fragment (8 consecutive elements) in an image [row of A | column of B][reduction index] of `pitch` elements per line
BG_LIN_FN int bg_lin_frag_off(int lane, int step, int pitch) { return bg_lin_frag_rc(lane) * pitch + bg_lin_frag_k(lane, step, 0); }
#ifdef BG_LIN_HOST
// The serial twins' scalar model of one instruction (bg_actor.h, bg_policy.h): acc[lane][g] += the sum over the step's 16 k, in ascending k, each product
// exact, every addition rounded to float32.  a(lane, j) / b(lane, j): element j of the lane's fragment, widened from bfloat16, fetched as the caller's kernel
// fetches it; the maps above place the operands and the results: they are what is under test.
template <class FA, class FB>
static inline void bg_lin_host_mfma(FA a, FB b, float acc[64][16]) {
  float A[BG_LIN_TILE][BG_LIN_KSTEP], B[BG_LIN_KSTEP][BG_LIN_TILE];
  for (int l = 0; l < 64; l++)
    for (int j = 0; j < 8; j++) {
      A[bg_lin_frag_rc(l)][bg_lin_frag_k(l, 0, j)] = a(l, j);
      B[bg_lin_frag_k(l, 0, j)][bg_lin_frag_rc(l)] = b(l, j);
    }
  for (int l = 0; l < 64; l++)
    for (int g = 0; g < 16; g++)
      for (int k = 0; k < BG_LIN_KSTEP; k++) acc[l][g] = acc[l][g] + A[bg_lin_acc_row(l, g)][k] * B[k][bg_lin_acc_col(l)];
}
#endif

// a gradient's split of m rows (this layer's and bg_extractor.h's): blocks of BG_LIN_ROWS rows, `per` consecutive blocks per row group, `groups` groups
// (= partials), for a grid of bg_lin_spans(H) x `kspans` workgroups per row group: kspans is 1 here, the k spans there
BG_LIN_FN int64_t bg_lin_blocks(int64_t m) { return (m + BG_LIN_ROWS - 1) / BG_LIN_ROWS; }
BG_LIN_FN int64_t bg_lin_spans(int H) { return (H + BG_LIN_NSPAN - 1) / BG_LIN_NSPAN; }
BG_LIN_FN int64_t bg_lin_blocks_per_group(int64_t m, int H, int kspans = 1) {
  const int64_t wg = kspans * bg_lin_spans(H), cap = BG_LIN_MAX_WG / wg > 0 ? BG_LIN_MAX_WG / wg : 1;
  return (bg_lin_blocks(m) + cap - 1) / cap;
}
BG_LIN_FN int64_t bg_lin_groups(int64_t m, int H, int kspans = 1) {
  const int64_t per = bg_lin_blocks_per_group(m, H, kspans);
  return (bg_lin_blocks(m) + per - 1) / per;
}
// the workspace of such a gradient: groups partials of [part_rows][H] float32; 0 where nothing is launched
BG_LIN_FN uint64_t bg_lin_workspace_bytes(int64_t m, int H, int kspans, int part_rows) {
  if (m <= 0 || H < 32 || H > 4096 || H % 32) return 0;
  return (uint64_t)bg_lin_groups(m, H, kspans) * (uint64_t)part_rows * (uint64_t)H * sizeof(float);
}
// max(v, +0.0) with a NaN kept
BG_LIN_FN float bg_lin_relu(float v) { return v > 0.f ? v : v != v ? v : 0.f; }

#ifndef BG_LIN_HOST
// ---- the kernels ----
// FORWARD, grid (ceil(m / 128), ysplit), 256 lanes = 4 waves:
//   1  four times phases 1-2 of the encode kernels for 32 records (gathered through the index; a record without a source is a row of +0.0), each
//      followed by the rounding of the 32 x 153 float32 tile to bfloat16 into XA[128][168] (columns 153..159 zero; 336-byte lines: 16-byte aligned
//      fragments);
//   2  wave w takes rows 32w..32w+31 of XA as ten A fragments into 40 registers, once;
//   3  for every chunk of 64 output units (chunks y, y + ysplit, ...): the 64 x 153 weights are read from the caller's matrix (bg_lin_stage_w: by
//      word when it is 4-byte aligned with an even pitch, else by element -- 2-byte alignment is all that is asked; consecutive lanes on consecutive
//      items, every load of a lane in flight before its first LDS store) into WB[64][168], over the LDS of phase 1 which is dead by then;
//      per 32 units a wave runs ten instructions over its A fragments and the B fragments of WB, adds the bias, applies the activation and stores its
//      32 x 32 tile: a register is one output row, the 32 lanes of a half-wave its 32 consecutive units.
// LDS 75.4 KB: two workgroups per CU.  ysplit spreads the chunks of a short call over more workgroups (phase 1 is then repeated per y).
// GRADIENT, grid (groups, ceil(H / 256)): a workgroup walks `per` blocks of 128 rows; per block phase 1 as above, but the rounding writes the
// TRANSPOSE XT[160][136] (line = column k of the input, 272 bytes); D'[k][n] = sum_i XT[k][i] * dp[i][n]: the A fragments are 16-byte reads of XT, the
// B fragment of a lane is 8 rows of ONE unit of dout, read from HBM directly (a half-wave reads 32 consecutive units of a row), masked by out > 0
// under ReLU and rounded to bfloat16; a wave keeps 2 x 5 accumulator tiles (160 registers) = all 160 k of its two unit tiles over all rows of the
// group, and the float32 sum of its dp values for dbias.  Partial p = [161][H] float32 in the workspace; bg_linear_reduce_kernel sums the partials in
// index order in float64.  No atomics: two calls give the same bits.
#define BG_LIN_BLOCK 256
#define BG_LIN_PITCH 168   /* bf16 elements of a line of XA / WB */
#define BG_LIN_TPITCH (BG_LIN_ROWS + 8) /* bf16 elements of a line of XT */
#define BG_LIN_WCHUNK 64
#define BG_LIN_STAGE_WORDS (BG_ENC_RECS * BG_ENC_REC_PITCH / 4 + BG_ENC_RECS * BG_LIN_K)
static_assert(BG_LIN_BLOCK == BG_ENC_BLOCK && BG_LIN_K == BG_ENC_PRODUCED_COLS && BG_LIN_K == BG_NORM_COLS, "phases 1-2 are the encode kernels'");
static_assert(BG_LIN_ROWS % BG_ENC_RECS == 0 && BG_LIN_ROWS / BG_LIN_TILE == BG_LIN_BLOCK / 64, "one sub-tile of records per wave");
static_assert(BG_LIN_PITCH % 8 == 0 && BG_LIN_TPITCH % 8 == 0 && BG_LIN_PITCH >= BG_LIN_KPAD, "fragments are 16-byte reads");
static_assert(BG_LIN_WCHUNK * BG_LIN_PITCH * 2 <= BG_LIN_STAGE_WORDS * 4, "a weight chunk fits the staging area it reuses");
static_assert((BG_ENC_RECS * BG_ENC_REC_PITCH) % 16 == 0, "the float32 tile behind the records stays 16-byte aligned");

typedef __bf16 bg_lin_ab __attribute__((ext_vector_type(8)));
typedef float bg_lin_c16 __attribute__((ext_vector_type(16)));
typedef uint32_t bg_lin_u4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bg_lin_ab bg_lin_ld_frag(const uint16_t* p) {
  return __builtin_bit_cast(bg_lin_ab, *reinterpret_cast<const bg_lin_u4*>(__builtin_assume_aligned(p, 16)));
}
__device__ __forceinline__ float bg_lin_widen(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }

// phases 1-2 for the 32 records [rec0, rec0 + nrec) of the call -> `tile`; ends behind a barrier.  nrec <= 0: nothing (uniform over the workgroup).
template <bool NORM>
__device__ __forceinline__ void bg_lin_tile32(const uint8_t* __restrict__ rows, uint64_t row_stride, const int32_t* __restrict__ index, long long store_rows,
                                              long long rec0, int nrec, const double* __restrict__ mean, const double* denom, double clip, long long* src,
                                              uint32_t* recs32, uint32_t* tile) {
  if (nrec <= 0) return;
  bg_enc_stage_gather(rows, row_stride, index, store_rows, rec0, nrec, src, recs32);
  __syncthreads();
  if (NORM) bg_enc_fill_tile<BG_LIN_K, true>(recs32, tile, rec0, nrec, src, BgNormConvert<true>{mean, 0, 1, denom, clip});
  else bg_enc_fill_tile<BG_LIN_K, true>(recs32, tile, rec0, nrec, src, BgEncConvert<BG_ENC_PRODUCED>{});
  __syncthreads();
}

// the BG_LIN_ROWS records from rec0 as bfloat16 into `x`: [row][k] of BG_LIN_PITCH (TRANSPOSED false) or [k][row] of BG_LIN_TPITCH; rows at or
// beyond m and columns 153..159 are +0.0.  Ends behind a barrier.
template <bool NORM, bool TRANSPOSED>
__device__ __forceinline__ void bg_lin_build_x(const uint8_t* __restrict__ rows, uint64_t row_stride, const int32_t* __restrict__ index, long long store_rows,
                                               long long m, long long rec0, const double* __restrict__ mean, const double* denom, double clip, long long* src,
                                               uint32_t* stage, uint16_t* x) {
  uint32_t* const recs32 = stage;
  uint32_t* const tile = stage + BG_ENC_RECS * BG_ENC_REC_PITCH / 4;
  for (int sub = 0; sub < BG_LIN_ROWS / BG_ENC_RECS; sub++) {
    const long long r0 = rec0 + sub * BG_ENC_RECS;
    const int nrec = (int)(m - r0 < BG_ENC_RECS ? m - r0 : BG_ENC_RECS);
    bg_lin_tile32<NORM>(rows, row_stride, index, store_rows, r0, nrec, mean, denom, clip, src, recs32, tile);
    for (int e = threadIdx.x; e < BG_ENC_RECS * BG_LIN_KPAD; e += BG_LIN_BLOCK) {
      int r, k;
      if (TRANSPOSED) { k = e / BG_ENC_RECS; r = e - k * BG_ENC_RECS; }
      else { r = e / BG_LIN_KPAD; k = e - r * BG_LIN_KPAD; }
      const uint16_t v = r < nrec && k < BG_LIN_K ? bg_enc_bf16(tile[r * BG_LIN_K + k]) : (uint16_t)0;
      if (TRANSPOSED) x[k * BG_LIN_TPITCH + sub * BG_ENC_RECS + r] = v;
      else x[(sub * BG_ENC_RECS + r) * BG_LIN_PITCH + k] = v;
    }
    __syncthreads();
  }
}

// A chunk of BG_LIN_WCHUNK units of the weight -> WB, every line padded to 160 with zeros (units at or beyond H: zeros).  All of a lane's loads are issued
// before its first LDS store (in batches of 20), so a chunk costs one or two trips to L2, not one per element.  W4 (the weight 4-byte aligned with an even row pitch, e.g. a
// [H, 628] tensor): a line is 76 words, element 152 and three words of padding; otherwise 160 elements.
template <bool W4>
__device__ __forceinline__ void bg_lin_stage_w(const uint16_t* __restrict__ weight, uint32_t wstride, int n0, int H, uint16_t* wb) {
  const uint16_t* const base = weight + (size_t)n0 * wstride;   // uniform; a lane's offsets below fit 32 bits (wstride <= 2**24: bg_linear_rows)
  // every load is unconditional -- a line at or beyond H reads the chunk's first element instead and is replaced by zero -- so a batch is 19 or 20
  // independent loads and no branch
  if (W4) {
    constexpr int WORDS = BG_LIN_K / 2, PER = BG_LIN_WCHUNK * WORDS / BG_LIN_BLOCK;   // 76 whole words of a line: 19 per lane
    static_assert(BG_LIN_WCHUNK * WORDS % BG_LIN_BLOCK == 0 && BG_LIN_K % 2 == 1 && BG_LIN_WCHUNK <= 64, "whole words per lane; element 152 by the first wave");
    uint32_t v[PER];
#pragma unroll
    for (int i = 0; i < PER; i++) {
      const int e = threadIdx.x + i * BG_LIN_BLOCK, n = e / WORDS, j = e - n * WORDS;
      const bool ok = n0 + n < H;
      const uint32_t w = *reinterpret_cast<const uint32_t*>(__builtin_assume_aligned(base + (ok ? (uint32_t)n * wstride + 2u * j : 0u), 4));
      v[i] = ok ? w : 0u;
    }
    uint32_t last = 0u;
    if (threadIdx.x < BG_LIN_WCHUNK) {
      const bool ok = n0 + (int)threadIdx.x < H;
      const uint16_t w = base[ok ? threadIdx.x * wstride + (BG_LIN_K - 1) : 0u];
      last = ok ? w : 0u;
    }
#pragma unroll
    for (int i = 0; i < PER; i++) {
      const int e = threadIdx.x + i * BG_LIN_BLOCK, n = e / WORDS, j = e - n * WORDS;
      *reinterpret_cast<uint32_t*>(wb + n * BG_LIN_PITCH + 2 * j) = v[i];
    }
    if (threadIdx.x < BG_LIN_WCHUNK) {   // element 152 and the padding to 160
      uint32_t* const tail = reinterpret_cast<uint32_t*>(wb + threadIdx.x * BG_LIN_PITCH + BG_LIN_K - 1);
      tail[0] = last; tail[1] = 0u; tail[2] = 0u; tail[3] = 0u;
    }
  } else {
    constexpr int PER = BG_LIN_WCHUNK * BG_LIN_KPAD / BG_LIN_BLOCK, BATCH = 20;
    static_assert(BG_LIN_WCHUNK * BG_LIN_KPAD % BG_LIN_BLOCK == 0 && PER % BATCH == 0, "whole batches per lane");
#pragma unroll 1
    for (int b0 = 0; b0 < PER; b0 += BATCH) {
      uint16_t v[BATCH];
#pragma unroll
      for (int i = 0; i < BATCH; i++) {
        const int e = threadIdx.x + (b0 + i) * BG_LIN_BLOCK, n = e / BG_LIN_KPAD, j = e - n * BG_LIN_KPAD;
        const bool ok = n0 + n < H && j < BG_LIN_K;
        const uint16_t w = base[ok ? (uint32_t)n * wstride + (uint32_t)j : 0u];
        v[i] = ok ? w : (uint16_t)0;
      }
#pragma unroll
      for (int i = 0; i < BATCH; i++) {
        const int e = threadIdx.x + (b0 + i) * BG_LIN_BLOCK, n = e / BG_LIN_KPAD, j = e - n * BG_LIN_KPAD;
        wb[n * BG_LIN_PITCH + j] = v[i];
      }
    }
  }
}

// one element of a forward's output: the activation, then the store as float32 or rounded to bfloat16
template <int ODT>
__device__ __forceinline__ void bg_lin_emit(void* out, size_t at, float v, int relu) {
  if (relu) v = bg_lin_relu(v);
  if (ODT == BG_ENC_F32) reinterpret_cast<float*>(out)[at] = v;
  else reinterpret_cast<uint16_t*>(out)[at] = bg_enc_bf16(__float_as_uint(v));
}

template <bool NORM, int ODT>
__global__ __launch_bounds__(BG_LIN_BLOCK, 2) void bg_linear_rows_kernel(const uint8_t* __restrict__ rows, uint64_t row_stride, const int32_t* __restrict__ index,
                                                                      long long store_rows, long long m, const double* __restrict__ mean,
                                                                      const double* __restrict__ var, double epsilon, double clip,
                                                                      const uint16_t* __restrict__ weight, uint64_t wstride, const float* __restrict__ bias, int H,
                                                                      int relu, void* __restrict__ out, uint64_t ostride) {
  __shared__ __attribute__((aligned(16))) uint32_t stage[BG_LIN_STAGE_WORDS];
  __shared__ __attribute__((aligned(16))) uint16_t xa[BG_LIN_ROWS * BG_LIN_PITCH];
  __shared__ long long src[BG_ENC_RECS];
  __shared__ double denom[NORM ? BG_LIN_K : 1];
  const long long rec0 = (long long)blockIdx.x * BG_LIN_ROWS;
  if (NORM && threadIdx.x < BG_LIN_K) denom[threadIdx.x] = bg_norm_denom(var[threadIdx.x], epsilon);   // (bg_enc_stage_gather's barrier is in front of its use)
  bg_lin_build_x<NORM, false>(rows, row_stride, index, store_rows, m, rec0, mean, denom, clip, src, stage, xa);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  bg_lin_ab a[BG_LIN_KPAD / BG_LIN_KSTEP];
#pragma unroll
  for (int s = 0; s < BG_LIN_KPAD / BG_LIN_KSTEP; s++) a[s] = bg_lin_ld_frag(xa + wave * BG_LIN_TILE * BG_LIN_PITCH + bg_lin_frag_off(lane, s, BG_LIN_PITCH));
  uint16_t* const wb = reinterpret_cast<uint16_t*>(stage);
  const bool w4 = ((uintptr_t)weight & 3) == 0 && (wstride & 1) == 0;
  const int nchunks = (H + BG_LIN_WCHUNK - 1) / BG_LIN_WCHUNK;
  const long long row_base = rec0 + wave * BG_LIN_TILE;
  for (int chunk = blockIdx.y; chunk < nchunks; chunk += gridDim.y) {
    const int n0 = chunk * BG_LIN_WCHUNK;
    const int nn = H - n0 < BG_LIN_WCHUNK ? H - n0 : BG_LIN_WCHUNK;   // 32 or 64
    __syncthreads();   // the previous chunk's fragments are read
    if (w4) bg_lin_stage_w<true>(weight, (uint32_t)wstride, n0, H, wb);
    else bg_lin_stage_w<false>(weight, (uint32_t)wstride, n0, H, wb);
    __syncthreads();
    for (int t = 0; t < nn / BG_LIN_TILE; t++) {
      bg_lin_c16 acc;
#pragma unroll
      for (int g = 0; g < 16; g++) acc[g] = 0.f;
#pragma unroll
      for (int s = 0; s < BG_LIN_KPAD / BG_LIN_KSTEP; s++) {
        const bg_lin_ab b = bg_lin_ld_frag(wb + t * BG_LIN_TILE * BG_LIN_PITCH + bg_lin_frag_off(lane, s, BG_LIN_PITCH));
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s], b, acc, 0, 0, 0);
      }
      const int col = n0 + t * BG_LIN_TILE + bg_lin_acc_col(lane);
      const float bv = bias ? bias[col] : 0.f;
#pragma unroll
      for (int g = 0; g < 16; g++) {
        const long long row = row_base + bg_lin_acc_row(lane, g);
        if (row < m) bg_lin_emit<ODT>(out, (size_t)row * ostride + (size_t)col, bias ? acc[g] + bv : acc[g], relu);
      }
    }
  }
}

// one element of dp: dout rounded to bfloat16, +0.0 for a row at or beyond m and, under ReLU, where the forward's output is not > 0
__device__ __forceinline__ uint16_t bg_lin_dp(const void* __restrict__ dout, int dout_bf16, uint64_t dstride, const void* __restrict__ out, int out_bf16,
                                              uint64_t ostride, long long i, int n, long long m) {
  if (i >= m) return 0;
  if (out) {
    const size_t at = (size_t)i * ostride + (size_t)n;
    const float o = out_bf16 ? bg_lin_widen(reinterpret_cast<const uint16_t*>(out)[at]) : reinterpret_cast<const float*>(out)[at];
    if (!(o > 0.f)) return 0;
  }
  const size_t at = (size_t)i * dstride + (size_t)n;
  return dout_bf16 ? reinterpret_cast<const uint16_t*>(dout)[at] : bg_enc_bf16(__float_as_uint(reinterpret_cast<const float*>(dout)[at]));
}

template <bool NORM>
__global__ __launch_bounds__(BG_LIN_BLOCK) void bg_linear_rows_grad_kernel(const uint8_t* __restrict__ rows, uint64_t row_stride, const int32_t* __restrict__ index,
                                                                           long long store_rows, long long m, const double* __restrict__ mean,
                                                                           const double* __restrict__ var, double epsilon, double clip,
                                                                           const void* __restrict__ dout, int dout_bf16, uint64_t dstride,
                                                                           const void* __restrict__ out, int out_bf16, uint64_t ostride, int H,
                                                                           long long per, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) uint32_t stage[BG_LIN_STAGE_WORDS];
  __shared__ __attribute__((aligned(16))) uint16_t xt[BG_LIN_KPAD * BG_LIN_TPITCH];
  __shared__ long long src[BG_ENC_RECS];
  __shared__ double denom[NORM ? BG_LIN_K : 1];
  if (NORM && threadIdx.x < BG_LIN_K) denom[threadIdx.x] = bg_norm_denom(var[threadIdx.x], epsilon);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int KT = BG_LIN_KPAD / BG_LIN_TILE, NT = BG_LIN_NSPAN / BG_LIN_TILE / (BG_LIN_BLOCK / 64);   // 5 tiles of k; 2 unit tiles per wave
  int ncol[NT];      // the lane's unit in tile t, or -1: the tile is beyond H (uniform over the wave)
  bg_lin_c16 acc[NT][KT];
  float dbsum[NT];
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
    bg_lin_build_x<NORM, true>(rows, row_stride, index, store_rows, m, rec0, mean, denom, clip, src, stage, xt);
    for (int s = 0; s < BG_LIN_ROWS / BG_LIN_KSTEP; s++) {
#pragma unroll
      for (int t = 0; t < NT; t++) {
        if (ncol[t] < 0) continue;
        uint32_t p[4];
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          const uint16_t lo = bg_lin_dp(dout, dout_bf16, dstride, out, out_bf16, ostride, rec0 + bg_lin_frag_k(lane, s, j), ncol[t], m);
          const uint16_t hi = bg_lin_dp(dout, dout_bf16, dstride, out, out_bf16, ostride, rec0 + bg_lin_frag_k(lane, s, j + 1), ncol[t], m);
          dbsum[t] = dbsum[t] + bg_lin_widen(lo);
          dbsum[t] = dbsum[t] + bg_lin_widen(hi);
          p[j / 2] = (uint32_t)lo | (uint32_t)hi << 16;
        }
        bg_lin_u4 pv;
        pv[0] = p[0]; pv[1] = p[1]; pv[2] = p[2]; pv[3] = p[3];
        const bg_lin_ab bf = __builtin_bit_cast(bg_lin_ab, pv);
#pragma unroll
        for (int kt = 0; kt < KT; kt++) {
          const bg_lin_ab af = bg_lin_ld_frag(xt + kt * BG_LIN_TILE * BG_LIN_TPITCH + bg_lin_frag_off(lane, s, BG_LIN_TPITCH));
          acc[t][kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc[t][kt], 0, 0, 0);
        }
      }
    }
    __syncthreads();   // XT is read before the next block overwrites it
  }
  float* const mine = part + (size_t)blockIdx.x * BG_LIN_PART_ROWS * (size_t)H;
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const float other = __shfl_xor(dbsum[t], 32);
    if (ncol[t] < 0) continue;
    const int n = ncol[t] - bg_lin_frag_rc(lane) + bg_lin_acc_col(lane);
#pragma unroll
    for (int kt = 0; kt < KT; kt++)
#pragma unroll
      for (int g = 0; g < 16; g++) mine[(size_t)(kt * BG_LIN_TILE + bg_lin_acc_row(lane, g)) * H + n] = acc[t][kt][g];
    if (lane < 32) mine[(size_t)BG_LIN_KPAD * H + n] = dbsum[t] + other;
  }
}

// dweight[n][k] (k < K) / dbias[n] = the elements of the partials [KPAD + 1][H] summed in index order in float64, rounded once: the body of this layer's
// reduce kernel and of bg_extractor.h's
template <int K, int KPAD>
__device__ __forceinline__ void bg_lin_reduce(const float* __restrict__ part, long long groups, int H, float* __restrict__ dweight, uint64_t dwstride,
                                              float* __restrict__ dbias) {
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long long)(KPAD + 1) * H) return;
  const int k = (int)(item / H), n = (int)(item - (long long)k * H);
  if (k >= K && (k != KPAD || !dbias)) return;
  double s = 0.0;
  for (long long p = 0; p < groups; p++) s = s + (double)part[(size_t)p * (KPAD + 1) * (size_t)H + (size_t)item];
  if (k < K) dweight[(size_t)n * dwstride + k] = (float)s;
  else dbias[n] = (float)s;
}
__global__ __launch_bounds__(256) void bg_linear_reduce_kernel(const float* __restrict__ part, long long groups, int H, float* __restrict__ dweight, uint64_t dwstride,
                                                               float* __restrict__ dbias) {
  bg_lin_reduce<BG_LIN_K, BG_LIN_KPAD>(part, groups, H, dweight, dwstride, dbias);
}
#endif  // BG_LIN_HOST
#endif
