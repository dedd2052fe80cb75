// bg_norm.h -- bg_norm_obs_rows / bg_norm_reward_rows: SB3's VecNormalize(norm_obs, norm_reward) over [K, N] packed records.
//
//   bg_norm_obs_rows     per step t a RunningMeanStd update of the 153 PRODUCED columns with the batch of N records (t, 0..N-1), then
//                        clip((x - mean) / sqrt(var + epsilon)) with the statistics after that update, as float32 / bf16
//   bg_norm_reward_rows  ret = ret * gamma + reward per env, a RunningMeanStd update with the N returns, clip(reward / sqrt(var + epsilon)),
//                        ret = 0 where the record's terminated byte is set
//
// What is bit for bit numpy and what is bounded (include/balatro_mi355x.h has the text): everything BEHIND the cross-env reduction -- the
// RunningMeanStd merge chain, the normalisation, the return recurrence -- is the float64 expression of VecNormalize, operation by operation, in
// its order of evaluation; the library is built with -ffp-contract=off, `/` and sqrt are IEEE operations.  The reduction itself (batch mean,
// batch population variance over the N envs) cannot be numpy's to the bit: numpy's order of additions is an implementation detail.  Here it is
// (n, mean, M2) triples merged in a FIXED tree, so the same inputs give the same bits on every call, and a column that is constant over the batch
// has batch variance exactly 0.0.
// DEVIATION, on purpose: the batch moments are those of float64(x) for every column.  SB3 sums the float32 key `progress_ratio` in float32
// (numpy.mean / numpy.var of a float32 array accumulate in float32); these moments are the more accurate ones.
//
// The per-element and per-step arithmetic is plain C++ behind BG_NORM_FN, so the text the GPU runs compiles with g++ (define BG_NORM_HOST
// before including; the pattern of bg_gae.h / tests/test_gae_rows_host.py).
#ifndef BG_NORM_H
#define BG_NORM_H
#include <stdint.h>
#ifdef BG_NORM_HOST
#include <math.h>
#ifndef BG_ENC_HOST
#define BG_ENC_HOST
#endif
#define BG_NORM_FN static inline
#else
#define BG_NORM_FN __host__ __device__ __forceinline__
#endif
#include "bg_encode.h" // the PRODUCED column table, bg_enc_word, bg_enc_bf16
static_assert(BG_NORM_COLS == BG_ENC_PRODUCED_COLS, "VecNormalize's statistics are those of the PRODUCED columns");

// ---- one column of one record as float64: numpy's `x.astype(float64)` of the key's own dtype (exact but for |int64| > 2**53: nearest even) ----
BG_NORM_FN double bg_norm_value64(const uint8_t* rec, uint32_t d) {
  const uint32_t off = BG_ENC_OFF(d), type = BG_ENC_TYPE(d);
  const uint32_t lo = bg_enc_word(rec, off & ~3u);
  if (type == BG_ENC_SRC_F32) { float f; __builtin_memcpy(&f, &lo, 4); return (double)f; }
  if (type == BG_ENC_SRC_I64) return (double)(int64_t)((uint64_t)bg_enc_word(rec, off + 4u) << 32 | lo);
  const uint32_t v = lo >> ((off & 3u) * 8u);
  return (double)(type == BG_ENC_SRC_I8 ? (int32_t)(int8_t)v : type == BG_ENC_SRC_I16 ? (int32_t)(int16_t)v : (int32_t)v);
}
BG_NORM_FN double bg_norm_reward64(const uint8_t* rec) {
  double r;
  __builtin_memcpy(&r, __builtin_assume_aligned(rec + BG_ROW_REWARD, 8), 8);
  return r;
}

// ---- partial moments: n samples, their mean, M2 = sum of (x - mean)**2 ----
struct BgMoments { double n, mean, m2; };
BG_NORM_FN BgMoments bg_norm_none() { BgMoments o; o.n = 0.0; o.mean = 0.0; o.m2 = 0.0; return o; }
BG_NORM_FN BgMoments bg_norm_one(double x) { BgMoments o; o.n = 1.0; o.mean = x; o.m2 = 0.0; return o; }
// The pairwise merge (Chan et al.): `a` is the LEFT operand -- the merge is not symmetric in its roundings, so every tree below fixes who is left.
// Two parts of one constant column merge to that constant and M2 = 0.0 exactly (delta is 0.0).
BG_NORM_FN BgMoments bg_norm_merge(BgMoments a, BgMoments b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  const double n = a.n + b.n, delta = b.mean - a.mean;
  BgMoments o;
  o.n = n;
  o.mean = a.mean + delta * b.n / n;
  o.m2 = a.m2 + b.m2 + delta * delta * a.n * b.n / n;
  return o;
}
// The leaf of the observation tree: up to BG_NORM_TILE values of one column, two passes over values shifted by the first one (a difference of
// two such values is exact for integers below 2**53; a constant tile gives d = 0.0 everywhere, so mean = the constant and M2 = 0.0 exactly).
#define BG_NORM_TILE 32
BG_NORM_FN BgMoments bg_norm_tile(const double* v, int n) {   // 1 <= n <= BG_NORM_TILE
  const double p = v[0];
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < BG_NORM_TILE; i++)
    if (i < n) s = s + (v[i] - p);
  const double md = s / (double)n;
  double m2 = 0.0;
#pragma unroll
  for (int i = 0; i < BG_NORM_TILE; i++)
    if (i < n) { const double d = (v[i] - p) - md; m2 = m2 + d * d; }
  BgMoments o;
  o.n = (double)n; o.mean = p + md; o.m2 = m2;
  return o;
}
BG_NORM_FN double bg_norm_batch_var(BgMoments m) { return m.m2 / m.n; }   // population variance

// ---- RunningMeanStd.update_from_moments, float64, in numpy's order of evaluation (left to right) ----
struct BgRms { double mean, var, count; };
BG_NORM_FN BgRms bg_norm_rms_update(BgRms s, double bm, double bv, double n) {
  const double delta = bm - s.mean;
  const double tot = s.count + n;
  BgRms o;
  o.mean = s.mean + delta * n / tot;
  const double m_a = s.var * s.count;
  const double m_b = bv * n;
  const double m_2 = m_a + m_b + (delta * delta) * s.count * n / (s.count + n);
  o.var = m_2 / (s.count + n);
  o.count = n + s.count;
  return o;
}

// ---- the normalisation ----
BG_NORM_FN double bg_norm_denom(double var, double epsilon) { return sqrt(var + epsilon); }
BG_NORM_FN double bg_norm_clip(double z, double c) { return z < -c ? -c : z > c ? c : z; }   // numpy.clip: a NaN stays a NaN
// clip((obs - mean) / sqrt(var + epsilon), -clip_obs, clip_obs).astype(float32), as float32 bits
BG_NORM_FN uint32_t bg_norm_obs_bits(double x, double mean, double denom, double clip) {
  return bg_enc_float_bits((float)bg_norm_clip((x - mean) / denom, clip));
}
// returns = returns * gamma + reward;  clip(reward / sqrt(ret_rms.var + epsilon), -clip_reward, clip_reward);  returns[done] = 0
BG_NORM_FN double bg_norm_ret_step(double ret, double gamma, double r) { return ret * gamma + r; }
BG_NORM_FN double bg_norm_reward(double r, double denom, double clip) { return bg_norm_clip(r / denom, clip); }
BG_NORM_FN double bg_norm_ret_done(double ret, bool done) { return done ? 0.0 : ret; }

#ifndef BG_NORM_HOST
// ---- the kernels ----
// Observation call, update != 0, four launches on the caller's stream:
//   1  bg_norm_obs_partials   grid K * ceil(N / 256): a workgroup of 192 lanes takes 256 consecutive envs of one step in 8 tiles of 32 records, each
//      read from HBM once, 16 bytes per lane, into LDS (bg_enc_stage: whole-line reads).  Lane = column (153 of 192): it decodes its
//      column of the tile's records into registers, takes the tile's moments (bg_norm_tile) and merges them, tile after tile, into its triple;
//      one division per column and tile, not per element.  The triple (mean, M2; n follows from the chunk index) goes to the workspace.
//   2  bg_norm_obs_combine    grid K, lane = column: the chunks of a step merged left to right -> batch mean / batch variance of the step.
//   3  bg_norm_obs_chain      one workgroup, lane = column: the K RunningMeanStd updates in order; per step the mean and sqrt(var + epsilon) the rows of
//      that step are normalised with go to the workspace (a sqrt per column and step instead of per element), the final statistics to the caller.
//   4  bg_norm_obs_kernel     the records-to-tile pipeline of bg_encode.h with BgNormConvert in phase 2: (x - mean) / denom, clip, convert, in float64,
//      into the float32 tile.
// update == 0: a one-step launch of 3 that only takes the square roots of the frozen statistics, then 4.
// Every order of merging is fixed by indices alone: no atomics, nothing depends on scheduling.
#define BG_NORM_PBLOCK 192
#define BG_NORM_CHUNK 256 /* envs of a partial: BG_NORM_CHUNK / BG_NORM_TILE tiles */
static_assert(BG_NORM_PBLOCK >= BG_NORM_COLS && BG_NORM_CHUNK % BG_NORM_TILE == 0 && BG_NORM_TILE == BG_ENC_RECS, "lane = column; tiles as bg_encode_rows stages them");

__global__ __launch_bounds__(BG_NORM_PBLOCK) void bg_norm_obs_partials(const uint8_t* __restrict__ rows, uint64_t row_stride, long long N, long long nchunks,
                                                                       double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) uint32_t recs32[BG_NORM_TILE * BG_ENC_REC_PITCH / 4];
  const uint8_t* const recs = reinterpret_cast<const uint8_t*>(recs32);
  const long long t = blockIdx.x / nchunks, chunk = blockIdx.x - t * nchunks;
  const long long e0 = chunk * BG_NORM_CHUNK;
  const int nenv = (int)(N - e0 < BG_NORM_CHUNK ? N - e0 : BG_NORM_CHUNK);
  const int c = threadIdx.x;
  const uint32_t desc = c < BG_NORM_COLS ? BgEncTab<BG_ENC_PRODUCED>::t.d[c] : 0u;
  BgMoments acc = bg_norm_none();
  for (int r0 = 0; r0 < nenv; r0 += BG_NORM_TILE) {
    const int nrec = nenv - r0 < BG_NORM_TILE ? nenv - r0 : BG_NORM_TILE;
    const size_t rec0 = (size_t)t * (size_t)N + (size_t)(e0 + r0);
    if (r0) __syncthreads();
    bg_enc_stage<BG_NORM_PBLOCK>(rows, row_stride, nrec, recs32, [rec0](int r) { return rec0 + r; });
    __syncthreads();
    if (c < BG_NORM_COLS) {
      double v[BG_NORM_TILE];
#pragma unroll
      for (int i = 0; i < BG_NORM_TILE; i++) v[i] = i < nrec ? bg_norm_value64(recs + i * BG_ENC_REC_PITCH, desc) : 0.0;
      acc = bg_norm_merge(acc, bg_norm_tile(v, nrec));
    }
  }
  if (c < BG_NORM_COLS) {
    double* const o = part + ((size_t)t * (size_t)nchunks + (size_t)chunk) * (2 * BG_NORM_COLS);
    o[c] = acc.mean;
    o[BG_NORM_COLS + c] = acc.m2;
  }
}

__global__ __launch_bounds__(BG_NORM_PBLOCK) void bg_norm_obs_combine(const double* __restrict__ part, long long N, long long nchunks, double* __restrict__ mom) {
  const int c = threadIdx.x;
  if (c >= BG_NORM_COLS) return;
  const size_t t = blockIdx.x;
  BgMoments acc = bg_norm_none();
  for (long long k = 0; k < nchunks; k++) {
    const double* const p = part + (t * (size_t)nchunks + (size_t)k) * (2 * BG_NORM_COLS);
    BgMoments b;
    b.n = (double)(N - k * BG_NORM_CHUNK < BG_NORM_CHUNK ? N - k * BG_NORM_CHUNK : BG_NORM_CHUNK);
    b.mean = p[c]; b.m2 = p[BG_NORM_COLS + c];
    acc = bg_norm_merge(acc, b);
  }
  mom[t * (2 * BG_NORM_COLS) + c] = acc.mean;
  mom[t * (2 * BG_NORM_COLS) + BG_NORM_COLS + c] = bg_norm_batch_var(acc);
}

// UPDATE: stat[t] = (mean, denom) after the update with step t's moments, and the caller's statistics are written; else stat[0] from the frozen statistics.
template <bool UPDATE>
__global__ __launch_bounds__(BG_NORM_PBLOCK) void bg_norm_obs_chain(const double* __restrict__ mom, int K, double n, double epsilon, double* mean_io, double* var_io,
                                                                    double* count_io, double* __restrict__ stat) {
  const int c = threadIdx.x < BG_NORM_COLS ? threadIdx.x : 0;   // the spare lanes shadow column 0 and store nothing
  const bool mine = threadIdx.x < BG_NORM_COLS;
  BgRms s;
  s.mean = mean_io[c]; s.var = var_io[c]; s.count = count_io[0];
  if (!UPDATE) {
    if (mine) {
      stat[c] = s.mean;
      stat[BG_NORM_COLS + c] = bg_norm_denom(s.var, epsilon);
    }
    return;
  }
  __syncthreads();   // every lane has read the shared count before lane 0 writes it
  if (!mine) return;
  for (int t = 0; t < K; t++) {
    s = bg_norm_rms_update(s, mom[(size_t)t * (2 * BG_NORM_COLS) + c], mom[(size_t)t * (2 * BG_NORM_COLS) + BG_NORM_COLS + c], n);
    stat[(size_t)t * (2 * BG_NORM_COLS) + c] = s.mean;
    stat[(size_t)t * (2 * BG_NORM_COLS) + BG_NORM_COLS + c] = bg_norm_denom(s.var, epsilon);
  }
  mean_io[c] = s.mean;
  var_io[c] = s.var;
  if (c == 0) count_io[0] = s.count;
}

// st: the 153 means followed by the 153 sqrt(var + epsilon) the record is normalised with; SPLIT (the GATHER variant): the roots are at dn instead
template <int S, bool SPLIT>
__device__ __forceinline__ void bg_norm_convert_slice(const uint8_t* rec, const double* __restrict__ st, const double* __restrict__ dn, double clip, uint32_t* dst) {
  constexpr int CH = (BG_NORM_COLS + BG_ENC_SLICES - 1) / BG_ENC_SLICES;
#pragma unroll
  for (int i = S * CH; i < (S + 1) * CH; i++)
    if (i < BG_NORM_COLS) dst[i] = bg_norm_obs_bits(bg_norm_value64(rec, BgEncTab<BG_ENC_PRODUCED>::t.d[i]), st[i], SPLIT ? dn[i] : st[BG_NORM_COLS + i], clip);
}

// the converter of phase 2 (bg_encode.h) with statistics.  Record i of the call belongs to step i / N: it is normalised with stat + (i / N) * step_stride
// (step_stride 0: frozen statistics, one set for every record)
template <bool SPLIT>
struct BgNormConvert {
  const double* stat;
  size_t step_stride;
  long long N;
  const double* dn;
  double clip;
  template <int S>
  __device__ __forceinline__ void operator()(std::integral_constant<int, S>, const uint8_t* rec, long long i, uint32_t* dst) const {
    bg_norm_convert_slice<S, SPLIT>(rec, stat + (size_t)(i / N) * step_stride, dn, clip, dst);
  }
};

// LAYOUT BG_ENC_PRODUCED | BG_ENC_FIXED; DT / ST as bg_encode_kernel; FIXED's never-filled columns are (0 - 0) / sqrt(var + epsilon) = +0.0, which is
// what bg_enc_store writes for them.
template <int LAYOUT, int DT, int ST>
__global__ __launch_bounds__(BG_ENC_BLOCK) void bg_norm_obs_kernel(const uint8_t* __restrict__ rows, uint64_t row_stride, long long m, long long N,
                                                                   const double* __restrict__ stat, size_t stat_step_stride, double clip, void* __restrict__ out,
                                                                   uint64_t pitch) {
  bg_enc_body<LAYOUT, DT, ST, false>(rows, row_stride, m, out, pitch, nullptr, 0, BgNormConvert<false>{stat, stat_step_stride, N, nullptr, clip});
}
// output row i from record index[i] (NULL: record i), normalised with the frozen statistics mean / var (bg_encode_rows_ex).  The call has no workspace,
// so lane c < 153 takes sqrt(var[c] + epsilon) -- the expression and the bits of bg_norm_obs_chain<false> -- into LDS once per workgroup (1 224 bytes:
// still five workgroups per CU; bg_enc_stage_gather's barrier is in front of its use).  A record without a source becomes a row of +0.0, not of
// normalised zeros.
template <int LAYOUT, int DT, int ST>
__global__ __launch_bounds__(BG_ENC_BLOCK) void bg_norm_obs_gather_kernel(const uint8_t* __restrict__ rows, uint64_t row_stride, const int32_t* __restrict__ index,
                                                                          long long store_rows, long long m, const double* __restrict__ mean,
                                                                          const double* __restrict__ var, double epsilon, double clip, void* __restrict__ out,
                                                                          uint64_t pitch) {
  __shared__ double denom[BG_NORM_COLS];
  if (threadIdx.x < BG_NORM_COLS) denom[threadIdx.x] = bg_norm_denom(var[threadIdx.x], epsilon);
  bg_enc_body<LAYOUT, DT, ST, true>(rows, row_stride, m, out, pitch, index, store_rows, BgNormConvert<true>{mean, 0, 1, denom, clip});
}

// Reward call, update != 0, four launches:
//   1  bg_norm_ret_partials  bg_gae_kernel's shape: lane = env, ONE wave per workgroup, K walked forwards in batches of 16 steps whose loads (reward,
//      terminated byte) are all in flight before the first is used.  Per step the wave's 64 returns are merged in a fixed shuffle tree (lane i takes
//      lane i + 1, 2, 4, .. as its RIGHT operand; lane 0 ends with the wave's triple) and lane 0 stores (mean, M2).  The carry is read once and
//      written once.
//   2  bg_norm_ret_combine   grid K, one wave: lane i merges its run of consecutive chunks left to right, then the same tree -> batch moments.
//   3  bg_norm_ret_chain     one lane: the K RunningMeanStd updates, sqrt(var + epsilon) per step to the workspace, the final statistics to the caller.
//   4  bg_norm_reward_kernel lane = (step, env): clip(reward / denom[t]).
// update == 0: 3 (frozen: one square root) and 4.
#define BG_NORM_RBLOCK 64
#define BG_NORM_RBATCH 16

__device__ __forceinline__ BgMoments bg_norm_wave_tree(BgMoments a) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    BgMoments b;
    b.n = __shfl_down(a.n, off, 64); b.mean = __shfl_down(a.mean, off, 64); b.m2 = __shfl_down(a.m2, off, 64);
    if ((int)(threadIdx.x & 63) + off >= 64) b = bg_norm_none();   // no lane there: the shuffle returned the lane's own triple
    a = bg_norm_merge(a, b);
  }
  return a;
}

__global__ __launch_bounds__(BG_NORM_RBLOCK) void bg_norm_ret_partials(const uint8_t* __restrict__ rows, uint64_t row_stride, int K, long long N, long long nchunks,
                                                                       double gamma, double* __restrict__ carry, double* __restrict__ part) {
  const long long e = (long long)blockIdx.x * BG_NORM_RBLOCK + threadIdx.x;
  const bool live = e < N;   // a lane beyond N stays for the shuffles and contributes the empty triple
  double ret = live ? carry[e] : 0.0;
  for (int t0 = 0; t0 < K; t0 += BG_NORM_RBATCH) {
    double r64[BG_NORM_RBATCH];
    uint8_t dn[BG_NORM_RBATCH];
#pragma unroll
    for (int j = 0; j < BG_NORM_RBATCH; j++) {
      const int t = t0 + j;
      r64[j] = 0.0; dn[j] = 0;
      if (t < K && live) {
        const uint8_t* const rec = rows + ((size_t)t * (size_t)N + (size_t)e) * row_stride;
        r64[j] = bg_norm_reward64(rec);
        dn[j] = rec[BG_ROW_TERMINATED];
      }
    }
#pragma unroll
    for (int j = 0; j < BG_NORM_RBATCH; j++) {
      const int t = t0 + j;
      if (t < K) {   // uniform over the wave
        ret = bg_norm_ret_step(ret, gamma, r64[j]);
        const BgMoments w = bg_norm_wave_tree(live ? bg_norm_one(ret) : bg_norm_none());
        if (threadIdx.x == 0) {
          double* const o = part + ((size_t)t * (size_t)nchunks + (size_t)blockIdx.x) * 2;
          o[0] = w.mean; o[1] = w.m2;
        }
        ret = bg_norm_ret_done(ret, dn[j] != 0);
      }
    }
  }
  if (live) carry[e] = ret;
}

__global__ __launch_bounds__(BG_NORM_RBLOCK) void bg_norm_ret_combine(const double* __restrict__ part, long long N, long long nchunks, double* __restrict__ mom) {
  const size_t t = blockIdx.x;
  const long long per = (nchunks + 63) / 64;
  BgMoments acc = bg_norm_none();
  for (long long k = (long long)threadIdx.x * per; k < ((long long)threadIdx.x + 1) * per && k < nchunks; k++) {
    const double* const p = part + (t * (size_t)nchunks + (size_t)k) * 2;
    BgMoments b;
    b.n = (double)(N - k * BG_NORM_RBLOCK < BG_NORM_RBLOCK ? N - k * BG_NORM_RBLOCK : BG_NORM_RBLOCK);
    b.mean = p[0]; b.m2 = p[1];
    acc = bg_norm_merge(acc, b);
  }
  acc = bg_norm_wave_tree(acc);
  if (threadIdx.x == 0) { mom[t * 2] = acc.mean; mom[t * 2 + 1] = bg_norm_batch_var(acc); }
}

template <bool UPDATE>
__global__ __launch_bounds__(64) void bg_norm_ret_chain(const double* __restrict__ mom, int K, double n, double epsilon, double* stats_io, double* __restrict__ denom) {
  if (threadIdx.x) return;
  BgRms s;
  s.mean = stats_io[0]; s.var = stats_io[1]; s.count = stats_io[2];
  if (!UPDATE) { denom[0] = bg_norm_denom(s.var, epsilon); return; }
  for (int t = 0; t < K; t++) {
    s = bg_norm_rms_update(s, mom[(size_t)t * 2], mom[(size_t)t * 2 + 1], n);
    denom[t] = bg_norm_denom(s.var, epsilon);
  }
  stats_io[0] = s.mean; stats_io[1] = s.var; stats_io[2] = s.count;
}

__global__ __launch_bounds__(256) void bg_norm_reward_kernel(const uint8_t* __restrict__ rows, uint64_t row_stride, long long m, long long N, const double* __restrict__ denom,
                                                             int denom_per_step, double clip, double* __restrict__ rewards) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  rewards[i] = bg_norm_reward(bg_norm_reward64(rows + (size_t)i * row_stride), denom[denom_per_step ? i / N : 0], clip);
}
#endif  // BG_NORM_HOST
#endif
