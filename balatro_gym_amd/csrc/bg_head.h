// bg_head.h -- bg_sample_actions / bg_evaluate_actions: the masked categorical policy head over [m, 60] logits.
//
// The last link of the collection loop that was torch glue: logits -> the int32 actions bg_step_rows / bg_step_many_rows take, with the
// log-probability and entropy PPO stores (SB3's CategoricalDistribution.sample / log_prob / entropy / mode), drawn only from the env's
// action_mask (the discipline of the reference's own driver loop; include/balatro_mi355x.h has the citations).  The per-row arithmetic is plain
// C++ behind BG_HEAD_FN, so the text the GPU runs compiles with g++ (define BG_HEAD_HOST before including; the pattern of bg_gae.h / bg_norm.h).
// The library is built with -ffp-contract=off (build.FLAGS): no multiply-add is fused, every operation rounds to float32 on its own.
//
// THE CONTRACT.  A row is 60 logits l[j] (float32, or bfloat16 widened exactly: bits << 16) and 60 mask bytes k[j] (non-zero = valid; no mask =
// every action valid).  V = the valid j.
//   degenerate   V is empty, or a valid logit is NaN or +inf, or every valid logit is -inf:  action = -1, log_prob = entropy = quiet NaN
//                (0x7fc00000), in every mode.  (-1 is an invalid action to the step entry points.)  A valid -inf logit beside finite ones is
//                allowed and has probability 0.
//   common       m = max over V of l[j];  d[j] = l[j] - m;  e[j] = expf(d[j]) for j in V;  P[j] = the running float32 sum of e over the valid
//                j in index order 0..59 (invalid j contribute nothing);  S = P[59];  A = the running sum in the same order of e[j] * d[j] over
//                the valid j with e[j] > 0 (so there is no 0 * -inf).
//   sample       h = bg_head_hash(seed, index0 + i, t)  (bg_policy_hash of bg_device.h: the rollout's counter hash);  u = float(h >> 8) * 2^-24
//                (exact, in [0, 1));  thr = u * S;  action = the smallest valid j with P[j] > thr, else the largest valid j with e[j] > 0.
//                (thr < S for finite inputs -- u <= 1 - 2^-24 and rounding is monotone -- so the fallback is never taken; it is kept.)
//   deterministic  action = the smallest valid j with l[j] == m.
//   log_prob     d[action] - logf(S)
//   entropy      logf(S) - A / S
//   evaluate     the action is given: in range and masked -> log_prob = -inf; outside [0, 60) -> log_prob = NaN; the entropy is unchanged.
// Consequences: a masked action is never returned (only valid j are candidates); an action with e[j] == 0 is never returned (P[j] == P[j-1]
// there, so a smaller j wins, and P[first valid] == 0 is never > thr >= 0); the result is a pure function of (logits row, mask row, seed,
// index0 + i, t), so it does not depend on m, on the launch shape or on sharding.
// expf / logf are the math library's accurate functions (the device library's on the GPU, not the fast intrinsics): the same inputs give the same
// bits on every call, but not promised glibc's or numpy's bits -- tests/head_ref.py bounds them.
#ifndef BG_HEAD_H
#define BG_HEAD_H
#include <stdint.h>

#ifdef BG_HEAD_HOST
#include <math.h>
#define BG_HEAD_FN static inline
#else
#define BG_HEAD_FN __host__ __device__ __forceinline__
#endif

#define BG_HEAD_ACTIONS 60
#define BG_HEAD_SAMPLE 0
#define BG_HEAD_ARGMAX 1   /* BG_HEAD_DETERMINISTIC */
#define BG_HEAD_EVALUATE 2
#define BG_HEAD_QNAN 0x7fc00000u
#define BG_HEAD_NEG_INF 0xff800000u

// bg_policy_hash (bg_device.h), the same text where host code can compile it: the splitmix64 finaliser over (seed, env index, step), high 32 bits
BG_HEAD_FN uint32_t bg_head_hash(uint64_t policy_seed, uint64_t env_index, uint64_t t) {
  uint64_t x = policy_seed + 0x9E3779B97F4A7C15ull * (env_index + 1) + 0xD1B54A32D192ED03ull * (t + 1);
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (uint32_t)(x >> 32);
}
// 24 bits of the hash as a float32 in [0, 1): both the conversion and the product are exact
BG_HEAD_FN float bg_head_u(uint32_t h) { return (float)(h >> 8) * 5.9604644775390625e-08f; }
BG_HEAD_FN float bg_head_from_bits(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
BG_HEAD_FN float bg_head_widen_bf16(uint16_t b) { return bg_head_from_bits((uint32_t)b << 16); }

struct BgHeadOut {
  int32_t action;
  float log_prob, entropy;
};

// byte j of a row's mask: kw is the 60 mask bytes as 15 little-endian words
BG_HEAD_FN bool bg_head_valid(const uint32_t* kw, int32_t j) { return ((kw[j >> 2] >> ((j & 3) * 8)) & 0xffu) != 0u; }

// One row.  l: the 60 logits; kw: the 60 mask bytes as 15 words (read only when MASKED); P: 60 floats of scratch (LDS on the GPU) that take the prefix
// sums; u: bg_head_u of the row's hash (BG_HEAD_SAMPLE); given: the action to evaluate (BG_HEAD_EVALUATE).
// Written without branches on the mask: an invalid j adds e = +0.0 to S (S >= +0, so S + 0 is S to the bit) and leaves m, A and `last` alone, so the
// loops unroll into straight-line code whose LDS reads are all in flight at once.
template <int MODE, bool MASKED>
BG_HEAD_FN BgHeadOut bg_head_row(const float* l, const uint32_t* kw, float* P, float u, int32_t given) {
  const float ninf = bg_head_from_bits(BG_HEAD_NEG_INF), qnan = bg_head_from_bits(BG_HEAD_QNAN);
  BgHeadOut o;
  // pass 1: the maximum over V, its first index, and whether a valid logit is NaN
  float m = ninf;
  int32_t arg = -1;
  bool nan = false;
#pragma unroll
  for (int j = 0; j < BG_HEAD_ACTIONS; j++) {
    const bool ok = !MASKED || bg_head_valid(kw, j);
    const float v = l[j];
    nan = nan || (ok && v != v);
    const bool up = ok && v > m;
    m = up ? v : m;
    arg = up ? j : arg;
  }
  if (nan || m == ninf || m == -ninf) {   // (m == -inf: V is empty or holds only -inf)
    o.action = -1; o.log_prob = qnan; o.entropy = qnan;
    return o;
  }
  // pass 2: e, the prefix sums, A; an invalid j stores -1, which no threshold (>= 0) is below
  float S = 0.0f, A = 0.0f;
  int32_t last = -1;
#pragma unroll
  for (int j = 0; j < BG_HEAD_ACTIONS; j++) {
    const bool ok = !MASKED || bg_head_valid(kw, j);
    const float d = l[j] - m;
    const float e = ok ? expf(d) : 0.0f;
    S = S + e;
    const bool pos = e > 0.0f;
    A = pos ? A + e * d : A;
    last = pos ? j : last;
    if (MODE == BG_HEAD_SAMPLE) P[j] = ok ? S : -1.0f;
  }
  int32_t a = MODE == BG_HEAD_EVALUATE ? given : arg;
  if (MODE == BG_HEAD_SAMPLE) {
    const float thr = u * S;
    a = last;
#pragma unroll
    for (int j = BG_HEAD_ACTIONS - 1; j >= 0; j--) a = P[j] > thr ? j : a;   // ends on the smallest such j
  }
  const float logS = logf(S);
  o.action = a;
  o.entropy = logS - A / S;
  if (MODE == BG_HEAD_EVALUATE && (a < 0 || a >= BG_HEAD_ACTIONS)) o.log_prob = qnan;
  else if (MODE == BG_HEAD_EVALUATE && MASKED && !bg_head_valid(kw, a)) o.log_prob = ninf;
  else o.log_prob = (l[a] - m) - logS;
  return o;
}

#ifdef BG_HEAD_HOST
// The serial twins' row: the run-time choice among the six instantiations, with the draw of row `row` = index0 + i in BG_HEAD_SAMPLE
static inline BgHeadOut bg_head_row_host(int mode, bool masked, const float* l, const uint32_t* kw, float* P, uint64_t seed, uint64_t row, uint64_t t, int32_t given) {
  const float u = mode == BG_HEAD_SAMPLE ? bg_head_u(bg_head_hash(seed, row, t)) : 0.0f;
  if (mode == BG_HEAD_SAMPLE) return masked ? bg_head_row<BG_HEAD_SAMPLE, true>(l, kw, P, u, given) : bg_head_row<BG_HEAD_SAMPLE, false>(l, kw, P, u, given);
  if (mode == BG_HEAD_ARGMAX) return masked ? bg_head_row<BG_HEAD_ARGMAX, true>(l, kw, P, u, given) : bg_head_row<BG_HEAD_ARGMAX, false>(l, kw, P, u, given);
  return masked ? bg_head_row<BG_HEAD_EVALUATE, true>(l, kw, P, u, given) : bg_head_row<BG_HEAD_EVALUATE, false>(l, kw, P, u, given);
}
#else
// ---- the kernel ----
// The contract fixes the order of the additions inside a row, so the parallelism is across rows: lane = row.  Read that way from HBM, consecutive
// lanes would sit 240 (120) bytes apart, so a workgroup -- ONE wave, BG_HEAD_ROWS = 64 consecutive rows; 4 096 rows are 64 workgroups on 64 CUs, as the
// GAE kernel's -- stages first, as bg_encode_kernel does:
//   1  the rows' logits come from HBM with consecutive lanes on consecutive pieces and go, widened to float32, into LDS at a pitch of 61 words; the
//      mask bytes into LDS at a pitch of 15 words (both odd: phase 2's lanes, one row each, read without bank conflicts).  Piece size by alignment:
//        BG_HEAD_LD_ROWS16  pointer and row pitch 16-byte aligned: 16-byte pieces of one row (the 12 / 8-byte tail of a mask / bf16 row by word)
//        BG_HEAD_LD_FLAT16  rows are not 16-byte aligned but dense (pitch == 60) and the pointer is aligned: a workgroup's rows are ONE aligned run
//                           (64 * 120 and 64 * 60 bytes are multiples of 16), so pieces run across row ends         [bf16 logits, int8 masks]
//        BG_HEAD_LD_WORD    4 bytes per lane: a float32 logit, two bf16 logits, four mask bytes
//        BG_HEAD_LD_HALF    2 bytes per lane                                                                       [bf16 logits at odd offsets]
//   2  lane = row runs bg_head_row over its LDS row: the max, then exp / prefix / A with the 60 prefix sums stored to a second LDS tile (pitch 61
//      again), then the selection walks that tile.  The loops carry no branch on the mask and unroll into straight-line code, so a pass's LDS reads
//      are all in flight at once (a form that branches per element waits per element; DESIGN.md section 4 has both, measured).
//   3  a lane's outputs are consecutive elements: 64 x 4 bytes per store instruction.
// LDS: 15 616 bytes of logits + 15 616 of prefix sums (BG_HEAD_SAMPLE only) + 3 840 of masks: four one-wave workgroups per CU in sample mode, so the
// registers the unrolled code takes (DESIGN.md has every instantiation's) cost no occupancy that LDS had not taken.
// Development builds: -DBG_HEAD_ROWS=r -DBG_HEAD_BLOCK=b give r rows and b lanes per workgroup (lanes beyond r only stage); DESIGN.md has the A/B.
#ifndef BG_HEAD_ROWS
#define BG_HEAD_BLOCK 64
#define BG_HEAD_ROWS 64
#endif
#define BG_HEAD_LPITCH (BG_HEAD_ACTIONS + 1)
#define BG_HEAD_MWORDS (BG_HEAD_ACTIONS / 4)
#define BG_HEAD_LD_NONE 0 /* masks only: mask_dev == NULL */
#define BG_HEAD_LD_ROWS16 1
#define BG_HEAD_LD_FLAT16 2
#define BG_HEAD_LD_WORD 3
#define BG_HEAD_LD_HALF 4
static_assert(BG_HEAD_LPITCH % 2 == 1 && BG_HEAD_MWORDS % 2 == 1, "odd word pitches: lane = row reads are conflict-free");
static_assert(BG_HEAD_ACTIONS % 4 == 0 && (BG_HEAD_ROWS * BG_HEAD_ACTIONS) % 16 == 0, "a workgroup's dense rows start on a 16-byte boundary");
static_assert(BG_ROW_ACTION_MASK % 16 == 0, "a record's mask takes the 16-byte path");

__device__ __forceinline__ void bg_head_put_bf16x2(float* dst, uint32_t w) {
  dst[0] = bg_head_from_bits(w << 16);
  dst[1] = bg_head_from_bits(w & 0xffff0000u);
}

// phase 1 for the logits: `nrow` rows from row `rec0` on -> lg[r * BG_HEAD_LPITCH + c] as float32
template <bool BF16>
__device__ __forceinline__ void bg_head_stage_logits(const void* __restrict__ logits, int ld, uint64_t stride, long long rec0, int nrow, float* lg) {
  constexpr int W = BG_HEAD_ACTIONS, ES = BF16 ? 2 : 4, E = 16 / ES;
  const uint8_t* const base = reinterpret_cast<const uint8_t*>(logits);
  if (ld == BG_HEAD_LD_ROWS16) {
    constexpr int U = (W + E - 1) / E;   // 15 pieces of 4 floats; 7 pieces of 8 bf16 and one of 4
    for (int u = threadIdx.x; u < nrow * U; u += BG_HEAD_BLOCK) {
      const int r = u / U, c = (u - r * U) * E;
      const uint8_t* const src = base + ((size_t)(rec0 + r) * stride + c) * ES;
      float* const dst = lg + r * BG_HEAD_LPITCH + c;
      if (BF16 && c + E > W) {   // the 8-byte tail of a bf16 row
        const uint2 v = *reinterpret_cast<const uint2*>(src);
        bg_head_put_bf16x2(dst, v.x); bg_head_put_bf16x2(dst + 2, v.y);
      } else {
        const uint4 v = *reinterpret_cast<const uint4*>(src);
        if (BF16) { bg_head_put_bf16x2(dst, v.x); bg_head_put_bf16x2(dst + 2, v.y); bg_head_put_bf16x2(dst + 4, v.z); bg_head_put_bf16x2(dst + 6, v.w); }
        else { dst[0] = bg_head_from_bits(v.x); dst[1] = bg_head_from_bits(v.y); dst[2] = bg_head_from_bits(v.z); dst[3] = bg_head_from_bits(v.w); }
      }
    }
  } else if (BF16 && ld == BG_HEAD_LD_FLAT16) {
    const uint16_t* const run = reinterpret_cast<const uint16_t*>(base) + (size_t)rec0 * W;   // 16-byte aligned: rec0 is a multiple of BG_HEAD_ROWS
    const int n = nrow * W, full = n / E;
    for (int u = threadIdx.x; u < full; u += BG_HEAD_BLOCK) {
      const uint4 v = *reinterpret_cast<const uint4*>(run + u * E);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int q = 0; q < 4; q++) {   // a pair never straddles a row: W is even
        const int e0 = u * E + 2 * q, r = e0 / W, c = e0 - r * W;
        bg_head_put_bf16x2(lg + r * BG_HEAD_LPITCH + c, w[q]);
      }
    }
    for (int e0 = full * E + threadIdx.x; e0 < n; e0 += BG_HEAD_BLOCK) {   // an odd row count leaves 8 bytes
      const int r = e0 / W, c = e0 - r * W;
      lg[r * BG_HEAD_LPITCH + c] = bg_head_widen_bf16(run[e0]);
    }
  } else if (BF16 && ld == BG_HEAD_LD_WORD) {
    for (int u = threadIdx.x; u < nrow * (W / 2); u += BG_HEAD_BLOCK) {
      const int r = u / (W / 2), c = (u - r * (W / 2)) * 2;
      bg_head_put_bf16x2(lg + r * BG_HEAD_LPITCH + c, *reinterpret_cast<const uint32_t*>(base + ((size_t)(rec0 + r) * stride + c) * ES));
    }
  } else {   // one element per lane
    for (int u = threadIdx.x; u < nrow * W; u += BG_HEAD_BLOCK) {
      const int r = u / W, c = u - r * W;
      const uint8_t* const src = base + ((size_t)(rec0 + r) * stride + c) * ES;
      lg[r * BG_HEAD_LPITCH + c] = BF16 ? bg_head_widen_bf16(*reinterpret_cast<const uint16_t*>(src)) : *reinterpret_cast<const float*>(src);
    }
  }
}

// phase 1 for the masks: mk[r * BG_HEAD_MWORDS + w] = bytes 4w .. 4w+3 of row r's mask (the LDS image is the dense [rows, 60] byte matrix)
__device__ __forceinline__ void bg_head_stage_mask(const int8_t* __restrict__ mask, int ld, uint64_t stride, long long rec0, int nrow, uint32_t* mk) {
  const uint8_t* const base = reinterpret_cast<const uint8_t*>(mask);
  if (ld == BG_HEAD_LD_ROWS16) {
    for (int u = threadIdx.x; u < nrow * 4; u += BG_HEAD_BLOCK) {
      const int r = u >> 2, p = u & 3;
      const uint8_t* const src = base + (size_t)(rec0 + r) * stride + p * 16;
      uint32_t* const dst = mk + r * BG_HEAD_MWORDS + p * 4;
      if (p < 3) {
        const uint4 v = *reinterpret_cast<const uint4*>(src);
        dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
      } else {   // bytes 48..59
        const uint2 v = *reinterpret_cast<const uint2*>(src);
        dst[0] = v.x; dst[1] = v.y; dst[2] = *reinterpret_cast<const uint32_t*>(src + 8);
      }
    }
  } else if (ld == BG_HEAD_LD_FLAT16) {
    const uint32_t* const run = reinterpret_cast<const uint32_t*>(base + (size_t)rec0 * BG_HEAD_ACTIONS);
    const int n = nrow * BG_HEAD_MWORDS, full = n / 4;
    for (int u = threadIdx.x; u < full; u += BG_HEAD_BLOCK) {
      const uint4 v = *reinterpret_cast<const uint4*>(run + u * 4);
      mk[u * 4] = v.x; mk[u * 4 + 1] = v.y; mk[u * 4 + 2] = v.z; mk[u * 4 + 3] = v.w;
    }
    for (int w = full * 4 + threadIdx.x; w < n; w += BG_HEAD_BLOCK) mk[w] = run[w];
  } else {
    for (int u = threadIdx.x; u < nrow * BG_HEAD_MWORDS; u += BG_HEAD_BLOCK) {
      const int r = u / BG_HEAD_MWORDS, w = u - r * BG_HEAD_MWORDS;
      mk[u] = *reinterpret_cast<const uint32_t*>(base + (size_t)(rec0 + r) * stride + w * 4);
    }
  }
}

// The LDS of a head-ended kernel (this one, bg_actor_head_kernel, bg_policy_kernel) in mode MODE for ROWS rows: it DECLARES lg, the float32 logits tile;
// pf, the prefix sums of BG_HEAD_SAMPLE; mk, the mask words.  A macro because three arrays compile to another text than one object that holds them.
#define BG_HEAD_LDS(MODE, ROWS)                                               \
  __shared__ float lg[(ROWS) * BG_HEAD_LPITCH];                               \
  __shared__ float pf[(MODE) == BG_HEAD_SAMPLE ? (ROWS) * BG_HEAD_LPITCH : 1];  \
  __shared__ uint32_t mk[(ROWS) * BG_HEAD_MWORDS]

// MODE: BG_HEAD_SAMPLE / BG_HEAD_ARGMAX write actions_out; BG_HEAD_EVALUATE reads actions_in.  log_prob / entropy may be NULL.  m >= 1.
template <int MODE>
__global__ __launch_bounds__(BG_HEAD_BLOCK) void bg_head_kernel(const void* __restrict__ logits, int bf16, int lld, uint64_t lstride,
                                                                const int8_t* __restrict__ mask, int mld, uint64_t mstride, long long m, uint64_t seed,
                                                                uint64_t index0, uint64_t t, const int32_t* __restrict__ actions_in,
                                                                int32_t* __restrict__ actions_out, float* __restrict__ log_prob, float* __restrict__ entropy) {
  BG_HEAD_LDS(MODE, BG_HEAD_ROWS);   // lg, pf, mk
  const long long rec0 = (long long)blockIdx.x * BG_HEAD_ROWS;
  const int nrow = (int)(m - rec0 < BG_HEAD_ROWS ? m - rec0 : BG_HEAD_ROWS);
  if (bf16) bg_head_stage_logits<true>(logits, lld, lstride, rec0, nrow, lg);
  else bg_head_stage_logits<false>(logits, lld, lstride, rec0, nrow, lg);
  if (mld != BG_HEAD_LD_NONE) bg_head_stage_mask(mask, mld, mstride, rec0, nrow, mk);
  __syncthreads();
  const int r = threadIdx.x;
  if (r >= nrow) return;
  const long long i = rec0 + r;
  const float* const l = lg + r * BG_HEAD_LPITCH;
  float* const P = pf + (MODE == BG_HEAD_SAMPLE ? r * BG_HEAD_LPITCH : 0);
  const uint32_t* const k = mk + r * BG_HEAD_MWORDS;
  const float u = MODE == BG_HEAD_SAMPLE ? bg_head_u(bg_head_hash(seed, index0 + (uint64_t)i, t)) : 0.0f;
  const int32_t given = MODE == BG_HEAD_EVALUATE ? actions_in[i] : 0;
  const BgHeadOut o = mld != BG_HEAD_LD_NONE ? bg_head_row<MODE, true>(l, k, P, u, given) : bg_head_row<MODE, false>(l, k, P, u, given);
  if (MODE != BG_HEAD_EVALUATE) actions_out[i] = o.action;
  if (log_prob) log_prob[i] = o.log_prob;
  if (entropy) entropy[i] = o.entropy;
}
#endif  // BG_HEAD_HOST
#endif
