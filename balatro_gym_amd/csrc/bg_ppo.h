// bg_ppo.h -- bg_ppo_loss: PPO's clipped loss over the masked categorical head of bg_head.h, with its gradient, in one pass over the logits.
//
// The link between bg_evaluate_actions (forward only) and a learner: SB3's `PPO.train` loss for a minibatch of m rows, its diagnostics, and the gradient
// of the loss with respect to the logits and the values, produced in the forward pass (as fused cross-entropy operators do), so that the backward of the
// autograd node on top is one multiplication by the incoming scalar.  It replaces the torch composite masked_fill -> log_softmax -> gather -> exp ->
// clamp -> min -> mean plus the entropy and value terms, and their backward (hpc_train.py:77-88, train_balatro_fixed.py:346-357,
// train_balatro_agent.py:326-337, robust_training.py:140-151: clip_range 0.2, ent_coef 0.01, vf_coef 0.5; train_progressive.py:161-176: 0.3 / 0.02).
// The per-row arithmetic is plain C++ behind BG_HEAD_FN: define BG_PPO_HOST before including and the text the GPU runs compiles with g++, with a serial
// twin of the launch sequence (bg_ppo_host) that follows the orders fixed below.  The library is built with -ffp-contract=off: nothing is fused.
//
// THE CONTRACT.  Everything is float32 and every operation rounds on its own, except the sums across rows, which are float64.
//   row i        reads its logits and values at minibatch row i.  With index (SB3's RolloutBuffer.get permutation) the STORED arrays -- mask, actions,
//                old_log_prob, advantages, returns -- are read at row src = index[i] of store_rows rows, else at src = i.
//   head         m_, d[j], e[j], S, A, logS = logf(S) exactly as bg_head_row computes them (same expressions, same order); log_prob = d[a] - logS and
//                entropy H = logS - A / S are BIT FOR BIT what bg_evaluate_actions returns for the row (quiet NaN / -inf cases included).
//   adv'         = adv, or with BG_PPO_NORMALIZE_ADV and n > 1:  (adv - mean) / (std + 1e-8f), mean / std the float32 roundings of the float64 mean and
//                unbiased standard deviation sqrt(M2 / (n - 1)) of the n advantages of this call (n = m; rows whose index is out of range have no
//                advantage and are left out, n counts the others).  This is SB3's rule, its `len(advantages) > 1` included.  Accumulated as (n, mean, M2)
//                triples merged pairwise (bg_ppo_merge: delta = mean_b - mean_a; mean = mean_a + delta * (n_b / n); M2 = (M2_a + M2_b) + (delta * delta) *
//                (n_a * n_b / n); an empty side returns the other unchanged): 256 consecutive rows per workgroup by the TREE below, the workgroups' triples
//                by SLICES-THEN-TREE below.
//   policy       lr = log_prob - old_log_prob;  ratio = expf(lr);  lo = 1 - clip;  hi = 1 + clip;  rc = min(max(ratio, lo), hi);  s1 = adv' * ratio;
//                s2 = adv' * rc;  policy term = -min(s1, s2);  g = adv' * ratio if (lo <= ratio <= hi) or s1 < s2, else 0  (what torch's min / clamp
//                backward give, ties included);  kl term = (ratio - 1) - lr;  clipped = |ratio - 1| > clip.
//   value        with values / returns:  dv = v - ret;  value term = dv * dv;  dvalues[i] = ((vf_coef * 2) * dv) / float(m).
//   gradient     p = e[j] / S.  valid j with e[j] > 0:  dlogits[i, j] = ((ent_coef * p) * ((d[j] - logS) + H) - g * (1[j == a] - p)) / float(m);
//                valid j with e[j] == 0:  (0 - g) / float(m) if j == a, else +0.0;  invalid j: +0.0.  bfloat16 output is this float32 value rounded to
//                nearest even (NaN -> 0x7fc0).  Padding columns of a strided output are not written.
//   EXCLUDED     a row the head calls degenerate, whose action is outside [0, 60) or masked, whose old_log_prob, adv, adv', value or return is not
//                finite, or whose index is outside [0, store_rows) (nothing is read for it; its log_prob and entropy are quiet NaN): it adds nothing to
//                any sum, its dlogits row and dvalue are +0.0, it is counted in `excluded`, and the divisor stays m.
//   sums         per row, as float64: policy term, value term, H, kl term, clipped (0 / 1), excluded (0 / 1).  A workgroup is 64 consecutive rows and sums
//                them by the TREE; the workgroups' partials (caller's workspace) are summed by SLICES-THEN-TREE in a one-workgroup kernel.  Then, in
//                float64, policy_loss = sum / m, value_loss = sum / m, entropy_loss = -(sum H) / m, approx_kl = sum / m, clip_fraction = sum / m,
//                loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss, each rounded to float32 once.
//   TREE, SLICES-THEN-TREE  the two orders every sum across rows of this header, bg_bc.h, bg_dqn.h and bg_actor.h takes: stated once, at THE REDUCTION ORDER below.
// No floating-point atomics, and the launch sequence is fixed (statistics partials, statistics, rows, finish), so the result is a function of the
// arguments alone: two calls give the same bits.  expf / logf as in bg_head.h: bounded by tests/ppo_ref.py, not promised another library's bits.
// Out of scope: clip_range_vf, temperature, target_kl (the caller reads approx_kl), gradient clipping, the optimiser.
#ifndef BG_PPO_H
#define BG_PPO_H
#if defined(BG_PPO_HOST) && !defined(BG_HEAD_HOST)
#define BG_HEAD_HOST
#endif
#include "bg_head.h"
#ifdef BG_PPO_HOST
#include <string.h>
#endif

#define BG_PPO_SUMS 6      /* policy, value, entropy, kl, clipped, excluded */
#ifdef BG_HEAD_ROWS
#define BG_PPO_ROWS BG_HEAD_ROWS   /* rows per workgroup partial */
#else
#define BG_PPO_ROWS 64
#endif
#define BG_PPO_LANES 256   /* rows per statistics partial; lanes of the statistics and the finishing workgroup */
#define BG_PPO_WS_HEAD 16  /* workspace: float mean, float std, uint32 apply, pad; then the statistics partials; then the row partials */

struct BgPpoMoments { double n, mean, m2; };
BG_HEAD_FN BgPpoMoments bg_ppo_merge(BgPpoMoments a, BgPpoMoments b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  BgPpoMoments o;
  o.n = a.n + b.n;
  const double delta = b.mean - a.mean;
  o.mean = a.mean + delta * (b.n / o.n);
  o.m2 = (a.m2 + b.m2) + (delta * delta) * (a.n * b.n / o.n);
  return o;
}
BG_HEAD_FN uint32_t bg_ppo_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
BG_HEAD_FN bool bg_ppo_finite(float f) { return (bg_ppo_bits(f) & 0x7f800000u) != 0x7f800000u; }
BG_HEAD_FN uint16_t bg_ppo_bf16(float f) {   // round to nearest even
  const uint32_t u = bg_ppo_bits(f);
  if (f != f) return 0x7fc0u;
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
BG_HEAD_FN uint64_t bg_ppo_stat_parts(long long m) { return ((uint64_t)m + BG_PPO_LANES - 1) / BG_PPO_LANES; }
BG_HEAD_FN uint64_t bg_ppo_row_parts(long long m) { return ((uint64_t)m + BG_PPO_ROWS - 1) / BG_PPO_ROWS; }
// bg_ppo_loss_workspace_bytes(m) for m > 0: the head, one triple per statistics partial, BG_PPO_SUMS float64 per row partial
BG_HEAD_FN uint64_t bg_ppo_ws_bytes(long long m) {
  return BG_PPO_WS_HEAD + bg_ppo_stat_parts(m) * sizeof(BgPpoMoments) + bg_ppo_row_parts(m) * (BG_PPO_SUMS * sizeof(double));
}

struct BgPpoTerms {
  float log_prob, entropy, policy, value, kl, dvalue;
  int32_t clipped, excluded;
};
struct BgPpoCoef {
  float clip, lo, hi, ent_coef, vf_coef, fm;
};

// One row.  l: the 60 logits on entry, the 60 gradient values on return (LDS on the GPU: a lane overwrites its own row); kw: the mask words (MASKED);
// E: 60 floats of scratch that keep e[j] for the gradient pass (KEEP), else unused and expf runs again on the same argument (the same bits either way).
// src_ok: the row's index is in range; a, old_lp, adv (as stored), advn (adv'), v, ret: the row's inputs (v / ret read only with has_v).
template <bool MASKED, bool KEEP>
BG_HEAD_FN BgPpoTerms bg_ppo_row(float* l, const uint32_t* kw, float* E, bool src_ok, int32_t a, float old_lp, float adv, float advn, bool has_v, float v,
                                 float ret, const BgPpoCoef c) {
  const float ninf = bg_head_from_bits(BG_HEAD_NEG_INF), qnan = bg_head_from_bits(BG_HEAD_QNAN);
  BgPpoTerms o;
  o.policy = 0.0f; o.value = 0.0f; o.kl = 0.0f; o.dvalue = 0.0f; o.clipped = 0; o.excluded = 1;
  // pass 1 of bg_head_row: the maximum over V and whether a valid logit is NaN
  float m = ninf;
  bool nan = false;
#pragma unroll
  for (int j = 0; j < BG_HEAD_ACTIONS; j++) {
    const bool ok = !MASKED || bg_head_valid(kw, j);
    const float x = l[j];
    nan = nan || (ok && x != x);
    m = (ok && x > m) ? x : m;
  }
  if (!src_ok || nan || m == ninf || m == -ninf) {
    o.log_prob = qnan; o.entropy = qnan;
#pragma unroll
    for (int j = 0; j < BG_HEAD_ACTIONS; j++) l[j] = 0.0f;
    return o;
  }
  // pass 2 of bg_head_row: S and A
  float S = 0.0f, A = 0.0f;
#pragma unroll
  for (int j = 0; j < BG_HEAD_ACTIONS; j++) {
    const bool ok = !MASKED || bg_head_valid(kw, j);
    const float d = l[j] - m;
    const float e = ok ? expf(d) : 0.0f;
    S = S + e;
    A = e > 0.0f ? A + e * d : A;
    if (KEEP) E[j] = e;
  }
  const float logS = logf(S);
  const float H = logS - A / S;
  const bool in_range = a >= 0 && a < BG_HEAD_ACTIONS;
  const bool hidden = in_range && MASKED && !bg_head_valid(kw, a);
  o.entropy = H;
  if (!in_range) o.log_prob = qnan;
  else if (hidden) o.log_prob = ninf;
  else o.log_prob = (l[a] - m) - logS;
  const bool bad_v = has_v && (!bg_ppo_finite(v) || !bg_ppo_finite(ret));
  if (!in_range || hidden || !bg_ppo_finite(old_lp) || !bg_ppo_finite(adv) || !bg_ppo_finite(advn) || bad_v) {
#pragma unroll
    for (int j = 0; j < BG_HEAD_ACTIONS; j++) l[j] = 0.0f;
    return o;
  }
  o.excluded = 0;
  const float lr = o.log_prob - old_lp;
  const float ratio = expf(lr);
  const float rc = fminf(fmaxf(ratio, c.lo), c.hi);
  const float s1 = advn * ratio, s2 = advn * rc;
  o.policy = 0.0f - fminf(s1, s2);
  const float g = ((c.lo <= ratio && ratio <= c.hi) || s1 < s2) ? s1 : 0.0f;
  o.kl = (ratio - 1.0f) - lr;
  o.clipped = fabsf(ratio - 1.0f) > c.clip ? 1 : 0;
  if (has_v) {
    const float dv = v - ret;
    o.value = dv * dv;
    o.dvalue = ((c.vf_coef * 2.0f) * dv) / c.fm;
  }
  // pass 3: the gradient row over the logits row
#pragma unroll
  for (int j = 0; j < BG_HEAD_ACTIONS; j++) {
    const bool ok = !MASKED || bg_head_valid(kw, j);
    const float d = l[j] - m;
    const float e = KEEP ? E[j] : (ok ? expf(d) : 0.0f);
    const float hit = j == a ? 1.0f : 0.0f;
    const float p = e / S;
    const float t1 = g * (hit - p);
    const float t2 = (c.ent_coef * p) * ((d - logS) + H);
    const float live = (t2 - t1) / c.fm;
    const float dead = j == a ? (0.0f - g) / c.fm : 0.0f;
    l[j] = ok ? (e > 0.0f ? live : dead) : 0.0f;
  }
  return o;
}

// what the finishing step writes: stats[BG_PPO_STATS] from the six float64 sums
BG_HEAD_FN void bg_ppo_finish_stats(const double* sum, long long m, float ent_coef, float vf_coef, float adv_mean, float adv_std, float* stats) {
  const double dm = (double)m;
  const double pl = sum[0] / dm, vl = sum[1] / dm, el = (0.0 - sum[2]) / dm;
  stats[0] = (float)(pl + (double)ent_coef * el + (double)vf_coef * vl);
  stats[1] = (float)pl;
  stats[2] = (float)vl;
  stats[3] = (float)el;
  stats[4] = (float)(sum[3] / dm);
  stats[5] = (float)(sum[4] / dm);
  stats[6] = adv_mean;
  stats[7] = adv_std;
  stats[8] = (float)sum[5];
  stats[9] = (float)dm;
}

struct BgPpoArgs {
  const void* logits; uint64_t lstride; int lld;
  const int8_t* mask; uint64_t mstride; int mld;
  const int32_t* actions; const float* old_lp; const float* adv; const float* values; const float* returns;
  const int32_t* index; long long store_rows, m;
  BgPpoCoef c; int normalize;
  void* dlogits; uint64_t dstride; int dst;
  float* dvalues; float* log_prob; float* entropy;
  const float* head;   // workspace: mean, std, apply
  double* partials;    // workspace: [row partials][BG_PPO_SUMS]
};

// ---- THE REDUCTION ORDER of the loss calls (bg_ppo_loss, bg_bc_loss, bg_dqn_loss, bg_actor_ppo_loss), stated once: the device helpers and the host
// template below are the two spellings of it, and the g++ tests hold them to each other bit for bit. ----
//   TREE         over t[0 .. n), n a power of two (rows beyond m hold zero): for s = n / 2, n / 4, .. 1:  t[r] = t[r] (+) t[r + s] for r < s; the result is t[0].
//   SLICES-THEN-TREE  over P partials with L = 256 lanes: per = ceil(P / L); lane q folds partials [q * per, min(P, (q + 1) * per)) in ascending order from
//                zero; the L lane values go through the TREE.
// A row pass: a workgroup is 64 consecutive rows, every term of a row is one float64, term k of the 64 rows goes through the TREE and the workgroup's
// partial is [SUMS] values at partials[workgroup * SUMS]; one workgroup of 256 lanes then takes the partials of every term through SLICES-THEN-TREE
// (the finish).  A pre-pass (PPO's advantage moments, BC's weight sum): 256 consecutive rows per workgroup by the TREE, the workgroups' values by
// SLICES-THEN-TREE (the combine).  (+) is a fold functor called as fold(k, a, b), k the term: BgLossSum, BgPpoMerge, bg_dqn.h's BgDqnFold.
// Spelled out where sharing moved the compiled kernel ("Source-only changes"): the three finish kernels (bg_ppo_finish, bg_bc_finish,
// bg_dqn_finish: SLICES-THEN-TREE per term, then their *_finish_stats) and the tail of bg_actor_ppo_kernel (bg_loss_tile_reduce's text).
#ifdef BG_PPO_HOST
#define BG_LOSS_FOLD inline   /* a member: BG_HEAD_FN is `static inline` under g++ */
#else
#define BG_LOSS_FOLD BG_HEAD_FN
#endif
struct BgLossSum { BG_LOSS_FOLD double operator()(int, double a, double b) const { return a + b; } };
struct BgPpoMerge { BG_LOSS_FOLD BgPpoMoments operator()(int, BgPpoMoments a, BgPpoMoments b) const { return bg_ppo_merge(a, b); } };
#ifdef BG_PPO_HOST
// TREE over t[0 .. n) in place -> t[0]
template <class T, class F>
static inline T bg_loss_host_tree(T* t, int n, int k, F fold) {
  for (int s = n / 2; s; s >>= 1) for (int r = 0; r < s; r++) t[r] = fold(k, t[r], t[r + s]);
  return t[0];
}
// SLICES-THEN-TREE over part[p * stride + k], p in [0, P)
template <class T, class F>
static inline T bg_loss_host_slices(const T* part, uint64_t P, int stride, int k, T zero, F fold) {
  T t[BG_PPO_LANES];
  const uint64_t per = (P + BG_PPO_LANES - 1) / BG_PPO_LANES;
  for (uint64_t q = 0; q < BG_PPO_LANES; q++) {
    t[q] = zero;
    for (uint64_t p = q * per; p < P && p < (q + 1) * per; p++) t[q] = fold(k, t[q], part[p * stride + k]);
  }
  return bg_loss_host_tree(t, BG_PPO_LANES, k, fold);
}
// the row pass' two levels: t[k][r] of one workgroup -> its partial; the partials -> sum[SUMS]
template <int SUMS, class F>
static inline void bg_loss_host_tile(double (*t)[BG_PPO_ROWS], double* part, F fold) {
  for (int k = 0; k < SUMS; k++) part[k] = bg_loss_host_tree(t[k], BG_PPO_ROWS, k, fold);
}
template <int SUMS, class F>
static inline void bg_loss_host_finish(const double* part, uint64_t P, double* sum, F fold) {
  for (int k = 0; k < SUMS; k++) sum[k] = bg_loss_host_slices(part, P, SUMS, k, 0.0, fold);
}
#else
static_assert((BG_HEAD_ROWS & (BG_HEAD_ROWS - 1)) == 0 && BG_HEAD_ROWS <= BG_HEAD_BLOCK, "the sums of a workgroup go through a power-of-two tree");
// the tail of a row pass: the lane's terms t[SUMS] (zero beyond the rows) -> red (LDS, [SUMS][BG_HEAD_ROWS]) -> the partial of workgroup `block`
template <int SUMS, class F>
__device__ __forceinline__ void bg_loss_tile_reduce(const double* t, double* red, double* partials, size_t block, F fold) {
  const int r = threadIdx.x;
  if (r < BG_HEAD_ROWS) {
#pragma unroll
    for (int k = 0; k < SUMS; k++) red[k * BG_HEAD_ROWS + r] = t[k];
  }
  __syncthreads();
  for (int s = BG_HEAD_ROWS / 2; s; s >>= 1) {
    if (r < s) {
#pragma unroll
      for (int k = 0; k < SUMS; k++) red[k * BG_HEAD_ROWS + r] = fold(k, red[k * BG_HEAD_ROWS + r], red[k * BG_HEAD_ROWS + r + s]);
    }
    __syncthreads();
  }
  if (r < SUMS) partials[block * SUMS + r] = red[r * BG_HEAD_ROWS];
}
// a pre-pass: the lane's value v of 256 consecutive rows -> part[workgroup]; and one workgroup: the P parts -> t[0] (read it behind the call).  t: LDS, [256]
template <class T, class F>
__device__ __forceinline__ void bg_loss_stat_partials(T v, T* t, T* __restrict__ part, F fold) {
  const int r = threadIdx.x;
  t[r] = v;
  __syncthreads();
  for (int s = BG_PPO_LANES / 2; s; s >>= 1) {
    if (r < s) t[r] = fold(0, t[r], t[r + s]);
    __syncthreads();
  }
  if (r == 0) part[blockIdx.x] = t[0];
}
template <class T, class F>
__device__ __forceinline__ void bg_loss_stat_combine(const T* __restrict__ part, long long P, T v, T* t, F fold) {
  const int r = threadIdx.x;
  const long long per = (P + BG_PPO_LANES - 1) / BG_PPO_LANES;
  for (long long k = r * per; k < P && k < (r + 1) * per; k++) v = fold(0, v, part[k]);
  t[r] = v;
  __syncthreads();
  for (int s = BG_PPO_LANES / 2; s; s >>= 1) {
    if (r < s) t[r] = fold(0, t[r], t[r + s]);
    __syncthreads();
  }
}
#endif

#ifdef BG_PPO_HOST
// ---- the serial twin: the launch sequence below, one "workgroup" after the other, in the orders of the contract ----
static inline BgPpoMoments bg_ppo_host_moments(const BgPpoArgs& A) {
  const uint64_t P = bg_ppo_stat_parts(A.m);
  const BgPpoMoments zero = {0.0, 0.0, 0.0};
  BgPpoMoments* part = new BgPpoMoments[P ? P : 1];
  for (uint64_t b = 0; b < P; b++) {
    BgPpoMoments t[BG_PPO_LANES];
    for (int r = 0; r < BG_PPO_LANES; r++) {
      const long long i = (long long)b * BG_PPO_LANES + r;
      t[r] = zero;
      if (i < A.m) {
        const long long src = A.index ? A.index[i] : i;
        if (!A.index || (src >= 0 && src < A.store_rows)) { t[r].n = 1.0; t[r].mean = (double)A.adv[src]; }
      }
    }
    part[b] = bg_loss_host_tree(t, BG_PPO_LANES, 0, BgPpoMerge{});
  }
  const BgPpoMoments all = bg_loss_host_slices(part, P, 1, 0, zero, BgPpoMerge{});
  delete[] part;
  return all;
}

// logits_bf16: logits and dlogits are bfloat16 bits.  Every pointer is a host pointer; A.head / A.partials are not used.
static inline void bg_ppo_host(const BgPpoArgs& A, bool bf16, bool keep, float* stats) {
  float mean = 0.0f, sd = 0.0f;
  bool apply = false;
  if (A.normalize) {
    const BgPpoMoments mo = bg_ppo_host_moments(A);
    apply = mo.n > 1.0;
    mean = (float)mo.mean;
    sd = apply ? (float)sqrt(mo.m2 / (mo.n - 1.0)) : 0.0f;
  }
  const uint64_t P = bg_ppo_row_parts(A.m);
  double* part = new double[(P ? P : 1) * BG_PPO_SUMS];
  for (uint64_t b = 0; b < P; b++) {
    double t[BG_PPO_SUMS][BG_PPO_ROWS];
    for (int r = 0; r < BG_PPO_ROWS; r++) {
      const long long i = (long long)b * BG_PPO_ROWS + r;
      for (int k = 0; k < BG_PPO_SUMS; k++) t[k][r] = 0.0;
      if (i >= A.m) continue;
      float l[BG_HEAD_ACTIONS], E[BG_HEAD_ACTIONS];
      uint32_t kw[BG_HEAD_ACTIONS / 4] = {};
      for (int j = 0; j < BG_HEAD_ACTIONS; j++) {
        if (bf16) l[j] = bg_head_widen_bf16(((const uint16_t*)A.logits)[(size_t)i * A.lstride + j]);
        else l[j] = ((const float*)A.logits)[(size_t)i * A.lstride + j];
      }
      const long long src = A.index ? A.index[i] : i;
      const bool ok = !A.index || (src >= 0 && src < A.store_rows);
      if (A.mask && ok) memcpy(kw, (const uint8_t*)A.mask + (size_t)src * A.mstride, BG_HEAD_ACTIONS);
      const int32_t a = ok ? A.actions[src] : -1;
      const float olp = ok ? A.old_lp[src] : 0.0f, adv = ok ? A.adv[src] : 0.0f;
      const float advn = apply ? (adv - mean) / (sd + 1e-8f) : adv;
      const bool has_v = A.values != nullptr;
      const float v = has_v ? A.values[i] : 0.0f, ret = has_v && ok ? A.returns[src] : 0.0f;
      BgPpoTerms o;
      if (A.mask) o = keep ? bg_ppo_row<true, true>(l, kw, E, ok, a, olp, adv, advn, has_v, v, ret, A.c) : bg_ppo_row<true, false>(l, kw, E, ok, a, olp, adv, advn, has_v, v, ret, A.c);
      else o = keep ? bg_ppo_row<false, true>(l, kw, E, ok, a, olp, adv, advn, has_v, v, ret, A.c) : bg_ppo_row<false, false>(l, kw, E, ok, a, olp, adv, advn, has_v, v, ret, A.c);
      if (!o.excluded) { t[0][r] = (double)o.policy; t[1][r] = (double)o.value; t[2][r] = (double)o.entropy; t[3][r] = (double)o.kl; t[4][r] = (double)o.clipped; }
      t[5][r] = (double)o.excluded;
      for (int j = 0; j < BG_HEAD_ACTIONS; j++) {
        if (bf16) ((uint16_t*)A.dlogits)[(size_t)i * A.dstride + j] = bg_ppo_bf16(l[j]);
        else ((float*)A.dlogits)[(size_t)i * A.dstride + j] = l[j];
      }
      if (A.dvalues) A.dvalues[i] = o.dvalue;
      if (A.log_prob) A.log_prob[i] = o.log_prob;
      if (A.entropy) A.entropy[i] = o.entropy;
    }
    bg_loss_host_tile<BG_PPO_SUMS>(t, part + b * BG_PPO_SUMS, BgLossSum{});
  }
  double sum[BG_PPO_SUMS];
  bg_loss_host_finish<BG_PPO_SUMS>(part, P, sum, BgLossSum{});
  delete[] part;
  bg_ppo_finish_stats(sum, A.m, A.c.ent_coef, A.c.vf_coef, mean, sd, stats);
}
#else
// ---- the kernels ----
// bg_ppo_kernel has bg_head_kernel's shape: a workgroup is ONE wave and BG_HEAD_ROWS = 64 consecutive minibatch rows.
//   1  the logits come in through bg_head_stage_logits (rows16 / flat16 / word / half by alignment) into LDS at the odd pitch of 61 words.  The masks come
//      through bg_head_stage_mask, or, with an index, row by row from record index[i] (16-byte pieces when pointer and stride allow, words otherwise: the
//      run-across-rows path does not apply to gathered rows); an index out of range stages an all-invalid mask and reads nothing.
//   2  lane = row runs bg_ppo_row over its LDS row and leaves the 60 gradient values IN that row (its quantities are in registers by then); the row's
//      scalar inputs are four 4-byte gathers, its outputs (dvalue, log_prob, entropy) consecutive elements.  The six float64 terms go through a 64-entry
//      LDS tree, and lane 0 writes the workgroup's partial.
//   3  after the barrier the tile leaves for HBM as it came: consecutive lanes on consecutive 16-byte pieces (BG_HEAD_LD_ROWS16 / _FLAT16), words or
//      halves, chosen by the alignment of dlogits -- never as 240-byte-strided scalar stores.
// LDS: 15 616 bytes of logits / gradient + 3 840 of masks + 3 072 of sums (+ 15 616 with -DBG_PPO_KEEP_E, the development build that keeps e[j] in a
// second tile instead of calling expf again; DESIGN.md has both, measured).
#ifdef BG_PPO_KEEP_E
#define BG_PPO_KEEP true
#else
#define BG_PPO_KEEP false
#endif

// phase 1 for gathered masks: row r of the tile is stored row index[rec0 + r]
__device__ __forceinline__ void bg_ppo_stage_mask_gather(const int8_t* __restrict__ mask, int ld, uint64_t stride, const int32_t* __restrict__ index,
                                                         long long store_rows, long long rec0, int nrow, uint32_t* mk) {
  const uint8_t* const base = reinterpret_cast<const uint8_t*>(mask);
  if (ld == BG_HEAD_LD_ROWS16) {
    for (int u = threadIdx.x; u < nrow * 4; u += BG_HEAD_BLOCK) {
      const int r = u >> 2, p = u & 3;
      const long long src = index[rec0 + r];
      uint32_t* const dst = mk + r * BG_HEAD_MWORDS + p * 4;
      if (src < 0 || src >= store_rows) {
        dst[0] = 0u; dst[1] = 0u; dst[2] = 0u;
        if (p < 3) dst[3] = 0u;
      } else if (p < 3) {
        const uint4 v = *reinterpret_cast<const uint4*>(base + (size_t)src * stride + p * 16);
        dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
      } else {   // bytes 48..59
        const uint8_t* const s = base + (size_t)src * stride + 48;
        const uint2 v = *reinterpret_cast<const uint2*>(s);
        dst[0] = v.x; dst[1] = v.y; dst[2] = *reinterpret_cast<const uint32_t*>(s + 8);
      }
    }
  } else {
    for (int u = threadIdx.x; u < nrow * BG_HEAD_MWORDS; u += BG_HEAD_BLOCK) {
      const int r = u / BG_HEAD_MWORDS, w = u - r * BG_HEAD_MWORDS;
      const long long src = index[rec0 + r];
      mk[u] = (src < 0 || src >= store_rows) ? 0u : *reinterpret_cast<const uint32_t*>(base + (size_t)src * stride + w * 4);
    }
  }
}

// phase 1 of bg_ppo_kernel and bg_bc_kernel: the logits, and the masks flat (rows in order) or gathered through the index
template <bool BF16>
__device__ __forceinline__ void bg_loss_stage(const void* __restrict__ logits, int lld, uint64_t lstride, const int8_t* __restrict__ mask, int mld,
                                              uint64_t mstride, const int32_t* __restrict__ index, long long store_rows, long long rec0, int nrow, float* lg,
                                              uint32_t* mk) {
  bg_head_stage_logits<BF16>(logits, lld, lstride, rec0, nrow, lg);
  if (mld != BG_HEAD_LD_NONE) {
    if (index) bg_ppo_stage_mask_gather(mask, mld, mstride, index, store_rows, rec0, nrow, mk);
    else bg_head_stage_mask(mask, mld, mstride, rec0, nrow, mk);
  }
}

__device__ __forceinline__ uint32_t bg_ppo_bf16x2(const float* s) { return (uint32_t)bg_ppo_bf16(s[0]) | ((uint32_t)bg_ppo_bf16(s[1]) << 16); }

// phase 3: lg[r * BG_HEAD_LPITCH + c] -> `nrow` rows of dlogits from row `rec0` on; the mirror of bg_head_stage_logits
template <bool BF16>
__device__ __forceinline__ void bg_ppo_store_rows(void* __restrict__ out, int st, uint64_t stride, long long rec0, int nrow, const float* lg) {
  constexpr int W = BG_HEAD_ACTIONS, ES = BF16 ? 2 : 4, E = 16 / ES;
  uint8_t* const base = reinterpret_cast<uint8_t*>(out);
  if (st == BG_HEAD_LD_ROWS16) {
    constexpr int U = (W + E - 1) / E;
    for (int u = threadIdx.x; u < nrow * U; u += BG_HEAD_BLOCK) {
      const int r = u / U, c = (u - r * U) * E;
      uint8_t* const dst = base + ((size_t)(rec0 + r) * stride + c) * ES;
      const float* const s = lg + r * BG_HEAD_LPITCH + c;
      if (BF16 && c + E > W) {   // the 8-byte tail of a bf16 row
        uint2 v; v.x = bg_ppo_bf16x2(s); v.y = bg_ppo_bf16x2(s + 2);
        *reinterpret_cast<uint2*>(dst) = v;
      } else {
        uint4 v;
        if (BF16) { v.x = bg_ppo_bf16x2(s); v.y = bg_ppo_bf16x2(s + 2); v.z = bg_ppo_bf16x2(s + 4); v.w = bg_ppo_bf16x2(s + 6); }
        else { v.x = bg_ppo_bits(s[0]); v.y = bg_ppo_bits(s[1]); v.z = bg_ppo_bits(s[2]); v.w = bg_ppo_bits(s[3]); }
        *reinterpret_cast<uint4*>(dst) = v;
      }
    }
  } else if (BF16 && st == BG_HEAD_LD_FLAT16) {
    uint16_t* const run = reinterpret_cast<uint16_t*>(base) + (size_t)rec0 * W;   // 16-byte aligned: rec0 is a multiple of BG_HEAD_ROWS
    const int n = nrow * W, full = n / E;
    for (int u = threadIdx.x; u < full; u += BG_HEAD_BLOCK) {
      uint32_t w[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {   // a pair never straddles a row: W is even
        const int e0 = u * E + 2 * q, r = e0 / W, c = e0 - r * W;
        w[q] = bg_ppo_bf16x2(lg + r * BG_HEAD_LPITCH + c);
      }
      uint4 v; v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
      *reinterpret_cast<uint4*>(run + u * E) = v;
    }
    for (int e0 = full * E + threadIdx.x; e0 < n; e0 += BG_HEAD_BLOCK) {   // an odd row count leaves 8 bytes
      const int r = e0 / W, c = e0 - r * W;
      run[e0] = bg_ppo_bf16(lg[r * BG_HEAD_LPITCH + c]);
    }
  } else if (BF16 && st == BG_HEAD_LD_WORD) {
    for (int u = threadIdx.x; u < nrow * (W / 2); u += BG_HEAD_BLOCK) {
      const int r = u / (W / 2), c = (u - r * (W / 2)) * 2;
      *reinterpret_cast<uint32_t*>(base + ((size_t)(rec0 + r) * stride + c) * ES) = bg_ppo_bf16x2(lg + r * BG_HEAD_LPITCH + c);
    }
  } else {   // one element per lane
    for (int u = threadIdx.x; u < nrow * W; u += BG_HEAD_BLOCK) {
      const int r = u / W, c = u - r * W;
      uint8_t* const dst = base + ((size_t)(rec0 + r) * stride + c) * ES;
      const float x = lg[r * BG_HEAD_LPITCH + c];
      if (BF16) *reinterpret_cast<uint16_t*>(dst) = bg_ppo_bf16(x);
      else *reinterpret_cast<float*>(dst) = x;
    }
  }
}

// the n advantages of the call -> one (n, mean, M2) triple per 256 rows
__global__ __launch_bounds__(BG_PPO_LANES) void bg_ppo_adv_partials(const float* __restrict__ adv, const int32_t* __restrict__ index, long long store_rows,
                                                                    long long m, BgPpoMoments* __restrict__ part) {
  __shared__ BgPpoMoments t[BG_PPO_LANES];
  const long long i = (long long)blockIdx.x * BG_PPO_LANES + threadIdx.x;
  BgPpoMoments v;
  v.n = 0.0; v.mean = 0.0; v.m2 = 0.0;
  if (i < m) {
    const long long src = index ? (long long)index[i] : i;
    if (!index || (src >= 0 && src < store_rows)) { v.n = 1.0; v.mean = (double)adv[src]; }
  }
  bg_loss_stat_partials(v, t, part, BgPpoMerge{});
}

// one workgroup: the triples -> head[0] = mean, head[1] = std, head[2] = apply (n > 1)
__global__ __launch_bounds__(BG_PPO_LANES) void bg_ppo_adv_combine(const BgPpoMoments* __restrict__ part, long long P, float* __restrict__ head) {
  __shared__ BgPpoMoments t[BG_PPO_LANES];
  BgPpoMoments v;
  v.n = 0.0; v.mean = 0.0; v.m2 = 0.0;
  bg_loss_stat_combine(part, P, v, t, BgPpoMerge{});
  if (threadIdx.x == 0) {
    const bool apply = t[0].n > 1.0;
    head[0] = (float)t[0].mean;
    head[1] = apply ? (float)sqrt(t[0].m2 / (t[0].n - 1.0)) : 0.0f;
    reinterpret_cast<uint32_t*>(head)[2] = apply ? 1u : 0u;
  }
}

template <bool BF16>
__global__ __launch_bounds__(BG_HEAD_BLOCK) void bg_ppo_kernel(const BgPpoArgs A) {
  __shared__ float lg[BG_HEAD_ROWS * BG_HEAD_LPITCH];
  __shared__ float ek[BG_PPO_KEEP ? BG_HEAD_ROWS * BG_HEAD_LPITCH : 1];
  __shared__ uint32_t mk[BG_HEAD_ROWS * BG_HEAD_MWORDS];
  __shared__ double red[BG_PPO_SUMS * BG_HEAD_ROWS];
  const long long rec0 = (long long)blockIdx.x * BG_HEAD_ROWS;
  const int nrow = (int)(A.m - rec0 < BG_HEAD_ROWS ? A.m - rec0 : BG_HEAD_ROWS);
  bg_loss_stage<BF16>(A.logits, A.lld, A.lstride, A.mask, A.mld, A.mstride, A.index, A.store_rows, rec0, nrow, lg, mk);
  __syncthreads();
  const int r = threadIdx.x;
  double t[BG_PPO_SUMS];
#pragma unroll
  for (int k = 0; k < BG_PPO_SUMS; k++) t[k] = 0.0;
  if (r < nrow) {
    const long long i = rec0 + r;
    const long long src = A.index ? (long long)A.index[i] : i;
    const bool ok = !A.index || (src >= 0 && src < A.store_rows);
    const int32_t a = ok ? A.actions[src] : -1;
    const float old_lp = ok ? A.old_lp[src] : 0.0f, adv = ok ? A.adv[src] : 0.0f;
    const bool has_v = A.values != nullptr;
    const float v = has_v ? A.values[i] : 0.0f, ret = has_v && ok ? A.returns[src] : 0.0f;
    float advn = adv;
    if (A.normalize && reinterpret_cast<const uint32_t*>(A.head)[2] != 0u) advn = (adv - A.head[0]) / (A.head[1] + 1e-8f);
    float* const l = lg + r * BG_HEAD_LPITCH;
    float* const E = ek + (BG_PPO_KEEP ? r * BG_HEAD_LPITCH : 0);
    const uint32_t* const k = mk + r * BG_HEAD_MWORDS;
    const BgPpoTerms o = A.mld != BG_HEAD_LD_NONE ? bg_ppo_row<true, BG_PPO_KEEP>(l, k, E, ok, a, old_lp, adv, advn, has_v, v, ret, A.c)
                                                  : bg_ppo_row<false, BG_PPO_KEEP>(l, k, E, ok, a, old_lp, adv, advn, has_v, v, ret, A.c);
    if (!o.excluded) { t[0] = (double)o.policy; t[1] = (double)o.value; t[2] = (double)o.entropy; t[3] = (double)o.kl; t[4] = (double)o.clipped; }
    t[5] = (double)o.excluded;
    if (A.dvalues) A.dvalues[i] = o.dvalue;
    if (A.log_prob) A.log_prob[i] = o.log_prob;
    if (A.entropy) A.entropy[i] = o.entropy;
  }
  bg_loss_tile_reduce<BG_PPO_SUMS>(t, red, A.partials, blockIdx.x, BgLossSum{});
  bg_ppo_store_rows<BF16>(A.dlogits, A.dst, A.dstride, rec0, nrow, lg);
}

// one workgroup: the row partials -> stats[BG_PPO_STATS]
__global__ __launch_bounds__(BG_PPO_LANES) void bg_ppo_finish(const double* __restrict__ partials, long long P, long long m, float ent_coef, float vf_coef,
                                                              int normalize, const float* __restrict__ head, float* __restrict__ stats) {
  __shared__ double t[BG_PPO_SUMS * BG_PPO_LANES];
  const int r = threadIdx.x;
  const long long per = (P + BG_PPO_LANES - 1) / BG_PPO_LANES;
  double acc[BG_PPO_SUMS];
#pragma unroll
  for (int k = 0; k < BG_PPO_SUMS; k++) acc[k] = 0.0;
  for (long long p = r * per; p < P && p < (r + 1) * per; p++) {
#pragma unroll
    for (int k = 0; k < BG_PPO_SUMS; k++) acc[k] = acc[k] + partials[p * BG_PPO_SUMS + k];
  }
#pragma unroll
  for (int k = 0; k < BG_PPO_SUMS; k++) t[k * BG_PPO_LANES + r] = acc[k];
  __syncthreads();
  for (int s = BG_PPO_LANES / 2; s; s >>= 1) {
    if (r < s) {
#pragma unroll
      for (int k = 0; k < BG_PPO_SUMS; k++) t[k * BG_PPO_LANES + r] = t[k * BG_PPO_LANES + r] + t[k * BG_PPO_LANES + r + s];
    }
    __syncthreads();
  }
  if (r == 0) {
    double sum[BG_PPO_SUMS];
#pragma unroll
    for (int k = 0; k < BG_PPO_SUMS; k++) sum[k] = t[k * BG_PPO_LANES];
    bg_ppo_finish_stats(sum, m, ent_coef, vf_coef, normalize ? head[0] : 0.0f, normalize ? head[1] : 0.0f, stats);
  }
}
#endif  // BG_PPO_HOST
#endif
