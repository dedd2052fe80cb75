// bg_bc.h -- bg_bc_loss: behaviour cloning over the masked categorical head of bg_head.h: the weighted cross-entropy of stored actions, its accuracy
// and its gradient, in one pass over the logits.
//
// The reference's `BehavioralCloning` (train_balatro_agent.py:220-262) keeps the steps of trajectories with final_ante >= 5 and stops at
// `# TODO: Implement actual BC training loop`.  This is that loop's loss: the torch composite masked_fill -> log_softmax -> gather -> weighted mean,
// the entropy term and their backward, with the gradient produced in the forward pass (as bg_ppo_loss does), so that the backward of the autograd node
// on top is one multiplication.  The filter is a weight: weights = (end_ante >= 5) from bg_episode_outcome_rows (bg_outcome.h).
// The per-row arithmetic is plain C++ behind BG_HEAD_FN: define BG_BC_HOST before including and the text the GPU runs compiles with g++, with a serial
// twin of the launch sequence (bg_bc_host) that follows the orders fixed below.  The library is built with -ffp-contract=off: nothing is fused.
// What bg_ppo.h has -- the staging of logits and masks, the gathered masks, the store of the gradient tile, bf16 rounding, the partial counts -- is
// used from there.
//
// THE CONTRACT.  Everything is float32 and every operation rounds on its own, except the sums across rows, which are float64.
//   row i        reads its logits at minibatch row i.  With index the STORED arrays -- mask, actions, weights -- are read at row src = index[i] of
//                store_rows rows, else at src = i.  The action is the int32 at actions + src * actions_stride_bytes (4: a dense array; a record
//                pitch: BG_ROW_ACTION in place), the mask the 60 bytes at mask + src * mask_stride_bytes.
//   head         m_, d[j], e[j], S, A, logS = logf(S) exactly as bg_head_row computes them (same expressions, same order); log_prob = d[a] - logS and
//                entropy H = logS - A / S are BIT FOR BIT what bg_evaluate_actions returns for the row (quiet NaN / -inf cases included).
//   weight       w = 1, or weights[src].
//   EXCLUDED     a row the head calls degenerate, whose action is outside [0, 60) or masked, whose log_prob is not finite (a valid -inf logit at the
//                action), whose weight is not finite or is negative, or whose index is outside [0, store_rows) (nothing is read for it; its log_prob
//                and entropy are quiet NaN): it adds nothing to any sum, its dlogits row is +0.0, and it is counted in `excluded`.
//   divisor      W = the float64 sum of the weights (1 without weights) of all rows whose index is in range and whose weight is finite and >= 0: known
//                from the weights and the index alone, BEFORE the row pass; rows excluded for other reasons stay in it, as m stays in PPO's.  256
//                consecutive rows per workgroup by the TREE, the workgroups' sums by SLICES-THEN-TREE (both of bg_ppo.h).  Without weights and
//                index W = m and that pass is skipped.  Wf = float(W).  W == 0: every scalar but `excluded` and `m` is 0 and every gradient row +0.0.
//   terms        nll = 0 - log_prob;  hit = 1 where the first maximum among the valid logits is the action (bg_sample_actions' deterministic rule: an
//                exact float32 comparison of the inputs, so no row is undecidable), else 0.  Per row, as float64: w * nll, w * H, w * hit (each
//                product of two float32 values, exact in float64), excluded (0 / 1).
//   gradient     p = e[j] / S.  valid j with e[j] > 0:  dlogits[i, j] = (((ent_coef * p) * ((d[j] - logS) + H) - (1[j == a] - p)) * w) / Wf;
//                valid j with e[j] == 0:  ((0 - 1) * w) / Wf if j == a, else +0.0;  invalid j: +0.0.  bfloat16 output is this float32 value rounded to
//                nearest even (NaN -> 0x7fc0).  Padding columns of a strided output are not written.
//   sums         a workgroup is 64 consecutive rows and sums them by the TREE; the workgroups' partials (caller's workspace) are summed by
//                SLICES-THEN-TREE in a one-workgroup kernel.  Then, in float64, nll_loss = (sum w nll) / W, entropy_loss = (0 - sum w H) / W,
//                accuracy = (sum w hit) / W, loss = nll_loss + ent_coef * entropy_loss, each rounded to float32 once.
//   stats        BG_BC_STATS floats: loss, nll_loss, entropy_loss, accuracy, weight_sum (= float(W)), excluded, m.
// TREE and SLICES-THEN-TREE are bg_ppo.h's.  No floating-point atomics, and the launch sequence is fixed (weight partials, combine, rows, finish), so
// the result is a function of the arguments alone: two calls give the same bits.  expf / logf as in bg_head.h.
// Out of scope: label smoothing, an L2 term (the optimiser's weight decay), (the demonstration ring is bg_demo.h; the expert policy is bg_expert_actions, bg_expert.h).
#ifndef BG_BC_H
#define BG_BC_H
#if defined(BG_BC_HOST) && !defined(BG_PPO_HOST)
#define BG_PPO_HOST
#endif
#include "bg_ppo.h"

#define BG_BC_SUMS 4      /* w nll, w H, w hit, excluded */
#define BG_BC_WS_HEAD 16  /* workspace: float Wf, pad, double W; then the weight partials; then the row partials */

struct BgBcTerms {
  float log_prob, entropy, nll, hit;
  int32_t excluded;
};

// the weight of a row as the divisor counts it: 0 for a row whose index is out of range or whose weight is not finite or negative
BG_HEAD_FN bool bg_bc_weight_ok(float w) { return bg_ppo_finite(w) && w >= 0.0f; }

// One row.  l: the 60 logits on entry, the 60 gradient values on return; kw: the mask words (MASKED); E: 60 floats of scratch (KEEP), as bg_ppo_row.
// src_ok: the row's index is in range; a: the stored action; w: the row's weight; Wf: the divisor (0: every gradient row is +0.0).
template <bool MASKED, bool KEEP>
BG_HEAD_FN BgBcTerms bg_bc_row(float* l, const uint32_t* kw, float* E, bool src_ok, int32_t a, float w, float ent_coef, float Wf) {
  const float ninf = bg_head_from_bits(BG_HEAD_NEG_INF), qnan = bg_head_from_bits(BG_HEAD_QNAN);
  BgBcTerms o;
  o.nll = 0.0f; o.hit = 0.0f; o.excluded = 1;
  // pass 1 of bg_head_row: the maximum over V, its first index, and whether a valid logit is NaN
  float m = ninf;
  int32_t arg = -1;
  bool nan = false;
#pragma unroll
  for (int j = 0; j < BG_HEAD_ACTIONS; j++) {
    const bool ok = !MASKED || bg_head_valid(kw, j);
    const float x = l[j];
    nan = nan || (ok && x != x);
    const bool up = ok && x > m;
    m = up ? x : m;
    arg = up ? j : arg;
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
  if (!in_range || hidden || !bg_ppo_finite(o.log_prob) || !bg_bc_weight_ok(w)) {
#pragma unroll
    for (int j = 0; j < BG_HEAD_ACTIONS; j++) l[j] = 0.0f;
    return o;
  }
  o.excluded = 0;
  o.nll = 0.0f - o.log_prob;
  o.hit = arg == a ? 1.0f : 0.0f;
  const bool zero = Wf == 0.0f;
  // pass 3: the gradient row over the logits row
#pragma unroll
  for (int j = 0; j < BG_HEAD_ACTIONS; j++) {
    const bool ok = !MASKED || bg_head_valid(kw, j);
    const float d = l[j] - m;
    const float e = KEEP ? E[j] : (ok ? expf(d) : 0.0f);
    const float one = j == a ? 1.0f : 0.0f;
    const float p = e / S;
    const float t1 = one - p;
    const float t2 = (ent_coef * p) * ((d - logS) + H);
    const float live = ((t2 - t1) * w) / Wf;
    const float dead = j == a ? ((0.0f - 1.0f) * w) / Wf : 0.0f;
    l[j] = (ok && !zero) ? (e > 0.0f ? live : dead) : 0.0f;
  }
  return o;
}

// what the finishing step writes: stats[BG_BC_STATS] from the four float64 sums and W
BG_HEAD_FN void bg_bc_finish_stats(const double* sum, double W, long long m, float ent_coef, float* stats) {
  const bool zero = W == 0.0;
  const double nl = zero ? 0.0 : sum[0] / W, el = zero ? 0.0 : (0.0 - sum[1]) / W, ac = zero ? 0.0 : sum[2] / W;
  stats[0] = (float)(nl + (double)ent_coef * el);
  stats[1] = (float)nl;
  stats[2] = (float)el;
  stats[3] = (float)ac;
  stats[4] = (float)W;
  stats[5] = (float)sum[3];
  stats[6] = (float)(double)m;
}

struct BgBcArgs {
  const void* logits; uint64_t lstride; int lld;
  const int8_t* mask; uint64_t mstride; int mld;
  const int32_t* actions; uint64_t astride;   // bytes
  const float* weights;
  const int32_t* index; long long store_rows, m;
  float ent_coef, fm;
  void* dlogits; uint64_t dstride; int dst;
  float* log_prob; float* entropy;
  const float* head;   // workspace: Wf, pad, double W -- NULL when W = m (no weights, no index)
  double* partials;    // workspace: [row partials][BG_BC_SUMS]
};

BG_HEAD_FN int32_t bg_bc_action(const int32_t* actions, uint64_t astride, long long src) {
  int32_t a;
  __builtin_memcpy(&a, __builtin_assume_aligned(reinterpret_cast<const uint8_t*>(actions) + (size_t)src * astride, 4), 4);
  return a;
}
// the share of minibatch row i in W
BG_HEAD_FN double bg_bc_weight_of(const float* weights, const int32_t* index, long long store_rows, long long i) {
  const long long src = index ? (long long)index[i] : i;
  if (index && (src < 0 || src >= store_rows)) return 0.0;
  if (!weights) return 1.0;
  const float w = weights[src];
  return bg_bc_weight_ok(w) ? (double)w : 0.0;
}

#ifdef BG_BC_HOST
// ---- the serial twin: the launch sequence below, one "workgroup" after the other, in the orders of the contract ----
static inline double bg_bc_host_weight_sum(const BgBcArgs& A) {
  const uint64_t P = bg_ppo_stat_parts(A.m);
  double* part = new double[P ? P : 1];
  for (uint64_t b = 0; b < P; b++) {
    double t[BG_PPO_LANES];
    for (int r = 0; r < BG_PPO_LANES; r++) {
      const long long i = (long long)b * BG_PPO_LANES + r;
      t[r] = i < A.m ? bg_bc_weight_of(A.weights, A.index, A.store_rows, i) : 0.0;
    }
    part[b] = bg_loss_host_tree(t, BG_PPO_LANES, 0, BgLossSum{});
  }
  const double W = bg_loss_host_slices(part, P, 1, 0, 0.0, BgLossSum{});
  delete[] part;
  return W;
}

// bf16: logits and dlogits are bfloat16 bits.  Every pointer is a host pointer; A.head / A.partials / A.fm are not used.
static inline void bg_bc_host(const BgBcArgs& A, bool bf16, bool keep, float* stats) {
  const double W = (A.weights || A.index) ? bg_bc_host_weight_sum(A) : (double)A.m;
  const float Wf = (float)W;
  const uint64_t P = bg_ppo_row_parts(A.m);
  double* part = new double[(P ? P : 1) * BG_BC_SUMS];
  for (uint64_t b = 0; b < P; b++) {
    double t[BG_BC_SUMS][BG_PPO_ROWS];
    for (int r = 0; r < BG_PPO_ROWS; r++) {
      const long long i = (long long)b * BG_PPO_ROWS + r;
      for (int k = 0; k < BG_BC_SUMS; k++) t[k][r] = 0.0;
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
      const int32_t a = ok ? bg_bc_action(A.actions, A.astride, src) : -1;
      const float w = A.weights && ok ? A.weights[src] : 1.0f;
      BgBcTerms o;
      if (A.mask) o = keep ? bg_bc_row<true, true>(l, kw, E, ok, a, w, A.ent_coef, Wf) : bg_bc_row<true, false>(l, kw, E, ok, a, w, A.ent_coef, Wf);
      else o = keep ? bg_bc_row<false, true>(l, kw, E, ok, a, w, A.ent_coef, Wf) : bg_bc_row<false, false>(l, kw, E, ok, a, w, A.ent_coef, Wf);
      if (!o.excluded) { t[0][r] = (double)w * (double)o.nll; t[1][r] = (double)w * (double)o.entropy; t[2][r] = (double)w * (double)o.hit; }
      t[3][r] = (double)o.excluded;
      for (int j = 0; j < BG_HEAD_ACTIONS; j++) {
        if (bf16) ((uint16_t*)A.dlogits)[(size_t)i * A.dstride + j] = bg_ppo_bf16(l[j]);
        else ((float*)A.dlogits)[(size_t)i * A.dstride + j] = l[j];
      }
      if (A.log_prob) A.log_prob[i] = o.log_prob;
      if (A.entropy) A.entropy[i] = o.entropy;
    }
    bg_loss_host_tile<BG_BC_SUMS>(t, part + b * BG_BC_SUMS, BgLossSum{});
  }
  double sum[BG_BC_SUMS];
  bg_loss_host_finish<BG_BC_SUMS>(part, P, sum, BgLossSum{});
  delete[] part;
  bg_bc_finish_stats(sum, W, A.m, A.ent_coef, stats);
}
#else
// ---- the kernels ----
// bg_bc_kernel is bg_ppo_kernel with another row function: ONE wave and BG_HEAD_ROWS = 64 consecutive minibatch rows per workgroup; the logits come in
// through bg_head_stage_logits, the masks through bg_head_stage_mask or (with an index) bg_ppo_stage_mask_gather; lane = row runs bg_bc_row over its LDS
// row and leaves the 60 gradient values IN that row; the row's scalar inputs are two 4-byte gathers (the action at its byte pitch, the weight); the
// four float64 terms go through a 64-entry LDS tree; the tile leaves through bg_ppo_store_rows.
// LDS: 15 616 bytes of logits / gradient + 3 840 of masks + 2 048 of sums (+ 15 616 with -DBG_PPO_KEEP_E).

// the weights of the call -> one float64 sum per 256 rows
__global__ __launch_bounds__(BG_PPO_LANES) void bg_bc_weight_partials(const float* __restrict__ weights, const int32_t* __restrict__ index, long long store_rows,
                                                                      long long m, double* __restrict__ part) {
  __shared__ double t[BG_PPO_LANES];
  const long long i = (long long)blockIdx.x * BG_PPO_LANES + threadIdx.x;
  bg_loss_stat_partials(i < m ? bg_bc_weight_of(weights, index, store_rows, i) : 0.0, t, part, BgLossSum{});
}

// one workgroup: the partial sums -> head: float Wf at 0, double W at byte 8
__global__ __launch_bounds__(BG_PPO_LANES) void bg_bc_weight_combine(const double* __restrict__ part, long long P, float* __restrict__ head) {
  __shared__ double t[BG_PPO_LANES];
  bg_loss_stat_combine(part, P, 0.0, t, BgLossSum{});
  if (threadIdx.x == 0) {
    head[0] = (float)t[0];
    head[1] = 0.0f;
    reinterpret_cast<double*>(head)[1] = t[0];
  }
}

template <bool BF16>
__global__ __launch_bounds__(BG_HEAD_BLOCK) void bg_bc_kernel(const BgBcArgs A) {
  __shared__ float lg[BG_HEAD_ROWS * BG_HEAD_LPITCH];
  __shared__ float ek[BG_PPO_KEEP ? BG_HEAD_ROWS * BG_HEAD_LPITCH : 1];
  __shared__ uint32_t mk[BG_HEAD_ROWS * BG_HEAD_MWORDS];
  __shared__ double red[BG_BC_SUMS * BG_HEAD_ROWS];
  const long long rec0 = (long long)blockIdx.x * BG_HEAD_ROWS;
  const int nrow = (int)(A.m - rec0 < BG_HEAD_ROWS ? A.m - rec0 : BG_HEAD_ROWS);
  bg_loss_stage<BF16>(A.logits, A.lld, A.lstride, A.mask, A.mld, A.mstride, A.index, A.store_rows, rec0, nrow, lg, mk);
  __syncthreads();
  const int r = threadIdx.x;
  double t[BG_BC_SUMS];
#pragma unroll
  for (int k = 0; k < BG_BC_SUMS; k++) t[k] = 0.0;
  if (r < nrow) {
    const long long i = rec0 + r;
    const long long src = A.index ? (long long)A.index[i] : i;
    const bool ok = !A.index || (src >= 0 && src < A.store_rows);
    const int32_t a = ok ? bg_bc_action(A.actions, A.astride, src) : -1;
    const float w = A.weights && ok ? A.weights[src] : 1.0f;
    const float Wf = A.head ? A.head[0] : A.fm;
    float* const l = lg + r * BG_HEAD_LPITCH;
    float* const E = ek + (BG_PPO_KEEP ? r * BG_HEAD_LPITCH : 0);
    const uint32_t* const k = mk + r * BG_HEAD_MWORDS;
    const BgBcTerms o = A.mld != BG_HEAD_LD_NONE ? bg_bc_row<true, BG_PPO_KEEP>(l, k, E, ok, a, w, A.ent_coef, Wf)
                                                 : bg_bc_row<false, BG_PPO_KEEP>(l, k, E, ok, a, w, A.ent_coef, Wf);
    if (!o.excluded) { t[0] = (double)w * (double)o.nll; t[1] = (double)w * (double)o.entropy; t[2] = (double)w * (double)o.hit; }
    t[3] = (double)o.excluded;
    if (A.log_prob) A.log_prob[i] = o.log_prob;
    if (A.entropy) A.entropy[i] = o.entropy;
  }
  bg_loss_tile_reduce<BG_BC_SUMS>(t, red, A.partials, blockIdx.x, BgLossSum{});
  bg_ppo_store_rows<BF16>(A.dlogits, A.dst, A.dstride, rec0, nrow, lg);
}

// one workgroup: the row partials -> stats[BG_BC_STATS]
__global__ __launch_bounds__(BG_PPO_LANES) void bg_bc_finish(const double* __restrict__ partials, long long P, long long m, float ent_coef,
                                                             const float* __restrict__ head, float* __restrict__ stats) {
  __shared__ double t[BG_BC_SUMS * BG_PPO_LANES];
  const int r = threadIdx.x;
  const long long per = (P + BG_PPO_LANES - 1) / BG_PPO_LANES;
  double acc[BG_BC_SUMS];
#pragma unroll
  for (int k = 0; k < BG_BC_SUMS; k++) acc[k] = 0.0;
  for (long long p = r * per; p < P && p < (r + 1) * per; p++) {
#pragma unroll
    for (int k = 0; k < BG_BC_SUMS; k++) acc[k] = acc[k] + partials[p * BG_BC_SUMS + k];
  }
#pragma unroll
  for (int k = 0; k < BG_BC_SUMS; k++) t[k * BG_PPO_LANES + r] = acc[k];
  __syncthreads();
  for (int s = BG_PPO_LANES / 2; s; s >>= 1) {
    if (r < s) {
#pragma unroll
      for (int k = 0; k < BG_BC_SUMS; k++) t[k * BG_PPO_LANES + r] = t[k * BG_PPO_LANES + r] + t[k * BG_PPO_LANES + r + s];
    }
    __syncthreads();
  }
  if (r == 0) {
    double sum[BG_BC_SUMS];
#pragma unroll
    for (int k = 0; k < BG_BC_SUMS; k++) sum[k] = t[k * BG_PPO_LANES];
    bg_bc_finish_stats(sum, head ? reinterpret_cast<const double*>(head)[1] : (double)m, m, ent_coef, stats);
  }
}
#endif  // BG_BC_HOST
#endif
