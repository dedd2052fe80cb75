// bg_dqn.h -- bg_dqn_loss: DQN's temporal-difference loss over packed records, with its gradient, in one pass over the minibatch; and
// bg_sample_actions_eps: epsilon-greedy exploration in the masked head of bg_head.h.
//
// The reference's main training script offers `--algorithm {PPO, DQN, A2C}` (train_balatro_agent.py); its DQN configuration (lines 344-362) names a
// replay buffer of 100 000 transitions, batch 32, exploration from 1.0 to 0.05, target_update_interval 1000 and tau 1.0.  A ring of packed records IS
// that replay buffer (vec_env.RowReplay): a record carries the observation and mask of the next decision and the action, reward, terminated byte and
// end flags of the step that produced it.  bg_dqn_loss is SB3's `DQN.train` between "two [m, 60] Q matrices" and "a gradient": it replaces the torch
// composite gather -> masked max -> where(done) -> multiply-add -> smooth_l1_loss -> mean and its backward.
// The per-row arithmetic is plain C++ behind BG_HEAD_FN: define BG_DQN_HOST before including and the text the GPU runs compiles with g++, with a serial
// twin of the launch sequence (bg_dqn_host).  The library is built with -ffp-contract=off (build.FLAGS), as the host twin is: nothing is fused.
//
// THE CONTRACT.  Everything is float32 and every operation rounds on its own, except the sums across rows, which are float64.
//   row i        reads q[i, :], q_next[i, :] (and q_next_online[i, :]) at minibatch row i, and the record nx = next_index[i] of store_rows records: the
//                transition's NEXT record.  a = its BG_ROW_ACTION;  r = float(its float64 BG_ROW_REWARD), or rewards[nx] when rewards is given;
//                done = its BG_ROW_TERMINATED byte != 0;  end_flags = its BG_ROW_END_FLAGS byte;  with BG_DQN_MASK_NEXT its 60 BG_ROW_ACTION_MASK bytes.
//                (The observation record is not an argument: the caller computed q from it.)
//   V'           the j whose mask byte is non-zero (BG_DQN_MASK_NEXT), else all 60.
//   plain        n = max over V' of q_next[j]
//   double       (q_next_online given)  a' = the smallest j in V' with q_next_online[j] == max over V' of q_next_online;  n = q_next[a']
//   target       y = done ? r : r + gamma * n          (a done row reads neither q_next matrix: a NaN there does not matter)
//   loss         d = q[a] - y;  Huber (SB3's smooth_l1, beta 1):  term = |d| < 1 ? (0.5 * d) * d : |d| - 0.5;  g = |d| < 1 ? d : copysign(1, d)
//                BG_DQN_MSE:  term = d * d;  g = 2 * d
//   gradient     dq[i, a] = g / float(m); every other column of the row +0.0.  bfloat16 output is this float32 value rounded to nearest even.  Padding
//                columns of a strided dq are not written.  td[i] = d.
//   EXCLUDED     next_index outside [0, store_rows) (nothing is read for the row); the action outside [0, 60); r or q[a] not finite; the row not done and
//                V' empty, or a Q value that enters a max NaN, or n not finite; BG_DQN_TIMEOUT_EXCLUDE set, the row done and end_flags == BG_END_MAX_STEPS
//                exactly.  Such a row has a dq row of +0.0 and td = quiet NaN, adds nothing to any sum, is counted, and the divisor stays m.
//   sums         per included row, as float64: term, q[a], y, |d|, done (0 / 1); per row: excluded (0 / 1); and the maximum of |d| over the included rows.
//                A workgroup is 64 consecutive rows and folds them by bg_ppo.h's TREE; the workgroups' partials (caller's workspace) are folded by
//                SLICES-THEN-TREE with 256 lanes in a one-workgroup kernel (the maximum takes the same path with max in place of +).  Then, in float64,
//                stats = sum term / m, sum q[a] / m, sum y / m, sum |d| / m, max |d|, sum done / m, excluded, m: each rounded to float32 once.
// No floating-point atomics and a fixed launch sequence (rows, finish): two calls give the same bits.
// STEP-LIMIT ENDINGS.  SB3 bootstraps a row that only the step limit ended from `terminal_observation`.  That record is not in the ring
// (EpisodeLimits.terminal() has it only until the next call), so BG_DQN_TIMEOUT_EXCLUDE leaves such a row out; without the flag it is an ordinary done
// row (y = r).  Bootstrapping it from the terminal record is out of scope.  At a 1000-step limit these are at most one row in a thousand.
// Out of scope: Polyak / hard target updates, the optimiser, gradient clipping, prioritised sampling (td is provided for it), n-step returns.
//
// EPSILON-GREEDY (bg_sample_actions_eps).  h = bg_head_hash(seed, index0 + i, t) and u = bg_head_u(h) as bg_sample_actions draws them;
// explore = u < epsilon (an exact float32 comparison).  A greedy row takes the BG_HEAD_DETERMINISTIC rule.  An exploring row takes
// h2 = bg_head_hash(seed + 0x632BE59BD9B4E019 (mod 2^64), index0 + i, t) and, with k the number of valid actions, the ((uint64)h2 * k) >> 32 -th valid
// action in index order.  A row the head calls degenerate gives -1 in both branches.  DEVIATION: the decision is per env.  SB3 draws once for the whole
// batch, which at 65 536 envs would make every env explore together.
#ifndef BG_DQN_H
#define BG_DQN_H
#if defined(BG_DQN_HOST) && !defined(BG_PPO_HOST)
#define BG_PPO_HOST
#endif
#include "bg_ppo.h"   // bg_head.h's tile loads, bg_ppo_store_rows, bg_ppo_stage_mask_gather, bg_ppo_bf16 / _finite: one copy of each

#define BG_DQN_SUMS 7      /* term, q[a], y, |d|, done, excluded: sums; [6]: the maximum of |d| */
#define BG_DQN_MAX 6
#define BG_DQN_ROWS BG_PPO_ROWS     /* rows per workgroup partial */
#define BG_DQN_LANES BG_PPO_LANES   /* lanes of the finishing workgroup */
#define BG_DQN_EPS_SALT 0x632BE59BD9B4E019ull
#define BG_HEAD_EPS 3      /* the head's fourth mode: bg_sample_actions_eps */

BG_HEAD_FN uint64_t bg_dqn_row_parts(long long m) { return ((uint64_t)m + BG_DQN_ROWS - 1) / BG_DQN_ROWS; }
BG_HEAD_FN double bg_dqn_fold(int k, double a, double b) { return k == BG_DQN_MAX ? (b > a ? b : a) : a + b; }
struct BgDqnFold { BG_LOSS_FOLD double operator()(int k, double a, double b) const { return bg_dqn_fold(k, a, b); } };

struct BgDqnTerms {
  float term, qa, y, absd, td, dq;
  int32_t done, excluded;
};

// One row.  qn: the 60 target-network values at the next record; qo: the online network's there (DOUBLE); kw: the next record's mask words (MASKED).
// src_ok: next_index is in range; a, r, done, end_flags: the record's fields; qa: q[a] (read only when src_ok and a is in range).
template <bool MASKED, bool DOUBLE>
BG_HEAD_FN BgDqnTerms bg_dqn_row(const float* qn, const float* qo, const uint32_t* kw, bool src_ok, int32_t a, float r, float qa, bool done,
                                 uint32_t end_flags, float gamma, uint32_t flags, float fm) {
  const float ninf = bg_head_from_bits(BG_HEAD_NEG_INF), qnan = bg_head_from_bits(BG_HEAD_QNAN);
  BgDqnTerms o;
  o.term = 0.0f; o.qa = 0.0f; o.y = 0.0f; o.absd = 0.0f; o.td = qnan; o.dq = 0.0f; o.done = 0; o.excluded = 1;
  if (!src_ok || a < 0 || a >= BG_HEAD_ACTIONS) return o;
  if (!bg_ppo_finite(r) || !bg_ppo_finite(qa)) return o;
  if (done && (flags & BG_DQN_TIMEOUT_EXCLUDE) && end_flags == BG_END_MAX_STEPS) return o;
  float y = r;
  if (!done) {
    const float* const sel = DOUBLE ? qo : qn;
    float mx = ninf;
    int32_t arg = -1;
    bool nan = false;
#pragma unroll
    for (int j = 0; j < BG_HEAD_ACTIONS; j++) {
      const bool ok = !MASKED || bg_head_valid(kw, j);
      const float x = sel[j];
      nan = nan || (ok && x != x);
      const bool up = ok && (arg < 0 || x > mx);   // the first valid j, then every strictly larger one: ends on the smallest j of the maximum
      mx = up ? x : mx;
      arg = up ? j : arg;
    }
    if (arg < 0 || nan) return o;
    const float n = DOUBLE ? qn[arg] : mx;
    if (!bg_ppo_finite(n)) return o;
    y = r + gamma * n;
  }
  const float d = qa - y;
  const float ad = fabsf(d);
  float g;
  if (flags & BG_DQN_MSE) { o.term = d * d; g = 2.0f * d; }
  else if (ad < 1.0f) { o.term = (0.5f * d) * d; g = d; }
  else { o.term = ad - 0.5f; g = copysignf(1.0f, d); }
  o.qa = qa; o.y = y; o.absd = ad; o.td = d; o.dq = g / fm; o.done = done ? 1 : 0; o.excluded = 0;
  return o;
}

// what the finishing step writes: stats[BG_DQN_STATS] from the folded values
BG_HEAD_FN void bg_dqn_finish_stats(const double* sum, long long m, float* stats) {
  const double dm = (double)m;
  stats[0] = (float)(sum[0] / dm);
  stats[1] = (float)(sum[1] / dm);
  stats[2] = (float)(sum[2] / dm);
  stats[3] = (float)(sum[3] / dm);
  stats[4] = (float)sum[BG_DQN_MAX];
  stats[5] = (float)(sum[4] / dm);
  stats[6] = (float)sum[5];
  stats[7] = (float)dm;
}

struct BgDqnArgs {
  const void* q; uint64_t qstride;
  const void* qn; uint64_t nstride; int nld;
  const void* qo; uint64_t ostride; int old;
  const uint8_t* rows; uint64_t rstride; long long store_rows;
  const int32_t* next_index; const float* rewards; long long m;
  float gamma, fm; uint32_t flags;
  void* dq; uint64_t dstride; int dst;
  float* td;
  double* partials;   // workspace: [row partials][BG_DQN_SUMS]
};

// the record fields of one row, from the record at `rec` (16-byte aligned)
struct BgDqnFields { int32_t a; float r; bool done; uint32_t end_flags; };
BG_HEAD_FN BgDqnFields bg_dqn_fields(const uint8_t* rec_) {
  const uint8_t* const rec = (const uint8_t*)__builtin_assume_aligned(rec_, 16);
  BgDqnFields f;
  double r64;
  uint32_t tail;
  __builtin_memcpy(&f.a, rec + BG_ROW_ACTION, 4);
  __builtin_memcpy(&r64, rec + BG_ROW_REWARD, 8);
  __builtin_memcpy(&tail, rec + (BG_ROW_TERMINATED & ~3), 4);   // bytes 340..343: the terminated byte and the end flags
  f.r = (float)r64;
  f.done = ((tail >> ((BG_ROW_TERMINATED & 3) * 8)) & 0xffu) != 0u;
  f.end_flags = (tail >> ((BG_ROW_END_FLAGS & 3) * 8)) & 0xffu;
  return f;
}
static_assert(BG_ROW_ACTION % 4 == 0 && BG_ROW_REWARD % 8 == 0 && (BG_ROW_TERMINATED & ~3) == (BG_ROW_END_FLAGS & ~3), "aligned fields; both bytes in one word");

// One row of bg_sample_actions_eps.  l, kw as bg_head_row; u = bg_head_u(h); h2: the second hash.
template <bool MASKED>
BG_HEAD_FN int32_t bg_head_eps_row(const float* l, const uint32_t* kw, float u, float epsilon, uint32_t h2) {
  const float ninf = bg_head_from_bits(BG_HEAD_NEG_INF);
  float m = ninf;
  int32_t arg = -1;
  uint32_t k = 0;
  bool nan = false;
#pragma unroll
  for (int j = 0; j < BG_HEAD_ACTIONS; j++) {   // pass 1 of bg_head_row, and the number of valid actions
    const bool ok = !MASKED || bg_head_valid(kw, j);
    const float v = l[j];
    nan = nan || (ok && v != v);
    const bool up = ok && v > m;
    m = up ? v : m;
    arg = up ? j : arg;
    k += ok ? 1u : 0u;
  }
  if (nan || m == ninf || m == -ninf) return -1;
  if (!(u < epsilon)) return arg;
  const uint32_t pick = (uint32_t)(((uint64_t)h2 * (uint64_t)k) >> 32);   // < k
  uint32_t seen = 0;
  int32_t a = -1;
#pragma unroll
  for (int j = 0; j < BG_HEAD_ACTIONS; j++) {
    const bool ok = !MASKED || bg_head_valid(kw, j);
    a = (ok && seen == pick) ? j : a;
    seen += ok ? 1u : 0u;
  }
  return a;
}

#ifdef BG_DQN_HOST
// ---- the serial twin: the launch sequence below, one "workgroup" after the other, in the orders of the contract.  Every pointer is a host pointer. ----
static inline void bg_dqn_host(const BgDqnArgs& A, bool bf16, float* stats) {
  const uint64_t P = bg_dqn_row_parts(A.m);
  double* part = new double[(P ? P : 1) * BG_DQN_SUMS];
  const bool masked = (A.flags & BG_DQN_MASK_NEXT) != 0, dbl = A.qo != nullptr;
  for (uint64_t b = 0; b < P; b++) {
    double t[BG_DQN_SUMS][BG_DQN_ROWS];
    for (int r = 0; r < BG_DQN_ROWS; r++) {
      const long long i = (long long)b * BG_DQN_ROWS + r;
      for (int k = 0; k < BG_DQN_SUMS; k++) t[k][r] = 0.0;
      if (i >= A.m) continue;
      float qn[BG_HEAD_ACTIONS], qo[BG_HEAD_ACTIONS], out[BG_HEAD_ACTIONS];
      uint32_t kw[BG_HEAD_ACTIONS / 4] = {};
      for (int j = 0; j < BG_HEAD_ACTIONS; j++) {
        if (bf16) {
          qn[j] = bg_head_widen_bf16(((const uint16_t*)A.qn)[(size_t)i * A.nstride + j]);
          qo[j] = dbl ? bg_head_widen_bf16(((const uint16_t*)A.qo)[(size_t)i * A.ostride + j]) : 0.0f;
        } else {
          qn[j] = ((const float*)A.qn)[(size_t)i * A.nstride + j];
          qo[j] = dbl ? ((const float*)A.qo)[(size_t)i * A.ostride + j] : 0.0f;
        }
        out[j] = 0.0f;
      }
      const long long nx = A.next_index[i];
      const bool ok = nx >= 0 && nx < A.store_rows;
      BgDqnFields f;
      f.a = -1; f.r = 0.0f; f.done = false; f.end_flags = 0;
      float qa = 0.0f;
      if (ok) {
        const uint8_t* const rec = A.rows + (size_t)nx * A.rstride;
        f = bg_dqn_fields(rec);
        if (A.rewards) f.r = A.rewards[nx];
        if (masked) memcpy(kw, rec + BG_ROW_ACTION_MASK, BG_HEAD_ACTIONS);
        if (f.a >= 0 && f.a < BG_HEAD_ACTIONS)
          qa = bf16 ? bg_head_widen_bf16(((const uint16_t*)A.q)[(size_t)i * A.qstride + f.a]) : ((const float*)A.q)[(size_t)i * A.qstride + f.a];
      }
      BgDqnTerms o;
      if (masked) o = dbl ? bg_dqn_row<true, true>(qn, qo, kw, ok, f.a, f.r, qa, f.done, f.end_flags, A.gamma, A.flags, A.fm)
                          : bg_dqn_row<true, false>(qn, qo, kw, ok, f.a, f.r, qa, f.done, f.end_flags, A.gamma, A.flags, A.fm);
      else o = dbl ? bg_dqn_row<false, true>(qn, qo, kw, ok, f.a, f.r, qa, f.done, f.end_flags, A.gamma, A.flags, A.fm)
                   : bg_dqn_row<false, false>(qn, qo, kw, ok, f.a, f.r, qa, f.done, f.end_flags, A.gamma, A.flags, A.fm);
      if (!o.excluded) {
        t[0][r] = (double)o.term; t[1][r] = (double)o.qa; t[2][r] = (double)o.y; t[3][r] = (double)o.absd; t[4][r] = (double)o.done;
        t[BG_DQN_MAX][r] = (double)o.absd;
        out[f.a] = o.dq;
      }
      t[5][r] = (double)o.excluded;
      for (int j = 0; j < BG_HEAD_ACTIONS; j++) {
        if (bf16) ((uint16_t*)A.dq)[(size_t)i * A.dstride + j] = bg_ppo_bf16(out[j]);
        else ((float*)A.dq)[(size_t)i * A.dstride + j] = out[j];
      }
      if (A.td) A.td[i] = o.td;
    }
    bg_loss_host_tile<BG_DQN_SUMS>(t, part + b * BG_DQN_SUMS, BgDqnFold{});
  }
  double sum[BG_DQN_SUMS];
  bg_loss_host_finish<BG_DQN_SUMS>(part, P, sum, BgDqnFold{});
  delete[] part;
  bg_dqn_finish_stats(sum, A.m, stats);
}
#else
// ---- the kernels ----
// bg_dqn_kernel has bg_ppo_kernel's shape: a workgroup is ONE wave and BG_HEAD_ROWS = 64 consecutive minibatch rows.
//   1  q_next (and, DOUBLE, q_next_online) come in through bg_head_stage_logits into LDS at the odd pitch of 61 words; with BG_DQN_MASK_NEXT the masks
//      come row by row from record next_index[i] through bg_ppo_stage_mask_gather (16-byte pieces: a record's mask sits at a 16-byte aligned offset of a
//      16-byte aligned row; an index out of range stages an all-invalid mask and reads nothing).
//   2  lane = row reads its record's fields (four aligned loads) and ONE element of q, q[i, a] -- the only element of that matrix the loss needs, so the
//      q matrix is never staged -- runs bg_dqn_row over its LDS rows, then overwrites its own q_next row with the gradient row: 60 zeros and dq[a].
//      The seven float64 terms go through a 64-entry LDS tree, and lane 0 writes the workgroup's partial.
//   3  after the barrier the tile leaves for HBM through bg_ppo_store_rows: consecutive lanes on consecutive 16-byte pieces, words or halves, chosen by
//      the alignment of dq.  That write is nearly all zeros but autograd reads the whole row; it dominates the traffic.
// LDS: 15 616 bytes of q_next / gradient (+ 15 616 DOUBLE) + 3 840 of masks + 3 584 of sums.
template <bool BF16, bool DOUBLE>
__global__ __launch_bounds__(BG_HEAD_BLOCK) void bg_dqn_kernel(const BgDqnArgs A) {
  __shared__ float qn[BG_HEAD_ROWS * BG_HEAD_LPITCH];
  __shared__ float qo[DOUBLE ? BG_HEAD_ROWS * BG_HEAD_LPITCH : 1];
  __shared__ uint32_t mk[BG_HEAD_ROWS * BG_HEAD_MWORDS];
  __shared__ double red[BG_DQN_SUMS * BG_HEAD_ROWS];
  const long long rec0 = (long long)blockIdx.x * BG_HEAD_ROWS;
  const int nrow = (int)(A.m - rec0 < BG_HEAD_ROWS ? A.m - rec0 : BG_HEAD_ROWS);
  const bool masked = (A.flags & BG_DQN_MASK_NEXT) != 0u;
  bg_head_stage_logits<BF16>(A.qn, A.nld, A.nstride, rec0, nrow, qn);
  if (DOUBLE) bg_head_stage_logits<BF16>(A.qo, A.old, A.ostride, rec0, nrow, qo);
  if (masked)
    bg_ppo_stage_mask_gather(reinterpret_cast<const int8_t*>(A.rows + BG_ROW_ACTION_MASK), BG_HEAD_LD_ROWS16, A.rstride, A.next_index, A.store_rows, rec0, nrow, mk);
  __syncthreads();
  const int r = threadIdx.x;
  double t[BG_DQN_SUMS];
#pragma unroll
  for (int k = 0; k < BG_DQN_SUMS; k++) t[k] = 0.0;
  if (r < nrow) {
    const long long i = rec0 + r;
    const long long nx = (long long)A.next_index[i];
    const bool ok = nx >= 0 && nx < A.store_rows;
    BgDqnFields f;
    f.a = -1; f.r = 0.0f; f.done = false; f.end_flags = 0u;
    float qa = 0.0f;
    if (ok) {
      f = bg_dqn_fields(A.rows + (size_t)nx * A.rstride);
      if (A.rewards) f.r = A.rewards[nx];
      if (f.a >= 0 && f.a < BG_HEAD_ACTIONS) {
        const uint8_t* const src = reinterpret_cast<const uint8_t*>(A.q) + ((size_t)i * A.qstride + (size_t)f.a) * (BF16 ? 2 : 4);
        qa = BF16 ? bg_head_widen_bf16(*reinterpret_cast<const uint16_t*>(src)) : *reinterpret_cast<const float*>(src);
      }
    }
    float* const l = qn + r * BG_HEAD_LPITCH;
    const float* const lo = qo + (DOUBLE ? r * BG_HEAD_LPITCH : 0);
    const uint32_t* const k = mk + r * BG_HEAD_MWORDS;
    const BgDqnTerms o = masked ? bg_dqn_row<true, DOUBLE>(l, lo, k, ok, f.a, f.r, qa, f.done, f.end_flags, A.gamma, A.flags, A.fm)
                                : bg_dqn_row<false, DOUBLE>(l, lo, k, ok, f.a, f.r, qa, f.done, f.end_flags, A.gamma, A.flags, A.fm);
#pragma unroll
    for (int j = 0; j < BG_HEAD_ACTIONS; j++) l[j] = 0.0f;
    if (!o.excluded) {
      l[f.a] = o.dq;   // 0 <= f.a < 60: an included row's action is in range
      t[0] = (double)o.term; t[1] = (double)o.qa; t[2] = (double)o.y; t[3] = (double)o.absd; t[4] = (double)o.done; t[BG_DQN_MAX] = (double)o.absd;
    }
    t[5] = (double)o.excluded;
    if (A.td) A.td[i] = o.td;
  }
  bg_loss_tile_reduce<BG_DQN_SUMS>(t, red, A.partials, blockIdx.x, BgDqnFold{});
  bg_ppo_store_rows<BF16>(A.dq, A.dst, A.dstride, rec0, nrow, qn);
}

// one workgroup: the row partials -> stats[BG_DQN_STATS]
__global__ __launch_bounds__(BG_DQN_LANES) void bg_dqn_finish(const double* __restrict__ partials, long long P, long long m, float* __restrict__ stats) {
  __shared__ double t[BG_DQN_SUMS * BG_DQN_LANES];
  const int r = threadIdx.x;
  const long long per = (P + BG_DQN_LANES - 1) / BG_DQN_LANES;
  double acc[BG_DQN_SUMS];
#pragma unroll
  for (int k = 0; k < BG_DQN_SUMS; k++) acc[k] = 0.0;
  for (long long p = r * per; p < P && p < (r + 1) * per; p++) {
#pragma unroll
    for (int k = 0; k < BG_DQN_SUMS; k++) acc[k] = bg_dqn_fold(k, acc[k], partials[p * BG_DQN_SUMS + k]);
  }
#pragma unroll
  for (int k = 0; k < BG_DQN_SUMS; k++) t[k * BG_DQN_LANES + r] = acc[k];
  __syncthreads();
  for (int s = BG_DQN_LANES / 2; s; s >>= 1) {
    if (r < s) {
#pragma unroll
      for (int k = 0; k < BG_DQN_SUMS; k++) t[k * BG_DQN_LANES + r] = bg_dqn_fold(k, t[k * BG_DQN_LANES + r], t[k * BG_DQN_LANES + r + s]);
    }
    __syncthreads();
  }
  if (r == 0) {
    double sum[BG_DQN_SUMS];
#pragma unroll
    for (int k = 0; k < BG_DQN_SUMS; k++) sum[k] = t[k * BG_DQN_LANES];
    bg_dqn_finish_stats(sum, m, stats);
  }
}

// bg_sample_actions_eps: bg_head_kernel's staging, bg_head_eps_row per lane.  m >= 1.
__global__ __launch_bounds__(BG_HEAD_BLOCK) void bg_head_eps_kernel(const void* __restrict__ logits, int bf16, int lld, uint64_t lstride,
                                                                    const int8_t* __restrict__ mask, int mld, uint64_t mstride, long long m, uint64_t seed,
                                                                    uint64_t index0, uint64_t t, float epsilon, int32_t* __restrict__ actions_out) {
  __shared__ float lg[BG_HEAD_ROWS * BG_HEAD_LPITCH];
  __shared__ uint32_t mk[BG_HEAD_ROWS * BG_HEAD_MWORDS];
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
  const uint32_t* const k = mk + r * BG_HEAD_MWORDS;
  const float u = bg_head_u(bg_head_hash(seed, index0 + (uint64_t)i, t));
  const uint32_t h2 = bg_head_hash(seed + BG_DQN_EPS_SALT, index0 + (uint64_t)i, t);
  actions_out[i] = mld != BG_HEAD_LD_NONE ? bg_head_eps_row<true>(l, k, u, epsilon, h2) : bg_head_eps_row<false>(l, k, u, epsilon, h2);
}
#endif  // BG_DQN_HOST
#endif
