// bg_ends.h -- bg_episode_ends_rows: the scan that turns a finished [K, N] rollout of packed records into a report of its ended episodes and into
// the curriculum's cap updates (include/balatro_mi355x.h has the contract).
//
// An ended step's record -- byte BG_ROW_TERMINATED set -- says why in byte BG_ROW_END_FLAGS and, when the handle's episode summary was on
// (bg_set_episode_summary), what the episode reached in bytes BG_ROW_END_ANTE / _ROUND / _CHIPS.  All of that lies in the record's last 16 bytes
// (336..351), so a record costs ONE 16-byte load, i.e. one 128-byte line of HBM traffic.  The scan is the shape of bg_gae.h's episode scan: lane = env,
// one wave per workgroup, forwards along K in batches whose loads are all issued before the first is used.  Per env it is SERIAL in t -- the
// curriculum's rule (CurriculumTracker.update, sb3_adapter.py; CurriculumBalatroEnv, train_balatro_agent.py:126-170) depends on the order of an
// env's endings -- and the envs are independent: the report's sums are integers, so integer atomics give the same values on every run.
// The per-record rule is plain C++ behind BG_ENDS_FN, so the text the GPU runs compiles with g++ (define BG_ENDS_HOST before including, with
// include/balatro_mi355x.h in front; the pattern of bg_safe.h / bg_gae.h): tests/test_episode_ends_host.py drives it.
#ifndef BG_ENDS_H
#define BG_ENDS_H
#include <stdint.h>

#ifdef BG_ENDS_HOST
#define BG_ENDS_FN static inline
#else
#define BG_ENDS_FN __host__ __device__ __forceinline__
#endif

#define BG_ENDS_TAIL 336   // the 16 bytes of a record the scan reads: 336..351 (records are 16-byte aligned)
// the report's words (int64 [BG_ENDS_WORDS])
#define BG_ENDS_W_ENDED 0
#define BG_ENDS_W_GAME 1
#define BG_ENDS_W_INVALID 2
#define BG_ENDS_W_MAX_STEPS 3
#define BG_ENDS_W_ANTE_SUM 4
#define BG_ENDS_W_ANTE_MAX 5
#define BG_ENDS_W_CHIPS_SUM 6
#define BG_ENDS_W_CHIPS_MAX 7
#define BG_ENDS_W_RAISED 8
#define BG_ENDS_W_NO_SUMMARY 9
#define BG_ENDS_W_HIST 16
#define BG_ENDS_HIST_TOP 15   // antes of 15 and more share the last bin
#define BG_ENDS_CAP_MAX 255   // Env::max_ante is a byte

// ---- one record: words 1..3 of its last 16 bytes (bytes 340..351, little endian) ----
struct BgEndRec {
  bool ended;       // byte BG_ROW_TERMINATED
  uint32_t flags;   // byte BG_ROW_END_FLAGS
  int32_t ante;     // BG_ROW_END_ANTE (int16); <= 0: the record was made without the episode summary
  int32_t round;    // BG_ROW_END_ROUND (int8)
  uint32_t chips;   // BG_ROW_END_CHIPS
};
BG_ENDS_FN BgEndRec bg_ends_record(uint32_t w1, uint32_t w2, uint32_t w3) {
  BgEndRec r;
  r.ended = ((w1 >> 16) & 0xffu) != 0u;
  r.flags = w1 >> 24;
  r.ante = (int32_t)(int16_t)(uint16_t)(w2 & 0xffffu);
  r.round = (int32_t)(int8_t)(uint8_t)((w2 >> 16) & 0xffu);
  r.chips = w3;
  return r;
}

// ---- the report: one env's (one lane's) share ----
struct BgEndsAcc {
  uint32_t ended, game, invalid, max_steps, no_summary;   // (an env ends at most K < 2**31 times in a call)
  uint64_t ante_sum, chips_sum;
  uint32_t ante_max, chips_max;
};
BG_ENDS_FN void bg_ends_acc_init(BgEndsAcc& a) {
  a.ended = a.game = a.invalid = a.max_steps = a.no_summary = 0u;
  a.ante_sum = a.chips_sum = 0ull;
  a.ante_max = a.chips_max = 0u;
}
// Counts an ENDED record.  Returns its histogram bin (min(ante, 15)), or -1 for a record without a summary: such a record counts in words 0..3 and
// 9 only and is not fed to the curriculum.
BG_ENDS_FN int32_t bg_ends_count(BgEndsAcc& a, const BgEndRec& r) {
  a.ended += 1u;
  a.game += (r.flags & BG_END_GAME) ? 1u : 0u;
  a.invalid += (r.flags & BG_END_INVALID) ? 1u : 0u;
  a.max_steps += r.flags == BG_END_MAX_STEPS ? 1u : 0u;
  if (r.ante <= 0) { a.no_summary += 1u; return -1; }
  a.ante_sum += (uint64_t)r.ante;
  a.ante_max = (uint32_t)r.ante > a.ante_max ? (uint32_t)r.ante : a.ante_max;
  a.chips_sum += (uint64_t)r.chips;
  a.chips_max = r.chips > a.chips_max ? r.chips : a.chips_max;
  return r.ante < BG_ENDS_HIST_TOP ? r.ante : BG_ENDS_HIST_TOP;
}

// ---- the curriculum: one finished episode of one env (CurriculumTracker.update's body for that env, sb3_adapter.py:260-279) ----
struct BgCurEnv {
  int32_t cap;        // current_max_ante
  int64_t count;      // episodes ever finished
  int32_t at_level;   // episodes since the last raise
  bool raised;        // a cap rose in this call
};
// hist: the env's column of hist_dev [window, N] (entry k at hist[k * stride]).  The division is float64 and always by `window`, also while fewer
// than `window` episodes are kept (the reference's `sum(...) / self.success_window`), and the compare is as written: the result is exact.
BG_ENDS_FN void bg_ends_curriculum(BgCurEnv& c, int16_t* hist, size_t stride, int32_t ante, int32_t window, int32_t increment, double threshold) {
  hist[(size_t)((uint64_t)c.count % (uint64_t)window) * stride] = (int16_t)ante;   // (unsigned: no count can aim in front of the column)
  c.count += 1;
  if (c.at_level < 0x7fffffff) c.at_level += 1;
  if (c.at_level >= window && c.cap > 0) {   // (cap 0 = no cap: there is nothing to raise)
    const int32_t kept = c.count < (int64_t)window ? (int32_t)c.count : window;
    int32_t reached = 0;
    for (int32_t k = 0; k < kept; k++) reached += (int32_t)hist[(size_t)k * stride] >= c.cap ? 1 : 0;
    if ((double)reached / (double)window >= threshold) {
      c.cap = c.cap + increment < BG_ENDS_CAP_MAX ? c.cap + increment : BG_ENDS_CAP_MAX;
      c.at_level = 0;
      c.raised = true;
    }
  }
}

#ifndef BG_ENDS_HOST
// ---- the kernel ----
#define BG_ENDS_BLOCK 64
#define BG_ENDS_ENVS BG_ENDS_BLOCK /* envs of a workgroup: the grid is ceil(N / BG_ENDS_ENVS) */
#define BG_ENDS_BATCH 16
typedef uint32_t bg_ends_u32x4 __attribute__((ext_vector_type(4)));

// CUR: the curriculum's state is read, advanced and written (cur.* are then all set).  `report` has been zeroed in front of the launch.  K >= 1.
template <bool CUR>
__global__ __launch_bounds__(BG_ENDS_BLOCK) void bg_episode_ends_kernel(const uint8_t* __restrict__ rows, uint64_t row_stride, int K, long long N,
                                                                       unsigned long long* __restrict__ report, bg_curriculum cur) {
  __shared__ unsigned long long s_rep[BG_ENDS_WORDS];
  if (threadIdx.x < BG_ENDS_WORDS) s_rep[threadIdx.x] = 0ull;
  __syncthreads();
  const long long e = (long long)blockIdx.x * BG_ENDS_BLOCK + threadIdx.x;
  if (e < N) {
    BgEndsAcc acc;
    bg_ends_acc_init(acc);
    BgCurEnv c;
    c.cap = 0; c.count = 0; c.at_level = 0; c.raised = false;
    if (CUR) { c.cap = cur.cap_dev[e]; c.count = cur.count_dev[e]; c.at_level = cur.at_level_dev[e]; }
    for (int t0 = 0; t0 < K; t0 += BG_ENDS_BATCH) {
      bg_ends_u32x4 tail[BG_ENDS_BATCH];
#pragma unroll
      for (int j = 0; j < BG_ENDS_BATCH; j++) {
        const int t = t0 + j;
        tail[j] = bg_ends_u32x4{0u, 0u, 0u, 0u};
        if (t < K) tail[j] = *(const bg_ends_u32x4*)(rows + ((size_t)t * (size_t)N + (size_t)e) * row_stride + BG_ENDS_TAIL);
      }
#pragma unroll
      for (int j = 0; j < BG_ENDS_BATCH; j++) {
        const BgEndRec r = bg_ends_record(tail[j].y, tail[j].z, tail[j].w);   // (a slot past K is all zeros: not ended)
        if (r.ended) {
          const int32_t bin = bg_ends_count(acc, r);
          if (bin >= 0) {
            atomicAdd(&s_rep[BG_ENDS_W_HIST + bin], 1ull);
            if (CUR) bg_ends_curriculum(c, cur.hist_dev + e, (size_t)N, r.ante, cur.window, cur.increment, cur.threshold);
          }
        }
      }
    }
    if (CUR) {
      cur.cap_dev[e] = c.cap; cur.count_dev[e] = c.count; cur.at_level_dev[e] = c.at_level;
      cur.raised_dev[e] = c.raised ? 1 : 0;
      if (c.raised) atomicAdd(&s_rep[BG_ENDS_W_RAISED], 1ull);
    }
    if (acc.ended) {
      atomicAdd(&s_rep[BG_ENDS_W_ENDED], (unsigned long long)acc.ended);
      atomicAdd(&s_rep[BG_ENDS_W_GAME], (unsigned long long)acc.game);
      atomicAdd(&s_rep[BG_ENDS_W_INVALID], (unsigned long long)acc.invalid);
      atomicAdd(&s_rep[BG_ENDS_W_MAX_STEPS], (unsigned long long)acc.max_steps);
      atomicAdd(&s_rep[BG_ENDS_W_NO_SUMMARY], (unsigned long long)acc.no_summary);
      atomicAdd(&s_rep[BG_ENDS_W_ANTE_SUM], (unsigned long long)acc.ante_sum);
      atomicAdd(&s_rep[BG_ENDS_W_CHIPS_SUM], (unsigned long long)acc.chips_sum);
      atomicMax(&s_rep[BG_ENDS_W_ANTE_MAX], (unsigned long long)acc.ante_max);
      atomicMax(&s_rep[BG_ENDS_W_CHIPS_MAX], (unsigned long long)acc.chips_max);
    }
  }
  __syncthreads();
  if (threadIdx.x < BG_ENDS_WORDS) {
    const unsigned long long v = s_rep[threadIdx.x];
    if (v) {
      if (threadIdx.x == BG_ENDS_W_ANTE_MAX || threadIdx.x == BG_ENDS_W_CHIPS_MAX) atomicMax(&report[threadIdx.x], v);
      else atomicAdd(&report[threadIdx.x], v);
    }
  }
}
#endif  // BG_ENDS_HOST
#endif
