// bg_outcome.h -- bg_episode_outcome_rows: every step of a finished [K, N] rollout of packed records learns the outcome of its OWN episode.
//
// A record says how its episode ended only in the record of the ending step (BG_ROW_TERMINATED, BG_ROW_END_FLAGS, BG_ROW_END_ANTE).  Behaviour
// cloning's filter ("only use successful trajectories": the steps of episodes with final_ante >= 5, train_balatro_agent.py:220-262), the Monte-Carlo
// return of a step (value pre-training, self-imitation, reward-weighted regression) and the distance to the episode's end all need that knowledge at
// every step: one pass backwards along K, per env.  bg_episode_stats_rows / bg_episode_ends_rows run forwards and report per ended episode.
//
// THE CONTRACT.  Per env e, for t = K-1 down to 0; `next` is the state of step t + 1, or the tail (defaults -1, -1, 0, 0.0) at t = K-1:
//   the record's terminated byte is set:  steps = 0;  ante = the record's int16 BG_ROW_END_ANTE;  flags = its BG_ROW_END_FLAGS byte;  ret = r
//   elsewhere:                            steps = next.steps < 0 ? -1 : next.steps + 1;  ante = next.ante;  flags = next.flags;  ret = r + gamma * next.ret
// r is the record's float64 reward, or rewards[t][e].  ret is float64: the product rounds, then the sum rounds; nothing is fused (the library is built
// with -ffp-contract=off).  An episode that does not end inside the call and has no tail is OPEN: steps -1, ante -1, flags 0, ret the discounted sum so
// far.  The chain is SERIAL in t per env, as GAE's is, so every output is bit for bit the numpy loop (tests/outcome_ref.py).
// The per-step arithmetic is plain C++ behind BG_GAE_FN: define BG_OUTCOME_HOST before including and the text the GPU runs compiles with g++, with a
// serial twin of the launch (bg_outcome_host).
#ifndef BG_OUTCOME_H
#define BG_OUTCOME_H
#if defined(BG_OUTCOME_HOST) && !defined(BG_GAE_HOST)
#define BG_GAE_HOST
#endif
#include "bg_gae.h"

struct BgOutcome {
  int32_t steps, ante;
  uint32_t flags;
  double ret;
};

// bytes 340..347 of a record: boss_blind_active, boss_blind_type, BG_ROW_TERMINATED, BG_ROW_END_FLAGS, BG_ROW_END_ANTE (int16), end_round, 0 -- one
// 8-byte load (records are 16-byte aligned, so byte 340 is 4-byte aligned), in the 128-byte line GAE reads its terminated byte from
#define BG_OUTCOME_TAIL 340
static_assert(BG_ROW_TERMINATED == BG_OUTCOME_TAIL + 2 && BG_ROW_END_FLAGS == BG_OUTCOME_TAIL + 3 && BG_ROW_END_ANTE == BG_OUTCOME_TAIL + 4,
              "the terminated byte, the end flags and the end ante sit in bytes 340..347 of a record");
BG_GAE_FN uint64_t bg_outcome_tail64(const uint8_t* rec) {
  uint64_t w;
  __builtin_memcpy(&w, __builtin_assume_aligned(rec + BG_OUTCOME_TAIL, 4), 8);
  return w;
}
BG_GAE_FN bool bg_outcome_done(uint64_t w) { return ((w >> 16) & 0xffu) != 0u; }
BG_GAE_FN uint32_t bg_outcome_flags(uint64_t w) { return (uint32_t)((w >> 24) & 0xffu); }
BG_GAE_FN int32_t bg_outcome_ante(uint64_t w) { return (int32_t)(int16_t)(uint16_t)((w >> 32) & 0xffffu); }

// one step of the chain: w the record's bytes 340..347, r its reward, next the state of step t + 1
BG_GAE_FN BgOutcome bg_outcome_step(uint64_t w, double r, double gamma, BgOutcome next) {
  BgOutcome o;
  if (bg_outcome_done(w)) {
    o.steps = 0; o.ante = bg_outcome_ante(w); o.flags = bg_outcome_flags(w); o.ret = r;
  } else {
    o.steps = next.steps < 0 ? -1 : next.steps + 1;
    o.ante = next.ante; o.flags = next.flags;
    const double disc = gamma * next.ret;
    o.ret = r + disc;
  }
  return o;
}
// the state behind the last step of env e: the tails, or their defaults
BG_GAE_FN BgOutcome bg_outcome_start(const int32_t* tail_steps, const int32_t* tail_ante, const uint8_t* tail_flags, const double* tail_return, long long e) {
  BgOutcome o;
  o.steps = tail_steps ? tail_steps[e] : -1;
  o.ante = tail_ante ? tail_ante[e] : -1;
  o.flags = tail_flags ? (uint32_t)tail_flags[e] : 0u;
  o.ret = tail_return ? tail_return[e] : 0.0;
  return o;
}

#ifdef BG_OUTCOME_HOST
// ---- the serial twin: every pointer is a host pointer; outputs and tails may be NULL ----
static inline void bg_outcome_host(const uint8_t* rows, uint64_t row_stride, int K, long long N, double gamma, const double* rewards,
                                   const int32_t* tail_steps, const int32_t* tail_ante, const uint8_t* tail_flags, const double* tail_return,
                                   int32_t* steps, int32_t* ante, uint8_t* flags, double* returns) {
  for (long long e = 0; e < N; e++) {
    BgOutcome nx = bg_outcome_start(tail_steps, tail_ante, tail_flags, tail_return, e);
    for (int t = K - 1; t >= 0; t--) {
      const size_t at = (size_t)t * (size_t)N + (size_t)e;
      const uint8_t* const rec = rows + at * row_stride;
      nx = bg_outcome_step(bg_outcome_tail64(rec), rewards ? rewards[at] : bg_gae_reward64(rec), gamma, nx);
      if (steps) steps[at] = nx.steps;
      if (ante) ante[at] = nx.ante;
      if (flags) flags[at] = (uint8_t)nx.flags;
      if (returns) returns[at] = nx.ret;
    }
  }
}
#else
// ---- the kernel ----
// bg_gae_kernel's shape, for its reasons: no address depends on the chain, so lane = env, ONE wave per workgroup, no LDS, no barrier, and a lane
// walks K backwards in batches of BG_GAE_BATCH = 16 steps whose loads -- the 8 bytes at 340 and (RET) the reward, a second line -- are ALL issued
// into registers before the first is used.  A wave's stores of one step are 64 lanes x 4, 4, 1 and 8 consecutive bytes.
// RET: returns_dev is written; without it no reward is read and a record costs ONE line.  RW (only with RET): the reward is rewards[t][e].
// The int outputs are nullable at run time (a uniform branch per store).  Batch at t0, slot j is step t = t0 - j.  K >= 1.
template <bool RET, bool RW>
__global__ __launch_bounds__(BG_GAE_BLOCK) void bg_outcome_kernel(const uint8_t* __restrict__ rows, uint64_t row_stride, int K, long long N, double gamma,
                                                                  const double* __restrict__ rewards, const int32_t* __restrict__ tail_steps,
                                                                  const int32_t* __restrict__ tail_ante, const uint8_t* __restrict__ tail_flags,
                                                                  const double* __restrict__ tail_return, int32_t* __restrict__ steps,
                                                                  int32_t* __restrict__ ante, uint8_t* __restrict__ flags, double* __restrict__ returns) {
  const long long e = (long long)blockIdx.x * BG_GAE_BLOCK + threadIdx.x;
  if (e >= N) return;
  BgOutcome nx = bg_outcome_start(tail_steps, tail_ante, tail_flags, tail_return, e);
  for (int t0 = K - 1; t0 >= 0; t0 -= BG_GAE_BATCH) {
    uint64_t w[BG_GAE_BATCH];
    double r64[BG_GAE_BATCH];
#pragma unroll
    for (int j = 0; j < BG_GAE_BATCH; j++) {
      const int t = t0 - j;
      w[j] = 0; r64[j] = 0.0;
      if (t >= 0) {
        const size_t at = (size_t)t * (size_t)N + (size_t)e;
        const uint8_t* const rec = rows + at * row_stride;
        w[j] = bg_outcome_tail64(rec);
        if (RET) r64[j] = RW ? rewards[at] : bg_gae_reward64(rec);
      }
    }
#pragma unroll
    for (int j = 0; j < BG_GAE_BATCH; j++) {
      const int t = t0 - j;
      if (t >= 0) {
        nx = bg_outcome_step(w[j], r64[j], gamma, nx);
        const size_t at = (size_t)t * (size_t)N + (size_t)e;
        if (steps) steps[at] = nx.steps;
        if (ante) ante[at] = nx.ante;
        if (flags) flags[at] = (uint8_t)nx.flags;
        if (RET) returns[at] = nx.ret;
      }
    }
  }
}
#endif  // BG_OUTCOME_HOST
#endif
