// bg_gae.h -- bg_gae_rows / bg_episode_stats_rows: the two scans along K a PPO learner runs over a finished [K, N] rollout of packed records.
//
//   bg_gae_rows            SB3's RolloutBuffer.compute_returns_and_advantage on float32 buffers, backwards in t (include/balatro_mi355x.h has the text)
//   bg_episode_stats_rows  Monitor's per-episode reward sum and length, forwards in t, with a per-env carry across calls
//
// Both read two fields of a record -- BG_ROW_REWARD (float64) and BG_ROW_TERMINATED (one byte) -- and are SERIAL in t per env: a parallel scan
// would reorder the float additions and lose the bit-exactness that makes them testable.  The per-step arithmetic is plain C++ behind BG_GAE_FN, so
// the text the GPU runs compiles with g++ (define BG_GAE_HOST before including; the pattern of bg_encode.h / tests/test_encode_rows_host.py).
// The library is built with -ffp-contract=off (build.FLAGS): no multiply-add of the chain may be fused, every operation rounds to float32 on its own.
#ifndef BG_GAE_H
#define BG_GAE_H
#include <stdint.h>

#ifdef BG_GAE_HOST
#define BG_GAE_FN static inline
#else
#define BG_GAE_FN __host__ __device__ __forceinline__
#endif

// ---- the two fields of a record (records are 16-byte aligned, so the reward is 8-byte aligned) ----
BG_GAE_FN double bg_gae_reward64(const uint8_t* rec) {
  double r;
  __builtin_memcpy(&r, __builtin_assume_aligned(rec + BG_ROW_REWARD, 8), 8);
  return r;
}
BG_GAE_FN bool bg_gae_done(const uint8_t* rec) { return rec[BG_ROW_TERMINATED] != 0; }

// ---- GAE ----
// the float32 constants of a call: g = float32(gamma), gl = float32(gamma * gae_lambda) with the product taken in float64 first (numpy multiplies the
// Python floats before they meet the float32 array)
BG_GAE_FN float bg_gae_g(double gamma) { return (float)gamma; }
BG_GAE_FN float bg_gae_gl(double gamma, double gae_lambda) { return (float)(gamma * gae_lambda); }
// storing a float64 reward into SB3's float32 buffer: round to nearest even
BG_GAE_FN float bg_gae_reward32(double r) { return (float)r; }
// next_non_terminal = 1.0 - episode_starts[t + 1] = 1.0 - dones[t]
BG_GAE_FN float bg_gae_nnt(bool done) { return 1.0f - (done ? 1.0f : 0.0f); }
// one step of the chain: `last` is last_gae_lam of step t + 1 (0 behind the last step), `nv` values[t + 1] (last_values behind the last step).
//   delta        = rewards[t] + gamma * next_values * next_non_terminal - values[t]
//   last_gae_lam = delta + gamma * gae_lambda * next_non_terminal * last_gae_lam
// in numpy's order of evaluation, left to right, each operation rounded to float32.
BG_GAE_FN float bg_gae_step(float r, float nnt, float v, float nv, float g, float gl, float last) {
  const float delta = (r + (g * nv) * nnt) - v;
  return delta + ((gl * nnt) * last);
}
BG_GAE_FN float bg_gae_return(float adv, float v) { return adv + v; }

// ---- episode statistics ----
// one step of one env: a plain float64 sum in step order and a step count; a terminated step reports both and starts the next episode at 0.0 / 0
struct BgEpsStep {
  double carry_return, ep_return;
  int32_t carry_len, ep_len;
};
BG_GAE_FN BgEpsStep bg_eps_step(double r, bool done, double carry_return, int32_t carry_len) {
  const double sum = carry_return + r;
  const int32_t len = carry_len + 1;
  BgEpsStep o;
  o.ep_return = done ? sum : 0.0;
  o.ep_len = done ? len : 0;
  o.carry_return = done ? 0.0 : sum;
  o.carry_len = done ? 0 : len;
  return o;
}

#ifndef BG_GAE_HOST
// ---- the kernels ----
// No address depends on the chain, so the loading is what runs in parallel.  A record costs two scattered lines (the reward in bytes 128..255, the
// terminated byte in 256..383) for 9 useful bytes; a wave that loads a step, waits and computes would pay an HBM miss per step.  So: lane = env, ONE
// wave per workgroup (N = 4 096 is 64 workgroups on 64 CUs), no LDS, no barrier.  A lane walks K in batches of BG_GAE_BATCH = 16 steps (backwards for
// GAE, forwards for the episode scan) whose loads -- reward, terminated byte and (GAE) the value -- are ALL issued into registers before the first is
// used: 48 (32) loads in flight per lane.  A wave's stores of one step are 64 lanes x 4 or 8 consecutive bytes.
// This shape won the A/B (profiles/gae_rows.txt) against a 256-lane workgroup that stages tiles of 16 steps x 64 envs in double-buffered LDS for one
// chain wave; that one is kept as the partner in tools/micro/gae_variants.hip.
#define BG_GAE_BLOCK 64
#define BG_GAE_ENVS BG_GAE_BLOCK /* envs of a workgroup: the grid is ceil(N / BG_GAE_ENVS) */
#define BG_GAE_BATCH 16

// RET: returns_dev is written.  RW: the step's reward is rewards[t][e] (dense float64, bg_gae_rows_ex) instead of the record's.  Batch at t0, slot j
// is step t = t0 - j.  K >= 1.
template <bool RET, bool RW>
__global__ __launch_bounds__(BG_GAE_BLOCK) void bg_gae_kernel(const uint8_t* __restrict__ rows, uint64_t row_stride, int K, long long N,
                                                              const float* __restrict__ values, const float* __restrict__ last_values, float g, float gl,
                                                              float* __restrict__ advantages, float* __restrict__ returns, const double* __restrict__ rewards) {
  const long long e = (long long)blockIdx.x * BG_GAE_BLOCK + threadIdx.x;
  if (e >= N) return;
  float last = 0.0f, nv = last_values[e];
  for (int t0 = K - 1; t0 >= 0; t0 -= BG_GAE_BATCH) {
    double r64[BG_GAE_BATCH];
    uint8_t dn[BG_GAE_BATCH];
    float v[BG_GAE_BATCH];
#pragma unroll
    for (int j = 0; j < BG_GAE_BATCH; j++) {
      const int t = t0 - j;
      r64[j] = 0.0; dn[j] = 0; v[j] = 0.f;
      if (t >= 0) {
        const size_t at = (size_t)t * (size_t)N + (size_t)e;
        const uint8_t* const rec = rows + at * row_stride;
        r64[j] = RW ? rewards[at] : bg_gae_reward64(rec);
        dn[j] = rec[BG_ROW_TERMINATED];
        v[j] = values[at];
      }
    }
#pragma unroll
    for (int j = 0; j < BG_GAE_BATCH; j++) {
      const int t = t0 - j;
      if (t >= 0) {
        last = bg_gae_step(bg_gae_reward32(r64[j]), bg_gae_nnt(dn[j] != 0), v[j], nv, g, gl, last);
        nv = v[j];
        const size_t at = (size_t)t * (size_t)N + (size_t)e;
        advantages[at] = last;
        if (RET) returns[at] = bg_gae_return(last, v[j]);
      }
    }
  }
}

// WR / WL: ep_return_dev / ep_len_dev are written.  Batch at t0, slot j is step t = t0 + j.  K >= 1.
template <bool WR, bool WL>
__global__ __launch_bounds__(BG_GAE_BLOCK) void bg_episode_stats_kernel(const uint8_t* __restrict__ rows, uint64_t row_stride, int K, long long N,
                                                                        double* __restrict__ carry_return, int32_t* __restrict__ carry_len,
                                                                        double* __restrict__ ep_return, int32_t* __restrict__ ep_len) {
  const long long e = (long long)blockIdx.x * BG_GAE_BLOCK + threadIdx.x;
  if (e >= N) return;
  double cr = carry_return[e];
  int32_t cl = carry_len[e];
  for (int t0 = 0; t0 < K; t0 += BG_GAE_BATCH) {
    double r64[BG_GAE_BATCH];
    uint8_t dn[BG_GAE_BATCH];
#pragma unroll
    for (int j = 0; j < BG_GAE_BATCH; j++) {
      const int t = t0 + j;
      r64[j] = 0.0; dn[j] = 0;
      if (t < K) {
        const uint8_t* const rec = rows + ((size_t)t * (size_t)N + (size_t)e) * row_stride;
        r64[j] = bg_gae_reward64(rec);
        dn[j] = rec[BG_ROW_TERMINATED];
      }
    }
#pragma unroll
    for (int j = 0; j < BG_GAE_BATCH; j++) {
      const int t = t0 + j;
      if (t < K) {
        const BgEpsStep o = bg_eps_step(r64[j], dn[j] != 0, cr, cl);
        cr = o.carry_return; cl = o.carry_len;
        const size_t at = (size_t)t * (size_t)N + (size_t)e;
        if (WR) ep_return[at] = o.ep_return;
        if (WL) ep_len[at] = o.ep_len;
      }
    }
  }
  carry_return[e] = cr;
  carry_len[e] = cl;
}
#endif  // BG_GAE_HOST
#endif
