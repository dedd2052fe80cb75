// gae_variants.hip -- the A/B partners of bg_gae_kernel / bg_episode_stats_kernel (csrc/bg_gae.h), with the library's per-step text (bg_gae.h), so
// bit-identical results; tools/gae_rows.py asserts that and times them beside the library's calls (profiles/gae_rows.txt).  Not part of the product:
//     hipcc -O3 --offload-arch=gfx950 -std=c++17 -ffp-contract=off -fPIC -shared -Iinclude -Ibalatro_gym_amd/csrc -o tools/micro/libgae_variants.so tools/micro/gae_variants.hip
// The partner shape, LDS tiles: a workgroup of 256 lanes (4 waves) owns 64 consecutive envs and walks K in tiles of 16 steps (backwards for GAE, forwards
// for the episode scan).  ALL waves load a tile -- wave w the steps w, w + 4, w + 8, w + 12, lane = env: 12 (8) loads in flight per lane -- and put it into
// LDS in the form the chain reads (float32 reward / next_non_terminal / value; float64 reward + flag byte).  The loads of tile k + 1 are issued before wave
// 0 runs the chain over tile k out of LDS and are stored into the other LDS buffer after it: one barrier per tile (the buffer a chain read is next written
// behind that barrier).  Wave 0 writes the output rows.  37-39 / 28-32 VGPRs, 24 576 / 18 432 bytes of LDS, no scratch.  It lost to the library's
// lane = env kernels in every shape measured.
#include <hip/hip_runtime.h>
#include "balatro_mi355x.h"
#include "bg_gae.h"

#define GT_BLOCK 256
#define GT_ENVS 64
#define GT_WAVES (GT_BLOCK / GT_ENVS)
#define GT_TT 16
#define GT_PER (GT_TT / GT_WAVES) /* steps of a tile one lane loads */
static_assert(GT_ENVS == 64 && GT_TT % GT_WAVES == 0, "lane = env in a wave of 64; a tile splits evenly over the waves");

// RET: returns_dev is written.  Tile k, slot j is step t = K - 1 - (k * TT + j): slot 0 is the LATEST step, the chain walks the slots upwards.
template <bool RET>
__global__ __launch_bounds__(GT_BLOCK) void gae_tiles_kernel(const uint8_t* __restrict__ rows, uint64_t row_stride, int K, long long N,
                                                              const float* __restrict__ values, const float* __restrict__ last_values, float g, float gl,
                                                              float* __restrict__ advantages, float* __restrict__ returns) {
  __shared__ float s_r[2][GT_TT][GT_ENVS], s_nnt[2][GT_TT][GT_ENVS], s_v[2][GT_TT][GT_ENVS];
  const int lane = threadIdx.x % GT_ENVS, w = threadIdx.x / GT_ENVS;
  const long long e = (long long)blockIdx.x * GT_ENVS + lane;
  const bool live = e < N;
  const int ntiles = (K + GT_TT - 1) / GT_TT;
  double r64[GT_PER];
  uint8_t dn[GT_PER];
  float v[GT_PER];
  float last = 0.0f, nv = 0.0f;
  if (w == 0 && live) nv = last_values[e];
  // iteration k: issue the loads of tile k + 1, run the chain over tile k (none at k = -1), then store tile k + 1 into the other buffer
  for (int k = -1; k < ntiles; k++) {
    const bool more = k + 1 < ntiles;
    if (more) {
#pragma unroll
      for (int i = 0; i < GT_PER; i++) {
        const int t = K - 1 - ((k + 1) * GT_TT + w + i * GT_WAVES);
        r64[i] = 0.0; dn[i] = 0; v[i] = 0.f;
        if (live && t >= 0) {
          const size_t at = (size_t)t * (size_t)N + (size_t)e;
          const uint8_t* const rec = rows + at * row_stride;
          r64[i] = bg_gae_reward64(rec);
          dn[i] = rec[BG_ROW_TERMINATED];
          v[i] = values[at];
        }
      }
    }
    if (k >= 0 && w == 0 && live) {
      const int buf = k & 1, t0 = K - 1 - k * GT_TT;
#pragma unroll
      for (int j = 0; j < GT_TT; j++) {
        const int t = t0 - j;
        if (t >= 0) {
          const float vt = s_v[buf][j][lane];
          last = bg_gae_step(s_r[buf][j][lane], s_nnt[buf][j][lane], vt, nv, g, gl, last);
          nv = vt;
          const size_t at = (size_t)t * (size_t)N + (size_t)e;
          advantages[at] = last;
          if (RET) returns[at] = bg_gae_return(last, vt);
        }
      }
    }
    if (more) {
      const int buf = (k + 1) & 1;
#pragma unroll
      for (int i = 0; i < GT_PER; i++) {
        const int j = w + i * GT_WAVES;
        s_r[buf][j][lane] = bg_gae_reward32(r64[i]);
        s_nnt[buf][j][lane] = bg_gae_nnt(dn[i] != 0);
        s_v[buf][j][lane] = v[i];
      }
    }
    __syncthreads();
  }
}

// WR / WL: ep_return_dev / ep_len_dev are written.  Tile k, slot j is step t = k * TT + j.
template <bool WR, bool WL>
__global__ __launch_bounds__(GT_BLOCK) void eps_tiles_kernel(const uint8_t* __restrict__ rows, uint64_t row_stride, int K, long long N,
                                                                        double* __restrict__ carry_return, int32_t* __restrict__ carry_len,
                                                                        double* __restrict__ ep_return, int32_t* __restrict__ ep_len) {
  __shared__ double s_r[2][GT_TT][GT_ENVS];
  __shared__ uint8_t s_dn[2][GT_TT][GT_ENVS];
  const int lane = threadIdx.x % GT_ENVS, w = threadIdx.x / GT_ENVS;
  const long long e = (long long)blockIdx.x * GT_ENVS + lane;
  const bool live = e < N;
  const int ntiles = (K + GT_TT - 1) / GT_TT;
  double r64[GT_PER];
  uint8_t dn[GT_PER];
  double cr = 0.0;
  int32_t cl = 0;
  if (w == 0 && live) { cr = carry_return[e]; cl = carry_len[e]; }
  for (int k = -1; k < ntiles; k++) {
    const bool more = k + 1 < ntiles;
    if (more) {
#pragma unroll
      for (int i = 0; i < GT_PER; i++) {
        const int t = (k + 1) * GT_TT + w + i * GT_WAVES;
        r64[i] = 0.0; dn[i] = 0;
        if (live && t < K) {
          const uint8_t* const rec = rows + ((size_t)t * (size_t)N + (size_t)e) * row_stride;
          r64[i] = bg_gae_reward64(rec);
          dn[i] = rec[BG_ROW_TERMINATED];
        }
      }
    }
    if (k >= 0 && w == 0 && live) {
      const int buf = k & 1;
#pragma unroll
      for (int j = 0; j < GT_TT; j++) {
        const int t = k * GT_TT + j;
        if (t < K) {
          const BgEpsStep o = bg_eps_step(s_r[buf][j][lane], s_dn[buf][j][lane] != 0, cr, cl);
          cr = o.carry_return; cl = o.carry_len;
          const size_t at = (size_t)t * (size_t)N + (size_t)e;
          if (WR) ep_return[at] = o.ep_return;
          if (WL) ep_len[at] = o.ep_len;
        }
      }
    }
    if (more) {
      const int buf = (k + 1) & 1;
#pragma unroll
      for (int i = 0; i < GT_PER; i++) {
        const int j = w + i * GT_WAVES;
        s_r[buf][j][lane] = r64[i];
        s_dn[buf][j][lane] = dn[i];
      }
    }
    __syncthreads();
  }
  if (w == 0 && live) { carry_return[e] = cr; carry_len[e] = cl; }
}

extern "C" int gae_tiles(const uint8_t* rows, uint64_t row_stride, int K, long long N, const float* values, const float* last_values, double gamma,
                         double gae_lambda, float* advantages, float* returns, void* stream) {
  if (K <= 0 || N <= 0) return 0;
  hipLaunchKernelGGL(gae_tiles_kernel<true>, dim3((unsigned)((N + GT_ENVS - 1) / GT_ENVS)), dim3(GT_BLOCK), 0, (hipStream_t)stream, rows, row_stride, K, N, values,
                     last_values, bg_gae_g(gamma), bg_gae_gl(gamma, gae_lambda), advantages, returns);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int eps_tiles(const uint8_t* rows, uint64_t row_stride, int K, long long N, double* carry_return, int32_t* carry_len, double* ep_return,
                         int32_t* ep_len, void* stream) {
  if (K <= 0 || N <= 0) return 0;
  hipLaunchKernelGGL((eps_tiles_kernel<true, true>), dim3((unsigned)((N + GT_ENVS - 1) / GT_ENVS)), dim3(GT_BLOCK), 0, (hipStream_t)stream, rows, row_stride, K, N,
                     carry_return, carry_len, ep_return, ep_len);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
