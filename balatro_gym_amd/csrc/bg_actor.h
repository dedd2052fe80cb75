// bg_actor.h -- bg_actor_sample / bg_actor_evaluate / bg_actor_ppo_loss: the policy's last layer (SB3's action_net, nn.Linear(latent, 60)) fused with the
// masked head of bg_head.h and with the PPO loss of bg_ppo.h.
//
// The [m, 60] logits matrix never has to exist in HBM: a workgroup takes 64 consecutive rows of the last hidden activation h (bfloat16 [m, Hin]), a
// matrix-core product puts their 64 x 64 logits tile into LDS in the layout bg_head_kernel / bg_ppo_kernel stage theirs (float32, pitch 61), and the
// row functions of those kernels -- bg_head_row, bg_ppo_row -- run on it unchanged.  For training two more products consume the gradient tile before
// it leaves the CU.  The index arithmetic of the tiles and fragments is plain C++ (BG_LIN_FN of bg_linear.h); define BG_ACTOR_HOST before including
// and g++ compiles it with a serial twin (bg_actor_host) that drives it through a scalar model of the instruction.
//
// THE CONTRACT.
//   w_b          the weight [60, Hin] as bfloat16: a bfloat16 weight as it is, a float32 weight rounded on load (bg_ppo_bf16: nearest even, NaN -> 0x7fc0).
//   logits       logit[i][j] = float32(sum_k h[i][k] * w_b[j][k]) + bias[j]: the products are exact, the sum is the float32 accumulation of
//                v_mfma_f32_32x32x16_bf16 over k in ascending 16-blocks (the 60 units padded to 64 with zero weights), and the bias is ONE float32
//                addition behind it (no bias: no addition).  Padding units never reach the head.  Bounded by tests/actor_ref.py, not promised bit for
//                bit against another order of accumulation.
//   head / loss  GIVEN these logits (logits_out_dev returns them), actions, log_prob and entropy are bit for bit bg_sample_actions' /
//                bg_evaluate_actions', and every statistic, log_prob, entropy, dvalues and dlogits (dlogits_out_dev) bit for bit bg_ppo_loss': the
//                row functions, the 64-row partials, the advantage-statistics kernels and bg_ppo_finish are the same code in the same order.
//   dp           dp[i][j] = bfloat16(dlogits[i][j]) (bg_ppo_bf16), dlogits bg_ppo.h's float32 value; an excluded row is +0.0 throughout.
//   dh           dh[i][k] = float32(sum_j dp[i][j] * w_b[j][k]), the accumulation of the instruction over j in four 16-blocks; a bfloat16 dh is the
//                nearest-even rounding of that float32 value.
//   dweight      dweight[j][k] = sum_i dp[i][j] * h[i][k], dbias[j] = sum_i dp[i][j]: float32 inside a ROW GROUP (bg_act_blocks_per_group consecutive
//                blocks of 64 rows, one partial per group: the instruction's accumulation over i for dweight, a serial sum in row order for dbias), then
//                the groups' partials summed in float64 in index order and rounded once (bg_linear_rows_grad's scheme).  No floating-point atomics:
//                two calls give the same bits.
//   NON-FINITE   a NaN or infinity in h, w or bias is carried into the logits it touches, and the head's rules decide from there: a NaN or +inf at a
//                VALID unit makes the row degenerate (sample / evaluate: action -1, NaN) or excluded (loss: dlogits row +0.0), at a masked unit it
//                is ignored.  The products behind the loss are plain IEEE: dp = +0.0 times a non-finite w or h is NaN, so dh, dweight and dbias are
//                finite only where the operands they multiply are.
// THE KERNELS.
//   head         bg_actor_head_kernel: ONE wave per workgroup and 64 rows, as bg_head_kernel (four workgroups per CU: the row function's registers allow
//                one wave per SIMD).  The wave owns the four tiles of its 64 x 64 product and reads every fragment straight from HBM / L2 (16 bytes of
//                a row of h; 16 / 32 bytes of a unit's weights, or by element where the weight is not 16-byte aligned), no operand image and no barrier
//                in the k loop; then bg_head_stage_mask and bg_head_row as in bg_head_kernel.  LDS is bg_head_kernel's: it does not grow with Hin.
//   The loss: 256 lanes = 4 waves per workgroup; wave w owns tile (w & 1, w >> 1) of every 64 x 64 product.
//   logits       k runs in chunks of 64: the h chunk [64 rows][64 k] (16-byte pieces) and the weight chunk [64 units][64 k] (by element, converted) go to
//                two LDS images of pitch 72 bfloat16 (144-byte lines: 16-byte aligned fragments), four instructions per chunk and wave.  LDS does not
//                grow with Hin.  Rows at or beyond m, units 60..63 and k at or beyond Hin are zeros.
//   loss         grid (row groups, ceil(Hin / 256)): a workgroup owns a SPAN of 256 k of dh and dweight and walks the blocks of its group.  Per block:
//                the logits over ALL k (every span repeats them and the row function: the same bits), bg_ppo_row on wave 0, the 64-row sums by
//                bg_ppo_kernel's tree (span 0 writes them, and log_prob / entropy / dvalues / the optional tiles); dp goes to LDS twice, [i][j] and
//                [j][i]; per 64-k chunk of the span the transposed weight chunk [k][j] and the transposed h chunk [k][i] are staged, dh's tile is
//                four instructions over j and leaves from the accumulators (a half-wave writes 32 consecutive k of a row), dweight's tile is four
//                instructions over i into one of the wave's four accumulator tiles, which live across the blocks of the group.
//   reduce       bg_actor_reduce_kernel: one lane per element of dweight / dbias over the groups' partials.
#ifndef BG_ACTOR_H
#define BG_ACTOR_H
#ifdef BG_ACTOR_HOST
#ifndef BG_PPO_HOST
#define BG_PPO_HOST
#endif
#ifndef BG_LIN_HOST
#define BG_LIN_HOST
#endif
#endif
#include "bg_ppo.h"
#include "bg_linear.h"

#define BG_ACT_ROWS 64       /* rows of a block: BG_PPO_ROWS, so the 64-row partials are bg_ppo_loss' */
#define BG_ACT_UNITS 64      /* the 60 units padded to two accumulator tiles */
#define BG_ACT_KC 64         /* reduction length of a staged chunk */
#define BG_ACT_PITCH 72      /* bfloat16 elements of a line of every operand image */
#define BG_ACT_SPAN 256      /* k of dh / dweight one workgroup of the loss owns: four accumulator tiles per wave */
#define BG_ACT_MAX_WG 256    /* bound on the workgroups of the loss (row groups x spans): one per CU */
#define BG_ACT_HIN_MIN 32
#define BG_ACT_HIN_MAX 1024
#define BG_ACT_PART_TAIL 64  /* floats behind the [60][Hin] of a partial: dbias */
static_assert(BG_ACT_ROWS == BG_PPO_ROWS && BG_ACT_ROWS == 2 * BG_LIN_TILE && BG_ACT_UNITS == 2 * BG_LIN_TILE, "a 64 x 64 product is one tile per wave");
static_assert(BG_ACT_KC % BG_LIN_KSTEP == 0 && BG_ACT_PITCH % 8 == 0 && BG_ACT_PITCH >= BG_ACT_KC && BG_ACT_SPAN % BG_ACT_KC == 0, "fragments are 16-byte reads");

// wave w of a workgroup: the tile of the A operand's lines (= the output's rows) and of the B operand's lines (= the output's columns) it owns
BG_LIN_FN int bg_act_tile_a(int wave) { return wave & 1; }
BG_LIN_FN int bg_act_tile_b(int wave) { return wave >> 1; }
// element offset of a lane's fragment of k-step `step` in an operand image, `tile` = which 32 lines
BG_LIN_FN int bg_act_frag_off(int tile, int lane, int step) { return tile * BG_LIN_TILE * BG_ACT_PITCH + bg_lin_frag_off(lane, step, BG_ACT_PITCH); }
// the loss' split of m rows: blocks of 64, `per` consecutive blocks per row group, at most BG_ACT_MAX_WG / spans groups
BG_LIN_FN int64_t bg_act_blocks(int64_t m) { return (m + BG_ACT_ROWS - 1) / BG_ACT_ROWS; }
BG_LIN_FN int64_t bg_act_spans(int Hin) { return (Hin + BG_ACT_SPAN - 1) / BG_ACT_SPAN; }
BG_LIN_FN int64_t bg_act_blocks_per_group(int64_t m, int Hin) {
  const int64_t cap = BG_ACT_MAX_WG / bg_act_spans(Hin);
  return (bg_act_blocks(m) + cap - 1) / cap;
}
BG_LIN_FN int64_t bg_act_groups(int64_t m, int Hin) {
  const int64_t per = bg_act_blocks_per_group(m, Hin);
  return per > 0 ? (bg_act_blocks(m) + per - 1) / per : 0;   // (m <= 0: no group)
}
BG_LIN_FN bool bg_act_hin_ok(int Hin) { return Hin >= BG_ACT_HIN_MIN && Hin <= BG_ACT_HIN_MAX && Hin % 32 == 0; }
BG_LIN_FN uint64_t bg_act_part_floats(int Hin) { return (uint64_t)BG_HEAD_ACTIONS * (uint64_t)Hin + BG_ACT_PART_TAIL; }
// workspace: bg_ppo_loss' (head, statistics partials, row partials), rounded up to 16 bytes, then one partial per row group
BG_LIN_FN uint64_t bg_act_ppo_ws_bytes(int64_t m) { return (bg_ppo_ws_bytes(m) + 15u) & ~(uint64_t)15u; }
BG_LIN_FN uint64_t bg_act_workspace_bytes(int64_t m, int Hin) {
  if (m <= 0 || !bg_act_hin_ok(Hin)) return 0;
  return bg_act_ppo_ws_bytes(m) + (uint64_t)bg_act_groups(m, Hin) * bg_act_part_floats(Hin) * sizeof(float);
}

struct BgActorArgs {
  const uint16_t* h; uint64_t hstride;                    // bfloat16 [m, Hin]
  const void* weight; uint64_t wstride; int w_bf16;       // [60, Hin]
  const float* bias; int Hin;
  float* logits_out; uint64_t lostride; int lost;         // nullable; `lost`: its store path (BG_HEAD_LD_*)
};
struct BgActorGrad {
  void* dh; uint64_t dhstride; int dh_bf16;
  float* part;        // [groups][bg_act_part_floats]
  long long per;      // blocks per group
};

#ifdef BG_ACTOR_HOST
// ---- the serial twin ----
// One instruction (bg_lin_host_mfma): both operands are read from the images through the lane's fragment offsets.
static inline void bg_act_host_mfma(const uint16_t* a_img, int a_tile, const uint16_t* b_img, int b_tile, int step, float acc[64][16]) {
  bg_lin_host_mfma([&](int l, int j) { return bg_head_widen_bf16(a_img[bg_act_frag_off(a_tile, l, step) + j]); },
                   [&](int l, int j) { return bg_head_widen_bf16(b_img[bg_act_frag_off(b_tile, l, step) + j]); }, acc);
}
static inline uint16_t bg_act_host_w(const BgActorArgs& G, int j, int k) {
  if (j >= BG_HEAD_ACTIONS || k >= G.Hin) return 0;
  const size_t at = (size_t)j * G.wstride + k;
  return G.w_bf16 ? ((const uint16_t*)G.weight)[at] : bg_ppo_bf16(((const float*)G.weight)[at]);
}
static inline uint16_t bg_act_host_h(const BgActorArgs& G, long long i, long long m, int k) {
  return i < m && k < G.Hin ? G.h[(size_t)i * G.hstride + k] : (uint16_t)0;
}
// logits [m][60] (dense float32) of the twin: per block and wave the chunk loop of the kernel
static inline void bg_actor_host_logits(const BgActorArgs& G, long long m, float* logits) {
  static uint16_t sa[BG_ACT_ROWS * BG_ACT_PITCH], sb[BG_ACT_UNITS * BG_ACT_PITCH];
  for (long long rec0 = 0; rec0 < m; rec0 += BG_ACT_ROWS)
    for (int wave = 0; wave < 4; wave++) {
      float acc[64][16] = {};
      for (int k0 = 0; k0 < G.Hin; k0 += BG_ACT_KC) {
        for (int r = 0; r < BG_ACT_ROWS; r++)
          for (int k = 0; k < BG_ACT_KC; k++) { sa[r * BG_ACT_PITCH + k] = bg_act_host_h(G, rec0 + r, m, k0 + k); sb[r * BG_ACT_PITCH + k] = bg_act_host_w(G, r, k0 + k); }
        for (int s = 0; s < BG_ACT_KC / BG_LIN_KSTEP; s++)
          if (k0 + BG_LIN_KSTEP * s < G.Hin) bg_act_host_mfma(sa, bg_act_tile_a(wave), sb, bg_act_tile_b(wave), s, acc);
      }
      for (int l = 0; l < 64; l++)
        for (int g = 0; g < 16; g++) {
          const long long i = rec0 + bg_act_tile_a(wave) * BG_LIN_TILE + bg_lin_acc_row(l, g);
          const int j = bg_act_tile_b(wave) * BG_LIN_TILE + bg_lin_acc_col(l);
          if (i < m && j < BG_HEAD_ACTIONS) logits[(size_t)i * BG_HEAD_ACTIONS + j] = G.bias ? acc[l][g] + G.bias[j] : acc[l][g];
        }
    }
}
// The loss: A as bg_ppo_host takes it with A.logits / A.dlogits dense float32 [m][60] buffers the twin fills (the logits above, then bg_ppo_host itself:
// the statistics are its own).  dp uint16 [m][60], dh float32 [m][Hin] dense, dweight [60][Hin], dbias [60].
static inline void bg_actor_host(BgPpoArgs A, const BgActorArgs& G, float* stats, uint16_t* dp, float* dh, float* dweight, float* dbias) {
  const long long m = A.m;
  const int Hin = G.Hin;
  bg_actor_host_logits(G, m, (float*)A.logits);
  A.lstride = BG_HEAD_ACTIONS; A.dstride = BG_HEAD_ACTIONS;
  bg_ppo_host(A, false, false, stats);
  for (long long e = 0; e < m * BG_HEAD_ACTIONS; e++) dp[e] = bg_ppo_bf16(((const float*)A.dlogits)[e]);
  const long long per = bg_act_blocks_per_group(m, Hin), groups = bg_act_groups(m, Hin), nblk = bg_act_blocks(m);
  const uint64_t pf = bg_act_part_floats(Hin);
  float* part = new float[(size_t)groups * pf]();
  static uint16_t dpi[BG_ACT_ROWS * BG_ACT_PITCH], dpt[BG_ACT_UNITS * BG_ACT_PITCH], wt[BG_ACT_KC * BG_ACT_PITCH], ht[BG_ACT_KC * BG_ACT_PITCH];
  for (long long grp = 0; grp < groups; grp++) {
    float* mine = part + (size_t)grp * pf;
    for (int span = 0; span < (int)bg_act_spans(Hin); span++)
      for (int wave = 0; wave < 4; wave++) {
        const int ta = bg_act_tile_a(wave), tb = bg_act_tile_b(wave);
        float accw[BG_ACT_SPAN / BG_ACT_KC][64][16] = {};
        float dbsum[BG_ACT_UNITS] = {};
        for (long long b = grp * per; b < nblk && b < (grp + 1) * per; b++) {
          const long long rec0 = b * BG_ACT_ROWS;
          for (int i = 0; i < BG_ACT_ROWS; i++)
            for (int j = 0; j < BG_ACT_UNITS; j++) {
              const uint16_t v = rec0 + i < m && j < BG_HEAD_ACTIONS ? dp[(size_t)(rec0 + i) * BG_HEAD_ACTIONS + j] : (uint16_t)0;
              dpi[i * BG_ACT_PITCH + j] = v; dpt[j * BG_ACT_PITCH + i] = v;
            }
          if (span == 0 && wave == 3)
            for (int j = 0; j < BG_HEAD_ACTIONS; j++)
              for (int i = 0; i < BG_ACT_ROWS; i++) dbsum[j] = dbsum[j] + bg_head_widen_bf16(dpt[j * BG_ACT_PITCH + i]);
          for (int c = 0; c < BG_ACT_SPAN / BG_ACT_KC; c++) {
            const int k0 = span * BG_ACT_SPAN + c * BG_ACT_KC;
            if (k0 >= Hin) continue;
            for (int k = 0; k < BG_ACT_KC; k++)
              for (int q = 0; q < 64; q++) { wt[k * BG_ACT_PITCH + q] = bg_act_host_w(G, q, k0 + k); ht[k * BG_ACT_PITCH + q] = bg_act_host_h(G, rec0 + q, m, k0 + k); }
            float acc[64][16] = {};
            for (int s = 0; s < BG_ACT_UNITS / BG_LIN_KSTEP; s++) bg_act_host_mfma(dpi, ta, wt, tb, s, acc);
            for (int l = 0; l < 64; l++)
              for (int g = 0; g < 16; g++) {
                const long long i = rec0 + ta * BG_LIN_TILE + bg_lin_acc_row(l, g);
                const int k = k0 + tb * BG_LIN_TILE + bg_lin_acc_col(l);
                if (i < m && k < Hin) dh[(size_t)i * Hin + k] = acc[l][g];
              }
            for (int s = 0; s < BG_ACT_ROWS / BG_LIN_KSTEP; s++) bg_act_host_mfma(dpt, ta, ht, tb, s, accw[c]);
          }
        }
        for (int c = 0; c < BG_ACT_SPAN / BG_ACT_KC; c++) {
          const int k0 = span * BG_ACT_SPAN + c * BG_ACT_KC;
          for (int l = 0; l < 64; l++)
            for (int g = 0; g < 16; g++) {
              const int j = ta * BG_LIN_TILE + bg_lin_acc_row(l, g), k = k0 + tb * BG_LIN_TILE + bg_lin_acc_col(l);
              if (j < BG_HEAD_ACTIONS && k < Hin) mine[(size_t)j * Hin + k] = accw[c][l][g];
            }
        }
        if (span == 0 && wave == 3)
          for (int j = 0; j < BG_HEAD_ACTIONS; j++) mine[(size_t)BG_HEAD_ACTIONS * Hin + j] = dbsum[j];
      }
  }
  for (long long item = 0; item < (long long)BG_HEAD_ACTIONS * Hin + BG_HEAD_ACTIONS; item++) {
    double s = 0.0;
    for (long long p = 0; p < groups; p++) s = s + (double)part[(size_t)p * pf + item];
    if (item < (long long)BG_HEAD_ACTIONS * Hin) dweight[item] = (float)s;
    else dbias[item - (long long)BG_HEAD_ACTIONS * Hin] = (float)s;
  }
  delete[] part;
}
#else
// ---- the kernels ----
#define BG_ACT_BLOCK 256
static_assert(BG_HEAD_ROWS == BG_ACT_ROWS && BG_HEAD_BLOCK == 64, "wave 0 runs the staging and store loops of bg_head.h / bg_ppo.h, which step by BG_HEAD_BLOCK");

// the h chunk: rows rec0.., k0..k0+63.  TRANSPOSED false: img[row][k]; true: img[k][row].  Rows at or beyond nrow and k at or beyond Hin are zeros
// (Hin is a multiple of 32, so a 16-byte piece is inside or outside as a whole).
template <bool TRANSPOSED>
__device__ __forceinline__ void bg_act_stage_h(const uint16_t* __restrict__ h, uint64_t hstride, long long rec0, int nrow, int k0, int Hin, uint16_t* img) {
  constexpr int PER = BG_ACT_ROWS * (BG_ACT_KC / 8) / BG_ACT_BLOCK;   // 2 pieces per lane
  bg_lin_u4 v[PER];
#pragma unroll
  for (int q = 0; q < PER; q++) {
    const int u = threadIdx.x + q * BG_ACT_BLOCK, r = u >> 3, k = k0 + (u & 7) * 8;
    const bool ok = r < nrow && k < Hin;
    const bg_lin_u4 x = *reinterpret_cast<const bg_lin_u4*>(__builtin_assume_aligned(h + (ok ? (size_t)(rec0 + r) * hstride + (size_t)k : (size_t)rec0 * hstride), 16));
    const bg_lin_u4 z = {0u, 0u, 0u, 0u};
    v[q] = ok ? x : z;
  }
#pragma unroll
  for (int q = 0; q < PER; q++) {
    const int u = threadIdx.x + q * BG_ACT_BLOCK, r = u >> 3, p = (u & 7) * 8;
    if (TRANSPOSED) {
#pragma unroll
      for (int e = 0; e < 8; e++) img[(p + e) * BG_ACT_PITCH + r] = (uint16_t)(v[q][e >> 1] >> (16 * (e & 1)));
    } else *reinterpret_cast<bg_lin_u4*>(img + r * BG_ACT_PITCH + p) = v[q];
  }
}

// the weight chunk: units 0..63, k0..k0+63, as bfloat16.  TRANSPOSED false: img[unit][k]; true: img[k][unit].  Units 60..63 and k at or beyond Hin are zeros.
// Every load is unconditional (a refused element reads the matrix' first and is replaced), so a lane's 16 loads are in flight together.
template <bool TRANSPOSED>
__device__ __forceinline__ void bg_act_stage_w(const void* __restrict__ weight, int w_bf16, uint64_t wstride, int k0, int Hin, uint16_t* img) {
  constexpr int PER = BG_ACT_UNITS * BG_ACT_KC / BG_ACT_BLOCK;   // 16 elements per lane
  uint16_t v[PER];
#pragma unroll
  for (int q = 0; q < PER; q++) {
    const int e = threadIdx.x + q * BG_ACT_BLOCK, j = e >> 6, k = k0 + (e & 63);
    const bool ok = j < BG_HEAD_ACTIONS && k < Hin;
    const size_t at = ok ? (size_t)j * wstride + (size_t)k : 0;
    const uint16_t x = w_bf16 ? reinterpret_cast<const uint16_t*>(weight)[at] : bg_ppo_bf16(reinterpret_cast<const float*>(weight)[at]);
    v[q] = ok ? x : (uint16_t)0;
  }
#pragma unroll
  for (int q = 0; q < PER; q++) {
    const int e = threadIdx.x + q * BG_ACT_BLOCK, j = e >> 6, k = e & 63;
    img[TRANSPOSED ? k * BG_ACT_PITCH + j : j * BG_ACT_PITCH + k] = v[q];
  }
}

// four instructions (fewer where the reduction ends inside the chunk: `steps`, uniform) over two images
__device__ __forceinline__ bg_lin_c16 bg_act_mma(const uint16_t* a_img, int ta, const uint16_t* b_img, int tb, int lane, int steps, bg_lin_c16 acc) {
#pragma unroll
  for (int s = 0; s < BG_ACT_KC / BG_LIN_KSTEP; s++) {
    if (s < steps) {
      const bg_lin_ab a = bg_lin_ld_frag(a_img + bg_act_frag_off(ta, lane, s));
      const bg_lin_ab b = bg_lin_ld_frag(b_img + bg_act_frag_off(tb, lane, s));
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
  }
  return acc;
}

// the logits tile of the block's rows -> lg[row * BG_HEAD_LPITCH + unit], units 0..59.  Opens with a barrier (the images' and lg's previous readers are
// done); the caller places one behind it.
__device__ __forceinline__ void bg_act_logits(const BgActorArgs& G, long long rec0, int nrow, uint16_t* sa, uint16_t* sb, float* lg) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ta = bg_act_tile_a(wave), tb = bg_act_tile_b(wave);
  bg_lin_c16 acc;
#pragma unroll
  for (int g = 0; g < 16; g++) acc[g] = 0.f;
  for (int k0 = 0; k0 < G.Hin; k0 += BG_ACT_KC) {
    __syncthreads();
    bg_act_stage_h<false>(G.h, G.hstride, rec0, nrow, k0, G.Hin, sa);
    bg_act_stage_w<false>(G.weight, G.w_bf16, G.wstride, k0, G.Hin, sb);
    __syncthreads();
    acc = bg_act_mma(sa, ta, sb, tb, lane, (G.Hin - k0) / BG_LIN_KSTEP, acc);
  }
  const int col = tb * BG_LIN_TILE + bg_lin_acc_col(lane);
  if (col < BG_HEAD_ACTIONS) {
    const float bv = G.bias ? G.bias[col] : 0.f;
#pragma unroll
    for (int g = 0; g < 16; g++) lg[(ta * BG_LIN_TILE + bg_lin_acc_row(lane, g)) * BG_HEAD_LPITCH + col] = G.bias ? acc[g] + bv : acc[g];
  }
}

// ---- the head calls: ONE wave per workgroup, as bg_head_kernel, so that four workgroups share a CU and their row functions (249 registers in sample
// mode: one wave per SIMD) run side by side.  The wave owns all four tiles of its 64 x 64 product and reads its fragments straight from HBM / L2 -- a
// fragment is 16 consecutive bytes of one row of h or of one unit's weights -- so there is no operand image in LDS and no barrier in the k loop. ----
#define BG_ACT_W_VEC 1   /* weight fragments by 16-byte loads: the pointer and the row pitch in bytes are multiples of 16 */
// the lane's fragment of h: 8 consecutive k of row tile * 32 + (lane & 31) of the block; +0.0 for a row at or beyond nrow
__device__ __forceinline__ bg_lin_ab bg_act_ld_h(const uint16_t* __restrict__ h, uint64_t hstride, long long rec0, int nrow, int tile, int lane, int step) {
  const int r = tile * BG_LIN_TILE + bg_lin_frag_rc(lane);
  const bool ok = r < nrow;
  const bg_lin_u4 x = *reinterpret_cast<const bg_lin_u4*>(__builtin_assume_aligned(h + (size_t)(rec0 + (ok ? r : 0)) * hstride + (size_t)bg_lin_frag_k(lane, step, 0), 16));
  const bg_lin_u4 z = {0u, 0u, 0u, 0u};
  return __builtin_bit_cast(bg_lin_ab, ok ? x : z);
}
// the lane's fragment of w_b: 8 consecutive k of unit tile * 32 + (lane & 31); +0.0 for the padding units 60..63
__device__ __forceinline__ bg_lin_ab bg_act_ld_w(const void* __restrict__ weight, int w_bf16, int wvec, uint64_t wstride, int tile, int lane, int step) {
  const int j = tile * BG_LIN_TILE + bg_lin_frag_rc(lane);
  const bool ok = j < BG_HEAD_ACTIONS;
  const size_t at = (size_t)(ok ? j : 0) * wstride + (size_t)bg_lin_frag_k(lane, step, 0);
  bg_lin_u4 x;
  if (w_bf16) {
    const uint16_t* const p = reinterpret_cast<const uint16_t*>(weight) + at;
    if (wvec) x = *reinterpret_cast<const bg_lin_u4*>(__builtin_assume_aligned(p, 16));
    else {
#pragma unroll
      for (int q = 0; q < 4; q++) x[q] = (uint32_t)p[2 * q] | (uint32_t)p[2 * q + 1] << 16;
    }
  } else {
    const float* const p = reinterpret_cast<const float*>(weight) + at;
    float f[8];
    if (wvec) {
      const float4 lo = *reinterpret_cast<const float4*>(__builtin_assume_aligned(p, 16)), hi = *reinterpret_cast<const float4*>(__builtin_assume_aligned(p + 4, 16));
      f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w; f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
    } else {
#pragma unroll
      for (int q = 0; q < 8; q++) f[q] = p[q];
    }
#pragma unroll
    for (int q = 0; q < 4; q++) x[q] = (uint32_t)bg_ppo_bf16(f[2 * q]) | (uint32_t)bg_ppo_bf16(f[2 * q + 1]) << 16;
  }
  const bg_lin_u4 z = {0u, 0u, 0u, 0u};
  return __builtin_bit_cast(bg_lin_ab, ok ? x : z);
}

// MODE as bg_head_kernel's.  m >= 1.  64 lanes.
template <int MODE>
__global__ __launch_bounds__(BG_HEAD_BLOCK) void bg_actor_head_kernel(const BgActorArgs G, int wvec, const int8_t* __restrict__ mask, int mld, uint64_t mstride,
                                                                      long long m, uint64_t seed, uint64_t index0, uint64_t t,
                                                                      const int32_t* __restrict__ actions_in, int32_t* __restrict__ actions_out,
                                                                      float* __restrict__ log_prob, float* __restrict__ entropy) {
  BG_HEAD_LDS(MODE, BG_HEAD_ROWS);   // lg, pf, mk
  const long long rec0 = (long long)blockIdx.x * BG_ACT_ROWS;
  const int nrow = (int)(m - rec0 < BG_ACT_ROWS ? m - rec0 : BG_ACT_ROWS);
  const int lane = threadIdx.x;
  bg_lin_c16 acc[2][2];   // [row tile][unit tile]; every accumulator takes its k-steps in ascending order, as bg_act_logits' do
#pragma unroll
  for (int q = 0; q < 4; q++)
#pragma unroll
    for (int g = 0; g < 16; g++) acc[q >> 1][q & 1][g] = 0.f;
#pragma unroll 2
  for (int s = 0; s < G.Hin / BG_LIN_KSTEP; s++) {
    const bg_lin_ab a0 = bg_act_ld_h(G.h, G.hstride, rec0, nrow, 0, lane, s), a1 = bg_act_ld_h(G.h, G.hstride, rec0, nrow, 1, lane, s);
    const bg_lin_ab b0 = bg_act_ld_w(G.weight, G.w_bf16, wvec, G.wstride, 0, lane, s), b1 = bg_act_ld_w(G.weight, G.w_bf16, wvec, G.wstride, 1, lane, s);
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
  }
#pragma unroll
  for (int tb = 0; tb < 2; tb++) {
    const int col = tb * BG_LIN_TILE + bg_lin_acc_col(lane);
    if (col < BG_HEAD_ACTIONS) {
      const float bv = G.bias ? G.bias[col] : 0.f;
#pragma unroll
      for (int ta = 0; ta < 2; ta++)
#pragma unroll
        for (int g = 0; g < 16; g++) lg[(ta * BG_LIN_TILE + bg_lin_acc_row(lane, g)) * BG_HEAD_LPITCH + col] = G.bias ? acc[ta][tb][g] + bv : acc[ta][tb][g];
    }
  }
  if (mld != BG_HEAD_LD_NONE) bg_head_stage_mask(mask, mld, mstride, rec0, nrow, mk);
  __syncthreads();
  if (G.logits_out) bg_ppo_store_rows<false>(G.logits_out, G.lost, G.lostride, rec0, nrow, lg);
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

// grid (row groups, spans).  A as bg_ppo_kernel takes it: A.logits is not read, A.dlogits (float32, nullable here) is the optional dlogits_out.
// (A template, as bg_extractor.h's kernels are: instantiated behind every other kernel of the library; SUMS is BG_PPO_SUMS.)
template <int SUMS>
__global__ __launch_bounds__(BG_ACT_BLOCK) void bg_actor_ppo_kernel(const BgPpoArgs A, const BgActorArgs G, const BgActorGrad R) {
  __shared__ __attribute__((aligned(16))) uint16_t sa[BG_ACT_ROWS * BG_ACT_PITCH];    // h chunk [row][k], then [k][row]
  __shared__ __attribute__((aligned(16))) uint16_t sb[BG_ACT_UNITS * BG_ACT_PITCH];   // weight chunk [unit][k], then [k][unit]
  __shared__ __attribute__((aligned(16))) uint16_t dpi[BG_ACT_ROWS * BG_ACT_PITCH];   // dp [row][unit]
  __shared__ __attribute__((aligned(16))) uint16_t dpt[BG_ACT_UNITS * BG_ACT_PITCH];  // dp [unit][row]
  __shared__ float lg[BG_HEAD_ROWS * BG_HEAD_LPITCH];
  __shared__ uint32_t mk[BG_HEAD_ROWS * BG_HEAD_MWORDS];
  static_assert(SUMS == BG_PPO_SUMS, "the 64-row partials are bg_ppo_kernel's");
  __shared__ double red[BG_PPO_SUMS * BG_HEAD_ROWS];
  const int r = threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ta = bg_act_tile_a(wave), tb = bg_act_tile_b(wave);
  const bool first = blockIdx.y == 0;   // the span that writes what does not depend on the span
  const int kspan0 = blockIdx.y * BG_ACT_SPAN;
  constexpr int NC = BG_ACT_SPAN / BG_ACT_KC;
  bg_lin_c16 accw[NC];
#pragma unroll
  for (int c = 0; c < NC; c++)
#pragma unroll
    for (int g = 0; g < 16; g++) accw[c][g] = 0.f;
  float dbsum = 0.f;
  const long long nblk = bg_act_blocks(A.m);
  const long long b0 = (long long)blockIdx.x * R.per, b1 = b0 + R.per < nblk ? b0 + R.per : nblk;
  for (long long b = b0; b < b1; b++) {
    const long long rec0 = b * BG_ACT_ROWS;
    const int nrow = (int)(A.m - rec0 < BG_ACT_ROWS ? A.m - rec0 : BG_ACT_ROWS);
    bg_act_logits(G, rec0, nrow, sa, sb, lg);
    if (r < BG_HEAD_BLOCK && A.mld != BG_HEAD_LD_NONE) {
      if (A.index) bg_ppo_stage_mask_gather(A.mask, A.mld, A.mstride, A.index, A.store_rows, rec0, nrow, mk);
      else bg_head_stage_mask(A.mask, A.mld, A.mstride, rec0, nrow, mk);
    }
    __syncthreads();
    if (first && G.logits_out && r < BG_HEAD_BLOCK) bg_ppo_store_rows<false>(G.logits_out, G.lost, G.lostride, rec0, nrow, lg);   // wave 0, in front of its row function
    double t[BG_PPO_SUMS];
#pragma unroll
    for (int k = 0; k < BG_PPO_SUMS; k++) t[k] = 0.0;
    if (r < nrow) {   // bg_ppo_kernel's phase 2
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
      const uint32_t* const k = mk + r * BG_HEAD_MWORDS;
      const BgPpoTerms o = A.mld != BG_HEAD_LD_NONE ? bg_ppo_row<true, false>(l, k, nullptr, ok, a, old_lp, adv, advn, has_v, v, ret, A.c)
                                                    : bg_ppo_row<false, false>(l, k, nullptr, ok, a, old_lp, adv, advn, has_v, v, ret, A.c);
      if (!o.excluded) { t[0] = (double)o.policy; t[1] = (double)o.value; t[2] = (double)o.entropy; t[3] = (double)o.kl; t[4] = (double)o.clipped; }
      t[5] = (double)o.excluded;
      if (first) {
        if (A.dvalues) A.dvalues[i] = o.dvalue;
        if (A.log_prob) A.log_prob[i] = o.log_prob;
        if (A.entropy) A.entropy[i] = o.entropy;
      }
    }
    if (first) {   // (uniform over the workgroup) bg_ppo_kernel's tree: bg_loss_tile_reduce's text, spelled out (calling it moves this kernel: DESIGN.md)
      if (r < BG_HEAD_ROWS) {
#pragma unroll
        for (int k = 0; k < BG_PPO_SUMS; k++) red[k * BG_HEAD_ROWS + r] = t[k];
      }
      __syncthreads();
      for (int s = BG_HEAD_ROWS / 2; s; s >>= 1) {
        if (r < s) {
#pragma unroll
          for (int k = 0; k < BG_PPO_SUMS; k++) red[k * BG_HEAD_ROWS + r] = red[k * BG_HEAD_ROWS + r] + red[k * BG_HEAD_ROWS + r + s];
        }
        __syncthreads();
      }
      if (r < BG_PPO_SUMS) A.partials[(size_t)b * BG_PPO_SUMS + r] = red[r * BG_HEAD_ROWS];
      if (A.dlogits && r < BG_HEAD_BLOCK) bg_ppo_store_rows<false>(A.dlogits, A.dst, A.dstride, rec0, nrow, lg);
    } else __syncthreads();   // the gradient rows are in lg
    // dp, both ways round; rows at or beyond nrow and units 60..63 are +0.0
#pragma unroll
    for (int q = 0; q < BG_ACT_ROWS * BG_ACT_UNITS / BG_ACT_BLOCK; q++) {
      const int e = r + q * BG_ACT_BLOCK, i = e >> 6, j = e & 63;
      const uint16_t v = i < nrow && j < BG_HEAD_ACTIONS ? bg_ppo_bf16(lg[i * BG_HEAD_LPITCH + j]) : (uint16_t)0;
      dpi[i * BG_ACT_PITCH + j] = v;
      dpt[j * BG_ACT_PITCH + i] = v;
    }
    __syncthreads();
    if (first && wave == 3 && lane < BG_HEAD_ACTIONS) {   // dbias: unit `lane`, the block's rows in order
      for (int i = 0; i < BG_ACT_ROWS; i++) dbsum = dbsum + bg_lin_widen(dpt[lane * BG_ACT_PITCH + i]);
    }
#pragma unroll
    for (int c = 0; c < NC; c++) {
      const int k0 = kspan0 + c * BG_ACT_KC;
      if (k0 < G.Hin) {   // (uniform)
        if (c) __syncthreads();   // the previous chunk's fragments are read
        bg_act_stage_h<true>(G.h, G.hstride, rec0, nrow, k0, G.Hin, sa);
        bg_act_stage_w<true>(G.weight, G.w_bf16, G.wstride, k0, G.Hin, sb);
        __syncthreads();
        // dh[i][k] = sum_j dp[i][j] * w_b[j][k]: rows ta, k tile tb
        bg_lin_c16 acc;
#pragma unroll
        for (int g = 0; g < 16; g++) acc[g] = 0.f;
        acc = bg_act_mma(dpi, ta, sb, tb, lane, BG_ACT_UNITS / BG_LIN_KSTEP, acc);
        const int k = k0 + tb * BG_LIN_TILE + bg_lin_acc_col(lane);
        if (k < G.Hin) {
#pragma unroll
          for (int g = 0; g < 16; g++) {
            const int row = ta * BG_LIN_TILE + bg_lin_acc_row(lane, g);
            if (row < nrow) {
              const size_t at = (size_t)(rec0 + row) * R.dhstride + (size_t)k;
              if (R.dh_bf16) reinterpret_cast<uint16_t*>(R.dh)[at] = bg_ppo_bf16(acc[g]);
              else reinterpret_cast<float*>(R.dh)[at] = acc[g];
            }
          }
        }
        // dweight[j][k] += sum_i dp[i][j] * h[i][k]: units ta, k tile tb
        accw[c] = bg_act_mma(dpt, ta, sa, tb, lane, BG_ACT_ROWS / BG_LIN_KSTEP, accw[c]);
      }
    }
  }
  float* const mine = R.part + (size_t)blockIdx.x * bg_act_part_floats(G.Hin);
#pragma unroll
  for (int c = 0; c < NC; c++) {
    const int k = kspan0 + c * BG_ACT_KC + tb * BG_LIN_TILE + bg_lin_acc_col(lane);
    if (k < G.Hin) {
#pragma unroll
      for (int g = 0; g < 16; g++) {
        const int j = ta * BG_LIN_TILE + bg_lin_acc_row(lane, g);
        if (j < BG_HEAD_ACTIONS) mine[(size_t)j * G.Hin + k] = accw[c][g];
      }
    }
  }
  if (first && wave == 3 && lane < BG_HEAD_ACTIONS) mine[(size_t)BG_HEAD_ACTIONS * G.Hin + lane] = dbsum;
}

// dweight [60][Hin] and dbias [60] from the groups' partials: index order, float64, rounded once
template <int UNITS>
__global__ __launch_bounds__(256) void bg_actor_reduce_kernel(const float* __restrict__ part, long long groups, int Hin, float* __restrict__ dweight,
                                                              float* __restrict__ dbias) {
  const long long item = (long long)blockIdx.x * 256 + threadIdx.x, nw = (long long)UNITS * Hin;
  static_assert(UNITS == BG_HEAD_ACTIONS, "a partial is [60][Hin], then dbias");
  if (item >= nw + UNITS) return;
  const size_t pf = bg_act_part_floats(Hin);
  double s = 0.0;
  for (long long p = 0; p < groups; p++) s = s + (double)part[(size_t)p * pf + (size_t)item];
  if (item < nw) dweight[item] = (float)s;
  else dbias[item - nw] = (float)s;
}
#endif  // BG_ACTOR_HOST
#endif
