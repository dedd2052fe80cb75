// bg_policy.h -- bg_policy_forward: the network between the first layer and the env in ONE launch, for collection and evaluation: every hidden
// layer (SB3's mlp_extractor and what the reference puts in front of it), action_net, the masked head of bg_head.h and value_net.
//
// A workgroup takes 32 consecutive rows of h (bfloat16 [m, in0]: what RowExtractor / RowLinear return) and keeps their activations in LDS from the
// first layer to the head: no hidden activation and no logits matrix is written.  The index arithmetic of the fragments is plain C++ (BG_LIN_FN of
// bg_linear.h); define BG_POLICY_HOST before including and g++ compiles it with a serial twin (bg_policy_host) that drives it through a scalar model of
// the instruction, as BG_ACTOR_HOST does for bg_actor.h.
//
// THE NET (BgPolicyNet of include/balatro_mi355x.h, in HOST memory: bg_pol_check reads it on every call and it travels to the kernel as a launch
// argument, so a table outside the envelope cannot reach the kernel and nothing is uploaded).
//   sections     trunk (0..4 layers), then pi (0..4) and vf (0..4), both reading the trunk's output; the action layer [60, latent_pi] behind pi; the
//                value layer [1, latent_vf] behind vf when has_value.  Layers stand in that order in layer[].
//   envelope     every width, in0 included, a multiple of 32 in [32, 512]; weights bfloat16, 16-byte aligned, pitch a multiple of 8 elements; biases
//                float32; activation none / relu / tanh per hidden layer, none on the two last layers; vf layers need the value layer.
// THE CONTRACT.
//   one layer    y[i][j] = act(float32(sum_k x[i][k] * w[j][k]) + b[j]): the products are exact, the sum is the float32 accumulation of
//                v_mfma_f32_32x32x16_bf16 over k in ascending 16-blocks, the bias ONE float32 addition behind it, then the activation in float32, then
//                nearest-even rounding to bfloat16 (bg_ppo_bf16: NaN -> 0x7fc0) for the next layer.  relu: bg_lin_relu (a NaN is kept).
//   tanh         bg_pol_tanh: t = 2 |y|;  e = expf(t);  r = 1 - 2 / (e + 1);  the sign of y put back.  Every operation a float32 one rounded on its own
//                (-ffp-contract=off; IEEE division).  tests/policy_ref.py derives its absolute error.
//   last layers  the action layer's 60 logits and the value stay float32 (sum, then the bias).  The value goes through the same tile routine with
//                units 1..31 of its tile read as zero weights.
//   head         GIVEN these logits (logits_out returns them), actions, log_prob and entropy are bit for bit bg_sample_actions' / bg_evaluate_actions':
//                bg_head_row on the logits tile in LDS, as bg_actor_head_kernel runs it.
//   taps         bfloat16 [m, sum of the hidden widths]: every hidden layer's output in table order.  taps and logits_out are written beside the
//                other outputs and change no bit of them.
//   rows         a row's outputs are a pure function of (its h row, the net, its mask row, seed, index0 + i, t): they do not depend on m.
// THE KERNEL.  512 lanes = 8 waves, one workgroup per 32 rows.  Three LDS images of 32 x 520 bfloat16 (1 040-byte lines: a lane's 16-byte fragment
// reads fall on 16 different 16-byte slots per lane group): h goes to image 0; a trunk layer reads one of images 0 / 1 and writes
// the other; the trunk's output stays where it is while a branch alternates between the two other images.  Per layer, wave w takes the tiles of 32
// units w, w + 8, ...: the A fragment of a k-step is ONE 16-byte LDS read, the B fragment 16 bytes of one unit's weights straight from L2 (eight
// k-steps in flight, the next eight requested before the current eight are multiplied), one instruction per k-step into the tile's accumulator.  One
// barrier per layer.  Behind pi -- before vf takes pi's two images -- waves 0 and 1 take the two tiles of the action layer into the float32 logits
// tile (pitch 61, bg_head.h's); behind vf wave 2 takes the value tile; wave 0 stages the masks and runs bg_head_row, lane = row.
#ifndef BG_POLICY_H
#define BG_POLICY_H
#ifdef BG_POLICY_HOST
#ifndef BG_ACTOR_HOST
#define BG_ACTOR_HOST
#endif
#endif
#include "bg_actor.h"

#define BG_POL_ROWS 32          /* rows of a workgroup: one accumulator tile */
#define BG_POL_WMIN 32
#define BG_POL_WMAX 512         /* widest layer, in0 included */
#define BG_POL_PITCH 520        /* bfloat16 elements of a line of an activation image: 65 sixteen-byte slots, an odd count */
#define BG_POL_IMAGES 3
#define BG_POL_SECTION_MAX 4    /* layers of a section */
#define BG_POL_LAYERS_MAX 14    /* BG_POLICY_MAX_LAYERS: 3 sections, the action layer, the value layer */
#define BG_POL_NONE 0           /* BG_POLICY_ACT_* */
#define BG_POL_RELU 1
#define BG_POL_TANH 2
#define BG_POL_LPITCH (BG_HEAD_ACTIONS + 1) /* float32 elements of a line of the logits tile: BG_HEAD_LPITCH */
#ifndef BG_POL_BATCH
#define BG_POL_BATCH 8          /* k-steps whose weight fragments are in flight together (development builds: -DBG_POL_BATCH=, -DBG_POL_BLOCK=) */
#endif
static_assert(BG_POL_ROWS == BG_LIN_TILE && BG_POL_PITCH % 8 == 0 && BG_POL_PITCH >= BG_POL_WMAX && (BG_POL_PITCH / 8) % 2 == 1, "16-byte fragments on an odd slot pitch");
static_assert(BG_POL_WMAX % BG_LIN_TILE == 0 && BG_POL_WMIN % (2 * BG_LIN_KSTEP) == 0, "whole tiles, whole k-steps");

// The table as the kernel and the twin read it: BgPolicyLayer / BgPolicyNet of include/balatro_mi355x.h, field for field.
struct BgPolLayer {
  const uint16_t* w; const float* b;
  uint32_t wpitch; uint16_t in, out;
  uint32_t act, reserved;
};
struct BgPolNet {
  uint32_t ntrunk, npi, nvf, has_value, in0, reserved[3];
  BgPolLayer layer[BG_POL_LAYERS_MAX];
};
static_assert(sizeof(BgPolLayer) == 32 && sizeof(BgPolNet) == 32 + 32 * BG_POL_LAYERS_MAX, "the header's layout");

// ---- the index functions: the kernel and the twin ----
// element offset in an activation image of the lane's A fragment of k-step `step`: 8 consecutive k of row (lane & 31)
BG_LIN_FN int bg_pol_a_off(int lane, int step) { return bg_lin_frag_off(lane, step, BG_POL_PITCH); }
// the unit whose weights are the lane's B fragment in the tile that starts at unit0, and the fragment's first k
BG_LIN_FN int bg_pol_b_unit(int unit0, int lane) { return unit0 + bg_lin_frag_rc(lane); }
BG_LIN_FN int bg_pol_b_k(int lane, int step) { return bg_lin_frag_k(lane, step, 0); }
// the image a layer reads and the one it writes.  Images: h -> 0; trunk layer q: q & 1 -> (q & 1) ^ 1, so the trunk's output is image ntrunk & 1;
// a branch's layer q reads the trunk image (q == 0) or the branch's previous output, and writes the two other images in turn.
BG_LIN_FN int bg_pol_trunk_img(int ntrunk) { return ntrunk & 1; }
BG_LIN_FN int bg_pol_branch_out(int ntrunk, int q) { return (bg_pol_trunk_img(ntrunk) + 1 + (q & 1)) % BG_POL_IMAGES; }
BG_LIN_FN int bg_pol_branch_in(int ntrunk, int q) { return q == 0 ? bg_pol_trunk_img(ntrunk) : bg_pol_branch_out(ntrunk, q - 1); }
// the image a section's LAST output stands in (n == 0: the trunk's)
BG_LIN_FN int bg_pol_branch_last(int ntrunk, int n) { return bg_pol_branch_in(ntrunk, n); }
BG_LIN_FN int bg_pol_hidden(const BgPolNet& N) { return (int)(N.ntrunk + N.npi + N.nvf); }
// columns of the taps: the hidden widths in table order
BG_LIN_FN int bg_pol_tap_cols(const BgPolNet& N) {
  int s = 0;
  for (int q = 0; q < bg_pol_hidden(N); q++) s += N.layer[q].out;
  return s;
}
BG_LIN_FN bool bg_pol_width_ok(uint32_t w) { return w >= BG_POL_WMIN && w <= BG_POL_WMAX && w % 32 == 0; }

// tanh in float32 (THE CONTRACT).  t overflows to +inf beyond |y| > 1.7e38 and e beyond |y| > 44.4: 2 / inf = 0 and r = 1, tanh's value there.
BG_HEAD_FN float bg_pol_tanh(float y) {
  const float a = y < 0.f ? -y : y;
  const float t = 2.0f * a;
  const float e = expf(t);
  const float r = 1.0f - 2.0f / (e + 1.0f);
  return y != y ? y : y < 0.f ? -r : r;
}
BG_HEAD_FN float bg_pol_act(float v, uint32_t act) { return act == BG_POL_RELU ? bg_lin_relu(v) : act == BG_POL_TANH ? bg_pol_tanh(v) : v; }

// The envelope.  nullptr, or what is wrong with the table (host memory).
static inline const char* bg_pol_check(const BgPolNet* N) {
  if (!N) return "net must be a BgPolicyNet in host memory";
  if (N->ntrunk > BG_POL_SECTION_MAX || N->npi > BG_POL_SECTION_MAX || N->nvf > BG_POL_SECTION_MAX) return "a section holds at most 4 layers";
  if (N->has_value > 1u) return "has_value must be 0 or 1";
  if (N->nvf && !N->has_value) return "vf layers need the value layer";
  if (!bg_pol_width_ok(N->in0)) return "every width must be a multiple of 32 in [32, 512]";
  const int hidden = (int)(N->ntrunk + N->npi + N->nvf), total = hidden + 1 + (int)N->has_value;
  uint32_t trunk_out = N->in0, pi_out = 0, vf_out = 0;
  for (int q = 0; q < total; q++) {
    const BgPolLayer& L = N->layer[q];
    const bool last = q >= hidden;
    uint32_t want_in;
    if (q < (int)N->ntrunk) want_in = trunk_out;
    else if (q < (int)(N->ntrunk + N->npi)) want_in = q == (int)N->ntrunk ? trunk_out : pi_out;
    else if (q < hidden) want_in = q == (int)(N->ntrunk + N->npi) ? trunk_out : vf_out;
    else if (q == hidden) want_in = N->npi ? pi_out : trunk_out;
    else want_in = N->nvf ? vf_out : trunk_out;
    if (!bg_pol_width_ok(L.in) || (!last && !bg_pol_width_ok(L.out))) return "every width must be a multiple of 32 in [32, 512]";
    if (L.in != want_in) return "a layer's in_features must be the width of what it reads";
    if (q == hidden && L.out != BG_HEAD_ACTIONS) return "the action layer must have 60 units";
    if (q == hidden + 1 && L.out != 1) return "the value layer must have 1 unit";
    if (L.act > BG_POL_TANH) return "activation must be BG_POLICY_ACT_NONE, BG_POLICY_ACT_RELU or BG_POLICY_ACT_TANH";
    if (last && L.act != BG_POL_NONE) return "the action and value layers take no activation";
    if (!L.w || ((uintptr_t)L.w & 15)) return "a weight must be a 16-byte aligned device pointer to bfloat16";
    if (L.wpitch < L.in || (L.wpitch & 7)) return "a weight's pitch must be a multiple of 8 elements, >= in_features";
    if (!L.b || ((uintptr_t)L.b & 3)) return "a bias must be a 4-byte aligned device pointer to float32";
    if (q < (int)N->ntrunk) trunk_out = L.out;
    else if (q < (int)(N->ntrunk + N->npi)) pi_out = L.out;
    else if (q < hidden) vf_out = L.out;
  }
  return nullptr;
}

struct BgPolIo {
  const uint16_t* h; uint64_t hstride;                       // bfloat16 [m, in0]
  const int8_t* mask; int mld; uint64_t mstride;
  long long m; uint64_t seed, index0, t;
  const int32_t* actions_in; int32_t* actions_out;
  float* log_prob; float* entropy; float* values;            // nullable
  uint16_t* taps; uint64_t tstride;                          // nullable
  float* logits_out; uint64_t lostride; int lost;            // nullable; `lost`: its store path (BG_HEAD_LD_*)
};

#ifdef BG_POLICY_HOST
// ---- the serial twin ----
// One instruction of one tile: the A operand through the lane's fragment offsets in the image, the B operand through the lane's unit and k in the
// weight; units at or beyond `nunits` are zero weights.
static inline void bg_pol_host_mfma(const uint16_t* img, const BgPolLayer& L, int unit0, int nunits, int step, float acc[64][16]) {
  bg_lin_host_mfma([&](int l, int j) { return bg_head_widen_bf16(img[bg_pol_a_off(l, step) + j]); }, [&](int l, int j) {
    const int u = bg_pol_b_unit(unit0, l);
    return u < nunits ? bg_head_widen_bf16(L.w[(size_t)u * L.wpitch + bg_pol_b_k(l, step) + j]) : 0.f;
  }, acc);
}
static inline void bg_pol_host_tile(const uint16_t* img, const BgPolLayer& L, int unit0, int nunits, float acc[64][16]) {
  for (int l = 0; l < 64; l++)
    for (int g = 0; g < 16; g++) acc[l][g] = 0.f;
  for (int s = 0; s < L.in / BG_LIN_KSTEP; s++) bg_pol_host_mfma(img, L, unit0, nunits, s, acc);
}
// mode: BG_HEAD_SAMPLE / BG_HEAD_ARGMAX / BG_HEAD_EVALUATE.  The mask: int8 bytes, `mstride` apart (nullptr: none).  taps dense [m][tap cols], logits
// dense [m][60]; both nullable.
static inline void bg_policy_host(const BgPolNet& N, int mode, const uint16_t* h, uint64_t hstride, const int8_t* mask, uint64_t mstride, long long m, uint64_t seed,
                                  uint64_t index0, uint64_t t, int32_t* actions, float* log_prob, float* entropy, float* values, uint16_t* taps, float* logits) {
  static uint16_t img[BG_POL_IMAGES][BG_POL_ROWS * BG_POL_PITCH];
  static float lg[BG_POL_ROWS * BG_POL_LPITCH], pf[BG_POL_LPITCH];
  float acc[64][16];
  const int nt = (int)N.ntrunk, hidden = bg_pol_hidden(N), tcols = bg_pol_tap_cols(N);
  for (long long rec0 = 0; rec0 < m; rec0 += BG_POL_ROWS) {
    const int nrow = (int)(m - rec0 < BG_POL_ROWS ? m - rec0 : BG_POL_ROWS);
    for (int r = 0; r < BG_POL_ROWS; r++)
      for (int k = 0; k < (int)N.in0; k++) img[0][r * BG_POL_PITCH + k] = r < nrow ? h[(size_t)(rec0 + r) * hstride + k] : (uint16_t)0;
    int tap0 = 0;
    for (int q = 0; q <= hidden; q++) {
      if (q == nt + (int)N.npi) {   // the action layer, before vf takes pi's images
        const BgPolLayer& LA = N.layer[hidden];
        const uint16_t* const xa = img[bg_pol_branch_last(nt, (int)N.npi)];
        for (int u0 = 0; u0 < 2 * BG_LIN_TILE; u0 += BG_LIN_TILE) {
          bg_pol_host_tile(xa, LA, u0, BG_HEAD_ACTIONS, acc);
          for (int l = 0; l < 64; l++)
            for (int g = 0; g < 16; g++) {
              const int r = bg_lin_acc_row(l, g), j = u0 + bg_lin_acc_col(l);
              if (j < BG_HEAD_ACTIONS) lg[r * BG_POL_LPITCH + j] = acc[l][g] + LA.b[j];
            }
        }
      }
      if (q == hidden) break;
      const BgPolLayer& L = N.layer[q];
      int in, out;
      if (q < nt) { in = q & 1; out = in ^ 1; }
      else { const int b = q < nt + (int)N.npi ? q - nt : q - nt - (int)N.npi; in = bg_pol_branch_in(nt, b); out = bg_pol_branch_out(nt, b); }
      for (int u0 = 0; u0 < L.out; u0 += BG_LIN_TILE) {
        bg_pol_host_tile(img[in], L, u0, L.out, acc);
        for (int l = 0; l < 64; l++)
          for (int g = 0; g < 16; g++) {
            const int r = bg_lin_acc_row(l, g), j = u0 + bg_lin_acc_col(l);
            const uint16_t v = bg_ppo_bf16(bg_pol_act(acc[l][g] + L.b[j], L.act));
            img[out][r * BG_POL_PITCH + j] = v;
            if (taps && r < nrow) taps[(size_t)(rec0 + r) * tcols + tap0 + j] = v;
          }
      }
      tap0 += L.out;
    }
    if (N.has_value) {
      const BgPolLayer& LV = N.layer[hidden + 1];
      bg_pol_host_tile(img[bg_pol_branch_last(nt, (int)N.nvf)], LV, 0, 1, acc);
      for (int l = 0; l < 64; l++)
        for (int g = 0; g < 16; g++) {
          const int r = bg_lin_acc_row(l, g);
          if (bg_lin_acc_col(l) == 0 && r < nrow && values) values[rec0 + r] = acc[l][g] + LV.b[0];
        }
    }
    for (int r = 0; r < nrow; r++) {
      const long long i = rec0 + r;
      const float* const l = lg + r * BG_POL_LPITCH;
      if (logits)
        for (int j = 0; j < BG_HEAD_ACTIONS; j++) logits[(size_t)i * BG_HEAD_ACTIONS + j] = l[j];
      uint32_t kw[BG_HEAD_ACTIONS / 4] = {};
      if (mask) __builtin_memcpy(kw, mask + (size_t)i * mstride, BG_HEAD_ACTIONS);
      const BgHeadOut o = bg_head_row_host(mode, mask != nullptr, l, kw, pf, seed, index0 + (uint64_t)i, t, mode == BG_HEAD_EVALUATE ? actions[i] : 0);
      if (mode != BG_HEAD_EVALUATE) actions[i] = o.action;
      if (log_prob) log_prob[i] = o.log_prob;
      if (entropy) entropy[i] = o.entropy;
    }
  }
}
#else
// ---- the kernel ----
#ifndef BG_POL_BLOCK
#define BG_POL_BLOCK 512   /* 8 waves, two per SIMD: 256 lanes and a batch of 16 both measured slower */
#endif
#define BG_POL_WAVES (BG_POL_BLOCK / 64)
static_assert(BG_HEAD_BLOCK == 64 && BG_POL_LPITCH == BG_HEAD_LPITCH, "wave 0 runs the staging and store loops of bg_head.h / bg_ppo.h, which step by BG_HEAD_BLOCK");

// the lane's B fragments of k-steps s0 .. s0 + BG_POL_BATCH - 1 (those below `steps`), straight from L2.  wrow: the lane's unit's weights, or nullptr
// for a unit the tile pads (zero weights; uniform per lane over the whole tile).
__device__ __forceinline__ void bg_pol_ld_w(const uint16_t* __restrict__ wrow, int lane, int s0, int steps, bg_lin_u4 (&b)[BG_POL_BATCH]) {
#pragma unroll
  for (int q = 0; q < BG_POL_BATCH; q++) {
    const bg_lin_u4 z = {0u, 0u, 0u, 0u};
    b[q] = z;
    if (s0 + q < steps && wrow) b[q] = *reinterpret_cast<const bg_lin_u4*>(__builtin_assume_aligned(wrow + bg_pol_b_k(lane, s0 + q), 16));
  }
}

// One tile: 32 rows of the image x 32 units from unit0 on (units at or beyond nunits: zero weights) over all K = L.in, into a fresh accumulator.
__device__ __forceinline__ bg_lin_c16 bg_pol_tile(const uint16_t* img, const BgPolLayer& L, int unit0, int nunits, int lane) {
  const int unit = bg_pol_b_unit(unit0, lane);
  const uint16_t* const wrow = unit < nunits ? L.w + (size_t)unit * L.wpitch : nullptr;
  const int steps = (int)L.in / BG_LIN_KSTEP;
  bg_lin_c16 acc;
#pragma unroll
  for (int g = 0; g < 16; g++) acc[g] = 0.f;
  bg_lin_u4 cur[BG_POL_BATCH], nxt[BG_POL_BATCH];
  bg_pol_ld_w(wrow, lane, 0, steps, cur);
  for (int s0 = 0; s0 < steps; s0 += BG_POL_BATCH) {
    bg_pol_ld_w(wrow, lane, s0 + BG_POL_BATCH, steps, nxt);   // (beyond the end: zeros, no load)
#pragma unroll
    for (int q = 0; q < BG_POL_BATCH; q++) {
      if (s0 + q < steps) {   // (uniform)
        const bg_lin_ab a = bg_lin_ld_frag(img + bg_pol_a_off(lane, s0 + q));
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bg_lin_ab, cur[q]), acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int q = 0; q < BG_POL_BATCH; q++) cur[q] = nxt[q];
  }
  return acc;
}

// One hidden layer: image `in` -> image `out` (and the taps' columns tap0 ..).  The caller places a barrier behind it.
__device__ __forceinline__ void bg_pol_layer(const BgPolLayer& L, const uint16_t* in, uint16_t* out, const BgPolIo& O, long long rec0, int nrow, int tap0) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int u0 = wave * BG_LIN_TILE; u0 < (int)L.out; u0 += BG_POL_WAVES * BG_LIN_TILE) {
    const bg_lin_c16 acc = bg_pol_tile(in, L, u0, (int)L.out, lane);
    const int j = u0 + bg_lin_acc_col(lane);
    const float bv = L.b[j];
#pragma unroll
    for (int g = 0; g < 16; g++) {
      const int r = bg_lin_acc_row(lane, g);
      const uint16_t v = bg_ppo_bf16(bg_pol_act(acc[g] + bv, L.act));
      out[r * BG_POL_PITCH + j] = v;
      if (O.taps && r < nrow) O.taps[(size_t)(rec0 + r) * O.tstride + (size_t)(tap0 + j)] = v;
    }
  }
}

// MODE as bg_head_kernel's.  m >= 1.  N passed bg_pol_check.
template <int MODE>
__global__ __launch_bounds__(BG_POL_BLOCK) void bg_policy_kernel(const BgPolNet N, const BgPolIo O) {
  __shared__ __attribute__((aligned(16))) uint16_t img[BG_POL_IMAGES][BG_POL_ROWS * BG_POL_PITCH];
  BG_HEAD_LDS(MODE, BG_POL_ROWS);   // lg, pf, mk
  const long long rec0 = (long long)blockIdx.x * BG_POL_ROWS;
  const int nrow = (int)(O.m - rec0 < BG_POL_ROWS ? O.m - rec0 : BG_POL_ROWS);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // h -> image 0 by 16-byte pieces; rows at or beyond nrow are +0.0
  const int pieces = (int)N.in0 / 8;
  for (int u = threadIdx.x; u < BG_POL_ROWS * pieces; u += BG_POL_BLOCK) {
    const int r = u / pieces, p = (u - r * pieces) * 8;
    bg_lin_u4 v = {0u, 0u, 0u, 0u};
    if (r < nrow) v = *reinterpret_cast<const bg_lin_u4*>(__builtin_assume_aligned(O.h + (size_t)(rec0 + r) * O.hstride + (size_t)p, 16));
    *reinterpret_cast<bg_lin_u4*>(&img[0][r * BG_POL_PITCH + p]) = v;
  }
  if (wave == 0 && O.mld != BG_HEAD_LD_NONE) bg_head_stage_mask(O.mask, O.mld, O.mstride, rec0, nrow, mk);
  __syncthreads();
  const int nt = (int)N.ntrunk, npi = (int)N.npi, nvf = (int)N.nvf, hidden = nt + npi + nvf;
  int tap0 = 0;
  auto section = [&](int q0, int q1) {   // (uniform) layers q0 .. q1 - 1, a barrier behind each
    for (int q = q0; q < q1; q++) {
      const BgPolLayer& L = N.layer[q];
      int in, out;
      if (q < nt) { in = q & 1; out = in ^ 1; }
      else { const int b = q < nt + npi ? q - nt : q - nt - npi; in = bg_pol_branch_in(nt, b); out = bg_pol_branch_out(nt, b); }
      bg_pol_layer(L, img[in], img[out], O, rec0, nrow, tap0);
      tap0 += (int)L.out;
      __syncthreads();
    }
  };
  section(0, nt + npi);
  if (wave < 2) {   // the action layer, before vf takes pi's images: units 32 wave .. 32 wave + 31 of the 60, padded to 64
    const BgPolLayer& L = N.layer[hidden];
    const bg_lin_c16 acc = bg_pol_tile(img[bg_pol_branch_last(nt, npi)], L, wave * BG_LIN_TILE, BG_HEAD_ACTIONS, lane);
    const int j = wave * BG_LIN_TILE + bg_lin_acc_col(lane);
    if (j < BG_HEAD_ACTIONS) {
      const float bv = L.b[j];
#pragma unroll
      for (int g = 0; g < 16; g++) lg[bg_lin_acc_row(lane, g) * BG_HEAD_LPITCH + j] = acc[g] + bv;
    }
  }
  if (nvf) {   // (uniform)
    __syncthreads();
    section(nt + npi, hidden);
  }
  if (wave == 2 && N.has_value) {   // the value layer: unit 0 of one tile
    const BgPolLayer& L = N.layer[hidden + 1];
    const bg_lin_c16 acc = bg_pol_tile(img[bg_pol_branch_last(nt, nvf)], L, 0, 1, lane);
    if (bg_lin_acc_col(lane) == 0 && O.values) {
      const float bv = L.b[0];
#pragma unroll
      for (int g = 0; g < 16; g++) {
        const int r = bg_lin_acc_row(lane, g);
        if (r < nrow) O.values[rec0 + r] = acc[g] + bv;
      }
    }
  }
  __syncthreads();
  if (wave != 0) return;
  if (O.logits_out) bg_ppo_store_rows<false>(O.logits_out, O.lost, O.lostride, rec0, nrow, lg);
  const int r = threadIdx.x;
  if (r >= nrow) return;
  const long long i = rec0 + r;
  const float* const l = lg + r * BG_HEAD_LPITCH;
  float* const P = pf + (MODE == BG_HEAD_SAMPLE ? r * BG_HEAD_LPITCH : 0);
  const uint32_t* const k = mk + r * BG_HEAD_MWORDS;
  const float u = MODE == BG_HEAD_SAMPLE ? bg_head_u(bg_head_hash(O.seed, O.index0 + (uint64_t)i, O.t)) : 0.0f;
  const int32_t given = MODE == BG_HEAD_EVALUATE ? O.actions_in[i] : 0;
  const BgHeadOut o = O.mld != BG_HEAD_LD_NONE ? bg_head_row<MODE, true>(l, k, P, u, given) : bg_head_row<MODE, false>(l, k, P, u, given);
  if (MODE != BG_HEAD_EVALUATE) O.actions_out[i] = o.action;
  if (O.log_prob) O.log_prob[i] = o.log_prob;
  if (O.entropy) O.entropy[i] = o.entropy;
}
#endif  // BG_POLICY_HOST
#endif
