// bg_optim.h -- bg_optim_step: the learner's `clip_grad_norm_ ; optimizer.step() ; zero_grad()` over ALL parameter tensors in three launches, with the
// bfloat16 copies the first layers and the actor read and DQN's target network written in the same pass.
//
// Every training script of the reference passes max_grad_norm 0.5; PPO and DQN use Adam (SB3's policy: eps 1e-5), `--algorithm A2C` of
// train_balatro_agent.py uses SB3's RMSpropTFLike (a per-tensor Python loop; torch has no fused form of it), and DQN copies its target network every
// 1000 steps (tau 1.0).  The four "out of scope" lists of bg_ppo.h, bg_dqn.h, bg_bc.h and the first layers defer exactly these to "the optimiser".
// The element arithmetic is plain C++ behind BG_HEAD_FN: define BG_OPTIM_HOST before including and the text the GPU runs compiles with g++, with a
// serial twin of the launch sequence (bg_optim_host).  The library is built with -ffp-contract=off: nothing is fused.
//
// THE TABLE (device memory).  ntensors entries of 64 bytes (BgOptTensor): param, grad, state1, state2 (float32, contiguous, numel elements each),
// shadow (bfloat16, nullable) with cols and pitch (element i of the parameter is shadow[(i / cols) * pitch + i % cols], pitch >= cols), target
// (float32, nullable), numel.  Behind the entries: uint32 prefix[ntensors + 1], prefix[t] the number of chunks of the tensors before t.  A CHUNK is
// 1 024 consecutive elements of ONE tensor -- 256 lanes, 16 bytes per lane -- and never straddles tensors; tensor t has ceil(numel / 1024) of them.
// A workgroup is one chunk and finds its tensor by a binary search over the prefix with its workgroup index (wave-uniform: scalar loads).  A tensor
// whose four float32 pointers are all 16-byte aligned moves 16 bytes per lane; any other tensor, and the ragged last lane of a tensor, one element at
// a time, with the same arithmetic.  At most 1 024 tensors.  Loads and stores are plain: the forward pass reads the parameters next.
//
// THE CONTRACT.  Float32, every operation rounded on its own, except the norm (float64) and the carried bias corrections (float64).
//   norm       lane l of chunk k holds elements 1024 k + 4 l .. + 3 of its tensor and adds (double)g * (double)g of those that exist, ascending, from
//              zero; the 256 lane values go through bg_ppo.h's TREE; the chunk partials, in table order, through SLICES-THEN-TREE with 256 lanes: S.
//              norm = float32(sqrt(S)), the root in float64.  nonfinite = the number of gradient elements that are NaN or infinite (same path, exact).
//   clip       c = min(1, max_norm / (norm + 1e-6f)) in float32 (torch's clip_grad_norm_), or 1 with max_norm <= 0.
//   skip       norm not finite: skipped = 1, the carried state is not advanced, and p, the states, the shadows and the targets are not written.  The
//              gradients ARE zeroed under BG_OPTIM_ZERO_GRAD, so the next backward does not accumulate onto a NaN.
//   carry      32 bytes owned by the optimiser: int64 step, float64 b1pow, float64 b2pow (start: 0, 1, 1).  A step that is not skipped does step += 1
//              and, for Adam, b1pow *= beta1, b2pow *= beta2: the iterated product stands in for beta ** step (at most step * 2**-53 relative apart).
//              a = float32(lr / (1 - b1pow)), s2 = float32(sqrt(1 - b2pow)), division and root in float64.  RMSprop: a = float32(lr), s2 = 1.
//   element    g = g * c;  if weight_decay != 0: g = g + p * wd   (L2 as torch.optim.Adam, behind the clip)
//     Adam         m = m + (g - m) * float32(1 - beta1);  v = v * beta2 + ((1 - beta2) * g) * g;  p = p + (m / (sqrt(v) / s2 + eps)) * (-a)
//                  (torch's _single_tensor_adam: lerp, addcmul in its CPU kernel's order (value * t1) * t2, addcdiv in its GPU kernel's order
//                  value * (t1 / t2))
//     RMSpropTFLike  state1 = sq starts at ONES, state2 is unused (may be NULL):  sq = sq * alpha + ((1 - alpha) * g) * g;
//                  p = p + (g / sqrt(sq + eps)) * (-a).  The eps sits inside the root; not centred, no momentum, no bias correction.
//     shadow       bfloat16(p_new), round to nearest even (bg_ppo_bf16: a NaN becomes 0x7fc0)
//     target       with tau > 0: target = target * float32(1 - tau) + p_new * tau; at tau == 1 a plain copy of p_new
//     zero_grad    grad = +0.0
//   stats      32 bytes: float32 grad_norm, float32 clip_coef, int32 skipped, int32 0, int64 nonfinite, int64 step (after this call).
// No floating-point atomics and a fixed launch sequence (norm partials, combine, update): two calls on equal inputs give the same bits.
// BG_OPTIM_SHADOW_ONLY: one launch that writes every shadow from the current parameters and nothing else (RowOptimizer.refresh()).
// Out of scope: AdamW, amsgrad, momentum or centred RMSprop, parameter groups, sparse or non-float32 parameters, lr as a device scalar, multi-GPU
// gradient reduction.
#ifndef BG_OPTIM_H
#define BG_OPTIM_H
#if defined(BG_OPTIM_HOST) && !defined(BG_PPO_HOST)
#define BG_PPO_HOST
#endif
#include "bg_ppo.h"   // THE REDUCTION ORDER (TREE, SLICES-THEN-TREE), bg_ppo_bf16, bg_ppo_finite: one copy of each

#define BG_OPT_LANES BG_PPO_LANES   /* lanes of a chunk's workgroup and of the combining one */
#define BG_OPT_PER_LANE 4           /* float32 elements per lane: 16 bytes */
#define BG_OPT_CHUNK (BG_OPT_LANES * BG_OPT_PER_LANE)
#define BG_OPT_WS_HEAD 32           /* workspace: BgOptHead, then one BgOptPart per chunk */
static_assert(BG_OPT_CHUNK == BG_OPTIM_CHUNK, "include/balatro_mi355x.h states the chunk; its BG_OPTIM_* algorithms and flags are used as they are");

typedef float bg_opt_f4 __attribute__((vector_size(16)));      // 16 bytes of a lane, to hipcc and to g++ alike
typedef uint32_t bg_opt_u2 __attribute__((vector_size(8)));

struct BgOptTensor {
  float* param; float* grad; float* state1; float* state2;
  uint16_t* shadow; float* target;
  uint64_t numel;
  uint32_t cols, pitch;
};
static_assert(sizeof(BgOptTensor) == 64, "a table entry is 64 bytes (balatro_gym_amd/optim.py packs it)");
struct BgOptPart { double ss, nf; };                       // a partial: the sum of squares and the count of non-finite elements
struct BgOptCarry { long long step; double b1pow, b2pow, pad; };
struct BgOptHead { float c, a, s2; uint32_t skipped; uint32_t pad[4]; };
struct BgOptStats { float grad_norm, clip_coef; int32_t skipped, zero; long long nonfinite, step; };
static_assert(sizeof(BgOptCarry) == 32 && sizeof(BgOptHead) == BG_OPT_WS_HEAD && sizeof(BgOptStats) == 32 && sizeof(BgOptPart) == 16, "block sizes of the C ABI");
struct BgOptFold {
  BG_LOSS_FOLD BgOptPart operator()(int, BgOptPart a, BgOptPart b) const { BgOptPart o; o.ss = a.ss + b.ss; o.nf = a.nf + b.nf; return o; }
};
// what the call's scalar arguments become, once, on the host
struct BgOptHyper {
  double lr, beta1, beta2;     // the combine's float64 inputs (RMSprop: beta1 is alpha)
  float max_norm;              // <= 0: no clipping
  float omb1, b2, omb2, al, eps, wd, tau, omt;   // float32(1 - beta1), beta2, float32(1 - beta2), alpha = float32(beta1), eps, weight_decay, tau, float32(1 - tau)
  int algo;
  uint32_t flags;
};
BG_HEAD_FN BgOptHyper bg_optim_hyper(int algo, double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm, double tau, uint32_t flags) {
  BgOptHyper h;
  h.lr = lr; h.beta1 = beta1; h.beta2 = beta2; h.max_norm = (float)max_norm;
  h.omb1 = (float)(1.0 - beta1); h.b2 = (float)beta2; h.omb2 = (float)(1.0 - beta2); h.al = (float)beta1;
  h.eps = (float)eps; h.wd = (float)weight_decay; h.tau = (float)tau; h.omt = (float)(1.0 - tau);
  h.algo = algo; h.flags = flags;
  return h;
}
BG_HEAD_FN uint64_t bg_optim_chunks_of(uint64_t numel) { return (numel + BG_OPT_CHUNK - 1) / BG_OPT_CHUNK; }
BG_HEAD_FN uint64_t bg_optim_ws_bytes(long long chunks) { return chunks > 0 ? BG_OPT_WS_HEAD + (uint64_t)chunks * sizeof(BgOptPart) : 0; }

// ---- the element functions: the one spelling of the arithmetic ----
BG_HEAD_FN void bg_optim_norm_elem(float g, BgOptPart& acc) {
  acc.ss = acc.ss + (double)g * (double)g;
  acc.nf = acc.nf + (bg_ppo_finite(g) ? 0.0 : 1.0);
}
// g, p, s1 (m or sq), s2v (v): updated in place
template <int ALGO>
BG_HEAD_FN void bg_optim_elem(float g, float& p, float& s1, float& s2v, const BgOptHyper& h, float c, float a, float s2) {
  g = g * c;
  if (h.wd != 0.0f) g = g + p * h.wd;
  if (ALGO == BG_OPTIM_ADAM) {
    s1 = s1 + (g - s1) * h.omb1;
    s2v = s2v * h.b2 + (h.omb2 * g) * g;
    p = p + (s1 / (sqrtf(s2v) / s2 + h.eps)) * (-a);
  } else {
    s1 = s1 * h.al + (h.omb1 * g) * g;
    p = p + (g / sqrtf(s1 + h.eps)) * (-a);
  }
}
BG_HEAD_FN float bg_optim_polyak(float t, float p, const BgOptHyper& h) { return h.tau == 1.0f ? p : t * h.omt + p * h.tau; }
BG_HEAD_FN uint64_t bg_optim_shadow_at(uint64_t i, uint32_t cols, uint32_t pitch) { return cols == pitch ? i : (i / cols) * pitch + i % cols; }

// what lane 0 of the combining workgroup does with the sum: clip coefficient, skip verdict, carried state, the step's scalars, the stats block
BG_HEAD_FN void bg_optim_finish(BgOptPart sum, const BgOptHyper& h, BgOptCarry* carry, BgOptHead* head, BgOptStats* stats) {
  const float norm = (float)sqrt(sum.ss);
  const bool skip = !bg_ppo_finite(norm);
  float c = 1.0f;
  if (h.max_norm > 0.0f) c = fminf(1.0f, h.max_norm / (norm + 1e-6f));
  long long step = carry->step;
  double b1 = carry->b1pow, b2 = carry->b2pow;
  if (!skip) {
    step = step + 1;
    if (h.algo == BG_OPTIM_ADAM) { b1 = b1 * h.beta1; b2 = b2 * h.beta2; }
    carry->step = step; carry->b1pow = b1; carry->b2pow = b2;
  }
  head->c = c;
  head->a = h.algo == BG_OPTIM_ADAM ? (float)(h.lr / (1.0 - b1)) : (float)h.lr;
  head->s2 = h.algo == BG_OPTIM_ADAM ? (float)sqrt(1.0 - b2) : 1.0f;
  head->skipped = skip ? 1u : 0u;
  stats->grad_norm = norm; stats->clip_coef = c; stats->skipped = skip ? 1 : 0; stats->zero = 0;
  stats->nonfinite = (long long)sum.nf; stats->step = step;
}

// up to four consecutive floats of a lane: one 16-byte access (vec), or n single ones
BG_HEAD_FN void bg_opt_load(const float* src, uint64_t base, int n, bool vec, float* x) {
  if (vec) { const bg_opt_f4 q = *reinterpret_cast<const bg_opt_f4*>(src + base); x[0] = q[0]; x[1] = q[1]; x[2] = q[2]; x[3] = q[3]; }
  else for (int j = 0; j < n; j++) x[j] = src[base + j];
}
BG_HEAD_FN void bg_opt_store(float* dst, uint64_t base, int n, bool vec, const float* x) {
  if (vec) { bg_opt_f4 q; q[0] = x[0]; q[1] = x[1]; q[2] = x[2]; q[3] = x[3]; *reinterpret_cast<bg_opt_f4*>(dst + base) = q; }
  else for (int j = 0; j < n; j++) dst[base + j] = x[j];
}

// one lane's share of the update pass: n (1..4) elements from `base` on; vec: n == 4 and the tensor's four float32 pointers are 16-byte aligned
template <int ALGO, bool SHADOW_ONLY>
BG_HEAD_FN void bg_optim_lane(const BgOptTensor& T, uint64_t base, int n, bool vec, const BgOptHyper& h, const BgOptHead& hd) {
  const bool zero = (h.flags & BG_OPTIM_ZERO_GRAD) != 0u, has2 = ALGO == BG_OPTIM_ADAM;
  const float zeros[BG_OPT_PER_LANE] = {0.0f, 0.0f, 0.0f, 0.0f};
  float p[BG_OPT_PER_LANE] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (SHADOW_ONLY) {
    if (!T.shadow) return;
    bg_opt_load(T.param, base, n, vec, p);
  } else if (hd.skipped != 0u) {
    if (zero) bg_opt_store(T.grad, base, n, vec, zeros);
    return;
  } else {
    const bool has_t = T.target != nullptr && h.tau > 0.0f, vec_t = vec && ((uintptr_t)T.target & 15) == 0;
    float g[BG_OPT_PER_LANE] = {0.0f, 0.0f, 0.0f, 0.0f}, s1[BG_OPT_PER_LANE] = {0.0f, 0.0f, 0.0f, 0.0f}, s2v[BG_OPT_PER_LANE] = {0.0f, 0.0f, 0.0f, 0.0f};
    float tg[BG_OPT_PER_LANE] = {0.0f, 0.0f, 0.0f, 0.0f};
    bg_opt_load(T.grad, base, n, vec, g);
    bg_opt_load(T.param, base, n, vec, p);
    bg_opt_load(T.state1, base, n, vec, s1);
    if (has2) bg_opt_load(T.state2, base, n, vec, s2v);
    if (has_t && h.tau != 1.0f) bg_opt_load(T.target, base, n, vec_t, tg);
#pragma unroll
    for (int j = 0; j < BG_OPT_PER_LANE; j++) {
      if (j < n) {
        bg_optim_elem<ALGO>(g[j], p[j], s1[j], s2v[j], h, hd.c, hd.a, hd.s2);
        if (has_t) tg[j] = bg_optim_polyak(tg[j], p[j], h);
      }
    }
    bg_opt_store(T.param, base, n, vec, p);
    bg_opt_store(T.state1, base, n, vec, s1);
    if (has2) bg_opt_store(T.state2, base, n, vec, s2v);
    if (has_t) bg_opt_store(T.target, base, n, vec_t, tg);
    if (zero) bg_opt_store(T.grad, base, n, vec, zeros);
  }
  if (T.shadow) {
    if (n == BG_OPT_PER_LANE && T.cols == T.pitch && (((uintptr_t)T.shadow | (base * 2)) & 7) == 0) {   // four halves of one dense run: 8 bytes
      bg_opt_u2 w;
      w[0] = (uint32_t)bg_ppo_bf16(p[0]) | ((uint32_t)bg_ppo_bf16(p[1]) << 16);
      w[1] = (uint32_t)bg_ppo_bf16(p[2]) | ((uint32_t)bg_ppo_bf16(p[3]) << 16);
      *reinterpret_cast<bg_opt_u2*>(T.shadow + base) = w;
    } else {
      for (int j = 0; j < n; j++) T.shadow[bg_optim_shadow_at(base + j, T.cols, T.pitch)] = bg_ppo_bf16(p[j]);
    }
  }
}
BG_HEAD_FN bool bg_optim_vec(const BgOptTensor& T) {
  return ((((uintptr_t)T.param | (uintptr_t)T.grad | (uintptr_t)T.state1 | (uintptr_t)T.state2) & 15) == 0);
}
// the tensor of chunk `chunk`: the largest t with prefix[t] <= chunk (prefix[0] = 0, prefix[ntensors] = the chunks of the call)
BG_HEAD_FN int bg_optim_find(const uint32_t* prefix, int ntensors, uint32_t chunk) {
  int lo = 0, hi = ntensors;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= chunk) lo = mid; else hi = mid;
  }
  return lo;
}
BG_HEAD_FN int bg_optim_lane_count(uint64_t numel, uint64_t base) { return base >= numel ? 0 : (numel - base < BG_OPT_PER_LANE ? (int)(numel - base) : BG_OPT_PER_LANE); }

#ifdef BG_OPTIM_HOST
// ---- the serial twin: the launch sequence below, one "workgroup" after the other.  Every pointer is a host pointer; prefix stands behind the table. ----
static inline void bg_optim_host(const BgOptTensor* table, int ntensors, long long chunks, const BgOptHyper& h, BgOptCarry* carry, BgOptStats* stats) {
  const uint32_t* prefix = reinterpret_cast<const uint32_t*>(table + ntensors);
  BgOptHead head;
  memset(&head, 0, sizeof head);
  if (!(h.flags & BG_OPTIM_SHADOW_ONLY)) {
    BgOptPart* part = new BgOptPart[chunks ? chunks : 1];
    for (long long b = 0; b < chunks; b++) {
      const int t = bg_optim_find(prefix, ntensors, (uint32_t)b);
      const BgOptTensor& T = table[t];
      BgOptPart lane[BG_OPT_LANES];
      for (int l = 0; l < BG_OPT_LANES; l++) {
        const uint64_t base = ((uint64_t)b - prefix[t]) * BG_OPT_CHUNK + (uint64_t)l * BG_OPT_PER_LANE;
        const int n = bg_optim_lane_count(T.numel, base);
        lane[l].ss = 0.0; lane[l].nf = 0.0;
        for (int j = 0; j < n; j++) bg_optim_norm_elem(T.grad[base + j], lane[l]);
      }
      part[b] = bg_loss_host_tree(lane, BG_OPT_LANES, 0, BgOptFold{});
    }
    const BgOptPart zero = {0.0, 0.0};
    const BgOptPart sum = bg_loss_host_slices(part, (uint64_t)chunks, 1, 0, zero, BgOptFold{});
    delete[] part;
    bg_optim_finish(sum, h, carry, &head, stats);
  }
  for (long long b = 0; b < chunks; b++) {
    const int t = bg_optim_find(prefix, ntensors, (uint32_t)b);
    const BgOptTensor& T = table[t];
    for (int l = 0; l < BG_OPT_LANES; l++) {
      const uint64_t base = ((uint64_t)b - prefix[t]) * BG_OPT_CHUNK + (uint64_t)l * BG_OPT_PER_LANE;
      const int n = bg_optim_lane_count(T.numel, base);
      if (n == 0) continue;
      const bool vec = n == BG_OPT_PER_LANE && bg_optim_vec(T);
      if (h.flags & BG_OPTIM_SHADOW_ONLY) bg_optim_lane<BG_OPTIM_ADAM, true>(T, base, n, vec, h, head);
      else if (h.algo == BG_OPTIM_ADAM) bg_optim_lane<BG_OPTIM_ADAM, false>(T, base, n, vec, h, head);
      else bg_optim_lane<BG_OPTIM_RMSPROP_TF, false>(T, base, n, vec, h, head);
    }
  }
}
#else
// ---- the kernels ----  (all three are templates, as bg_extractor.h's are: read behind every other header, they leave the text of every other kernel as it was)
// 1  one workgroup per chunk: the chunk's float64 sum of squares and its count of non-finite gradient elements -> part[chunk]
template <int LANES>
__global__ __launch_bounds__(LANES) void bg_optim_norm_partials(const BgOptTensor* __restrict__ table, int ntensors, BgOptPart* __restrict__ part) {
  static_assert(LANES == BG_PPO_LANES, "bg_ppo.h's TREE runs over its 256 lanes");
  __shared__ BgOptPart t[LANES];
  const uint32_t* const prefix = reinterpret_cast<const uint32_t*>(table + ntensors);
  const int ti = bg_optim_find(prefix, ntensors, blockIdx.x);
  const BgOptTensor T = table[ti];
  const uint64_t base = ((uint64_t)blockIdx.x - prefix[ti]) * BG_OPT_CHUNK + (uint64_t)threadIdx.x * BG_OPT_PER_LANE;
  const int n = bg_optim_lane_count(T.numel, base);
  BgOptPart v;
  v.ss = 0.0; v.nf = 0.0;
  float g[BG_OPT_PER_LANE] = {0.0f, 0.0f, 0.0f, 0.0f};
  bg_opt_load(T.grad, base, n, n == BG_OPT_PER_LANE && ((uintptr_t)T.grad & 15) == 0, g);
  for (int j = 0; j < n; j++) bg_optim_norm_elem(g[j], v);
  bg_loss_stat_partials(v, t, part, BgOptFold{});
}

// 2  one workgroup: the chunk partials -> the step's scalars (workspace head), the carried state and the stats block
template <int LANES>
__global__ __launch_bounds__(LANES) void bg_optim_combine(const BgOptPart* __restrict__ part, long long P, const BgOptHyper h, BgOptCarry* __restrict__ carry,
                                                                 BgOptHead* __restrict__ head, BgOptStats* __restrict__ stats) {
  __shared__ BgOptPart t[LANES];
  BgOptPart v;
  v.ss = 0.0; v.nf = 0.0;
  bg_loss_stat_combine(part, P, v, t, BgOptFold{});
  if (threadIdx.x == 0) bg_optim_finish(t[0], h, carry, head, stats);
}

// 3  one workgroup per chunk: the update, the shadows, the targets, the zeroing
template <int ALGO, bool SHADOW_ONLY>
__global__ __launch_bounds__(BG_OPT_LANES) void bg_optim_update(const BgOptTensor* __restrict__ table, int ntensors, const BgOptHyper h, const BgOptHead* __restrict__ head) {
  const uint32_t* const prefix = reinterpret_cast<const uint32_t*>(table + ntensors);
  const int ti = bg_optim_find(prefix, ntensors, blockIdx.x);
  const BgOptTensor T = table[ti];
  const uint64_t base = ((uint64_t)blockIdx.x - prefix[ti]) * BG_OPT_CHUNK + (uint64_t)threadIdx.x * BG_OPT_PER_LANE;
  const int n = bg_optim_lane_count(T.numel, base);
  if (n == 0) return;
  BgOptHead hd;
  hd.c = 1.0f; hd.a = 0.0f; hd.s2 = 1.0f; hd.skipped = 0u;
  if (!SHADOW_ONLY) hd = *head;
  bg_optim_lane<ALGO, SHADOW_ONLY>(T, base, n, n == BG_OPT_PER_LANE && bg_optim_vec(T), h, hd);
}
#endif  // BG_OPTIM_HOST
#endif
