// bg_demo.h -- bg_demo_append_rows / bg_demo_sample: the KEPT demonstration steps of a finished [K + 1, N] store of packed records, compacted into a
// ring of self-contained records on the device, and uniform draws over the ring's filled slots.
//
// Behaviour cloning's data set in the reference is `self.expert_trajectories` (train_balatro_agent.py:220-262): only the steps of the kept episodes,
// growing call by call.  bg_bc_loss can express the filter as a weight over the whole store, but then every minibatch is mostly zero-weight rows, the
// kept steps cost the whole store, and a demonstration stays split over two records (observation and mask in store[t], action and outcome in
// store[t + 1]).  Here the kept rows leave the store.
//
// THE CONTRACT of bg_demo_append_rows -- all of it integer work, held bit for bit (tests/demo_ref.py restates it in numpy):
//   candidate row i = t * N + e, 0 <= t < K, pairs the observation record store[t][e] with the next record store[t + 1][e]
//   row i is KEPT iff weights[i] is finite and > 0 (bg_demo_keep: on the bits, so a denormal is kept whatever the float mode)
//   kept = the kept rows of the call;  T0 = cursor[0] before the call;  the rank r of a kept row = the kept rows with a smaller i
//   the kept row of rank r goes to slot (T0 + r) mod capacity;  with kept > capacity the rows of rank r < kept - capacity are written NOWHERE, so the
//   last `capacity` kept rows survive and no two rows of one call meet in a slot
//   afterwards cursor[0] = T0 + kept, cursor[1] = kept;  the ring holds min(cursor[0], capacity) records
//   the record written = bytes 0..351 of the observation record, but for (bg_demo_blend)
//     bytes 136..143 (BG_ROW_REWARD, float64)                        returns[i] if given, else the next record's
//     bytes 172..175 (BG_ROW_ACTION)                                  the next record's
//     bytes 342..351 (BG_ROW_TERMINATED, _END_FLAGS, _END_ANTE, _END_ROUND, _END_CHIPS)   the next record's
//   bytes 340..341 (boss_blind_active, boss_blind_type) are observation and stay;  bytes 352.. of a ring slot are never written
//   demo_weight[slot] = weights[i] (its bits);  demo_source[slot] = i (when given)
// A demo record is then self-contained: its mask, its action (bytes 172..175), its weight and its return go to bg_encode_rows_ex, bg_linear_rows,
// bg_extractor_rows and bg_bc_loss(actions = a strided view of the ring, mask = the ring, weights = demo_weight, index) as they are.
//
// THREE LAUNCHES, the partials / combine / pass shape of the learner calls; a deterministic order needs the ranks before the scatter:
//   1 bg_demo_count_kernel    per chunk of 1 024 candidate rows (256 lanes x one 16-byte weight load, ballot + popcount) the kept count -> workspace
//   2 bg_demo_scan_kernel     ONE workgroup: the exclusive scan of the chunk counts in index order, 256 chunks per pass with a carry; it reads and
//                             advances the cursor and leaves T0 mod capacity and the drop threshold max(kept - capacity, 0) in the workspace head
//   3 bg_demo_scatter_kernel  per chunk: the same ballots give every kept row its rank, the kept rows that survive are listed in LDS in rank order,
//                             then all 256 lanes copy records as 16-byte pieces (22 per record; consecutive lanes write consecutive pieces)
// No atomics anywhere: two calls on the same inputs give the same bytes.  The cursor never leaves the device.  Vector stores in plain C++ only (the
// ring's through __builtin_nontemporal_store).
//
// bg_demo_sample: filled = min(cursor[0], capacity) read on the device; index[i] = (int32)(((uint64)h * filled) >> 32) with h = bg_head_hash(seed,
// index0 + i, t) -- the rollout's and the head's counter hash; filled == 0 gives -1 (the index bg_bc_loss and bg_encode_rows_ex exclude / zero).  The
// multiply-high draw is biased by at most filled / 2**32 per slot.  The slots of a full ring are all equally old to a learner: the draw is over slots.
//
// The per-row functions are plain C++ behind BG_HEAD_FN: define BG_DEMO_HOST before including and the text the GPU runs compiles with g++, with a
// serial twin of the three launches (bg_demo_append_host) and of the draw (bg_demo_sample_host).
// Out of scope: prioritised or age-aware sampling, deduplication of identical records, a ring shared between GPUs.  (The expert policy that fills the ring is bg_expert_actions, bg_expert.h.)
#ifndef BG_DEMO_H
#define BG_DEMO_H
#if defined(BG_DEMO_HOST) && !defined(BG_HEAD_HOST)
#define BG_HEAD_HOST
#endif
#include "bg_head.h"   // BG_HEAD_FN, bg_head_hash

#define BG_DEMO_LANES 256
#define BG_DEMO_PER_LANE 4                                  /* float32 weights per lane: 16 bytes */
#define BG_DEMO_CHUNK (BG_DEMO_LANES * BG_DEMO_PER_LANE)    /* candidate rows per workgroup */
#define BG_DEMO_PIECES (BG_ROW_BYTES / 16)                  /* 16-byte pieces of a record */
#define BG_DEMO_WS_HEAD 16                                  /* workspace: int64 T0 mod capacity, int64 drop threshold; then uint32 per chunk */
#define BG_DEMO_P_REWARD 8                                  /* the piece whose upper half is the reward */
#define BG_DEMO_P_ACTION 10                                 /* the piece whose last word is the action */
#define BG_DEMO_P_END 21                                    /* the piece of bytes 336..351: 336..341 observation, 342..351 the step that followed */
#define BG_DEMO_UNROLL 4                                    /* pieces a lane has in flight in the copy loop */
#ifndef BG_DEMO_NT
#define BG_DEMO_NT 0                                        /* 1: the store's records are read with non-temporal loads.  Measured and lost */
#endif
#ifndef BG_DEMO_NT_ST
#define BG_DEMO_NT_ST 1                                     /* 1: the ring's records are written with non-temporal stores.  Measured and kept */
#endif
static_assert(BG_ROW_BYTES == 16 * BG_DEMO_PIECES && BG_ROW_REWARD == 16 * BG_DEMO_P_REWARD + 8 && BG_ROW_ACTION == 16 * BG_DEMO_P_ACTION + 12 &&
              BG_ROW_BOSS_BLIND_ACTIVE == 16 * BG_DEMO_P_END + 4 && BG_ROW_TERMINATED == 16 * BG_DEMO_P_END + 6 && BG_ROW_END_CHIPS + 4 == BG_ROW_BYTES,
              "the pieces bg_demo_blend patches are where the record's reward, action and ending fields sit");

typedef uint32_t bg_demo_u4 __attribute__((vector_size(16)));   // a 16-byte piece, to hipcc and to g++ alike

// ---- the per-row functions: the one spelling of every rule ----
// a weight's bits: finite and > 0, i.e. in [0x00000001, 0x7f7fffff] (-0.0, negatives, +inf and every NaN fall outside)
BG_HEAD_FN bool bg_demo_keep(uint32_t wbits) { return wbits - 1u < 0x7f7fffffu; }
// t0m = T0 mod capacity and r are both below 2**31: the sum fits 32 bits
BG_HEAD_FN uint32_t bg_demo_slot(uint32_t t0m, uint32_t r, uint32_t capacity) { return (t0m + r) % capacity; }
BG_HEAD_FN bool bg_demo_needs_next(int p, bool has_ret) { return (p == BG_DEMO_P_REWARD && !has_ret) || p == BG_DEMO_P_ACTION || p == BG_DEMO_P_END; }
// piece p of the demo record from piece p of the observation record (o) and of the next record (n; read only where bg_demo_needs_next)
BG_HEAD_FN bg_demo_u4 bg_demo_blend(int p, bg_demo_u4 o, bg_demo_u4 n, bool has_ret, uint64_t ret_bits) {
  if (p == BG_DEMO_P_REWARD) { o[2] = has_ret ? (uint32_t)ret_bits : n[2]; o[3] = has_ret ? (uint32_t)(ret_bits >> 32) : n[3]; }
  else if (p == BG_DEMO_P_ACTION) o[3] = n[3];
  else if (p == BG_DEMO_P_END) { o[1] = (o[1] & 0x0000ffffu) | (n[1] & 0xffff0000u); o[2] = n[2]; o[3] = n[3]; }
  return o;
}
BG_HEAD_FN uint64_t bg_demo_chunks_of(int64_t store_rows) { return store_rows > 0 ? ((uint64_t)store_rows + BG_DEMO_CHUNK - 1) / BG_DEMO_CHUNK : 0; }
BG_HEAD_FN uint64_t bg_demo_ws_bytes(int64_t store_rows) {
  return store_rows > 0 ? BG_DEMO_WS_HEAD + ((bg_demo_chunks_of(store_rows) * sizeof(uint32_t) + 15) & ~(uint64_t)15) : 0;
}
// what the scan's lane 0 does at its end with the call's kept count: the head for pass 3 and the cursor
BG_HEAD_FN void bg_demo_finish(uint32_t kept, int64_t capacity, int64_t* cursor, int64_t* head) {
  const int64_t T0 = cursor[0] < 0 ? 0 : cursor[0];   // (a negative count is not a state the call leaves: it is taken as an empty ring)
  head[0] = T0 % capacity;
  head[1] = (int64_t)kept > capacity ? (int64_t)kept - capacity : 0;
  cursor[0] = T0 + (int64_t)kept;
  cursor[1] = (int64_t)kept;
}
// the kept rows of a chunk that survive are those of chunk rank >= first (the dropped ranks are a prefix of the call's, so of the chunk's)
BG_HEAD_FN uint32_t bg_demo_first(int64_t drop, uint32_t off, uint32_t cnt) {
  if (drop <= (int64_t)off) return 0u;
  const int64_t d = drop - (int64_t)off;
  return d < (int64_t)cnt ? (uint32_t)d : cnt;
}
BG_HEAD_FN int64_t bg_demo_filled(int64_t total, int64_t capacity) { return total < 0 ? 0 : total < capacity ? total : capacity; }
BG_HEAD_FN int32_t bg_demo_draw(uint32_t h, int64_t filled) { return filled <= 0 ? -1 : (int32_t)(((uint64_t)h * (uint64_t)filled) >> 32); }

// the 4 keep bits of one lane: rows base .. base + 3 of M (vec: the weights are 16-byte aligned, so a lane whose rows all exist takes one load)
BG_HEAD_FN uint32_t bg_demo_lane_mask(const uint32_t* wbits, int64_t base, int64_t M, bool vec) {
  uint32_t mask = 0u;
  if (vec && base + BG_DEMO_PER_LANE <= M) {
    const bg_demo_u4 q = *reinterpret_cast<const bg_demo_u4*>(wbits + base);
    mask = (bg_demo_keep(q[0]) ? 1u : 0u) | (bg_demo_keep(q[1]) ? 2u : 0u) | (bg_demo_keep(q[2]) ? 4u : 0u) | (bg_demo_keep(q[3]) ? 8u : 0u);
  } else {
    for (int j = 0; j < BG_DEMO_PER_LANE; j++)
      if (base + j < M && bg_demo_keep(wbits[base + j])) mask |= 1u << j;
  }
  return mask;
}

struct BgDemoArgs {
  const uint8_t* rows; uint64_t stride; int64_t N, M;          // the store and its K * N candidate rows
  const uint32_t* wbits; int vec;                              // the weights' bits; 16-byte aligned
  const uint64_t* ret_bits;                                    // nullable: the returns' bits
  uint8_t* demo; uint64_t dstride; int64_t capacity;
  uint32_t* demo_weight; int32_t* demo_source;                 // demo_source nullable
  const int64_t* head; const uint32_t* offs;                   // the workspace after the scan
};

#ifdef BG_DEMO_HOST
// ---- the serial twin of the three launches: every pointer is a host pointer; workspace as the device's ----
static inline void bg_demo_append_host(const uint8_t* rows, uint64_t stride, int K, int64_t N, const float* weights, const double* returns, uint8_t* demo,
                                       uint64_t dstride, int64_t capacity, float* demo_weight, int32_t* demo_source, int64_t* cursor, void* workspace) {
  const int64_t M = (int64_t)K * N;
  if (M <= 0) return;
  const uint32_t* const wbits = (const uint32_t*)weights;
  const uint64_t* const rbits = (const uint64_t*)returns;
  int64_t* const head = (int64_t*)workspace;
  uint32_t* const offs = (uint32_t*)((uint8_t*)workspace + BG_DEMO_WS_HEAD);
  const int64_t chunks = (int64_t)bg_demo_chunks_of(M);
  const bool vec = ((uintptr_t)weights & 15) == 0;
  for (int64_t c = 0; c < chunks; c++) {                       // 1: count
    uint32_t n = 0;
    for (int l = 0; l < BG_DEMO_LANES; l++) n += (uint32_t)__builtin_popcount(bg_demo_lane_mask(wbits, c * BG_DEMO_CHUNK + l * BG_DEMO_PER_LANE, M, vec));
    offs[c] = n;
  }
  uint32_t carry = 0;                                          // 2: scan
  for (int64_t c = 0; c < chunks; c++) { const uint32_t n = offs[c]; offs[c] = carry; carry += n; }
  bg_demo_finish(carry, capacity, cursor, head);
  const uint32_t t0m = (uint32_t)head[0];
  for (int64_t c = 0; c < chunks; c++) {                       // 3: scatter
    const uint32_t cnt = (c + 1 < chunks ? offs[c + 1] : carry) - offs[c];
    const uint32_t first = bg_demo_first(head[1], offs[c], cnt);
    uint32_t p = 0;
    for (int l = 0; l < BG_DEMO_LANES; l++) {
      const int64_t base = c * BG_DEMO_CHUNK + l * BG_DEMO_PER_LANE;
      const uint32_t mask = bg_demo_lane_mask(wbits, base, M, vec);
      for (int j = 0; j < BG_DEMO_PER_LANE; j++) {
        if (!((mask >> j) & 1u)) continue;
        const uint32_t rank = p++;
        if (rank < first) continue;
        const int64_t i = base + j;
        const uint32_t slot = bg_demo_slot(t0m, offs[c] + rank, (uint32_t)capacity);
        const uint8_t* const ob = rows + (uint64_t)i * stride;
        const uint8_t* const nx = rows + (uint64_t)(i + N) * stride;
        uint8_t* const out = demo + (uint64_t)slot * dstride;
        for (int pc = 0; pc < BG_DEMO_PIECES; pc++) {
          bg_demo_u4 o, n = {0u, 0u, 0u, 0u};
          __builtin_memcpy(&o, ob + 16 * pc, 16);
          if (bg_demo_needs_next(pc, rbits != nullptr)) __builtin_memcpy(&n, nx + 16 * pc, 16);
          o = bg_demo_blend(pc, o, n, rbits != nullptr, rbits && pc == BG_DEMO_P_REWARD ? rbits[i] : 0ull);
          __builtin_memcpy(out + 16 * pc, &o, 16);
        }
        __builtin_memcpy(&demo_weight[slot], &wbits[i], 4);
        if (demo_source) demo_source[slot] = (int32_t)i;
      }
    }
  }
}
static inline void bg_demo_sample_host(const int64_t* cursor, int64_t capacity, uint64_t seed, uint64_t index0, uint64_t t, int32_t* index, int64_t m) {
  const int64_t filled = bg_demo_filled(cursor[0], capacity);
  for (int64_t i = 0; i < m; i++) index[i] = bg_demo_draw(bg_head_hash(seed, index0 + (uint64_t)i, t), filled);
}
#else
// ---- the kernels ----
// what a lane learns from the ballots of its wave over the 4 keep bits: the kept rows of the lower lanes (all of a smaller i) and of the whole wave
struct BgDemoWave { uint32_t below, total; };
__device__ __forceinline__ BgDemoWave bg_demo_wave(uint32_t mask) {
  const unsigned long long lower = (1ull << (threadIdx.x & 63u)) - 1ull;
  BgDemoWave w; w.below = 0u; w.total = 0u;
#pragma unroll
  for (int j = 0; j < BG_DEMO_PER_LANE; j++) {
    const unsigned long long b = __ballot((mask >> j) & 1u);
    w.total += (uint32_t)__popcll(b);
    w.below += (uint32_t)__popcll(b & lower);
  }
  return w;
}

// (every kernel here is a template, as bg_optim.h's are: the compiler then emits them behind the kernels that exist, whose text stays as it was)
template <int LANES>
__global__ __launch_bounds__(LANES) void bg_demo_count_kernel(const uint32_t* __restrict__ wbits, int64_t M, int vec, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wave_n[BG_DEMO_LANES / 64];
  const int64_t base = (int64_t)blockIdx.x * BG_DEMO_CHUNK + (int64_t)threadIdx.x * BG_DEMO_PER_LANE;
  const BgDemoWave w = bg_demo_wave(bg_demo_lane_mask(wbits, base, M, vec != 0));
  if ((threadIdx.x & 63u) == 0u) wave_n[threadIdx.x >> 6] = w.total;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}

// one workgroup; counts[c] becomes the kept rows of the chunks in front of c.  256 chunks per pass: a wave scans its 64 by shuffles, the four wave
// totals meet in LDS, the carry runs from pass to pass in a register every lane holds.
template <int LANES>
__global__ __launch_bounds__(LANES) void bg_demo_scan_kernel(uint32_t* __restrict__ counts, int64_t chunks, int64_t capacity, int64_t* __restrict__ cursor,
                                                                     int64_t* __restrict__ head) {
  __shared__ uint32_t wave_t[BG_DEMO_LANES / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t carry = 0u;
  for (int64_t c0 = 0; c0 < chunks; c0 += BG_DEMO_LANES) {
    const int64_t c = c0 + threadIdx.x;
    const uint32_t v = c < chunks ? counts[c] : 0u;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(x, d);
      if (lane >= (uint32_t)d) x += y;
    }
    if (lane == 63u) wave_t[wave] = x;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
#pragma unroll
    for (uint32_t q = 0; q < BG_DEMO_LANES / 64; q++) { const uint32_t n = wave_t[q]; total += n; if (q < wave) before += n; }
    if (c < chunks) counts[c] = carry + before + (x - v);
    carry += total;
    __syncthreads();   // wave_t is written again in the next pass
  }
  if (threadIdx.x == 0) bg_demo_finish(carry, capacity, cursor, head);
}

template <bool NT>
__device__ __forceinline__ bg_demo_u4 bg_demo_load(const uint8_t* p) {
  return NT ? __builtin_nontemporal_load(reinterpret_cast<const bg_demo_u4*>(p)) : *reinterpret_cast<const bg_demo_u4*>(p);
}
// RET: returns are given.  NT: the store's records are read with non-temporal loads -- they are streamed once, but a record is read twice, as a
// row's observation and as the next record of the row one step earlier, and the plain load keeps it for the second reader: the A/B kept plain loads.
// The ring is written with non-temporal stores (BG_DEMO_NT_ST; 0 builds the other side of that A/B): a slot's 352 of 384 bytes leave as they are, and
// the learner's first gather of a minibatch from the ring costs the same either way.
template <bool RET, bool NT>
__global__ __launch_bounds__(BG_DEMO_LANES) void bg_demo_scatter_kernel(BgDemoArgs A) {
  __shared__ uint32_t list[BG_DEMO_CHUNK];                    // the chunk's kept rows (their index inside the chunk) in rank order
  __shared__ uint32_t wave_n[BG_DEMO_LANES / 64];
  const uint32_t wave = threadIdx.x >> 6;
  const int64_t chunk0 = (int64_t)blockIdx.x * BG_DEMO_CHUNK;
  const uint32_t mask = bg_demo_lane_mask(A.wbits, chunk0 + (int64_t)threadIdx.x * BG_DEMO_PER_LANE, A.M, A.vec != 0);
  const BgDemoWave w = bg_demo_wave(mask);
  if ((threadIdx.x & 63u) == 0u) wave_n[wave] = w.total;
  __syncthreads();
  uint32_t p = w.below, cnt = 0u;
#pragma unroll
  for (uint32_t q = 0; q < BG_DEMO_LANES / 64; q++) { const uint32_t n = wave_n[q]; cnt += n; if (q < wave) p += n; }
#pragma unroll
  for (int j = 0; j < BG_DEMO_PER_LANE; j++)
    if ((mask >> j) & 1u) list[p++] = threadIdx.x * BG_DEMO_PER_LANE + (uint32_t)j;
  __syncthreads();
  const uint32_t off = A.offs[blockIdx.x], t0m = (uint32_t)A.head[0], cap = (uint32_t)A.capacity;
  const uint32_t first = bg_demo_first(A.head[1], off, cnt);
  const uint32_t n = cnt - first;                              // records this workgroup writes (<= 1 024)
  for (uint32_t q = threadIdx.x; q < n; q += BG_DEMO_LANES) {  // the side arrays
    const int64_t i = chunk0 + (int64_t)list[first + q];
    const uint32_t slot = bg_demo_slot(t0m, off + first + q, cap);
    A.demo_weight[slot] = A.wbits[i];
    if (A.demo_source) A.demo_source[slot] = (int32_t)i;
  }
  const uint32_t items = n * BG_DEMO_PIECES;                   // 16-byte pieces: consecutive lanes write consecutive pieces of a record
  for (uint32_t it0 = threadIdx.x; it0 < items; it0 += BG_DEMO_LANES * BG_DEMO_UNROLL) {
    bg_demo_u4 o[BG_DEMO_UNROLL], nx[BG_DEMO_UNROLL];
    uint64_t rb[BG_DEMO_UNROLL];
    uint64_t doff[BG_DEMO_UNROLL];                             // the piece's offset in the ring: the address is formed at the store, from A.demo, so it stays a global one
    int pc[BG_DEMO_UNROLL];
#pragma unroll
    for (int u = 0; u < BG_DEMO_UNROLL; u++) {
      const uint32_t it = it0 + (uint32_t)u * BG_DEMO_LANES;
      pc[u] = -1; rb[u] = 0ull; doff[u] = 0ull;
      nx[u] = bg_demo_u4{0u, 0u, 0u, 0u};
      if (it < items) {
        const uint32_t q = it / BG_DEMO_PIECES;
        pc[u] = (int)(it - q * BG_DEMO_PIECES);
        const int64_t i = chunk0 + (int64_t)list[first + q];
        const uint8_t* const ob = A.rows + (uint64_t)i * A.stride + 16u * (uint32_t)pc[u];
        doff[u] = (uint64_t)bg_demo_slot(t0m, off + first + q, cap) * A.dstride + 16u * (uint32_t)pc[u];
        o[u] = bg_demo_load<NT>(ob);
        if (bg_demo_needs_next(pc[u], RET)) nx[u] = bg_demo_load<NT>(ob + (uint64_t)A.N * A.stride);
        if (RET && pc[u] == BG_DEMO_P_REWARD) rb[u] = A.ret_bits[i];
      }
    }
#pragma unroll
    for (int u = 0; u < BG_DEMO_UNROLL; u++)
      if (pc[u] >= 0) {
        const bg_demo_u4 v = bg_demo_blend(pc[u], o[u], nx[u], RET, rb[u]);
        bg_demo_u4* const dst = reinterpret_cast<bg_demo_u4*>(A.demo + doff[u]);
        if (BG_DEMO_NT_ST) __builtin_nontemporal_store(v, dst);
        else *dst = v;
      }
  }
}
template <int LANES>
__global__ __launch_bounds__(LANES) void bg_demo_sample_kernel(const int64_t* __restrict__ cursor, int64_t capacity, uint64_t seed, uint64_t index0, uint64_t t,
                                                                       int32_t* __restrict__ index, int64_t m) {
  const int64_t i = (int64_t)blockIdx.x * BG_DEMO_LANES + threadIdx.x;
  if (i >= m) return;
  index[i] = bg_demo_draw(bg_head_hash(seed, index0 + (uint64_t)i, t), bg_demo_filled(cursor[0], capacity));
}
#endif  // BG_DEMO_HOST
#endif
