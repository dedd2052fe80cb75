// bg_encode.h -- bg_encode_rows: packed records (BG_ROW_*) -> the float matrix a policy network reads.
//
// Three layouts, all restatements of what the reference feeds its networks (include/balatro_mi355x.h has the citations):
//   BG_ENC_PRODUCED  the 31 keys the env fills, in the reference's key order, every element as float        153 columns
//   BG_ENC_FIXED     PRODUCED + the 20 declared-but-never-filled keys of BalatroEnvFixed as zeros           628 columns
//   BG_ENC_EXTRACTOR what BalatroFeaturesExtractor.forward builds: hand one-hot, joker ids, 21 state features 447 columns
//
// ONE column table per layout, built at compile time from the X-macro lists below (key, record offset, source type, count [, divisor]):
// the kernel, bg_encode_cols, the host build of tests/test_encode_rows_host.py and -- through that test -- _native.ENC_COLUMNS all
// read these lists and nothing else.  The per-element conversion and the bf16 rounding are plain C++ behind BG_ENC_FN, so the text the
// GPU runs compiles with g++ (define BG_ENC_HOST before including; the pattern of tests/test_seed_slot_host.py).
#ifndef BG_ENCODE_H
#define BG_ENCODE_H
#include <stdint.h>

#ifdef BG_ENC_HOST
#define BG_ENC_FN static inline
#define BG_ENC_TABLE static constexpr
#else
#define BG_ENC_FN __host__ __device__ __forceinline__
#define BG_ENC_TABLE static __device__ constexpr
#endif

// source types of a record field
#define BG_ENC_SRC_I8 0
#define BG_ENC_SRC_I16 1
#define BG_ENC_SRC_I32 2
#define BG_ENC_SRC_I64 3
#define BG_ENC_SRC_F32 4 /* copied bit for bit */
// per-column rule
#define BG_ENC_OP_NONE 0
#define BG_ENC_OP_DIV 1    /* float32(value) / float32(divisor): an IEEE division, as numpy / torch-CPU compute `x.float() / c` */
#define BG_ENC_OP_ONEHOT 2 /* 1.0 where the int8 field equals the column's card (a card is >= 0, so the -1 padding never matches) */
#define BG_ENC_OP_ZERO 3   /* a never-produced key of the fixed space */

// X(key, record offset, source type, elements): the keys `_get_observation()` fills, in the order of the reference's observation space
// (balatro_env_2.py:388-468; _native.OBS_KEYS; tests/golden/sb3_fixed.npz `keys`[:31])
#define BG_ENC_PRODUCED_KEYS(X)                                   \
  X(hand, BG_ROW_HAND, BG_ENC_SRC_I8, 8)                              \
  X(hand_size, BG_ROW_HAND_SIZE, BG_ENC_SRC_I8, 1)                    \
  X(deck_size, BG_ROW_DECK_SIZE, BG_ENC_SRC_I8, 1)                    \
  X(selected_cards, BG_ROW_SELECTED_CARDS, BG_ENC_SRC_I64, 8)         \
  X(chips_scored, BG_ROW_CHIPS_SCORED, BG_ENC_SRC_I64, 1)             \
  X(round_chips_scored, BG_ROW_ROUND_CHIPS_SCORED, BG_ENC_SRC_I32, 1) \
  X(progress_ratio, BG_ROW_PROGRESS_RATIO, BG_ENC_SRC_F32, 1)         \
  X(mult, BG_ROW_MULT, BG_ENC_SRC_I32, 1)                             \
  X(chips_needed, BG_ROW_CHIPS_NEEDED, BG_ENC_SRC_I32, 1)             \
  X(money, BG_ROW_MONEY, BG_ENC_SRC_I32, 1)                           \
  X(ante, BG_ROW_ANTE, BG_ENC_SRC_I16, 1)                             \
  X(round, BG_ROW_ROUND, BG_ENC_SRC_I8, 1)                            \
  X(hands_left, BG_ROW_HANDS_LEFT, BG_ENC_SRC_I8, 1)                  \
  X(discards_left, BG_ROW_DISCARDS_LEFT, BG_ENC_SRC_I8, 1)            \
  X(joker_count, BG_ROW_JOKER_COUNT, BG_ENC_SRC_I8, 1)                \
  X(joker_ids, BG_ROW_JOKER_IDS, BG_ENC_SRC_I16, 10)                  \
  X(joker_slots, BG_ROW_JOKER_SLOTS, BG_ENC_SRC_I8, 1)                \
  X(consumable_count, BG_ROW_CONSUMABLE_COUNT, BG_ENC_SRC_I8, 1)      \
  X(consumables, BG_ROW_CONSUMABLES, BG_ENC_SRC_I16, 5)               \
  X(consumable_slots, BG_ROW_CONSUMABLE_SLOTS, BG_ENC_SRC_I8, 1)      \
  X(shop_items, BG_ROW_SHOP_ITEMS, BG_ENC_SRC_I16, 10)                \
  X(shop_costs, BG_ROW_SHOP_COSTS, BG_ENC_SRC_I16, 10)                \
  X(shop_rerolls, BG_ROW_SHOP_REROLLS, BG_ENC_SRC_I16, 1)             \
  X(hand_levels, BG_ROW_HAND_LEVELS, BG_ENC_SRC_I8, 12)               \
  X(phase, BG_ROW_PHASE, BG_ENC_SRC_I8, 1)                            \
  X(action_mask, BG_ROW_ACTION_MASK, BG_ENC_SRC_I8, 60)               \
  X(hands_played, BG_ROW_HANDS_PLAYED, BG_ENC_SRC_I32, 1)             \
  X(best_hand_this_ante, BG_ROW_BEST_HAND_THIS_ANTE, BG_ENC_SRC_I32, 1) \
  X(boss_blind_active, BG_ROW_BOSS_BLIND_ACTIVE, BG_ENC_SRC_I8, 1)    \
  X(boss_blind_type, BG_ROW_BOSS_BLIND_TYPE, BG_ENC_SRC_I8, 1)        \
  X(face_down_cards, BG_ROW_FACE_DOWN_CARDS, BG_ENC_SRC_I64, 8)
// X(key, elements): the keys the env declares (balatro_env_2.py:386-470) and never fills; BalatroEnvFixed zero-fills them
// (train_balatro_fixed.py:125-207), in the order of the fixed space (sb3_fixed.npz `keys`[31:])
#define BG_ENC_ZERO_KEYS(X)      \
  X(hand_one_hot, 416)           \
  X(hand_suits, 8)               \
  X(hand_ranks, 8)               \
  X(rank_counts, 13)             \
  X(suit_counts, 4)              \
  X(straight_potential, 1)       \
  X(flush_potential, 1)          \
  X(avg_score_per_hand, 1)       \
  X(hands_until_shop, 1)         \
  X(rounds_until_boss, 1)        \
  X(has_mult_jokers, 1)          \
  X(has_chip_jokers, 1)          \
  X(has_xmult_jokers, 1)         \
  X(has_economy_jokers, 1)       \
  X(hand_potential_scores, 12)   \
  X(joker_synergy_score, 1)      \
  X(risk_level, 1)               \
  X(economy_health, 1)           \
  X(blind_difficulty, 1)         \
  X(win_probability, 1)
// X(key, record offset, source type, elements, divisor index | -1): `game_features` of BalatroFeaturesExtractor.forward
// (train_balatro_agent.py:102-113), behind the hand one-hot (:86-93) and `joker_ids.float()` (:98)
#define BG_ENC_EXTRACTOR_STATE(X)                        \
  X(chips_scored, BG_ROW_CHIPS_SCORED, BG_ENC_SRC_I64, 1, 0) \
  X(chips_needed, BG_ROW_CHIPS_NEEDED, BG_ENC_SRC_I32, 1, 1) \
  X(progress_ratio, BG_ROW_PROGRESS_RATIO, BG_ENC_SRC_F32, 1, -1) \
  X(money, BG_ROW_MONEY, BG_ENC_SRC_I32, 1, 2)               \
  X(ante, BG_ROW_ANTE, BG_ENC_SRC_I16, 1, 3)                 \
  X(round, BG_ROW_ROUND, BG_ENC_SRC_I8, 1, 4)                \
  X(hands_left, BG_ROW_HANDS_LEFT, BG_ENC_SRC_I8, 1, 3)      \
  X(discards_left, BG_ROW_DISCARDS_LEFT, BG_ENC_SRC_I8, 1, 5) \
  X(hand_levels, BG_ROW_HAND_LEVELS, BG_ENC_SRC_I8, 12, 3)   \
  X(phase, BG_ROW_PHASE, BG_ENC_SRC_I8, 1, 4)

#define BG_ENC_COUNT4(k, o, t, n) +(n)
#define BG_ENC_COUNT2(k, n) +(n)
#define BG_ENC_COUNT5(k, o, t, n, d) +(n)
#define BG_ENC_PRODUCED_COLS (0 BG_ENC_PRODUCED_KEYS(BG_ENC_COUNT4))
#define BG_ENC_FIXED_COLS (BG_ENC_PRODUCED_COLS BG_ENC_ZERO_KEYS(BG_ENC_COUNT2))
#define BG_ENC_ONEHOT_COLS (8 * 52)
#define BG_ENC_ONEHOT_SLOT(c) ((c) / 52) /* one-hot column c = slot * 52 + card */
#define BG_ENC_ONEHOT_CARD(c) ((c) % 52)
#define BG_ENC_JOKER_COLS 10
#define BG_ENC_EXTRACTOR_COLS (BG_ENC_ONEHOT_COLS + BG_ENC_JOKER_COLS BG_ENC_EXTRACTOR_STATE(BG_ENC_COUNT5))
#define BG_ENC_MAX_COLS BG_ENC_FIXED_COLS
static_assert(BG_ENC_PRODUCED_COLS == 153 && BG_ENC_FIXED_COLS == 628 && BG_ENC_EXTRACTOR_COLS == 447, "layout widths of include/balatro_mi355x.h");

constexpr int bg_enc_cols(int layout) {
  return layout == BG_ENC_PRODUCED ? BG_ENC_PRODUCED_COLS : layout == BG_ENC_FIXED ? BG_ENC_FIXED_COLS : layout == BG_ENC_EXTRACTOR ? BG_ENC_EXTRACTOR_COLS : -1;
}

// A column: bits 0..8 byte offset of the element in the record, 9..11 source type, 12..13 rule, 14..19 the one-hot card / the divisor index
constexpr uint32_t bg_enc_desc(uint32_t off, uint32_t type, uint32_t op, uint32_t par) { return off | type << 9 | op << 12 | par << 14; }
#define BG_ENC_OFF(d) ((d) & 0x1ffu)
#define BG_ENC_TYPE(d) (((d) >> 9) & 7u)
#define BG_ENC_OP(d) (((d) >> 12) & 3u)
#define BG_ENC_PAR(d) (((d) >> 14) & 0x3fu)
constexpr uint32_t bg_enc_type_bytes(uint32_t t) { return t == BG_ENC_SRC_I8 ? 1u : t == BG_ENC_SRC_I16 ? 2u : t == BG_ENC_SRC_I64 ? 8u : 4u; }

template <int LAYOUT>
struct BgEncTable {
  uint32_t d[BG_ENC_MAX_COLS] = {};
  constexpr BgEncTable() {
    int c = 0;
    if (LAYOUT == BG_ENC_EXTRACTOR) {
      for (; c < BG_ENC_ONEHOT_COLS; c++) d[c] = bg_enc_desc(BG_ROW_HAND + BG_ENC_ONEHOT_SLOT(c), BG_ENC_SRC_I8, BG_ENC_OP_ONEHOT, BG_ENC_ONEHOT_CARD(c));
      for (int j = 0; j < BG_ENC_JOKER_COLS; j++) d[c++] = bg_enc_desc(BG_ROW_JOKER_IDS + 2 * j, BG_ENC_SRC_I16, BG_ENC_OP_NONE, 0);
#define BG_ENC_X(k, o, t, n, dv) \
  for (int i = 0; i < (n); i++) d[c++] = bg_enc_desc((o) + i * bg_enc_type_bytes(t), t, (dv) >= 0 ? BG_ENC_OP_DIV : BG_ENC_OP_NONE, (dv) >= 0 ? (dv) : 0);
      BG_ENC_EXTRACTOR_STATE(BG_ENC_X)
#undef BG_ENC_X
    } else {
#define BG_ENC_X(k, o, t, n) \
  for (int i = 0; i < (n); i++) d[c++] = bg_enc_desc((o) + i * bg_enc_type_bytes(t), t, BG_ENC_OP_NONE, 0);
      BG_ENC_PRODUCED_KEYS(BG_ENC_X)
#undef BG_ENC_X
      if (LAYOUT == BG_ENC_FIXED)
        while (c < BG_ENC_FIXED_COLS) d[c++] = bg_enc_desc(0, BG_ENC_SRC_F32, BG_ENC_OP_ZERO, 0);
    }
  }
};
template <int LAYOUT>
struct BgEncTab { BG_ENC_TABLE BgEncTable<LAYOUT> t{}; };

// an aligned 32-bit word of a record (records are 16-byte aligned in HBM, in LDS and in the host build's buffers)
BG_ENC_FN uint32_t bg_enc_word(const uint8_t* rec, uint32_t off) {
  uint32_t w;
  __builtin_memcpy(&w, __builtin_assume_aligned(rec + off, 4), 4);
  return w;
}
BG_ENC_FN uint32_t bg_enc_float_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
BG_ENC_FN uint32_t bg_enc_onehot(int32_t hand_value, int32_t card) { return hand_value == card ? 0x3f800000u : 0u; }   // float32 bits of 1.0 / 0.0
BG_ENC_FN float bg_enc_divisor(uint32_t i) {
  return i == 0 ? 1e6f : i == 1 ? 1e5f : i == 2 ? 100.f : i == 3 ? 10.f : i == 4 ? 3.f : 5.f;
}

// The float32 BIT PATTERN of one column of one record: numpy.float32(value) (round to nearest even from int32 / int64), a float field
// bit for bit, then the column's rule.
template <int LAYOUT>
BG_ENC_FN uint32_t bg_enc_element(const uint8_t* rec, uint32_t d) {
  const uint32_t off = BG_ENC_OFF(d), type = BG_ENC_TYPE(d), op = BG_ENC_OP(d);
  if (LAYOUT == BG_ENC_FIXED && op == BG_ENC_OP_ZERO) return 0u;
  const uint32_t lo = bg_enc_word(rec, off & ~3u);
  if (type == BG_ENC_SRC_F32) return lo;
  float f;
  if (type == BG_ENC_SRC_I64) {
    const uint32_t hi = bg_enc_word(rec, off + 4u);
    f = (float)(int64_t)((uint64_t)hi << 32 | lo);
  } else {
    const uint32_t v = lo >> ((off & 3u) * 8u);
    const int32_t s = type == BG_ENC_SRC_I8 ? (int32_t)(int8_t)v : type == BG_ENC_SRC_I16 ? (int32_t)(int16_t)v : (int32_t)v;
    if (LAYOUT == BG_ENC_EXTRACTOR && op == BG_ENC_OP_ONEHOT) return bg_enc_onehot(s, (int32_t)BG_ENC_PAR(d));
    f = (float)s;
  }
  if (LAYOUT == BG_ENC_EXTRACTOR && op == BG_ENC_OP_DIV) f = f / bg_enc_divisor(BG_ENC_PAR(d));
  return bg_enc_float_bits(f);
}

// float32 bits -> bfloat16 bits, round to nearest even; a NaN becomes the canonical quiet NaN (what torch's float -> bfloat16 gives)
BG_ENC_FN uint16_t bg_enc_bf16(uint32_t u) {
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)0x7fc0u;
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// bg_encode_rows_ex's index: the record an index value names, or -1 ("none": the output row is zeros and nothing is read) when it is outside
// [0, store_rows) -- the rule by which bg_ppo_loss excludes a row, so the two calls agree on a minibatch
BG_ENC_FN int64_t bg_enc_source_row(int32_t index, int64_t store_rows) { return index >= 0 && (int64_t)index < store_rows ? (int64_t)index : (int64_t)-1; }

#ifndef BG_ENC_HOST
#include <type_traits>
// ---- the records-to-tile pipeline ----
// bg_encode_kernel, bg_norm_obs_kernel, their GATHER variants (bg_norm.h) and the first layer (bg_linear.h) are this code; they differ in the converter
// of phase 2 alone.  A workgroup of 256 lanes takes BG_ENC_RECS = 32 records, in three phases with a barrier between them:
//   1  bg_enc_stage: the records' 352 bytes are read from HBM once, 16 bytes per lane, into LDS (record pitch 356 bytes = 89 words: odd, so phase 2's
//      lanes, one record each, read without bank conflicts);
//   2  bg_enc_fill_tile: lane = (record, one of 8 column slices).  bg_enc_slices hands the slice to the converter as a compile-time constant, so the
//      layout's DENSE columns -- the 153 produced ones; for EXTRACTOR the 31 behind the one-hot -- are converted with the column index a constant (the
//      table folds away: one LDS read, a bit-field extract and a convert per column; the int64, division and float64 sequences only where a column
//      needs them) into a float32 tile in LDS (pitch 153 / 31 words: odd again).  The converters: BgEncConvert<LAYOUT> here, BgNormConvert (bg_norm.h);
//   3  bg_enc_store: the lanes walk the output with consecutive lanes on consecutive 16-byte pieces, reading finished values from the tile:
//        BG_ENC_ST_ROWS  out_dev and the row pitch are 16-byte aligned: a piece is 4 (f32) / 8 (bf16) columns of one row, the row's tail by element
//        BG_ENC_ST_FLAT  rows are not 16-byte aligned but the matrix is dense (pitch == columns) and out_dev aligned: a workgroup's rows are ONE
//                        aligned run of RECS * D elements, so pieces run across row ends (RECS * D * 2 bytes is a multiple of 16)
//        BG_ENC_ST_ELEM  anything else: one element per lane
//      FIXED's 475 zero columns touch neither LDS nor the table; EXTRACTOR's 416 one-hot columns are computed here from the record's hand bytes
//      (bg_enc_onehot: a byte read and a compare per element).
// LDS: 11 392 bytes of records + 19 584 (153-column tile) or 3 968 (EXTRACTOR) bytes: five / eight workgroups per CU.
// GATHER (bg_encode_rows_ex; a compile-time variant): phase 1 first resolves the workgroup's 32 indices once (bg_enc_source_row) into LDS, a barrier,
// then the 22 pieces of record r come from rows + src[r] * stride -- still consecutive lanes on consecutive 16-byte pieces of a record, so a record of
// stride 384 is fetched as its three lines.  A record with no source is not read: its LDS image is filled with 0xff (a hand of -1: phase 3's one-hot
// columns come out 0.0) and phase 2 writes zeros into its tile row, so phase 3 is the same code.  index == NULL is the identity (statistics without an
// index).
#define BG_ENC_BLOCK 256
#define BG_ENC_RECS 32
#define BG_ENC_SLICES (BG_ENC_BLOCK / BG_ENC_RECS)
#define BG_ENC_CHUNKS (BG_ROW_BYTES / 16)
#define BG_ENC_REC_PITCH (BG_ROW_BYTES + 4)
#define BG_ENC_ST_ROWS 0
#define BG_ENC_ST_FLAT 1
#define BG_ENC_ST_ELEM 2
static_assert(BG_ROW_BYTES % 16 == 0 && BG_ENC_RECS % 8 == 0, "records are staged in 16-byte pieces; a workgroup's dense output starts on a 16-byte boundary");
static_assert((BG_ENC_REC_PITCH / 4) % 2 == 1 && BG_ENC_REC_PITCH % 4 == 0, "odd word pitch: lane = record reads are conflict-free");
static_assert(BG_ENC_SLICES == 8, "bg_enc_slices names every slice");

// the dense columns of a layout: [first, first + count) are staged in the tile
constexpr int bg_enc_dense_first(int layout) { return layout == BG_ENC_EXTRACTOR ? BG_ENC_ONEHOT_COLS : 0; }
constexpr int bg_enc_dense_cols(int layout) { return layout == BG_ENC_EXTRACTOR ? BG_ENC_EXTRACTOR_COLS - BG_ENC_ONEHOT_COLS : BG_ENC_PRODUCED_COLS; }

// phase 1: the first nrec records of the workgroup into LDS, in 16-byte pieces, by BLOCK lanes.  from(r) is the record of `rows` that fills slot r; a
// signed source may say -1 (no record: the image is 0xff and nothing is read), an unsigned one never does and the test folds away
template <int BLOCK, class FROM>
__device__ __forceinline__ void bg_enc_stage(const uint8_t* __restrict__ rows, uint64_t row_stride, int nrec, uint32_t* recs32, FROM from) {
  for (int c = threadIdx.x; c < nrec * BG_ENC_CHUNKS; c += BLOCK) {
    const int r = c / BG_ENC_CHUNKS, p = c - r * BG_ENC_CHUNKS;
    const auto at = from(r);
    const uint4 v = at >= 0 ? *reinterpret_cast<const uint4*>(rows + (size_t)at * row_stride + p * 16) : make_uint4(~0u, ~0u, ~0u, ~0u);
    uint32_t* const w = recs32 + r * (BG_ENC_REC_PITCH / 4) + p * 4;
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  }
}
// phase 1 of the GATHER variants: the workgroup's sources into LDS (one barrier), then the records
__device__ __forceinline__ void bg_enc_stage_gather(const uint8_t* __restrict__ rows, uint64_t row_stride, const int32_t* __restrict__ index, long long store_rows,
                                                    long long rec0, int nrec, long long* src, uint32_t* recs32) {
  if ((int)threadIdx.x < nrec) src[threadIdx.x] = index ? bg_enc_source_row(index[rec0 + threadIdx.x], store_rows) : rec0 + threadIdx.x;
  __syncthreads();
  bg_enc_stage<BG_ENC_BLOCK>(rows, row_stride, nrec, recs32, [src](int r) { return src[r]; });
}

template <int LAYOUT, int S>
__device__ __forceinline__ void bg_enc_convert_slice(const uint8_t* rec, uint32_t* dst) {
  constexpr int N = bg_enc_dense_cols(LAYOUT), C0 = bg_enc_dense_first(LAYOUT), CH = (N + BG_ENC_SLICES - 1) / BG_ENC_SLICES;
#pragma unroll
  for (int i = S * CH; i < (S + 1) * CH; i++)
    if (i < N) dst[i] = bg_enc_element<LAYOUT>(rec, BgEncTab<LAYOUT>::t.d[C0 + i]);
}
// a converter of phase 2: slice S of record `i` of the call, whose LDS image is `rec`, into its tile row `dst`
template <int LAYOUT>
struct BgEncConvert {
  template <int S>
  __device__ __forceinline__ void operator()(std::integral_constant<int, S>, const uint8_t* rec, long long, uint32_t* dst) const { bg_enc_convert_slice<LAYOUT, S>(rec, dst); }
};

// the tile row of a record without a source (GATHER): slice `s` of its N dense columns as +0.0
template <int N>
__device__ __forceinline__ void bg_enc_zero_slice(int s, uint32_t* dst) {
  constexpr int CH = (N + BG_ENC_SLICES - 1) / BG_ENC_SLICES;
  for (int i = s * CH; i < (s + 1) * CH && i < N; i++) dst[i] = 0u;
}

// the lane's slice number -> f(std::integral_constant<int, slice>): what f indexes with it is a compile-time constant
template <class F>
__device__ __forceinline__ void bg_enc_slices(F f) {
  switch (threadIdx.x / BG_ENC_RECS) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    default: f(std::integral_constant<int, 7>{}); break;
  }
}
// phase 2: the staged records [rec0, rec0 + nrec) of the call -> tile rows of N columns.  src: the workgroup's resolved sources, read only with GATHER
template <int N, bool GATHER, class CONVERT>
__device__ __forceinline__ void bg_enc_fill_tile(const uint32_t* recs32, uint32_t* tile, long long rec0, int nrec, const long long* src, CONVERT convert) {
  const int r = threadIdx.x % BG_ENC_RECS;
  if (r >= nrec) return;
  const uint8_t* const rec = reinterpret_cast<const uint8_t*>(recs32) + r * BG_ENC_REC_PITCH;
  uint32_t* const dst = tile + r * N;
  if (GATHER && src[r] < 0) bg_enc_zero_slice<N>(threadIdx.x / BG_ENC_RECS, dst);
  else bg_enc_slices([&](auto s) { convert(s, rec, rec0 + r, dst); });
}

// whether column c of the layout holds anything: FIXED's never-filled columns are +0.0 and touch neither LDS nor the table
template <int LAYOUT>
__device__ __forceinline__ bool bg_enc_filled(int c) { return LAYOUT != BG_ENC_FIXED || c < BG_ENC_PRODUCED_COLS; }
// one finished element in phase 3 (k-th column `c` of record `r` of the workgroup)
template <int LAYOUT>
__device__ __forceinline__ uint32_t bg_enc_fetch(const uint8_t* recs, const uint32_t* tile, int r, int c) {
  if (!bg_enc_filled<LAYOUT>(c)) return 0u;
  if (LAYOUT == BG_ENC_EXTRACTOR && c < BG_ENC_ONEHOT_COLS)   // the table's rule for these columns, without the table: one byte of the record's hand
    return bg_enc_onehot((int8_t)recs[r * BG_ENC_REC_PITCH + BG_ROW_HAND + BG_ENC_ONEHOT_SLOT(c)], BG_ENC_ONEHOT_CARD(c));
  return tile[r * bg_enc_dense_cols(LAYOUT) + c - bg_enc_dense_first(LAYOUT)];
}

// phase 3: rows [rec0, rec0 + nrec) of the caller's matrix from the tile (and, for EXTRACTOR, the records)
template <int LAYOUT, int DT, int ST>
__device__ __forceinline__ void bg_enc_store(const uint8_t* recs, const uint32_t* tile, long long rec0, int nrec, void* __restrict__ out, uint64_t pitch) {
  constexpr int D = bg_enc_cols(LAYOUT);
  constexpr int E = ST == BG_ENC_ST_ELEM ? 1 : DT == BG_ENC_F32 ? 4 : 8;   // elements of a 16-byte piece
  constexpr int U = (D + E - 1) / E;   // pieces of a row (BG_ENC_ST_ROWS)
  const int nunits = ST == BG_ENC_ST_ROWS ? nrec * U : (nrec * D + E - 1) / E;
  uint32_t* const o32 = reinterpret_cast<uint32_t*>(out);
  uint16_t* const o16 = reinterpret_cast<uint16_t*>(out);
  for (int u = threadIdx.x; u < nunits; u += BG_ENC_BLOCK) {
    int r, c, nvalid;
    size_t at;   // element index of the piece in `out`
    if (ST == BG_ENC_ST_ROWS) { r = u / U; c = (u - r * U) * E; nvalid = D - c < E ? D - c : E; at = (size_t)(rec0 + r) * pitch + c; }
    else if (ST == BG_ENC_ST_FLAT) { const int e0 = u * E; r = e0 / D; c = e0 - r * D; nvalid = nrec * D - e0 < E ? nrec * D - e0 : E; at = (size_t)rec0 * D + e0; }
    else { r = u / D; c = u - r * D; nvalid = 1; at = (size_t)(rec0 + r) * pitch + c; }
    uint32_t w[E];
    // a piece inside FIXED's zero columns needs no fetch; tested only where a row's run of such pieces is as long as a wave, so that whole waves skip
    // (float32 pieces and single elements: 118 / 475 per row; bfloat16 pieces are 59, the test would be pure cost)
    constexpr bool ZERO_RUN = LAYOUT == BG_ENC_FIXED && (D - BG_ENC_PRODUCED_COLS) / E >= 64;
    if (ZERO_RUN && c >= BG_ENC_PRODUCED_COLS && c + E <= D) {
#pragma unroll
      for (int k = 0; k < E; k++) w[k] = 0u;
    } else {
#pragma unroll
      for (int k = 0; k < E; k++) {
        int rk = r, ck = c + k;
        if (ST == BG_ENC_ST_FLAT && ck >= D) { ck -= D; rk++; }
        w[k] = k < nvalid && bg_enc_filled<LAYOUT>(ck) ? bg_enc_fetch<LAYOUT>(recs, tile, rk, ck) : 0u;   // one test in front of the LDS read, not two nested
      }
    }
    if (DT == BG_ENC_F32) {
      if (E == 4 && nvalid == E) *reinterpret_cast<uint4*>(o32 + at) = make_uint4(w[0], w[E > 1 ? 1 : 0], w[E > 2 ? 2 : 0], w[E > 3 ? 3 : 0]);
      else
        for (int k = 0; k < nvalid; k++) o32[at + k] = w[k];
    } else {
      if (E == 8 && nvalid == E) {
        uint32_t p[4];
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = (uint32_t)bg_enc_bf16(w[E > 1 ? 2 * k : 0]) | (uint32_t)bg_enc_bf16(w[E > 1 ? 2 * k + 1 : 0]) << 16;
        *reinterpret_cast<uint4*>(o16 + at) = make_uint4(p[0], p[1], p[2], p[3]);
      } else
        for (int k = 0; k < nvalid; k++) o16[at + k] = bg_enc_bf16(w[k]);
    }
  }
}

// the three phases for the workgroup's 32 rows of the call; GATHER: row i is record index[i] (NULL: i) of the store_rows records at `rows`
template <int LAYOUT, int DT, int ST, bool GATHER, class CONVERT>
__device__ __forceinline__ void bg_enc_body(const uint8_t* __restrict__ rows, uint64_t row_stride, long long m, void* __restrict__ out, uint64_t pitch,
                                            const int32_t* __restrict__ index, long long store_rows, CONVERT convert) {
  __shared__ __attribute__((aligned(16))) uint32_t recs32[BG_ENC_RECS * BG_ENC_REC_PITCH / 4];
  __shared__ __attribute__((aligned(16))) uint32_t tile[BG_ENC_RECS * bg_enc_dense_cols(LAYOUT)];
  __shared__ long long src[GATHER ? BG_ENC_RECS : 1];
  const long long rec0 = (long long)blockIdx.x * BG_ENC_RECS;
  const int nrec = (int)(m - rec0 < BG_ENC_RECS ? m - rec0 : BG_ENC_RECS);
  if (GATHER) bg_enc_stage_gather(rows, row_stride, index, store_rows, rec0, nrec, src, recs32);
  else bg_enc_stage<BG_ENC_BLOCK>(rows, row_stride, nrec, recs32, [rec0](int r) { return (size_t)(rec0 + r); });
  __syncthreads();
  bg_enc_fill_tile<bg_enc_dense_cols(LAYOUT), GATHER>(recs32, tile, rec0, nrec, src, convert);
  __syncthreads();
  bg_enc_store<LAYOUT, DT, ST>(reinterpret_cast<const uint8_t*>(recs32), tile, rec0, nrec, out, pitch);
}

template <int LAYOUT, int DT, int ST>
__global__ __launch_bounds__(BG_ENC_BLOCK) void bg_encode_kernel(const uint8_t* __restrict__ rows, uint64_t row_stride, long long m, void* __restrict__ out,
                                                                 uint64_t pitch) {
  bg_enc_body<LAYOUT, DT, ST, false>(rows, row_stride, m, out, pitch, nullptr, 0, BgEncConvert<LAYOUT>{});
}
// output row i from record index[i] of the store_rows records at `rows` (bg_encode_rows_ex)
template <int LAYOUT, int DT, int ST>
__global__ __launch_bounds__(BG_ENC_BLOCK) void bg_encode_gather_kernel(const uint8_t* __restrict__ rows, uint64_t row_stride, const int32_t* __restrict__ index,
                                                                        long long store_rows, long long m, void* __restrict__ out, uint64_t pitch) {
  bg_enc_body<LAYOUT, DT, ST, true>(rows, row_stride, m, out, pitch, index, store_rows, BgEncConvert<LAYOUT>{});
}

// ---- host side ----
// the store path of a call, from the alignment of the caller's matrix of D columns of es bytes.  A dense [m, 628] float32 matrix has 2 512-byte rows, so
// it is stored by rows: the <FIXED, f32, FLAT> instantiations exist for the dispatch's sake and are never launched
static inline int bg_enc_store_path(const void* out_dev, uint64_t out_stride_elems, uint64_t es, int D) {
  const bool base16 = ((uintptr_t)out_dev & 15) == 0;
  return base16 && (out_stride_elems * es) % 16 == 0 ? BG_ENC_ST_ROWS : base16 && out_stride_elems == (uint64_t)D ? BG_ENC_ST_FLAT : BG_ENC_ST_ELEM;
}
// v, one of A, B and C (C is taken for anything else), as a compile-time constant: f(std::integral_constant<int, v>)
template <int A, int B, int C, class F>
static inline void bg_enc_pick(int v, F f) {
  if (v == A) f(std::integral_constant<int, A>{});
  else if (v == B) f(std::integral_constant<int, B>{});
  else f(std::integral_constant<int, C>{});
}
// (layout, out_dtype, st) of a checked call -> launch(LAYOUT, DT, ST) as constants, for the kernel family `launch` instantiates.  LAST is the family's
// last layout: BG_ENC_EXTRACTOR, or BG_ENC_FIXED for the kernels with statistics, which have no EXTRACTOR instantiation
template <int LAST, class F>
static inline void bg_enc_dispatch(int layout, int out_dtype, int st, F launch) {
  bg_enc_pick<BG_ENC_PRODUCED, BG_ENC_FIXED, LAST>(layout, [&](auto L) {
    bg_enc_pick<BG_ENC_F32, BG_ENC_BF16, BG_ENC_BF16>(out_dtype, [&](auto T) {
      bg_enc_pick<BG_ENC_ST_ROWS, BG_ENC_ST_FLAT, BG_ENC_ST_ELEM>(st, [&](auto S) { launch(L, T, S); });
    });
  });
}
#endif  // BG_ENC_HOST
#endif
