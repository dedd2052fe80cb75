// bg_expert.h -- bg_expert_actions: a scripted expert policy over packed records, one int32 action (and one int32 `detail` word) per record.
//
// What the behaviour-cloning half (bg_episode_outcome_rows, bg_bc_loss, bg_demo_append_rows) was missing: a policy on the device that gets somewhere.
// The reference's expert_agent.py (BalatroExpertAgent) calls methods it never defines and values a hand as len(cards) * 10; its intent is kept --
// enumerate the subsets of up to five hand cards, value each, select the best card by card, PLAY_HAND; in the shop buy a joker if one can be bought,
// else leave -- with the value restated from ScoringEngine.score_hand's formula (scoring_engine.py:103-122): (base chips + card chips) * base mult.
// The rule is stateless: a pure function of ONE record, so the same call labels a finished [K, N] store of anyone's states (DAgger) and drives a
// collection loop.  All of it is integer work; tests/expert_ref.py restates it in numpy and the g++ twin (BG_EXPERT_HOST, the pattern of bg_head.h)
// and the GPU equal it action for action and detail for detail.
//
// THE RULE.  mask[a] = byte BG_ROW_ACTION_MASK + a;  ok(a) = 0 <= a < 60 and mask[a] != 0;  fallback() = the first ok a in the order 45, 46, 47, 31,
// 55, 0, then 1..59 ascending, -1 if there is none -- it sets FELLBACK (bit 13) in detail whenever it is used.  By the byte BG_ROW_PHASE:
//   2 blind select   the first ok of 45, 46, 47 (never a skip), else fallback()
//   1 shop           among the slots i in 0..9 with shop_items[i] == 3 (ItemType.JOKER) and ok(20 + i) the smallest (shop_costs[i], i) -> 20 + i;
//                    with no such slot 31 if ok, else fallback().  Never a reroll.
//   3 pack open      55 if ok, else fallback()
//   other values     fallback()
//   0 play           slot i (0..7) is LIVE if 0 <= hand[i] <= 51, UP if live and face_down_cards[i] == 0;  V = the up slots if any, else the live
//                    slots;  no live slot: fallback().  For every non-empty S within V of at most 5 slots (at most 218), cards in slot order:
//                    ht = bg_classify(cards, |S|);  L = min(max(hand_levels[ht], 1), 15);  (c, m) = bg_hand_base(ht, L);
//                    value(S) = (c + the sum of bg_card_chips) * m.   P = the S of greatest value, ties to fewer cards, then to the smaller 8-bit
//                    slot mask.   remaining = max(int64 chips_needed - int64 round_chips_scored, 0).   PLAY MODE if discards_left <= 0, or
//                    hands_left <= 1, or int64 value(P) * hands_left >= remaining, or every live slot is in P;  else DISCARD MODE with D = the
//                    first five (or fewer) slots of live \ P by (bg_card_chips, slot) ascending.   T = P and final = 0 (PLAY_HAND), or T = D and
//                    final = 1 (DISCARD).  C = the slots with selected_cards[i] != 0.  C == T: final;  else C & ~T non-empty: 2 + ctz(C & ~T)
//                    (deselect first);  else 2 + ctz(T & ~C).  That action not ok: fallback().
//   detail           bits 0-7 T, 8-11 ht of P, 12 discard mode, 13 FELLBACK, 16-31 min(value(P), 65535); 0 outside phase 0 but for FELLBACK.
// T reads nothing a card toggle changes but selected_cards, so it is the same on every step until the hand changes: at most 8 + 5 toggles lie
// between two PLAY_HAND / DISCARD actions.  value is an estimate, not the env's score: it counts every selected card and knows no joker,
// enhancement or boss effect.  The observation's hand_levels may be 0 where the engine's level is 1: the clamp is the definition.
//
// The hand's card code is the one bg_classify / bg_card_chips read (bg_device.h): (rank - 2) * 4 + suit in 0..51, -1 for an empty slot -- checked
// against tests/encode_ref.py (its one-hot takes exactly the codes 0..51 of `hand`) and tests/helpers.forced_hand_cards.  The three game functions
// are restated here behind BG_EXPERT_FN so that g++ compiles them (bg_device.h's are __device__ only); tests/test_expert_rows_host.py holds their
// text to bg_device.h's.
//
// THE KERNEL.  bg_expert_kernel<G>: G lanes per record (a power of two, 1..64), the masks 1..255 over V's cards dealt m = 1 + lane + G * j; every
// lane values its share, the argmax is a 32-bit key (value << 11 | (5 - |S|) << 8 | 255 - m: V is compacted in slot order, so the order of the
// compacted masks is the order of the slot masks) reduced by __shfl_xor within the group, and every lane of the group then decides alike; lane 0
// stores.  G = 1 is the plain walk: m is uniform over the wave, so the subset filter is a scalar branch.  bg_expert_lanes(m) picks G = 64, 8 or 1.  Per record the rank histogram increment,
// the suit bit and the chips of each card, and (c / 5, m) of the nine classifiable hand types at the record's levels, are set up once; a subset is
// eight selects and adds and the tail of bg_classify.  Each record's 22 pieces are read as 8-byte words the compiler merges; no LDS, no atomics,
// one store per output per record.  DESIGN.md section 4 has the A/B of G.
#ifndef BG_EXPERT_H
#define BG_EXPERT_H
#include <stdint.h>

#ifdef BG_EXPERT_HOST
#define BG_EXPERT_FN static inline
#define BG_EXPERT_MFN inline
#else
#define BG_EXPERT_FN __host__ __device__ __forceinline__
#define BG_EXPERT_MFN __host__ __device__ __forceinline__
#endif

#define BG_EXPERT_FELLBACK 0x2000
#define BG_EXPERT_DISCARD 0x1000
#define BG_EXPERT_BLOCK 256
// The lane group when the caller does not say, by the number of records: the measured crossovers of the three mappings (profiles/expert_rows.txt,
// DESIGN.md section 4).  One lane per record needs the fewest instructions per record but one wave walks its 255 masks alone for ~0.1 ms, so it wins
// only once the records fill the machine several times over; a wave per record has the shortest walk and the most instructions per record.
#define BG_EXPERT_WAVE_MAX 8192      /* m <= : 64 lanes per record */
#define BG_EXPERT_GROUP_MAX 131072   /* m <= : 8 lanes per record; above: 1 */

struct BgExpertOut {
  int32_t action, detail;
};
BG_EXPERT_FN int bg_expert_lanes(int64_t m) { return m <= BG_EXPERT_WAVE_MAX ? 64 : m <= BG_EXPERT_GROUP_MAX ? 8 : 1; }

// cards.py:52-60 Rank.base_chips, on a card code (bg_card_chips of bg_device.h)
BG_EXPERT_FN int bg_expert_card_chips(int code) {
  int r = (code >> 2) + 2;
  return r <= 10 ? r : (r == 14 ? 11 : 10);
}
// scoring_engine.py:27-40,87-101 get_hand_chips_mult (bg_hand_base of bg_device.h)
BG_EXPERT_FN void bg_expert_hand_base(int ht, int level, int& chips, int& mult) {
  int bc, bm;
  switch (ht) {
    case 0: bc = 5; bm = 1; break;
    case 1: bc = 10; bm = 2; break;
    case 2: bc = 20; bm = 2; break;
    case 3: bc = 30; bm = 3; break;
    case 4: bc = 30; bm = 4; break;
    case 5: bc = 35; bm = 4; break;
    case 6: bc = 40; bm = 4; break;
    case 7: bc = 60; bm = 7; break;
    case 8: bc = 100; bm = 8; break;
    case 9: bc = 120; bm = 12; break;
    case 10: bc = 140; bm = 14; break;
    default: bc = 160; bm = 16; break;
  }
  chips = bc + (level - 1) * 10;
  mult = bm + (level - 1);
}
// balatro_game.py:40-93 _classify_hand from the 4-bit-per-rank histogram and the suit set of n >= 1 cards: bg_classify of bg_device.h behind its loop
BG_EXPERT_FN int bg_expert_classify_hist(uint64_t hist, uint32_t suits, int n) {
  const uint64_t M = 0x1111111111111ull;
  const uint64_t b0 = hist & M, b1 = (hist >> 1) & M, b2 = (hist >> 2) & M, b3 = (hist >> 3) & M;
  const uint64_t ge1 = b0 | b1 | b2 | b3, ge2 = b1 | b2 | b3, ge3 = b3 | b2 | (b1 & b0), ge4 = b3 | b2, ge5 = b3 | (b2 & (b1 | b0));
  const int n2 = __builtin_popcountll(ge2), n3 = __builtin_popcountll(ge3), n4 = __builtin_popcountll(ge4), n5 = __builtin_popcountll(ge5);
  bool flush = (__builtin_popcount(suits) == 1) && n >= 5;                                    // :60
  const uint64_t run = ge1 & (ge1 >> 4) & (ge1 >> 8) & (ge1 >> 12) & (ge1 >> 16);
  const uint64_t wheel = 0x1000000001111ull;
  bool straight = run != 0ull || (ge1 & wheel) == wheel;
  if (straight && flush) return 8;
  if (n4 >= 1 && n5 == 0) return 7;              // counts[0] == 4
  if (n3 == 1 && n4 == 0 && n2 >= 2) return 6;   // counts[0] == 3 and counts[1] == 2
  if (flush) return 5;
  if (straight && n >= 5) return 4;
  if (n3 >= 1 && n4 == 0) return 3;              // counts[0] == 3
  if (n2 >= 2 && n3 == 0) return 2;              // counts[0] == 2 and counts[1] == 2
  if (n2 >= 1 && n3 == 0) return 1;              // counts[0] == 2
  return 0;
}
// bg_classify itself: `cards` = up to 8 card codes, n of them valid
BG_EXPERT_FN int bg_expert_classify(uint64_t cards, int n) {
  if (n <= 0) return 0;
  uint64_t hist = 0; // 13 nibbles
  uint32_t suits = 0;
  for (int i = 0; i < 8; i++) {
    if (i < n) {
      int c = (int)((cards >> (8 * i)) & 0xff);
      hist += 1ull << (4 * (c >> 2));
      suits |= 1u << (c & 3);
    }
  }
  return bg_expert_classify_hist(hist, suits, n);
}

// the 8-byte word of a record at a multiple of 8 (records are 16-byte aligned, their pitch a multiple of 16)
BG_EXPERT_FN uint64_t bg_expert_w(const uint8_t* r, int off) { return *reinterpret_cast<const uint64_t*>(r + off); }
// bit j = byte j of the word is non-zero
BG_EXPERT_FN uint32_t bg_expert_nz8(uint64_t w) {
  const uint64_t k = 0x7f7f7f7f7f7f7f7full;
  const uint64_t t = (((w & k) + k) | w) & ~k;                 // 0x80 in every non-zero byte
  return (uint32_t)(((t >> 7) * 0x0102040810204080ull) >> 56);   // the eight flags gathered into the top byte
}
BG_EXPERT_FN int bg_expert_i16(uint64_t w, int j) { return (int)(int16_t)(uint16_t)(w >> (16 * j)); }
BG_EXPERT_FN int bg_expert_i8(uint64_t w, int j) { return (int)(int8_t)(uint8_t)(w >> (8 * j)); }

BG_EXPERT_FN int bg_expert_fallback(uint64_t ok) {
  if ((ok >> 45) & 1) return 45;
  if ((ok >> 46) & 1) return 46;
  if ((ok >> 47) & 1) return 47;
  if ((ok >> 31) & 1) return 31;
  if ((ok >> 55) & 1) return 55;
  return ok ? __builtin_ctzll(ok) : -1;   // 0, then 1..59 ascending
}
BG_EXPERT_FN BgExpertOut bg_expert_take(uint64_t ok, int a, int detail) {
  BgExpertOut o;
  if (a >= 0 && a < 60 && ((ok >> a) & 1)) { o.action = a; o.detail = detail; }
  else { o.action = bg_expert_fallback(ok); o.detail = detail | BG_EXPERT_FELLBACK; }
  return o;
}

// What a subset's value is computed from, set up once per record: V's cards compacted in slot order
struct BgExpertHand {
  uint64_t inc[8];     // 1 << 4 * rank: the card's step in the rank histogram
  uint32_t suit[8];    // 1 << suit
  int32_t chips[8];
  int k;               // cards in V
  uint64_t cpk, mpk;   // hand type ht at the record's level: chips / 5 in bits 6 ht .. 6 ht + 5, mult in bits 5 ht .. 5 ht + 4
};
// the key of the compacted mask m: 0 where m names no subset to value
BG_EXPERT_FN uint32_t bg_expert_key(const BgExpertHand& H, uint32_t m) {
  const int n = __builtin_popcount(m);
  if (m == 0u || n > 5 || (m >> H.k) != 0u) return 0u;
  uint64_t hist = 0;
  uint32_t suits = 0;
  int chips = 0;
#ifndef BG_EXPERT_HOST
#pragma unroll
#endif
  for (int i = 0; i < 8; i++) {
    const bool in = (m >> i) & 1u;
    hist += in ? H.inc[i] : 0ull;
    suits |= in ? H.suit[i] : 0u;
    chips += in ? H.chips[i] : 0;
  }
  const int ht = bg_expert_classify_hist(hist, suits, n);
  const int c = (int)((H.cpk >> (6 * ht)) & 63u) * 5, mu = (int)((H.mpk >> (5 * ht)) & 31u);
  const uint32_t value = (uint32_t)((c + chips) * mu);   // <= (240 + 55) * 22
  return value << 11 | (uint32_t)(5 - n) << 8 | (255u - m);
}
// the plain walk: every mask in ascending order
struct BgExpertSerial {
  BG_EXPERT_MFN uint32_t operator()(const BgExpertHand& H) const {
    uint32_t best = 0u;
    const uint32_t end = 1u << H.k;
    for (uint32_t m = 1u; m < end; m++) {
      const uint32_t key = bg_expert_key(H, m);
      best = key > best ? key : best;
    }
    return best;
  }
};

// One record.  search(H) -> the greatest bg_expert_key over the masks 1..255 (BgExpertSerial, or a lane group's share and its reduction)
template <class Search>
BG_EXPERT_FN BgExpertOut bg_expert_row(const uint8_t* r, Search search) {
  // the action mask as 60 bits (bytes 176..235; 236.. are joker_ids)
  uint64_t ok = 0;
#ifndef BG_EXPERT_HOST
#pragma unroll
#endif
  for (int j = 0; j < 8; j++) ok |= (uint64_t)bg_expert_nz8(bg_expert_w(r, BG_ROW_ACTION_MASK + 8 * j)) << (8 * j);
  ok &= 0x0fffffffffffffffull;
  const int phase = bg_expert_i8(bg_expert_w(r, 336), BG_ROW_PHASE - 336);
  if (phase == 2) {
    const uint64_t blinds = (ok >> 45) & 7u;
    return bg_expert_take(ok, blinds ? 45 + __builtin_ctzll(blinds) : -1, 0);
  }
  if (phase == 3) return bg_expert_take(ok, 55, 0);
  if (phase == 1) {
    // shop_items int16[10] at 256, shop_costs int16[10] at 276: five words, the third shared
    const uint64_t w[5] = {bg_expert_w(r, 256), bg_expert_w(r, 264), bg_expert_w(r, 272), bg_expert_w(r, 280), bg_expert_w(r, 288)};
    int best = 0x7fffffff, slot = -1;
#ifndef BG_EXPERT_HOST
#pragma unroll
#endif
    for (int i = 0; i < 10; i++) {
      const int item = bg_expert_i16(w[i >> 2], i & 3), cost = bg_expert_i16(w[(i + 10) >> 2], (i + 10) & 3);
      const int key = cost * 16 + i;   // (cost, i) in one word: cost is an int16
      if (item == 3 && ((ok >> (20 + i)) & 1) && key < best) { best = key; slot = i; }
    }
    return bg_expert_take(ok, slot >= 0 ? 20 + slot : 31, 0);
  }
  if (phase != 0) return bg_expert_take(ok, -1, 0);

  // ---- play ----
  const uint64_t w304 = bg_expert_w(r, 304), w312 = bg_expert_w(r, 312), w320 = bg_expert_w(r, 320), w328 = bg_expert_w(r, 328);
  const uint64_t hand = (w304 >> 48) | (w312 << 16);                 // bytes 310..317
  const uint64_t levels_lo = (w312 >> 48) | (w320 << 16);            // hand_levels[0..7], bytes 318..325
  const int level8 = bg_expert_i8(w320, 326 - 320);
  uint32_t live = 0, down = 0, sel = 0;
#ifndef BG_EXPERT_HOST
#pragma unroll
#endif
  for (int i = 0; i < 8; i++) {
    const int c = bg_expert_i8(hand, i);
    live |= (c >= 0 && c <= 51 ? 1u : 0u) << i;
    sel |= (bg_expert_w(r, BG_ROW_SELECTED_CARDS + 8 * i) != 0ull ? 1u : 0u) << i;
    down |= (bg_expert_w(r, BG_ROW_FACE_DOWN_CARDS + 8 * i) != 0ull ? 1u : 0u) << i;
  }
  if (live == 0u) return bg_expert_take(ok, -1, 0);
  const uint32_t up = live & ~down, V = up ? up : live;

  BgExpertHand H;
  H.k = 0; H.cpk = 0; H.mpk = 0;
#ifndef BG_EXPERT_HOST
#pragma unroll
#endif
  for (int i = 0; i < 8; i++) { H.inc[i] = 0; H.suit[i] = 0; H.chips[i] = 0; }
  // compaction in slot order.  Written over the TARGET position q so that every index is a constant: q-th card of V = the slot of V's q-th set bit
  {
    uint32_t rest = V;
#ifndef BG_EXPERT_HOST
#pragma unroll
#endif
    for (int q = 0; q < 8; q++) {
      if (rest) {
        const int i = __builtin_ctz(rest);
        rest &= rest - 1u;
        const int c = (int)((hand >> (8 * i)) & 0xff);
        H.inc[q] = 1ull << (4 * (c >> 2));
        H.suit[q] = 1u << (c & 3);
        H.chips[q] = bg_expert_card_chips(c);
        H.k = q + 1;
      }
    }
  }
#ifndef BG_EXPERT_HOST
#pragma unroll
#endif
  for (int ht = 0; ht < 9; ht++) {
    int L = ht < 8 ? bg_expert_i8(levels_lo, ht) : level8;
    L = L < 1 ? 1 : L > 15 ? 15 : L;
    int c, mu;
    bg_expert_hand_base(ht, L, c, mu);
    H.cpk |= (uint64_t)(c / 5) << (6 * ht);
    H.mpk |= (uint64_t)mu << (5 * ht);
  }

  const uint32_t key = search(H);
  const uint32_t pm = 255u - (key & 255u);   // P over the compacted cards
  const int64_t value = (int64_t)(key >> 11);
  // back to slots, with the hand type of P
  uint32_t P = 0;
  uint64_t hist = 0;
  uint32_t suits = 0;
  {
    uint32_t rest = V;
#ifndef BG_EXPERT_HOST
#pragma unroll
#endif
    for (int q = 0; q < 8; q++) {
      if (rest) {
        const int i = __builtin_ctz(rest);
        rest &= rest - 1u;
        if ((pm >> q) & 1u) { P |= 1u << i; hist += H.inc[q]; suits |= H.suit[q]; }
      }
    }
  }
  const int ht = bg_expert_classify_hist(hist, suits, __builtin_popcount(P));

  const int64_t round_chips = (int64_t)(int32_t)(uint32_t)bg_expert_w(r, 144), needed = (int64_t)(int32_t)(uint32_t)(bg_expert_w(r, 152) >> 32);
  const int64_t remaining = needed - round_chips > 0 ? needed - round_chips : 0;
  const int hands_left = bg_expert_i8(w328, BG_ROW_HANDS_LEFT - 328), discards_left = bg_expert_i8(w328, BG_ROW_DISCARDS_LEFT - 328);
  const bool play = discards_left <= 0 || hands_left <= 1 || value * (int64_t)hands_left >= remaining || (live & ~P) == 0u;
  uint32_t T = P;
  if (!play) {
    // the five cheapest of live \ P by (chips, slot): five times the smallest (chips << 3 | slot) left
    uint32_t rest = live & ~P;
    T = 0;
    for (int t = 0; t < 5 && rest; t++) {
      int bestk = 0x7fffffff;
#ifndef BG_EXPERT_HOST
#pragma unroll
#endif
      for (int i = 0; i < 8; i++) {
        const int kk = bg_expert_card_chips((int)((hand >> (8 * i)) & 0xff)) << 3 | i;
        if (((rest >> i) & 1u) && kk < bestk) bestk = kk;
      }
      T |= 1u << (bestk & 7);
      rest &= ~(1u << (bestk & 7));
    }
  }
  const int final_action = play ? 0 : 1;
  const int detail = (int)(T | (uint32_t)ht << 8 | (play ? 0u : (uint32_t)BG_EXPERT_DISCARD) | (uint32_t)(value > 65535 ? 65535 : value) << 16);
  const uint32_t off = sel & ~T, on = T & ~sel;
  const int a = sel == T ? final_action : off ? 2 + __builtin_ctz(off) : 2 + __builtin_ctz(on);
  return bg_expert_take(ok, a, detail);
}

#ifdef BG_EXPERT_HOST
// the serial twin of the launch
static inline void bg_expert_actions_host(const uint8_t* rows, uint64_t stride, int64_t m, const int32_t* index, int64_t store_rows, int32_t* actions,
                                          int32_t* detail) {
  for (int64_t i = 0; i < m; i++) {
    const int64_t src = index ? (int64_t)index[i] : i;
    BgExpertOut o = {-1, 0};
    if (src >= 0 && src < store_rows) o = bg_expert_row(rows + (uint64_t)src * stride, BgExpertSerial{});
    actions[i] = o.action;
    if (detail) detail[i] = o.detail;
  }
}
#else
// a lane group's share of the masks, and the greatest key of the group
template <int G>
struct BgExpertGroup {
  uint32_t g;   // the lane within its group
  __device__ __forceinline__ uint32_t operator()(const BgExpertHand& H) const {
    uint32_t best = 0u;
    const uint32_t end = 1u << H.k;
#pragma unroll 1
    for (uint32_t m0 = 1u; m0 < end; m0 += G) {
      const uint32_t key = bg_expert_key(H, m0 + g);
      best = key > best ? key : best;
    }
#pragma unroll
    for (int d = G / 2; d >= 1; d >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)best, d);
      best = o > best ? o : best;
    }
    return best;
  }
};

// G lanes per record; records [0, m) in order, or the records index_dev names (outside [0, store_rows): action -1, detail 0)
template <int G, bool DETAIL>
__global__ __launch_bounds__(BG_EXPERT_BLOCK) void bg_expert_kernel(const uint8_t* __restrict__ rows, uint64_t stride, long long m,
                                                                    const int32_t* __restrict__ index, long long store_rows,
                                                                    int32_t* __restrict__ actions, int32_t* __restrict__ detail) {
  static_assert(G >= 1 && G <= 64 && (G & (G - 1)) == 0, "a lane group is a power of two within one wave");
  const long long i = ((long long)blockIdx.x * BG_EXPERT_BLOCK + threadIdx.x) / G;
  if (i >= m) return;   // (a whole group leaves together: BG_EXPERT_BLOCK is a multiple of G)
  const long long src = index ? (long long)index[i] : i;
  BgExpertOut o = {-1, 0};
  if (src >= 0 && src < store_rows) {
    const uint8_t* r = (const uint8_t*)__builtin_assume_aligned(rows + (uint64_t)src * stride, 16);
    if (G == 1) o = bg_expert_row(r, BgExpertSerial{});
    else o = bg_expert_row(r, BgExpertGroup<G>{(uint32_t)threadIdx.x & (G - 1)});
  }
  if ((threadIdx.x & (G - 1)) == 0) {
    actions[i] = o.action;
    if (DETAIL) detail[i] = o.detail;
  }
}
#endif
#endif
