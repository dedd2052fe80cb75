"""The numpy / plain-Python restatement of bg_expert_actions' rule (csrc/bg_expert.h; include/balatro_mi355x.h has the contract), written from the rule's
text and from the reference's `_classify_hand` (balatro_game.py:40-93) and `get_hand_chips_mult` (scoring_engine.py:27-40,87-101) -- not from the kernel:
the classifier below counts ranks and suits in dictionaries as the reference does, the subsets come from itertools.combinations, the tie-break is a
tuple comparison.  Python integers do not overflow, which is the rule's "int64 where stated".

`expert_one(rec)` takes one observation (key -> value, the env's keys) and returns (action, detail); `expert_obs(obs)` runs it over key -> [m, ...]
arrays; `expert_rows(rows, index=)` over packed records (unpacked through encode_ref.unpack_records), an index outside [0, len(rows)) giving (-1, 0).
`synthetic_obs()` is the set of hand-made observations both test files run: every case the issue lists, by name, plus seeded random ones."""
from __future__ import annotations

import functools
import itertools
import random

import numpy as np

from tests.helpers import OBS_KEYS, forced_hand_cards

FELLBACK, DISCARD_MODE = 1 << 13, 1 << 12
FALLBACK_ORDER = [45, 46, 47, 31, 55, 0] + list(range(1, 60))
BASE = {0: (5, 1), 1: (10, 2), 2: (20, 2), 3: (30, 3), 4: (30, 4), 5: (35, 4), 6: (40, 4), 7: (60, 7), 8: (100, 8)}   # BASE_HAND_VALUES, by HandType value
OBS_SHAPES = {"hand": (8,), "selected_cards": (8,), "joker_ids": (10,), "consumables": (5,), "shop_items": (10,), "shop_costs": (10,),
              "hand_levels": (12,), "action_mask": (60,), "face_down_cards": (8,)}


def card_chips(code):
    """cards.py:52-60 Rank.base_chips: 2..10 their number, J Q K 10, A 11.  code = (rank - 2) * 4 + suit."""
    rank = code // 4 + 2
    return rank if rank <= 10 else 11 if rank == 14 else 10


def classify(codes):
    """balatro_game.py:40-93 _classify_hand over card codes, literally."""
    if not codes:
        return 0
    rank_counts, suit_counts, ranks = {}, {}, []
    for c in codes:
        rank, suit = c // 4 + 2, c % 4
        rank_counts[rank] = rank_counts.get(rank, 0) + 1
        suit_counts[suit] = suit_counts.get(suit, 0) + 1
        ranks.append(rank)
    counts = sorted(rank_counts.values(), reverse=True)
    is_flush = len(suit_counts) == 1 and len(codes) >= 5
    sorted_ranks = sorted(set(ranks))
    is_straight = False
    if len(sorted_ranks) >= 5:
        for i in range(len(sorted_ranks) - 4):
            if sorted_ranks[i + 4] - sorted_ranks[i] == 4:
                is_straight = True
                break
        if not is_straight and 14 in sorted_ranks and {2, 3, 4, 5}.issubset(set(sorted_ranks)):
            is_straight = True
    if is_straight and is_flush and len(codes) >= 5:
        return 8
    if counts[0] == 4:
        return 7
    if len(counts) >= 2 and counts[0] == 3 and counts[1] == 2:
        return 6
    if is_flush and len(codes) >= 5:
        return 5
    if is_straight and len(codes) >= 5:
        return 4
    if counts[0] == 3:
        return 3
    if len(counts) >= 2 and counts[0] == 2 and counts[1] == 2:
        return 2
    if counts[0] == 2:
        return 1
    return 0


def subset_value(codes, levels):
    """(value, hand type) of the cards `codes` (in slot order) at the observation's hand_levels."""
    ht = classify(list(codes))
    L = min(max(int(levels[ht]), 1), 15)
    bc, bm = BASE[ht]
    c, m = bc + (L - 1) * 10, bm + (L - 1)
    return (c + sum(card_chips(x) for x in codes)) * m, ht


@functools.lru_cache(maxsize=1 << 16)
def _subsets(slots, codes, levels):
    """Every non-empty subset of at most five of `slots` -> [(value, size, slot mask, hand type)]."""
    out = []
    for n in range(1, min(5, len(slots)) + 1):
        for pick in itertools.combinations(range(len(slots)), n):
            v, ht = subset_value(tuple(codes[j] for j in pick), levels)
            out.append((v, n, sum(1 << slots[j] for j in pick), ht))
    return out


def subsets(rec):
    """The valued subsets of an observation in the play phase ([] with no live slot)."""
    hand = [int(x) for x in rec["hand"]]
    live = [i for i in range(8) if 0 <= hand[i] <= 51]
    up = [i for i in live if int(rec["face_down_cards"][i]) == 0]
    V = up if up else live
    return _subsets(tuple(V), tuple(hand[i] for i in V), tuple(int(x) for x in rec["hand_levels"])) if V else []


def expert_one(rec):
    mask = [int(x) != 0 for x in rec["action_mask"]]

    def ok(a):
        return 0 <= a < 60 and mask[a]

    def fallback(detail):
        for a in FALLBACK_ORDER:
            if ok(a):
                return a, detail | FELLBACK
        return -1, detail | FELLBACK

    def take(a, detail=0):
        return (a, detail) if a is not None and ok(a) else fallback(detail)

    phase = int(rec["phase"])
    if phase == 2:
        return take(next((a for a in (45, 46, 47) if ok(a)), None))
    if phase == 1:
        cands = [(int(rec["shop_costs"][i]), i) for i in range(10) if int(rec["shop_items"][i]) == 3 and ok(20 + i)]
        return take(20 + min(cands)[1] if cands else 31)
    if phase == 3:
        return take(55)
    if phase != 0:
        return fallback(0)
    hand = [int(x) for x in rec["hand"]]
    live = [i for i in range(8) if 0 <= hand[i] <= 51]
    if not live:
        return fallback(0)
    value, _, P, ht = max(subsets(rec), key=lambda s: (s[0], -s[1], -s[2]))
    live_mask = sum(1 << i for i in live)
    remaining = max(int(rec["chips_needed"]) - int(rec["round_chips_scored"]), 0)
    hands_left, discards_left = int(rec["hands_left"]), int(rec["discards_left"])
    play = discards_left <= 0 or hands_left <= 1 or value * hands_left >= remaining or (live_mask & ~P) == 0
    if play:
        T, final = P, 0
    else:
        rest = sorted((i for i in live if not (P >> i) & 1), key=lambda i: (card_chips(hand[i]), i))
        T, final = sum(1 << i for i in rest[:5]), 1
    detail = T | ht << 8 | (0 if play else DISCARD_MODE) | min(value, 65535) << 16
    C = sum(1 << i for i in range(8) if int(rec["selected_cards"][i]) != 0)
    if C == T:
        a = final
    elif C & ~T:
        a = 2 + ((C & ~T) & -(C & ~T)).bit_length() - 1
    else:
        a = 2 + ((T & ~C) & -(T & ~C)).bit_length() - 1
    a, detail = take(a, detail)
    return a, detail - (1 << 32) if detail >= 1 << 31 else detail


def expert_obs(obs):
    m = len(obs["hand"])
    out = [expert_one({k: obs[k][i] for k in ("hand", "face_down_cards", "selected_cards", "hand_levels", "action_mask", "phase", "shop_items", "shop_costs",
                                              "chips_needed", "round_chips_scored", "hands_left", "discards_left")}) for i in range(m)]
    return np.array([o[0] for o in out], np.int32).reshape(m), np.array([o[1] for o in out], np.int32).reshape(m)


def expert_rows(rows, index=None):
    """rows uint8 [n, stride] -> (actions int32, detail int32) per record, or per entry of `index`."""
    from tests import encode_ref
    rows = np.ascontiguousarray(rows)
    a, d = expert_obs(encode_ref.unpack_records(rows))
    if index is None:
        return a, d
    index = np.asarray(index, np.int64)
    inside = (index >= 0) & (index < len(rows))
    safe = np.where(inside, index, 0)
    return np.where(inside, a[safe], -1).astype(np.int32), np.where(inside, d[safe], 0).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- the synthetic set
def _code(rank, suit):
    return (rank - 2) * 4 + suit


def _base(**kw):
    """One observation the env could show in the play phase: eight cards of no pattern, every play-phase action valid."""
    rec = {k: np.zeros(OBS_SHAPES.get(k, ()), np.int64) for k in OBS_KEYS}
    rec["hand"] = np.array([_code(2, 0), _code(5, 1), _code(7, 2), _code(9, 3), _code(11, 0), _code(13, 1), _code(4, 2), _code(14, 3)], np.int64)
    rec["hand_levels"] = np.ones(12, np.int64)
    rec["action_mask"][0:10] = 1
    rec["hands_left"], rec["discards_left"] = np.int64(4), np.int64(3)
    rec["chips_needed"] = np.int64(300)
    rec["hand_size"] = np.int64(8)
    for k, v in kw.items():
        rec[k] = np.asarray(v, np.int64)
    return rec


def _best(rec):
    return max(subsets(rec), key=lambda s: (s[0], -s[1], -s[2]))


def _tied(rec):
    """The sizes of the subsets that reach the greatest value, ascending."""
    ss = subsets(rec)
    top = max(s[0] for s in ss)
    return sorted(s[1] for s in ss if s[0] == top)


def _find_ties(rr, same_size, want=3):
    """Small hands and levels whose greatest value is reached by subsets of equal size / of different sizes, found with the restatement's own
    enumeration (seeded), so that each tie-break rule decides at least one action of the set.  Different sizes need levels: with a pair (r, r) and a
    kicker k, high card {r, k} at level L0 against the pair {r, r, k} at level L1 -- e.g. r = 5, k = 2, L0 = 3, L1 = 2: both 96.  Equal sizes: a bare
    pair (r, r) whose high-card level makes one card worth more than the pair -- the two single cards tie."""
    out = []
    combos = [(r, k, L0, L1) for r in range(2, 15) for k in range(2, 15) if k != r for L0 in range(1, 16) for L1 in range(1, 16)]
    rr.shuffle(combos)
    for r, k, L0, L1 in combos:
        hand = [-1] * 8
        slots = rr.sample(range(8), 3)
        suits = rr.sample(range(4), 2)
        hand[slots[0]], hand[slots[1]], hand[slots[2]] = _code(r, suits[0]), _code(r, suits[1]), _code(k, rr.randrange(4))
        levels = [1] * 12
        levels[0], levels[1] = L0, L1
        if same_size:
            hand[slots[2]] = -1   # a bare pair whose single cards are worth more than the pair: the two singles tie
        rec = _base(hand=hand, hand_levels=levels)
        sizes = _tied(rec)
        if len(sizes) >= 2 and ((sizes[0] == sizes[-1]) if same_size else (sizes[0] != sizes[-1])):
            out.append(rec)
            if len(out) == want:
                return out
    raise AssertionError("no tie found")


def synthetic_cases():
    """[(name, observation)]: the issue's list, by name."""
    rr = random.Random(20251021)
    cases = []

    def add(name, rec):
        cases.append((name, rec))

    # every phase
    for j, valid in enumerate(([45, 46, 47, 48], [46, 47, 49], [47], [48, 49, 31], [])):
        m = np.zeros(60, np.int64); m[valid] = 1
        add(f"phase2_{j}", _base(phase=2, action_mask=m))
    items = [3, 1, 3, 2, 3, 0, 3, 4, 3, 3]
    costs = [6, 1, 4, 2, 4, 0, 9, 3, 5, 2]
    full = np.zeros(60, np.int64); full[20:32] = 1
    add("shop_cheapest_joker", _base(phase=1, shop_items=items, shop_costs=costs, action_mask=full))
    m = full.copy(); m[29] = 0
    add("shop_cheapest_masked_tie_to_lower_slot", _base(phase=1, shop_items=items, shop_costs=costs, action_mask=m))
    m = full.copy(); m[[20, 22, 24, 26, 28, 29]] = 0
    add("shop_every_joker_masked", _base(phase=1, shop_items=items, shop_costs=costs, action_mask=m))
    add("shop_no_joker", _base(phase=1, shop_items=[1, 2, 4, 0, 0, 1, 2, 4, 0, 0], shop_costs=costs, action_mask=full))
    m = full.copy(); m[31] = 0
    add("shop_no_joker_31_masked", _base(phase=1, shop_items=[1, 2, 4, 0, 0, 1, 2, 4, 0, 0], shop_costs=costs, action_mask=m))
    add("shop_negative_cost", _base(phase=1, shop_items=items, shop_costs=[6, 1, 4, 2, -4, 0, 9, 3, 5, 2], action_mask=full))
    m = np.zeros(60, np.int64); m[[55, 56]] = 1
    add("pack_55", _base(phase=3, action_mask=m))
    m = np.zeros(60, np.int64); m[[56, 12]] = 1
    add("pack_55_masked", _base(phase=3, action_mask=m))
    for ph in (4, 5, -1, 100, -128, 127):
        m = np.zeros(60, np.int64); m[[0, 17]] = 1
        add(f"phase_other_{ph}", _base(phase=ph, action_mask=m))
    # hands of 0, 1, 4, 5 and 8 live cards with -1 holes in the middle (and codes above 51, which are no cards)
    base_hand = _base()["hand"]
    for live in ([], [3], [0, 2, 5, 7], [1, 2, 4, 6, 7], list(range(8))):
        hand = np.full(8, -1, np.int64)
        hand[live] = base_hand[live]
        add(f"live_{len(live)}", _base(hand=hand))
        add(f"live_{len(live)}_selected", _base(hand=hand, selected_cards=[1, 0, 1, 0, 0, 0, 0, 1]))
    add("codes_above_51", _base(hand=[52, 3, 127, 17, -128, 30, 64, 51]))
    # face-down cards
    add("all_face_down", _base(face_down_cards=[1] * 8))
    add("mixed_face_down", _base(face_down_cards=[0, 1, 0, 0, 7, 0, -1, 0]))
    add("mixed_face_down_pair_hidden", _base(hand=[_code(14, 0), _code(14, 1), _code(3, 2), _code(6, 3), _code(8, 0), _code(10, 1), -1, -1], face_down_cards=[1, 0, 0, 0, 0, 0, 0, 0]))
    add("face_down_on_an_empty_slot", _base(hand=[_code(14, 0), -1, _code(3, 2), -1, _code(8, 0), _code(10, 1), -1, -1], face_down_cards=[0, 1, 0, 1, 0, 0, 1, 1]))
    # the nine classifiable hand types, forced
    for ht in range(9):
        for rep in range(3):
            cards = forced_hand_cards(ht, rr)
            rest = [c for c in range(52) if c not in cards]
            hand = np.full(8, -1, np.int64)
            slots = sorted(rr.sample(range(8), len(cards)))
            hand[slots] = cards
            if rep:   # fill the other slots
                for s in range(8):
                    if hand[s] < 0:
                        hand[s] = rest.pop(rr.randrange(len(rest)))
            add(f"forced_ht{ht}_{rep}", _base(hand=hand, discards_left=rep % 2 * 2))
    # levels
    for L in (0, 1, 15, 16, -3, 127):
        add(f"level_{L}", _base(hand_levels=[L] * 12, hand=[_code(9, 0), _code(9, 1), _code(4, 2), _code(4, 3), _code(12, 0), _code(13, 1), _code(2, 2), _code(6, 3)]))
    add("levels_mixed", _base(hand_levels=[15, 0, 1, 16, 2, 3, 4, 5, 6, 7, 8, 9]))
    # value ties
    add("two_pair_of_equal_chips", _base(hand=[_code(13, 0), _code(13, 1), _code(12, 0), _code(12, 1), -1, -1, -1, -1]))
    for j, rec in enumerate(_find_ties(rr, True)):
        add(f"tie_equal_size_{j}", rec)
    for j, rec in enumerate(_find_ties(rr, False)):
        add(f"tie_different_size_{j}", rec)
    # remaining against value * hands_left
    b = _base()
    v = _best(b)[0]
    for delta in (-1, 0, 1):
        add(f"remaining_{delta:+d}", _base(hands_left=3, chips_needed=3 * v + delta + 50, round_chips_scored=50))
    add("needed_below_scored", _base(chips_needed=100, round_chips_scored=5000))
    add("needed_int32_extremes", _base(chips_needed=2 ** 31 - 1, round_chips_scored=-2 ** 31))
    add("no_discards", _base(discards_left=0, chips_needed=10 ** 6))
    add("negative_discards", _base(discards_left=-1, chips_needed=10 ** 6))
    add("last_hand", _base(hands_left=1, chips_needed=10 ** 6))
    add("discard_mode", _base(chips_needed=10 ** 6))
    add("discard_mode_negative_hands", _base(hands_left=-5, chips_needed=10 ** 6))
    add("discard_fewer_than_five_left", _base(hand=[_code(9, 0), _code(9, 1), _code(9, 2), _code(9, 3), _code(14, 0), _code(2, 1), _code(3, 1), -1], chips_needed=10 ** 6))
    add("discard_five_of_six", _base(hand=[_code(2, 0), _code(2, 1), _code(2, 2), _code(2, 3), _code(3, 0), _code(3, 1), _code(3, 2), _code(3, 3)],
                                     hand_levels=[15] + [1] * 11, chips_needed=10 ** 6))
    add("every_live_card_in_P", _base(hand=[_code(9, 0), -1, _code(9, 2), -1, _code(14, 0), -1, -1, -1], chips_needed=10 ** 6))
    # the mask
    add("all_zero_mask", _base(action_mask=np.zeros(60, np.int64)))
    add("all_zero_mask_shop", _base(phase=1, action_mask=np.zeros(60, np.int64)))
    T = _best(b)[2]
    first = (T & -T).bit_length() - 1
    m = b["action_mask"].copy(); m[2 + first] = 0
    add("intended_toggle_masked", _base(action_mask=m, chips_needed=0))
    sel = [(T >> i) & 1 for i in range(8)]
    m = b["action_mask"].copy(); m[0] = 0
    add("play_masked_when_selected", _base(selected_cards=sel, action_mask=m, chips_needed=0))
    add("play_when_selected", _base(selected_cards=sel, chips_needed=0))
    m = np.zeros(60, np.int64); m[[59]] = 1
    add("only_59_valid", _base(action_mask=m))
    m = np.ones(60, np.int64) * -1
    add("mask_of_minus_ones", _base(action_mask=m))
    # stale selections
    stale = [1 - s for s in sel]
    add("stale_selection_outside_T", _base(selected_cards=stale, chips_needed=0))
    add("stale_and_wanted_selection", _base(selected_cards=[1] * 8, chips_needed=0))
    add("selection_on_an_empty_slot", _base(hand=[_code(9, 0), -1, _code(9, 2), -1, _code(14, 0), -1, -1, -1], selected_cards=[1, 1, 0, 0, 0, 0, 0, 2 ** 40]))
    add("discard_mode_stale", _base(chips_needed=10 ** 6, selected_cards=sel))
    return cases


def random_obs(n, seed):
    """n seeded random observations over the fields the rule reads (and zeros elsewhere): phases 0..4, hands from -1..53, any selection, thin masks."""
    rng = np.random.default_rng(seed)
    obs = {k: np.zeros((n,) + OBS_SHAPES.get(k, ()), np.int64) for k in OBS_KEYS}
    obs["phase"] = rng.choice([0, 0, 0, 0, 1, 2, 3, 4], n)
    obs["hand"] = rng.integers(-1, 54, (n, 8))
    obs["hand"][rng.random((n, 8)) < 0.15] = -1
    obs["selected_cards"] = (rng.random((n, 8)) < 0.3).astype(np.int64)
    obs["face_down_cards"] = (rng.random((n, 8)) < 0.15).astype(np.int64)
    obs["hand_levels"] = rng.integers(0, 6, (n, 12))
    obs["action_mask"] = (rng.random((n, 60)) < rng.choice([0.05, 0.5, 0.95], (n, 1))).astype(np.int64)
    obs["shop_items"] = rng.integers(0, 5, (n, 10))
    obs["shop_costs"] = rng.integers(0, 12, (n, 10))
    obs["chips_needed"] = rng.choice([0, 100, 300, 800, 5000], n)
    obs["round_chips_scored"] = rng.integers(0, 400, n)
    obs["hands_left"] = rng.integers(0, 5, n)
    obs["discards_left"] = rng.integers(0, 4, n)
    return obs


_synthetic_cache = {}


def synthetic_obs(n_random=400):
    """(names, key -> [m, ...] arrays): the named cases, then n_random random ones."""
    if n_random not in _synthetic_cache:
        cases = synthetic_cases()
        rnd = random_obs(n_random, 77)
        obs = {k: np.concatenate([np.stack([np.asarray(c[1][k], np.int64) for c in cases]), rnd[k]]) for k in OBS_KEYS}
        _synthetic_cache[n_random] = ([c[0] for c in cases] + [f"random_{i}" for i in range(n_random)], obs)
    return _synthetic_cache[n_random]


def synthetic_rows(stride, n_random=400):
    """(names, uint8 [m, stride] records, (actions, detail) of the restatement on the observations they were packed from)."""
    from tests import encode_ref
    key = ("rows", stride, n_random)
    if key not in _synthetic_cache:
        names, obs = synthetic_obs(n_random)
        _synthetic_cache[key] = (names, encode_ref.pack_records(obs, stride).copy(), expert_obs(obs))
    return _synthetic_cache[key]
