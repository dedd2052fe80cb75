"""GPU parity tests of the OPERATOR-level entry points (run with -m gpu): the units the reference exposes as callables of
their own -- BalatroGame._classify_hand, UnifiedScorer.score_hand, BalatroSimulator.evaluate_hand / calculate_score -- batched
through the C ABI, against the golden vectors generated from the Python reference (tests/golden/, oracle/gen_golden.py).
These are the same device functions the step path runs, so hand types and joker combinations a random env almost never
reaches (STRAIGHT_FLUSH, FLUSH, FOUR_KIND ...) get their GPU evidence here.  Everything is bit-exact (tolerance 0).
"""
import json
import os
import random
import zlib
from itertools import combinations

import numpy as np
import pytest

from tests.helpers import GOLD, POISON, assert_step_outputs, forced_deck, forced_hand_script, poison_env_outputs

pytestmark = pytest.mark.gpu

# BG_TEST_SEED_OFFSET=<k> moves every oracle-compared test below to other games (a soak runs the suite under several offsets)
SEED_OFFSET = int(os.environ.get("BG_TEST_SEED_OFFSET", "0"))


LANES = pytest.mark.parametrize("lanes", [1, 8], ids=["lane_per_case", "8_lanes_per_case"])


@LANES
def test_classify_batch_golden(lanes):
    """All 20 000 rows of classify.npz (random 1..8-card subsets) through bg_classify_batch, in both lane mappings."""
    import torch
    from balatro_gym_amd import classify_batch
    g = np.load(os.path.join(GOLD, "classify.npz"))
    dev = torch.device("cuda:0")
    got = classify_batch(torch.from_numpy(g["cards"]).to(dev), torch.from_numpy(g["n"]).to(dev), lanes_per_case=lanes).cpu().numpy()
    bad = np.nonzero(got != g["hand_type"])[0]
    assert bad.size == 0, f"row {bad[0]}: cards {g['cards'][bad[0]][:g['n'][bad[0]]]} got {got[bad[0]]} want {g['hand_type'][bad[0]]}"
    counts = np.bincount(g["hand_type"], minlength=9)
    assert (counts[:8] > 0).all()  # hand types 0..7 occur among the random subsets (straight flushes: the C(52,5) sweep below)


@LANES
def test_classify_batch_all_five_card_hands(lanes):
    """Every one of the C(52,5) = 2 598 960 five-card hands in lexicographic order: per-type counts and the CRC32 of the type
    sequence as the reference produced them (tests/golden/classify.npz all5_*)."""
    import torch
    from balatro_gym_amd import classify_batch
    g = np.load(os.path.join(GOLD, "classify.npz"))
    combos = np.fromiter((c for combo in combinations(range(52), 5) for c in combo), dtype=np.uint8, count=2598960 * 5).reshape(-1, 5)
    cards = np.zeros((combos.shape[0], 8), np.uint8)
    cards[:, :5] = combos
    dev = torch.device("cuda:0")
    n = torch.full((cards.shape[0],), 5, dtype=torch.uint8, device=dev)
    got = classify_batch(torch.from_numpy(cards).to(dev), n, lanes_per_case=lanes).cpu().numpy()
    assert np.bincount(got, minlength=12).tolist() == g["all5_counts"].tolist()
    assert zlib.crc32(got.tobytes()) == int(g["all5_crc32"])


def _score_cases(fixture="score_hand.json"):
    cases = json.load(open(os.path.join(GOLD, fixture)))
    rec = np.zeros((len(cases), 40), np.int32)
    for i, c in enumerate(cases):
        for k, (rank, suit, chips) in enumerate(c["cards"]):
            rec[i, 3 * k:3 * k + 3] = (rank, suit, chips)
        rec[i, 24], rec[i, 25], rec[i, 26], rec[i, 27], rec[i, 28] = len(c["cards"]), c["nscoring"], c["hand_type"], c["style"], c["level"]
        rec[i, 29] = len(c["jokers"])
        rec[i, 30:30 + len(c["jokers"])] = c["jokers"]
        rec[i, 35], rec[i, 36], rec[i, 37] = c["hands_left"], c["discards_left"], c["deck_len"]
        rec[i, 38] = np.uint32(c["gseed"]).astype(np.int32)
    return cases, rec


@LANES
def test_score_hand_batch_repeated_jokers(lanes):
    """1 000 reference cases whose joker lists hold an id more than once (Ankh's copies): two or three Bloodstones and 8 Balls each
    draw per card, so their RNG words sit at offsets that depend on every other copy."""
    import torch
    from balatro_gym_amd import score_hand_batch
    cases, rec = _score_cases("score_hand_dups.json")
    out = score_hand_batch(torch.from_numpy(rec).to("cuda:0"), lanes_per_case=lanes).cpu().numpy()
    for i, c in enumerate(cases):
        ctx = f"case {i}: {c} -> {out[i].tolist()}"
        assert out[i, 0] == c["score"] and out[i, 1] == c["chips"] and out[i, 2] == c["mult"], ctx
        assert float(out[i, 3:4].view(np.float64)[0]).hex() == c["x_mult"], ctx
        assert out[i, 4] == c["money"] and out[i, 6] == c["probe"], ctx
    assert sum(len(set(c["jokers"])) < len(c["jokers"]) for c in cases) > 300


@LANES
def test_score_hand_batch_golden(lanes):
    """All 3 000 UnifiedScorer.score_hand cases (joker name lists of 0..5 from all 150 ids, both hand-name styles, scoring
    subsets, STONE cards, levels 1..15): score, final chips / mult / x_mult bits, money, and the position of the global
    stream afterwards (the next getrandbits(32) equals the reference's probe, i.e. exactly as many draws were consumed)."""
    import torch
    from balatro_gym_amd import score_hand_batch
    cases, rec = _score_cases()
    out = score_hand_batch(torch.from_numpy(rec).to("cuda:0"), lanes_per_case=lanes).cpu().numpy()
    for i, c in enumerate(cases):
        ctx = f"case {i}: {c} -> {out[i].tolist()}"
        assert out[i, 0] == c["score"], ctx
        assert out[i, 1] == c["chips"] and out[i, 2] == c["mult"], ctx
        assert float(out[i, 3:4].view(np.float64)[0]).hex() == c["x_mult"], ctx
        assert out[i, 4] == c["money"], ctx
        assert out[i, 6] == c["probe"], ctx
    assert len({c["hand_type"] for c in cases}) == 12 and any(c["style"] for c in cases)


def test_score_hand_batch_vs_oracle_fresh_cases():
    """20 000 fresh random cases (denser in jokers and in the hand types of the joker conditions than the fixture) against
    the CPU oracle's bo_score_hand, incl. the number of words drawn."""
    import torch
    from balatro_gym_amd import score_hand_batch
    from oracle import pyoracle as po
    r = random.Random(2025)
    M = 20000
    rec = np.zeros((M, 40), np.int32)
    want = []
    for i in range(M):
        ncards = r.randint(1, 8)
        cards = []
        for _ in range(ncards):
            rank, suit = r.randint(2, 14), r.randrange(4)
            chips = 11 if rank == 14 else min(rank, 10)
            if r.random() < 0.08:
                rank, suit, chips = 0, 4, chips + 50
            elif r.random() < 0.2:
                chips += r.choice([30, 50, 80])
            cards.append((rank, suit, chips))
        nsc = ncards if r.random() < 0.6 else r.randint(1, ncards)
        style, ht, level = r.randrange(2), r.choice([0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 7, 8, 9, 10, 11]), r.choice([1, 1, 2, 7, 15])
        jokers = [r.choice([117, 26, 147, 116, 1, 31, 27]) for _ in range(r.randint(2, 5))] if r.random() < 0.15 else \
            r.sample(range(1, 151), r.randint(1, 5)) if r.random() < 0.3 else \
            r.sample([1, 136, 27, 38, 61, 16, 34, 108, 23, 22, 53, 97, 50, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 131, 132, 133,
                      134, 135, 48, 128, 122, 72, 140, 31, 39, 40, 41, 101, 124, 26, 33, 104, 147, 118, 119, 116, 117], r.randint(1, 5))
        hl, dl, deck_len, gseed = r.randint(1, 4), r.randint(0, 3), r.choice([52, 52, 40, 47, 60]), r.randrange(2 ** 32)
        for k, cd in enumerate(cards):
            rec[i, 3 * k:3 * k + 3] = cd
        rec[i, 24:29] = (ncards, nsc, ht, style, level)
        rec[i, 29] = len(jokers)
        rec[i, 30:30 + len(jokers)] = jokers
        rec[i, 35:38] = (hl, dl, deck_len)
        rec[i, 38] = np.uint32(gseed).astype(np.int32)
        o = po.score_hand(cards, cards[:nsc], ht, style, level, jokers, hl, dl, deck_len, gseed)
        want.append((o.score, o.chips, o.mult, np.float64(o.x_mult).view(np.int64), o.money, o.draws))
    want = np.array(want, dtype=np.int64)
    for lanes in (1, 8):  # lane = case, and 8 lanes per case (shuffle reductions)
        out = score_hand_batch(torch.from_numpy(rec).to("cuda:0"), lanes_per_case=lanes).cpu().numpy()
        bad = np.nonzero((out[:, :6] != want).any(axis=1))[0]
        assert bad.size == 0, f"lanes {lanes} case {bad[0]}: {rec[bad[0]].tolist()} got {out[bad[0]].tolist()} want {want[bad[0]].tolist()}"


@pytest.mark.parametrize("scorer", [False, True])
def test_forced_rare_hands_vs_oracle(scorer):
    """Env-level: decks arranged so that the first play of every episode IS a chosen hand type (bg_inject_deck; a straight
    flush / four of a kind / flush ... at deck[0..k-1], classified on deck[position]), at antes 1..8 with and
    without jokers, small / big / boss blinds: reward shaping (hand quality, efficiency, strategy, synergy, the log10 score
    term), final score, the score breakdown and every other output word against the oracle (tests/helpers.py assert_step_outputs,
    into buffers poisoned before each call), then 40 more steps of the counter-hash policy with the highlights accumulating."""
    import torch
    from balatro_gym_amd import BalatroVecEnv
    from oracle import pyoracle as po
    n = 9 * 64
    seeds = [123_000 + SEED_OFFSET + 11 * i for i in range(n)]
    rr = random.Random(77)
    hts = [i % 9 for i in range(n)]
    decks, scripts = [], []
    for i in range(n):
        d, k = forced_deck(hts[i], rr)
        decks.append(d)
        scripts.append(forced_hand_script(k, rr, blind=[45, 46, 47][(i // 9) % 3]))
    jokers = [rr.sample(range(1, 151), rr.randint(0, 5)) if i % 4 else [] for i in range(n)] if scorer else [[113, 40, 33][: i % 4] for i in range(n)]
    antes = [1 + (i // 27) % 8 for i in range(n)]
    env = BalatroVecEnv(n, seeds, device=0, scorer_jokers=scorer, autoreset=False, max_ante=0)
    env.inject(jokers=jokers, ante=antes, apply_now=True)
    env.inject_deck(decks)
    orc = [po.OracleEnv(s, scorer_jokers=scorer) for s in seeds]
    for o, js, a, d in zip(orc, jokers, antes, decks):
        o.set_jokers(js); o.set_ante(a); o.set_deck(d)
    seen = np.zeros(9, np.int64)
    T = max(len(s) for s in scripts) + 40
    for t in range(T):
        acts = np.array([scripts[i][t] if t < len(scripts[i]) else o.policy_action(0, 31, i, t) for i, o in enumerate(orc)], dtype=np.int32)
        res = [o.step(int(a)) for o, a in zip(orc, acts)]
        poison_env_outputs(env)
        ob, reward, term, trunc, info = env.step(torch.from_numpy(acts).to(env.device))
        ctx = f"scorer {scorer} t {t}"
        assert_step_outputs(ctx, res, reward, term, trunc, info, obs=ob)
        wh = np.array([r[4].hand_type for r in res], dtype=np.int8)
        wt = np.array([r[2] for r in res], dtype=np.uint8)
        for i in range(n):
            if t == len(scripts[i]) - 1 and wh[i] >= 0:
                assert wh[i] == hts[i], (i, wh[i], hts[i])  # the forced play produced the intended type (boss rejections aside)
                seen[wh[i]] += 1
        if wt.any():
            for i in np.nonzero(wt)[0]:
                orc[i].reset(); orc[i].set_jokers(jokers[i]); orc[i].set_ante(antes[i])
            env.reset(mask=torch.from_numpy(wt).to(env.device))
    env.check()
    env.close()
    assert (seen >= 30).all(), seen.tolist()  # every hand type, STRAIGHT_FLUSH included, was played dozens of times


def test_sim_evaluate_batch_golden():
    """balatro_sim.evaluate_hand: all 10 000 hands of sim_eval.npz (every hand type incl. Five of a Kind / Flush House / Flush
    Five, with and without Four Fingers / Shortcut): top, list counts and the first list of all 12 types, position by position."""
    import torch
    from balatro_gym_amd import sim_evaluate_batch
    g = np.load(os.path.join(GOLD, "sim_eval.npz"))
    dev = torch.device("cuda:0")
    flags = g["e_ff"].astype(np.int32) | (g["e_sc"].astype(np.int32) << 1)
    out = sim_evaluate_batch(torch.from_numpy(g["e_cards"].astype(np.int32)).to(dev), torch.from_numpy(g["e_n"].astype(np.int32)).to(dev),
                             torch.from_numpy(flags).to(dev)).cpu().numpy()
    assert np.array_equal(out[:, 0], g["e_top"])
    assert np.array_equal(out[:, 1:13], g["e_nlists"])
    assert np.array_equal(out[:, 13:25], g["e_n0"])
    assert np.array_equal(out[:, 32:128].reshape(-1, 12, 8), g["e_pos"])
    assert (np.bincount(g["e_top"], minlength=12) > 0).all()


def test_sim_score_batch_golden():
    """balatro_sim.calculate_score: the 2 000 cases of sim_eval.npz (score, money, stream position) and the 14 known answers the
    reference itself holds in balatro_trajectories.json."""
    import torch
    from balatro_gym_amd import sim_score_batch
    g = np.load(os.path.join(GOLD, "sim_eval.npz"))
    kat = json.load(open(os.path.join(GOLD, "kat.json")))["trajectories"]
    M = len(g["s_n"])
    rec = np.zeros((M + len(kat), 64), np.int32)
    rec[:M, :48] = g["s_cards"].reshape(M, 48)
    rec[:M, 48], rec[:M, 49] = g["s_n"], g["s_njokers"]
    rec[:M, 50:55] = g["s_jokers"]
    rec[:M, 55], rec[:M, 56], rec[:M, 57] = g["s_hands_left"], g["s_discards_left"], g["s_deck_len"]
    rec[:M, 58] = g["s_seed"].astype(np.int32)
    for i, k in enumerate(kat):
        for q, (r, s) in enumerate(k["cards"]):
            rec[M + i, 6 * q:6 * q + 3] = (r, s, 11 if r == 14 else min(r, 10))
        rec[M + i, 48], rec[M + i, 55], rec[M + i, 58] = len(k["cards"]), 1, 1
    out = sim_score_batch(torch.from_numpy(rec).to("cuda:0")).cpu().numpy()
    bad = np.nonzero((out[:M, 0] != g["s_score"]) | (out[:M, 4] != g["s_money"]) | (out[:M, 6] != g["s_probe"].astype(np.int64)))[0]
    assert bad.size == 0, f"case {bad[0]}: {rec[bad[0]].tolist()} got {out[bad[0]].tolist()} want {g['s_score'][bad[0]], g['s_money'][bad[0]], g['s_probe'][bad[0]]}"
    assert [int(x) for x in out[M:, 0]] == [k["score"] for k in kat]
    # the words the fixture does not hold (chips, added mult, x_mult bits, words drawn, top | nscoring << 8) from the oracle, which
    # tests/test_oracle_golden.py holds to the same fixture
    want = np.array([_sim_words_of_rec(rec[i]) for i in range(len(rec))], dtype=np.int64)
    bad = np.nonzero((out != want).any(axis=1))[0]
    assert bad.size == 0, f"case {bad[0]}: {rec[bad[0]].tolist()} got {out[bad[0]].tolist()} want {want[bad[0]].tolist()}"


def _sim_words_of_rec(c):
    """pyoracle.sim_score_words of one bg_sim_score_batch case record."""
    from oracle import pyoracle as po
    n, nj = int(c[48]), int(c[49])
    cards = [tuple(int(x) for x in c[6 * q:6 * q + 6]) for q in range(n)]
    return po.sim_score_words(cards, [int(j) for j in c[50:50 + nj]], int(c[55]), int(c[56]), int(c[57]), int(np.uint32(c[58])))


def _fresh_sim_cases(M, seed):
    """M bg_sim_score_batch case records: 1-8 cards (every enhancement / edition / seal, duplicate cards), 0-5 jokers with repeats,
    Four Fingers (18) and Shortcut (69) among them, hands_left / discards_left / deck length at their edges."""
    from oracle.gen_golden import IMPLEMENTED, sim_random_hand
    r = random.Random(seed)
    rec = np.zeros((M, 64), np.int32)
    for i in range(M):
        cards = sim_random_hand(r, n=r.randint(1, 8))
        if r.random() < 0.3:   # dense card modifiers
            cards = [(rk, su, bv, r.randrange(9), r.randrange(5), r.randrange(5)) for rk, su, bv, _, _, _ in cards]
        if r.random() < 0.15 and len(cards) < 8:   # an exact duplicate of a card
            cards.insert(r.randrange(len(cards) + 1), r.choice(cards))
        nj = r.randint(0, 5)
        pool = IMPLEMENTED if r.random() < 0.8 else list(range(1, 151))
        jokers = [r.choice(pool) for _ in range(nj)] if r.random() < 0.3 else r.sample(pool, nj)
        for util in (18, 69):
            if r.random() < 0.3 and len(jokers) < 5:
                jokers.insert(r.randint(0, len(jokers)), util)
        hl, dl = r.choice([0, 1, 1, 2, 4, 127]), r.choice([0, 0, 1, 3, 127])
        deck_len = r.choice([0, 1, 8, 40, 52, 53, 127])
        for q, cd in enumerate(cards):
            rec[i, 6 * q:6 * q + 6] = cd
        rec[i, 48], rec[i, 49] = len(cards), len(jokers)
        rec[i, 50:50 + len(jokers)] = jokers
        rec[i, 55:58] = (hl, dl, deck_len)
        rec[i, 58] = np.uint32(r.choice([0, 1, 2 ** 32 - 1, r.randrange(2 ** 32)])).astype(np.int32)
    return rec


def test_sim_score_batch_vs_oracle_fresh_cases():
    """balatro_sim.calculate_score: 20 000 fresh cases against pyoracle.sim_score, ALL 8 output words (score, chips, added mult, x_mult bits,
    money, words drawn, the next getrandbits(32), top | nscoring << 8)."""
    import torch
    from balatro_gym_amd import sim_score_batch
    rec = _fresh_sim_cases(20000, 31337)
    want = np.array([_sim_words_of_rec(c) for c in rec], dtype=np.int64)
    out = sim_score_batch(torch.from_numpy(rec).to("cuda:0")).cpu().numpy()
    bad = np.nonzero((out != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} cases differ; case {bad[0]}: {rec[bad[0]].tolist()} got {out[bad[0]].tolist()} want {want[bad[0]].tolist()}"
    js = rec[:, 50:55]
    assert ((js == 18).any(axis=1).sum() > 1000) and ((js == 69).any(axis=1).sum() > 1000)
    assert len(np.unique(want[:, 7] & 0xff)) == 12   # every top hand type, Five of a Kind / Flush House / Flush Five included


def _fresh_sim_hands(M, seed):
    from oracle.gen_golden import sim_random_hand
    r = random.Random(seed)
    hands = np.zeros((M, 8, 6), np.int32)
    n = np.zeros(M, np.int32)
    flags = np.array([i % 4 for i in range(M)], np.int32)   # none, Four Fingers, Shortcut, both
    for i in range(M):
        cards = sim_random_hand(r, n=r.randint(1, 8))
        n[i] = len(cards)
        hands[i, :len(cards)] = cards
    return hands, n, flags


def _sim_eval_want(hands, n, flags):
    from oracle import pyoracle as po
    return np.stack([po.sim_evaluate_bytes([tuple(int(x) for x in c) for c in hands[i, :n[i]]], bool(flags[i] & 1), bool(flags[i] & 2))
                     for i in range(len(n))])


SIM_EVAL_DOCUMENTED = np.r_[0:25, 32:128]   # bytes of a bg_sim_evaluate_batch row the header defines (25..31 are left untouched)


def test_sim_evaluate_batch_vs_oracle_fresh_hands():
    """balatro_sim.evaluate_hand: 50 000 fresh hands (1-8 cards, duplicates, one-suit and run-heavy hands) with and without Four Fingers /
    Shortcut against pyoracle.sim_evaluate: top, list counts, first-list lengths and positions of all 12 types."""
    import torch
    from balatro_gym_amd import sim_evaluate_batch
    hands, n, flags = _fresh_sim_hands(50000, 2718)
    want = _sim_eval_want(hands, n, flags)
    dev = torch.device("cuda:0")
    out = sim_evaluate_batch(torch.from_numpy(hands).to(dev), torch.from_numpy(n).to(dev), torch.from_numpy(flags).to(dev)).cpu().numpy()
    g, w = out[:, SIM_EVAL_DOCUMENTED], want[:, SIM_EVAL_DOCUMENTED]
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} hands differ; hand {bad[0]} flags {flags[bad[0]]}: {hands[bad[0], :n[bad[0]]].tolist()} got {g[bad[0]].tolist()} want {w[bad[0]].tolist()}"
    assert (np.bincount(want[:, 0], minlength=12) > 0).all()


# ---------------------------------------------------------------------------------------------------------
# guard regions: inputs and outputs as views at an offset inside larger buffers filled with a byte pattern
# ---------------------------------------------------------------------------------------------------------
GUARD_M = [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000]
GUARD_BEFORE, GUARD_AFTER = 16, 256   # rows of pattern in front of row 0 and behind row m (a whole 256-lane block)


class _Guarded:
    """A POISON-filled device byte buffer of GUARD_BEFORE + m + GUARD_AFTER rows of `row_bytes`; `view` = rows [GUARD_BEFORE, +m) as `dtype`."""

    def __init__(self, m, row_bytes, dtype, fill=None):
        import torch
        self.m, self.rb = m, row_bytes
        self.buf = torch.full(((GUARD_BEFORE + m + GUARD_AFTER) * row_bytes,), POISON, dtype=torch.uint8, device="cuda:0")
        self.view = self.buf[GUARD_BEFORE * row_bytes:(GUARD_BEFORE + m) * row_bytes].view(dtype)
        if fill is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(fill)).view(dtype).reshape(-1).to("cuda:0"))

    def ptr(self):
        import ctypes as C
        return C.c_void_p(self.view.data_ptr())

    def rows(self):
        return self.view.cpu().numpy().view(np.uint8).reshape(self.m, self.rb)

    def assert_guards(self, ctx):
        b = self.buf.cpu().numpy()
        lo, hi = GUARD_BEFORE * self.rb, (GUARD_BEFORE + self.m) * self.rb
        assert (b[:lo] == POISON).all(), f"{ctx}: the guard in front of row 0 was written"
        assert (b[hi:] == POISON).all(), f"{ctx}: the guard behind row m was written (first at row {self.m + (np.argmax(b[hi:] != POISON) // self.rb)})"


def _operator_call(rc, what):
    from balatro_gym_amd import _native as nat
    if rc != 0:
        raise nat.NativeError(f"{what} failed ({rc}): {nat.load().bg_last_error(None).decode()}")


def test_operator_guard_regions():
    """All four operators -- both lane mappings of bg_classify_batch_ex / bg_score_hand_batch_ex -- through the C ABI for m in GUARD_M, inputs
    and outputs as views inside larger buffers filled with a byte pattern: every documented output word of rows [0, m) equals the oracle's,
    the pattern in front of row 0 and in the 256 rows behind row m is untouched (inputs' guards included), and what the header says of the
    other output bytes holds -- bg_sim_evaluate_batch leaves bytes 25..31 of a row untouched, bg_score_hand_batch writes 0 into word 7."""
    import ctypes as C
    import torch
    from balatro_gym_amd import _native as nat
    from oracle import pyoracle as po
    L = nat.load()
    M = max(GUARD_M)
    st = C.c_void_p(torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)
    rr = random.Random(99)
    # inputs of the largest m, oracle answers once; every m uses a prefix
    cls_cards = np.zeros((M, 8), np.uint8)
    cls_n = np.zeros(M, np.uint8)
    for i in range(M):
        k = rr.randint(0, 8)
        cls_cards[i, :k] = rr.sample(range(52), k)
        cls_n[i] = k
    cls_want = np.array([po.classify([int(x) for x in cls_cards[i, :cls_n[i]]]) for i in range(M)], np.uint8)
    cases, sh_rec = _score_cases()
    sh_rec = sh_rec[:M]
    sh_want = np.array([po.score_hand_words(c["cards"], c["cards"][:c["nscoring"]], c["hand_type"], c["style"], c["level"], c["jokers"],
                                            c["hands_left"], c["discards_left"], c["deck_len"], c["gseed"]) for c in cases[:M]], np.int64)
    hands, sn, sflags = _fresh_sim_hands(M, 4242)
    se_want = _sim_eval_want(hands, sn, sflags)
    ss_rec = _fresh_sim_cases(M, 777)
    ss_want = np.array([_sim_words_of_rec(c) for c in ss_rec], np.int64)
    for m in GUARD_M:
        for lanes in (1, 8):
            ctx = f"bg_classify_batch_ex m {m} lanes {lanes}"
            ci, ni, out = _Guarded(m, 8, torch.uint8, cls_cards[:m]), _Guarded(m, 1, torch.uint8, cls_n[:m]), _Guarded(m, 1, torch.uint8)
            _operator_call(L.bg_classify_batch_ex(ci.ptr(), ni.ptr(), out.ptr(), C.c_int64(m), lanes, None, st), ctx)
            torch.cuda.synchronize()
            assert np.array_equal(out.rows()[:, 0], cls_want[:m]), ctx
            for b in (ci, ni, out):
                b.assert_guards(ctx)
            ctx = f"bg_score_hand_batch_ex m {m} lanes {lanes}"
            ci, out = _Guarded(m, 160, torch.int32, sh_rec[:m]), _Guarded(m, 64, torch.int64)
            _operator_call(L.bg_score_hand_batch_ex(ci.ptr(), out.ptr(), m, lanes, None, st), ctx)
            got = out.rows().view(np.int64)
            bad = np.nonzero((got != sh_want[:m]).any(axis=1))[0]
            assert bad.size == 0, f"{ctx}: case {bad[0]} got {got[bad[0]].tolist()} want {sh_want[bad[0]].tolist()}"
            ci.assert_guards(ctx); out.assert_guards(ctx)
        ctx = f"bg_sim_evaluate_batch m {m}"
        hi, ni, fi, out = (_Guarded(m, 192, torch.int32, hands[:m]), _Guarded(m, 4, torch.int32, sn[:m]), _Guarded(m, 4, torch.int32, sflags[:m]),
                           _Guarded(m, 128, torch.int8))
        _operator_call(L.bg_sim_evaluate_batch(hi.ptr(), ni.ptr(), fi.ptr(), out.ptr(), m, st), ctx)
        torch.cuda.synchronize()
        got = out.rows().view(np.int8)
        assert np.array_equal(got[:, SIM_EVAL_DOCUMENTED], se_want[:m, SIM_EVAL_DOCUMENTED]), ctx
        assert (got[:, 25:32].view(np.uint8) == POISON).all(), f"{ctx}: bytes 25..31 of a row were written"
        for b in (hi, ni, fi, out):
            b.assert_guards(ctx)
        ctx = f"bg_sim_score_batch m {m}"
        ci, out = _Guarded(m, 256, torch.int32, ss_rec[:m]), _Guarded(m, 64, torch.int64)
        _operator_call(L.bg_sim_score_batch(ci.ptr(), out.ptr(), m, st), ctx)
        got = out.rows().view(np.int64)
        bad = np.nonzero((got != ss_want[:m]).any(axis=1))[0]
        assert bad.size == 0, f"{ctx}: case {bad[0]} got {got[bad[0]].tolist()} want {ss_want[bad[0]].tolist()}"
        ci.assert_guards(ctx); out.assert_guards(ctx)


def test_cross_wave_state_handover_litmus():
    """The step engine hands an env from one service wave to another of the same workgroup through an LDS word, after plain GLOBAL stores
    of the env's state and with plain global loads on the other side (bg_engine.h: no vmcnt drain, no cache-bypassing loads; it relies on
    the CU's one in-order vector-memory pipeline).  tools/micro/litmus_hot.hip runs that hand-over 1 000 workgroups x 2 000 rounds x 512
    16-byte chunks with the reader holding the OLD lines in L1 and two more waves streaming non-temporal stores: no stale read."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tools", "micro", "litmus_hot")
    src = exe + ".hip"
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        if not os.path.exists(hipcc):
            pytest.skip("hipcc not available and tools/micro/litmus_hot not built")
        subprocess.check_call([hipcc, "-O3", "--offload-arch=gfx950", "-o", exe, src])
    out = subprocess.run([exe, "2000"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("stale 0 of ") and int(out.stdout.split()[-1]) >= 1_000_000_000, out.stdout
