"""Envs ABOVE their curriculum cap, on the oracle: the scenario of tests/test_above_cap_host.py (no GPU) and tests/test_above_cap.py (GPU).

The reference ends an episode on EVERY step taken while state.ante > current_max_ante (train_balatro_agent.py:147-152; oracle/balatro_oracle.c
bo_step).  An env gets above its cap in two ways: it exceeds the cap by play and, with auto-reset off, is stepped on; or the cap is LOWERED below
the ante of a running env (bg_set_max_ante, RowCurriculum.load_state_dict(apply=True), CurriculumTracker).  The scenario has both:

  N = 300 envs (two 256-env workgroups of bg_engine.h, the second partly live; five 64-env blocks of bg_engine3.h), level-15 hands (antes rise
  within tens of steps), caps 3 + i % 2;
  W warm-up steps under the oracle's uniform counter-hash policy;
  then the caps are lowered by env index: to 1 for i % 4 in (0, 1), to 2 for i % 4 == 2, unchanged for i % 4 == 3;
  K further steps: an env above its cap takes one of EIGHT KINDS of action chosen from (i, t) and its phase -- a toggle, an out-of-range action, an
  in-range action the mask forbids, PLAY_HAND, a blind selection, a shop leave, DISCARD, a shop reroll -- every other env the policy's.

"caller" mode, auto-reset ON: every env the lowering leaves above its cap ends its episode on the next step and plays on in a new one.
"caller" mode, auto-reset OFF: nothing is ever reset; such an env stays above its cap for all K steps (and an env that exceeded cap 3 / 4 by play
during the warm-up is stepped on as well), every step terminated with flag 256.
"policy" mode (the rollouts: always auto-reset): every action is the policy's.

W was chosen from the oracle (`python -m tests.above_cap_ref` prints the counts for a range of W): the smallest multiple of 4 at which the
conditions of tests/test_above_cap_host.py hold with room to spare."""
import functools
import os

import numpy as np

from tests.helpers import OBS_KEYS

SEED_OFFSET = int(os.environ.get("BG_TEST_SEED_OFFSET", "0"))   # (the suite's convention: tests/test_gpu_parity.py)
N, W, K = 300, 52, 24
POLICY, PSEED = 0, 31
KINDS = ("toggle", "out_of_range", "masked", "play", "blind", "leave", "discard", "reroll")
# what a step of an above-cap env turned out to be (the action is only a toggle where the phase and the mask allow it)
DONE = ("toggle", "leave", "invalid", "play", "blind", "discard", "shop", "other")
# A BLIND SELECTION is never valid above a cap: the game offers one only behind a reset (leaving the shop goes straight to the play phase), where the ante
# is the reset template's, which bg_set_max_ante and bg_inject keep at or below the cap.  Action 45 is still sent -- it is then an in-range action the
# mask forbids -- and DISCARD and a shop reroll stand in as further service kinds.  (tests/test_oracle_vs_reference.py forces the state on the reference.)
CHEAP, SERVICE = ("toggle", "leave", "invalid"), ("play", "discard", "shop")


def seeds():
    return [417_000 + SEED_OFFSET + 3 * i for i in range(N)]


def caps0():
    return np.array([3 + i % 2 for i in range(N)], np.int32)


def caps1():
    c = caps0()
    for i in range(N):
        if i % 4 in (0, 1):
            c[i] = 1
        elif i % 4 == 2:
            c[i] = 2
    return c


def set_levels(o):
    for ht in range(12):
        o.set_hand_level(ht, 15)


def oracle_envs():
    from oracle import pyoracle as po
    orc = [po.OracleEnv(s, max_ante=int(c)) for s, c in zip(seeds(), caps0())]
    for o in orc:
        set_levels(o)
    return orc


# which kind an above-cap env takes at (i, t), by its phase (0 play, 1 shop, 2 blind selection): the kinds the phase has no use for would all come
# out as the same masked action
BY_PHASE = ((0, 1, 2, 3, 4, 6), (5, 1, 2, 7, 5, 4), (4, 1, 2, 4, 4, 1))


def kind_of(i, t, phase):
    return BY_PHASE[phase][(i // 4 + t) % 6]


def kind_action(kind, i, t, mask):
    """The action of kind KINDS[kind] for env i at step t under the 60-entry action mask `mask`."""
    if kind == 0:
        return 2 + (i + t) % 8
    if kind == 1:
        return (60, -1, 1000, 32768 + 2)[(i + t) % 4]
    if kind == 2:
        return int(np.flatnonzero(np.asarray(mask) == 0)[(i + t) % 3])   # (a mask always forbids more than three actions)
    if kind == 4:   # the blind on offer (one of 45 / 46 / 47 at a time)
        on = [a for a in (45, 46, 47) if mask[a]]
        return on[0] if on else 45
    return {3: 0, 5: 31, 6: 1, 7: 30}[kind]


def classify(phase, action, mask):
    """DONE index of `action` taken in `phase` under `mask`."""
    if not (0 <= action < 60 and mask[action]):
        return 2
    if phase == 0 and 2 <= action < 10:
        return 0
    if phase == 1 and action == 31:
        return 1
    if phase == 0 and action == 0:
        return 3
    if phase == 2 and 45 <= action < 48:
        return 4
    if phase == 0 and action == 1:
        return 5
    return 6 if phase == 1 else 7


class Scenario:
    """acts int32 [T, N]; res[t][i] = (None, reward, terminated, False, Info) as OracleEnv.step returned them; want_obs[t] = the observation a step's
    outputs show, stacked per key (with auto-reset: the new episode's); reward float64 / terminated uint8 / flags int32 / error int32 [T, N];
    above bool [T, N]: the env stood above its cap BEFORE step t; done int8 [T, N]: DONE index of the step of an above-cap env (-1 elsewhere);
    final = the observation behind the last step."""

    def __init__(self, mode, autoreset, T):
        self.mode, self.autoreset, self.T = mode, autoreset, T
        self.acts = np.zeros((T, N), np.int32)
        self.reward = np.zeros((T, N), np.float64)
        self.terminated = np.zeros((T, N), np.uint8)
        self.flags = np.zeros((T, N), np.int32)
        self.error = np.zeros((T, N), np.int32)
        self.above = np.zeros((T, N), bool)
        self.done = np.full((T, N), -1, np.int8)
        self.res, self.want_obs = [], []
        self.final = None

    def records(self, lo, hi):
        """Steps lo .. hi - 1 as packed records uint8 [hi - lo, N, 352] (byte 343 and the bytes behind it zero)."""
        from tests.test_step_many_safe import _pack
        rows = np.stack([_pack(self.want_obs[t], self.reward[t], self.acts[t], self.terminated[t]) for t in range(lo, hi)])
        rows[:, :, 343] = 0
        return rows

    def stats(self, lo, hi, t0=0):
        """The five oracle-checked rollout stats of steps lo .. hi - 1, step lo counted as step t0."""
        bits = plays = score = 0
        for t in range(lo, hi):
            for b in self.reward[t].view(np.uint64):
                bits ^= (int(b) * (2 * (t0 + t - lo) + 1)) & (2 ** 64 - 1)
            for r in self.res[t]:
                if r[4].hand_type >= 0:
                    plays += 1
                    score += r[4].final_score
        return {"steps": (hi - lo) * N, "episodes": int((self.terminated[lo:hi] != 0).sum()), "plays": plays, "score_sum": score, "reward_bits": bits}


def run(mode, autoreset, warmup=W, steps=K, lower=True):
    """The scenario on the oracle (see the module docstring); `lower=False` leaves the caps alone (for choosing W)."""
    assert mode in ("caller", "policy") and (autoreset or mode == "caller")
    orc = oracle_envs()
    cap = caps0().copy()
    T = warmup + steps
    sc = Scenario(mode, autoreset, T)
    cur = [o.obs() for o in orc]
    for t in range(T):
        if t == warmup and lower:
            cap = caps1()
            for o, c in zip(orc, cap):
                o.set_max_ante(int(c))
        res = []
        for i, o in enumerate(orc):
            ob = cur[i]
            ab = int(ob["ante"]) > cap[i]
            sc.above[t, i] = ab
            if ab and mode == "caller":
                a = kind_action(kind_of(i, t, int(ob["phase"])), i, t, ob["action_mask"])
            else:
                a = o.policy_action(POLICY, PSEED, i, t)
            if ab:
                sc.done[t, i] = classify(int(ob["phase"]), a, ob["action_mask"])
            sc.acts[t, i] = a
            nob, r, term, _, info = o.step(int(a))
            sc.reward[t, i], sc.terminated[t, i], sc.flags[t, i], sc.error[t, i] = r, term, info.flags, info.error
            if term and autoreset:
                o.reset(); set_levels(o)
                nob = o.obs()
            cur[i] = nob
            res.append((None, r, term, False, info))
        sc.res.append(res)
        sc.want_obs.append({k: np.stack([np.asarray(w[k]) for w in cur]) for k in OBS_KEYS})
    sc.final = sc.want_obs[-1]
    for a in (sc.acts, sc.reward, sc.terminated, sc.flags, sc.error, sc.above, sc.done):
        a.setflags(write=False)
    return sc


@functools.lru_cache(maxsize=None)
def scenario(mode, autoreset):
    """run(mode, autoreset) with the module's W and K: computed once per process, shared, never modified."""
    return run(mode, autoreset)


WRAP_LIMITS = (4, 60)   # SafeBalatroEnv's max_invalid_actions / max_episode_steps of the wrapped scenario


def summary_bytes(ob):
    """Bytes 344..351 of the record of a step that ended an episode in the state `ob` shows (bg_set_episode_summary)."""
    out = np.zeros(8, np.uint8)
    out[0:2] = np.array([int(ob["ante"])], np.int16).view(np.uint8)
    out[2:3] = np.array([int(ob["round"])], np.int8).view(np.uint8)
    out[4:8] = np.array([min(max(int(ob["chips_scored"]), 0), 2 ** 32 - 1)], np.uint32).view(np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def wrapped(progress):
    """The "caller" scenario with auto-reset under SafeBalatroEnv's limits WRAP_LIMITS (tests/safe_ref.py), with progress=True under
    ProgressionRewardWrapper in front of them (tests/progress_ref.py), the episode summary on: a cap ending is an ending the ENV made -- flags
    END_GAME, counters and carry back at their reset values, the summary in bytes 344..351 -- whatever action the env took.  Env i with i % 16 == 5
    sends runs of out-of-range actions while below its cap (kills).  Returns two calls, the W warm-up steps and the K steps behind the lowering:
    (actions [k, N], expected records [k, N, 352], terminal records ((t, e, record)), the limits' counters [N, 2], the packed progression carry
    [N, 4] or None), and `cap_ended` bool [W + K, N]: the env stood above its cap before the step.  Computed once, never modified."""
    from tests import progress_ref, safe_ref
    from tests.test_step_many_safe import _pack
    orc = oracle_envs()
    cap = caps0().copy()
    cur = [o.obs() for o in orc]
    wr = [progress_ref.ProgressSafe(*WRAP_LIMITS) if progress else safe_ref.SafeCounters(*WRAP_LIMITS) for _ in range(N)]
    cap_ended = np.zeros((W + K, N), bool)
    calls = []
    for lo, hi in ((0, W), (W, W + K)):
        if lo:
            cap = caps1()
            for o, c in zip(orc, cap):
                o.set_max_ante(int(c))
        k = hi - lo
        acts, want, terminal = np.zeros((k, N), np.int32), np.zeros((k, N, 352), np.uint8), []
        for j in range(k):
            t = lo + j
            rew, flags, extra = np.zeros(N), np.zeros(N, np.uint8), {}
            for i, o in enumerate(orc):
                ob = cur[i]
                ab = int(ob["ante"]) > cap[i]
                cap_ended[t, i] = ab
                if ab:
                    a = kind_action(kind_of(i, t, int(ob["phase"])), i, t, ob["action_mask"])
                elif i % 16 == 5 and t % 8 < 5:
                    a = 60
                else:
                    a = o.policy_action(POLICY, PSEED, i, t)
                acts[j, i] = a
                nob, r, term, _, info = o.step(int(a))
                assert bool(term) and info.flags & 256 if ab else True
                if progress:
                    rew[i], flags[i] = wr[i].step(r, bool(term), int(nob["ante"]), int(nob["round"]))
                else:
                    rew[i], flags[i] = wr[i].step(r, bool(term))
                if safe_ref.wrapper_ending(int(flags[i])):
                    terminal.append((j, i, _pack({key: np.asarray(nob[key])[None] for key in OBS_KEYS}, rew[i:i + 1], acts[j, i:i + 1], flags[i:i + 1])[0]))
                if flags[i]:   # SAME_STEP reset, whoever ended the episode: the record shows the new one and the summary the old one's end
                    extra[i] = summary_bytes(nob)
                    o.reset(); set_levels(o)
                    nob = o.obs()
                cur[i] = nob
            want[j] = _pack({key: np.stack([np.asarray(w[key]) for w in cur]) for key in OBS_KEYS}, rew, acts[j], flags)
            for i, s in extra.items():
                want[j, i, 344:352] = s
        if progress:
            counters = np.array([[x.safe.episode_steps, x.safe.consecutive_invalid] for x in wr], np.int32)
            carry = np.stack([x.prog.pack() for x in wr])
        else:
            counters, carry = np.array([[x.episode_steps, x.consecutive_invalid] for x in wr], np.int32), None
        for a in (acts, want, counters) + ((carry,) if progress else ()):
            a.setflags(write=False)
        calls.append((acts, want, tuple(terminal), counters, carry))
    cap_ended.setflags(write=False)
    return tuple(calls), cap_ended


def counts(sc, warmup=W):
    """What the GPU tests rest on, from the oracle side alone (tests/test_above_cap_host.py asserts it)."""
    ab = sc.above[warmup]
    first = sc.done[warmup]
    run_len = np.zeros(N, np.int64)   # consecutive steps above the cap from the lowering on
    for i in range(N):
        t = warmup
        while t < sc.T and sc.above[t, i]:
            t += 1
        run_len[i] = t - warmup
    return {"above_at_lowering": int(ab.sum()), "of_them_env_256_up": int(ab[256:].sum()),
            "per_64_block": [int(ab[k:k + 64].sum()) for k in range(0, N, 64)],
            "first_action": {name: int((first[ab] == DONE.index(name)).sum()) for name in DONE},
            "envs_5_steps_above": int((run_len >= 5).sum()),
            "steps_above_after_lowering": int(sc.above[warmup:].sum()),
            "steps_above_in_warmup": int(sc.above[:warmup].sum())}


if __name__ == "__main__":   # how W was chosen: the counts at the lowering for a range of warm-up lengths
    for autoreset in (True, False):
        sc = run("caller", autoreset, warmup=80, steps=0, lower=False)
        new = caps1()
        for w in range(24, 81, 4):
            ob = sc.want_obs[w - 1]   # the observation in front of step w
            ab = ob["ante"] > new
            first = np.array([classify(int(ob["phase"][i]), kind_action(kind_of(i, w, int(ob["phase"][i])), i, w, ob["action_mask"][i]), ob["action_mask"][i])
                              for i in range(N)])
            print(f"autoreset {autoreset} W {w}: above {int(ab.sum())}, env >= 256 {int(ab[256:].sum())}, per block "
                  f"{[int(ab[k:k + 64].sum()) for k in range(0, N, 64)]}, first action {[int((first[ab] == d).sum()) for d in range(len(DONE))]} {DONE}")
