"""ProgressionRewardWrapper (train_progressive.py:21-120) restated in Python and composed with tests/safe_ref.SafeCounters the way train_progressive.py
stacks the two (SafeBalatroEnv outside): the oracle-side wrapper of the bg_step_many_rows_progress tests.  `ProgressCarry.step` is the rule of
csrc/bg_progress.h for one env; tests/test_step_many_progress_host.py holds both to the reference's own wrapper output (tests/golden/progression.npz)."""
import os

import numpy as np

from tests import safe_ref
from tests.helpers import GOLD

END_GAME, END_INVALID, END_MAX_STEPS, END_STUCK = 1, 2, 4, 8
STUCK_STEPS = 300


class ProgressCarry:
    """The wrapper's state for one env; the defaults are the state after reset()."""

    def __init__(self, total_steps=0, steps_on_current_ante=0, last_ante=1, last_round=1, max_ante_reached=1):
        self.total_steps, self.steps_on_current_ante = int(total_steps), int(steps_on_current_ante)
        self.last_ante, self.last_round, self.max_ante_reached = int(last_ante), int(last_round), int(max_ante_reached)

    def reset(self):
        self.__init__()

    def step(self, reward, ante, round_):
        """(shaped reward, stuck) of one step whose env returned `reward` (float64) and stands at state.ante / state.round = ante / round_.  Python
        floats are float64 and every `+=` is one rounding, as in the reference."""
        reward, ante, round_ = float(reward), int(ante), int(round_)
        stuck = False
        self.total_steps += 1
        if ante == self.last_ante:
            self.steps_on_current_ante += 1
        else:
            self.steps_on_current_ante = 0
        if ante > self.last_ante:
            reward += 200 * (ante - self.last_ante)
            self.last_ante = ante
        if round_ > self.last_round and ante == self.last_ante:
            reward += 20
            self.last_round = round_
        if ante > self.max_ante_reached:
            self.max_ante_reached = ante
            reward += 100
        if ante == 1 and self.steps_on_current_ante > 150:
            reward += -0.5 * (self.steps_on_current_ante - 150)
            if self.steps_on_current_ante > STUCK_STEPS:
                stuck = True
                reward -= 50
        if self.total_steps > 200 and ante < 2:
            reward -= 0.2
        elif self.total_steps > 400 and ante < 3:
            reward -= 0.3
        elif self.total_steps > 600 and ante < 4:
            reward -= 0.4
        if ante >= 3 and self.total_steps < 300:
            reward += 50
        if ante != self.last_ante:
            self.last_round = round_
        return reward, stuck

    def values(self):
        return (self.total_steps, self.steps_on_current_ante, self.last_ante, self.last_round, self.max_ante_reached)

    def pack(self):
        """The four int32 words of bg_progress_rewards.counters_dev."""
        w2 = ((self.last_ante - 1) & 0xffff) | (((self.max_ante_reached - 1) & 0xffff) << 16)
        return np.array([self.total_steps, self.steps_on_current_ante, w2 - ((w2 >> 31) << 32), self.last_round - 1], np.int32)   # (w2 as a signed word)

    @classmethod
    def unpack(cls, w):
        w = [int(x) for x in w]
        w2 = w[2] & 0xffffffff
        return cls(w[0], w[1], (w2 & 0xffff) + 1, w[3] + 1, (w2 >> 16) + 1)


class ProgressSafe:
    """SafeBalatroEnv(ProgressionRewardWrapper(env), max_invalid_actions, max_episode_steps) for one env, with the reset SB3's VecEnv gives it."""

    def __init__(self, max_invalid_actions=50, max_episode_steps=1000):
        self.safe = safe_ref.SafeCounters(max_invalid_actions, max_episode_steps)
        self.prog = ProgressCarry()

    def step(self, reward, env_terminated, ante, round_):
        """(reward to record, flags) of one step: BG_END_GAME only for the env's own ending, BG_END_STUCK for the wrapper's; flags != 0 = SB3's done,
        and both wrappers are back in their reset state."""
        shaped, stuck = self.prog.step(reward, ante, round_)
        out, f = self.safe.step(shaped, bool(env_terminated) or stuck)
        flags = (f & ~END_GAME) | (END_GAME if env_terminated else 0) | (END_STUCK if stuck else 0)
        if flags:
            self.prog.reset()
        return out, flags


def wrapper_ending(flags):
    """A wrapper ended the episode and the env itself did not: the env still needs its reset, and SB3 keeps a terminal_observation."""
    return flags != 0 and not flags & END_GAME


def terminal_slots(K, max_invalid_actions, max_episode_steps):
    return K // min(max_invalid_actions, max_episode_steps, STUCK_STEPS + 1) + 1


def load_golden():
    with np.load(os.path.join(GOLD, "progression.npz")) as z:
        return {k: z[k] for k in z.files}
