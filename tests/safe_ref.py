"""SafeBalatroEnv's episode limits (train_balatro_fixed.py:228-277) restated in Python: the oracle-side wrapper of the bg_step_many_rows_ex tests.
`SafeCounters.step` is the rule of csrc/bg_safe.h for one env; tests/test_step_many_safe_host.py holds both to the reference's own wrapper output
(tests/golden/sb3_fixed.npz).  Also here: the golden's inner signals, a Monitor restatement over wrapped steps, and SB3's time-limit bootstrap."""
import os

import numpy as np

from tests.helpers import GOLD

END_GAME, END_INVALID, END_MAX_STEPS = 1, 2, 4


class SafeCounters:
    """The wrapper's two counters for one env."""

    def __init__(self, max_invalid_actions=50, max_episode_steps=1000, episode_steps=0, consecutive_invalid=0):
        self.max_invalid_actions, self.max_episode_steps = int(max_invalid_actions), int(max_episode_steps)
        self.episode_steps, self.consecutive_invalid = int(episode_steps), int(consecutive_invalid)

    def step(self, reward, env_terminated):
        """(reward to record, BG_END_* flags) of one step whose env returned `reward` (float64) and `env_terminated`; flags != 0 = SB3's done,
        and both counters are back at 0 (the reset that follows)."""
        reward = float(reward)
        self.episode_steps += 1
        kill = False
        if reward == -1.0 and not env_terminated:
            self.consecutive_invalid += 1
            if self.consecutive_invalid >= self.max_invalid_actions:
                kill, reward = True, -50.0
        else:
            self.consecutive_invalid = 0
        max_steps = self.episode_steps >= self.max_episode_steps
        flags = (END_GAME if env_terminated else 0) | (END_INVALID if kill else 0) | (END_MAX_STEPS if max_steps else 0)
        if flags:
            self.episode_steps = self.consecutive_invalid = 0
        return reward, flags


def wrapper_ending(flags):
    """The wrapper ended the episode and the env itself did not: the env still needs its reset, and SB3 keeps a terminal_observation."""
    return flags != 0 and not flags & END_GAME


def terminal_slots(K, max_invalid_actions, max_episode_steps):
    return K // min(max_invalid_actions, max_episode_steps) + 1


def load_golden():
    with np.load(os.path.join(GOLD, "sb3_fixed.npz")) as z:
        return {k: z[k] for k in z.files}


def golden_inner(g):
    """What the env INSIDE the wrapper returned in the golden run, [env, step]: (reward float64 with the wrapper's -50 taken back to the -1.0 it
    replaced, env terminated) -- and the flags byte the wrapper's outputs amount to."""
    kill = g["invalid_action_termination"] != 0
    reward = g["rewards"].astype(np.float64)
    assert (reward[kill] == -50.0).all()
    reward[kill] = -1.0
    env_term = (g["terminated"] != 0) & ~kill
    flags = env_term * END_GAME + kill * END_INVALID + (g["max_steps_reached"] != 0) * END_MAX_STEPS
    return reward, env_term, flags.astype(np.uint8)


def monitor(rewards, dones, carry_return=None, carry_len=None):
    """Monitor outside SafeBalatroEnv over [K, N] wrapped steps (it sees the -50s and every ending): (ep_return float64, ep_len int32) [K, N],
    the finished episode's plain float64 reward sum in step order and its length on a done step, 0 elsewhere; the carries are updated in place."""
    K, N = rewards.shape
    cr = np.zeros(N, np.float64) if carry_return is None else carry_return
    cl = np.zeros(N, np.int32) if carry_len is None else carry_len
    er, el = np.zeros((K, N), np.float64), np.zeros((K, N), np.int32)
    for t in range(K):
        cr += rewards[t]
        cl += 1
        d = dones[t] != 0
        er[t, d], el[t, d] = cr[d], cl[d]
        cr[d], cl[d] = 0.0, 0
    return er, el


def bootstrap(rewards, flags, index, terminal_values, gamma):
    """SB3's collect_rollouts: rewards[idx] += gamma * terminal_value where the episode was truncated and not terminated.  rewards float64 [K, N],
    flags uint8 [K, N], index int [M] = t * N + e of every wrapper ending, terminal_values [M]."""
    out = np.array(rewards, np.float64).copy().reshape(-1)
    f = np.asarray(flags).reshape(-1)
    for i, v in zip(np.asarray(index, np.int64), np.asarray(terminal_values)):
        if f[i] == END_MAX_STEPS:
            out[i] += float(gamma) * float(np.float64(v))
    return out.reshape(np.asarray(rewards).shape)
