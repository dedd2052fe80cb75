#!/usr/bin/env python3
"""Makes tests/golden/progression.npz from the Python reference (build container only: it needs the reference tree, see oracle/refharness.py).

    python tools/gen_progress_golden.py [out.npz]

The reference's own `train_progressive.ProgressionRewardWrapper` is imported from where it lies and stepped inside its own SafeBalatroEnv, as
`make_progression_env` stacks them: SafeBalatroEnv(ProgressionRewardWrapper(BalatroEnvFixed(seed + rank)), MAX_INVALID, MAX_STEPS).  Only the recorded
numbers are committed.  Per step and env ([env, step] arrays): the action; the INNER env's reward and terminated (what BalatroEnvFixed.step returned,
taken by an instance attribute around it, so that the wrapper still finds `env.env.state`); state.ante and state.round behind the step; the stack's
reward, terminated and truncated; the info flags stuck_on_ante_1, invalid_action_termination and max_steps_reached.  After a done the stack is reset(),
as SB3's VecEnv does, and the env's script re-applies what it injected.

The envs (ROLES): scripted so that a short run holds every branch of the wrapper -- see tests/test_step_many_progress_host.py, which asserts that the
file holds them."""
import contextlib
import io
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import refharness as rh   # noqa: E402

SEED0, T = 4200, 640
MAX_INVALID, MAX_STEPS = 50, 610
ROLES = ["idle", "idle_ante2", "idle_ante3", "invalid", "invalid_late", "play", "play", "play_ante2"]


def _load_wrapper():
    rh.load_fixed_wrappers()
    for name, attrs in (("gymnasium.wrappers", ["TimeLimit"]), ("stable_baselines3.common.utils", ["set_random_seed"])):
        if name not in sys.modules:
            m = types.ModuleType(name)
            for a in attrs:
                setattr(m, a, type(a, (), {"__init__": lambda self, *x, **k: None}))
            sys.modules[name] = m
    with contextlib.redirect_stdout(io.StringIO()):
        import train_progressive as tp
    return tp


class Stack:
    """One env of the stack with the harness's per-env global random stream (oracle/refharness.py RefFixedEnv)."""

    def __init__(self, tp, seed, role):
        tbf = rh.load_fixed_wrappers()
        self.role = role
        self.inner = None
        random.seed(rh.global_seed(seed))
        with contextlib.redirect_stdout(io.StringIO()):
            self.fixed = tbf.BalatroEnvFixed(seed=seed)
            inner_step = self.fixed.step

            def recorded(action):
                out = inner_step(action)
                self.inner = (float(out[1]), bool(out[2]))
                return out
            self.fixed.step = recorded
            self.env = tbf.SafeBalatroEnv(tp.ProgressionRewardWrapper(self.fixed), max_invalid_actions=MAX_INVALID, max_episode_steps=MAX_STEPS)
        self._g = random.getstate()
        self.reset()

    def _call(self, fn, *a):
        random.setstate(self._g)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                return fn(*a)
        finally:
            self._g = random.getstate()

    @property
    def state(self):
        return self.fixed.env.state

    def reset(self):
        self._call(self.env.reset)
        if self.role.endswith("ante2"):
            self.state.ante = 2
        if self.role.endswith("ante3"):
            self.state.ante = 3
        if self.role.startswith("play"):   # level-15 hands beat every blind at once
            se = rh.load_reference()["se"]
            for ht in range(12):
                self.fixed.env.engine.set_hand_level(se.HandType(ht), 15)
                self.state.hand_levels[se.HandType(ht)] = self.fixed.env.engine.get_hand_level(se.HandType(ht))

    def action(self, t):
        phase, nsel = int(self.state.phase), len(self.state.selected_cards)
        if self.role == "invalid" or (self.role == "invalid_late" and t >= 205):
            return 59   # in range, never valid
        if phase == 2:
            return 45
        if phase == 1:
            return 31
        if self.role.startswith("play") and self.state.ante < 4:   # (from ante 4 on it idles: the money of more level-15 wins leaves the observation's int16)
            return 0 if nsel > 0 else 2
        return 2 + t % 8


def main(out):
    tp = _load_wrapper()
    S = len(ROLES)
    envs = [Stack(tp, SEED0 + r, ROLES[r]) for r in range(S)]
    rec = {k: np.zeros((S, T), dt) for k, dt in (("actions", np.int32), ("inner_reward", np.float64), ("inner_terminated", np.uint8), ("ante", np.int32),
                                                  ("round", np.int32), ("reward", np.float64), ("terminated", np.uint8), ("truncated", np.uint8),
                                                  ("stuck_on_ante_1", np.uint8), ("invalid_action_termination", np.uint8), ("max_steps_reached", np.uint8))}
    for t in range(T):
        for e, s in enumerate(envs):
            a = s.action(t)
            _, reward, terminated, truncated, info = s._call(s.env.step, a)
            assert "error" not in info or reward != -100.0, (e, t, info)
            rec["actions"][e, t] = a
            rec["inner_reward"][e, t], rec["inner_terminated"][e, t] = s.inner
            rec["ante"][e, t], rec["round"][e, t] = s.state.ante, s.state.round
            rec["reward"][e, t], rec["terminated"][e, t], rec["truncated"][e, t] = reward, terminated, truncated
            for k in ("stuck_on_ante_1", "invalid_action_termination", "max_steps_reached"):
                rec[k][e, t] = bool(info.get(k, False))
            if terminated or truncated:
                s.reset()
    np.savez_compressed(out, seed0=np.int64(SEED0), max_invalid_actions=np.int32(MAX_INVALID), max_episode_steps=np.int32(MAX_STEPS),
                        roles=np.array(ROLES), **rec)
    print(out, os.path.getsize(out), "bytes;", {k: int(rec[k].sum()) for k in ("terminated", "truncated", "stuck_on_ante_1", "invalid_action_termination", "max_steps_reached")})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "progression.npz"))
