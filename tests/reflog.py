"""The Python reference's answers to tests/test_oracle_vs_reference.py, recorded once and replayed by the tests.

The tests put questions to the reference (construct an env, step it, inject state, read its observation, score a hand) and compare the
answers with the C oracle, which runs live.  `Recorder` asks the live reference (oracle/refharness.py) and logs every call with its
answer; `oracle/gen_golden.py reference_logs` runs each test with one and writes tests/golden/reflog_<test>.npz.  `Replayer` answers
from that log and checks that the test asks exactly the recorded questions, in the recorded order, so the inputs cannot drift from
the ones the answers belong to.  Observations are kept in the reference's own dtypes and shapes; every other answer as JSON (floats
round-trip exactly).
"""
from __future__ import annotations

import json
import os

import numpy as np

from tests.helpers import GOLD, OBS_KEYS

TERMS = ["progress", "milestone", "score", "hand_quality", "efficiency", "synergy", "strategy", "ante_bonus"]
EXCEPTIONS = {"IndexError": IndexError, "OverflowError": OverflowError, "ValueError": ValueError, "KeyError": KeyError}


def log_path(name: str) -> str:
    return os.path.join(GOLD, "reflog_" + name.replace("[", "_").replace("]", "") + ".npz")


def _py(v):
    return v.item() if isinstance(v, np.generic) else v


class _Log:
    """Shared by Recorder and Replayer: the call counter, and the decoding of a logged answer."""

    def __init__(self, name: str):
        self.name = name
        self.n_envs = 0

    def _obs(self, idx: int) -> dict:
        return {k: self.obs_table[k][idx] for k in OBS_KEYS}

    def _decode(self, kind: str, enc):
        if isinstance(enc, dict) and "raise" in enc:
            raise EXCEPTIONS[enc["raise"]](f"(recorded) {enc['msg']}")
        if kind == "obs":
            return self._obs(enc)
        if kind == "step":
            info = {}
            if enc["info"] is not None:
                info = dict(enc["info"])
                info["reward_breakdown"] = dict(zip(TERMS, info.pop("terms")))
            return self._obs(enc["obs"]), enc["r"], enc["t"], enc["u"], info
        if kind == "sim_evaluate":
            top, per = enc
            return top, {t: (n, pos) for t, n, pos in per}
        if kind == "sim_score":
            return tuple(enc)
        return enc

    def env(self, seed: int, scorer_jokers: bool = False, max_ante: int = 0) -> "RefEnvLog":
        self.n_envs += 1
        e = RefEnvLog(self, self.n_envs - 1)
        self._call(f"env({seed}, {scorer_jokers}, {max_ante})", None, lambda: self._live_env(e, seed, scorer_jokers, max_ante))
        return e

    def sim_evaluate(self, cards, four_fingers=False, shortcut=False):
        return self._call(f"sim_evaluate({cards!r}, {four_fingers}, {shortcut})", "sim_evaluate",
                          lambda: self._live_sim_evaluate(cards, four_fingers, shortcut))

    def sim_score(self, cards, jokers, game_state_keys, deck_len, seed):
        return self._call(f"sim_score({cards!r}, {jokers!r}, {game_state_keys!r}, {deck_len}, {seed})", "sim_score",
                          lambda: self._live_sim_score(cards, jokers, game_state_keys, deck_len, seed))


class RefEnvLog:
    """One reference env of a log, with the surface of oracle.refharness.RefEnv the tests use (the deck is read through
    deck_len / deck_real_cards instead of the reference's objects)."""

    def __init__(self, log: _Log, no: int):
        self._log, self._no, self.live = log, no, None

    def _c(self, call, kind, fn):
        return self._log._call(f"{self._no}.{call}", kind, fn)

    def obs(self):
        return self._c("obs()", "obs", lambda: self.live.obs())

    def reset(self, seed=None):
        return self._c(f"reset({seed})", "obs", lambda: self.live.reset(seed=seed))

    def step(self, action: int):
        return self._c(f"step({int(action)})", "step", lambda: self.live.step(action))

    def deck_len(self) -> int:
        return self._c("deck_len()", None, lambda: len(self.live.env.state.deck))

    def deck_real_cards(self) -> int:
        """Cards of the deck that are the reference's own Card objects (Cryptid's copies are consumables.Card)."""
        return self._c("deck_real_cards()", None, lambda: sum(1 for c in self.live.env.state.deck if type(c).__module__.endswith("cards")))

    def __getattr__(self, name):
        if not name.startswith("set_"):
            raise AttributeError(name)

        def setter(*args):
            return self._c(f"{name}{tuple(args)!r}", None, lambda: getattr(self.live, name)(*args))
        return setter


class Recorder(_Log):
    """Asks the live reference and logs the answers (needs the reference tree: oracle/refharness.py)."""

    def __init__(self, name: str):
        super().__init__(name)
        from oracle import refharness as rh
        self.rh = rh
        self.calls, self.answers = [], []
        self.obs_table = {k: [] for k in OBS_KEYS}

    def _add_obs(self, o) -> int:
        for k in OBS_KEYS:
            self.obs_table[k].append(np.asarray(o[k]))
        return len(self.obs_table[OBS_KEYS[0]]) - 1

    def _encode(self, kind, v):
        if kind == "obs":
            return self._add_obs(v)
        if kind == "step":
            obs, r, t, u, info = v
            inf = None
            if "final_score" in info:
                inf = {"final_score": _py(info["final_score"]), "hand_type": int(info["hand_type"]), "cards_played": _py(info["cards_played"]),
                       "terms": [float(info["reward_breakdown"][k]) for k in TERMS]}
            return {"obs": self._add_obs(obs), "r": float(r), "t": bool(t), "u": bool(u), "info": inf}
        if kind == "sim_evaluate":
            top, per = v
            return [int(top), [[int(t), int(n), [int(p) for p in pos]] for t, (n, pos) in sorted(per.items())]]
        if kind == "sim_score":
            return [int(x) for x in v]
        return _py(v)

    def _call(self, call, kind, fn):
        try:
            enc = self._encode(kind, fn())
        except tuple(EXCEPTIONS.values()) as ex:
            enc = {"raise": type(ex).__name__, "msg": str(ex)}
        self.calls.append(call)
        self.answers.append(json.dumps(enc))
        # the test sees what a replay will give it
        return self._decode(kind, enc)

    def _live_env(self, e, seed, scorer_jokers, max_ante):
        e.live = self.rh.RefEnv(seed, scorer_jokers=scorer_jokers, max_ante=max_ante)

    def _live_sim_evaluate(self, cards, ff, sc):
        return self.rh.sim_evaluate(cards, ff, sc)

    def _live_sim_score(self, cards, jokers, gs, dl, seed):
        return self.rh.sim_score(cards, jokers, gs, dl, seed)

    def save(self):
        rec = {"calls": np.array(self.calls), "answers": np.array(self.answers)}
        for k in OBS_KEYS:
            if self.obs_table[k]:
                rec["obs_" + k] = np.stack(self.obs_table[k])
        np.savez_compressed(log_path(self.name), **rec)


class Replayer(_Log):
    """Answers from tests/golden/reflog_<name>.npz."""

    def __init__(self, name: str):
        super().__init__(name)
        with np.load(log_path(name)) as z:
            self.calls = [str(c) for c in z["calls"]]
            self.answers = [str(a) for a in z["answers"]]
            self.obs_table = {k: z["obs_" + k] if "obs_" + k in z.files else None for k in OBS_KEYS}
        self.pos = 0

    def _call(self, call, kind, fn):
        assert self.pos < len(self.calls), f"{self.name}: the test asks the reference `{call}` after the end of the recorded log"
        want = self.calls[self.pos]
        assert call == want, f"{self.name}: call {self.pos} is `{call}`, the log recorded `{want}` (regenerate: oracle/gen_golden.py reference_logs)"
        enc = json.loads(self.answers[self.pos])
        self.pos += 1
        return self._decode(kind, enc)

    def _live_env(self, e, seed, scorer_jokers, max_ante):
        return None

    def finish(self):
        assert self.pos == len(self.calls), f"{self.name}: the test asked {self.pos} of the {len(self.calls)} recorded questions"


def reference_space_path() -> str:
    return os.path.join(GOLD, "reference_spaces.npz")


def describe_space(space) -> dict:
    """name -> arrays of a Dict space: key order, kind (class name), dtype, shape, n, and low / high flattened in their own dtype (empty where none)."""
    keys = list(space.spaces)
    out = {"keys": np.array(keys), "kind": np.array([type(space.spaces[k]).__name__ for k in keys]),
           "dtype": np.array([np.dtype(space.spaces[k].dtype).name for k in keys]),
           "shape": np.array([json.dumps(list(space.spaces[k].shape)) for k in keys]),
           "n": np.array([int(getattr(space.spaces[k], "n", -1)) for k in keys])}
    for k in keys:
        s = space.spaces[k]
        for b in ("low", "high"):
            out[f"{b}_{k}"] = np.asarray(getattr(s, b)).reshape(-1) if hasattr(s, b) else np.zeros(0)
    return out
