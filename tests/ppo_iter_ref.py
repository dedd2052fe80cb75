"""The host reference of ONE PPO ITERATION over packed records (tests/test_ppo_iteration.py on the MI355X, tests/test_ppo_iteration_host.py without one):
the chain  observe -> normalise -> policy -> act -> step -> normalise reward -> ... -> GAE -> episode statistics -> minibatches -> loss -> SGD  restated
from data that never passed through a record the product wrote.  The transitions come from the C oracle (oracle/pyoracle.py, `OracleEnv`) stepped on the
host in SB3's alignment:
    o[t]      t = 0..K   the observation BEFORE action t (o[0]: what the previous iteration left, or the reset observation); o[K] gives last_values
    mask[t]   = o[t]["action_mask"]: the mask action t was drawn under
    reward[t], done[t]   of action t; after a terminated step the env is reset inside the step (SAME_STEP), so o[t + 1] shows the new episode
The reference records rec[t] (t = 0..K) mirror the product's store: the observation o[t] packed by encode_ref.pack_records, plus reward[t - 1], a[t - 1]
and done[t - 1] (zeros for t = 0).  rec[:K] are the OBSERVATION records (encode / normalize(index=) / ppo_loss's mask), rec[1:] the REWARD records
(gae_rows / normalize_reward / EpisodeStats): one step apart.  The references of the single operators (encode_ref, norm_ref, gae_ref, head_ref, ppo_ref)
then run on those records unchanged, with their own bounds; this file adds no tolerance.

The transition driver is stated twice (`collect_literal`: SB3's collect_rollouts loop over a DummyVecEnv with Python lists, time-major, one env at a time
through OracleEnv's own dict observations; `collect_vectorised`: env-major, the oracle's observation structs read through one numpy structured view);
the host test holds the two to each other."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests import encode_ref, gae_ref, head_ref, norm_ref, ppo_ref
from tests.helpers import OBS_KEYS

STRIDE = 384
ROW_ACTION = 172
GAMMA, GAE_LAMBDA = 0.99, 0.95
CLIP, ENT_COEF, VF_COEF = 0.2, 0.01, 0.5
HIDDEN = 64

# The workload both tests run.  N = 100: no multiple of the 32-record encode workgroup, the 64-row head workgroup or the 256-env engine workgroup.
# max_ante = 1 ends an episode at the first failed or beaten Ante-1 boss, so that K = 48 steps of a near-uniform policy end a good number of episodes
# at many step positions and leave most envs mid-episode at the iteration boundary (tests/test_ppo_iteration_host.py prints the counts).
WORKLOAD = dict(N=100, K=48, iterations=2, max_ante=1, seed0=6000, net_seed=7, act_seed=20250117, perm_seed=11, batch=1000, lr=0.05)
CASES = {"produced_f32": ("produced", "float32"), "fixed_bf16": ("fixed", "bfloat16")}


# ---------------------------------------------------------------------------------------------------------------- the oracle, N envs
def make_oracles(seeds, scorer_jokers=True, max_ante=1, jokers=None):
    from oracle import pyoracle
    envs = [pyoracle.OracleEnv(int(s), scorer_jokers=scorer_jokers, max_ante=max_ante) for s in seeds]
    if jokers:
        for e, js in zip(envs, jokers):
            e.set_jokers(js)
    return envs


def _stack(dicts):
    return {k: np.stack([np.asarray(d[k]) for d in dicts]) for k in OBS_KEYS}


def collect_literal(envs, actions, jokers=None):
    """SB3's `OnPolicyAlgorithm.collect_rollouts` over a `DummyVecEnv`, literally, with Python lists: `_last_obs` is stored with the action taken from it,
    `step_wait` steps env after env and resets the one that terminated, keeping the new episode's observation.  actions int [K, N].
    -> {"obs": key -> [K + 1, N, ...], "mask": int8 [K + 1, N, 60], "reward": float64 [K, N], "done": bool [K, N]}"""
    actions = np.asarray(actions)
    K, N = actions.shape
    assert N == len(envs)
    last_obs = [e.obs() for e in envs]
    buf_obs, buf_rew, buf_done = [], [], []
    for n_steps in range(K):
        new_obs, rewards, dones = [], [], []
        for env_idx in range(N):   # DummyVecEnv.step_wait
            obs, rew, terminated, truncated, _ = envs[env_idx].step(int(actions[n_steps][env_idx]))
            done = terminated or truncated
            if done:
                obs = envs[env_idx].reset()
                if jokers:
                    envs[env_idx].set_jokers(jokers[env_idx])
                    obs = envs[env_idx].obs()
            new_obs.append(obs); rewards.append(rew); dones.append(done)
        buf_obs.append(last_obs); buf_rew.append(rewards); buf_done.append(dones)   # rollout_buffer.add(self._last_obs, actions, rewards, ...)
        last_obs = new_obs
    buf_obs.append(last_obs)   # what compute_returns_and_advantage's last_values are computed from
    obs = {k: np.stack([np.stack([np.asarray(o[k]) for o in row]) for row in buf_obs]) for k in OBS_KEYS}
    return {"obs": obs, "mask": obs["action_mask"].astype(np.int8), "reward": np.array(buf_rew, np.float64).reshape(K, N),
            "done": np.array(buf_done, bool).reshape(K, N)}


def _read_obs(L, handles):
    """The observation structs of the given oracle handles through ONE structured numpy view -> key -> [n, ...] in the reference's dtypes."""
    from oracle import pyoracle
    arr = (pyoracle.Obs * len(handles))()
    for i, h in enumerate(handles):
        L.bo_get_obs(h, C.byref(arr[i]))
    view = np.frombuffer(arr, dtype=np.dtype(pyoracle.Obs))
    return {k: np.array(view[k]).astype(pyoracle.OBS_DTYPES[k]) for k in OBS_KEYS}


def collect_vectorised(envs, actions, jokers=None):
    """The same transitions env-major (the envs are independent): every env runs its K steps into preallocated arrays through the C ABI, and each env's
    K + 1 observations are read at once from a kept array of structs."""
    from oracle import pyoracle
    L = pyoracle.lib()
    actions = np.asarray(actions)
    K, N = actions.shape
    assert N == len(envs)
    reward, done = np.zeros((K, N), np.float64), np.zeros((K, N), bool)
    obs = {k: np.zeros((K + 1, N) + pyoracle.OBS_SHAPES.get(k, ()), pyoracle.OBS_DTYPES[k]) for k in OBS_KEYS}
    r, tm, info = C.c_double(), C.c_uint8(), pyoracle.Info()
    for i, e in enumerate(envs):
        h = e.handle
        structs = (pyoracle.Obs * (K + 1))()
        L.bo_get_obs(h, C.byref(structs[0]))
        for t in range(K):
            L.bo_step(h, int(actions[t, i]), C.byref(r), C.byref(tm), C.byref(info))
            reward[t, i], done[t, i] = r.value, bool(tm.value)
            if tm.value:
                L.bo_reset(h, 0, 0)
                if jokers:
                    e.set_jokers(jokers[i])
            L.bo_get_obs(h, C.byref(structs[t + 1]))
        view = np.frombuffer(structs, dtype=np.dtype(pyoracle.Obs))
        for k in OBS_KEYS:
            obs[k][:, i] = view[k]
    return {"obs": obs, "mask": obs["action_mask"].astype(np.int8), "reward": reward, "done": done}


class OracleVec:
    """N oracle envs stepped one [N] action vector at a time (the dry run, where the policy needs o[t] before it gives a[t]); `transitions()` returns what
    was collected since the last call, in collect_*'s form, and starts the next iteration from the last observation."""

    def __init__(self, envs, jokers=None):
        from oracle import pyoracle
        self.envs, self.jokers, self.L = envs, jokers, pyoracle.lib()
        self._obs, self._rew, self._done = [self.observe()], [], []

    def observe(self):
        return _read_obs(self.L, [e.handle for e in self.envs])

    def step(self, actions):
        rew, done = np.zeros(len(self.envs), np.float64), np.zeros(len(self.envs), bool)
        for i, e in enumerate(self.envs):
            _, rew[i], done[i], _, _ = e.step(int(actions[i]))
            if done[i]:
                e.reset()
                if self.jokers:
                    e.set_jokers(self.jokers[i])
        self._obs.append(self.observe()); self._rew.append(rew); self._done.append(done)
        return self._obs[-1], rew, done

    def transitions(self):
        obs = {k: np.stack([o[k] for o in self._obs]) for k in OBS_KEYS}
        out = {"obs": obs, "mask": obs["action_mask"].astype(np.int8), "reward": np.array(self._rew, np.float64), "done": np.array(self._done, bool)}
        self._obs, self._rew, self._done = [self._obs[-1]], [], []
        return out


# ---------------------------------------------------------------------------------------------------------------- reference records
def step_records(obs_t, reward=None, action=None, done=None, stride=STRIDE):
    """One step's reference records uint8 [N, stride]: obs_t (key -> [N, ...]) packed, plus the reward / action / terminated fields of the step that led
    to it (None: the record of a reset, zeros)."""
    rows = encode_ref.pack_records(obs_t, stride).copy()
    n = rows.shape[0]
    if reward is not None:
        rows[:, gae_ref.ROW_REWARD:gae_ref.ROW_REWARD + 8] = np.ascontiguousarray(reward, np.float64).view(np.uint8).reshape(n, 8)
        rows[:, ROW_ACTION:ROW_ACTION + 4] = np.ascontiguousarray(action, np.int32).view(np.uint8).reshape(n, 4)
        rows[:, gae_ref.ROW_TERMINATED] = np.asarray(done).astype(np.uint8)
    return rows


def records(tr, actions, stride=STRIDE):
    """The reference store uint8 [K + 1, N, stride] of one iteration's transitions; [:K] the observation records, [1:] the reward records."""
    K = tr["reward"].shape[0]
    first = step_records({k: tr["obs"][k][0] for k in OBS_KEYS}, stride=stride)
    rest = [step_records({k: tr["obs"][k][t + 1] for k in OBS_KEYS}, tr["reward"][t], actions[t], tr["done"][t], stride) for t in range(K)]
    return np.stack([first] + rest)


def record_fields(rows):
    """uint8 [..., stride] records -> (key -> array, reward float64, action int32, terminated uint8) with the records' leading shape."""
    rows = np.ascontiguousarray(rows)
    lead, stride = rows.shape[:-1], rows.shape[-1]
    flat = rows.reshape(-1, stride)
    obs = {k: v.reshape(lead + v.shape[1:]) for k, v in encode_ref.unpack_records(flat).items()}
    reward = np.ascontiguousarray(flat[:, gae_ref.ROW_REWARD:gae_ref.ROW_REWARD + 8]).view(np.float64).reshape(lead)
    action = np.ascontiguousarray(flat[:, ROW_ACTION:ROW_ACTION + 4]).view(np.int32).reshape(lead)
    return obs, reward, action, flat[:, gae_ref.ROW_TERMINATED].reshape(lead)


# ---------------------------------------------------------------------------------------------------------------- VecNormalize, one call at a time
_OBS_STATE, _RET_STATE = ("obs_mean", "obs_var", "obs_count"), ("ret_mean", "ret_var", "ret_count", "returns")


def norm_obs_step(rec, moments, state):
    """VecNormalize's observation half of one step (reset() or step_wait()): obs_rms.update with the batch `moments` (float64 [2, 153]), then normalise.
    rec uint8 [N, stride].  -> (float32 [N, 153], the state with its observation statistics advanced).  norm_ref.from_moments does the arithmetic."""
    out = norm_ref.from_moments(rec[None], {"obs": np.asarray(moments)[None], "ret": np.zeros((1, 2))}, state, **norm_ref.DEFAULTS)
    new = norm_ref.copy_state(state)
    for k in _OBS_STATE:
        new[k] = out["state"][k]
    return out["obs"][0], new


def norm_reward_step(rec, moments, state):
    """The reward half: returns = returns * gamma + reward, ret_rms.update with `moments` (float64 [2]), normalise, zero the returns where done.
    -> (float64 [N], the state with its return statistics and carry advanced)."""
    out = norm_ref.from_moments(rec[None], {"obs": np.zeros((1, 2, norm_ref.COLS)), "ret": np.asarray(moments)[None]}, state, **norm_ref.DEFAULTS)
    new = norm_ref.copy_state(state)
    for k in _RET_STATE:
        new[k] = out["state"][k]
    return out["reward"][0], new


def returns_before_update(rec, state):
    """The batch whose moments the reward half takes: returns * gamma + reward, float64 [N]."""
    reward, _ = gae_ref.unpack_records(rec[None])
    return np.array(state["returns"], np.float64) * norm_ref.DEFAULTS["gamma"] + reward[0]


def frozen_features(rec, state, layout, dtype):
    """rec uint8 [m, stride] -> the bit patterns [m, D] of the records normalised with the statistics as they stand (uint32, or uint16 for bfloat16)."""
    out = norm_ref.from_moments(rec[None], None, state, training=False, **norm_ref.DEFAULTS)
    return norm_ref.obs_bits(out["obs"][0], layout, dtype)


def bits_to_float32(bits, dtype):
    """Feature bit patterns -> the float32 values a float32 network reads (bfloat16 widened exactly)."""
    return head_ref.widen_bf16(bits) if dtype == "bfloat16" else np.ascontiguousarray(bits, np.uint32).view(np.float32)


# ---------------------------------------------------------------------------------------------------------------- Monitor
def monitor_literal(reward, done, carry=None):
    """`Monitor.step`, literally, env by env: rewards appended to a list, and on done ep_rew = sum(rewards), ep_len = len(rewards).
    reward float64 [K, N], done [K, N]; carry: the per-env reward lists an earlier call left.  -> (ep_return float64 [K, N], ep_len int32 [K, N], carry)"""
    K, N = reward.shape
    carry = [[] for _ in range(N)] if carry is None else [list(c) for c in carry]
    ep_r, ep_l = np.zeros((K, N), np.float64), np.zeros((K, N), np.int32)
    for i in range(N):
        rewards = carry[i]
        for t in range(K):
            rewards.append(float(reward[t, i]))
            if done[t, i]:
                ep_r[t, i], ep_l[t, i] = sum(rewards), len(rewards)
                rewards = []
        carry[i] = rewards
    return ep_r, ep_l, carry


# ---------------------------------------------------------------------------------------------------------------- the network and the loss
def make_net(D, seed):
    """Linear(D, 64) -> Tanh -> Linear(64, 61) in float32 on the CPU, seeded: 60 logits and the value."""
    import torch
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(D, HIDDEN), torch.nn.Tanh(), torch.nn.Linear(HIDDEN, 61))


def make_case(logits, values, tr_mask, actions, old_log_prob, advantages, returns, index):
    """ppo_ref.Case of one minibatch over the stored rollout: tr_mask int8 [K, N, 60] is the ORACLE's mask of the observation each action was drawn
    from (mask[t], not the record after the step)."""
    K, N = actions.shape
    return ppo_ref.Case(np.ascontiguousarray(logits, np.float32), np.ascontiguousarray(tr_mask, np.int8).reshape(K * N, 60),
                        np.ascontiguousarray(actions, np.int32).reshape(-1), np.ascontiguousarray(old_log_prob, np.float32).reshape(-1),
                        np.ascontiguousarray(advantages, np.float32).reshape(-1), np.ascontiguousarray(values, np.float32),
                        np.ascontiguousarray(returns, np.float32).reshape(-1), np.ascontiguousarray(index, np.int32), K * N)


def minibatch_indices(K, N, batch, seed):
    """int32 slices of one torch.randperm(K * N) drawn from a seeded CPU generator (SB3's RolloutBuffer.get)."""
    import torch
    perm = torch.randperm(K * N, generator=torch.Generator().manual_seed(seed)).to(torch.int32)
    return [perm[s:s + batch].contiguous() for s in range(0, K * N, batch)]


def conditions(tr_list):
    """What keeps the test from passing vacuously, counted over the iterations' transitions: per iteration the terminated records and the distinct step
    positions they sit at; the episodes that begin in one iteration and end in the next."""
    out = {"terminated": [], "positions": [], "spanning": 0}
    started = None
    for tr in tr_list:
        done = tr["done"]
        out["terminated"].append(int(done.sum()))
        out["positions"].append(int(done.any(axis=1).sum()))
        if started is not None:   # envs that were mid-episode at the boundary (at least one step in) and end that episode in this iteration
            out["spanning"] += int((started & done.any(axis=0)).sum())
        started = ~done[-1]   # the last step of the iteration did not end an episode: the running one has at least one step
    return out
