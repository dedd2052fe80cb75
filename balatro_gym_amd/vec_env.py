"""BalatroVecEnv -- N lockstep Balatro envs on one MI355X behind the reference's reset()/step() surface.

Host-side mirror of `balatro_gym/balatro_env_2.py::BalatroEnv` (observation keys/dtypes, Discrete(60) actions, reward
/ terminated / truncated / info semantics), vectorised: every quantity gains a leading [N] axis and lives in HBM as a
torch tensor.  All game logic runs in libbalatro_mi355x.so (hand-written HIP); torch only owns device buffers and the
stream.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import random as _pyrandom
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _native as nat

_TORCH_DT = {"int8": torch.int8, "int16": torch.int16, "int32": torch.int32, "int64": torch.int64,
             "float32": torch.float32, "float64": torch.float64, "uint8": torch.uint8, "uint32": torch.uint32}


def _align(n: int, a: int = 256) -> int:
    return (n + a - 1) // a * a


def _check_out_tensor(name: str, t: Optional[torch.Tensor], dtype: torch.dtype, device: torch.device, n: int, rows: Optional[int]):
    """A caller tensor the library writes through its data_ptr(): `dtype`, on `device`, contiguous, and [n] (rows None) or [>= rows, n]."""
    if t is None:
        return
    if t.dtype != dtype or t.device != device or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor on {device} (got {t.dtype} on {t.device}"
                         f"{'' if t.is_contiguous() else ', not contiguous'})")
    ok = tuple(t.shape) == (n,) if rows is None else (t.dim() == 2 and t.shape[1] == n and t.shape[0] >= rows)
    if not ok:
        raise ValueError(f"{name} has shape {tuple(t.shape)}; expected " + (f"[{n}]" if rows is None else f"[>= {rows}, {n}] (one row per step)"))


def obs_flat_bytes(n: int, steps: int = 1) -> int:
    """Bytes of the flat observation buffer of `n` envs (every key's array, each aligned like `ObsBuffers` lays them out)."""
    off = 0
    for k in nat.OBS_KEYS:
        dt, shape = nat.OBS_SPEC[k]
        off = _align(off + n * steps * int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize)
    return off


class ObsBuffers:
    """The 31 observation arrays as views into ONE flat device byte buffer (one collective gathers all keys)."""

    def __init__(self, n: int, device: torch.device, steps: int = 1):
        self.n, self.steps = n, steps
        rows = n * steps
        off = 0
        self.layout = {}
        for k in nat.OBS_KEYS:
            dt, shape = nat.OBS_SPEC[k]
            nbytes = rows * int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize
            self.layout[k] = (off, nbytes)
            off = _align(off + nbytes)
        self.flat = torch.zeros(off, dtype=torch.uint8, device=device)
        self.tensors: Dict[str, torch.Tensor] = {}
        for k in nat.OBS_KEYS:
            dt, shape = nat.OBS_SPEC[k]
            o, nb = self.layout[k]
            lead = (steps, n) if steps > 1 else (n,)
            self.tensors[k] = self.flat[o:o + nb].view(_TORCH_DT[dt]).view(*lead, *shape)
        self.ptrs = nat.ObsPtrs(**{k: self.tensors[k].data_ptr() for k in nat.OBS_KEYS})


class RowBuffers:
    """[steps, N] packed records for `BalatroVecEnv.rollout` (bg_rollout_rows) and `step_many` (bg_step_many_rows): one 352-byte record per (step, env),
    every observation key -- plus the step's reward / action / terminated -- a strided, correctly typed VIEW of the
    same byte tensor (`tensors[key]`, `reward`, `action`, `terminated`); `.contiguous()` gives the dense per-key array.
    """

    def __init__(self, n: int, device: torch.device, steps: int = 1, row_stride: int = 0):
        """row_stride: bytes from one record to the next (a multiple of 16, >= 352; 0 = 352, densely packed).  384
        (`_native.ROW_STRIDE_LINES`) is the FAST layout: every record is written as three whole 128-byte lines (bytes 352..383 zeros),
        which the HBM takes 1.7x faster than records that end in partial lines."""
        self.n, self.steps = n, steps
        self.row_stride = int(row_stride) or nat.ROW_BYTES
        if self.row_stride < nat.ROW_BYTES or self.row_stride % 16:
            raise ValueError("row_stride must be a multiple of 16 and >= the 352-byte record")
        self.rows = torch.zeros((steps, n, self.row_stride), dtype=torch.uint8, device=device)
        self.tensors: Dict[str, torch.Tensor] = {}
        for k in nat.OBS_KEYS:
            dt, shape = nat.OBS_SPEC[k]
            self.tensors[k] = self._view(nat.ROW_OFFSETS[k], dt, shape)
        self.reward = self._view(nat.ROW_EXTRA["reward"][0], "float64", ())
        self.action = self._view(nat.ROW_EXTRA["action"][0], "int32", ())
        self.terminated = self._view(nat.ROW_EXTRA["terminated"][0], "uint8", ())
        # byte BG_ROW_END_FLAGS: why a step ended its episode (END_GAME | END_INVALID | END_MAX_STEPS, and with `progression=` END_STUCK, bit 8: the
        # ProgressionRewardWrapper's own ending), written by `step_many(..., limits=)`; 0 otherwise
        self.end_flags = self._view(nat.ROW_EXTRA["end_flags"][0], "uint8", ())
        # the ended episode's final ante (int16), round (int8) and min(chips_scored, 2**32 - 1) (uint32; `.to(torch.int64)` for arithmetic) where
        # `terminated` is set, written by `step_many(..., limits=EpisodeLimits(..., summary=True))`; 0 otherwise
        self.end_ante = self._view(*nat.ROW_EXTRA["end_ante"], ())
        self.end_round = self._view(*nat.ROW_EXTRA["end_round"], ())
        self.end_chips = self._view(*nat.ROW_EXTRA["end_chips"], ())

    def encode(self, layout: str = "produced", dtype: torch.dtype = torch.float32, out: Optional[torch.Tensor] = None, *,
               index: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The records as ONE [steps, n, D] float matrix for a policy network (`encode_rows`: one launch over all steps * n records); with `index`
        (int32 [m], one tensor of `minibatches`) the [m, D] matrix of those records, gathered inside the launch."""
        return encode_rows(self.rows, layout, dtype, out, index=index)

    def minibatches(self, batch_size: int, *, generator: Optional[torch.Generator] = None, drop_last: bool = False):
        """SB3's `RolloutBuffer.get(batch_size)`: yields int32 [<= batch_size] tensors on the records' device, consecutive slices of ONE
        torch.randperm(steps * n) (drawn on `generator`'s device, or the records' without one).  Index t * n + e names record (t, e), the order in
        which `ppo_loss(index=)` reads dense [steps, n] stored arrays: one tensor serves `encode_rows(index=)`, `normalize_obs(index=)` and
        `ppo_loss(index=)` over the OBSERVATION records -- the record each action was drawn from, one step BEFORE the record that carries its reward.  A
        `RowBuffers` filled by `step_many` / `rollout` holds the records AFTER each action (what `gae` reads): with the record before the call in front
        they make the [steps + 1, n] store whose first `steps` rows are the observation records ("One PPO iteration over records"); the
        index itself depends on steps * n alone.  The last tensor is shorter when steps * n is no multiple of batch_size; drop_last=True leaves it out."""
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        total = self.steps * self.n
        if total >= 2 ** 31:
            raise ValueError("the stored records hold at most 2**31 - 1 rows")
        dev = self.rows.device
        perm = torch.randperm(total, generator=generator, device=generator.device if generator is not None else dev).to(device=dev, dtype=torch.int32)
        for start in range(0, total, batch_size):
            if drop_last and start + batch_size > total:
                return
            yield perm[start:start + batch_size]

    def gae(self, values: torch.Tensor, last_values: torch.Tensor, gamma: float = 0.99, gae_lambda: float = 0.95,
            advantages: Optional[torch.Tensor] = None, returns: Optional[torch.Tensor] = None, timing: bool = False,
            rewards: Optional[torch.Tensor] = None):
        """(advantages, returns) float32 [steps, n] of these records (`gae_rows`: SB3's compute_returns_and_advantage in one launch)."""
        return gae_rows(self.rows, values, last_values, gamma, gae_lambda, advantages, returns, timing, rewards)

    def normalize(self, norm: "RowNormalizer", layout: str = "produced", dtype: torch.dtype = torch.float32, out: Optional[torch.Tensor] = None, *,
                  index: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The records as VecNormalize would hand them to the network, [steps, n, D] (`RowNormalizer.normalize_obs`); with `index` (int32 [m]) the
        [m, D] matrix of those records under the statistics as they stand (frozen)."""
        return norm.normalize_obs(self.rows, layout, dtype, out, index=index)

    def linear(self, layer: "RowLinear", index: Optional[torch.Tensor] = None, norm: Optional["RowNormalizer"] = None) -> torch.Tensor:
        """The first layer of the network over these records, [steps * n, H] or with `index` [m, H] (`RowLinear.forward`: bg_linear_rows, and
        bg_linear_rows_grad under autograd): the feature matrix is never written."""
        return layer(self.rows, index, norm)

    def normalize_reward(self, norm: "RowNormalizer", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The records' rewards as VecNormalize would hand them to the learner, float64 [steps, n] (`RowNormalizer.normalize_reward`)."""
        return norm.normalize_reward(self.rows, out)

    def sample(self, logits: torch.Tensor, step: int = -1, **kwargs):
        """(actions, log_prob, entropy) drawn from `logits` [n, 60] under the action mask of record row `step` (`sample_actions`; seed= and t= are
        required): the mask a record carries is the one after its step, i.e. the mask of the action to take next.  epsilon= gives the
        epsilon-greedy actions of `sample_actions(epsilon=)` instead: (actions, None, None)."""
        return sample_actions(logits, self.rows[step], **kwargs)

    def bootstrap_rewards(self, limits: "EpisodeLimits", terminal_values: torch.Tensor, gamma: float = 0.99,
                          rewards: Optional[torch.Tensor] = None) -> torch.Tensor:
        """float64 [steps, n] rewards for `gae(..., rewards=)` with SB3's time-limit bootstrap (`collect_rollouts`: rewards[idx] += gamma *
        terminal_value where the episode was truncated and not terminated): the records' rewards, or the given ones (float64 [steps, n], e.g.
        `normalize_reward`'s output; not modified), plus gamma * terminal_values[i] at entry `limits.terminal()[0][i]` wherever that step's
        `end_flags` are exactly END_MAX_STEPS.  terminal_values: float [M], the value network's output on the M records of `limits.terminal()`
        (all of them, in that order), after the `step_many(..., limits=)` call that filled these records."""
        if limits.n != self.n or limits.steps > self.steps:
            raise ValueError("limits.terminal() names steps these records do not hold (limits of other envs, or of longer calls)")
        index, _ = limits.terminal()
        if rewards is None:
            out = self.reward.clone(memory_format=torch.contiguous_format)   # (one copy of the strided view)
        else:
            _check_scan_tensor("rewards", rewards, torch.float64, (self.steps, self.n), self.rows.device)
            out = rewards.clone()
        terminal_values = torch.as_tensor(terminal_values, device=self.rows.device)
        if tuple(terminal_values.shape) != (int(index.numel()),):
            raise ValueError(f"terminal_values must have shape [{int(index.numel())}], one value per record of limits.terminal()")
        if index.numel():   # (index < limits.steps * n <= steps * n: checked above on the shapes, without reading the device)
            idx = index.long()
            only = self.end_flags.reshape(-1)[idx] == nat.END_MAX_STEPS
            out.view(-1)[idx[only]] += float(gamma) * terminal_values[only].to(torch.float64)
        return out

    def episode_stats(self, stats: "EpisodeStats"):
        """(ep_return float64, ep_len int32) [steps, n] of these records, continuing the episodes `stats` carries (`EpisodeStats.update`)."""
        return stats.update(self.rows)

    def episode_ends(self, curriculum: Optional["RowCurriculum"] = None, apply: bool = True) -> torch.Tensor:
        """The report of these records' ended episodes, int64 [32] on the device (`episode_ends`); with a `RowCurriculum` its state is advanced and
        its raised caps are set (`RowCurriculum.update`)."""
        return episode_ends(self.rows) if curriculum is None else curriculum.update(self.rows, apply=apply)

    def _view(self, off: int, dt: str, shape) -> torch.Tensor:
        item = np.dtype(dt).itemsize
        count = int(np.prod(shape, dtype=np.int64))
        v = self.rows[:, :, off:off + count * item].view(_TORCH_DT[dt])  # [steps, n, count], last dim contiguous
        return v if shape else v[:, :, 0]


class BalatroVecEnv:
    """N independent Balatro games stepped in lockstep on one GPU.

    seeds[i] plays the role of `BalatroEnv(seed=seeds[i])` (balatro_env_2.py:359): it seeds the 16 named streams
    (`(seed + 1000*i) % 2**32`, :105) and -- harness convention -- a per-env stand-in for the process-global
    `random` module with G(seed) = (seed + 16000) % 2**32.  Like the reference constructor, __init__ ends with reset().
    """

    num_actions = 60

    def __init__(self, num_envs: int, seeds: Optional[Sequence[int]] = None, *, device: int | str | torch.device = 0,
                 scorer_jokers: bool = False, autoreset: bool = True, max_ante: int = 0, info_terms: bool = True,
                 card_states: bool = False, fused_steps: int = 0, obs_layout: str = "keys"):
        """obs_layout: "keys" -- one contiguous tensor per observation key (bg_step / bg_observe, the reference's dict of arrays);
        "rows" -- ONE packed 384-byte record per env (bg_step_rows / bg_observe_rows): `obs[key]` are strided, correctly typed views of it
        (`obs_rows` is the [N, 384] byte tensor, what a policy network would concatenate anyway) and `step()` is ~10 % shorter (bench.py `step_path`)."""
        if obs_layout not in ("keys", "rows"):
            raise ValueError("obs_layout must be 'keys' or 'rows'")
        self.obs_layout = obs_layout
        if not torch.cuda.is_available():
            raise nat.NativeError("BalatroVecEnv needs a HIP device (torch.cuda.is_available() is False); "
                                  "there is no CPU fallback")
        self._L = nat.load()
        self.device = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        self.num_envs = int(num_envs)
        self.autoreset = bool(autoreset)
        self.scorer_jokers = bool(scorer_jokers)
        self.max_ante = int(max_ante)
        self.card_states = bool(card_states)
        flags = ((nat.FLAG_SCORER_JOKERS if scorer_jokers else 0) | (nat.FLAG_AUTORESET if autoreset else 0) |
                 (nat.FLAG_CARD_STATES if card_states else 0))
        self._h = C.c_void_p()
        # fused_steps: the longest rollout / step_many the caller will fuse into one launch (0 = 372-step launches): sizes the RNG
        # look-ahead rings, i.e. the HBM this handle holds (0.66 MB per env at full depth, ~42 KB per env at 16)
        rc = self._L.bg_create_ex(self.num_envs, self.device.index or 0, flags, self.max_ante, int(fused_steps), C.byref(self._h))
        if rc != 0:
            raise nat.NativeError(f"bg_create failed ({rc}): {self._L.bg_last_error(None).decode()}")
        n, dev = self.num_envs, self.device
        with torch.cuda.device(dev):
            self._obs = ObsBuffers(n, dev)
            self._rowbuf = RowBuffers(n, dev, steps=1, row_stride=nat.ROW_STRIDE_LINES) if obs_layout == "rows" else None
            self._row_tensors = {k: v[0] for k, v in self._rowbuf.tensors.items()} if self._rowbuf is not None else None
            self.reward = torch.zeros(n, dtype=torch.float64, device=dev)
            self.terminated = torch.zeros(n, dtype=torch.uint8, device=dev)
            self.truncated = torch.zeros(n, dtype=torch.uint8, device=dev)
            self.info = {k: torch.zeros((n,) + nat.INFO_SPEC[k][1], dtype=_TORCH_DT[nat.INFO_SPEC[k][0]], device=dev)
                         for k in nat.INFO_KEYS if info_terms or k not in ("reward_terms", "score_breakdown")}
            self._info_ptrs = nat.InfoPtrs(**{k: (self.info[k].data_ptr() if k in self.info else None)
                                              for k in nat.INFO_KEYS})
            self._stats = torch.zeros(6, dtype=torch.int64, device=dev)
        # the constant arguments of bg_step, converted once
        self._step_args = (C.byref(self._obs.ptrs), C.c_void_p(self.reward.data_ptr()), C.c_void_p(self.terminated.data_ptr()),
                           C.c_void_p(self.truncated.data_ptr()), C.byref(self._info_ptrs))
        if self._rowbuf is not None:
            self._rows_args = (C.c_void_p(self._rowbuf.rows.data_ptr()), C.c_uint64(self._rowbuf.row_stride))
        self.seed(seeds)
        self.reset()

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc: int, what: str):
        if rc != 0:
            raise nat.NativeError(f"{what} failed ({rc}): {self._L.bg_last_error(self._h).decode()}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @property
    def obs(self) -> Dict[str, torch.Tensor]:
        """The live observation tensors (updated in place by reset/step; clone() to keep a copy).  obs_layout "rows": views of `obs_rows`."""
        return self._row_tensors if self._row_tensors is not None else self._obs.tensors

    @property
    def obs_rows(self) -> torch.Tensor:
        """obs_layout "rows": the [N, 384] byte tensor of packed records (BG_ROW_* offsets) behind `obs`."""
        if self._rowbuf is None:
            raise AttributeError("obs_rows exists with obs_layout='rows'")
        return self._rowbuf.rows[0]

    def features(self, layout: str = "produced", dtype: torch.dtype = torch.float32, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """obs_layout "rows": the live records as the [N, D] float matrix a policy network reads (`encode_rows(env.obs_rows, ...)`)."""
        if self._rowbuf is None:
            raise ValueError("features() encodes the packed records of an obs_layout='rows' env")
        return encode_rows(self._rowbuf.rows[0], layout, dtype, out)

    def act(self, logits: torch.Tensor, *, seed: int, t: int, deterministic: bool = False, log_prob: Optional[torch.Tensor] = None,
            entropy: Optional[torch.Tensor] = None, epsilon: Optional[float] = None) -> torch.Tensor:
        """int32 [N] actions for `step()`, drawn from `logits` [N, 60] under the CURRENT action mask (`sample_actions` with index0 = 0: the live records
        of an obs_layout="rows" env, `obs["action_mask"]` otherwise), so no env takes an invalid action.  log_prob / entropy: float32 [N] tensors that
        receive what PPO stores.  epsilon: epsilon-greedy over `logits` as Q values instead (`sample_actions(epsilon=)`: DQN's exploration, per env)."""
        mask = self._rowbuf.rows[0] if self._rowbuf is not None else self._obs.tensors["action_mask"]
        return sample_actions(logits, mask, seed=seed, t=t, deterministic=deterministic, log_prob=log_prob, entropy=entropy, epsilon=epsilon)[0]

    @property
    def obs_flat(self) -> torch.Tensor:
        return self._rowbuf.rows[0].reshape(-1) if self._rowbuf is not None else self._obs.flat

    def set_gather_peers(self, buffers: Sequence[Optional[torch.Tensor]], rank: int) -> None:
        """Sharded jobs: `buffers[r]` = rank r's gather buffer (uint8 [world, N, 352]) as a tensor in THIS process -- the own one allocated here, the
        peers' opened from their CUDA IPC handles.  From now on the last launch of every packed-record `rollout` also writes every env's current
        record into slot [rank] of all of them (bg_set_gather_peers).  An empty list switches it off."""
        world = len(buffers)
        if world == 0:
            self._check(self._L.bg_set_gather_peers(self._h, None, 0, 0), "bg_set_gather_peers")
            self._gather_keep = None
            return
        for b in buffers:
            if b.dtype != torch.uint8 or tuple(b.shape) != (world, self.num_envs, nat.ROW_BYTES) or not b.is_contiguous():
                raise ValueError(f"every gather buffer must be a contiguous uint8 [{world}, {self.num_envs}, {nat.ROW_BYTES}] tensor")
        arr = (C.c_void_p * world)(*[b.data_ptr() for b in buffers])
        self._check(self._L.bg_set_gather_peers(self._h, C.cast(arr, C.c_void_p), world, int(rank)), "bg_set_gather_peers")
        self._gather_keep = list(buffers)   # the mappings must outlive the handle's use of them

    def obs_flat_bytes(self, n: int) -> int:
        """Bytes `obs_flat` takes for `n` envs in THIS env's layout: n records of `row_stride` bytes with obs_layout "rows", else the per-key
        arrays as `ObsBuffers` lays them out (what a sharded gather pads every rank's buffer to)."""
        return int(n) * self._rowbuf.row_stride if self._rowbuf is not None else obs_flat_bytes(int(n))

    def state_bytes(self) -> int:
        return int(self._L.bg_state_bytes(self._h))

    @property
    def max_fused_steps(self) -> int:
        """Steps `rollout` runs as one kernel launch (bg_max_fused_steps): the natural length of [T, N] obs buffers."""
        return int(self._L.bg_max_fused_steps(self._h))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            torch.cuda.synchronize(self.device)
            self._L.bg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ reference surface
    def seed(self, seeds: Optional[Sequence[int]] = None, mask: Optional[Sequence[bool]] = None, reseed_global: bool = True):
        """`DeterministicRNG(seed)` per env (balatro_env_2.py:84-106).  None -> `random.randint(0, 2**32-1)` (:88)."""
        n = self.num_envs
        if seeds is None:
            seeds = [_pyrandom.randint(0, 2 ** 32 - 1) for _ in range(n)]
        arr = np.ascontiguousarray(np.asarray(seeds, dtype=np.int64))
        if arr.shape != (n,):
            raise ValueError(f"seeds must have shape ({n},)")
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask, dtype=np.uint8))
        with torch.cuda.device(self.device):
            self._check(self._L.bg_seed(self._h, arr.ctypes.data_as(C.c_void_p),
                                        None if m is None else m.ctypes.data_as(C.c_void_p),
                                        1 if reseed_global else 0, self._stream()), "bg_seed")
        self.seeds = arr.copy() if mask is None else np.where(np.asarray(mask, bool), arr, getattr(self, "seeds", arr))

    def reset(self, *, seed: Optional[Sequence[int]] = None, mask: Optional[torch.Tensor] = None):
        """`reset(seed=...)` for the masked envs (all when mask is None); returns the observation dict of ALL envs."""
        if seed is not None:
            hm = None if mask is None else mask.to("cpu").numpy().astype(np.uint8)
            self.seed(seed, hm, reseed_global=False)  # reset(seed=s) rebuilds the streams, not the global module (:507-509)
        mptr = None
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            mptr = C.c_void_p(mask.data_ptr())
        with torch.cuda.device(self.device):
            if self._rowbuf is not None:
                self._check(self._L.bg_reset(self._h, mptr, None, self._stream()), "bg_reset")
                self._check(self._L.bg_observe_rows(self._h, self._rows_args[0], self._rows_args[1], self._stream()), "bg_observe_rows")
            else:
                self._check(self._L.bg_reset(self._h, mptr, C.byref(self._obs.ptrs), self._stream()), "bg_reset")
        return self.obs

    def step(self, actions: torch.Tensor):
        """One lockstep `step(action)` (balatro_env_2.py:616).  actions: int32 [N] on this device."""
        if actions.numel() != self.num_envs:
            raise ValueError(f"actions must hold {self.num_envs} elements, one per env (got {tuple(actions.shape)})")
        if actions.dtype != torch.int32 or actions.device != self.device or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=torch.int32).contiguous()
        # (no torch.cuda.device() context: every entry point of the library switches to the handle's device itself, and a step is
        #  short enough for two extra hipSetDevice calls and seven ctypes conversions to show)
        a = self._step_args
        if self._rowbuf is not None:
            r = self._rows_args
            rc = self._L.bg_step_rows(self._h, actions.data_ptr(), r[0], r[1], a[1], a[2], a[3], a[4],
                                      torch.cuda.current_stream(self.device).cuda_stream)
            if rc != 0:
                self._check(rc, "bg_step_rows")
            return self._row_tensors, self.reward, self.terminated, self.truncated, self.info
        rc = self._L.bg_step(self._h, actions.data_ptr(), a[0], a[1], a[2], a[3], a[4],
                             torch.cuda.current_stream(self.device).cuda_stream)
        if rc != 0:
            self._check(rc, "bg_step")
        return self._obs.tensors, self.reward, self.terminated, self.truncated, self.info

    def step_many(self, actions: torch.Tensor, obs_buffers: Optional["ObsBuffers"] = None, reward: Optional[torch.Tensor] = None,
                  terminated: Optional[torch.Tensor] = None, limits: Optional["EpisodeLimits"] = None,
                  progression: Optional["ProgressionRewards"] = None):
        """K consecutive `step()` calls in one launch (bg_step_many): actions int32 [K, N].  With `obs_buffers` of at least K rows
        every call's observation is kept, and so are its reward / terminated when float64 / uint8 [>= K, N] tensors on this device are
        given; the returned truncated and info are None, and so is reward / terminated when no tensor was given for it: this call
        writes none of them (a per-step output never goes into the live [N] tensors; bg_step_many with per-step info buffers gives
        the info).  Otherwise the live tensors hold the last call's observation / reward / terminated / truncated / info, and
        reward / terminated must not be given.

        A `RowBuffers` selects the packed-record engine (bg_step_many_rows: the rollout's kernel with the caller's actions, several times
        the rate of the per-key path): every step's record is kept when it has at least K rows, a one-row `RowBuffers` holds the last
        step's.  Returns (rb.tensors, rb.reward, rb.terminated, None, None) -- views of the records; `rb.action` holds the actions as
        given.  This path produces no per-step truncated / info; reward / terminated tensors are refused (the records carry them).

        limits (an `EpisodeLimits`, with a `RowBuffers` only): SafeBalatroEnv's episode limits inside the launch (bg_step_many_rows_ex).  `terminated`
        is then SB3's done, `rb.end_flags` says why, a killed step's reward is -50.0, an env the wrapper ended is reset inside the step, and
        `limits.terminal()` has the records before those resets.  With `EpisodeLimits(..., summary=True)` the record of every ended step also
        carries the ended episode's final ante, round and score (`rb.end_ante` / `rb.end_round` / `rb.end_chips`; bg_set_episode_summary).

        progression (a `ProgressionRewards`, with `limits` only): ProgressionRewardWrapper's reward shaping in front of the limits, as
        train_progressive.py stacks them (bg_step_many_rows_progress).  The records' rewards are then the shaped ones, an episode the wrapper ends
        for being stuck on ante 1 has END_STUCK in `rb.end_flags` and a terminal record like a kill; `limits` must have been made with
        `progression=True` (a stuck ending needs terminal slots of its own)."""
        if actions.dtype != torch.int32 or actions.device != self.device or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=torch.int32).contiguous()
        if actions.dim() != 2 or actions.shape[1] != self.num_envs:
            raise ValueError(f"actions must be [K, {self.num_envs}]")
        K = int(actions.shape[0])
        if isinstance(obs_buffers, RowBuffers):
            if K < 1:
                raise ValueError(f"actions must be [K, {self.num_envs}] with K >= 1")
            if obs_buffers.steps < K and obs_buffers.steps > 1:
                raise ValueError("obs_buffers has fewer rows than steps")
            if reward is not None or terminated is not None:
                raise ValueError("packed records already carry reward / action / terminated")
            if obs_buffers.n != self.num_envs or obs_buffers.rows.device != self.device:
                raise ValueError(f"obs_buffers must hold records of {self.num_envs} envs on {self.device}")
            self._stats.zero_()
            if limits is not None:
                if not isinstance(limits, EpisodeLimits) or limits.n != self.num_envs or limits.device != self.device:
                    raise ValueError(f"limits must be an EpisodeLimits of {self.num_envs} envs on {self.device}")
                if progression is not None and (not isinstance(progression, ProgressionRewards) or progression.n != self.num_envs or progression.device != self.device):
                    raise ValueError(f"progression must be a ProgressionRewards of {self.num_envs} envs on {self.device}")
                self._check(self._L.bg_set_episode_summary(self._h, 1 if limits.summary else 0), "bg_set_episode_summary")
                if progression is not None:
                    rc = self._L.bg_step_many_rows_progress(
                        self._h, K, C.c_void_p(actions.data_ptr()), C.c_void_p(obs_buffers.rows.data_ptr()), C.c_uint64(obs_buffers.row_stride),
                        1 if obs_buffers.steps > 1 else 0, C.byref(limits._struct()), C.byref(progression._struct()),
                        C.c_void_p(self._stats.data_ptr()), self._stream())
                    if rc != 0:
                        self._check(rc, "bg_step_many_rows_progress")
                else:
                    rc = self._L.bg_step_many_rows_ex(
                        self._h, K, C.c_void_p(actions.data_ptr()), C.c_void_p(obs_buffers.rows.data_ptr()), C.c_uint64(obs_buffers.row_stride),
                        1 if obs_buffers.steps > 1 else 0, C.byref(limits._struct()), C.c_void_p(self._stats.data_ptr()), self._stream())
                    if rc != 0:
                        self._check(rc, "bg_step_many_rows_ex")
                limits._terminal = None
            elif progression is not None:
                raise ValueError("progression needs limits: ProgressionRewardWrapper runs inside SafeBalatroEnv's rule (pass an EpisodeLimits)")
            else:
                rc = self._L.bg_step_many_rows(
                    self._h, K, C.c_void_p(actions.data_ptr()), C.c_void_p(obs_buffers.rows.data_ptr()), C.c_uint64(obs_buffers.row_stride),
                    1 if obs_buffers.steps > 1 else 0, C.c_void_p(self._stats.data_ptr()), self._stream())
                if rc != 0:
                    self._check(rc, "bg_step_many_rows")
            if self._rowbuf is not None:
                self.observe()   # (obs_layout "rows": the live records follow)
            return obs_buffers.tensors, obs_buffers.reward, obs_buffers.terminated, None, None
        if limits is not None or progression is not None:
            raise ValueError("limits exist on the packed-record path: pass a RowBuffers as obs_buffers")
        keep = obs_buffers is not None and obs_buffers.steps > 1
        if keep and obs_buffers.steps < K:
            raise ValueError("obs_buffers has fewer rows than steps")
        if not keep and (reward is not None or terminated is not None):
            raise ValueError("reward / terminated tensors need per-step obs_buffers: without them the live tensors hold the last call's values")
        _check_out_tensor("reward", reward, torch.float64, self.device, self.num_envs, K)
        _check_out_tensor("terminated", terminated, torch.uint8, self.device, self.num_envs, K)
        ob = obs_buffers if keep else self._obs
        # per-step outputs are [K, N]: the live [N] tensors cannot take them, an output without a per-step tensor is not written (NULL)
        rw = reward if keep else self.reward
        tm = terminated if keep else self.terminated
        with torch.cuda.device(self.device):
            self._check(self._L.bg_step_many(
                self._h, K, C.c_void_p(actions.data_ptr()), C.byref(ob.ptrs), 1 if keep else 0, None if rw is None else C.c_void_p(rw.data_ptr()),
                None if tm is None else C.c_void_p(tm.data_ptr()), None if keep else C.c_void_p(self.truncated.data_ptr()),
                None if keep else C.byref(self._info_ptrs), self._stream()), "bg_step_many")
        if self._rowbuf is not None:
            self.observe()   # (obs_layout "rows": the live records follow)
            if not keep:
                return self._row_tensors, rw, tm, self.truncated, self.info
        if keep:
            return ob.tensors, rw, tm, None, None
        return ob.tensors, rw, tm, self.truncated, self.info

    def observe(self):
        with torch.cuda.device(self.device):
            if self._rowbuf is not None:
                self._check(self._L.bg_observe_rows(self._h, self._rows_args[0], self._rows_args[1], self._stream()), "bg_observe_rows")
            else:
                self._check(self._L.bg_observe(self._h, C.byref(self._obs.ptrs), self._stream()), "bg_observe")
        return self.obs

    # ------------------------------------------------------------------ extras
    def rollout(self, steps: int, policy: int = nat.POLICY_UNIFORM, policy_seed: int = 0, env_index0: int = 0,
                t0: int = 0, obs_buffers: Optional[ObsBuffers] = None, reward: Optional[torch.Tensor] = None,
                terminated: Optional[torch.Tensor] = None, actions: Optional[torch.Tensor] = None,
                zero_stats: bool = True):
        """Fused random-policy rollout (bg_rollout).  With obs_buffers of `steps` rows every step's observation is
        kept ([T, N, ...]); otherwise the live observation tensors are overwritten each step.  A `RowBuffers` selects
        the packed-record output (bg_rollout_rows): same values, one record per (step, env).  reward / terminated / actions
        (optional; float64 / uint8 / int32, contiguous, on this device) are [>= T, N] with per-step obs_buffers, else [N]."""
        if isinstance(obs_buffers, RowBuffers):
            if obs_buffers.steps < steps and obs_buffers.steps > 1:
                raise ValueError("obs_buffers has fewer rows than steps")
            if reward is not None or terminated is not None or actions is not None:
                raise ValueError("packed records already carry reward / action / terminated")
            if zero_stats:
                self._stats.zero_()
            # (no torch.cuda.device() context, as in step(): the library switches to the handle's device itself, and on a 20-step launch the
            #  two device exchanges of the context manager are a few per cent of the call)
            rc = self._L.bg_rollout_rows(
                self._h, int(steps), int(policy), C.c_uint64(policy_seed), C.c_uint64(env_index0), C.c_uint64(t0),
                C.c_void_p(obs_buffers.rows.data_ptr()), C.c_uint64(getattr(obs_buffers, "row_stride", nat.ROW_BYTES)), 1 if obs_buffers.steps > 1 else 0,
                C.c_void_p(self._stats.data_ptr()), self._stream())
            if rc != 0:
                self._check(rc, "bg_rollout_rows")
            if self._rowbuf is not None:
                self.observe()
            return self._stats
        ob = obs_buffers or self._obs
        stride = 1 if (obs_buffers is not None and obs_buffers.steps > 1) else 0
        if stride and obs_buffers.steps < steps:
            raise ValueError("obs_buffers has fewer rows than steps")
        if not stride and steps > 1:
            # reward / terminated / actions share the observation's row stride (bg_rollout: row = env + t * N only when obs_stride_steps != 0):
            # without per-step observation buffers every step writes ROW 0 of them.  A [steps, N] tensor here would come back with one filled row.
            for name, tns in (("reward", reward), ("terminated", terminated), ("actions", actions)):
                if tns is not None and ((tns.dim() > 1 and tns.shape[0] > 1) or tns.numel() > self.num_envs):
                    raise ValueError(f"{name} has {tns.numel()} elements in shape {tuple(tns.shape)} but no per-step obs_buffers were given: every "
                                     f"step would overwrite row 0 (pass ObsBuffers(n, device, steps={steps}), or a [N] tensor for the last step's values)")
        for name, tns, dt in (("reward", reward, torch.float64), ("terminated", terminated, torch.uint8), ("actions", actions, torch.int32)):
            _check_out_tensor(name, tns, dt, self.device, self.num_envs, int(steps) if stride else None)
        if zero_stats:
            self._stats.zero_()
        with torch.cuda.device(self.device):
            self._check(self._L.bg_rollout(
                self._h, int(steps), int(policy), C.c_uint64(policy_seed), C.c_uint64(env_index0), C.c_uint64(t0),
                C.byref(ob.ptrs), stride,
                None if reward is None else C.c_void_p(reward.data_ptr()),
                None if terminated is None else C.c_void_p(terminated.data_ptr()),
                None if actions is None else C.c_void_p(actions.data_ptr()),
                C.c_void_p(self._stats.data_ptr()), self._stream()), "bg_rollout")
        if self._rowbuf is not None:
            self.observe()   # (obs_layout "rows": the live records follow)
        return self._stats

    def stats(self) -> Dict[str, int]:
        """Aggregate counters of the rollouts since the last zeroing.  Also checks the device error word (a look-ahead ring
        that ran dry would otherwise go unnoticed behind a return code of 0)."""
        self.check()
        s = self._stats.cpu().numpy()
        u = s.view(np.uint64)
        return {"steps": int(u[0]), "episodes": int(u[1]), "plays": int(u[2]), "score_sum": int(s[3]),
                "reward_bits": int(u[4]), "obs_hash": int(u[5])}

    def inject(self, jokers=None, money=None, ante=None, levels=None, mask=None, apply_now: bool = True):
        """Harness injection (reset template + optionally the live state): jokers = list of id lists per env."""
        n = self.num_envs
        jptr = nptr = mptr = aptr = lptr = kptr = None
        keep = []
        if jokers is not None:
            ja = np.zeros((n, 5), np.int32)
            na = np.zeros(n, np.int32)
            for i, js in enumerate(jokers):
                na[i] = len(js)
                ja[i, :len(js)] = js
            keep += [ja, na]
            jptr, nptr = ja.ctypes.data_as(C.c_void_p), na.ctypes.data_as(C.c_void_p)
        if money is not None:
            ma = np.ascontiguousarray(np.asarray(money, np.int64)); keep.append(ma); mptr = ma.ctypes.data_as(C.c_void_p)
        if ante is not None:
            aa = np.ascontiguousarray(np.asarray(ante, np.int32)); keep.append(aa); aptr = aa.ctypes.data_as(C.c_void_p)
        if levels is not None:
            la = np.ascontiguousarray(np.asarray(levels, np.uint8)); keep.append(la); lptr = la.ctypes.data_as(C.c_void_p)
        if mask is not None:
            ka = np.ascontiguousarray(np.asarray(mask, np.uint8)); keep.append(ka); kptr = ka.ctypes.data_as(C.c_void_p)
        with torch.cuda.device(self.device):
            self._check(self._L.bg_inject(self._h, jptr, nptr, mptr, aptr, lptr, kptr, 1 if apply_now else 0,
                                          self._stream()), "bg_inject")

    def set_max_ante(self, max_ante, mask=None):
        """`CurriculumBalatroEnv.current_max_ante` (train_balatro_agent.py:129-166): one int for every (masked) env, or one
        per env.  0 = no cap.  Takes effect from the next step on; survives reset()."""
        mk = None if mask is None else np.ascontiguousarray(np.asarray(mask, np.uint8))
        per = None
        if not np.isscalar(max_ante):
            per = np.ascontiguousarray(np.asarray(max_ante, np.int32))
            if per.shape != (self.num_envs,):
                raise ValueError(f"per-env caps must have shape ({self.num_envs},)")
        with torch.cuda.device(self.device):
            self._check(self._L.bg_set_max_ante(
                self._h, 0 if per is not None else int(max_ante), None if per is None else per.ctypes.data_as(C.c_void_p),
                None if mk is None else mk.ctypes.data_as(C.c_void_p), self._stream()), "bg_set_max_ante")
        if per is None and mask is None:
            self.max_ante = int(max_ante)

    def inject_deck(self, decks, mask=None):
        """The live deck order per env ([N, 52] card codes (rank-2)*4+suit, each row a permutation): what a harness does by
        writing env.state.deck (balatro_env_2.py:528-531).  The next reset() reshuffles."""
        da = np.ascontiguousarray(np.asarray(decks, np.uint8))
        if da.shape != (self.num_envs, 52):
            raise ValueError(f"decks must have shape ({self.num_envs}, 52)")
        mk = None if mask is None else np.ascontiguousarray(np.asarray(mask, np.uint8))
        with torch.cuda.device(self.device):
            self._check(self._L.bg_inject_deck(self._h, da.ctypes.data_as(C.c_void_p),
                                               None if mk is None else mk.ctypes.data_as(C.c_void_p), self._stream()),
                        "bg_inject_deck")
        self.observe()

    def inject_cards(self, cards, mask=None, apply_now: bool = True):
        """Card states (cards.py CardState) per env: cards[i] = iterable of (deck_index, enhancement, edition, seal) codes.
        Re-applied after every reset, like `inject` (needs card_states=True)."""
        n = self.num_envs
        enh = np.zeros((n, 52), np.uint8); edi = np.zeros((n, 52), np.uint8); seal = np.zeros((n, 52), np.uint8)
        for i, cs in enumerate(cards):
            for (idx, e, d, s) in cs:
                enh[i, idx], edi[i, idx], seal[i, idx] = e, d, s
        mk = None if mask is None else np.ascontiguousarray(np.asarray(mask, np.uint8))
        with torch.cuda.device(self.device):
            self._check(self._L.bg_inject_cards(
                self._h, enh.ctypes.data_as(C.c_void_p), edi.ctypes.data_as(C.c_void_p), seal.ctypes.data_as(C.c_void_p),
                None if mk is None else mk.ctypes.data_as(C.c_void_p), 1 if apply_now else 0, self._stream()), "bg_inject_cards")
        if apply_now:
            self.observe()

    def inject_consumables(self, consumables, mask=None, apply_now: bool = True):
        """state.consumables per env (reset template, like `inject`): consumables[i] = up to 2 ids as in
        `_get_consumable_ids` (balatro_env_2.py:1545-1567): tarots 1-22, planets 30-41, spectrals 50-67.  Tarot and
        spectral cards edit card states, so they need card_states=True."""
        n = self.num_envs
        ids = np.zeros((n, 2), np.int32)
        cnt = np.zeros(n, np.int32)
        for i, cs in enumerate(consumables):
            cnt[i] = len(cs)
            ids[i, :len(cs)] = list(cs)[:2]
        mk = None if mask is None else np.ascontiguousarray(np.asarray(mask, np.uint8))
        with torch.cuda.device(self.device):
            self._check(self._L.bg_inject_consumables(
                self._h, ids.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p),
                None if mk is None else mk.ctypes.data_as(C.c_void_p), 1 if apply_now else 0, self._stream()),
                "bg_inject_consumables")
        if apply_now:
            self.observe()

    def get_state(self, env_index: int) -> bytes:
        """save_state() (balatro_env_2.py:1575-1593) as a versioned binary blob."""
        nb = int(self._L.bg_state_blob_bytes(self._h))
        buf = (C.c_uint8 * nb)()
        self._check(self._L.bg_get_state(self._h, int(env_index), buf, nb), "bg_get_state")
        return bytes(buf)

    def set_state(self, env_index: int, blob: bytes):
        """load_state() (balatro_env_2.py:1595-1615)."""
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        self._check(self._L.bg_set_state(self._h, int(env_index), buf, len(blob)), "bg_set_state")

    # ------------------------------------------------------------------ many envs at once: checkpoint, restore, fork (bg_snapshot.h)
    @property
    def state_blob_stride(self) -> int:
        """Bytes per row of `get_states()`: the blob size (bg_state_blob_bytes) rounded up to 16."""
        return (int(self._L.bg_state_blob_bytes(self._h)) + 15) & ~15

    @staticmethod
    def _host_indices(idx, what: str) -> np.ndarray:
        """An index list (sequence, range, numpy array or tensor -- a device tensor is brought to the host) as contiguous int32."""
        if isinstance(idx, torch.Tensor):
            idx = idx.detach().to("cpu").numpy()
        a = np.asarray(idx if isinstance(idx, np.ndarray) else list(idx))
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise ValueError(f"{what} must be a one-dimensional list of integers")
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError(f"{what} must fit int32")
        return np.ascontiguousarray(a.astype(np.int32))

    def _blob_matrix(self, t: torch.Tensor, what: str) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 2 or t.device != self.device or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous uint8 [blobs, stride] tensor on {self.device}")
        return t

    def get_states(self, env_indices=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The state blobs of many envs (all when env_indices is None; repeats are allowed) as uint8 [m, stride] on this env's device, in one
        kernel launch (bg_get_states): row i is byte for byte `get_state(env_indices[i])`, then padding up to the stride, which is never written.
        `out`: a contiguous uint8 [>= m, stride] tensor on this device, stride a multiple of 16 and at least the blob size.  `torch.save` the
        result beside `RowNormalizer.state_dict()` to checkpoint a job; the caller's EpisodeLimits / EpisodeStats / RowNormalizer carries are
        not part of a blob.  `parse_state_blob` reads a row."""
        idx = None if env_indices is None else self._host_indices(env_indices, "env_indices")
        m = self.num_envs if idx is None else int(idx.size)
        if out is None:
            out = torch.empty((m, self.state_blob_stride), dtype=torch.uint8, device=self.device)
            out[:, int(self._L.bg_state_blob_bytes(self._h)):].zero_()   # (the kernel never writes the padding: a saved checkpoint is the same bytes every time)
        else:
            self._blob_matrix(out, "out")
            if out.shape[0] < m:
                raise ValueError(f"out holds {out.shape[0]} blobs, {m} are asked for")
        if m:
            self._check(self._L.bg_get_states(self._h, None if idx is None else idx.ctypes.data_as(C.c_void_p), m, C.c_void_p(out.data_ptr()),
                                              C.c_uint64(out.shape[1]), self._stream()), "bg_get_states")
        return out[:m]

    def set_states(self, env_indices, blobs: torch.Tensor, blob_index=None, observe: bool = True):
        """Restore many envs in one launch (bg_set_states): env env_indices[i] becomes blob blob_index[i] (row i when blob_index is None) of
        `blobs`, a uint8 [n, stride] tensor on this device as `get_states` returns it.  One blob may go to many envs; env_indices must be distinct.
        observe=True refreshes the live observation (`obs` / `obs_rows`) afterwards, as `inject(apply_now=True)` does."""
        idx = self._host_indices(env_indices, "env_indices")
        bidx = None if blob_index is None else self._host_indices(blob_index, "blob_index")
        if bidx is not None and bidx.size != idx.size:
            raise ValueError("blob_index must name one blob per env index")
        self._blob_matrix(blobs, "blobs")
        self._check(self._L.bg_set_states(self._h, idx.ctypes.data_as(C.c_void_p), int(idx.size), C.c_void_p(blobs.data_ptr()), C.c_uint64(blobs.shape[1]),
                                          int(blobs.shape[0]), None if bidx is None else bidx.ctypes.data_as(C.c_void_p), self._stream()), "bg_set_states")
        if observe and idx.size:
            self.observe()

    def copy_states(self, dst_indices, src_indices, source: Optional["BalatroVecEnv"] = None, observe: bool = True):
        """Env src_indices[i] of `source` (this env when None) -> env dst_indices[i] of this env, on the device and with no blob in between
        (bg_copy_states): the call a search loop makes every step.  `source` must be on the same device with the same ring depths and card-state
        flag; dst_indices must be distinct and, on one env, no dst may be the src of another pair."""
        src = self if source is None else source
        d, s = self._host_indices(dst_indices, "dst_indices"), self._host_indices(src_indices, "src_indices")
        if d.size != s.size:
            raise ValueError("dst_indices and src_indices must have the same length")
        self._check(self._L.bg_copy_states(self._h, d.ctypes.data_as(C.c_void_p), src._h, s.ctypes.data_as(C.c_void_p), int(d.size), self._stream()),
                    "bg_copy_states")
        if observe and d.size:
            self.observe()

    def fork(self, src_env: int, dst_indices, observe: bool = True):
        """Env `src_env` into every env of dst_indices (`copy_states` with one repeated source): 60 copies stepped with the 60 actions are an
        exact one-step look-ahead."""
        d = self._host_indices(dst_indices, "dst_indices")
        self.copy_states(d, np.full(d.size, int(src_env), np.int32), observe=observe)

    @staticmethod
    def parse_state_blob(blob: bytes) -> Dict[str, object]:
        """Named views of a state blob (bg_get_state): what save_state() (balatro_env_2.py:1575-1593) leaves out -- the RNG streams --
        is in here, so tests can look at a full shuffled deck, the pre-shuffled decks, the raw global-stream blocks and the shop seeds."""
        padded = not isinstance(blob, (bytes, bytearray))   # a row of `get_states` (a uint8 tensor or array) carries padding behind the blob
        if isinstance(blob, torch.Tensor):
            blob = blob.detach().to("cpu").numpy()
        b = np.ascontiguousarray(blob, np.uint8).reshape(-1) if padded else np.frombuffer(blob, np.uint8)
        hdr = b[:16].view(np.uint32)
        kg, cards, ks, kd = int(hdr[2] & 0xffff), bool(hdr[2] & 0x10000), int(hdr[3] & 0xffff), int(hdr[3] >> 16)
        out: Dict[str, object] = {"magic": int(hdr[0]), "version": int(hdr[1]), "KG": kg, "KS": ks, "KD": kd, "card_states": cards}
        off = 16

        def take(name, nbytes, dtype=np.uint8, shape=None):
            nonlocal off
            a = b[off:off + nbytes].view(dtype)
            out[name] = a.reshape(shape) if shape else a
            off += nbytes
        take("hot", nat.BLOB_NHOT * 16, np.uint32, (nat.BLOB_NHOT, 4))
        take("deck", nat.BLOB_NDECK * 16)                       # 52 card codes (rank - 2) * 4 + suit, then padding
        take("cold", nat.BLOB_NCOLD * 16)
        take("tmpl", nat.BLOB_NTMPL * 16)
        take("ring_decks", kd * nat.BLOB_NDECK * 16, np.uint8, (kd, nat.BLOB_NDECK * 16))
        take("global_blocks", kg * nat.BLOB_MTS * 4, np.uint32, (kg, nat.BLOB_MTS))   # RAW MT19937 words (tempered on read)
        take("shop_slots", ks * nat.SHOP_SLOT_WORDS * 4, np.uint32, (ks, nat.SHOP_SLOT_WORDS))
        take("shop_overflow", nat.BLOB_MTS * 4, np.uint32)
        take("deck_stream", nat.BLOB_MTS * 4, np.uint32)
        take("shopgen_stream", nat.BLOB_MTS * 4, np.uint32)
        take("shop_seed_ring", nat.BLOB_SSEED * 4, np.uint32)
        take("shop_seed_meta", 4, np.uint32)
        take("producers", 4, np.uint32)
        if cards:
            take("card_states", nat.BLOB_NCST * 16, np.uint16)
            take("card_template", nat.BLOB_NCST * 16, np.uint16)
            take("card_stream", nat.BLOB_MTS * 4, np.uint32)
            take("seal_stream", nat.BLOB_MTS * 4, np.uint32)
        if off != len(b) and not (padded and off < len(b)):   # (a row of get_states: the blob, then padding up to the stride)
            raise ValueError(f"state blob of {len(b)} bytes does not parse ({off} bytes understood)")
        out["deck"] = out["deck"][:52]
        out["ring_decks"] = out["ring_decks"][:, :52]
        out["shop_slot_seeds"] = out["shop_slots"][:, nat.SHOP_SLOT_SEED_WORD]
        hot7 = out["hot"][7]
        out["shop_slot_current"] = int(hot7[1] & 0xff)
        # words of the per-env global stream consumed since it was seeded (the block counter is a byte: modulo 256 blocks of 624 words)
        out["global_words_consumed"] = int((out["hot"][6][3] >> 24) & 0xff) * 624 + int(hot7[0] & 0xffff)
        return out

    def set_profiling(self, enable: bool):
        self._check(self._L.bg_set_profiling(self._h, 1 if enable else 0), "bg_set_profiling")

    def get_profile(self) -> Dict[str, float]:
        """Per-kernel HIP-event timings since the last call (synchronises)."""
        out = (C.c_double * 8)()
        self._check(self._L.bg_get_profile(self._h, out), "bg_get_profile")
        return {"rollout_ms": out[0], "rollout_launches": int(out[1]), "rollout_fused_steps": int(out[2]),
                "refill_ms": out[3], "refill_launches": int(out[4]), "step_ms": out[5], "step_launches": int(out[6])}

    def check(self):
        """Raise if the device reported an internal invariant violation (RNG look-ahead underflow)."""
        with torch.cuda.device(self.device):
            self._check(self._L.bg_check(self._h, self._stream()), "bg_check")


# ---------------------------------------------------------------------- operator-level entry points
def classify_batch(cards: torch.Tensor, n: torch.Tensor, lanes_per_case: int = 1, timing: bool = False):
    """`BalatroGame._classify_hand` (balatro_game.py:40-93) for M hands at once: cards uint8 [M, 8] card codes
    (rank-2)*4+suit, n uint8 [M] valid cards per row -> uint8 [M] HandType values.  Device tensors in, device tensor out.
    lanes_per_case: 1 (lane = hand) or 8 (lane = card, shuffle reductions inside 8-lane groups); identical results.
    timing=True returns (out, kernel milliseconds)."""
    L = nat.load()
    if cards.dtype != torch.uint8 or n.dtype != torch.uint8 or cards.dim() != 2 or cards.shape[1] != 8 or not cards.is_cuda \
            or tuple(n.shape) != (cards.shape[0],) or n.device != cards.device:
        raise ValueError("cards must be a uint8 [M, 8] device tensor, n a uint8 [M] tensor on the same device")
    cards, n = cards.contiguous(), n.contiguous()
    out = torch.empty(cards.shape[0], dtype=torch.uint8, device=cards.device)
    ms = C.c_float(0.0)
    with torch.cuda.device(cards.device):
        rc = L.bg_classify_batch_ex(C.c_void_p(cards.data_ptr()), C.c_void_p(n.data_ptr()), C.c_void_p(out.data_ptr()),
                                    C.c_int64(cards.shape[0]), int(lanes_per_case), C.byref(ms) if timing else None,
                                    C.c_void_p(torch.cuda.current_stream(cards.device).cuda_stream))
    if rc != 0:
        raise nat.NativeError(f"bg_classify_batch failed ({rc}): {L.bg_last_error(None).decode()}")
    return (out, float(ms.value)) if timing else out


def _check_index(index, shape: Optional[tuple], device: torch.device) -> None:
    """The `index=` of ppo_loss and encode_rows (SB3's `RolloutBuffer.get` permutation): contiguous int32 on `device`, of `shape` (None: any [m])."""
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or (tuple(index.shape) != shape if shape is not None else index.dim() != 1) \
            or not index.is_contiguous() or index.device != device:
        raise ValueError(f"index must be a contiguous torch.int32 tensor of shape {list(shape) if shape is not None else '[m]'} on {device}")


def encode_rows(rows: torch.Tensor, layout: str = "produced", dtype: torch.dtype = torch.float32, out: Optional[torch.Tensor] = None,
                timing: bool = False, *, index: Optional[torch.Tensor] = None, norm: Optional["RowNormalizer"] = None):
    """Packed records -> the float matrix a policy network reads, in one launch (bg_encode_rows).  rows: a contiguous uint8 device tensor
    [..., stride] of records as `rollout` / `step_many` / an obs_layout="rows" env write them (`RowBuffers.rows`, `env.obs_rows`).
    layout: "produced" -- the 31 observation keys in the reference's key order, every element as float (153 columns: what SB3's
    CombinedExtractor concatenates); "fixed" -- those followed by the 475 zeros of BalatroEnvFixed's never-filled keys (628);
    "extractor" -- what BalatroFeaturesExtractor.forward builds: hand one-hot, joker ids, 21 normalised state features (447).
    `_native.ENC_COLUMNS[layout]` names the column ranges.  dtype: torch.float32 or torch.bfloat16 (round to nearest even).
    out: optional [..., >= D] tensor of `dtype` on the same device with the same leading shape, last dimension contiguous and the leading
    dimensions dense over its row pitch (e.g. a column slice of a wider matrix): columns beyond D are left untouched.
    Returns the [..., D] matrix (a view of `out` when given); timing=True returns (matrix, kernel milliseconds).
    index: int32 [m] on the rows' device -- the tensor `ppo_loss(index=)` takes (`RowBuffers.minibatches`): the result (and `out`) is [m, D], row i
    made from record index[i] of the flattened rows (t * N + e names record (t, e)), gathered inside the launch (bg_encode_rows_ex); a row whose index
    is out of range is zeros, the row `ppo_loss` excludes.  norm: a `RowNormalizer`: the rows as its `normalize_obs` gives them with the statistics
    frozen ("produced" / "fixed"); its statistics, epsilon and clip_obs are read, never updated.  Without index and norm the call is bg_encode_rows."""
    if layout not in nat.ENC_LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(nat.ENC_LAYOUTS)} (got {layout!r})")
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("dtype must be torch.float32 or torch.bfloat16")
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.uint8 or rows.dim() < 1 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous uint8 tensor [..., stride] of packed records")
    stride = int(rows.shape[-1])
    if stride < nat.ROW_BYTES or stride % 16:
        raise ValueError(f"the last dimension of rows is the record stride: a multiple of 16, >= {nat.ROW_BYTES} (got {stride})")
    D = nat.ENC_COLS[nat.ENC_LAYOUTS[layout]]
    lead = tuple(rows.shape[:-1])
    store_rows = int(np.prod(lead, dtype=np.int64))
    if index is not None:
        _check_index(index, None, rows.device)
        if store_rows >= 2 ** 31:
            raise ValueError("the stored records hold at most 2**31 - 1 rows")
        lead = (int(index.shape[0]),)
    if norm is not None:
        if not isinstance(norm, RowNormalizer):
            raise ValueError("norm must be a RowNormalizer")
        if not norm.norm_obs:
            raise ValueError("this RowNormalizer was made with norm_obs=False: use encode_rows without norm")
        if layout not in ("produced", "fixed"):
            raise ValueError(f"layout must be 'produced' or 'fixed' with norm (got {layout!r}): VecNormalize wraps the env's keys, not the extractor's tensors")
        if norm.device != rows.device:
            raise ValueError(f"norm holds its statistics on {norm.device}, rows are on {rows.device}")
        if not (np.isfinite(norm.epsilon) and norm.epsilon >= 0.0 and np.isfinite(norm.clip_obs) and norm.clip_obs >= 0.0):
            raise ValueError("norm.epsilon and norm.clip_obs must be finite and >= 0")
    m = int(np.prod(lead, dtype=np.int64))
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != dtype or out.device != rows.device:
            raise ValueError(f"out must be a {dtype} tensor on {rows.device}")
        if tuple(out.shape[:-1]) != lead or out.shape[-1] < D:
            raise ValueError(f"out must have shape {lead + ('>= %d' % D,)} (got {tuple(out.shape)})")
        pitch = int(out.stride(-2)) if out.dim() >= 2 else int(out.shape[-1])
        dense = out.stride(-1) == 1 and pitch >= out.shape[-1]
        for d in range(out.dim() - 2, 0, -1):   # leading dimensions: one run of rows `pitch` elements apart
            dense = dense and out.stride(d - 1) == out.stride(d) * out.shape[d]
        if not dense:
            raise ValueError("out must have a contiguous last dimension and leading dimensions that are dense over its row pitch")
    if not rows.is_cuda:
        raise ValueError("rows must be a device tensor (there is no CPU fallback)")
    if rows.data_ptr() % 16:
        raise ValueError("rows must be 16-byte aligned")
    if out is None:
        out = torch.empty(lead + (D,), dtype=dtype, device=rows.device)
        pitch = D
    if m == 0:   # nothing to launch (an empty tensor has no pointer to hand over)
        return (out[..., :D], 0.0) if timing else out[..., :D]
    L = nat.load()
    ms = C.c_float(0.0)
    odt = nat.ENC_F32 if dtype == torch.float32 else nat.ENC_BF16
    tail = (C.c_void_p(out.data_ptr()), C.c_uint64(pitch), C.byref(ms) if timing else None, C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream))
    with torch.cuda.device(rows.device):
        if index is None and norm is None:
            name = "bg_encode_rows"
            rc = L.bg_encode_rows(C.c_void_p(rows.data_ptr()), C.c_uint64(stride), C.c_int64(m), nat.ENC_LAYOUTS[layout], odt, *tail)
        else:
            name = "bg_encode_rows_ex"
            rc = L.bg_encode_rows_ex(C.c_void_p(rows.data_ptr()), C.c_uint64(stride), C.c_int64(store_rows),
                                     C.c_void_p(index.data_ptr()) if index is not None else None, C.c_int64(m), nat.ENC_LAYOUTS[layout], odt,
                                     C.c_void_p(norm.obs_mean.data_ptr()) if norm is not None else None,
                                     C.c_void_p(norm.obs_var.data_ptr()) if norm is not None else None,
                                     C.c_double(norm.epsilon if norm is not None else 0.0), C.c_double(norm.clip_obs if norm is not None else 0.0), *tail)
    if rc != 0:
        raise nat.NativeError(f"{name} failed ({rc}): {L.bg_last_error(None).decode()}")
    res = out[..., :D]
    return (res, float(ms.value)) if timing else res


def _linear_common(rows, index, norm, layout, activation):
    """The arguments linear_rows and its gradient share -> (stride, store_rows, m).  Every refusal is a ValueError before the library is loaded."""
    if layout not in ("produced", "fixed"):
        raise ValueError(f"layout must be 'produced' or 'fixed' (got {layout!r}): the extractor's one-hot columns want an embedding gather, not this layer")
    if activation not in nat.LIN_ACTIVATIONS:
        raise ValueError(f"activation must be None or 'relu' (got {activation!r}): tanh stays in torch")
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.uint8 or rows.dim() < 1 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous uint8 tensor [..., stride] of packed records")
    stride = int(rows.shape[-1])
    if stride < nat.ROW_BYTES or stride % 16:
        raise ValueError(f"the last dimension of rows is the record stride: a multiple of 16, >= {nat.ROW_BYTES} (got {stride})")
    store_rows = int(np.prod(tuple(rows.shape[:-1]), dtype=np.int64))
    m = store_rows
    if index is not None:
        _check_index(index, None, rows.device)
        if store_rows >= 2 ** 31:
            raise ValueError("the stored records hold at most 2**31 - 1 rows")
        m = int(index.shape[0])
    if norm is not None:
        if not isinstance(norm, RowNormalizer):
            raise ValueError("norm must be a RowNormalizer")
        if not norm.norm_obs:
            raise ValueError("this RowNormalizer was made with norm_obs=False: call without norm")
        if norm.device != rows.device:
            raise ValueError(f"norm holds its statistics on {norm.device}, rows are on {rows.device}")
        if not (np.isfinite(norm.epsilon) and norm.epsilon >= 0.0 and np.isfinite(norm.clip_obs) and norm.clip_obs >= 0.0):
            raise ValueError("norm.epsilon and norm.clip_obs must be finite and >= 0")
    return stride, store_rows, m


def _linear_matrix(name: str, t, dtypes: tuple, m: int, H: int, device: torch.device) -> int:
    """A [m, >= H] matrix with a contiguous last dimension -> its row pitch in elements."""
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.device != device or t.dim() != 2 or t.shape[0] != m or t.shape[1] < H \
            or t.stride(1) != 1 or (m > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f"{name} must be a {' / '.join(str(d) for d in dtypes)} tensor [{m}, >= {H}] on {device} with a contiguous last dimension")
    return int(t.stride(0)) if m > 1 else int(t.shape[1])


def _linear_weight(weight) -> int:
    if not isinstance(weight, torch.Tensor) or weight.dtype != torch.bfloat16 or weight.dim() != 2 or weight.shape[1] not in (nat.LIN_K, nat.ENC_COLS[nat.ENC_FIXED]) \
            or not weight.is_contiguous():
        raise ValueError("weight must be a contiguous torch.bfloat16 tensor [H, 153] or [H, 628] (nn.Linear.weight's orientation)")
    H = int(weight.shape[0])
    if H < 32 or H > 4096 or H % 32:
        raise ValueError(f"the layer's width must be a multiple of 32 in [32, 4096] (got {H})")
    return H


def _linear_rows_args(rows, index, norm):
    return (C.c_void_p(norm.obs_mean.data_ptr()) if norm is not None else None, C.c_void_p(norm.obs_var.data_ptr()) if norm is not None else None,
            C.c_double(norm.epsilon if norm is not None else 0.0), C.c_double(norm.clip_obs if norm is not None else 0.0))


def linear_rows(rows: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, index: Optional[torch.Tensor] = None,
                norm: Optional["RowNormalizer"] = None, layout: str = "fixed", activation: Optional[str] = None, dtype: torch.dtype = torch.bfloat16,
                out: Optional[torch.Tensor] = None, timing: bool = False):
    """The network's first layer straight from packed records, on the matrix cores, in one launch (bg_linear_rows):
    act(x @ weight[:, :153].T + bias), x the bfloat16 rows `encode_rows(rows, layout, torch.bfloat16, index=index, norm=norm)` gives -- which are never
    written.  weight: torch.bfloat16 [H, 153] or [H, 628] (nn.Linear.weight's orientation; of 628 columns only the first 153 are read: the others meet the
    475 zeros of the "fixed" layout), H a multiple of 32 in [32, 4096]; bias: float32 [H] or None; activation: None or "relu".  layout "fixed" or
    "produced": the same result.  index / norm: as `encode_rows`; a row whose index is out of range is act(bias).  dtype: torch.bfloat16 or
    torch.float32 (float32 accumulation either way, one rounding).  out: optional [m, >= H] tensor of `dtype`; columns beyond H are left untouched.
    Returns the [m, H] matrix (m = all records flattened, or len(index)); timing=True returns (matrix, kernel milliseconds).  There is no CPU path."""
    stride, store_rows, m = _linear_common(rows, index, norm, layout, activation)
    H = _linear_weight(weight)
    if weight.device != rows.device:
        raise ValueError(f"weight must be on {rows.device}")
    if bias is not None and (not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or tuple(bias.shape) != (H,) or not bias.is_contiguous()
                             or bias.device != rows.device):
        raise ValueError(f"bias must be a contiguous torch.float32 tensor [{H}] on {rows.device}")
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("dtype must be torch.float32 or torch.bfloat16")
    pitch = _linear_matrix("out", out, (dtype,), m, H, rows.device) if out is not None else H
    if not rows.is_cuda:
        raise ValueError("rows must be a device tensor (there is no CPU fallback)")
    if rows.data_ptr() % 16:
        raise ValueError("rows must be 16-byte aligned")
    if out is None:
        out = torch.empty((m, H), dtype=dtype, device=rows.device)
    if m == 0:
        return (out[:, :H], 0.0) if timing else out[:, :H]
    L = nat.load()
    ms = C.c_float(0.0)
    with torch.cuda.device(rows.device):
        rc = L.bg_linear_rows(C.c_void_p(rows.data_ptr()), C.c_uint64(stride), C.c_int64(store_rows), C.c_void_p(index.data_ptr()) if index is not None else None,
                              C.c_int64(m), nat.ENC_LAYOUTS[layout], *_linear_rows_args(rows, index, norm), C.c_void_p(weight.data_ptr()),
                              C.c_uint64(int(weight.shape[1])), C.c_void_p(bias.data_ptr()) if bias is not None else None, H, nat.LIN_ACTIVATIONS[activation],
                              nat.ENC_F32 if dtype == torch.float32 else nat.ENC_BF16, C.c_void_p(out.data_ptr()), C.c_uint64(pitch),
                              C.byref(ms) if timing else None, C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream))
    if rc != 0:
        raise nat.NativeError(f"bg_linear_rows failed ({rc}): {L.bg_last_error(None).decode()}")
    return (out[:, :H], float(ms.value)) if timing else out[:, :H]


def linear_rows_grad(rows: torch.Tensor, dout: torch.Tensor, *, out: Optional[torch.Tensor] = None, index: Optional[torch.Tensor] = None,
                     norm: Optional["RowNormalizer"] = None, layout: str = "fixed", activation: Optional[str] = None, dweight: Optional[torch.Tensor] = None,
                     bias: bool = True, workspace: Optional[torch.Tensor] = None, timing: bool = False):
    """The weight and bias gradient of `linear_rows`, straight from the records (bg_linear_rows_grad): dweight[n, k] = sum_i dp[i, n] * x[i, k],
    dbias[n] = sum_i dp[i, n], dp = bfloat16(dout), under activation="relu" masked where the forward's `out` (required then) is not > 0.  dout: float32 or
    bfloat16 [m, >= H].  dweight: optional float32 [H, 153] or [H, 628] (columns beyond 153 are not written); without one a zero-filled [H, 628] ("fixed")
    or [H, 153] ("produced") is made, so the columns beyond 153 carry their exact gradient, zero.  Returns (dweight, dbias or None) -- with timing=True
    (dweight, dbias, kernel milliseconds).  Sums over rows are deterministic (no atomics)."""
    stride, store_rows, m = _linear_common(rows, index, norm, layout, activation)
    if not isinstance(dout, torch.Tensor) or dout.dim() != 2:
        raise ValueError("dout must be a float32 / bfloat16 tensor [m, H]")
    H = int(dweight.shape[0]) if isinstance(dweight, torch.Tensor) and dweight.dim() == 2 else int(dout.shape[1])
    if H < 32 or H > 4096 or H % 32:
        raise ValueError(f"the layer's width must be a multiple of 32 in [32, 4096] (got {H})")
    dpitch = _linear_matrix("dout", dout, (torch.float32, torch.bfloat16), m, H, rows.device)
    relu = activation == "relu"
    if relu != (out is not None):
        raise ValueError("out (the forward's output) is required with activation='relu' and must be None without it")
    opitch = _linear_matrix("out", out, (torch.float32, torch.bfloat16), m, H, rows.device) if relu else 0
    if dweight is not None and (not isinstance(dweight, torch.Tensor) or dweight.dtype != torch.float32 or dweight.dim() != 2 or dweight.shape[1] < nat.LIN_K
                                or not dweight.is_contiguous() or dweight.device != rows.device):
        raise ValueError(f"dweight must be a contiguous torch.float32 tensor [H, >= {nat.LIN_K}] on {rows.device}")
    if not rows.is_cuda:
        raise ValueError("rows must be a device tensor (there is no CPU fallback)")
    if rows.data_ptr() % 16:
        raise ValueError("rows must be 16-byte aligned")
    if dweight is None:
        dweight = torch.zeros((H, nat.ENC_COLS[nat.ENC_LAYOUTS[layout]]), dtype=torch.float32, device=rows.device)
    dbias = torch.zeros(H, dtype=torch.float32, device=rows.device) if bias else None
    if m == 0:
        dweight[:, :nat.LIN_K] = 0.0
        return (dweight, dbias, 0.0) if timing else (dweight, dbias)
    L = nat.load()
    need = int(L.bg_linear_rows_workspace_bytes(C.c_int64(m), H))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=rows.device)
    elif not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != rows.device or not workspace.is_contiguous() \
            or workspace.numel() < need:
        raise ValueError(f"workspace must be a contiguous uint8 tensor of >= {need} bytes on {rows.device}")
    ms = C.c_float(0.0)
    with torch.cuda.device(rows.device):
        rc = L.bg_linear_rows_grad(C.c_void_p(rows.data_ptr()), C.c_uint64(stride), C.c_int64(store_rows), C.c_void_p(index.data_ptr()) if index is not None else None,
                                   C.c_int64(m), nat.ENC_LAYOUTS[layout], *_linear_rows_args(rows, index, norm), C.c_void_p(dout.data_ptr()),
                                   nat.ENC_F32 if dout.dtype == torch.float32 else nat.ENC_BF16, C.c_uint64(dpitch),
                                   C.c_void_p(out.data_ptr()) if relu else None, (nat.ENC_F32 if out.dtype == torch.float32 else nat.ENC_BF16) if relu else 0,
                                   C.c_uint64(opitch), H, nat.LIN_ACTIVATIONS[activation], C.c_void_p(dweight.data_ptr()), C.c_uint64(int(dweight.shape[1])),
                                   C.c_void_p(dbias.data_ptr()) if bias else None, C.c_void_p(workspace.data_ptr()), C.c_uint64(workspace.numel()),
                                   C.byref(ms) if timing else None, C.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream))
    if rc != 0:
        raise nat.NativeError(f"bg_linear_rows_grad failed ({rc}): {L.bg_last_error(None).decode()}")
    return (dweight, dbias, float(ms.value)) if timing else (dweight, dbias)


class _RowLinearFn(torch.autograd.Function):
    """out = linear_rows(records); backward = ONE bg_linear_rows_grad call.  The records carry no gradient."""

    @staticmethod
    def forward(ctx, weight, bias, rows, index, norm, layout, activation, dtype):
        out = linear_rows(rows, weight.detach().to(torch.bfloat16), bias.detach() if bias is not None else None, index=index, norm=norm, layout=layout,
                          activation=activation, dtype=dtype)
        ctx.save_for_backward(out)
        ctx.call = (rows, index, norm, layout, activation, tuple(weight.shape), bias is not None)
        return out

    @staticmethod
    def backward(ctx, grad):
        rows, index, norm, layout, activation, wshape, has_bias = ctx.call
        out, = ctx.saved_tensors
        dout = grad if grad.dtype in (torch.float32, torch.bfloat16) and grad.dim() == 2 and grad.stride(1) == 1 and (grad.shape[0] <= 1 or grad.stride(0) >= grad.shape[1]) \
            else grad.to(torch.float32).contiguous()
        dweight = torch.zeros(wshape, dtype=torch.float32, device=rows.device)   # columns at or beyond 153: zero, their exact gradient
        dweight, dbias = linear_rows_grad(rows, dout, out=out if activation == "relu" else None, index=index, norm=norm, layout=layout, activation=activation,
                                          dweight=dweight, bias=has_bias)
        return dweight, dbias, None, None, None, None, None, None


class RowLinear(torch.nn.Module):
    """The first `nn.Linear` of a policy over packed records: `forward(rows)` is `linear_rows` and its backward one `linear_rows_grad` call, so neither pass
    materialises the feature matrix.  Parameters are float32 -- weight [out_features, 628] ("fixed": SB3's MultiInputPolicy over BalatroEnvFixed) or
    [out_features, 153] ("produced"), bias [out_features] -- initialised as nn.Linear; `from_linear` / `to_linear` move them to and from an nn.Linear, so a
    policy trained here loads into SB3's module and back.  The weight is cast to bfloat16 for every call (the master copy stays float32); columns at or
    beyond 153 of a 628-wide weight get a zero gradient, which is their exact gradient: their inputs are zero."""

    def __init__(self, out_features: int, in_layout: str = "fixed", activation: Optional[str] = None, dtype: torch.dtype = torch.bfloat16, device=None):
        super().__init__()
        if in_layout not in ("produced", "fixed"):
            raise ValueError(f"in_layout must be 'produced' or 'fixed' (got {in_layout!r})")
        if activation not in nat.LIN_ACTIVATIONS:
            raise ValueError(f"activation must be None or 'relu' (got {activation!r}): tanh stays in torch")
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("dtype must be torch.float32 or torch.bfloat16")
        out_features = int(out_features)
        if out_features < 32 or out_features > 4096 or out_features % 32:
            raise ValueError(f"out_features must be a multiple of 32 in [32, 4096] (got {out_features})")
        self.out_features, self.in_layout, self.activation, self.dtype = out_features, in_layout, activation, dtype
        self.in_features = nat.ENC_COLS[nat.ENC_LAYOUTS[in_layout]]
        lin = torch.nn.Linear(self.in_features, out_features, device=device)   # nn.Linear's own initialisation
        self.weight = torch.nn.Parameter(lin.weight.detach().clone())
        self.bias = torch.nn.Parameter(lin.bias.detach().clone())

    @classmethod
    def from_linear(cls, linear: torch.nn.Linear, activation: Optional[str] = None, dtype: torch.dtype = torch.bfloat16) -> "RowLinear":
        if not isinstance(linear, torch.nn.Linear) or linear.in_features not in (nat.LIN_K, nat.ENC_COLS[nat.ENC_FIXED]) or linear.bias is None:
            raise ValueError("from_linear takes an nn.Linear with bias and 153 ('produced') or 628 ('fixed') inputs")
        layer = cls(linear.out_features, "produced" if linear.in_features == nat.LIN_K else "fixed", activation, dtype, device=linear.weight.device)
        with torch.no_grad():
            layer.weight.copy_(linear.weight)
            layer.bias.copy_(linear.bias)
        return layer

    def to_linear(self) -> torch.nn.Linear:
        lin = torch.nn.Linear(self.in_features, self.out_features, device=self.weight.device)
        with torch.no_grad():
            lin.weight.copy_(self.weight)
            lin.bias.copy_(self.bias)
        return lin

    def forward(self, rows: torch.Tensor, index: Optional[torch.Tensor] = None, norm: Optional["RowNormalizer"] = None) -> torch.Tensor:
        _linear_common(rows, index, norm, self.in_layout, self.activation)
        if not rows.is_cuda or self.weight.device != rows.device:
            raise ValueError("rows and the layer must be on the same GPU (there is no CPU fallback)")
        return _RowLinearFn.apply(self.weight, self.bias, rows, index, norm, self.in_layout, self.activation, self.dtype)

    def extra_repr(self) -> str:
        return f"in_layout={self.in_layout!r}, out_features={self.out_features}, activation={self.activation!r}, dtype={self.dtype}"


def _head_logits(logits) -> tuple:
    """logits of sample_actions / evaluate_actions: float32 / bfloat16 [..., 60] with a contiguous last dimension and leading dimensions dense over the
    row pitch (e.g. 60 columns of a wider matrix) -> (leading shape, m, row pitch in elements)."""
    if not isinstance(logits, torch.Tensor) or logits.dtype not in (torch.float32, torch.bfloat16) or logits.dim() < 1 or logits.shape[-1] != 60:
        raise ValueError("logits must be a float32 or bfloat16 tensor [..., 60]")
    pitch = int(logits.stride(-2)) if logits.dim() >= 2 else 60
    dense = logits.stride(-1) == 1 and pitch >= 60
    for d in range(logits.dim() - 2, 0, -1):   # leading dimensions: one run of rows `pitch` elements apart
        dense = dense and logits.stride(d - 1) == logits.stride(d) * logits.shape[d]
    if not dense:
        raise ValueError("logits must have a contiguous last dimension and leading dimensions that are dense over its row pitch")
    lead = tuple(logits.shape[:-1])
    return lead, int(np.prod(lead, dtype=np.int64)), pitch


def _head_mask(mask, lead: tuple, device: torch.device) -> tuple:
    """mask of sample_actions / evaluate_actions -> (tensor to keep alive, byte offset of the first row's mask, row pitch in bytes): packed records
    (a contiguous uint8 tensor [..., stride], recognised as encode_rows recognises them), an int8 [..., 60] matrix, or None."""
    if mask is None:
        return None, 0, 0
    if not isinstance(mask, torch.Tensor) or mask.dim() < 1:
        raise ValueError("mask must be a uint8 tensor [..., stride] of packed records, an int8 tensor [..., 60] or None")
    if mask.dtype == torch.uint8:
        stride = int(mask.shape[-1])
        if not mask.is_contiguous() or stride < nat.ROW_BYTES or stride % 16:
            raise ValueError(f"a uint8 mask is a contiguous tensor [..., stride] of packed records: stride a multiple of 16, >= {nat.ROW_BYTES}")
        off = nat.ROW_OFFSETS["action_mask"]
    elif mask.dtype == torch.int8 and mask.shape[-1] == 60:
        stride = int(mask.stride(-2)) if mask.dim() >= 2 else 60
        dense = mask.stride(-1) == 1 and stride >= 60
        for d in range(mask.dim() - 2, 0, -1):
            dense = dense and mask.stride(d - 1) == mask.stride(d) * mask.shape[d]
        if not dense or stride % 4:
            raise ValueError("an int8 mask must have a contiguous last dimension and leading dimensions dense over a row pitch that is a multiple of 4")
        off = 0
    else:
        raise ValueError("mask must be a uint8 tensor [..., stride] of packed records, an int8 tensor [..., 60] or None")
    if tuple(mask.shape[:-1]) != lead:
        raise ValueError(f"mask must have the leading shape of logits {list(lead)} (got {list(mask.shape[:-1])})")
    if mask.device != device:
        raise ValueError(f"mask must be on {device}")
    return mask, off, stride


def _head_call(name: str, logits, mask, given, flags: int, seed: int, index0: int, t: int, actions, log_prob, entropy, timing: bool,
               epsilon: Optional[float] = None):
    lead, m, pitch = _head_logits(logits)
    dev = logits.device
    mask, moff, mstride = _head_mask(mask, lead, dev)
    if epsilon is not None:
        return _head_call_eps(logits, lead, m, pitch, mask, moff, mstride, flags, seed, index0, t, actions, log_prob, entropy, timing, epsilon)
    for what, v in (("seed", seed), ("index0", index0), ("t", t)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= int(v) < 2 ** 64:
            raise ValueError(f"{what} must be an integer in [0, 2**64)")
    if given is not None:
        _check_scan_tensor("actions", given, torch.int32, lead, dev)
    for what, tt, dt in (("actions", actions, torch.int32), ("log_prob", log_prob, torch.float32), ("entropy", entropy, torch.float32)):
        if tt is not None:
            _check_scan_tensor(what, tt, dt, lead, dev)
    if not logits.is_cuda:
        raise ValueError("logits must be a device tensor (there is no CPU fallback)")
    if mask is not None and (mask.data_ptr() + moff) % 4:
        raise ValueError("mask must be 4-byte aligned")
    if given is None and actions is None:
        actions = torch.empty(lead, dtype=torch.int32, device=dev)
    if log_prob is None:
        log_prob = torch.empty(lead, dtype=torch.float32, device=dev)
    if entropy is None:
        entropy = torch.empty(lead, dtype=torch.float32, device=dev)
    res = (log_prob, entropy) if given is not None else (actions, log_prob, entropy)
    if m == 0:   # nothing to launch (an empty tensor has no pointer to hand over)
        return res + (0.0,) if timing else res
    outs = [x.data_ptr() for x in res]
    ins = [logits.data_ptr()] + ([mask.data_ptr()] if mask is not None else []) + ([given.data_ptr()] if given is not None else [])
    if len(set(outs)) != len(outs) or set(outs) & set(ins):
        raise ValueError("outputs must not share memory with the inputs or with each other")
    L = nat.load()
    ms = C.c_float(0.0)
    with torch.cuda.device(dev):
        head = (C.c_void_p(logits.data_ptr()), nat.HEAD_F32 if logits.dtype == torch.float32 else nat.HEAD_BF16, C.c_uint64(pitch),
                C.c_void_p(mask.data_ptr() + moff) if mask is not None else None, C.c_uint64(mstride), C.c_int64(m))
        tail = (C.c_void_p(log_prob.data_ptr()), C.c_void_p(entropy.data_ptr()), C.byref(ms) if timing else None,
                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if given is None:
            rc = L.bg_sample_actions(*head, C.c_uint32(flags), C.c_uint64(int(seed)), C.c_uint64(int(index0)), C.c_uint64(int(t)),
                                     C.c_void_p(actions.data_ptr()), *tail)
        else:
            rc = L.bg_evaluate_actions(*head, C.c_void_p(given.data_ptr()), *tail)
    if rc != 0:
        raise nat.NativeError(f"{name} failed ({rc}): {L.bg_last_error(None).decode()}")
    return res + (float(ms.value),) if timing else res


def _head_call_eps(logits, lead, m, pitch, mask, moff, mstride, flags, seed, index0, t, actions, log_prob, entropy, timing, epsilon):
    """bg_sample_actions_eps: the checks of `_head_call` for the sampling form, then the epsilon-greedy launch -> (actions, None, None)."""
    dev = logits.device
    if isinstance(epsilon, bool) or not isinstance(epsilon, (int, float, np.integer, np.floating)) or not 0.0 <= float(epsilon) <= 1.0:
        raise ValueError("epsilon must be a number in [0, 1] (or None: the categorical head)")
    if flags:
        raise ValueError("epsilon and deterministic=True exclude each other (epsilon=0.0 is the greedy rule)")
    if log_prob is not None or entropy is not None:
        raise ValueError("an epsilon-greedy action has no categorical log_prob / entropy: pass neither with epsilon")
    for what, v in (("seed", seed), ("index0", index0), ("t", t)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= int(v) < 2 ** 64:
            raise ValueError(f"{what} must be an integer in [0, 2**64)")
    if actions is not None:
        _check_scan_tensor("actions", actions, torch.int32, lead, dev)
    if not logits.is_cuda:
        raise ValueError("logits must be a device tensor (there is no CPU fallback)")
    if mask is not None and (mask.data_ptr() + moff) % 4:
        raise ValueError("mask must be 4-byte aligned")
    if actions is None:
        actions = torch.empty(lead, dtype=torch.int32, device=dev)
    res = (actions, None, None)
    if m == 0:
        return res + (0.0,) if timing else res
    if actions.data_ptr() in {logits.data_ptr()} | ({mask.data_ptr()} if mask is not None else set()):
        raise ValueError("outputs must not share memory with the inputs or with each other")
    L = nat.load()
    ms = C.c_float(0.0)
    with torch.cuda.device(dev):
        rc = L.bg_sample_actions_eps(C.c_void_p(logits.data_ptr()), nat.HEAD_F32 if logits.dtype == torch.float32 else nat.HEAD_BF16, C.c_uint64(pitch),
                                     C.c_void_p(mask.data_ptr() + moff) if mask is not None else None, C.c_uint64(mstride), C.c_int64(m), C.c_uint32(0),
                                     C.c_uint64(int(seed)), C.c_uint64(int(index0)), C.c_uint64(int(t)), C.c_float(float(epsilon)),
                                     C.c_void_p(actions.data_ptr()), None, None, C.byref(ms) if timing else None,
                                     C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise nat.NativeError(f"bg_sample_actions_eps failed ({rc}): {L.bg_last_error(None).decode()}")
    return res + (float(ms.value),) if timing else res


def sample_actions(logits: torch.Tensor, mask: Optional[torch.Tensor] = None, *, seed: int, t: int, index0: int = 0, deterministic: bool = False,
                   actions: Optional[torch.Tensor] = None, log_prob: Optional[torch.Tensor] = None, entropy: Optional[torch.Tensor] = None,
                   timing: bool = False, epsilon: Optional[float] = None):
    """The masked categorical policy head in one launch (bg_sample_actions): logits float32 / bfloat16 [..., 60] -> (actions int32, log_prob float32,
    entropy float32), each [...].  mask: packed records (a contiguous uint8 tensor [..., stride]: `RowBuffers.rows[t]`, `env.obs_rows` -- their
    action_mask field is read in place), an int8 [..., 60] matrix (`obs["action_mask"]`) or None (every action valid).  A masked action is never
    drawn; a row with no valid action (or a NaN / +inf valid logit) gives action -1 and NaN.  Row i draws with the counter hash of (seed, index0 + i,
    t), the rollout's: the same arguments give the same bits, whatever the batch shape or sharding (a shard passes its first global env as index0).
    deterministic=True takes the first valid maximum instead (SB3's `mode()`).  A record's mask is the mask AFTER its step: it goes with the logits
    computed from that record.  actions / log_prob / entropy: optional contiguous tensors to write into.  timing=True appends kernel milliseconds.
    epsilon (None: the categorical head above, untouched): epsilon-greedy over the logits as Q values (bg_sample_actions_eps) -> (actions, None,
    None).  Row i explores when its uniform draw u -- the one the categorical head would use -- is below epsilon, and then takes a uniformly drawn
    valid action from a second hash; otherwise the first valid maximum.  The decision is PER ENV (SB3's DQN draws once for the whole batch, which
    at 65 536 envs would make every env explore together).  epsilon excludes deterministic=True, log_prob and entropy."""
    return _head_call("bg_sample_actions", logits, mask, None, nat.HEAD_DETERMINISTIC if deterministic else 0, seed, index0, t, actions, log_prob,
                      entropy, timing, epsilon)


def evaluate_actions(logits: torch.Tensor, actions: torch.Tensor, mask: Optional[torch.Tensor] = None, *, log_prob: Optional[torch.Tensor] = None,
                     entropy: Optional[torch.Tensor] = None, timing: bool = False):
    """(log_prob, entropy) float32 [...] of given int32 actions [...] under the masked distribution of `sample_actions` (bg_evaluate_actions; a
    forward pass -- `ppo_loss` is the call that takes part in autograd): bit for bit what the sampler returned for the actions it drew.  A masked
    action has log_prob -inf, one outside [0, 60) NaN."""
    if not isinstance(actions, torch.Tensor):
        raise ValueError("actions must be an int32 tensor with the leading shape of logits")
    return _head_call("bg_evaluate_actions", logits, mask, actions, 0, 0, 0, 0, None, log_prob, entropy, timing)


class PpoStats:
    """What `ppo_loss` returns beside the loss: the scalars of `_native.PPO_STATS` as 0-dim float32 device tensors (views of `raw`, no host
    synchronisation), `log_prob` / `entropy` [...] of the minibatch rows (bit for bit `evaluate_actions`'), and the gradient the call produced --
    `dlogits` [..., 60] in the dtype of the logits, `dvalues` [...] or None.  `kernel_ms` with timing=True."""

    def __init__(self, raw, log_prob, entropy, dlogits, dvalues, kernel_ms=None):
        self.raw, self.log_prob, self.entropy, self.dlogits, self.dvalues, self.kernel_ms = raw, log_prob, entropy, dlogits, dvalues, kernel_ms
        for k, name in enumerate(nat.PPO_STATS):
            setattr(self, name, raw[k])

    def __repr__(self):
        return "PpoStats(" + ", ".join(nat.PPO_STATS) + ", log_prob, entropy, dlogits, dvalues)"


class _PpoLossGrad(torch.autograd.Function):
    """The node `ppo_loss` hangs on its loss: the forward pass already produced the gradient, the backward is one multiplication."""

    @staticmethod
    def forward(ctx, loss, dlogits, dvalues, logits, values):
        ctx.save_for_backward(dlogits, dvalues if dvalues is not None else dlogits.new_empty(0))
        ctx.has_values = dvalues is not None
        return loss.clone()

    @staticmethod
    def backward(ctx, grad):
        dlogits, dvalues = ctx.saved_tensors
        gl = (dlogits * grad).to(dlogits.dtype) if ctx.needs_input_grad[3] else None
        gv = dvalues * grad if ctx.has_values and ctx.needs_input_grad[4] else None
        return None, None, None, gl, gv


_ppo_workspaces: dict = {}


def _ppo_workspace(L, dev: torch.device, m: int) -> torch.Tensor:
    need = int(L.bg_ppo_loss_workspace_bytes(C.c_int64(m)))
    key = (dev, need)
    if key not in _ppo_workspaces:
        _ppo_workspaces[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    return _ppo_workspaces[key]


def ppo_loss(logits: torch.Tensor, actions: torch.Tensor, old_log_prob: torch.Tensor, advantages: torch.Tensor, mask: Optional[torch.Tensor] = None, *,
             values: Optional[torch.Tensor] = None, returns: Optional[torch.Tensor] = None, index: Optional[torch.Tensor] = None,
             clip_range: float = 0.2, ent_coef: float = 0.0, vf_coef: float = 0.5, normalize_advantage: bool = True, timing: bool = False):
    """SB3's `PPO.train` loss over the masked head of `sample_actions`, its diagnostics and its gradient, in one pass over the logits (bg_ppo_loss):
    -> (loss, stats).  loss: 0-dim float32; when `logits` (or `values`) require grad it carries an autograd node whose backward is
    grad_output * stats.dlogits (and * stats.dvalues) -- `loss.backward()` drives the network's own backward with nothing recomputed.  stats: `PpoStats`.
    logits float32 / bfloat16 [..., 60] and values float32 [...] are the network's outputs for the minibatch.  Without `index`, actions int32,
    old_log_prob / advantages / returns float32 and the mask (forms of `sample_actions`) have the leading shape of logits.  With `index` (int32 [...],
    SB3's `RolloutBuffer.get` permutation) they are the STORED arrays of the whole rollout, one common shape, read at row index[i]: the minibatch is
    gathered inside the launch, a record's mask in place.  A row that cannot take part (degenerate mask, masked or out-of-range action, non-finite
    input, index out of range) is excluded: zero gradient, counted in stats.excluded, the divisor stays m.  values / returns: both or neither."""
    lead, m, pitch = _head_logits(logits)
    dev = logits.device
    if index is not None:
        _check_index(index, lead, dev)
        if not isinstance(actions, torch.Tensor):
            raise ValueError("actions must be an int32 tensor")
        store = tuple(actions.shape)
    else:
        store = lead
    store_rows = int(np.prod(store, dtype=np.int64))
    if store_rows >= 2 ** 31:
        raise ValueError("the stored arrays hold at most 2**31 - 1 rows")
    mask, moff, mstride = _head_mask(mask, store, dev)
    _check_scan_tensor("actions", actions, torch.int32, store, dev)
    _check_scan_tensor("old_log_prob", old_log_prob, torch.float32, store, dev)
    _check_scan_tensor("advantages", advantages, torch.float32, store, dev)
    if (values is None) != (returns is None):
        raise ValueError("values and returns go together: both or neither")
    if values is not None:
        _check_scan_tensor("values", values, torch.float32, lead, dev)
        _check_scan_tensor("returns", returns, torch.float32, store, dev)
    for what, v in (("clip_range", clip_range), ("ent_coef", ent_coef), ("vf_coef", vf_coef)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError(f"{what} must be a finite number")
    if not 0.0 < float(np.float32(clip_range)) < 1.0:
        raise ValueError("clip_range must be in (0, 1)")
    if not logits.is_cuda:
        raise ValueError("logits must be a device tensor (there is no CPU fallback)")
    if mask is not None and (mask.data_ptr() + moff) % 4:
        raise ValueError("mask must be 4-byte aligned")
    lg = logits.detach()
    vals = values.detach() if values is not None else None
    raw = torch.zeros(len(nat.PPO_STATS), dtype=torch.float32, device=dev)
    dlogits = torch.empty(lead + (60,), dtype=logits.dtype, device=dev)
    dvalues = torch.empty(lead, dtype=torch.float32, device=dev) if values is not None else None
    log_prob = torch.empty(lead, dtype=torch.float32, device=dev)
    entropy = torch.empty(lead, dtype=torch.float32, device=dev)
    ms = C.c_float(0.0)
    if m > 0:
        L = nat.load()

        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(dev):
            ws = _ppo_workspace(L, dev, m)
            rc = L.bg_ppo_loss(ptr(lg), nat.HEAD_F32 if logits.dtype == torch.float32 else nat.HEAD_BF16, C.c_uint64(pitch),
                               C.c_void_p(mask.data_ptr() + moff) if mask is not None else None, C.c_uint64(mstride), ptr(actions), ptr(old_log_prob),
                               ptr(advantages), ptr(vals), ptr(returns), ptr(index), C.c_int64(store_rows), C.c_int64(m), C.c_float(clip_range),
                               C.c_float(ent_coef), C.c_float(vf_coef), C.c_uint32(nat.PPO_NORMALIZE_ADV if normalize_advantage else 0), ptr(dlogits),
                               C.c_uint64(60), ptr(dvalues), ptr(log_prob), ptr(entropy), ptr(raw), ptr(ws), C.c_uint64(ws.numel()),
                               C.byref(ms) if timing else None, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != 0:
            raise nat.NativeError(f"bg_ppo_loss failed ({rc}): {L.bg_last_error(None).decode()}")
    stats = PpoStats(raw, log_prob, entropy, dlogits, dvalues, float(ms.value) if timing else None)
    loss = raw[0]
    if torch.is_grad_enabled() and (logits.requires_grad or (values is not None and values.requires_grad)):
        loss = _PpoLossGrad.apply(loss, dlogits, dvalues, logits, values)
    return loss, stats


class DqnStats:
    """What `dqn_loss` returns beside the loss: the scalars of `_native.DQN_STATS` as 0-dim float32 device tensors (views of `raw`, no host
    synchronisation), `td` float32 [...] (q[a] - y per row, NaN on an excluded row: for prioritised replay), and the gradient the call produced --
    `dq` [..., 60] in the dtype of q.  `kernel_ms` with timing=True."""

    def __init__(self, raw, td, dq, kernel_ms=None):
        self.raw, self.td, self.dq, self.kernel_ms = raw, td, dq, kernel_ms
        for k, name in enumerate(nat.DQN_STATS):
            setattr(self, name, raw[k])

    def __repr__(self):
        return "DqnStats(" + ", ".join(nat.DQN_STATS) + ", td, dq)"


class _DqnLossGrad(torch.autograd.Function):
    """The node `dqn_loss` hangs on its loss (`_PpoLossGrad`'s pattern): the forward pass already produced the gradient."""

    @staticmethod
    def forward(ctx, loss, dq, q):
        ctx.save_for_backward(dq)
        return loss.clone()

    @staticmethod
    def backward(ctx, grad):
        dq, = ctx.saved_tensors
        return None, None, (dq * grad).to(dq.dtype) if ctx.needs_input_grad[2] else None


_dqn_workspaces: dict = {}


def _dqn_workspace(L, dev: torch.device, m: int) -> torch.Tensor:
    need = int(L.bg_dqn_loss_workspace_bytes(C.c_int64(m)))
    key = (dev, need)
    if key not in _dqn_workspaces:
        _dqn_workspaces[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    return _dqn_workspaces[key]


def dqn_loss(q: torch.Tensor, q_next: torch.Tensor, rows: torch.Tensor, next_index: torch.Tensor, *, q_next_online: Optional[torch.Tensor] = None,
             rewards: Optional[torch.Tensor] = None, gamma: float = 0.99, mask_next: bool = True, loss: str = "huber", timeouts: str = "exclude",
             timing: bool = False):
    """SB3's `DQN.train` loss over a store of packed records, its diagnostics and its gradient with respect to q, in one pass (bg_dqn_loss):
    -> (loss, stats).  loss: 0-dim float32; when `q` requires grad it carries an autograd node whose backward is grad_output * stats.dq -- nothing
    is recomputed.  stats: `DqnStats`.
    q float32 / bfloat16 [..., 60]: the online network at the OBSERVATION records (`encode_rows(store, index=index)`); q_next, same dtype and leading
    shape: the target network at the NEXT records (`index=next_index`); q_next_online: the online network there -- given, it selects double DQN.
    rows: the store, a contiguous uint8 [..., stride] tensor of records (`RowReplay.store`).  next_index int32 [...]: the flat row of each transition's
    next record -- the record that holds the step's action, reward, terminated byte and end flags and the mask of the next decision, all read in
    place.  rewards: float32 with the store's leading shape, read at next_index instead of the records' rewards (normalised rewards).
    mask_next: the maximum over the next record's valid actions only.  loss: "huber" (SB3's smooth_l1) or "mse".  timeouts: "exclude" leaves out rows
    that only the step limit ended (SB3 bootstraps them from a terminal observation the store does not hold); "terminal" treats them as ordinary done
    rows.  mask_next=False, loss="huber", timeouts="terminal" is SB3's rule literally.  A row that cannot take part (next_index or action out of
    range, non-finite reward, q[a] or target, no valid next action) is excluded: zero gradient, NaN td, counted in stats.excluded, the divisor stays m."""
    lead, m, pitch = _head_logits(q)
    dev = q.device
    if not isinstance(q_next, torch.Tensor) or q_next.dtype != q.dtype:
        raise ValueError("q_next must be a tensor [..., 60] of the dtype of q")
    nlead, _, npitch = _head_logits(q_next)
    if nlead != lead or q_next.device != dev:
        raise ValueError(f"q_next must have the leading shape of q {list(lead)} on {dev}")
    opitch = 0
    if q_next_online is not None:
        if not isinstance(q_next_online, torch.Tensor) or q_next_online.dtype != q.dtype:
            raise ValueError("q_next_online must be a tensor [..., 60] of the dtype of q")
        olead, _, opitch = _head_logits(q_next_online)
        if olead != lead or q_next_online.device != dev:
            raise ValueError(f"q_next_online must have the leading shape of q {list(lead)} on {dev}")
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.uint8 or rows.dim() < 2 or not rows.is_contiguous() or rows.device != dev:
        raise ValueError(f"rows must be a contiguous uint8 tensor [..., stride] of packed records on {dev}")
    stride = int(rows.shape[-1])
    if stride < nat.ROW_BYTES or stride % 16:
        raise ValueError(f"the last dimension of rows is the record stride: a multiple of 16, >= {nat.ROW_BYTES} (got {stride})")
    store = tuple(rows.shape[:-1])
    store_rows = int(np.prod(store, dtype=np.int64))
    if store_rows >= 2 ** 31:
        raise ValueError("the store holds at most 2**31 - 1 records")
    if not isinstance(next_index, torch.Tensor) or next_index.dtype != torch.int32 or tuple(next_index.shape) != lead or not next_index.is_contiguous() \
            or next_index.device != dev:
        raise ValueError(f"next_index must be a contiguous torch.int32 tensor of shape {list(lead)} on {dev}")
    if rewards is not None:
        _check_scan_tensor("rewards", rewards, torch.float32, store, dev)
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float, np.integer, np.floating)) or not 0.0 <= float(gamma) <= 1.0:
        raise ValueError("gamma must be a number in [0, 1]")
    if loss not in ("huber", "mse"):
        raise ValueError("loss must be 'huber' or 'mse'")
    if timeouts not in ("exclude", "terminal"):
        raise ValueError("timeouts must be 'exclude' or 'terminal'")
    if not q.is_cuda:
        raise ValueError("q must be a device tensor (there is no CPU fallback)")
    if rows.data_ptr() % 16:
        raise ValueError("rows must be 16-byte aligned")
    flags = (nat.DQN_MASK_NEXT if mask_next else 0) | (nat.DQN_MSE if loss == "mse" else 0) | (nat.DQN_TIMEOUT_EXCLUDE if timeouts == "exclude" else 0)
    qd, qn = q.detach(), q_next.detach()
    qo = q_next_online.detach() if q_next_online is not None else None
    raw = torch.zeros(len(nat.DQN_STATS), dtype=torch.float32, device=dev)
    dq = torch.empty(lead + (60,), dtype=q.dtype, device=dev)
    td = torch.empty(lead, dtype=torch.float32, device=dev)
    ms = C.c_float(0.0)
    if m > 0:
        L = nat.load()

        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(dev):
            ws = _dqn_workspace(L, dev, m)
            rc = L.bg_dqn_loss(ptr(qd), C.c_uint64(pitch), ptr(qn), C.c_uint64(npitch), ptr(qo), C.c_uint64(opitch),
                               nat.HEAD_F32 if q.dtype == torch.float32 else nat.HEAD_BF16, ptr(rows), C.c_uint64(stride), C.c_int64(store_rows),
                               ptr(next_index), ptr(rewards), C.c_int64(m), C.c_float(float(gamma)), C.c_uint32(flags), ptr(dq), C.c_uint64(60), ptr(td),
                               ptr(raw), ptr(ws), C.c_uint64(ws.numel()), C.byref(ms) if timing else None,
                               C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != 0:
            raise nat.NativeError(f"bg_dqn_loss failed ({rc}): {L.bg_last_error(None).decode()}")
    stats = DqnStats(raw, td, dq, float(ms.value) if timing else None)
    out = raw[0]
    if torch.is_grad_enabled() and q.requires_grad:
        out = _DqnLossGrad.apply(out, dq, q)
    return out, stats


class RowReplay:
    """DQN's replay buffer as a ring of packed records: `capacity_steps` slots of `n` records, [C, N, stride] uint8, 128-byte aligned.  A record
    already carries the observation and action mask of one decision and the action, reward, terminated byte and end flags of the step that led to
    it, so consecutive slots (s, s + 1) of one env ARE a transition and nothing is stored twice (SB3's DictReplayBuffer keeps obs and next_obs).
    `store` goes to `encode_rows(index=)` / `RowLinear(index=)` / `dqn_loss` as it is.
    The ring holds ONE unbroken chain of steps: `start(env.obs_rows)` writes the record before the first step, every `add(buf.rows)` the K records
    of a `step_many` call that continues from the last record added.  Auto-reset envs never break the chain (a record whose terminated byte is set
    already shows the new episode, and `dqn_loss` does not bootstrap across it); a caller who resets envs by hand calls `clear()` and `start()`
    again.  Writing `step_many`'s records into the ring in place is out of scope: `add` is one device copy (two where the ring wraps)."""

    def __init__(self, capacity_steps: int, n: int, device, row_stride: int = 384):
        C_, N, stride = int(capacity_steps), int(n), int(row_stride)
        if C_ < 2 or N < 1:
            raise ValueError("capacity_steps must be >= 2 (a transition is two records) and n >= 1")
        if stride < nat.ROW_BYTES or stride % 16:
            raise ValueError(f"row_stride must be a multiple of 16 and >= the {nat.ROW_BYTES}-byte record")
        if C_ * N >= 2 ** 31:
            raise ValueError("capacity_steps * n must be below 2**31 (int32 row indices)")
        self.capacity_steps, self.n, self.row_stride = C_, N, stride
        self.device = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        nbytes = C_ * N * stride
        self._flat = torch.zeros(nbytes + 128, dtype=torch.uint8, device=self.device)
        off = (-self._flat.data_ptr()) % 128
        self.store = self._flat[off:off + nbytes].view(C_, N, stride)
        self._head = 0      # the slot the next record goes to (the write head)
        self._filled = 0    # slots that hold a record

    def __len__(self) -> int:
        """Valid transitions: (filled slots - 1) * n."""
        return max(self._filled - 1, 0) * self.n

    def clear(self) -> None:
        self._head, self._filled = 0, 0

    def _check_records(self, what: str, t, dims: int):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != dims or tuple(t.shape[-2:]) != (self.n, self.row_stride) \
                or t.device != self.device:
            lead = "[K, " if dims == 3 else "["
            raise ValueError(f"{what} must be a uint8 tensor {lead}{self.n}, {self.row_stride}] of packed records on {self.device}")

    def start(self, obs_rows: torch.Tensor) -> None:
        """Begin a chain: the record BEFORE the first step (`env.obs_rows`, [N, stride]).  Whatever the ring held is dropped."""
        self._check_records("obs_rows", obs_rows, 2)
        self.store[0].copy_(obs_rows)
        self._head, self._filled = 1 % self.capacity_steps, 1

    def add(self, rows_kn: torch.Tensor) -> None:
        """Append the K step records of one `step_many` call ([K, N, stride], `RowBuffers.rows`), wrapping."""
        self._check_records("rows_kn", rows_kn, 3)
        K, C_ = int(rows_kn.shape[0]), self.capacity_steps
        if K >= C_:
            raise ValueError(f"K = {K} step records do not fit a ring of {C_} slots beside the record they continue from (K < capacity_steps)")
        if self._filled == 0:
            raise ValueError("start(obs_rows) writes the record before the first step; add() continues from it")
        first = min(K, C_ - self._head)
        self.store[self._head:self._head + first].copy_(rows_kn[:first])
        if first < K:
            self.store[:K - first].copy_(rows_kn[first:])
        self._head = (self._head + K) % C_
        self._filled = min(self._filled + K, C_)

    def sample(self, m: int, generator: Optional[torch.Generator] = None):
        """(index, next_index): int32 [m] device tensors, drawn on the device with no host synchronisation.  The slot s is uniform over the slots
        whose successor (s + 1) % C is also filled and is not the write head, the env uniform over n; index = s * n + env names the observation
        record, next_index = ((s + 1) % C) * n + env the record of the step taken there."""
        m = int(m)
        if m < 0:
            raise ValueError("m must be >= 0")
        count = self._filled - 1
        if count < 1:
            raise ValueError("the ring holds no transition yet (start() and at least one add())")
        C_, N = self.capacity_steps, self.n
        oldest = self._head if self._filled == C_ else 0
        gdev = generator.device if generator is not None else self.device
        r = torch.randint(0, count * N, (m,), generator=generator, device=gdev, dtype=torch.int64).to(self.device)
        j, env = r // N, r % N
        s = (j + oldest) % C_
        return (s * N + env).to(torch.int32), (((s + 1) % C_) * N + env).to(torch.int32)

    def state_dict(self) -> dict:
        return {"store": self.store.clone(), "head": self._head, "filled": self._filled, "capacity_steps": self.capacity_steps, "n": self.n,
                "row_stride": self.row_stride}

    def load_state_dict(self, state: dict) -> None:
        shape = (int(state["capacity_steps"]), int(state["n"]), int(state["row_stride"]))
        if shape != (self.capacity_steps, self.n, self.row_stride):
            raise ValueError(f"the state is of a ring {list(shape)}, this one is {[self.capacity_steps, self.n, self.row_stride]}")
        head, filled = int(state["head"]), int(state["filled"])
        if not 0 <= filled <= self.capacity_steps or not 0 <= head < self.capacity_steps or (filled < self.capacity_steps and head != filled % self.capacity_steps):
            raise ValueError("the state's head / filled do not describe a ring of this capacity")
        self.store.copy_(state["store"])
        self._head, self._filled = head, filled


def _check_scan_rows(rows) -> tuple:
    """rows of gae_rows / EpisodeStats.update: contiguous uint8 [K, N, stride] -> (K, N, stride)."""
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.uint8 or rows.dim() != 3 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous uint8 tensor [K, N, stride] of packed records")
    K, N, stride = (int(x) for x in rows.shape)
    if stride < nat.ROW_BYTES or stride % 16:
        raise ValueError(f"the last dimension of rows is the record stride: a multiple of 16, >= {nat.ROW_BYTES} (got {stride})")
    return K, N, stride


def _check_scan_tensor(name: str, t, dtype: torch.dtype, shape: tuple, device: torch.device):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != device:
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {list(shape)} on {device}")


def gae_rows(rows: torch.Tensor, values: torch.Tensor, last_values: torch.Tensor, gamma: float = 0.99, gae_lambda: float = 0.95,
             advantages: Optional[torch.Tensor] = None, returns: Optional[torch.Tensor] = None, timing: bool = False,
             rewards: Optional[torch.Tensor] = None):
    """Advantages and returns of a finished [K, N] rollout of packed records in one launch (bg_gae_rows): bit for bit SB3's
    `RolloutBuffer.compute_returns_and_advantage` run in numpy on float32 buffers, with dones[t] = the record's terminated byte and the reward
    rounded from the record's float64.  rows: contiguous uint8 device tensor [K, N, stride] (`RowBuffers.rows`); values float32 [K, N] (the value
    network's output per step), last_values float32 [N] (its output on the observation after the last step).  advantages / returns: optional
    float32 [K, N] tensors to write into; they must not share memory with values or with each other.  rewards: optional float64 [K, N] device tensor
    to take the rewards from instead of the records (bg_gae_rows_ex; `RowNormalizer.normalize_reward`'s output), each rounded to float32 like the record's.
    Returns (advantages, returns); timing=True returns (advantages, returns, kernel milliseconds)."""
    K, N, stride = _check_scan_rows(rows)
    dev = rows.device
    _check_scan_tensor("values", values, torch.float32, (K, N), dev)
    _check_scan_tensor("last_values", last_values, torch.float32, (N,), dev)
    for name, t in (("advantages", advantages), ("returns", returns)):
        if t is not None:
            _check_scan_tensor(name, t, torch.float32, (K, N), dev)
    if rewards is not None:
        _check_scan_tensor("rewards", rewards, torch.float64, (K, N), dev)
    gamma, gae_lambda = float(gamma), float(gae_lambda)
    if not (np.isfinite(gamma) and np.isfinite(gae_lambda)):
        raise ValueError("gamma and gae_lambda must be finite")
    if not rows.is_cuda:
        raise ValueError("rows must be a device tensor (there is no CPU fallback)")
    if rows.data_ptr() % 16:
        raise ValueError("rows must be 16-byte aligned")
    if advantages is None:
        advantages = torch.empty((K, N), dtype=torch.float32, device=dev)
    if returns is None:
        returns = torch.empty((K, N), dtype=torch.float32, device=dev)
    ptrs = [values.data_ptr(), advantages.data_ptr(), returns.data_ptr()]
    if K * N and len(set(ptrs)) != 3:
        raise ValueError("advantages / returns must not share memory with values or with each other")
    if K * N == 0:   # nothing to launch (an empty tensor has no pointer to hand over)
        return (advantages, returns, 0.0) if timing else (advantages, returns)
    L = nat.load()
    ms = C.c_float(0.0)
    with torch.cuda.device(dev):
        args = (C.c_void_p(rows.data_ptr()), C.c_uint64(stride), K, C.c_int64(N), C.c_void_p(values.data_ptr()),
                C.c_void_p(last_values.data_ptr()), C.c_double(gamma), C.c_double(gae_lambda), C.c_void_p(advantages.data_ptr()),
                C.c_void_p(returns.data_ptr()))
        tail = (C.byref(ms) if timing else None, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        rc = L.bg_gae_rows(*args, *tail) if rewards is None else L.bg_gae_rows_ex(*args, C.c_void_p(rewards.data_ptr()), *tail)
    if rc != 0:
        raise nat.NativeError(f"bg_gae_rows failed ({rc}): {L.bg_last_error(None).decode()}")
    return (advantages, returns, float(ms.value)) if timing else (advantages, returns)


class EpisodeStats:
    """What `Monitor` reports per finished episode, for N envs on the device (bg_episode_stats_rows): owns the running reward sum (float64, a plain
    sum in step order) and step count (int32) of every env's current episode, across calls."""

    def __init__(self, n: int, device):
        if int(n) < 0:
            raise ValueError("n must be >= 0")
        self.n = int(n)
        self.device = torch.device(device)
        self.ep_return_carry = torch.zeros(self.n, dtype=torch.float64, device=self.device)
        self.ep_len_carry = torch.zeros(self.n, dtype=torch.int32, device=self.device)

    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """Forget the running episodes (of the envs where `mask` is set): for callers who `env.reset()` by hand."""
        if mask is None:
            self.ep_return_carry.zero_()
            self.ep_len_carry.zero_()
            return
        mask = torch.as_tensor(mask)
        if tuple(mask.shape) != (self.n,):
            raise ValueError(f"mask must have shape [{self.n}]")
        mask = mask.to(device=self.device, dtype=torch.bool)
        self.ep_return_carry.masked_fill_(mask, 0.0)
        self.ep_len_carry.masked_fill_(mask, 0)

    def update(self, rows: torch.Tensor, ep_return: Optional[torch.Tensor] = None, ep_len: Optional[torch.Tensor] = None, timing: bool = False):
        """The next K steps of every env: rows contiguous uint8 [K, N, stride] on this device.  Returns (ep_return float64 [K, N], ep_len int32
        [K, N]): on a terminated step the finished episode's reward sum and length, 0.0 / 0 elsewhere (`ep_len.nonzero()` lists the episodes);
        timing=True appends the kernel milliseconds.  ep_return / ep_len: optional tensors to write into."""
        K, N, stride = _check_scan_rows(rows)
        if N != self.n or rows.device != self.device:
            raise ValueError(f"rows must hold records of {self.n} envs on {self.device} (got {N} envs on {rows.device})")
        if ep_return is not None:
            _check_scan_tensor("ep_return", ep_return, torch.float64, (K, N), self.device)
        if ep_len is not None:
            _check_scan_tensor("ep_len", ep_len, torch.int32, (K, N), self.device)
        if not rows.is_cuda:
            raise ValueError("rows must be a device tensor (there is no CPU fallback)")
        if rows.data_ptr() % 16:
            raise ValueError("rows must be 16-byte aligned")
        if ep_return is None:
            ep_return = torch.empty((K, N), dtype=torch.float64, device=self.device)
        if ep_len is None:
            ep_len = torch.empty((K, N), dtype=torch.int32, device=self.device)
        if K * N == 0:
            return (ep_return, ep_len, 0.0) if timing else (ep_return, ep_len)
        L = nat.load()
        ms = C.c_float(0.0)
        with torch.cuda.device(self.device):
            rc = L.bg_episode_stats_rows(C.c_void_p(rows.data_ptr()), C.c_uint64(stride), K, C.c_int64(N), C.c_void_p(self.ep_return_carry.data_ptr()),
                                         C.c_void_p(self.ep_len_carry.data_ptr()), C.c_void_p(ep_return.data_ptr()), C.c_void_p(ep_len.data_ptr()),
                                         C.byref(ms) if timing else None, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        if rc != 0:
            raise nat.NativeError(f"bg_episode_stats_rows failed ({rc}): {L.bg_last_error(None).decode()}")
        return (ep_return, ep_len, float(ms.value)) if timing else (ep_return, ep_len)


class EpisodeLimits:
    """SafeBalatroEnv's episode limits for `BalatroVecEnv.step_many(actions, obs_buffers=rows, limits=...)` (bg_step_many_rows_ex): owns, on the
    device, the per-env counters the limits need across calls (int32 [n, 4]: episode_steps, consecutive_invalid, wrapper endings in the last call,
    0) and the buffers for the records before the resets the wrapper causes -- SB3's info["terminal_observation"]: `terminal_rows` uint8
    [S, n, row_stride] and `terminal_step` int32 [S, n] (the step of the last call whose ending filled the slot, else -1), S =
    steps // min(limits) + 1 slots per env for calls of up to `steps` steps.  summary=True: `step_many` turns the handle's episode summary on
    (bg_set_episode_summary), and the record of every ended step carries the ended episode's final ante, round and score.  progression=True: sized
    for `step_many(..., progression=)`, whose stuck endings need steps // min(limits, 301) + 1 slots (bg_progress_terminal_slots)."""

    def __init__(self, n: int, device, max_invalid_actions: int = 50, max_episode_steps: int = 1000, steps: int = 1, row_stride: int = 384,
                 summary: bool = False, progression: bool = False):
        if not isinstance(summary, (bool, np.bool_)):
            raise ValueError("summary must be a bool")
        if not isinstance(progression, (bool, np.bool_)):
            raise ValueError("progression must be a bool")
        self.summary = bool(summary)
        self.progression = bool(progression)
        self.n, self.steps = int(n), int(steps)
        self.device = torch.device(device)
        self.max_invalid_actions, self.max_episode_steps = int(max_invalid_actions), int(max_episode_steps)
        self.row_stride = int(row_stride) or nat.ROW_BYTES
        if self.n < 0 or self.steps < 1:
            raise ValueError("n must be >= 0 and steps >= 1")
        if min(self.max_invalid_actions, self.max_episode_steps) < nat.SAFE_MIN_LIMIT or max(self.max_invalid_actions, self.max_episode_steps) >= 2 ** 31:
            raise ValueError(f"max_invalid_actions and max_episode_steps must be >= {nat.SAFE_MIN_LIMIT} (and fit an int32)")
        if self.row_stride < nat.ROW_BYTES or self.row_stride % 16:
            raise ValueError("row_stride must be a multiple of 16 and >= the 352-byte record")
        self.slots = self.steps // min(self.max_invalid_actions, self.max_episode_steps) + 1   # bg_safe_terminal_slots
        if self.progression:
            self.slots = self.steps // min(self.max_invalid_actions, self.max_episode_steps, nat.PROGRESS_STUCK_STEPS + 1) + 1   # bg_progress_terminal_slots
        self.counters = torch.zeros((self.n, 4), dtype=torch.int32, device=self.device)
        self.terminal_rows = torch.zeros((self.slots, self.n, self.row_stride), dtype=torch.uint8, device=self.device)
        self.terminal_step = torch.full((self.slots, self.n), -1, dtype=torch.int32, device=self.device)
        self._terminal = None

    def _struct(self) -> "nat.SafeLimits":
        return nat.SafeLimits(self.max_invalid_actions, self.max_episode_steps, self.counters.data_ptr(), self.terminal_rows.data_ptr(),
                              self.row_stride, self.terminal_step.data_ptr(), self.slots)

    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """Zero the counters (of the envs where `mask` is set): beside `env.reset(mask=...)`, as SafeBalatroEnv.reset does."""
        if mask is None:
            self.counters.zero_()
            return
        mask = torch.as_tensor(mask)
        if tuple(mask.shape) != (self.n,):
            raise ValueError(f"mask must have shape [{self.n}]")
        self.counters.masked_fill_(mask.to(device=self.device, dtype=torch.bool).view(self.n, 1), 0)

    def state_dict(self) -> dict:
        return {"max_invalid_actions": self.max_invalid_actions, "max_episode_steps": self.max_episode_steps, "counters": self.counters.cpu().clone()}

    def load_state_dict(self, state: dict) -> None:
        if (int(state["max_invalid_actions"]), int(state["max_episode_steps"])) != (self.max_invalid_actions, self.max_episode_steps):
            raise ValueError("the saved counters belong to other limits")
        c = torch.as_tensor(state["counters"])
        if tuple(c.shape) != (self.n, 4):
            raise ValueError(f"counters must have shape [{self.n}, 4]")
        self.counters.copy_(c.to(device=self.device, dtype=torch.int32))

    def terminal(self):
        """(index int32 [M], records uint8 [M, row_stride]) of the last call's wrapper endings: index = t * n + e, ascending (the index `minibatches` /
        `ppo_loss(index=)` use for step t of env e); records[i] is the record of that step BEFORE the reset.  `encode_rows(records, layout)` -- with
        `norm=` a RowNormalizer for VecNormalize's frozen statistics -- takes the [M, row_stride] tensor as it is, M = 0 included (`normalize_obs`
        does not: it reads a 2-D tensor as ONE step of its N envs); the value network turns that matrix into `bootstrap_rewards`' terminal_values.  Made with torch on the
        device (M is at most slots * n); the result is kept until the next call."""
        if self._terminal is None:
            ts = self.terminal_step.reshape(-1)
            used = (ts >= 0).nonzero(as_tuple=False).flatten()          # slot j * n + e
            index = ts[used].to(torch.int64) * self.n + used % self.n    # t * n + e: distinct, so the order is total
            order = torch.argsort(index)
            self._terminal = (index[order].to(torch.int32), self.terminal_rows.view(-1, self.row_stride)[used[order]].contiguous())
        return self._terminal


class ProgressionRewards:
    """ProgressionRewardWrapper's state for `BalatroVecEnv.step_many(actions, obs_buffers=rows, limits=..., progression=...)`
    (bg_step_many_rows_progress): owns, on the device, the per-env carry of the wrapper across calls -- int32 [n, 4]: total_steps,
    steps_on_current_ante, (last_ante - 1) | (max_ante_reached - 1) << 16, last_round - 1, so that zeros are the state after the wrapper's reset().
    The constants of the rule are the reference's (train_progressive.py:21-120), not parameters."""

    def __init__(self, n: int, device):
        self.n = int(n)
        if self.n < 0:
            raise ValueError("n must be >= 0")
        self.device = torch.device(device)
        self.counters = torch.zeros((self.n, 4), dtype=torch.int32, device=self.device)

    def _struct(self) -> "nat.ProgressRewards":
        return nat.ProgressRewards(self.counters.data_ptr())

    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """Zero the carry (of the envs where `mask` is set): beside `env.reset(mask=...)`, as ProgressionRewardWrapper.reset does."""
        if mask is None:
            self.counters.zero_()
            return
        mask = torch.as_tensor(mask)
        if tuple(mask.shape) != (self.n,):
            raise ValueError(f"mask must have shape [{self.n}]")
        self.counters.masked_fill_(mask.to(device=self.device, dtype=torch.bool).view(self.n, 1), 0)

    def state_dict(self) -> dict:
        return {"counters": self.counters.cpu().clone()}

    def load_state_dict(self, state: dict) -> None:
        c = torch.as_tensor(state["counters"])
        if tuple(c.shape) != (self.n, 4):
            raise ValueError(f"counters must have shape [{self.n}, 4]")
        self.counters.copy_(c.to(device=self.device, dtype=torch.int32))


def _episode_ends_call(rows, cur: Optional["nat.Curriculum"], n_expected: Optional[int], timing: bool):
    K, N, stride = _check_scan_rows(rows)
    if n_expected is not None and N != n_expected:
        raise ValueError(f"rows must hold records of {n_expected} envs (got {N})")
    if not rows.is_cuda:
        raise ValueError("rows must be a device tensor (there is no CPU fallback)")
    if rows.data_ptr() % 16:
        raise ValueError("rows must be 16-byte aligned")
    dev = rows.device
    if K * N == 0:   # nothing to launch (an empty tensor has no pointer to hand over)
        return torch.zeros(nat.ENDS_WORDS, dtype=torch.int64, device=dev), 0.0
    report = torch.empty(nat.ENDS_WORDS, dtype=torch.int64, device=dev)
    L = nat.load()
    ms = C.c_float(0.0)
    with torch.cuda.device(dev):
        rc = L.bg_episode_ends_rows(C.c_void_p(rows.data_ptr()), C.c_uint64(stride), K, C.c_int64(N), C.c_void_p(report.data_ptr()),
                                    None if cur is None else C.byref(cur), C.byref(ms) if timing else None,
                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise nat.NativeError(f"bg_episode_ends_rows failed ({rc}): {L.bg_last_error(None).decode()}")
    return report, float(ms.value)


def episode_ends(rows: torch.Tensor, timing: bool = False):
    """The ended episodes of a finished [K, N] rollout of packed records in one launch (bg_episode_ends_rows): int64 [32] on the device, words by
    `_native.ENDS_REPORT` -- ended records, of which game overs / kills / step-limit-only endings, sum and maximum of the end ante and of the end
    chips, records without a summary -- and from `_native.ENDS_HIST` on the histogram of min(end ante, 15).  rows: contiguous uint8 device tensor
    [K, N, stride] (`RowBuffers.rows`) of `step_many(..., limits=EpisodeLimits(..., summary=True))`.  timing=True returns (report, kernel ms)."""
    report, ms = _episode_ends_call(rows, None, None, timing)
    return (report, ms) if timing else report


class RowCurriculum:
    """`CurriculumBalatroEnv` (train_balatro_agent.py:126-170) for the packed-record path, on the device: `sb3_adapter.CurriculumTracker`'s state --
    `cap` int32 [n], `hist` int16 [window, n] (the final antes of the last `window` episodes), `count` int64 [n], `at_level` int32 [n] -- advanced
    by bg_episode_ends_rows from the records of `step_many(..., limits=EpisodeLimits(..., summary=True))`.  A raised cap takes effect at the call
    boundary: episodes an env finishes later in the same rollout were played under the old cap and enter the history as played."""

    def __init__(self, env: "BalatroVecEnv", initial_max_ante: int = 3, ante_increment: int = 1, success_threshold: float = 0.8, window: int = 100):
        self.env = env
        self.n = int(env.num_envs)
        self.device = torch.device(env.device)
        self.increment, self.threshold, self.window = int(ante_increment), float(success_threshold), int(window)
        if not 1 <= int(initial_max_ante) <= nat.CURRICULUM_CAP_MAX:
            raise ValueError(f"initial_max_ante must be in 1..{nat.CURRICULUM_CAP_MAX}")
        if not 1 <= self.increment <= nat.CURRICULUM_CAP_MAX:
            raise ValueError(f"ante_increment must be in 1..{nat.CURRICULUM_CAP_MAX}")
        if self.window < 1 or self.window >= 2 ** 31:
            raise ValueError("window must be >= 1 (and fit an int32)")
        if not np.isfinite(self.threshold):
            raise ValueError("success_threshold must be finite")
        self.cap = torch.full((self.n,), int(initial_max_ante), dtype=torch.int32, device=self.device)
        self.hist = torch.zeros((self.window, self.n), dtype=torch.int16, device=self.device)
        self.count = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        self.at_level = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        self.raised = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
        env.set_max_ante(int(initial_max_ante))

    def _struct(self) -> "nat.Curriculum":
        return nat.Curriculum(self.cap.data_ptr(), self.hist.data_ptr(), self.count.data_ptr(), self.at_level.data_ptr(), self.raised.data_ptr(),
                              self.window, self.increment, self.threshold)

    def update(self, rows: torch.Tensor, apply: bool = True, timing: bool = False):
        """The ended episodes of rows (contiguous uint8 [K, n, stride] on the env's device) through the rule, per env in step order.  Returns the
        report (`episode_ends`; word `_native.ENDS_REPORT["raised"]` counts the envs whose cap rose, `self.raised` marks them); timing=True appends
        the kernel milliseconds.  apply=True reads that word -- the call's one 8-byte synchronisation -- and, only when it is non-zero, hands the
        raised caps to `env.set_max_ante`, which keeps the library's host mirror of the caps in step.  apply=False leaves that to the caller."""
        if isinstance(rows, torch.Tensor) and rows.device != self.device:
            raise ValueError(f"rows must hold records of {self.n} envs on {self.device} (got {rows.device})")
        report, ms = _episode_ends_call(rows, self._struct(), self.n, timing)
        if rows.shape[0] * rows.shape[1] == 0:
            self.raised.zero_()
        elif apply and int(report[nat.ENDS_REPORT["raised"]].item()):
            self.env.set_max_ante(self.cap.cpu().numpy(), mask=self.raised.cpu().numpy())
        return (report, ms) if timing else report

    def state_dict(self) -> dict:
        return {"window": self.window, "ante_increment": self.increment, "success_threshold": self.threshold, "cap": self.cap.cpu().clone(),
                "hist": self.hist.cpu().clone(), "count": self.count.cpu().clone(), "at_level": self.at_level.cpu().clone()}

    def load_state_dict(self, state: dict, apply: bool = True) -> None:
        """Restores the rule's state; apply=True also sets the env's caps from it (`env.set_max_ante`)."""
        if int(state["window"]) != self.window:
            raise ValueError("the saved history belongs to another window")
        new = {}
        for name, dt, shape in (("cap", torch.int32, (self.n,)), ("hist", torch.int16, (self.window, self.n)), ("count", torch.int64, (self.n,)),
                                ("at_level", torch.int32, (self.n,))):
            t = torch.as_tensor(state[name])
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} must have shape {list(shape)}")
            new[name] = t.to(dtype=dt)
        if new["cap"].numel() and (int(new["cap"].min()) < 0 or int(new["cap"].max()) > nat.CURRICULUM_CAP_MAX):
            raise ValueError(f"cap must be in 0..{nat.CURRICULUM_CAP_MAX}")
        self.increment, self.threshold = int(state["ante_increment"]), float(state["success_threshold"])
        for name, t in new.items():
            getattr(self, name).copy_(t.to(self.device))
        if apply:
            self.env.set_max_ante(new["cap"].numpy())


def _norm_rows(rows) -> torch.Tensor:
    """rows of RowNormalizer: [N, stride] (one step) or [K, N, stride] -> the [K, N, stride] view."""
    if isinstance(rows, torch.Tensor) and rows.dim() == 2:
        rows = rows.unsqueeze(0)
    return rows


class RowNormalizer:
    """SB3's `VecNormalize(norm_obs, norm_reward)` for N envs over packed records, on the device (bg_norm_obs_rows / bg_norm_reward_rows).  Owns what
    VecNormalize pickles -- one RunningMeanStd (mean, var float64 [153], one count) over the columns of the "produced" layout, the return statistics
    `ret_stats` (mean, var, count) -- plus the per-env discounted return `returns` (float64 [N]) and a cached workspace, all device tensors.
    Each of the K steps of a call is one VecNormalize step: update the statistics with the batch of N envs, then normalise with the updated statistics.
    training=False (or `.training = False` later) freezes the statistics: only the normalisation runs.  With norm_obs / norm_reward unset the matching
    call refuses: encode the records / read `RowBuffers.reward` instead."""

    def __init__(self, n: int, device, *, gamma: float = 0.99, epsilon: float = 1e-8, clip_obs: float = 10.0, clip_reward: float = 10.0,
                 norm_obs: bool = True, norm_reward: bool = True, training: bool = True):
        if int(n) < 0:
            raise ValueError("n must be >= 0")
        for name, v in (("gamma", gamma), ("epsilon", epsilon), ("clip_obs", clip_obs), ("clip_reward", clip_reward)):
            if not np.isfinite(float(v)):
                raise ValueError(f"{name} must be finite")
        self.n = int(n)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:   # "cuda" is the current device: tensors report it with its index
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.gamma, self.epsilon, self.clip_obs, self.clip_reward = float(gamma), float(epsilon), float(clip_obs), float(clip_reward)
        self.norm_obs, self.norm_reward, self.training = bool(norm_obs), bool(norm_reward), bool(training)
        f64 = dict(dtype=torch.float64, device=self.device)
        self.obs_mean = torch.zeros(nat.NORM_COLS, **f64)        # RunningMeanStd(epsilon=1e-4): mean 0, var 1, count 1e-4
        self.obs_var = torch.ones(nat.NORM_COLS, **f64)
        self.obs_count = torch.full((1,), 1e-4, **f64)
        self.ret_stats = torch.tensor([0.0, 1.0, 1e-4], **f64)   # mean, var, count
        self.returns = torch.zeros(self.n, **f64)
        self._workspace: Optional[torch.Tensor] = None

    def reset_returns(self, mask: Optional[torch.Tensor] = None) -> None:
        """Zero the discounted returns (of the envs where `mask` is set): VecNormalize.reset() does so for all envs."""
        if mask is None:
            self.returns.zero_()
            return
        mask = torch.as_tensor(mask)
        if tuple(mask.shape) != (self.n,):
            raise ValueError(f"mask must have shape [{self.n}]")
        self.returns.masked_fill_(mask.to(device=self.device, dtype=torch.bool), 0.0)

    def state_dict(self) -> dict:
        """Host copies of everything the next call depends on: the counterpart of VecNormalize's pickle.  `load_state_dict` restores it exactly."""
        return {"obs_mean": self.obs_mean.cpu().clone(), "obs_var": self.obs_var.cpu().clone(), "obs_count": self.obs_count.cpu().clone(),
                "ret_stats": self.ret_stats.cpu().clone(), "returns": self.returns.cpu().clone(),
                "gamma": self.gamma, "epsilon": self.epsilon, "clip_obs": self.clip_obs, "clip_reward": self.clip_reward,
                "norm_obs": self.norm_obs, "norm_reward": self.norm_reward, "training": self.training}

    def load_state_dict(self, state: dict) -> None:
        for name in ("obs_mean", "obs_var", "obs_count", "ret_stats", "returns"):
            mine, t = getattr(self, name), torch.as_tensor(state[name])
            if t.dtype != torch.float64 or tuple(t.shape) != tuple(mine.shape):
                raise ValueError(f"{name} must be a torch.float64 tensor of shape {list(mine.shape)}")
        for name in ("obs_mean", "obs_var", "obs_count", "ret_stats", "returns"):
            getattr(self, name).copy_(torch.as_tensor(state[name]))
        for name in ("gamma", "epsilon", "clip_obs", "clip_reward"):
            if name in state:
                setattr(self, name, float(state[name]))
        for name in ("norm_obs", "norm_reward", "training"):
            if name in state:
                setattr(self, name, bool(state[name]))

    def _check_rows(self, rows) -> tuple:
        K, N, stride = _check_scan_rows(_norm_rows(rows))
        if N != self.n or rows.device != self.device:
            raise ValueError(f"rows must hold records of {self.n} envs on {self.device} (got {N} envs on {rows.device})")
        return K, N, stride

    def _ready(self, L, K, N) -> torch.Tensor:
        need = int(L.bg_norm_workspace_bytes(K, C.c_int64(N)))
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._workspace

    def normalize_obs(self, rows: torch.Tensor, layout: str = "produced", dtype: torch.dtype = torch.float32, out: Optional[torch.Tensor] = None,
                      timing: bool = False, *, index: Optional[torch.Tensor] = None, update: Optional[bool] = None):
        """K VecNormalize steps over the observations of rows (contiguous uint8 [K, N, stride], or [N, stride] = one step): returns the normalised
        [K, N, D] (or [N, D]) matrix of `layout` ("produced" 153 columns, "fixed" 628: the never-filled columns are 0.0) in `dtype` (torch.float32 or
        torch.bfloat16).  out: optional contiguous tensor of that shape and dtype to write into.  timing=True appends the kernel milliseconds.
        update: None = `self.training`; False normalises with the statistics as they stand.  index: int32 [m] (`RowBuffers.minibatches`): the
        [m, D] matrix of records index[i], gathered inside the launch with the statistics FROZEN (`encode_rows(index=, norm=)`); a statistics update is
        defined per step over all N envs, not over a minibatch, so update=True with an index is refused."""
        if index is not None:
            if update:
                raise ValueError("update=True with an index: a statistics update is defined per step over all N envs, not over a minibatch")
            self._check_rows(rows)
            return encode_rows(rows, layout, dtype, out, index=index, norm=self, timing=timing)
        if not self.norm_obs:
            raise ValueError("this RowNormalizer was made with norm_obs=False: use encode_rows")
        if layout not in ("produced", "fixed"):
            raise ValueError(f"layout must be 'produced' or 'fixed' (got {layout!r}): VecNormalize wraps the env's keys, not the extractor's tensors")
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("dtype must be torch.float32 or torch.bfloat16")
        K, N, stride = self._check_rows(rows)
        D = nat.ENC_COLS[nat.ENC_LAYOUTS[layout]]
        shape = (K, N, D) if rows.dim() == 3 else (N, D)
        if out is not None:
            _check_scan_tensor("out", out, dtype, shape, self.device)
        if not rows.is_cuda:
            raise ValueError("rows must be a device tensor (there is no CPU fallback)")
        if rows.data_ptr() % 16:
            raise ValueError("rows must be 16-byte aligned")
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=self.device)
        if K * N == 0:
            return (out, 0.0) if timing else out
        L = nat.load()
        ms = C.c_float(0.0)
        with torch.cuda.device(self.device):
            ws = self._ready(L, K, N)
            rc = L.bg_norm_obs_rows(C.c_void_p(rows.data_ptr()), C.c_uint64(stride), K, C.c_int64(N), nat.ENC_LAYOUTS[layout],
                                    nat.ENC_F32 if dtype == torch.float32 else nat.ENC_BF16, C.c_void_p(self.obs_mean.data_ptr()),
                                    C.c_void_p(self.obs_var.data_ptr()), C.c_void_p(self.obs_count.data_ptr()), 1 if (self.training if update is None else update) else 0,
                                    C.c_double(self.epsilon), C.c_double(self.clip_obs), C.c_void_p(out.data_ptr()), C.c_uint64(D), None,
                                    C.c_void_p(ws.data_ptr()), C.c_uint64(ws.numel()), C.byref(ms) if timing else None,
                                    C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        if rc != 0:
            raise nat.NativeError(f"bg_norm_obs_rows failed ({rc}): {L.bg_last_error(None).decode()}")
        return (out, float(ms.value)) if timing else out

    def normalize_reward(self, rows: torch.Tensor, out: Optional[torch.Tensor] = None, timing: bool = False):
        """K VecNormalize steps over the rewards of rows: returns the normalised rewards, float64 [K, N] (or [N] for [N, stride] rows), what
        `gae_rows(..., rewards=)` takes.  out: optional contiguous float64 tensor of that shape.  timing=True appends the kernel milliseconds."""
        if not self.norm_reward:
            raise ValueError("this RowNormalizer was made with norm_reward=False: the records' own rewards are `RowBuffers.reward`")
        K, N, stride = self._check_rows(rows)
        shape = (K, N) if rows.dim() == 3 else (N,)
        if out is not None:
            _check_scan_tensor("out", out, torch.float64, shape, self.device)
        if not rows.is_cuda:
            raise ValueError("rows must be a device tensor (there is no CPU fallback)")
        if rows.data_ptr() % 16:
            raise ValueError("rows must be 16-byte aligned")
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=self.device)
        if K * N == 0:
            return (out, 0.0) if timing else out
        L = nat.load()
        ms = C.c_float(0.0)
        with torch.cuda.device(self.device):
            ws = self._ready(L, K, N)
            rc = L.bg_norm_reward_rows(C.c_void_p(rows.data_ptr()), C.c_uint64(stride), K, C.c_int64(N), C.c_void_p(self.returns.data_ptr()),
                                       C.c_void_p(self.ret_stats.data_ptr()), 1 if self.training else 0, C.c_double(self.gamma), C.c_double(self.epsilon),
                                       C.c_double(self.clip_reward), C.c_void_p(out.data_ptr()), None, C.c_void_p(ws.data_ptr()), C.c_uint64(ws.numel()),
                                       C.byref(ms) if timing else None, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        if rc != 0:
            raise nat.NativeError(f"bg_norm_reward_rows failed ({rc}): {L.bg_last_error(None).decode()}")
        return (out, float(ms.value)) if timing else out


def score_hand_batch(cases: torch.Tensor, lanes_per_case: int = 1, timing: bool = False):
    """`UnifiedScorer.score_hand` (unified_scoring.py:111-299) with joker NAMES for M cases at once: cases int32
    [M, 40] (layout: include/balatro_mi355x.h bg_score_hand_batch) -> int64 [M, 8] (score, chips, mult, x_mult bits, money,
    global-stream words consumed, next getrandbits(32), 0).  lanes_per_case / timing as in classify_batch."""
    L = nat.load()
    if cases.dtype != torch.int32 or cases.dim() != 2 or cases.shape[1] != nat.SCORE_CASE_WORDS or not cases.is_cuda:
        raise ValueError(f"cases must be an int32 [M, {nat.SCORE_CASE_WORDS}] device tensor")
    cases = cases.contiguous()
    out = torch.zeros((cases.shape[0], nat.SCORE_OUT_WORDS), dtype=torch.int64, device=cases.device)
    ms = C.c_float(0.0)
    with torch.cuda.device(cases.device):
        rc = L.bg_score_hand_batch_ex(C.c_void_p(cases.data_ptr()), C.c_void_p(out.data_ptr()), int(cases.shape[0]),
                                      int(lanes_per_case), C.byref(ms) if timing else None,
                                      C.c_void_p(torch.cuda.current_stream(cases.device).cuda_stream))
    if rc != 0:
        raise nat.NativeError(f"bg_score_hand_batch failed ({rc}): {L.bg_last_error(None).decode()}")
    return (out, float(ms.value)) if timing else out


def sim_evaluate_batch(hands: torch.Tensor, n: torch.Tensor, flags: torch.Tensor) -> torch.Tensor:
    """`BalatroSimulator.evaluate_hand` (balatro_sim.py:220-366) for M hands: hands int32 [M, 8, 6] sim cards (rank, suit,
    base_value, enhancement, edition, seal), n int32 [M], flags int32 [M] (1 Four Fingers, 2 Shortcut) -> int8 [M, 128]
    (layout: include/balatro_mi355x.h bg_sim_evaluate_batch)."""
    L = nat.load()
    if hands.dtype != torch.int32 or hands.dim() != 3 or tuple(hands.shape[1:]) != (8, 6) or not hands.is_cuda:
        raise ValueError("hands must be an int32 [M, 8, 6] device tensor")
    if tuple(n.shape) != (hands.shape[0],) or tuple(flags.shape) != (hands.shape[0],):
        raise ValueError("n and flags must have shape [M]")
    hands = hands.contiguous()   # n / flags may come from the host or as other integer types: moved and converted, never handed over as they are
    n, flags = n.to(device=hands.device, dtype=torch.int32).contiguous(), flags.to(device=hands.device, dtype=torch.int32).contiguous()
    out = torch.zeros((hands.shape[0], nat.SIM_EVAL_BYTES), dtype=torch.int8, device=hands.device)
    with torch.cuda.device(hands.device):
        rc = L.bg_sim_evaluate_batch(C.c_void_p(hands.data_ptr()), C.c_void_p(n.data_ptr()), C.c_void_p(flags.data_ptr()),
                                     C.c_void_p(out.data_ptr()), int(hands.shape[0]),
                                     C.c_void_p(torch.cuda.current_stream(hands.device).cuda_stream))
    if rc != 0:
        raise nat.NativeError(f"bg_sim_evaluate_batch failed ({rc}): {L.bg_last_error(None).decode()}")
    return out


def sim_score_batch(cases: torch.Tensor) -> torch.Tensor:
    """`BalatroSimulator.calculate_score` (balatro_sim.py:402-548) for M cases: int32 [M, 64] -> int64 [M, 8]
    (layouts: include/balatro_mi355x.h bg_sim_score_batch)."""
    L = nat.load()
    if cases.dtype != torch.int32 or cases.dim() != 2 or cases.shape[1] != nat.SIM_CASE_WORDS or not cases.is_cuda:
        raise ValueError(f"cases must be an int32 [M, {nat.SIM_CASE_WORDS}] device tensor")
    cases = cases.contiguous()
    out = torch.zeros((cases.shape[0], 8), dtype=torch.int64, device=cases.device)
    with torch.cuda.device(cases.device):
        rc = L.bg_sim_score_batch(C.c_void_p(cases.data_ptr()), C.c_void_p(out.data_ptr()), int(cases.shape[0]),
                                  C.c_void_p(torch.cuda.current_stream(cases.device).cuda_stream))
    if rc != 0:
        raise nat.NativeError(f"bg_sim_score_batch failed ({rc}): {L.bg_last_error(None).decode()}")
    return out
