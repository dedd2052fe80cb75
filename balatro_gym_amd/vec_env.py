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
# the learner's calls over records and logits live in rows.py; every name that used to be defined here stays importable from here
from .rows import (ActorPpoStats, BcStats, DemoBuffer, DqnStats, EpisodeLimits, EpisodeOutcomes, EpisodeStats, PpoStats, ProgressionRewards, RowActor, RowCurriculum, RowExtractor, RowLinear, RowNormalizer,  # noqa: F401
                   RowReplay, _check_scan_tensor, _dqn_workspaces, _ppo_workspaces, actor_evaluate, actor_ppo_loss, actor_sample, bc_loss, dqn_loss, encode_rows, episode_ends, episode_outcomes, evaluate_actions, expert_actions,
                   extractor_rows, extractor_rows_grad, gae_rows, linear_rows, linear_rows_grad, ppo_loss, sample_actions)

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

    def extractor(self, layer: "RowExtractor", index: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The first layer behind BalatroFeaturesExtractor's input over these records, [steps * n, H] or with `index` [m, H] (`RowExtractor.forward`:
        bg_extractor_rows, and bg_extractor_rows_grad under autograd): the [m, 447] matrix is never written."""
        return layer(self.rows, index)

    def normalize_reward(self, norm: "RowNormalizer", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The records' rewards as VecNormalize would hand them to the learner, float64 [steps, n] (`RowNormalizer.normalize_reward`)."""
        return norm.normalize_reward(self.rows, out)

    def sample(self, logits: torch.Tensor, step: int = -1, **kwargs):
        """(actions, log_prob, entropy) drawn from `logits` [n, 60] under the action mask of record row `step` (`sample_actions`; seed= and t= are
        required): the mask a record carries is the one after its step, i.e. the mask of the action to take next.  epsilon= gives the
        epsilon-greedy actions of `sample_actions(epsilon=)` instead: (actions, None, None)."""
        return sample_actions(logits, self.rows[step], **kwargs)

    def expert(self, step: int = -1, **kwargs):
        """The scripted expert's int32 [n] actions for the decisions of record row `step` (`expert_actions`; out=, detail=, timing= as there): the
        record after a step holds the observation and mask of the next decision, so this is the action to take next."""
        return expert_actions(self.rows[step], **kwargs)

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

    def outcomes(self, gamma: float = 1.0, *, rewards: Optional[torch.Tensor] = None, tail: Optional[dict] = None,
                 want=("steps_to_end", "end_ante", "end_flags", "returns"), timing: bool = False) -> "EpisodeOutcomes":
        """The outcome of every step's own episode over these records, [steps, n] per field (`episode_outcomes`: one launch, backwards along the
        steps): steps to the episode's end, its final ante and end flags, the discounted return.  `(outcomes.end_ante >= 5).float()` is the
        reference's behaviour-cloning filter as `bc_loss(weights=)` takes it."""
        return episode_outcomes(self.rows, gamma, rewards=rewards, tail=tail, want=want, timing=timing)

    def to_demo(self, demo: "DemoBuffer", first_record: torch.Tensor, weights: torch.Tensor, *, returns: Optional[torch.Tensor] = None,
                timing: bool = False):
        """Append the kept steps of these records to a `DemoBuffer` (`demo.add`: three launches, no synchronisation).  first_record: the record
        BEFORE the first step ([n, stride]: `env.obs_rows` as it stood before `step_many`); it is put in front of the K step records so that candidate
        row (t, e) pairs the observation of decision t with the step taken from it.  THAT IS A FULL COPY of these records into a new [steps + 1, n] store
        on every call (2.5 GB at 65 536 x 100: more memory and traffic than the append itself): a convenience for small rollouts.  The path without
        the copy is a [K + 1, N] store that the rollout is written into behind its first record, handed to `demo.add` as it is.  weights float32
        [steps, n], returns float64 [steps, n] or None: as `DemoBuffer.add`."""
        if not isinstance(first_record, torch.Tensor) or first_record.dtype != torch.uint8 or tuple(first_record.shape) != (self.n, self.row_stride) \
                or first_record.device != self.rows.device:
            raise ValueError(f"first_record must be a uint8 tensor [{self.n}, {self.row_stride}] of packed records on {self.rows.device}")
        return demo.add(torch.cat([first_record[None], self.rows]), weights, returns=returns, timing=timing)

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

    def expert_act(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int32 [N] actions for `step()` from the scripted expert over the live records of an obs_layout="rows" env (`expert_actions`): the place of
        `act(logits, ...)` in a collection loop that needs no network.  Never an invalid action while the mask has a valid one."""
        if self._rowbuf is None:
            raise ValueError("expert_act() reads the packed records of an obs_layout='rows' env")
        return expert_actions(self._rowbuf.rows[0], out=out)

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
