"""RowOptimizer: the learner's `clip_grad_norm_(...); opt.step(); opt.zero_grad()` as ONE call of libbalatro_mi355x.so (bg_optim_step, csrc/bg_optim.h).

Three launches cover every parameter tensor: the gradient norm in a fixed reduction order (the same bits on every run), the clip coefficient and the
bias corrections on the device (no host synchronisation), and the Adam or RMSpropTFLike update -- which, in the same pass, writes the bfloat16 weight
copies the record layers read (`attach`), DQN's target network (`set_target`) and the zeroed gradients.  A non-finite gradient skips the step instead
of poisoning the parameters.  torch only owns the buffers and the stream; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Optional

import numpy as np
import torch

from . import _native as nat
from .policy import RowDense, RowPolicy
from .rows import RowActor, RowExtractor, RowLinear, _native_call, _ptr

_ENTRY = np.dtype([("param", "<u8"), ("grad", "<u8"), ("state1", "<u8"), ("state2", "<u8"), ("shadow", "<u8"), ("target", "<u8"), ("numel", "<u8"),
                   ("cols", "<u4"), ("pitch", "<u4")])
assert _ENTRY.itemsize == nat.OPTIM_ENTRY_BYTES


class OptimStats:
    """What `RowOptimizer.step` returns: views of the 32-byte block the call wrote, still on the device -- reading one (`float(stats.grad_norm)`) is what
    synchronises, the call itself does not.  grad_norm: the float32 2-norm of all gradients before the clip; clip_coef: min(1, max_grad_norm /
    (grad_norm + 1e-6)); skipped: 1 when the norm was not finite and nothing but the gradients was written; nonfinite: the count of NaN / infinite
    gradient elements; step: the optimiser's step count behind this call.  kernel_ms: the launches' time with timing=True, else None."""

    def __init__(self, raw: torch.Tensor, kernel_ms: Optional[float] = None):
        self.raw, self.kernel_ms = raw, kernel_ms
        f, q = raw.view(torch.float32), raw.view(torch.int64)
        self.grad_norm, self.clip_coef, self.skipped, self.nonfinite, self.step = f[0], f[1], raw[2], q[2], q[3]

    def __repr__(self):
        return "OptimStats(" + ", ".join(nat.OPTIM_STATS) + ")"


def _check_param(what: str, t, device=None, shape=None) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() == 0:
        raise ValueError(f"{what} must be a contiguous, non-empty torch.float32 tensor")
    if device is not None and t.device != device:
        raise ValueError(f"{what} must be on {device}: all parameters, gradients and targets of a RowOptimizer live on one GPU")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must have the shape {list(shape)} of its parameter")


class RowOptimizer:
    """Clipped Adam or RMSpropTFLike over one parameter group (module docstring).

        opt = RowOptimizer(policy.parameters(), lr=3e-4, algorithm="adam", betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5)
        loss.backward(); stats = opt.step()        # clip + update + zero_grad, three launches, no synchronisation

    params: float32, contiguous tensors on one GPU (at most 1 024); anything else raises ValueError.  algorithm "adam": torch.optim.Adam's update with L2
    weight_decay (not AdamW), SB3's eps 1e-5 by default; "rmsprop_tf": SB3's RMSpropTFLike (A2C) -- square average started at ones, eps inside the
    root, smoothing `alpha`, no momentum, not centred.  max_grad_norm: `clip_grad_norm_`'s bound over all gradients; None or <= 0 turns clipping off.
    `step(lr=)` serves SB3's learning-rate schedules.  A parameter whose `.grad is None` is left out of that step, as in torch; its state is untouched.
    Checkpoints: `state_dict()` / `load_state_dict()`; `from_torch(adam)` / `to_torch()` carry exp_avg, exp_avg_sq and step to and from a
    torch.optim.Adam."""

    def __init__(self, params: Iterable[torch.Tensor], lr: float = 3e-4, algorithm: str = "adam", betas: tuple = (0.9, 0.999), eps: float = 1e-5,
                 alpha: float = 0.99, weight_decay: float = 0.0, max_grad_norm: Optional[float] = 0.5):
        if algorithm not in nat.OPTIM_ALGORITHMS:
            raise ValueError(f"algorithm must be 'adam' or 'rmsprop_tf' (got {algorithm!r})")
        self.params = list(params)
        if not self.params:
            raise ValueError("params is empty")
        for i, p in enumerate(self.params):
            _check_param(f"params[{i}]", p)
        self.device = self.params[0].device
        for i, p in enumerate(self.params):
            _check_param(f"params[{i}]", p, self.device)
        if len(set(id(p) for p in self.params)) != len(self.params):
            raise ValueError("params holds a tensor twice")
        if len(self.params) > nat.OPTIM_MAX_TENSORS:
            raise ValueError(f"at most {nat.OPTIM_MAX_TENSORS} parameter tensors (got {len(self.params)})")
        betas = tuple(float(b) for b in betas)
        for what, v, lo, hi in (("lr", lr, 0.0, 1e30), ("eps", eps, 0.0, 1e30), ("weight_decay", weight_decay, 0.0, 1e30), ("alpha", alpha, 0.0, 1.0),
                                ("betas[0]", betas[0], 0.0, 1.0), ("betas[1]", betas[1] if len(betas) == 2 else -1.0, 0.0, 1.0)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not (lo <= float(v) < hi):
                raise ValueError(f"{what} must be a number in [{lo:g}, {hi:g})")
        if max_grad_norm is not None and (isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float)) or not float(max_grad_norm) < 1e30):
            raise ValueError("max_grad_norm must be a number or None")
        self.algorithm, self.lr, self.betas, self.eps, self.alpha = algorithm, float(lr), betas, float(eps), float(alpha)
        self.weight_decay, self.max_grad_norm = float(weight_decay), float(max_grad_norm) if max_grad_norm is not None else 0.0
        adam = algorithm == "adam"
        self.state1 = [torch.zeros_like(p) if adam else torch.ones_like(p) for p in self.params]   # exp_avg, or RMSpropTFLike's square_avg (ones)
        self.state2 = [torch.zeros_like(p) for p in self.params] if adam else [None] * len(self.params)   # exp_avg_sq
        self._carry = torch.zeros(4, dtype=torch.float64, device=self.device)   # int64 step, float64 b1pow, b2pow, unused
        self._set_carry(0)
        self._shadows: dict = {}   # id(param) -> (shadow's storage tensor, cols, pitch, module)
        self._targets: dict = {}   # id(param) -> target tensor
        self._table = self._table_key = self._workspace = None
        self._chunks = 0

    # ------------------------------------------------------------------ the carried state
    def _beta12(self) -> tuple:
        return (self.betas[0], self.betas[1]) if self.algorithm == "adam" else (self.alpha, 0.0)

    def _set_carry(self, step: int) -> None:
        """step, and beta ** step as the library carries it: the iterated float64 product."""
        b1 = b2 = 1.0
        if self.algorithm == "adam":
            for _ in range(int(step)):
                b1, b2 = b1 * self.betas[0], b2 * self.betas[1]
        host = np.zeros(4, np.float64)
        host.view(np.int64)[0] = int(step)
        host[1], host[2] = b1, b2
        self._carry.copy_(torch.from_numpy(host))

    # ------------------------------------------------------------------ attach / set_target
    def _index_of(self, t, what: str) -> int:
        for i, p in enumerate(self.params):
            if p is t:
                return i
        raise ValueError(f"{what} is not one of this optimiser's parameters")

    def attach(self, module) -> None:
        """Keep a bfloat16 copy of `module.weight` -- a RowLinear, RowExtractor (pitch 448), RowActor or RowDense whose weight this optimiser steps
        (a RowPolicy: every one of its layers) -- written by
        the update pass itself, and let the module read it in place of its per-call cast: `module.weight_bf16` is set together with the weight's
        `_version` at this moment, and the module uses the copy only while that version still holds.  Any torch in-place write (`load_state_dict`,
        `copy_` under no_grad) bumps the version: the module falls back to its cast, still correct, until `refresh()`.  A write through `.data` does NOT
        bump the version: call `refresh()` after one."""
        if isinstance(module, RowPolicy):   # every layer of the policy, in the table's order
            for layer in module.layers():
                self.attach(layer)
            return
        if not isinstance(module, (RowLinear, RowExtractor, RowActor, RowDense)):
            raise ValueError("attach takes a RowLinear, a RowExtractor, a RowActor, a RowDense or a RowPolicy")
        w = module.weight
        self._index_of(w, "module.weight")
        if isinstance(module, RowDense):
            module.apply_mask()   # a masked layer: the copy is masked_weight(), and the update pass keeps a zero at zero
        rows, cols = int(w.shape[0]), int(w.shape[1])
        pitch = cols + 1 if isinstance(module, RowExtractor) else cols   # 448: 16-byte lines, what bg_extractor_rows stages fastest
        store = torch.zeros((rows, pitch), dtype=torch.bfloat16, device=w.device)
        view = store[:, :cols] if pitch != cols else store
        view.copy_(w.detach())   # once, here; from now on the update pass and refresh() write it
        self._shadows[id(w)] = (store, cols, pitch, module)
        module.weight_bf16, module._weight_bf16_version = view, w._version
        self._table_key = None

    def refresh(self) -> None:
        """Write every attached bfloat16 copy from the current parameters (one launch) and record the weights' versions again: the remedy after
        `load_state_dict`, a `copy_`, or a write through `.data`.  The off-block entries of a masked `RowDense` are set to zero first."""
        ids = [i for i, p in enumerate(self.params) if id(p) in self._shadows]
        if not ids:
            return
        self._check_gpu()
        for i in ids:
            module = self._shadows[id(self.params[i])][3]
            if isinstance(module, RowDense):
                module.apply_mask()   # (after a load_state_dict with off-block entries: the copy is masked_weight() again)
        table, chunks = self._build_table(ids, shadow_only=True)
        args = (_ptr(table), len(ids), C.c_int64(chunks), nat.OPTIM_ADAM, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, C.c_uint32(nat.OPTIM_SHADOW_ONLY), None, None, None)
        _native_call("bg_optim_step", self.device, args, None, False)
        for i in ids:
            _, _, _, module = self._shadows[id(self.params[i])]
            module._weight_bf16_version = self.params[i]._version

    def set_target(self, params: Iterable[torch.Tensor], target_params: Iterable[torch.Tensor]) -> None:
        """Pair DQN's target network: `step(target_tau=tau)` then also does target = target * (1 - tau) + param * tau (SB3's polyak_update; tau 1.0
        every 1000 steps is the reference's setting, a plain copy) in the pass that wrote the parameter."""
        params, targets = list(params), list(target_params)
        if len(params) != len(targets):
            raise ValueError("params and target_params must pair up")
        for k, (p, t) in enumerate(zip(params, targets)):
            self._index_of(p, f"params[{k}]")
            _check_param(f"target_params[{k}]", t, self.device, p.shape)
            if t is p or (t.numel() and t.data_ptr() == p.data_ptr()):
                raise ValueError(f"target_params[{k}] is its own parameter")
        for p, t in zip(params, targets):
            self._targets[id(p)] = t
        self._table_key = None

    # ------------------------------------------------------------------ the table
    def _check_gpu(self) -> None:
        if self.device.type != "cuda":
            raise ValueError("the parameters must be device tensors (there is no CPU fallback)")

    def _build_table(self, ids: list, shadow_only: bool = False) -> tuple:
        ent = np.zeros(len(ids), _ENTRY)
        prefix = np.zeros(len(ids) + 1, np.uint32)
        for k, i in enumerate(ids):
            p = self.params[i]
            e = ent[k]
            e["param"], e["numel"], e["cols"], e["pitch"] = p.data_ptr(), p.numel(), 1, 1
            if not shadow_only:
                e["grad"], e["state1"] = p.grad.data_ptr(), self.state1[i].data_ptr()
                e["state2"] = self.state2[i].data_ptr() if self.state2[i] is not None else 0
                if id(p) in self._targets:
                    e["target"] = self._targets[id(p)].data_ptr()
            if id(p) in self._shadows:
                store, cols, pitch, _ = self._shadows[id(p)]
                e["shadow"], e["cols"], e["pitch"] = store.data_ptr(), cols, pitch
            prefix[k + 1] = prefix[k] + -(-p.numel() // nat.OPTIM_CHUNK)
        blob = ent.tobytes() + prefix.tobytes()
        blob += b"\0" * (-len(blob) % 16)
        table = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(self.device)
        return table, int(prefix[-1])

    # ------------------------------------------------------------------ the step
    def zero_grad(self) -> None:
        """Fill the existing gradients with zero (they are not set to None: the table keeps pointing at them)."""
        grads = [p.grad for p in self.params if p.grad is not None]
        if grads:
            torch._foreach_zero_(grads)

    def step(self, lr: Optional[float] = None, zero_grad: bool = True, target_tau: float = 0.0, timing: bool = False) -> OptimStats:
        """Clip, update, write shadows and targets, zero the gradients (zero_grad=True) -> `OptimStats`.  lr: this step's learning rate (default: the
        constructor's).  target_tau in [0, 1]: the polyak coefficient of the tensors paired by `set_target`, 0 leaves them alone.  The table of pointers
        is built on the host and uploaded again only when one of them has changed."""
        lr = self.lr if lr is None else lr
        if isinstance(lr, bool) or not isinstance(lr, (int, float)) or not 0.0 <= float(lr) < 1e30:
            raise ValueError("lr must be a number in [0, 1e30)")
        if isinstance(target_tau, bool) or not isinstance(target_tau, (int, float)) or not 0.0 <= float(target_tau) <= 1.0:
            raise ValueError("target_tau must be a number in [0, 1]")
        ids = [i for i, p in enumerate(self.params) if p.grad is not None]
        for i in ids:
            _check_param(f"params[{i}].grad", self.params[i].grad, self.device, self.params[i].shape)
        self._check_gpu()
        if not ids:
            raw = torch.zeros(nat.OPTIM_STATS_BYTES // 4, dtype=torch.int32, device=self.device)
            raw.view(torch.float32)[1] = 1.0
            raw.view(torch.int64)[3] = self._carry.view(torch.int64)[0]
            return OptimStats(raw, 0.0 if timing else None)
        key = tuple((i, self.params[i].data_ptr(), self.params[i].grad.data_ptr()) for i in ids)
        if key != self._table_key:
            self._table, self._chunks = self._build_table(ids)
            self._table_key = key
            size = int(nat.load().bg_optim_workspace_size(C.c_int64(self._chunks)))
            if self._workspace is None or self._workspace.numel() < size:
                self._workspace = torch.empty(size, dtype=torch.uint8, device=self.device)
        raw = torch.empty(nat.OPTIM_STATS_BYTES // 4, dtype=torch.int32, device=self.device)
        b1, b2 = self._beta12()
        args = (_ptr(self._table), len(ids), C.c_int64(self._chunks), nat.OPTIM_ALGORITHMS[self.algorithm], float(lr), b1, b2, self.eps, self.weight_decay,
                self.max_grad_norm, float(target_tau), C.c_uint32(nat.OPTIM_ZERO_GRAD if zero_grad else 0), _ptr(self._carry), _ptr(self._workspace), _ptr(raw))
        res = _native_call("bg_optim_step", self.device, args, (), timing)
        return OptimStats(raw, *res)

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self) -> dict:
        """Copies of the state (this reads the step count: one synchronisation)."""
        return {"algorithm": self.algorithm, "lr": self.lr, "betas": self.betas, "eps": self.eps, "alpha": self.alpha, "weight_decay": self.weight_decay,
                "max_grad_norm": self.max_grad_norm, "step": int(self._carry.view(torch.int64)[0]),
                "state1": [s.clone() for s in self.state1], "state2": [s.clone() if s is not None else None for s in self.state2]}

    def load_state_dict(self, state: dict) -> None:
        if state.get("algorithm") != self.algorithm or len(state.get("state1", ())) != len(self.params):
            raise ValueError(f"the state is not one of a {self.algorithm!r} RowOptimizer over {len(self.params)} tensors")
        for mine, theirs in zip(self.state1 + self.state2, list(state["state1"]) + list(state["state2"])):
            if (mine is None) != (theirs is None) or (mine is not None and tuple(mine.shape) != tuple(theirs.shape)):
                raise ValueError("the state's tensors do not have the parameters' shapes")
        for k in ("lr", "eps", "alpha", "weight_decay", "max_grad_norm"):
            setattr(self, k, float(state[k]))
        self.betas = tuple(float(b) for b in state["betas"])
        with torch.no_grad():
            for mine, theirs in zip(self.state1 + self.state2, list(state["state1"]) + list(state["state2"])):
                if mine is not None:
                    mine.copy_(theirs)
        self._set_carry(int(state["step"]))

    @classmethod
    def from_torch(cls, optimizer: torch.optim.Adam, max_grad_norm: Optional[float] = 0.5) -> "RowOptimizer":
        """A RowOptimizer over the parameters of a torch.optim.Adam with one parameter group, with its lr, betas, eps, weight_decay and -- where the
        Adam has stepped -- its exp_avg, exp_avg_sq and step (b1pow / b2pow are rebuilt by the iterated product)."""
        if not isinstance(optimizer, torch.optim.Adam) or isinstance(optimizer, torch.optim.AdamW) or len(optimizer.param_groups) != 1:
            raise ValueError("from_torch takes a torch.optim.Adam (not AdamW) with one parameter group")
        g = optimizer.param_groups[0]
        if g.get("amsgrad") or g.get("maximize") or isinstance(g["lr"], torch.Tensor):
            raise ValueError("from_torch: amsgrad, maximize and a tensor lr are out of scope")
        opt = cls(g["params"], lr=g["lr"], algorithm="adam", betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"], max_grad_norm=max_grad_norm)
        steps = set()
        with torch.no_grad():
            for i, p in enumerate(opt.params):
                st = optimizer.state.get(p)
                if st:
                    opt.state1[i].copy_(st["exp_avg"])
                    opt.state2[i].copy_(st["exp_avg_sq"])
                    steps.add(int(st["step"]))
        if len(steps) > 1:
            raise ValueError(f"from_torch: the parameters have stepped differently often ({sorted(steps)}): there is one step count here")
        opt._set_carry(steps.pop() if steps else 0)
        return opt

    def to_torch(self) -> torch.optim.Adam:
        """A torch.optim.Adam over the same parameters with this optimiser's hyperparameters, moments and step (one synchronisation)."""
        if self.algorithm != "adam":
            raise ValueError("to_torch: torch has no RMSpropTFLike")
        adam = torch.optim.Adam(self.params, lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay)
        step = int(self._carry.view(torch.int64)[0])
        if step:
            for p, m, v in zip(self.params, self.state1, self.state2):
                adam.state[p] = {"step": torch.tensor(float(step)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        return adam
