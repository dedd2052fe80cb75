"""RowPolicy: everything between the network's first layer and the env as ONE call of libbalatro_mi355x.so (bg_policy_forward, csrc/bg_policy.h).

A collection step over packed records is `RowExtractor` (one launch) -> `RowPolicy.act` (one launch) -> `env.step`: the hidden layers, `action_net`,
the masked draw with its log-probability and `value_net` run in one kernel that keeps a row's activations on the compute unit -- no hidden activation
and no logits matrix is written.  Training keeps torch autograd for the hidden layers: `RowPolicy.latent` is the same topology as plain `F.linear` in
bfloat16 and feeds `policy.action.ppo_loss`.

Two implementations of one network have one consequence.  `act`'s log_prob (float32 accumulation on the matrix cores in ascending 16-blocks of k, the
tanh of csrc/bg_policy.h) and the log_prob the first epoch computes through `latent` (rocBLAS' accumulation order, torch's tanh) are the same number up
to those roundings, each followed by the same rounding to bfloat16 per layer: PPO's first ratio is near 1, not exactly 1.  tests/policy_ref.py bounds
the kernel's side of that difference per layer; tests/test_policy_train.py holds |log_prob(act) - log_prob(latent)| below log(1.2) on every row (measured: at most
0.039 on the reference's topology).  There is no CPU fallback for `act` / `evaluate`.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _native as nat
from .rows import RowActor, _check_counters, _check_device, _check_h, _check_mask_aligned, _check_scan_tensor, _head_mask, _live_shadow, _native_call, _ptr

_LAYER = np.dtype([("weight", "<u8"), ("bias", "<u8"), ("pitch", "<u4"), ("in", "<u2"), ("out", "<u2"), ("act", "<u4"), ("reserved", "<u4")])
_NET = np.dtype([("n_trunk", "<u4"), ("n_pi", "<u4"), ("n_vf", "<u4"), ("has_value", "<u4"), ("in0", "<u4"), ("reserved", "<u4", (3,)),
                 ("layer", _LAYER, (nat.POLICY_MAX_LAYERS,))])
assert _LAYER.itemsize == nat.POLICY_LAYER_BYTES and _NET.itemsize == nat.POLICY_NET_BYTES


def _check_policy_width(what: str, w: int) -> int:
    w = int(w)
    if w < nat.POLICY_WIDTH_MIN or w > nat.POLICY_WIDTH_MAX or w % 32:
        raise ValueError(f"{what} must be a multiple of 32 in [{nat.POLICY_WIDTH_MIN}, {nat.POLICY_WIDTH_MAX}] (got {w})")
    return w


class RowDense(torch.nn.Module):
    """One dense layer of a `RowPolicy`: float32 parameters `weight` [out_features, in_features] and `bias` [out_features], initialised as nn.Linear;
    activation None, "relu" or "tanh".  in_features and out_features: multiples of 32 in [32, 512]; out_features 1 is the value layer.  The launch reads
    a bfloat16 copy of the weight: the one `RowOptimizer.attach` keeps while it is current (`weight_bf16`, the shadow protocol of `RowActor`), else a
    cast per call.  mask: a 0 / 1 float32 [out_features, in_features] buffer (`block_mask`); `forward` multiplies the weight by it, so the gradient of an
    off-block entry is exactly zero and an entry that is zero stays zero under Adam and RMSprop, with L2 weight decay too (its term is wd * 0).
    THE INVARIANT of a masked layer: whatever a launch, an attached copy or `to_linear()` reads is `masked_weight()`.  It holds because the parameter
    itself obeys the mask wherever its raw value is read: the constructor zeroes the off-block entries (+0.0) behind nn.Linear's initialisation,
    `RowOptimizer.attach` and `RowOptimizer.refresh()` zero them again (`apply_mask`) before they copy the weight and record its version, the per-call
    cast and `to_linear()` go through `masked_weight()`, and `load_state_dict` bumps the version, so the masked cast serves until `refresh()`.
    `forward(x)` is the torch path (training): F.linear in x's dtype, then the activation."""

    def __init__(self, in_features: int, out_features: int, activation: Optional[str] = None, mask: Optional[torch.Tensor] = None, device=None):
        super().__init__()
        if activation not in nat.POLICY_ACTIVATIONS:
            raise ValueError(f"activation must be None, 'relu' or 'tanh' (got {activation!r})")
        in_features = _check_policy_width("in_features", in_features)
        out_features = int(out_features)
        if out_features != 1:
            _check_policy_width("out_features", out_features)
        self.in_features, self.out_features, self.activation = in_features, out_features, activation
        lin = torch.nn.Linear(in_features, out_features, device=device)   # nn.Linear's own initialisation
        self.weight = torch.nn.Parameter(lin.weight.detach().clone())
        self.bias = torch.nn.Parameter(lin.bias.detach().clone())
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (out_features, in_features):
                raise ValueError(f"mask must be a tensor [{out_features}, {in_features}]")
            mask = (mask != 0).to(dtype=torch.float32, device=self.weight.device)
        self.register_buffer("block_mask", mask)
        self.apply_mask()
        self.weight_bf16, self._weight_bf16_version = None, -1   # RowOptimizer.attach: a bfloat16 copy kept by the update pass (`_live_shadow`)

    @classmethod
    def from_linear(cls, linear: torch.nn.Linear, activation: Optional[str] = None) -> "RowDense":
        if not isinstance(linear, torch.nn.Linear) or linear.bias is None:
            raise ValueError("from_linear takes an nn.Linear with a bias")
        layer = cls(linear.in_features, linear.out_features, activation, device=linear.weight.device)
        with torch.no_grad():
            layer.weight.copy_(linear.weight)
            layer.bias.copy_(linear.bias)
        return layer

    def to_linear(self) -> torch.nn.Linear:
        lin = torch.nn.Linear(self.in_features, self.out_features, device=self.weight.device)
        with torch.no_grad():
            lin.weight.copy_(self.masked_weight())
            lin.bias.copy_(self.bias)
        return lin

    def apply_mask(self) -> None:
        """Set the off-block entries of the parameter to +0.0 (the invariant above).  Written through `.data`: the weight's version does not move, so
        the callers that copy the weight right behind it (`RowOptimizer.attach`, `refresh()`) record the version they read."""
        if self.block_mask is not None:
            self.weight.data.masked_fill_(self.block_mask == 0, 0.0)

    def masked_weight(self) -> torch.Tensor:
        return self.weight if self.block_mask is None else self.weight * self.block_mask

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        y = torch.nn.functional.linear(x, self.masked_weight().to(x.dtype), self.bias.to(x.dtype))
        return torch.relu(y) if self.activation == "relu" else torch.tanh(y) if self.activation == "tanh" else y

    def _w(self) -> torch.Tensor:
        """The bfloat16 weight a launch reads: the attached copy while it is current, else a cast (correct, slower)."""
        wb = _live_shadow(self)
        return wb if wb is not None else self.masked_weight().detach().to(torch.bfloat16).contiguous()

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}, activation={self.activation!r}, masked={self.block_mask is not None}"


def _section(name: str, layers) -> list:
    layers = list(layers)
    if len(layers) > nat.POLICY_MAX_SECTION:
        raise ValueError(f"{name} holds {len(layers)} layers: a section holds at most {nat.POLICY_MAX_SECTION}")
    for k, layer in enumerate(layers):
        if not isinstance(layer, RowDense) or layer.out_features == 1:
            raise ValueError(f"{name}[{k}] must be a RowDense with out_features a multiple of 32")
    return layers


def _pairs(name: str, pairs) -> list:
    out = []
    for k, p in enumerate(pairs):
        if not (isinstance(p, (tuple, list)) and len(p) == 2 and isinstance(p[0], torch.nn.Linear)):
            raise ValueError(f"{name}[{k}] must be a pair (nn.Linear, activation)")
        out.append(RowDense.from_linear(p[0], p[1]))
    return out


class RowPolicy(torch.nn.Module):
    """A policy network behind its first layer (module docstring): `trunk`, then `pi` and `vf` (lists of at most four `RowDense` each; both branches
    read the trunk's output, or h where the trunk is empty), `action` (a `RowActor` over pi's output) and `value` (a `RowDense(latent_vf, 1)`, or None:
    no values).  Every width is a multiple of 32 in [32, 512].

        policy = RowPolicy.from_modules(trunk=[(combined[0], "relu"), (combined[2], "relu")], pi=[(p0, "tanh"), (p1, "tanh")],
                                        vf=[(v0, "tanh"), (v1, "tanh")], action_net=sb3.action_net, value_net=sb3.value_net)
        actions, log_prob, values, _ = policy.act(h, env.obs_rows, seed=seed, t=t)     # collection: one launch
        latent_pi, values = policy.latent(h)                                           # training: torch autograd
        loss, stats = policy.action.ppo_loss(latent_pi, actions, old_log_prob, advantages, rows, values=values, returns=returns)

    `opt.attach(policy)` keeps every layer's bfloat16 copy current; a layer without one is cast per call."""

    def __init__(self, trunk: Sequence[RowDense], pi: Sequence[RowDense], vf: Sequence[RowDense], action: RowActor, value: Optional[RowDense] = None):
        super().__init__()
        trunk, pi, vf = _section("trunk", trunk), _section("pi", pi), _section("vf", vf)
        if not isinstance(action, RowActor):
            raise ValueError("action must be a RowActor")
        if value is not None and (not isinstance(value, RowDense) or value.out_features != 1 or value.activation is not None):
            raise ValueError("value must be a RowDense(latent_vf, 1) without activation, or None")
        if vf and value is None:
            raise ValueError("vf layers need the value layer: vf given without value")
        first = (trunk or pi or [action])[0]
        self.in_features = _check_policy_width("in_features", first.in_features)
        width = self.in_features
        for name, chain, last in (("trunk", trunk, None), ("pi", pi, action), ("vf", vf, value)):
            w = width
            for k, layer in enumerate(chain + ([last] if last is not None else [])):
                if layer.in_features != w:
                    what = f"{name}[{k}]" if k < len(chain) else ("action" if last is action else "value")
                    raise ValueError(f"{what} reads {layer.in_features} features where the layer in front of it gives {w}")
                w = layer.out_features
            if name == "trunk":
                width = w
        _check_policy_width("action.in_features", action.in_features)
        self.trunk, self.pi, self.vf = torch.nn.ModuleList(trunk), torch.nn.ModuleList(pi), torch.nn.ModuleList(vf)
        self.action, self.value = action, value
        self._table_key = self._table = self._keep = None

    # ------------------------------------------------------------------ SB3's modules, both ways
    @classmethod
    def from_modules(cls, trunk=(), pi=(), vf=(), *, action_net: torch.nn.Linear, value_net: Optional[torch.nn.Linear] = None) -> "RowPolicy":
        """trunk / pi / vf: lists of (nn.Linear, activation) pairs; action_net: nn.Linear(latent_pi, 60); value_net: nn.Linear(latent_vf, 1) or None.
        The parameters are copied exactly (float32)."""
        value = None
        if value_net is not None:
            if not isinstance(value_net, torch.nn.Linear) or value_net.out_features != 1:
                raise ValueError("value_net must be an nn.Linear(latent_vf, 1)")
            value = RowDense.from_linear(value_net, None)
        return cls(_pairs("trunk", trunk), _pairs("pi", pi), _pairs("vf", vf), RowActor.from_linear(action_net), value)

    def to_modules(self) -> dict:
        """-> {"trunk": [(nn.Linear, activation), ...], "pi": [...], "vf": [...], "action_net": nn.Linear, "value_net": nn.Linear or None}: copies."""
        return {"trunk": [(l.to_linear(), l.activation) for l in self.trunk], "pi": [(l.to_linear(), l.activation) for l in self.pi],
                "vf": [(l.to_linear(), l.activation) for l in self.vf], "action_net": self.action.to_linear(),
                "value_net": self.value.to_linear() if self.value is not None else None}

    @staticmethod
    def stack_blocks(linears: Sequence[torch.nn.Linear], activation: Optional[str] = "relu") -> RowDense:
        """Parallel layers over consecutive column ranges as ONE block-diagonal `RowDense` with its mask: the extractor's three second layers
        (256 -> 128, 128 -> 64, 64 -> 32) become a [224, 448] layer over `RowExtractor.from_linears`' output.  Off-block entries are zero and, through
        the mask, stay zero."""
        linears = list(linears)
        if not linears or any(not isinstance(l, torch.nn.Linear) or l.bias is None for l in linears):
            raise ValueError("stack_blocks takes nn.Linear layers with biases")
        rows, cols = sum(l.out_features for l in linears), sum(l.in_features for l in linears)
        mask = torch.zeros((rows, cols))
        r = c = 0
        for l in linears:
            mask[r:r + l.out_features, c:c + l.in_features] = 1.0
            r, c = r + l.out_features, c + l.in_features
        layer = RowDense(cols, rows, activation, mask=mask, device=linears[0].weight.device)
        with torch.no_grad():
            layer.weight.zero_()
            r = c = 0
            for l in linears:
                layer.weight[r:r + l.out_features, c:c + l.in_features] = l.weight
                layer.bias[r:r + l.out_features] = l.bias
                r, c = r + l.out_features, c + l.in_features
        return layer

    def layers(self) -> list:
        """Every layer in the table's order: trunk, pi, vf, action, value."""
        return list(self.trunk) + list(self.pi) + list(self.vf) + [self.action] + ([self.value] if self.value is not None else [])

    @property
    def tap_cols(self) -> int:
        return sum(l.out_features for l in list(self.trunk) + list(self.pi) + list(self.vf))

    # ------------------------------------------------------------------ the training path
    def latent(self, h: torch.Tensor):
        """-> (latent_pi, values float32 [...] or None): the torch path, under autograd -- each layer is F.linear in h's dtype (bfloat16) with the
        parameters cast to it, then its activation, exactly what the same nn.Linear modules give after `.to(torch.bfloat16)`."""
        x = h
        for layer in self.trunk:
            x = layer(x)
        p = v = x
        for layer in self.pi:
            p = layer(p)
        if self.value is None:
            return p, None
        for layer in self.vf:
            v = layer(v)
        return p, self.value(v).float().squeeze(-1)

    # ------------------------------------------------------------------ the launch
    def _net(self):
        """The host table (built once per parameter version: reused while every layer's bfloat16 copy is the attached one and no version moved)."""
        layers = self.layers()
        shadows = [_live_shadow(l) for l in layers]
        key = tuple((l.weight.data_ptr(), l.weight._version, l.bias.data_ptr(), l.bias._version, None if s is None else s.data_ptr()) for l, s in zip(layers, shadows))
        if all(s is not None for s in shadows) and key == self._table_key:
            return self._table
        net = np.zeros(1, _NET)
        n = net[0]
        n["n_trunk"], n["n_pi"], n["n_vf"], n["has_value"], n["in0"] = len(self.trunk), len(self.pi), len(self.vf), int(self.value is not None), self.in_features
        keep = []
        for k, (l, s) in enumerate(zip(layers, shadows)):
            w = s if s is not None else (l._w() if isinstance(l, RowDense) else l.weight.detach().to(torch.bfloat16).contiguous())
            b = l.bias.detach()
            keep += [w, b]
            e = n["layer"][k]
            e["weight"], e["bias"], e["pitch"], e["in"], e["out"] = w.data_ptr(), b.data_ptr(), int(w.stride(0)), l.in_features, l.out_features
            e["act"] = nat.POLICY_ACTIVATIONS[getattr(l, "activation", None)]
        self._table, self._keep = net, keep
        self._table_key = key if all(s is not None for s in shadows) else None
        return net

    def _call(self, h, mask, given, flags: int, seed: int, index0: int, t: int, entropy: bool, taps: bool, timing: bool):
        lead, m, _, pitch = _check_h(h, "h must be a torch.bfloat16 tensor [..., in_features] (the first layer's output)", (self.in_features,),
                                     f"the last dimension of h must be in_features = {self.in_features} (got %d)")
        dev = h.device
        mask, moff, mstride = _head_mask(mask, lead, dev)
        _check_counters(seed, index0, t)
        if given is not None:   # (the only tensor of `_head_outputs` that is the caller's: every output is allocated below)
            _check_scan_tensor("actions", given, torch.int32, lead, dev)
        if self.action.weight.device != dev:
            raise ValueError(f"the policy's parameters are on {self.action.weight.device}, h is on {dev}")
        _check_device(h.detach(), "h")
        _check_mask_aligned(mask, moff)
        actions = given if given is not None else torch.empty(lead, dtype=torch.int32, device=dev)
        log_prob = torch.empty(lead, dtype=torch.float32, device=dev)
        ent = torch.empty(lead, dtype=torch.float32, device=dev) if entropy else None
        values = torch.empty(lead, dtype=torch.float32, device=dev) if self.value is not None else None
        tap = torch.empty(lead + (self.tap_cols,), dtype=torch.bfloat16, device=dev) if taps else None
        logits = torch.empty(lead + (60,), dtype=torch.float32, device=dev) if taps else None
        res = ((log_prob, ent, values) if given is not None else (actions, log_prob, values, ent)) + ((tap, logits) if taps else ())
        if m == 0:
            return _native_call("bg_policy_forward", dev, (), res, timing, empty=True)
        net = self._net()
        args = (net.ctypes.data, _ptr(h.detach()), C.c_uint64(pitch), mask.data_ptr() + moff if mask is not None else None, C.c_uint64(mstride), C.c_int64(m),
                C.c_uint32(flags), C.c_uint64(int(seed)), C.c_uint64(int(index0)), C.c_uint64(int(t)), _ptr(actions), _ptr(log_prob), _ptr(ent), _ptr(values),
                _ptr(tap), C.c_uint64(self.tap_cols), _ptr(logits), C.c_uint64(60))
        return _native_call("bg_policy_forward", dev, args, res, timing)

    def act(self, h: torch.Tensor, mask: Optional[torch.Tensor] = None, *, seed: int, t: int, index0: int = 0, deterministic: bool = False,
            entropy: bool = False, taps: bool = False, timing: bool = False):
        """-> (actions int32, log_prob, values, entropy), each [...]: one launch, no autograd (inputs are detached).  h: bfloat16 [..., in_features] with
        a row pitch that is a multiple of 8 (what `RowExtractor` / `RowLinear` return, or a column slice of it); mask, seed, t, index0, deterministic: as
        `sample_actions`, and the draw is bit for bit `sample_actions` on this call's logits.  values is None without a value layer, entropy None unless
        asked for.  taps=True (tests): two more results, the bfloat16 [..., tap_cols] outputs of every hidden layer in table order and the float32
        [..., 60] logits; no other result changes by a bit.  timing=True appends the kernel milliseconds."""
        return self._call(h, mask, None, nat.HEAD_DETERMINISTIC if deterministic else 0, seed, index0, t, entropy, taps, timing)

    def evaluate(self, h: torch.Tensor, actions: torch.Tensor, mask: Optional[torch.Tensor] = None, *, taps: bool = False, timing: bool = False):
        """-> (log_prob, entropy, values) of given int32 actions [...] under the distribution `act` draws from: bit for bit `evaluate_actions` on this
        call's logits (a forward pass; the training path is `latent`)."""
        if not isinstance(actions, torch.Tensor):
            raise ValueError("actions must be an int32 tensor with the leading shape of h")
        return self._call(h, mask, actions, nat.POLICY_EVALUATE, 0, 0, 0, True, taps, timing)
