"""The learner's side of the packed-record path: everything that works on records or logits and needs no env -- encode_rows, the linear layer,
the masked policy head, the PPO, DQN and behaviour-cloning losses, the replay ring, the demonstration ring, GAE, the episode statistics / limits / endings / outcomes, the curriculum
and VecNormalize.

All of it runs in libbalatro_mi355x.so (hand-written HIP, the stateless entry points of csrc/bg_rows_api.h); torch only owns device buffers and the
stream.  There is no CPU fallback.  `vec_env` re-imports every public name, so `from balatro_gym_amd.vec_env import X` keeps working.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _native as nat


# ---------------------------------------------------------------------- what every call below shares
def _check_records(rows, dims: Optional[int] = None) -> tuple:
    """Packed records: a contiguous uint8 tensor [..., stride] of any rank (dims None) or of exactly `dims` dimensions (3: [K, N, stride]), the
    stride a multiple of 16, >= ROW_BYTES -> (leading shape, stride)."""
    if not isinstance(rows, torch.Tensor) or rows.dtype != torch.uint8 or (rows.dim() < 1 if dims is None else rows.dim() != dims) or not rows.is_contiguous():
        raise ValueError(f"rows must be a contiguous uint8 tensor {'[K, N, stride]' if dims == 3 else '[..., stride]'} of packed records")
    stride = int(rows.shape[-1])
    if stride < nat.ROW_BYTES or stride % 16:
        raise ValueError(f"the last dimension of rows is the record stride: a multiple of 16, >= {nat.ROW_BYTES} (got {stride})")
    return tuple(rows.shape[:-1]), stride


def _check_device(t: torch.Tensor, what: str = "rows", align: int = 16) -> None:
    """The tensor the library reads through its data_ptr() is on a GPU and (align > 0) starts on an `align`-byte boundary.  Every call makes this its
    last refusal before it allocates: the shape and dtype refusals come first, whatever the device."""
    if not t.is_cuda:
        raise ValueError(f"{what} must be a device tensor (there is no CPU fallback)")
    if align and t.data_ptr() % align:
        raise ValueError(f"{what} must be {align}-byte aligned")


def _native_call(name: str, dev: torch.device, args: tuple, result, timing: bool, empty: bool = False):
    """The call of a stateless entry point: `name(*args, kernel_ms_out, stream)` with `dev` the current device, the stream torch's current stream
    of `dev`, kernel_ms_out a float the library fills (timing) or NULL.  A non-zero return raises NativeError with `name` and bg_last_error's text.
    empty: the shape holds nothing to launch -- the library is neither loaded nor called, the time is 0.0.
    Returns `result`; with timing the kernel milliseconds join it: result + (ms,) where result is a tuple, (result, ms) otherwise."""
    ms = C.c_float(0.0)
    if not empty:
        L = nat.load()
        fn = getattr(L, name)
        if fn.argtypes is None:   # addresses travel as plain ints (`_ptr`): without declared argtypes ctypes would cut them to 32 bits
            raise nat.NativeError(f"{name} has no argtypes: declare them in _native.load()")
        with torch.cuda.device(dev):
            rc = fn(*args, C.byref(ms) if timing else None, torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise nat.NativeError(f"{name} failed ({rc}): {L.bg_last_error(None).decode()}")
    if not timing:
        return result
    return result + (float(ms.value),) if isinstance(result, tuple) else (result, float(ms.value))


def _check_norm(norm, rows: torch.Tensor, layout: str, instead: str) -> None:
    """The `norm=` of encode_rows and the linear layer: a RowNormalizer that normalises observations, on the rows' device, over the env's keys."""
    if not isinstance(norm, RowNormalizer):
        raise ValueError("norm must be a RowNormalizer")
    if not norm.norm_obs:
        raise ValueError(f"this RowNormalizer was made with norm_obs=False: {instead}")
    if layout not in ("produced", "fixed"):
        raise ValueError(f"layout must be 'produced' or 'fixed' with norm (got {layout!r}): VecNormalize wraps the env's keys, not the extractor's tensors")
    if norm.device != rows.device:
        raise ValueError(f"norm holds its statistics on {norm.device}, rows are on {rows.device}")
    if not (np.isfinite(norm.epsilon) and norm.epsilon >= 0.0 and np.isfinite(norm.clip_obs) and norm.clip_obs >= 0.0):
        raise ValueError("norm.epsilon and norm.clip_obs must be finite and >= 0")


def _norm_args(norm) -> tuple:
    """(mean_dev, var_dev, epsilon, clip_obs) of bg_encode_rows_ex and the linear layer; without a normaliser NULL, NULL, 0, 0."""
    if norm is None:
        return None, None, 0.0, 0.0
    return norm.obs_mean.data_ptr(), norm.obs_var.data_ptr(), norm.epsilon, norm.clip_obs


def _zero_where(mask, n: int, device: torch.device, *tensors) -> None:
    """Zero the per-env state `tensors` ([n] or [n, ...]) of the envs where `mask` ([n], anything torch.as_tensor takes) is set; None: of all."""
    if mask is None:
        for t in tensors:
            t.zero_()
        return
    mask = torch.as_tensor(mask)
    if tuple(mask.shape) != (n,):
        raise ValueError(f"mask must have shape [{n}]")
    mask = mask.to(device=device, dtype=torch.bool)
    for t in tensors:
        t.masked_fill_(mask.view((n,) + (1,) * (t.dim() - 1)), 0)


def _ptr(t):
    """A tensor's address as an entry point with declared argtypes takes it (ctypes converts the int to void*); None is NULL."""
    return None if t is None else t.data_ptr()


def _check_index(index, shape: Optional[tuple], device: torch.device) -> None:
    """The `index=` of ppo_loss and encode_rows (SB3's `RolloutBuffer.get` permutation): contiguous int32 on `device`, of `shape` (None: any [m])."""
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or (tuple(index.shape) != shape if shape is not None else index.dim() != 1) \
            or not index.is_contiguous() or index.device != device:
        raise ValueError(f"index must be a contiguous torch.int32 tensor of shape {list(shape) if shape is not None else '[m]'} on {device}")


def _row_pitch(t: torch.Tensor, width: int, lone_row_is_width: bool) -> tuple:
    """Is `t` (at least one dimension, rows of at least `width` elements) "last dimension contiguous, leading dimensions one run of rows", and at which
    pitch -> (ok, row pitch in elements).  One dimension: the pitch is `width`.  Where shape[-2] <= 1 the callers have two conventions, and each
    keeps its own:
      lone_row_is_width False  stride(-2) all the same: `encode_rows`' out; the logits of the head and loss calls; an int8 mask, in every call
      lone_row_is_width True   `width`: h of the actor calls and of `RowPolicy`; logits_out / dlogits_out of the actor calls"""
    stride, shape = t.stride(), t.shape
    pitch = stride[-2] if len(stride) >= 2 and not (lone_row_is_width and shape[-2] <= 1) else width
    ok = stride[-1] == 1 and pitch >= width
    for d in range(len(stride) - 2, 0, -1):   # leading dimensions: one run of rows `pitch` elements apart
        ok = ok and stride[d - 1] == stride[d] * shape[d]
    return ok, pitch


def _check_counters(*values, names: tuple = ("seed", "index0", "t")) -> None:
    """The words of the counter hash: each an integer (no bool) in [0, 2**64), refused in the order passed (`names`: that order, where it is another)."""
    for k, v in enumerate(values):
        if type(v) is int and 0 <= v < 2 ** 64:   # (the common case, at a third of the cost of the full test)
            continue
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 0 <= int(v) < 2 ** 64:
            raise ValueError(f"{names[k]} must be an integer in [0, 2**64)")


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
    lead, stride = _check_records(rows)
    D = nat.ENC_COLS[nat.ENC_LAYOUTS[layout]]
    store_rows = int(np.prod(lead, dtype=np.int64))
    if index is not None:
        _check_index(index, None, rows.device)
        if store_rows >= 2 ** 31:
            raise ValueError("the stored records hold at most 2**31 - 1 rows")
        lead = (int(index.shape[0]),)
    if norm is not None:
        _check_norm(norm, rows, layout, "use encode_rows without norm")
    m = int(np.prod(lead, dtype=np.int64))
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != dtype or out.device != rows.device:
            raise ValueError(f"out must be a {dtype} tensor on {rows.device}")
        if tuple(out.shape[:-1]) != lead or out.shape[-1] < D:
            raise ValueError(f"out must have shape {lead + ('>= %d' % D,)} (got {tuple(out.shape)})")
        dense, pitch = _row_pitch(out, int(out.shape[-1]), False)
        if not dense:
            raise ValueError("out must have a contiguous last dimension and leading dimensions that are dense over its row pitch")
    _check_device(rows)
    if out is None:
        out = torch.empty(lead + (D,), dtype=dtype, device=rows.device)
        pitch = D
    odt = nat.ENC_F32 if dtype == torch.float32 else nat.ENC_BF16
    tail = (out.data_ptr(), C.c_uint64(pitch))
    if index is None and norm is None:
        name, args = "bg_encode_rows", (_ptr(rows), C.c_uint64(stride), C.c_int64(m), nat.ENC_LAYOUTS[layout], odt, *tail)
    else:
        name, args = "bg_encode_rows_ex", (_ptr(rows), C.c_uint64(stride), C.c_int64(store_rows), _ptr(index), C.c_int64(m), nat.ENC_LAYOUTS[layout], odt,
                                           *_norm_args(norm), *tail)
    return _native_call(name, rows.device, args, out[..., :D], timing, empty=m == 0)   # (empty: an empty tensor has no pointer to hand over)


# ---------------------------------------------------------------------- the first layers: linear_rows and extractor_rows
def _first_layer_common(rows, index, activation):
    """The arguments every first-layer call shares -> (stride, store_rows, m).  Every refusal is a ValueError before the library is loaded."""
    if activation not in nat.LIN_ACTIVATIONS:
        raise ValueError(f"activation must be None or 'relu' (got {activation!r}): tanh stays in torch")
    lead, stride = _check_records(rows)
    store_rows = int(np.prod(lead, dtype=np.int64))
    m = store_rows
    if index is not None:
        _check_index(index, None, rows.device)
        if store_rows >= 2 ** 31:
            raise ValueError("the stored records hold at most 2**31 - 1 rows")
        m = int(index.shape[0])
    return stride, store_rows, m


def _linear_common(rows, index, norm, layout, activation):
    """`_first_layer_common` with linear_rows' layout in front of it and its norm behind it."""
    if layout not in ("produced", "fixed"):
        raise ValueError(f"layout must be 'produced' or 'fixed' (got {layout!r}): the extractor's one-hot columns want an embedding gather, not this layer")
    shape = _first_layer_common(rows, index, activation)
    if norm is not None:
        _check_norm(norm, rows, layout, "call without norm")
    return shape


def _check_width(H: int, what: str = "the layer's width") -> None:
    if H < 32 or H > 4096 or H % 32:
        raise ValueError(f"{what} must be a multiple of 32 in [32, 4096] (got {H})")


def _dtype_code(dtype: torch.dtype) -> int:
    return nat.ENC_F32 if dtype == torch.float32 else nat.ENC_BF16


def _linear_matrix(name: str, t, dtypes: tuple, m: int, H: int, device: torch.device) -> int:
    """A [m, >= H] matrix with a contiguous last dimension -> its row pitch in elements."""
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.device != device or t.dim() != 2 or t.shape[0] != m or t.shape[1] < H \
            or t.stride(1) != 1 or (m > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f"{name} must be a {' / '.join(str(d) for d in dtypes)} tensor [{m}, >= {H}] on {device} with a contiguous last dimension")
    return int(t.stride(0)) if m > 1 else int(t.shape[1])


def _check_vector(name: str, t, H: int, device: torch.device) -> None:
    """bias / dbias: a contiguous float32 [H] on the rows' device."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (H,) or not t.is_contiguous() or t.device != device:
        raise ValueError(f"{name} must be a contiguous torch.float32 tensor [{H}] on {device}")


def _forward_out(rows, weight, bias, H: int, dtype, out, m: int) -> tuple:
    """What a forward checks behind its weight -- the weight's device, bias, dtype, out -- and, behind the device check, the allocation -> (out, its pitch)."""
    if weight.device != rows.device:
        raise ValueError(f"weight must be on {rows.device}")
    if bias is not None:
        _check_vector("bias", bias, H, rows.device)
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("dtype must be torch.float32 or torch.bfloat16")
    pitch = _linear_matrix("out", out, (dtype,), m, H, rows.device) if out is not None else H
    _check_device(rows)
    if out is None:
        out = torch.empty((m, H), dtype=dtype, device=rows.device)
    return out, pitch


def _grad_matrices(rows, dout, out, dweight, activation, m: int) -> tuple:
    """What a gradient checks in front of its dweight: dout, the width, out against the activation -> (H, dout's pitch, relu, out's pitch)."""
    if not isinstance(dout, torch.Tensor) or dout.dim() != 2:
        raise ValueError("dout must be a float32 / bfloat16 tensor [m, H]")
    H = int(dweight.shape[0]) if isinstance(dweight, torch.Tensor) and dweight.dim() == 2 else int(dout.shape[1])
    _check_width(H)
    dpitch = _linear_matrix("dout", dout, (torch.float32, torch.bfloat16), m, H, rows.device)
    relu = activation == "relu"
    if relu != (out is not None):
        raise ValueError("out (the forward's output) is required with activation='relu' and must be None without it")
    opitch = _linear_matrix("out", out, (torch.float32, torch.bfloat16), m, H, rows.device) if relu else 0
    return H, dpitch, relu, opitch


def _grad_call(name: str, rows, head: tuple, m: int, K: int, dout, dpitch: int, out, opitch: int, H: int, activation, dweight, dbias, workspace, timing: bool):
    """A gradient behind its checks: an empty call zeroes what it would have written; otherwise the workspace (made here unless the caller gave one) and
    the call `name(*head, dout .. workspace)`.  Returns (dweight, dbias), with timing the kernel milliseconds behind them."""
    if m == 0:
        dweight[:, :K] = 0.0
        if dbias is not None:
            dbias.zero_()
        return _native_call(name, rows.device, (), (dweight, dbias), timing, empty=True)
    need = int(getattr(nat.load(), name.replace("_grad", "_workspace_bytes"))(C.c_int64(m), H))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=rows.device)
    elif not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.device != rows.device or not workspace.is_contiguous() \
            or workspace.numel() < need:
        raise ValueError(f"workspace must be a contiguous uint8 tensor of >= {need} bytes on {rows.device}")
    args = head + (_ptr(dout), _dtype_code(dout.dtype), C.c_uint64(dpitch), _ptr(out), _dtype_code(out.dtype) if out is not None else 0, C.c_uint64(opitch), H,
                   nat.LIN_ACTIVATIONS[activation], _ptr(dweight), C.c_uint64(int(dweight.stride(0))), _ptr(dbias), _ptr(workspace), C.c_uint64(workspace.numel()))
    return _native_call(name, rows.device, args, (dweight, dbias), timing)


def _grad_as_dout(grad: torch.Tensor) -> torch.Tensor:
    """autograd's gradient as a gradient call takes dout: as it is when it is a float32 / bfloat16 matrix with a contiguous last dimension, else a copy."""
    if grad.dtype in (torch.float32, torch.bfloat16) and grad.dim() == 2 and grad.stride(1) == 1 and (grad.shape[0] <= 1 or grad.stride(0) >= grad.shape[1]):
        return grad
    return grad.to(torch.float32).contiguous()


def _live_shadow(module):
    """The bfloat16 copy of `module.weight` that `RowOptimizer.attach` keeps (balatro_gym_amd/optim.py), or None: it is used only while the version
    recorded with it is still the weight's `_version` -- any torch in-place write to the weight bumps that, and the module casts again until
    `RowOptimizer.refresh()`.  (A write through `.data` does not bump it: call `refresh()` after one.)"""
    wb = module.weight_bf16
    return wb if wb is not None and module._weight_bf16_version == module.weight._version else None


class _RowFirstLayer(torch.nn.Module):
    """What RowLinear and RowExtractor share: the constructor's checks, float32 parameters initialised as nn.Linear(in_features, out_features), and the
    copies to and from an nn.Linear."""

    def __init__(self, in_features: int, out_features: int, activation: Optional[str], dtype: torch.dtype, device):
        super().__init__()
        if activation not in nat.LIN_ACTIVATIONS:
            raise ValueError(f"activation must be None or 'relu' (got {activation!r}): tanh stays in torch")
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("dtype must be torch.float32 or torch.bfloat16")
        out_features = int(out_features)
        _check_width(out_features, "out_features")
        self.in_features, self.out_features, self.activation, self.dtype = in_features, out_features, activation, dtype
        lin = torch.nn.Linear(in_features, out_features, device=device)   # nn.Linear's own initialisation
        self.weight = torch.nn.Parameter(lin.weight.detach().clone())
        self.bias = torch.nn.Parameter(lin.bias.detach().clone())
        self.weight_bf16, self._weight_bf16_version = None, -1   # RowOptimizer.attach: a bfloat16 copy kept by the update pass (`_live_shadow`)

    def _load(self, linear: torch.nn.Linear):
        with torch.no_grad():
            self.weight.copy_(linear.weight)
            self.bias.copy_(linear.bias)
        return self

    def to_linear(self) -> torch.nn.Linear:
        lin = torch.nn.Linear(self.in_features, self.out_features, device=self.weight.device)
        with torch.no_grad():
            lin.weight.copy_(self.weight)
            lin.bias.copy_(self.bias)
        return lin

    def _check_same_gpu(self, rows: torch.Tensor) -> None:
        if not rows.is_cuda or self.weight.device != rows.device:
            raise ValueError("rows and the layer must be on the same GPU (there is no CPU fallback)")


def _linear_weight(weight) -> int:
    if not isinstance(weight, torch.Tensor) or weight.dtype != torch.bfloat16 or weight.dim() != 2 or weight.shape[1] not in (nat.LIN_K, nat.ENC_COLS[nat.ENC_FIXED]) \
            or not weight.is_contiguous():
        raise ValueError("weight must be a contiguous torch.bfloat16 tensor [H, 153] or [H, 628] (nn.Linear.weight's orientation)")
    H = int(weight.shape[0])
    _check_width(H)
    return H


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
    out, pitch = _forward_out(rows, weight, bias, H, dtype, out, m)
    args = (_ptr(rows), C.c_uint64(stride), C.c_int64(store_rows), _ptr(index), C.c_int64(m), nat.ENC_LAYOUTS[layout], *_norm_args(norm), _ptr(weight),
            C.c_uint64(int(weight.shape[1])), _ptr(bias), H, nat.LIN_ACTIVATIONS[activation], _dtype_code(dtype), _ptr(out), C.c_uint64(pitch))
    return _native_call("bg_linear_rows", rows.device, args, out[:, :H], timing, empty=m == 0)


def linear_rows_grad(rows: torch.Tensor, dout: torch.Tensor, *, out: Optional[torch.Tensor] = None, index: Optional[torch.Tensor] = None,
                     norm: Optional["RowNormalizer"] = None, layout: str = "fixed", activation: Optional[str] = None, dweight: Optional[torch.Tensor] = None,
                     bias: bool = True, workspace: Optional[torch.Tensor] = None, timing: bool = False):
    """The weight and bias gradient of `linear_rows`, straight from the records (bg_linear_rows_grad): dweight[n, k] = sum_i dp[i, n] * x[i, k],
    dbias[n] = sum_i dp[i, n], dp = bfloat16(dout), under activation="relu" masked where the forward's `out` (required then) is not > 0.  dout: float32 or
    bfloat16 [m, >= H].  dweight: optional float32 [H, 153] or [H, 628] (columns beyond 153 are not written); without one a zero-filled [H, 628] ("fixed")
    or [H, 153] ("produced") is made, so the columns beyond 153 carry their exact gradient, zero.  Returns (dweight, dbias or None) -- with timing=True
    (dweight, dbias, kernel milliseconds).  Sums over rows are deterministic (no atomics)."""
    stride, store_rows, m = _linear_common(rows, index, norm, layout, activation)
    H, dpitch, _, opitch = _grad_matrices(rows, dout, out, dweight, activation, m)
    if dweight is not None and (not isinstance(dweight, torch.Tensor) or dweight.dtype != torch.float32 or dweight.dim() != 2 or dweight.shape[1] < nat.LIN_K
                                or not dweight.is_contiguous() or dweight.device != rows.device):
        raise ValueError(f"dweight must be a contiguous torch.float32 tensor [H, >= {nat.LIN_K}] on {rows.device}")
    _check_device(rows)
    if dweight is None:
        dweight = torch.zeros((H, nat.ENC_COLS[nat.ENC_LAYOUTS[layout]]), dtype=torch.float32, device=rows.device)
    dbias = torch.zeros(H, dtype=torch.float32, device=rows.device) if bias else None
    head = (_ptr(rows), C.c_uint64(stride), C.c_int64(store_rows), _ptr(index), C.c_int64(m), nat.ENC_LAYOUTS[layout], *_norm_args(norm))
    return _grad_call("bg_linear_rows_grad", rows, head, m, nat.LIN_K, dout, dpitch, out, opitch, H, activation, dweight, dbias, workspace, timing)


class _RowLinearFn(torch.autograd.Function):
    """out = linear_rows(records); backward = ONE bg_linear_rows_grad call.  The records carry no gradient."""

    @staticmethod
    def forward(ctx, weight, bias, rows, index, norm, layout, activation, dtype, weight_bf16=None):
        out = linear_rows(rows, weight_bf16 if weight_bf16 is not None else weight.detach().to(torch.bfloat16), bias.detach() if bias is not None else None, index=index, norm=norm, layout=layout,
                          activation=activation, dtype=dtype)
        ctx.save_for_backward(out)
        ctx.call = (rows, index, norm, layout, activation, tuple(weight.shape), bias is not None)
        return out

    @staticmethod
    def backward(ctx, grad):
        rows, index, norm, layout, activation, wshape, has_bias = ctx.call
        out, = ctx.saved_tensors
        dweight = torch.zeros(wshape, dtype=torch.float32, device=rows.device)   # columns at or beyond 153: zero, their exact gradient
        dweight, dbias = linear_rows_grad(rows, _grad_as_dout(grad), out=out if activation == "relu" else None, index=index, norm=norm, layout=layout,
                                          activation=activation, dweight=dweight, bias=has_bias)
        return dweight, dbias, None, None, None, None, None, None, None


class RowLinear(_RowFirstLayer):
    """The first `nn.Linear` of a policy over packed records: `forward(rows)` is `linear_rows` and its backward one `linear_rows_grad` call, so neither pass
    materialises the feature matrix.  Parameters are float32 -- weight [out_features, 628] ("fixed": SB3's MultiInputPolicy over BalatroEnvFixed) or
    [out_features, 153] ("produced"), bias [out_features] -- initialised as nn.Linear; `from_linear` / `to_linear` move them to and from an nn.Linear, so a
    policy trained here loads into SB3's module and back.  The weight is cast to bfloat16 for every call (the master copy stays float32) unless
    `RowOptimizer.attach` keeps a bfloat16 copy current; columns at or
    beyond 153 of a 628-wide weight get a zero gradient, which is their exact gradient: their inputs are zero."""

    def __init__(self, out_features: int, in_layout: str = "fixed", activation: Optional[str] = None, dtype: torch.dtype = torch.bfloat16, device=None):
        if in_layout not in ("produced", "fixed"):
            raise ValueError(f"in_layout must be 'produced' or 'fixed' (got {in_layout!r})")
        super().__init__(nat.ENC_COLS[nat.ENC_LAYOUTS[in_layout]], out_features, activation, dtype, device)
        self.in_layout = in_layout

    @classmethod
    def from_linear(cls, linear: torch.nn.Linear, activation: Optional[str] = None, dtype: torch.dtype = torch.bfloat16) -> "RowLinear":
        if not isinstance(linear, torch.nn.Linear) or linear.in_features not in (nat.LIN_K, nat.ENC_COLS[nat.ENC_FIXED]) or linear.bias is None:
            raise ValueError("from_linear takes an nn.Linear with bias and 153 ('produced') or 628 ('fixed') inputs")
        return cls(linear.out_features, "produced" if linear.in_features == nat.LIN_K else "fixed", activation, dtype, device=linear.weight.device)._load(linear)

    def forward(self, rows: torch.Tensor, index: Optional[torch.Tensor] = None, norm: Optional["RowNormalizer"] = None) -> torch.Tensor:
        _linear_common(rows, index, norm, self.in_layout, self.activation)
        self._check_same_gpu(rows)
        return _RowLinearFn.apply(self.weight, self.bias, rows, index, norm, self.in_layout, self.activation, self.dtype, _live_shadow(self))

    def extra_repr(self) -> str:
        return f"in_layout={self.in_layout!r}, out_features={self.out_features}, activation={self.activation!r}, dtype={self.dtype}"


def _extractor_weight(weight) -> tuple:
    """-> (H, row pitch in elements).  A [H, 447] view of a wider matrix (e.g. of a 16-byte aligned [H, 448] one, which the kernel stages fastest) passes."""
    if not isinstance(weight, torch.Tensor) or weight.dtype != torch.bfloat16 or weight.dim() != 2 or weight.shape[1] != nat.EXT_K or weight.stride(1) != 1 \
            or (weight.shape[0] > 1 and weight.stride(0) < nat.EXT_K):
        raise ValueError(f"weight must be a torch.bfloat16 tensor [H, {nat.EXT_K}] with a contiguous last dimension (nn.Linear.weight's orientation)")
    H = int(weight.shape[0])
    _check_width(H)
    return H, int(weight.stride(0))


def extractor_rows(rows: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, index: Optional[torch.Tensor] = None,
                   activation: Optional[str] = None, dtype: torch.dtype = torch.bfloat16, out: Optional[torch.Tensor] = None, timing: bool = False):
    """The first layer behind BalatroFeaturesExtractor's input (train_balatro_agent.py:84-119) straight from packed records, on the matrix cores, in
    one launch (bg_extractor_rows): act(x @ weight.T + bias), x the bfloat16 rows `encode_rows(rows, "extractor", torch.bfloat16, index=index)` gives --
    416 one-hot hand columns, 10 joker ids, 21 scaled state features -- which are never written.  weight: torch.bfloat16 [H, 447] (nn.Linear.weight's
    orientation; rows may be a view with a wider pitch), H a multiple of 32 in [32, 4096]; bias: float32 [H] or None; activation: None or "relu".
    index: as `encode_rows`; a row whose index is out of range is act(bias).  There is no norm=: VecNormalize wraps the env's keys, not these tensors.
    dtype: torch.bfloat16 or torch.float32 (float32 accumulation either way, one rounding).  out: optional [m, >= H] tensor of `dtype`; columns beyond H
    are left untouched.  Returns the [m, H] matrix; timing=True returns (matrix, kernel milliseconds).  There is no CPU path.
    The reference's constructor declares `joker_dim = 160` and `game_state_dim = 32`, but its `forward` builds 10 and 21 columns, so that class raises a
    shape error on its first batch as written.  The "extractor" layout, and therefore this layer, follow `forward`: 416 + 10 + 21 = 447."""
    stride, store_rows, m = _first_layer_common(rows, index, activation)
    H, wpitch = _extractor_weight(weight)
    out, pitch = _forward_out(rows, weight, bias, H, dtype, out, m)
    args = (_ptr(rows), C.c_uint64(stride), C.c_int64(store_rows), _ptr(index), C.c_int64(m), _ptr(weight), C.c_uint64(wpitch), _ptr(bias), H,
            nat.LIN_ACTIVATIONS[activation], _dtype_code(dtype), _ptr(out), C.c_uint64(pitch))
    return _native_call("bg_extractor_rows", rows.device, args, out[:, :H], timing, empty=m == 0)


def extractor_rows_grad(rows: torch.Tensor, dout: torch.Tensor, *, out: Optional[torch.Tensor] = None, index: Optional[torch.Tensor] = None,
                        activation: Optional[str] = None, dweight: Optional[torch.Tensor] = None, dbias: Optional[torch.Tensor] = None, timing: bool = False):
    """The weight and bias gradient of `extractor_rows`, straight from the records (bg_extractor_rows_grad): dweight[n, k] = sum_i dp[i, n] * x[i, k],
    dbias[n] = sum_i dp[i, n], dp = bfloat16(dout), under activation="relu" masked where the forward's `out` (required then) is not > 0.  dout: float32 or
    bfloat16 [m, >= H].  dweight: optional float32 [H, >= 447] with a contiguous last dimension (columns at or beyond 447 are not written); dbias: optional
    contiguous float32 [H]; without them new tensors are made.  Returns (dweight, dbias) -- with timing=True (dweight, dbias, kernel milliseconds).
    Sums over rows are deterministic (no atomics)."""
    stride, store_rows, m = _first_layer_common(rows, index, activation)
    H, dpitch, _, opitch = _grad_matrices(rows, dout, out, dweight, activation, m)
    if dweight is not None and (not isinstance(dweight, torch.Tensor) or dweight.dtype != torch.float32 or dweight.dim() != 2 or dweight.shape[1] < nat.EXT_K
                                or dweight.stride(1) != 1 or dweight.stride(0) < dweight.shape[1] or dweight.device != rows.device):
        raise ValueError(f"dweight must be a torch.float32 tensor [H, >= {nat.EXT_K}] on {rows.device} with a contiguous last dimension")
    if dbias is not None:
        _check_vector("dbias", dbias, H, rows.device)
    _check_device(rows)
    if dweight is None:
        dweight = torch.zeros((H, nat.EXT_K), dtype=torch.float32, device=rows.device)
    if dbias is None:
        dbias = torch.zeros(H, dtype=torch.float32, device=rows.device)
    head = (_ptr(rows), C.c_uint64(stride), C.c_int64(store_rows), _ptr(index), C.c_int64(m))
    return _grad_call("bg_extractor_rows_grad", rows, head, m, nat.EXT_K, dout, dpitch, out, opitch, H, activation, dweight, dbias, None, timing)


class _RowExtractorFn(torch.autograd.Function):
    """out = extractor_rows(records); backward = ONE bg_extractor_rows_grad call.  The records carry no gradient."""

    @staticmethod
    def forward(ctx, weight, bias, rows, index, activation, dtype, mask, weight_bf16=None):
        wb = weight_bf16
        if wb is None:
            wb = torch.empty((weight.shape[0], nat.EXT_K + 1), dtype=torch.bfloat16, device=weight.device)[:, :nat.EXT_K]   # pitch 448: 16-byte lines
            wb.copy_(weight.detach())
        out = extractor_rows(rows, wb, bias.detach(), index=index, activation=activation, dtype=dtype)
        ctx.save_for_backward(out)
        ctx.call = (rows, index, activation, mask)
        return out

    @staticmethod
    def backward(ctx, grad):
        rows, index, activation, mask = ctx.call
        out, = ctx.saved_tensors
        dweight, dbias = extractor_rows_grad(rows, _grad_as_dout(grad), out=out if activation == "relu" else None, index=index, activation=activation)
        if mask is not None:
            dweight.mul_(mask)
        return dweight, dbias, None, None, None, None, None, None


class RowExtractor(_RowFirstLayer):
    """The first layer of a network over BalatroFeaturesExtractor's input (train_balatro_agent.py:84-119), from packed records: `forward(rows)` is
    `extractor_rows` and its backward one `extractor_rows_grad` call, so neither pass materialises the [m, 447] matrix.  Parameters are float32 --
    weight [out_features, 447], bias [out_features] -- initialised as nn.Linear(447, out_features); `from_linear` / `to_linear` move them to and from an
    nn.Linear.  The weight is cast to bfloat16 for every call (the master copy stays float32) unless `RowOptimizer.attach` keeps a pitch-448 copy current.
    `from_linears(hand, joker, state)` stacks the first layers of the reference's `hand_net`, `joker_net` and `game_state_net` (416, 10 and 21 inputs)
    as ONE block-structured [h + j + s, 447] weight: `.splits == (h, j, s)`, so `out.split(layer.splits, dim=1)` gives the three sub-networks'
    activations; the block mask is a buffer and multiplies dweight in backward, so off-block weights stay exactly zero under any optimiser;
    `to_linears()` returns the three layers.
    The reference's constructor declares `joker_dim = 160` and `game_state_dim = 32`, but its `forward` builds 10 and 21 columns, so that class raises a
    shape error on its first batch as written.  The "extractor" layout, and therefore this layer, follow `forward`: 416 + 10 + 21 = 447."""

    def __init__(self, out_features: int, activation: Optional[str] = "relu", dtype: torch.dtype = torch.bfloat16, device=None):
        super().__init__(nat.EXT_K, out_features, activation, dtype, device)
        self.splits = (self.out_features,)
        self.register_buffer("block_mask", None)

    @classmethod
    def from_linear(cls, linear: torch.nn.Linear, activation: Optional[str] = "relu", dtype: torch.dtype = torch.bfloat16) -> "RowExtractor":
        if not isinstance(linear, torch.nn.Linear) or linear.in_features != nat.EXT_K or linear.bias is None:
            raise ValueError(f"from_linear takes an nn.Linear with bias and {nat.EXT_K} inputs")
        return cls(linear.out_features, activation, dtype, device=linear.weight.device)._load(linear)

    @classmethod
    def from_linears(cls, hand: torch.nn.Linear, joker: torch.nn.Linear, state: torch.nn.Linear, activation: Optional[str] = "relu",
                     dtype: torch.dtype = torch.bfloat16) -> "RowExtractor":
        parts = (hand, joker, state)
        for lin, cols, name in zip(parts, nat.EXT_SPLITS, ("hand", "joker", "state")):
            if not isinstance(lin, torch.nn.Linear) or lin.in_features != cols or lin.bias is None:
                raise ValueError(f"from_linears: {name} must be an nn.Linear with bias and in_features {cols} (the reference's forward builds 416, 10 and 21 columns)")
        splits = tuple(int(lin.out_features) for lin in parts)
        if sum(splits) % 32:
            raise ValueError(f"from_linears: the out_features {splits} must sum to a multiple of 32 (got {sum(splits)})")
        layer = cls(sum(splits), activation, dtype, device=hand.weight.device)
        layer.splits = splits
        mask = torch.zeros_like(layer.weight)
        with torch.no_grad():
            layer.weight.zero_()
            r = c = 0
            for lin, cols in zip(parts, nat.EXT_SPLITS):
                layer.weight[r:r + lin.out_features, c:c + cols] = lin.weight
                layer.bias[r:r + lin.out_features] = lin.bias
                mask[r:r + lin.out_features, c:c + cols] = 1.0
                r, c = r + lin.out_features, c + cols
        layer.block_mask = mask
        return layer

    def to_linears(self) -> tuple:
        if len(self.splits) != 3:
            raise ValueError("to_linears needs a layer made by from_linears")
        out, r, c = [], 0, 0
        for width, cols in zip(self.splits, nat.EXT_SPLITS):
            lin = torch.nn.Linear(cols, width, device=self.weight.device)
            with torch.no_grad():
                lin.weight.copy_(self.weight[r:r + width, c:c + cols])
                lin.bias.copy_(self.bias[r:r + width])
            out.append(lin)
            r, c = r + width, c + cols
        return tuple(out)

    def forward(self, rows: torch.Tensor, index: Optional[torch.Tensor] = None) -> torch.Tensor:
        _first_layer_common(rows, index, self.activation)
        self._check_same_gpu(rows)
        return _RowExtractorFn.apply(self.weight, self.bias, rows, index, self.activation, self.dtype, self.block_mask, _live_shadow(self))

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}, splits={self.splits}, activation={self.activation!r}, dtype={self.dtype}"


def _head_logits(logits) -> tuple:
    """logits of sample_actions / evaluate_actions: float32 / bfloat16 [..., 60] with a contiguous last dimension and leading dimensions dense over the
    row pitch (e.g. 60 columns of a wider matrix) -> (leading shape, m, row pitch in elements)."""
    if not isinstance(logits, torch.Tensor) or logits.dtype not in (torch.float32, torch.bfloat16) or logits.dim() < 1 or logits.shape[-1] != 60:
        raise ValueError("logits must be a float32 or bfloat16 tensor [..., 60]")
    dense, pitch = _row_pitch(logits, 60, False)
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
        dense, stride = _row_pitch(mask, 60, False)
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


def _check_mask_aligned(mask, moff: int) -> None:
    if mask is not None and (mask.data_ptr() + moff) % 4:
        raise ValueError("mask must be 4-byte aligned")


def _head_args(logits, pitch: int, mask, moff: int, mstride: int) -> tuple:
    """(logits_dev, logits_dtype, logits_stride_elems, mask_dev, mask_stride_bytes): how the head calls and the PPO loss begin."""
    return (_ptr(logits), nat.HEAD_F32 if logits.dtype == torch.float32 else nat.HEAD_BF16, C.c_uint64(pitch),
            mask.data_ptr() + moff if mask is not None else None, C.c_uint64(mstride))


def _head_outputs(lead: tuple, dev: torch.device, given, actions, log_prob, entropy):
    """The outputs of a head-ended call, in two steps around the caller's last refusals.  Now: `given` (the actions to evaluate) and whichever of
    actions / log_prob / entropy were passed are contiguous tensors of shape `lead` on `dev`.  The function returned, called behind the last refusal,
    allocates what was not passed -> res: (log_prob, entropy) with `given`, else (actions, log_prob, entropy)."""
    if given is not None:
        _check_scan_tensor("actions", given, torch.int32, lead, dev)
    if actions is not None or log_prob is not None or entropy is not None:   # (seldom: most callers let the call allocate)
        for what, tt, dt in (("actions", actions, torch.int32), ("log_prob", log_prob, torch.float32), ("entropy", entropy, torch.float32)):
            if tt is not None:
                _check_scan_tensor(what, tt, dt, lead, dev)

    def allocate() -> tuple:
        lp = log_prob if log_prob is not None else torch.empty(lead, dtype=torch.float32, device=dev)
        ent = entropy if entropy is not None else torch.empty(lead, dtype=torch.float32, device=dev)
        if given is not None:
            return lp, ent
        return actions if actions is not None else torch.empty(lead, dtype=torch.int32, device=dev), lp, ent
    return allocate


def _check_no_alias(ins, outs) -> None:
    """No output starts where an input or another output does (None: not passed).  For non-empty tensors: an empty one has no pointer."""
    outs = [x.data_ptr() for x in outs if x is not None]
    if len(set(outs)) != len(outs) or set(outs) & {x.data_ptr() for x in ins if x is not None}:
        raise ValueError("outputs must not share memory with the inputs or with each other")


def _head_call(name: str, logits, mask, given, flags: int, seed: int, index0: int, t: int, actions, log_prob, entropy, timing: bool,
               epsilon: Optional[float] = None):
    lead, m, pitch = _head_logits(logits)
    dev = logits.device
    mask, moff, mstride = _head_mask(mask, lead, dev)
    if epsilon is not None:
        return _head_call_eps(logits, lead, m, pitch, mask, moff, mstride, flags, seed, index0, t, actions, log_prob, entropy, timing, epsilon)
    _check_counters(seed, index0, t)
    allocate = _head_outputs(lead, dev, given, actions, log_prob, entropy)
    _check_device(logits, "logits", align=0)
    _check_mask_aligned(mask, moff)
    res = allocate()
    if m == 0:   # nothing to launch (an empty tensor has no pointer to hand over)
        return _native_call(name, dev, (), res, timing, empty=True)
    _check_no_alias((logits, mask, given), res)
    head = (*_head_args(logits, pitch, mask, moff, mstride), C.c_int64(m))
    front = (_ptr(given),) if given is not None else (C.c_uint32(flags), C.c_uint64(int(seed)), C.c_uint64(int(index0)), C.c_uint64(int(t)))
    return _native_call(name, dev, (*head, *front, *map(_ptr, res)), res, timing)


def _head_call_eps(logits, lead, m, pitch, mask, moff, mstride, flags, seed, index0, t, actions, log_prob, entropy, timing, epsilon):
    """bg_sample_actions_eps: what is the epsilon-greedy form's own -- epsilon, no deterministic, ONE output (so it checks and compares that one itself) --
    around the counters of `_head_call` -> (actions, None, None)."""
    dev = logits.device
    if isinstance(epsilon, bool) or not isinstance(epsilon, (int, float, np.integer, np.floating)) or not 0.0 <= float(epsilon) <= 1.0:
        raise ValueError("epsilon must be a number in [0, 1] (or None: the categorical head)")
    if flags:
        raise ValueError("epsilon and deterministic=True exclude each other (epsilon=0.0 is the greedy rule)")
    if log_prob is not None or entropy is not None:
        raise ValueError("an epsilon-greedy action has no categorical log_prob / entropy: pass neither with epsilon")
    _check_counters(seed, index0, t)
    if actions is not None:
        _check_scan_tensor("actions", actions, torch.int32, lead, dev)
    _check_device(logits, "logits", align=0)
    _check_mask_aligned(mask, moff)
    if actions is None:
        actions = torch.empty(lead, dtype=torch.int32, device=dev)
    res = (actions, None, None)
    if m == 0:
        return _native_call("bg_sample_actions_eps", dev, (), res, timing, empty=True)
    if actions.data_ptr() == logits.data_ptr() or (mask is not None and actions.data_ptr() == mask.data_ptr()):
        raise ValueError("outputs must not share memory with the inputs or with each other")
    args = (*_head_args(logits, pitch, mask, moff, mstride), C.c_int64(m), C.c_uint32(0), C.c_uint64(int(seed)), C.c_uint64(int(index0)), C.c_uint64(int(t)),
            C.c_float(float(epsilon)), _ptr(actions), None, None)
    return _native_call("bg_sample_actions_eps", dev, args, res, timing)


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
_dqn_workspaces: dict = {}


def _loss_workspace(cache: dict, size_fn: str, dev: torch.device, m: int, *more) -> torch.Tensor:
    """The workspace of a loss call over m rows, kept per (device, size) in `cache`; m == 0 needs none and loads nothing.  more: what the size
    function takes behind m."""
    if m == 0:
        return torch.empty(0, dtype=torch.uint8, device=dev)
    need = int(getattr(nat.load(), size_fn)(C.c_int64(m), *more))
    key = (dev, need)
    if key not in cache:
        cache[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    return cache[key]


def _stored_rows(lead: tuple, index, actions, mask, dev: torch.device) -> tuple:
    """How ppo_loss, actor_ppo_loss and bc_loss begin: the shape of the STORED arrays -- that of `actions` with an index, else the minibatch's -- and
    the mask over it -> (store, store_rows, mask, moff, mstride)."""
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
    return (store, store_rows, *_head_mask(mask, store, dev))


def _check_coef(name: str, value) -> None:
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not np.isfinite(value):
        raise ValueError(f"{name} must be a finite number")


def _ppo_inputs(lead: tuple, store: tuple, dev: torch.device, actions, old_log_prob, advantages, values, returns, clip_range, ent_coef, vf_coef) -> None:
    """The refusals ppo_loss and actor_ppo_loss share behind `_stored_rows`: the five tensors, then the coefficients."""
    _check_scan_tensor("actions", actions, torch.int32, store, dev)
    _check_scan_tensor("old_log_prob", old_log_prob, torch.float32, store, dev)
    _check_scan_tensor("advantages", advantages, torch.float32, store, dev)
    if (values is None) != (returns is None):
        raise ValueError("values and returns go together: both or neither")
    if values is not None:
        _check_scan_tensor("values", values, torch.float32, lead, dev)
        _check_scan_tensor("returns", returns, torch.float32, store, dev)
    for what, v in (("clip_range", clip_range), ("ent_coef", ent_coef), ("vf_coef", vf_coef)):
        _check_coef(what, v)
    if not 0.0 < float(np.float32(clip_range)) < 1.0:
        raise ValueError("clip_range must be in (0, 1)")


def _ppo_outputs(lead: tuple, values, dev: torch.device) -> tuple:
    """(raw, dvalues, log_prob, entropy) of the two PPO calls: allocated behind their last refusal, so not part of `_ppo_inputs`."""
    return (torch.zeros(len(nat.PPO_STATS), dtype=torch.float32, device=dev), torch.empty(lead, dtype=torch.float32, device=dev) if values is not None else None,
            torch.empty(lead, dtype=torch.float32, device=dev), torch.empty(lead, dtype=torch.float32, device=dev))


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
    store, store_rows, mask, moff, mstride = _stored_rows(lead, index, actions, mask, dev)
    _ppo_inputs(lead, store, dev, actions, old_log_prob, advantages, values, returns, clip_range, ent_coef, vf_coef)
    _check_device(logits, "logits", align=0)
    _check_mask_aligned(mask, moff)
    lg = logits.detach()
    vals = values.detach() if values is not None else None
    raw, dvalues, log_prob, entropy = _ppo_outputs(lead, values, dev)
    dlogits = torch.empty(lead + (60,), dtype=logits.dtype, device=dev)
    ws = _loss_workspace(_ppo_workspaces, "bg_ppo_loss_workspace_bytes", dev, m)
    args = (*_head_args(lg, pitch, mask, moff, mstride), _ptr(actions), _ptr(old_log_prob), _ptr(advantages), _ptr(vals), _ptr(returns), _ptr(index),
            C.c_int64(store_rows), C.c_int64(m), C.c_float(clip_range), C.c_float(ent_coef), C.c_float(vf_coef), C.c_uint32(nat.PPO_NORMALIZE_ADV if normalize_advantage else 0), _ptr(dlogits),
            C.c_uint64(60), _ptr(dvalues), _ptr(log_prob), _ptr(entropy), _ptr(raw), _ptr(ws), C.c_uint64(ws.numel()))
    kernel_ms = _native_call("bg_ppo_loss", dev, args, (), timing, empty=m == 0)   # () or (ms,)
    stats = PpoStats(raw, log_prob, entropy, dlogits, dvalues, *kernel_ms)
    loss = raw[0]
    if torch.is_grad_enabled() and (logits.requires_grad or (values is not None and values.requires_grad)):
        loss = _PpoLossGrad.apply(loss, dlogits, dvalues, logits, values)
    return loss, stats


# ---------------------------------------------------------------------- the last layer fused with the head and with PPO's loss (bg_actor.h)
def _check_h(h, not_h: str, widths, bad_width: str) -> tuple:
    """h of the actor calls and of `RowPolicy`: bfloat16 [..., width], width in `widths`, with a contiguous last dimension and leading dimensions
    dense over a row pitch that is a multiple of 8 -> (leading shape, m, width, row pitch).  The caller's own literals: `not_h` refuses what is no
    such tensor, `bad_width` a width outside `widths` (its "%d" is the width h has)."""
    if not isinstance(h, torch.Tensor) or h.dtype != torch.bfloat16 or h.dim() < 1:
        raise ValueError(not_h)
    width = int(h.shape[-1])
    if width not in widths:
        raise ValueError(bad_width % width)
    dense, pitch = _row_pitch(h, width, True)
    if not dense or pitch % 8:
        raise ValueError("h must have a contiguous last dimension and leading dimensions dense over a row pitch that is a multiple of 8 elements")
    lead = tuple(h.shape[:-1])
    return lead, int(np.prod(lead, dtype=np.int64)), width, pitch


_ACTOR_HINS = range(nat.ACTOR_HIN_MIN, nat.ACTOR_HIN_MAX + 1, 32)
_ACTOR_BAD_HIN = f"Hin, the last dimension of h, must be a multiple of 32 in [{nat.ACTOR_HIN_MIN}, {nat.ACTOR_HIN_MAX}] (got %d)"


def _actor_layer(h, weight, bias) -> tuple:
    """(h, weight, bias) of the actor calls -> (leading shape, m, h's row pitch, Hin, weight's row pitch).  h: `_check_h`; weight: float32 / bfloat16
    [60, Hin] (nn.Linear.weight's orientation) with a contiguous last dimension; bias: contiguous float32 [60] or None."""
    lead, m, Hin, pitch = _check_h(h, "h must be a torch.bfloat16 tensor [..., Hin] (the last hidden activation)", _ACTOR_HINS, _ACTOR_BAD_HIN)
    if not isinstance(weight, torch.Tensor) or weight.dtype not in (torch.float32, torch.bfloat16) or tuple(weight.shape) != (60, Hin) or weight.stride(1) != 1 \
            or weight.stride(0) < Hin:
        raise ValueError(f"weight must be a float32 / bfloat16 tensor [60, {Hin}] (nn.Linear.weight's orientation) with a contiguous last dimension")
    if weight.device != h.device:
        raise ValueError(f"weight must be on {h.device}")
    if bias is not None:
        _check_vector("bias", bias, 60, h.device)
    return lead, m, pitch, Hin, int(weight.stride(0))


def _actor_tile_out(name: str, t, lead: tuple, device: torch.device) -> int:
    """logits_out / dlogits_out: None, or a float32 tensor [..., >= 60] over the leading shape, rows dense over its pitch -> the pitch (60 for None)."""
    if t is None:
        return 60
    ok = isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == device and tuple(t.shape[:-1]) == lead and t.dim() >= 1 and t.shape[-1] >= 60
    ok, pitch = _row_pitch(t, int(t.shape[-1]), True) if ok else (False, 0)
    if not ok:
        raise ValueError(f"{name} must be a torch.float32 tensor {list(lead)} + [>= 60] on {device} with a contiguous last dimension and dense rows")
    return pitch


def _actor_head(h, hpitch: int, Hin: int, weight, wpitch: int, bias, mask, moff: int, mstride: int) -> tuple:
    """How the three actor calls begin: h, its pitch, Hin, weight, its dtype, its pitch, bias, mask, its pitch."""
    return (_ptr(h), C.c_uint64(hpitch), Hin, _ptr(weight), _dtype_code(weight.dtype), C.c_uint64(wpitch), _ptr(bias),
            mask.data_ptr() + moff if mask is not None else None, C.c_uint64(mstride))


def _actor_head_call(name: str, h, weight, bias, mask, given, flags: int, seed: int, index0: int, t: int, actions, log_prob, entropy, logits_out, timing: bool):
    lead, m, hpitch, Hin, wpitch = _actor_layer(h, weight, bias)
    dev = h.device
    mask, moff, mstride = _head_mask(mask, lead, dev)
    _check_counters(seed, index0, t)
    allocate = _head_outputs(lead, dev, given, actions, log_prob, entropy)
    lopitch = _actor_tile_out("logits_out", logits_out, lead, dev)
    _check_device(h, "h")
    _check_mask_aligned(mask, moff)
    res = allocate()
    if m == 0:
        return _native_call(name, dev, (), res, timing, empty=True)
    _check_no_alias((h, weight, bias, mask, given), (*res, logits_out))
    head = (*_actor_head(h, hpitch, Hin, weight, wpitch, bias, mask, moff, mstride), C.c_int64(m))
    front = (_ptr(given),) if given is not None else (C.c_uint32(flags), C.c_uint64(int(seed)), C.c_uint64(int(index0)), C.c_uint64(int(t)))
    return _native_call(name, dev, (*head, *front, *map(_ptr, res), _ptr(logits_out), C.c_uint64(lopitch)), res, timing)


def actor_sample(h: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, *, seed: int, t: int,
                 index0: int = 0, deterministic: bool = False, actions: Optional[torch.Tensor] = None, log_prob: Optional[torch.Tensor] = None,
                 entropy: Optional[torch.Tensor] = None, logits_out: Optional[torch.Tensor] = None, timing: bool = False):
    """The policy's last layer and the masked head in one launch (bg_actor_sample): h bfloat16 [..., Hin] (the last hidden activation; Hin a multiple
    of 32 in [32, 1024]), weight float32 / bfloat16 [60, Hin] and bias float32 [60] (SB3's `action_net`) -> (actions int32, log_prob, entropy), each
    [...].  The logits -- h @ bfloat16(weight).T accumulated in float32 on the matrix cores, + bias -- stay on the CU; `logits_out` (float32
    [..., >= 60]) receives them when given.  mask, seed, t, index0, deterministic, actions / log_prob / entropy: as `sample_actions`, and the results are
    bit for bit `sample_actions(logits_out, ...)`'s."""
    return _actor_head_call("bg_actor_sample", h, weight, bias, mask, None, nat.HEAD_DETERMINISTIC if deterministic else 0, seed, index0, t, actions, log_prob,
                            entropy, logits_out, timing)


def actor_evaluate(h: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], actions: torch.Tensor, mask: Optional[torch.Tensor] = None, *,
                   log_prob: Optional[torch.Tensor] = None, entropy: Optional[torch.Tensor] = None, logits_out: Optional[torch.Tensor] = None, timing: bool = False):
    """(log_prob, entropy) of given int32 actions [...] under the distribution `actor_sample` draws from (bg_actor_evaluate): bit for bit
    `evaluate_actions(logits_out, actions, mask)`.  A forward pass; `actor_ppo_loss` is the call that takes part in autograd."""
    if not isinstance(actions, torch.Tensor):
        raise ValueError("actions must be an int32 tensor with the leading shape of h")
    return _actor_head_call("bg_actor_evaluate", h, weight, bias, mask, actions, 0, 0, 0, 0, None, log_prob, entropy, logits_out, timing)


class ActorPpoStats(PpoStats):
    """`PpoStats` of `actor_ppo_loss`: the scalars, `log_prob`, `entropy` and `dvalues` as `ppo_loss` gives them, and in place of the logits' gradient
    the layer's -- `dh` [..., Hin], `dweight` float32 [60, Hin], `dbias` float32 [60].  `dlogits` is the float32 tile the caller asked for
    (dlogits_out=) or None."""

    def __init__(self, raw, log_prob, entropy, dlogits, dvalues, dh, dweight, dbias, kernel_ms=None):
        super().__init__(raw, log_prob, entropy, dlogits, dvalues, kernel_ms)
        self.dh, self.dweight, self.dbias = dh, dweight, dbias

    def __repr__(self):
        return "ActorPpoStats(" + ", ".join(nat.PPO_STATS) + ", log_prob, entropy, dh, dweight, dbias, dvalues)"


class _ActorPpoLossGrad(torch.autograd.Function):
    """The node `actor_ppo_loss` hangs on its loss (`_PpoLossGrad`'s pattern): the forward pass produced every gradient, the backward multiplies the
    stored ones by the incoming scalar."""

    @staticmethod
    def forward(ctx, loss, dh, dweight, dbias, dvalues, h, weight, bias, values):
        ctx.save_for_backward(dh, dweight, dbias, dvalues if dvalues is not None else dbias.new_empty(0))
        ctx.has_bias, ctx.has_values = bias is not None, dvalues is not None
        ctx.h_dtype, ctx.w_dtype = h.dtype, weight.dtype
        return loss.clone()

    @staticmethod
    def backward(ctx, grad):
        dh, dweight, dbias, dvalues = ctx.saved_tensors
        gh = (dh * grad).to(ctx.h_dtype) if ctx.needs_input_grad[5] else None
        gw = (dweight * grad).to(ctx.w_dtype) if ctx.needs_input_grad[6] else None
        gb = dbias * grad if ctx.has_bias and ctx.needs_input_grad[7] else None
        gv = dvalues * grad if ctx.has_values and ctx.needs_input_grad[8] else None
        return None, None, None, None, None, gh, gw, gb, gv


_actor_workspaces: dict = {}


def actor_rows_per_group(m: int, Hin: int) -> int:
    """The consecutive rows whose dweight / dbias terms `actor_ppo_loss` sums in float32 before the float64 sum over the groups
    (bg_actor_ppo_loss_rows_per_group): what bounds the rounding of those two outputs."""
    return int(nat.load().bg_actor_ppo_loss_rows_per_group(C.c_int64(m), Hin))


def actor_ppo_loss(h: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], actions: torch.Tensor, old_log_prob: torch.Tensor,
                   advantages: torch.Tensor, mask: Optional[torch.Tensor] = None, *, values: Optional[torch.Tensor] = None,
                   returns: Optional[torch.Tensor] = None, index: Optional[torch.Tensor] = None, clip_range: float = 0.2, ent_coef: float = 0.0,
                   vf_coef: float = 0.5, normalize_advantage: bool = True, dh_dtype: torch.dtype = torch.bfloat16, logits_out: Optional[torch.Tensor] = None,
                   dlogits_out: Optional[torch.Tensor] = None, timing: bool = False, weight_bf16: Optional[torch.Tensor] = None):
    """`ppo_loss` with the policy's last layer inside the launch (bg_actor_ppo_loss): h bfloat16 [..., Hin], weight float32 / bfloat16 [60, Hin] and
    bias float32 [60] or None in place of the logits -> (loss, `ActorPpoStats`).  Every other argument, the excluded rows and the statistics are
    `ppo_loss`'s, bit for bit on the logits this call computes (`logits_out`, float32 [..., >= 60], receives them; `dlogits_out` their float32 gradient).
    In place of dlogits the call writes stats.dh [..., Hin] (`dh_dtype`: float32, or bfloat16 = its nearest-even rounding), stats.dweight float32
    [60, Hin] and stats.dbias float32 [60], from dp = bfloat16(dlogits): dh = dp @ w, dweight = dp.T @ h, dbias = dp.sum(0).  When h, weight, bias or
    values require grad the loss carries one autograd node whose backward multiplies the stored gradients by the incoming scalar: `loss.backward()`
    fills weight.grad, bias.grad and h.grad (and so drives the network below) with nothing recomputed.  weight_bf16: a bfloat16 [60, Hin] copy of a float32
    `weight` that the launch reads in its place (`RowOptimizer.attach` keeps one); the gradient still belongs to `weight`."""
    lead, m, hpitch, Hin, wpitch = _actor_layer(h, weight, bias)
    if weight_bf16 is not None:
        if weight.dtype != torch.float32 or not isinstance(weight_bf16, torch.Tensor) or weight_bf16.dtype != torch.bfloat16:
            raise ValueError("weight_bf16 must be a torch.bfloat16 copy of a float32 weight")
        wpitch = _actor_layer(h, weight_bf16, bias)[4]
    dev = h.device
    store, store_rows, mask, moff, mstride = _stored_rows(lead, index, actions, mask, dev)
    _ppo_inputs(lead, store, dev, actions, old_log_prob, advantages, values, returns, clip_range, ent_coef, vf_coef)
    if dh_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("dh_dtype must be torch.float32 or torch.bfloat16")
    lopitch = _actor_tile_out("logits_out", logits_out, lead, dev)
    dlopitch = _actor_tile_out("dlogits_out", dlogits_out, lead, dev)
    _check_device(h, "h")
    _check_mask_aligned(mask, moff)
    if logits_out is not None and dlogits_out is not None and logits_out.data_ptr() == dlogits_out.data_ptr() and m:
        raise ValueError("logits_out and dlogits_out must not share memory")
    hd, wd = h.detach(), weight.detach() if weight_bf16 is None else weight_bf16
    bd = bias.detach() if bias is not None else None
    vals = values.detach() if values is not None else None
    raw, dvalues, log_prob, entropy = _ppo_outputs(lead, values, dev)
    dh = torch.empty(lead + (Hin,), dtype=dh_dtype, device=dev)
    dweight = torch.zeros((60, Hin), dtype=torch.float32, device=dev)
    dbias = torch.zeros(60, dtype=torch.float32, device=dev)
    ws = _loss_workspace(_actor_workspaces, "bg_actor_ppo_loss_workspace_bytes", dev, m, Hin)
    args = (*_actor_head(hd, hpitch, Hin, wd, wpitch, bd, mask, moff, mstride), _ptr(actions), _ptr(old_log_prob), _ptr(advantages), _ptr(vals), _ptr(returns),
            _ptr(index), C.c_int64(store_rows), C.c_int64(m), C.c_float(clip_range), C.c_float(ent_coef), C.c_float(vf_coef),
            C.c_uint32(nat.PPO_NORMALIZE_ADV if normalize_advantage else 0), _ptr(dh), _dtype_code(dh_dtype), C.c_uint64(Hin), _ptr(dweight), _ptr(dbias),
            _ptr(dvalues), _ptr(log_prob), _ptr(entropy), _ptr(raw), _ptr(logits_out), C.c_uint64(lopitch), _ptr(dlogits_out), C.c_uint64(dlopitch), _ptr(ws),
            C.c_uint64(ws.numel()))
    kernel_ms = _native_call("bg_actor_ppo_loss", dev, args, (), timing, empty=m == 0)   # () or (ms,)
    stats = ActorPpoStats(raw, log_prob, entropy, dlogits_out, dvalues, dh, dweight, dbias, *kernel_ms)
    loss = raw[0]
    if torch.is_grad_enabled() and (h.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad)
                                    or (values is not None and values.requires_grad)):
        loss = _ActorPpoLossGrad.apply(loss, dh, dweight, dbias, dvalues, h, weight, bias, values)
    return loss, stats


class RowActor(torch.nn.Module):
    """SB3's `action_net` -- nn.Linear(in_features, 60) -- as the layer the actor calls run: float32 parameters `weight` [60, in_features] and `bias`
    [60], initialised as nn.Linear, rounded to bfloat16 inside the launch (or read from the bfloat16 copy `RowOptimizer.attach` keeps).  in_features: a multiple of 32 in [32, 1024].  dtype: what the gradient of
    h is written in (bfloat16, or float32 rounded by autograd afterwards).  `from_linear` / `to_linear` carry SB3's parameters both ways."""

    def __init__(self, in_features: int, dtype: torch.dtype = torch.bfloat16, device=None):
        super().__init__()
        in_features = int(in_features)
        if in_features < nat.ACTOR_HIN_MIN or in_features > nat.ACTOR_HIN_MAX or in_features % 32:
            raise ValueError(f"in_features must be a multiple of 32 in [{nat.ACTOR_HIN_MIN}, {nat.ACTOR_HIN_MAX}] (got {in_features})")
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("dtype must be torch.float32 or torch.bfloat16")
        self.in_features, self.out_features, self.dtype = in_features, 60, dtype
        lin = torch.nn.Linear(in_features, 60, device=device)   # nn.Linear's own initialisation
        self.weight = torch.nn.Parameter(lin.weight.detach().clone())
        self.bias = torch.nn.Parameter(lin.bias.detach().clone())
        self.weight_bf16, self._weight_bf16_version = None, -1   # RowOptimizer.attach: a bfloat16 copy kept by the update pass (`_live_shadow`)

    @classmethod
    def from_linear(cls, linear: torch.nn.Linear, dtype: torch.dtype = torch.bfloat16) -> "RowActor":
        if not isinstance(linear, torch.nn.Linear) or linear.out_features != 60 or linear.bias is None:
            raise ValueError("from_linear takes an nn.Linear(in_features, 60) with a bias (SB3's action_net)")
        layer = cls(linear.in_features, dtype=dtype, device=linear.weight.device)
        with torch.no_grad():
            layer.weight.copy_(linear.weight)
            layer.bias.copy_(linear.bias)
        return layer

    def to_linear(self) -> torch.nn.Linear:
        lin = torch.nn.Linear(self.in_features, 60, device=self.weight.device)
        with torch.no_grad():
            lin.weight.copy_(self.weight)
            lin.bias.copy_(self.bias)
        return lin

    def _w(self) -> torch.Tensor:
        """What the forward-only calls read: the bfloat16 copy `RowOptimizer.attach` keeps while it is current, else the float32 weight (rounded in the launch)."""
        wb = _live_shadow(self)
        return wb if wb is not None else self.weight.detach()

    def act(self, h: torch.Tensor, mask: Optional[torch.Tensor] = None, *, seed: int, t: int, index0: int = 0, deterministic: bool = False,
            log_prob: Optional[torch.Tensor] = None, entropy: Optional[torch.Tensor] = None):
        """-> (actions, log_prob, entropy): `actor_sample` with this layer's parameters (no autograd: collection)."""
        return actor_sample(h.detach(), self._w(), self.bias.detach(), mask, seed=seed, t=t, index0=index0, deterministic=deterministic,
                            log_prob=log_prob, entropy=entropy)

    def evaluate(self, h: torch.Tensor, actions: torch.Tensor, mask: Optional[torch.Tensor] = None):
        """-> (log_prob, entropy): `actor_evaluate` with this layer's parameters (a forward pass)."""
        return actor_evaluate(h.detach(), self._w(), self.bias.detach(), actions, mask)

    def ppo_loss(self, h: torch.Tensor, actions: torch.Tensor, old_log_prob: torch.Tensor, advantages: torch.Tensor, mask: Optional[torch.Tensor] = None, *,
                 values: Optional[torch.Tensor] = None, returns: Optional[torch.Tensor] = None, index: Optional[torch.Tensor] = None, clip_range: float = 0.2,
                 ent_coef: float = 0.0, vf_coef: float = 0.5, normalize_advantage: bool = True):
        """-> (loss, `ActorPpoStats`): `actor_ppo_loss` with this layer's parameters; `loss.backward()` fills weight.grad, bias.grad and h.grad."""
        return actor_ppo_loss(h, self.weight, self.bias, actions, old_log_prob, advantages, mask, values=values, returns=returns, index=index,
                              clip_range=clip_range, ent_coef=ent_coef, vf_coef=vf_coef, normalize_advantage=normalize_advantage, dh_dtype=self.dtype,
                              weight_bf16=_live_shadow(self))

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features=60, dtype={self.dtype}"


class BcStats:
    """What `bc_loss` returns beside the loss: the scalars of `_native.BC_STATS` as 0-dim float32 device tensors (views of `raw`, no host
    synchronisation), `log_prob` / `entropy` [...] of the minibatch rows (bit for bit `evaluate_actions`'), and the gradient the call produced --
    `dlogits` [..., 60] in the dtype of the logits.  `kernel_ms` with timing=True."""

    def __init__(self, raw, log_prob, entropy, dlogits, kernel_ms=None):
        self.raw, self.log_prob, self.entropy, self.dlogits, self.kernel_ms = raw, log_prob, entropy, dlogits, kernel_ms
        for k, name in enumerate(nat.BC_STATS):
            setattr(self, name, raw[k])

    def __repr__(self):
        return "BcStats(" + ", ".join(nat.BC_STATS) + ", log_prob, entropy, dlogits)"


_bc_workspaces: dict = {}


def _bc_actions(actions, store: tuple, device: torch.device) -> int:
    """actions of bc_loss: an int32 tensor of shape `store`, contiguous or a strided view whose elements sit one fixed pitch apart in the order of the
    flattened shape (`RowBuffers.action`, the action view of `store[1:]`) -> that pitch in bytes."""
    if not isinstance(actions, torch.Tensor) or actions.dtype != torch.int32 or tuple(actions.shape) != store or actions.device != device:
        raise ValueError(f"actions must be a torch.int32 tensor of shape {list(store)} on {device}")
    dims = [d for d in range(actions.dim()) if actions.shape[d] != 1]
    if not dims or actions.numel() == 0:
        return 4
    pitch = int(actions.stride(dims[-1]))
    even = pitch >= 1
    for hi, lo in zip(dims[:-1], dims[1:]):
        even = even and actions.stride(hi) == actions.stride(lo) * actions.shape[lo]
    if not even:
        raise ValueError("actions must be contiguous or a view whose elements sit one fixed pitch apart (RowBuffers.action)")
    return pitch * 4


def bc_loss(logits: torch.Tensor, actions: torch.Tensor, mask: Optional[torch.Tensor] = None, *, weights: Optional[torch.Tensor] = None,
            index: Optional[torch.Tensor] = None, ent_coef: float = 0.0, timing: bool = False):
    """Behaviour cloning over the masked head of `sample_actions` (bg_bc_loss): the weighted cross-entropy of stored actions, its accuracy and its
    gradient, in one pass over the logits -> (loss, stats).  loss: 0-dim float32; when `logits` require grad it carries an autograd node whose backward
    is grad_output * stats.dlogits -- `loss.backward()` drives the network's own backward with nothing recomputed.  stats: `BcStats` (loss, nll_loss,
    entropy_loss, accuracy, weight_sum, excluded, m).  The reference's `BehavioralCloning` (train_balatro_agent.py:220-262) stops at its TODO; this is
    the loss of that loop.
    logits float32 / bfloat16 [..., 60]: the network's output for the minibatch.  Without `index`, actions (int32), weights (float32) and the mask
    (forms of `sample_actions`) have the leading shape of logits.  With `index` (int32 [...]) they are STORED arrays of one common shape, read at row
    index[i]: the minibatch is gathered inside the launch.  actions may be a strided view -- `RowBuffers.action`, or the action view of `store[1:]`
    for observations `store[:K]` -- and is then read in place.
    The alignment: a record holds the observation and mask of one decision and the action of the step that LED to it, so the demonstration of
    observation record `store[t]` is the action in `store[t + 1]`.  The reference's filter ("only use successful trajectories") is
    `weights = (outcomes.end_ante[1:] >= 5).float()` with `outcomes = episode_outcomes(store)`: the outcome of the step taken from `store[t]` stands
    at `t + 1`.
    loss = sum(w * -log_prob) / W + ent_coef * -sum(w * entropy) / W, W the sum of the weights that are finite and >= 0 (of rows whose index is in
    range); accuracy = the weighted share of rows whose action is `sample_actions(deterministic=True)`'s.  A row that cannot take part (degenerate
    mask, masked or out-of-range action, non-finite log-probability, negative or non-finite weight, index out of range) is excluded: zero gradient,
    counted in stats.excluded.  W == 0 gives loss 0 and a zero gradient."""
    lead, m, pitch = _head_logits(logits)
    dev = logits.device
    store, store_rows, mask, moff, mstride = _stored_rows(lead, index, actions, mask, dev)
    astride = _bc_actions(actions, store, dev)
    if weights is not None:
        _check_scan_tensor("weights", weights, torch.float32, store, dev)
    _check_coef("ent_coef", ent_coef)
    _check_device(logits, "logits", align=0)
    _check_mask_aligned(mask, moff)
    lg = logits.detach()
    raw = torch.zeros(len(nat.BC_STATS), dtype=torch.float32, device=dev)
    dlogits = torch.empty(lead + (60,), dtype=logits.dtype, device=dev)
    log_prob = torch.empty(lead, dtype=torch.float32, device=dev)
    entropy = torch.empty(lead, dtype=torch.float32, device=dev)
    ws = _loss_workspace(_bc_workspaces, "bg_bc_loss_workspace_bytes", dev, m)
    args = (*_head_args(lg, pitch, mask, moff, mstride), _ptr(actions), C.c_uint64(astride), _ptr(weights), _ptr(index), C.c_int64(store_rows), C.c_int64(m),
            C.c_float(ent_coef), _ptr(dlogits), C.c_uint64(60), _ptr(log_prob), _ptr(entropy), _ptr(raw), _ptr(ws), C.c_uint64(ws.numel()))
    kernel_ms = _native_call("bg_bc_loss", dev, args, (), timing, empty=m == 0)   # () or (ms,)
    stats = BcStats(raw, log_prob, entropy, dlogits, *kernel_ms)
    loss = raw[0]
    if torch.is_grad_enabled() and logits.requires_grad:
        loss = _PpoLossGrad.apply(loss, dlogits, None, logits, None)   # the same node: one multiplication
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
    store, stride = _check_records(rows)
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
    _check_device(q, "q", align=0)
    _check_device(rows)   # (on q's device: checked above)
    flags = (nat.DQN_MASK_NEXT if mask_next else 0) | (nat.DQN_MSE if loss == "mse" else 0) | (nat.DQN_TIMEOUT_EXCLUDE if timeouts == "exclude" else 0)
    qd, qn = q.detach(), q_next.detach()
    qo = q_next_online.detach() if q_next_online is not None else None
    raw = torch.zeros(len(nat.DQN_STATS), dtype=torch.float32, device=dev)
    dq = torch.empty(lead + (60,), dtype=q.dtype, device=dev)
    td = torch.empty(lead, dtype=torch.float32, device=dev)
    ws = _loss_workspace(_dqn_workspaces, "bg_dqn_loss_workspace_bytes", dev, m)
    args = (_ptr(qd), C.c_uint64(pitch), _ptr(qn), C.c_uint64(npitch), _ptr(qo), C.c_uint64(opitch), nat.HEAD_F32 if q.dtype == torch.float32 else nat.HEAD_BF16,
            _ptr(rows), C.c_uint64(stride), C.c_int64(store_rows), _ptr(next_index), _ptr(rewards), C.c_int64(m), C.c_float(float(gamma)), C.c_uint32(flags),
            _ptr(dq), C.c_uint64(60), _ptr(td), _ptr(raw), _ptr(ws), C.c_uint64(ws.numel()))
    kernel_ms = _native_call("bg_dqn_loss", dev, args, (), timing, empty=m == 0)   # () or (ms,)
    stats = DqnStats(raw, td, dq, *kernel_ms)
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


class DemoBuffer:
    """Behaviour cloning's data set as a ring of self-contained demo records on the device (bg_demo_append_rows / bg_demo_sample): the reference's
    `self.expert_trajectories` (train_balatro_agent.py:220-262), which holds only the steps of the kept episodes and grows call by call.
    `rows` uint8 [capacity, stride] (128-byte aligned), `weight` float32 [capacity], `source` int32 [capacity] (the flat index t * N + e the slot came
    from in ITS call), `cursor` int64 [2] on the device: rows ever kept, rows kept by the last `add`.  `actions` (int32) and `returns` (float64) are
    strided views of bytes 172..175 and 136..143 of the ring.
    A demo record is the observation record of a kept step with the action, the terminated byte / end flags / end ante / round / chips and the
    reward (or the return handed to `add`) of the step that FOLLOWED, so `rows` goes to `encode_rows(index=)`, `RowLinear`, `RowExtractor` and
    `bc_loss(logits, demo.actions, demo.rows, weights=demo.weight, index=)` as it is, and the store it came from can be dropped.
    `add` and `sample` never synchronise: the count of kept rows, the write position and the number of filled slots stay on the device.  `len(demo)` /
    `demo.filled()` read the cursor -- the one synchronisation, for logging.
    Out of scope: prioritised or age-aware sampling, deduplication of identical records, a ring shared between GPUs.  The expert policy that fills the ring is `expert_actions`."""

    def __init__(self, capacity: int, device, row_stride: int = 384):
        C_, stride = int(capacity), int(row_stride)
        if C_ < 1 or C_ >= 2 ** 31:
            raise ValueError("capacity must be in [1, 2**31) (int32 slot indices)")
        if stride < nat.ROW_BYTES or stride % 16:
            raise ValueError(f"row_stride must be a multiple of 16 and >= the {nat.ROW_BYTES}-byte record")
        self.capacity, self.row_stride = C_, stride
        self.device = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        nbytes = C_ * stride
        self._flat = torch.zeros(nbytes + 128, dtype=torch.uint8, device=self.device)
        off = (-self._flat.data_ptr()) % 128
        self.rows = self._flat[off:off + nbytes].view(C_, stride)
        self.weight = torch.zeros(C_, dtype=torch.float32, device=self.device)
        self.source = torch.full((C_,), -1, dtype=torch.int32, device=self.device)
        self.cursor = torch.zeros(2, dtype=torch.int64, device=self.device)
        a, r = nat.ROW_EXTRA["action"][0], nat.ROW_EXTRA["reward"][0]
        self.actions = self.rows[:, a:a + 4].view(torch.int32)[:, 0]
        self.returns = self.rows[:, r:r + 8].view(torch.float64)[:, 0]
        self._workspaces: dict = {}

    def filled(self) -> int:
        """Slots that hold a record: min(rows ever kept, capacity).  Reads the cursor: a host synchronisation."""
        return min(int(self.cursor[0].item()), self.capacity)

    def __len__(self) -> int:
        return self.filled()

    def clear(self) -> None:
        """Forget every record (the cursor returns to zero; no synchronisation)."""
        self.cursor.zero_()

    def add(self, store: torch.Tensor, weights: torch.Tensor, *, returns: Optional[torch.Tensor] = None, timing: bool = False):
        """Append the KEPT steps of a finished store in one call of three launches, no synchronisation.  store: contiguous uint8 device tensor
        [K + 1, N, stride] (the record before the first step in front of the K step records: `RowBuffers.to_demo`, or a chain held elsewhere);
        candidate row (t, e), t < K, pairs observation record `store[t][e]` with `store[t + 1][e]`.  weights float32 [K, N]: a row is kept iff its
        weight is finite and > 0 -- `(episode_outcomes(store).end_ante[1:] >= 5).float()` is the reference's filter.  returns: float64 [K, N] to
        write into the demo records' reward field (`episode_outcomes(store).returns[1:].contiguous()`); without it the field is the step's reward.
        Kept rows go to consecutive slots in the order of t * N + e, wrapping; of more than `capacity` kept rows the last `capacity` survive.
        Returns None; timing=True returns the kernel milliseconds."""
        (K1, N), stride = _check_records(store, 3)
        K = K1 - 1
        if N > 0 and K < 1:
            raise ValueError("store must be [K + 1, N, stride] with K >= 1: an observation record and the record of the step taken from it")
        if max(K, 0) * N >= 2 ** 31:
            raise ValueError("K * N must be below 2**31 (int32 row indices)")
        dev = store.device
        _check_scan_tensor("weights", weights, torch.float32, (max(K, 0), N), dev)
        if returns is not None:
            _check_scan_tensor("returns", returns, torch.float64, (max(K, 0), N), dev)
        if dev != self.device:
            raise ValueError(f"the ring is on {self.device}, store is on {dev}")
        if store.numel() and store.data_ptr() < self.rows.data_ptr() + self.rows.numel() and self.rows.data_ptr() < store.data_ptr() + store.numel():
            raise ValueError("the ring must not overlap the store")
        mine = {t.data_ptr() for t in (self.rows, self.weight, self.source, self.cursor)}
        if K * N > 0 and (weights.data_ptr() in mine or (returns is not None and returns.data_ptr() in mine)):
            raise ValueError("weights / returns must not share memory with the ring's own arrays")
        _check_device(store, "store")
        M = max(K, 0) * N
        ws = _loss_workspace(self._workspaces, "bg_demo_workspace_bytes", dev, M)
        args = (_ptr(store), C.c_uint64(stride), max(K, 0), C.c_int64(N), _ptr(weights), _ptr(returns), _ptr(self.rows), C.c_uint64(self.row_stride),
                C.c_int64(self.capacity), _ptr(self.weight), _ptr(self.source), _ptr(self.cursor), _ptr(ws), C.c_uint64(ws.numel()))
        kernel_ms = _native_call("bg_demo_append_rows", dev, args, (), timing, empty=M == 0)   # () or (ms,)
        return kernel_ms[0] if kernel_ms else None

    def sample(self, m: int, *, seed: int, t: int, index0: int = 0, timing: bool = False):
        """int32 [m] on the device: uniform draws over the filled slots from the counter hash of `sample_actions` over (seed, index0 + i, t), so a
        draw does not depend on m.  An empty ring gives -1 on every row, the index `bc_loss` excludes and `encode_rows` zeroes.  No synchronisation.
        timing=True returns (index, kernel milliseconds)."""
        m = int(m)
        if m < 0:
            raise ValueError("m must be >= 0")
        _check_counters(seed, t, index0, names=("seed", "t", "index0"))
        _check_device(self.cursor, "the ring", align=0)
        index = torch.empty(m, dtype=torch.int32, device=self.device)
        args = (_ptr(self.cursor), C.c_int64(self.capacity), C.c_uint64(int(seed)), C.c_uint64(int(index0)), C.c_uint64(int(t)), _ptr(index), C.c_int64(m))
        return _native_call("bg_demo_sample", self.device, args, index, timing, empty=m == 0)

    def state_dict(self) -> dict:
        return {"rows": self.rows.clone(), "weight": self.weight.clone(), "source": self.source.clone(), "cursor": self.cursor.clone(),
                "capacity": self.capacity, "row_stride": self.row_stride}

    def load_state_dict(self, state: dict) -> None:
        shape = (int(state["capacity"]), int(state["row_stride"]))
        if shape != (self.capacity, self.row_stride):
            raise ValueError(f"the state is of a ring {list(shape)}, this one is {[self.capacity, self.row_stride]}")
        cursor = torch.as_tensor(state["cursor"])
        if cursor.dtype != torch.int64 or tuple(cursor.shape) != (2,):
            raise ValueError("the state's cursor must be int64 [2]")
        if int(cursor[0]) < 0 or not 0 <= int(cursor[1]) <= int(cursor[0]):
            raise ValueError("the state's cursor must hold 0 <= rows kept by the last call <= rows ever kept")
        self.rows.copy_(state["rows"])
        self.weight.copy_(state["weight"])
        self.source.copy_(state["source"])
        self.cursor.copy_(cursor)


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
    (K, N), stride = _check_records(rows, 3)
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
    _check_device(rows)
    if advantages is None:
        advantages = torch.empty((K, N), dtype=torch.float32, device=dev)
    if returns is None:
        returns = torch.empty((K, N), dtype=torch.float32, device=dev)
    ptrs = [values.data_ptr(), advantages.data_ptr(), returns.data_ptr()]
    if K * N and len(set(ptrs)) != 3:
        raise ValueError("advantages / returns must not share memory with values or with each other")
    args = (_ptr(rows), C.c_uint64(stride), K, C.c_int64(N), _ptr(values), _ptr(last_values), C.c_double(gamma), C.c_double(gae_lambda), _ptr(advantages),
            _ptr(returns))
    name, args = ("bg_gae_rows", args) if rewards is None else ("bg_gae_rows_ex", args + (_ptr(rewards),))
    return _native_call(name, dev, args, (advantages, returns), timing, empty=K * N == 0)   # (empty: an empty tensor has no pointer to hand over)


def expert_actions(rows: torch.Tensor, *, index: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, detail=None, timing: bool = False,
                   lanes: int = 0):
    """The scripted expert's action for every packed record, in one launch (bg_expert_actions; csrc/bg_expert.h has the rule): blind select takes the
    first valid of 45, 46, 47; the shop buys the cheapest valid joker, else leaves; a pack is skipped; in play every subset of up to five hand cards
    is valued as (base chips at the hand's level + card chips) * base mult, the best one is selected card by card and played -- or, when a discard
    is worth more, the five cheapest other cards are selected and discarded.  Stateless: a pure function of one record.

    rows: a contiguous uint8 device tensor [m, stride] or [K, N, stride] -> int32 actions [m] or [K, N] (`out`: a contiguous int32 tensor of that
    shape to fill).  index: contiguous int32 [j] of record numbers into the flattened rows -> actions [j]; an entry outside the store gives -1.
    detail: True, or a contiguous int32 tensor of the actions' shape, also returns the detail word per record -- bits 0-7 the slot mask the expert
    is selecting towards, 8-11 the best subset's hand type, 12 discard mode, 13 the fallback was used, 16-31 the subset's value -- as
    (actions, detail).  An action of -1 (no valid action, or an index outside the store) is invalid to every step call and excluded by `bc_loss`.
    Two uses: `env.expert_act()` in a collection loop fills a `DemoBuffer` with no network and no host round trip; `expert_actions(store[:K])`
    relabels a finished store of the learner's own states for `bc_loss(actions=)` (DAgger).  lanes: the lane group per record (0: the library's
    choice; 1, 8, 64: the mappings measured in profiles/expert_rows.txt)."""
    lead, stride = _check_records(rows)
    if len(lead) not in (1, 2):
        raise ValueError("rows must be a contiguous uint8 tensor [m, stride] or [K, N, stride] of packed records")
    store = 1
    for d in lead:
        store *= int(d)
    dev = rows.device
    if index is not None:
        _check_index(index, None, dev)
        lead = (int(index.numel()),)
    m = 1
    for d in lead:
        m *= int(d)
    for name, t in (("out", out), ("detail", detail)):
        if t is None or (name == "detail" and isinstance(t, bool)):
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != lead or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous int32 tensor of shape {list(lead)} on {dev}" + (", True or None" if name == "detail" else ""))
    if lanes not in (0, 1, 8, 64):
        raise ValueError("lanes must be 0, 1, 8 or 64")
    _check_device(rows)
    if out is None:
        out = torch.empty(lead, dtype=torch.int32, device=dev)
    if detail is True:
        detail = torch.empty(lead, dtype=torch.int32, device=dev)
    elif detail is False:
        detail = None
    args = (_ptr(rows), C.c_int64(stride), C.c_int64(m), _ptr(index), C.c_int64(store), _ptr(out), _ptr(detail), int(lanes))
    return _native_call("bg_expert_actions_ex", dev, args, out if detail is None else (out, detail), timing, empty=m == 0)


OUTCOME_FIELDS = {"steps_to_end": torch.int32, "end_ante": torch.int32, "end_flags": torch.uint8, "returns": torch.float64}


class EpisodeOutcomes:
    """What `episode_outcomes` returns: per step of a [K, N] rollout the outcome of the step's OWN episode -- `steps_to_end` int32 (0 on the ending
    step, -1 in an episode that is still open), `end_ante` int32 (-1 open), `end_flags` uint8 (0 open), `returns` float64 (the discounted reward sum
    from the step to its episode's end) -- each [K, N], or None where it was not asked for.  `kernel_ms` with timing=True."""

    def __init__(self, steps_to_end=None, end_ante=None, end_flags=None, returns=None, kernel_ms=None):
        self.steps_to_end, self.end_ante, self.end_flags, self.returns, self.kernel_ms = steps_to_end, end_ante, end_flags, returns, kernel_ms

    def tail(self) -> dict:
        """Row 0 of every field that was computed: what `episode_outcomes(..., tail=)` of the PRECEDING chunk takes."""
        return {f: getattr(self, f)[0] for f in OUTCOME_FIELDS if getattr(self, f) is not None}

    def __repr__(self):
        return "EpisodeOutcomes(" + ", ".join(f for f in OUTCOME_FIELDS if getattr(self, f) is not None) + ")"


def episode_outcomes(rows: torch.Tensor, gamma: float = 1.0, *, rewards: Optional[torch.Tensor] = None, tail: Optional[dict] = None,
                     want=("steps_to_end", "end_ante", "end_flags", "returns"), timing: bool = False) -> EpisodeOutcomes:
    """Every step of a finished [K, N] rollout of packed records learns the outcome of its own episode, in one launch (bg_episode_outcome_rows): the
    backward pass along K that `end_ante` -- written only into the record of the ENDING step -- needs before it can filter steps, and the Monte-Carlo
    return of every step.  Bit for bit the numpy loop: per env, t = K-1 .. 0, a set terminated byte gives (0, the record's end ante, its end flags,
    r), any other step (next.steps + 1 or -1, next.ante, next.flags, r + gamma * next.ret) in float64.
    rows: contiguous uint8 device tensor [K, N, stride] (`RowBuffers.rows`, `RowReplay.store`) of `step_many(..., limits=EpisodeLimits(...,
    summary=True))` (without the summary end_ante is 0, without limits end_flags too).  rewards: float64 [K, N] to take instead of the records'
    rewards (`normalize_reward`'s output).  want: the fields to compute.  tail: `later.tail()` of the same call on the FOLLOWING chunk (a dict field
    -> [N] tensor), so a long store is processed in pieces from the back; without it an episode that does not end inside the call is open (-1, -1, 0,
    the sum so far).
    The alignment: the step taken from observation record `store[t]` is record `store[t + 1]`, so the reference's behaviour-cloning filter over
    observations `store[:K]` is `weights = (episode_outcomes(store).end_ante[1:] >= 5).float()` -- see `bc_loss`."""
    (K, N), stride = _check_records(rows, 3)
    dev = rows.device
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(f not in OUTCOME_FIELDS for f in want) or len(set(want)) != len(want):
        raise ValueError(f"want must name at least one of {list(OUTCOME_FIELDS)}, each once (got {list(want)})")
    if rewards is not None:
        _check_scan_tensor("rewards", rewards, torch.float64, (K, N), dev)
        if "returns" not in want:
            raise ValueError("rewards are read only for 'returns': ask for it or leave rewards out")
    tail = {} if tail is None else tail
    if not isinstance(tail, dict) or any(f not in OUTCOME_FIELDS for f in tail):
        raise ValueError(f"tail must be a dict with keys from {list(OUTCOME_FIELDS)} (EpisodeOutcomes.tail())")
    for f, t in tail.items():
        if f not in want:
            raise ValueError(f"tail[{f!r}] without its output: add {f!r} to want")
        _check_scan_tensor(f"tail[{f!r}]", t, OUTCOME_FIELDS[f], (N,), dev)
    gamma = float(gamma)
    if np.isnan(gamma):
        raise ValueError("gamma must not be NaN")
    _check_device(rows)
    outs = {f: torch.empty((K, N), dtype=OUTCOME_FIELDS[f], device=dev) if f in want else None for f in OUTCOME_FIELDS}
    args = (_ptr(rows), C.c_uint64(stride), K, C.c_int64(N), C.c_double(gamma), _ptr(rewards), *(_ptr(tail.get(f)) for f in OUTCOME_FIELDS),
            *(_ptr(outs[f]) for f in OUTCOME_FIELDS))
    kernel_ms = _native_call("bg_episode_outcome_rows", dev, args, (), timing, empty=K * N == 0)   # () or (ms,)
    return EpisodeOutcomes(**outs, kernel_ms=kernel_ms[0] if kernel_ms else None)


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
        _zero_where(mask, self.n, self.device, self.ep_return_carry, self.ep_len_carry)

    def update(self, rows: torch.Tensor, ep_return: Optional[torch.Tensor] = None, ep_len: Optional[torch.Tensor] = None, timing: bool = False):
        """The next K steps of every env: rows contiguous uint8 [K, N, stride] on this device.  Returns (ep_return float64 [K, N], ep_len int32
        [K, N]): on a terminated step the finished episode's reward sum and length, 0.0 / 0 elsewhere (`ep_len.nonzero()` lists the episodes);
        timing=True appends the kernel milliseconds.  ep_return / ep_len: optional tensors to write into."""
        (K, N), stride = _check_records(rows, 3)
        if N != self.n or rows.device != self.device:
            raise ValueError(f"rows must hold records of {self.n} envs on {self.device} (got {N} envs on {rows.device})")
        if ep_return is not None:
            _check_scan_tensor("ep_return", ep_return, torch.float64, (K, N), self.device)
        if ep_len is not None:
            _check_scan_tensor("ep_len", ep_len, torch.int32, (K, N), self.device)
        _check_device(rows)
        if ep_return is None:
            ep_return = torch.empty((K, N), dtype=torch.float64, device=self.device)
        if ep_len is None:
            ep_len = torch.empty((K, N), dtype=torch.int32, device=self.device)
        args = (_ptr(rows), C.c_uint64(stride), K, C.c_int64(N), _ptr(self.ep_return_carry), _ptr(self.ep_len_carry), _ptr(ep_return), _ptr(ep_len))
        return _native_call("bg_episode_stats_rows", self.device, args, (ep_return, ep_len), timing, empty=K * N == 0)


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
        _zero_where(mask, self.n, self.device, self.counters)

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
        _zero_where(mask, self.n, self.device, self.counters)

    def state_dict(self) -> dict:
        return {"counters": self.counters.cpu().clone()}

    def load_state_dict(self, state: dict) -> None:
        c = torch.as_tensor(state["counters"])
        if tuple(c.shape) != (self.n, 4):
            raise ValueError(f"counters must have shape [{self.n}, 4]")
        self.counters.copy_(c.to(device=self.device, dtype=torch.int32))


def _episode_ends_call(rows, cur: Optional["nat.Curriculum"], n_expected: Optional[int], timing: bool):
    """-> the report, with timing (report, kernel milliseconds)."""
    (K, N), stride = _check_records(rows, 3)
    if n_expected is not None and N != n_expected:
        raise ValueError(f"rows must hold records of {n_expected} envs (got {N})")
    _check_device(rows)
    empty = K * N == 0   # nothing to launch (an empty tensor has no pointer to hand over): the report is zeros
    report = (torch.zeros if empty else torch.empty)(nat.ENDS_WORDS, dtype=torch.int64, device=rows.device)
    args = (_ptr(rows), C.c_uint64(stride), K, C.c_int64(N), _ptr(report), None if cur is None else C.byref(cur))
    return _native_call("bg_episode_ends_rows", rows.device, args, report, timing, empty=empty)


def episode_ends(rows: torch.Tensor, timing: bool = False):
    """The ended episodes of a finished [K, N] rollout of packed records in one launch (bg_episode_ends_rows): int64 [32] on the device, words by
    `_native.ENDS_REPORT` -- ended records, of which game overs / kills / step-limit-only endings, sum and maximum of the end ante and of the end
    chips, records without a summary -- and from `_native.ENDS_HIST` on the histogram of min(end ante, 15).  rows: contiguous uint8 device tensor
    [K, N, stride] (`RowBuffers.rows`) of `step_many(..., limits=EpisodeLimits(..., summary=True))`.  timing=True returns (report, kernel ms)."""
    return _episode_ends_call(rows, None, None, timing)


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
        res = _episode_ends_call(rows, self._struct(), self.n, timing)
        report = res[0] if timing else res
        if rows.shape[0] * rows.shape[1] == 0:
            self.raised.zero_()
        elif apply and int(report[nat.ENDS_REPORT["raised"]].item()):
            self.env.set_max_ante(self.cap.cpu().numpy(), mask=self.raised.cpu().numpy())
        return res

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
        _zero_where(mask, self.n, self.device, self.returns)

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
        (K, N), stride = _check_records(_norm_rows(rows), 3)
        if N != self.n or rows.device != self.device:
            raise ValueError(f"rows must hold records of {self.n} envs on {self.device} (got {N} envs on {rows.device})")
        return K, N, stride

    def _ready(self, K, N) -> torch.Tensor:
        """The cached workspace, grown to what K steps of N envs need; an empty shape needs none and loads nothing."""
        need = int(nat.load().bg_norm_workspace_bytes(K, C.c_int64(N))) if K * N else 0
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
        _check_device(rows)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=self.device)
        ws = self._ready(K, N)
        args = (_ptr(rows), C.c_uint64(stride), K, C.c_int64(N), nat.ENC_LAYOUTS[layout], nat.ENC_F32 if dtype == torch.float32 else nat.ENC_BF16,
                _ptr(self.obs_mean), _ptr(self.obs_var), _ptr(self.obs_count), 1 if (self.training if update is None else update) else 0,
                C.c_double(self.epsilon), C.c_double(self.clip_obs), _ptr(out), C.c_uint64(D), None, _ptr(ws), C.c_uint64(ws.numel()))
        return _native_call("bg_norm_obs_rows", self.device, args, out, timing, empty=K * N == 0)

    def normalize_reward(self, rows: torch.Tensor, out: Optional[torch.Tensor] = None, timing: bool = False):
        """K VecNormalize steps over the rewards of rows: returns the normalised rewards, float64 [K, N] (or [N] for [N, stride] rows), what
        `gae_rows(..., rewards=)` takes.  out: optional contiguous float64 tensor of that shape.  timing=True appends the kernel milliseconds."""
        if not self.norm_reward:
            raise ValueError("this RowNormalizer was made with norm_reward=False: the records' own rewards are `RowBuffers.reward`")
        K, N, stride = self._check_rows(rows)
        shape = (K, N) if rows.dim() == 3 else (N,)
        if out is not None:
            _check_scan_tensor("out", out, torch.float64, shape, self.device)
        _check_device(rows)
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=self.device)
        ws = self._ready(K, N)
        args = (_ptr(rows), C.c_uint64(stride), K, C.c_int64(N), _ptr(self.returns), _ptr(self.ret_stats), 1 if self.training else 0, C.c_double(self.gamma),
                C.c_double(self.epsilon), C.c_double(self.clip_reward), _ptr(out), None, _ptr(ws), C.c_uint64(ws.numel()))
        return _native_call("bg_norm_reward_rows", self.device, args, out, timing, empty=K * N == 0)
