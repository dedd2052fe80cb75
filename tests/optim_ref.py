"""bg_optim_step restated in numpy float32: the whole call -- the norm in THE REDUCTION ORDER of csrc/bg_ppo.h, the clip, Adam and RMSpropTFLike, the L2
term, the skip on a non-finite norm, the bfloat16 shadows (by integer arithmetic), polyak and the zeroing -- one operation at a time, each rounded on its
own, exactly as csrc/bg_optim.h states its contract.  The g++ build of that header and the GPU are held to this file bit for bit.

Where torch's own kernels differ between devices the contract picks one: `addcmul` in the order of torch's CPU kernel, (value * t1) * t2, and `addcdiv`
in the order of its GPU kernel, value * (t1 / t2); `lerp` with a weight below one half is self + weight * (end - self) on both.

THE BOUND AGAINST FLOAT64 (`Err`, `step_bound`).  Let u = 2**-24.  A float32 operation returns fl(x op y) = (x op y)(1 + d), |d| <= u, or is off by at most
2**-149 where the result is subnormal.  Every quantity of the step is carried as a pair (v, e): v the float32 value this file computes, e a bound on
|v - x| with x the value exact arithmetic gives from the exact inputs.  With a^ = a + da, |da| <= e_a:
    product    |fl(a^ b^) - a b| <= u |v| + |a^| e_b + |b^| e_a + e_a e_b
    sum        |fl(a^ + b^) - (a + b)| <= u |v| + e_a + e_b
    quotient   a^/b^ - a/b = (v (b - b^) + (a^ - a)) / b, so |.| <= u |v| + (|v| e_b + e_a) / (|b^| - e_b)
    root       |sqrt(a^) - sqrt(a)| = |a^ - a| / (sqrt(a^) + sqrt(a)) <= min(e_a / sqrt(a^), sqrt(e_a)), plus u |v|
The inputs' errors: a hyperparameter rounded to float32 is off by u |h|; the norm float32(sqrt(S)) by u norm (S itself is a float64 sum: 2**-40
relative covers it) plus the 2-norm of the gradients' own errors; c = min(1, q) by the error of q, or by nothing where q - e_q >= 1; the carried
beta ** step by step * 2**-53 relative (the iterated product), so a = lr / (1 - b1pow) by a (u + 2 step 2**-53 b1pow / (1 - b1pow)) and s2 likewise.
`step_bound` runs the step's own expressions on such pairs, so the bound is made of the values of the very step it bounds; over k steps the errors of
p, m and v are carried from step to step and the gradients' differences enter as e_g (`KStepBound`).  The bound's own float64 arithmetic is covered by
a factor 1 + 2**-20."""
import numpy as np

LANES, PER_LANE = 256, 4
CHUNK = LANES * PER_LANE
ADAM, RMSPROP_TF = 0, 1
U = 2.0 ** -24
TINY = 2.0 ** -149
F = np.float32


def bf16_bits(x):
    """float32 -> bfloat16 bits, round to nearest even, by integer arithmetic; a NaN becomes 0x7fc0 (bg_ppo_bf16)."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    out = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    out[np.isnan(x)] = 0x7FC0
    return out


def chunks_of(numel):
    return -(-int(numel) // CHUNK)


def _tree(t):
    """TREE over the last axis (a power of two)."""
    t = t.copy()
    s = t.shape[-1] // 2
    while s:
        t[..., :s] = t[..., :s] + t[..., s:2 * s]
        s //= 2
    return t[..., 0]


def _slices_then_tree(part):
    P = len(part)
    per = -(-P // LANES)
    pad = np.zeros(LANES * per, np.float64)
    pad[:P] = part          # a lane folds from +0.0, and x + 0.0 is x: the padding changes nothing
    lanes = np.zeros(LANES, np.float64)
    sl = pad.reshape(LANES, per)
    for j in range(per):
        lanes = lanes + sl[:, j]
    return _tree(lanes)


def grad_norm(grads):
    """-> (S float64, nonfinite count) of the gradients (1-D float32 arrays) in table order, in the order of the contract."""
    parts, nf = [], 0
    with np.errstate(all="ignore"):
        for g in grads:
            g = np.ascontiguousarray(g, np.float32).ravel()
            k = chunks_of(g.size)
            q = np.zeros(k * CHUNK, np.float64)
            q[:g.size] = g.astype(np.float64)
            q = (q * q).reshape(k, LANES, PER_LANE)
            lane = np.zeros((k, LANES), np.float64)
            for j in range(PER_LANE):
                lane = lane + q[:, :, j]
            parts.append(_tree(lane))
            nf += int((~np.isfinite(g)).sum())
        S = _slices_then_tree(np.concatenate(parts)) if parts else np.float64(0.0)
    return S, nf


class Hyper:
    """The call's scalar arguments as the library rounds them once on the host (bg_optim_hyper)."""

    def __init__(self, algo=ADAM, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, weight_decay=0.0, max_norm=0.5, tau=0.0, zero_grad=True):
        self.algo, self.lr, self.beta1, self.beta2, self.zero_grad = algo, float(lr), float(beta1), float(beta2), bool(zero_grad)
        self.max_norm = F(max_norm)
        self.omb1, self.b2, self.omb2, self.al = F(1.0 - float(beta1)), F(beta2), F(1.0 - float(beta2)), F(beta1)
        self.eps, self.wd, self.tau, self.omt = F(eps), F(weight_decay), F(tau), F(1.0 - float(tau))
        self.raw = dict(eps=float(eps), weight_decay=float(weight_decay), max_norm=float(max_norm), tau=float(tau))


class Carry:
    def __init__(self, step=0, b1pow=1.0, b2pow=1.0):
        self.step, self.b1pow, self.b2pow = int(step), float(b1pow), float(b2pow)

    @classmethod
    def at(cls, step, beta1, beta2):
        """The carried state after `step` steps: the same iterated products."""
        c = cls()
        for _ in range(step):
            c.b1pow, c.b2pow = c.b1pow * beta1, c.b2pow * beta2
        c.step = step
        return c


class Tensor:
    """One table entry on the host: flat float32 p, g, s1, s2 (s2 None for RMSprop), an optional shadow (uint16 [rows * pitch] with cols / pitch) and an
    optional float32 target."""

    def __init__(self, p, g, s1, s2=None, shadow=None, cols=0, pitch=0, target=None):
        self.p, self.g, self.s1, self.s2, self.shadow, self.cols, self.pitch, self.target = p, g, s1, s2, shadow, int(cols), int(pitch), target

    def shadow_index(self):
        i = np.arange(self.p.size, dtype=np.int64)
        return i if self.cols == self.pitch else (i // self.cols) * self.pitch + i % self.cols


def finish(S, nf, h: Hyper, carry: Carry):
    """bg_optim_finish: -> (c, a, s2, stats); advances `carry` unless the step is skipped."""
    with np.errstate(all="ignore"):
        norm = F(np.sqrt(np.float64(S)))
        skip = not np.isfinite(norm)
        c = F(1.0)
        if h.max_norm > 0:
            c = F(np.fmin(F(1.0), h.max_norm / (norm + F(1e-6))))   # fminf: of (1, NaN) it is 1; a NaN norm is a skipped step either way
    if not skip:
        carry.step += 1
        if h.algo == ADAM:
            carry.b1pow, carry.b2pow = carry.b1pow * h.beta1, carry.b2pow * h.beta2
    if h.algo == ADAM:
        a, s2 = F(h.lr / (1.0 - carry.b1pow)), F(np.sqrt(1.0 - carry.b2pow))
    else:
        a, s2 = F(h.lr), F(1.0)
    return c, a, s2, dict(grad_norm=norm, clip_coef=c, skipped=int(skip), nonfinite=int(nf), step=carry.step)


def elem(h: Hyper, g, p, s1, s2v, c, a, s2):
    """bg_optim_elem on arrays: -> (p, s1, s2v)."""
    with np.errstate(all="ignore"):
        g = g * c
        if h.wd != 0:
            g = g + p * h.wd
        if h.algo == ADAM:
            s1 = s1 + (g - s1) * h.omb1
            s2v = s2v * h.b2 + (h.omb2 * g) * g
            p = p + (s1 / (np.sqrt(s2v) / s2 + h.eps)) * (-a)
        else:
            s1 = s1 * h.al + (h.omb1 * g) * g
            p = p + (g / np.sqrt(s1 + h.eps)) * (-a)
    for x in (p, s1):
        assert x.dtype == np.float32
    return p, s1, s2v


def step(tensors, h: Hyper, carry: Carry):
    """The whole call, in place on `tensors` and `carry` -> stats."""
    S, nf = grad_norm([t.g for t in tensors])
    c, a, s2, stats = finish(S, nf, h, carry)
    for t in tensors:
        if not stats["skipped"]:
            t.p[:], t.s1[:], s2v = elem(h, t.g, t.p, t.s1, t.s2 if h.algo == ADAM else None, c, a, s2)
            if h.algo == ADAM:
                t.s2[:] = s2v
            if t.shadow is not None:
                t.shadow[t.shadow_index()] = bf16_bits(t.p)
            if t.target is not None and h.tau > 0:
                t.target[:] = t.p if h.tau == 1 else t.target * h.omt + t.p * h.tau
        if h.zero_grad:
            t.g[:] = 0
    return stats


def refresh(tensors):
    """BG_OPTIM_SHADOW_ONLY."""
    for t in tensors:
        if t.shadow is not None:
            t.shadow[t.shadow_index()] = bf16_bits(t.p)


# ---------------------------------------------------------------------------------------------------- the bound against float64
class Err:
    """(v, e): a float32 value and a bound on its distance from the exact one (module docstring)."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float32)
        self.e = np.asarray(e, np.float64) + np.zeros(self.v.shape)

    @staticmethod
    def const(x):
        """A hyperparameter rounded to float32."""
        return Err(F(x), U * abs(float(x)))

    def _r(self, v):
        return U * np.abs(v.astype(np.float64)) + TINY

    def __mul__(self, o):
        v = self.v * o.v
        a, b = np.abs(self.v.astype(np.float64)), np.abs(o.v.astype(np.float64))
        return Err(v, self._r(v) + a * o.e + b * self.e + self.e * o.e)

    def __add__(self, o):
        v = self.v + o.v
        return Err(v, self._r(v) + self.e + o.e)

    def __sub__(self, o):
        v = self.v - o.v
        return Err(v, self._r(v) + self.e + o.e)

    def __truediv__(self, o):
        v = self.v / o.v
        den = np.abs(o.v.astype(np.float64)) - o.e
        with np.errstate(all="ignore"):
            e = np.where(den > 0, (np.abs(v.astype(np.float64)) * o.e + self.e) / np.where(den > 0, den, 1.0), np.inf)
        return Err(v, self._r(v) + e)

    def sqrt(self):
        v = np.sqrt(self.v)
        with np.errstate(all="ignore"):
            e = np.minimum(np.where(v > 0, self.e / np.where(v > 0, v.astype(np.float64), 1.0), np.inf), np.sqrt(self.e))
        return Err(v, self._r(v) + e)

    def neg(self):
        return Err(-self.v, self.e)


def step_bound(h: Hyper, carry_after: Carry, S, p, g, s1, s2v, e_p=0.0, e_g=0.0, e_s1=0.0, e_s2v=0.0, e_g_norm=0.0):
    """One step that is not skipped: the contract's expressions on (value, error) pairs.  p, g, s1, s2v: the float32 inputs of one tensor (arrays);
    S: the float64 sum of squares of ALL gradients of the call; carry_after: the carried state behind this step; e_*: the inputs' own errors
    (0: exact inputs); e_g_norm: the 2-norm of all gradients' errors.  -> (Err p, Err s1, Err s2v): .v are the step's float32 results, .e the bounds."""
    with np.errstate(all="ignore"):
        norm = F(np.sqrt(np.float64(S)))
        if h.max_norm > 0:
            e_norm = (U + 2.0 ** -40) * float(norm) + float(e_g_norm)
            d = Err(norm, e_norm) + Err(F(1e-6), U * 1e-6)
            q = Err(h.max_norm, U * float(h.max_norm)) / d
            cv = np.minimum(F(1.0), q.v)
            C = Err(cv, 0.0 if float(q.v) - float(q.e) >= 1.0 else q.e)
        else:
            C = Err(F(1.0))
        n = carry_after.step
        if h.algo == ADAM:
            a = F(h.lr / (1.0 - carry_after.b1pow))
            s2 = F(np.sqrt(1.0 - carry_after.b2pow))
            A = Err(a, float(a) * (U + 2.0 * n * 2.0 ** -53 * carry_after.b1pow / (1.0 - carry_after.b1pow)))
            S2 = Err(s2, float(s2) * (U + 2.0 * n * 2.0 ** -53 * carry_after.b2pow / (1.0 - carry_after.b2pow)))
        else:
            A, S2 = Err.const(h.lr), Err(F(1.0))
        P, G, S1 = Err(p, e_p), Err(g, e_g), Err(s1, e_s1)
        G = G * C
        if h.wd != 0:
            G = G + P * Err.const(h.raw["weight_decay"])
        if h.algo == ADAM:
            V = Err(s2v, e_s2v)
            S1 = S1 + (G - S1) * Err.const(1.0 - h.beta1)
            V = V * Err.const(h.beta2) + (Err.const(1.0 - h.beta2) * G) * G
            P = P + (S1 / (V.sqrt() / S2 + Err.const(h.raw["eps"]))) * A.neg()
        else:
            V = None
            S1 = S1 * Err.const(h.beta1) + (Err.const(1.0 - h.beta1) * G) * G
            P = P + (G / (S1 + Err.const(h.raw["eps"])).sqrt()) * A.neg()
    slack = 1.0 + 2.0 ** -20
    for x in (P, S1) + ((V,) if V is not None else ()):
        x.e = x.e * slack
    return P, S1, V


def exact_step(h: Hyper, step_after, p, g, s1, s2v, norm):
    """The step in float64 with beta ** step: what torch.optim.Adam / RMSpropTFLike compute on float64 tensors (tests hold this to torch itself)."""
    p, g, s1 = p.astype(np.float64), g.astype(np.float64), s1.astype(np.float64)
    mn = h.raw["max_norm"]
    c = min(1.0, mn / (norm + 1e-6)) if mn > 0 else 1.0
    g = g * c
    if h.raw["weight_decay"] != 0:
        g = g + p * h.raw["weight_decay"]
    if h.algo == ADAM:
        s2v = s2v.astype(np.float64)
        s1 = s1 + (g - s1) * (1.0 - h.beta1)
        s2v = s2v * h.beta2 + (1.0 - h.beta2) * g * g
        a = h.lr / (1.0 - h.beta1 ** step_after)
        p = p - a * (s1 / (np.sqrt(s2v) / np.sqrt(1.0 - h.beta2 ** step_after) + h.raw["eps"]))
    else:
        s1 = s1 * h.beta1 + (1.0 - h.beta1) * g * g
        p = p - h.lr * (g / np.sqrt(s1 + h.raw["eps"]))
    return p, s1, s2v


class KStepBound:
    """The k-step bound: one per trajectory.  Each `advance` takes the float32 inputs of one step of every tensor (before the step), the errors of
    the gradients against the exact trajectory's, and carries the errors of p, m and v forward."""

    def __init__(self, h: Hyper, ntensors: int):
        self.h, self.carry = h, Carry()
        self.e = [(0.0, 0.0, 0.0)] * ntensors   # (e_p, e_s1, e_s2v) per tensor

    def advance(self, ps, gs, s1s, s2s, e_gs, e_norm=0.0):
        """e_norm: what the norm this trajectory clipped with is off by beyond the contract's own rounding (torch's float32 reduction, measured)."""
        S, _ = grad_norm(gs)
        e_g_norm = float(np.sqrt(sum(float((np.asarray(e, np.float64) ** 2).sum()) for e in e_gs))) + float(e_norm)
        self.carry.step += 1
        if self.h.algo == ADAM:
            self.carry.b1pow, self.carry.b2pow = self.carry.b1pow * self.h.beta1, self.carry.b2pow * self.h.beta2
        out = []
        for i, (p, g, s1, s2v, e_g) in enumerate(zip(ps, gs, s1s, s2s, e_gs)):
            e_p, e_s1, e_s2 = self.e[i]
            P, S1, V = step_bound(self.h, self.carry, S, p.ravel(), g.ravel(), s1.ravel(), None if s2v is None else s2v.ravel(), e_p, np.asarray(e_g, np.float64).ravel(),
                                  e_s1, e_s2, e_g_norm)
            self.e[i] = (P.e, S1.e, V.e if V is not None else 0.0)
            out.append(P)
        return out


# ---------------------------------------------------------------------------------------------------- test sets
BASE_SHAPES = [(1,), (3,), (4,), (5,), (60,), (1023,), (1024,), (1025,), (32, 447), (60, 256)]
OFFSET_TENSOR = 4   # this tensor of the base set starts one float into its storage: the element path
SHADOWED = {8: 448, 9: 256}   # tensor -> its shadow's pitch
TARGETED = (5, 7, 9)


def random_set(seed, shapes=BASE_SHAPES, algo=ADAM, gscale=1.0):
    """-> list of dicts of float32 arrays (p, g, s1, s2) with random state: m ~ N(0, 0.1), v uniform in [1e-4, 1e-1], sq likewise."""
    rng = np.random.default_rng(seed)
    out = []
    for shape in shapes:
        n = int(np.prod(shape))
        out.append(dict(shape=shape, p=rng.normal(0, 1, n).astype(F), g=(rng.normal(0, 1, n) * gscale).astype(F),
                        s1=(rng.normal(0, 0.1, n) if algo == ADAM else rng.uniform(1e-4, 1e-1, n)).astype(F),
                        s2=rng.uniform(1e-4, 1e-1, n).astype(F), target=rng.normal(0, 1, n).astype(F)))
    return out


# ---------------------------------------------------------------------------------------------------- the C ABI's blocks, for the tests that build them
ENTRY = np.dtype([("param", "<u8"), ("grad", "<u8"), ("state1", "<u8"), ("state2", "<u8"), ("shadow", "<u8"), ("target", "<u8"), ("numel", "<u8"),
                  ("cols", "<u4"), ("pitch", "<u4")])
CARRY = np.dtype([("step", "<i8"), ("b1pow", "<f8"), ("b2pow", "<f8"), ("pad", "<f8")])
STATS = np.dtype([("grad_norm", "<f4"), ("clip_coef", "<f4"), ("skipped", "<i4"), ("zero", "<i4"), ("nonfinite", "<i8"), ("step", "<i8")])
ZERO_GRAD, SHADOW_ONLY = 1, 2


def aligned(n, dtype=np.float32, skew=0):
    """n elements of `dtype` in host memory that starts `skew` elements behind a 16-byte boundary."""
    item = np.dtype(dtype).itemsize
    raw = np.zeros((n + skew) * item + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + (n + skew) * item].view(dtype)[skew:]


def pack_table(tensors):
    """Host `Tensor`s -> (the table's bytes as a 16-byte aligned uint8 array, chunks): entries, then the prefix of chunk counts."""
    ent = np.zeros(len(tensors), ENTRY)
    prefix = np.zeros(len(tensors) + 1, np.uint32)
    for k, t in enumerate(tensors):
        e = ent[k]
        e["param"], e["grad"], e["state1"], e["numel"] = t.p.ctypes.data, t.g.ctypes.data, t.s1.ctypes.data, t.p.size
        e["state2"] = t.s2.ctypes.data if t.s2 is not None else 0
        e["shadow"] = t.shadow.ctypes.data if t.shadow is not None else 0
        e["target"] = t.target.ctypes.data if t.target is not None else 0
        e["cols"], e["pitch"] = (t.cols, t.pitch) if t.shadow is not None else (1, 1)
        prefix[k + 1] = prefix[k] + chunks_of(t.p.size)
    blob = ent.tobytes() + prefix.tobytes()
    out = aligned(len(blob), np.uint8)
    out[:] = np.frombuffer(blob, np.uint8)
    return out, int(prefix[-1])


def host_set(data, algo, skew_tensor=OFFSET_TENSOR, shadowed=SHADOWED, targeted=TARGETED):
    """`random_set`'s dicts -> two equal lists of `Tensor`s in separate memory: one for the code under test (16-byte aligned arrays, tensor
    `skew_tensor` one float behind a boundary; shadows prefilled with 0x7b7b so untouched padding shows) and one for this reference."""
    def build(copy_aligned):
        out = []
        for i, d in enumerate(data):
            n = d["p"].size
            skew = 1 if i == skew_tensor else 0

            def arr(x, skew=skew):
                if not copy_aligned:
                    return x.copy()
                a = aligned(n, np.float32, skew)
                a[:] = x
                return a
            sh = cols = pitch = None
            if i in shadowed:
                cols, pitch = d["shape"][1], shadowed[i]
                sh = aligned(d["shape"][0] * pitch, np.uint16) if copy_aligned else np.zeros(d["shape"][0] * pitch, np.uint16)
                sh[:] = 0x7B7B
            out.append(Tensor(arr(d["p"]), arr(d["g"]), arr(d["s1"]), arr(d["s2"]) if algo == ADAM else None, sh, cols or 0, pitch or 0,
                              arr(d["target"], 0) if i in targeted else None))
        return out
    return build(True), build(False)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
