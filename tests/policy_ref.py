"""Shared by tests/test_policy_rows_host.py and tests/test_policy_rows.py: the float64 statement of one layer of bg_policy_forward over the WIDENED
bfloat16 operands, its bound, and the nets the two files run.  The head behind the logits is not restated: it is held bit for bit to sample_actions /
evaluate_actions on the same logits, which tests/head_ref.py holds to float64.

ONE LAYER.  x bfloat16 [m, in], w bfloat16 [out, in], b float32 [out]:  s = sum_k x w + b in float64.  A bfloat16 x bfloat16 product is exact in
float32, so only the accumulation rounds; as in tests/actor_ref.py a float32 sum of L terms in any order is within (L - 1) u S of the exact sum
(u = 2**-24, S the sum of the magnitudes), (L + 2) with the bias add and the slack of the first-order statement, and a factor 2 because the matrix
unit's internal adder is not documented as round-to-nearest:
    pre-activation   |y - s| <= B = 2 (in + 2) u (sum_k |x w| + |b|) + u |s|          (the last term: one float32 rounding of the result)
    none, relu       the same B: max(., 0) moves two numbers no further apart
    tanh             |got - tanh(s)| <= B + TANH_ABS: tanh is 1-Lipschitz, and the float32 formula adds TANH_ABS (below)
The logits and the value stay float32 and are checked against ref +- B directly.  A hidden layer's output is rounded to nearest-even bfloat16, and
rounding is monotone: the bfloat16 output must lie in [rne(ref - bound), rne(ref + bound)] (`check_interval`; rne through float32 first, as the kernel
rounds a float32 -- a composition of monotone roundings).  Every layer is checked against the kernel's OWN tapped input of that layer, so no error
propagates from layer to layer.

THE TANH FORMULA (csrc/bg_policy.h, bg_pol_tanh):  a = |y|;  t = 2 a;  e = expf(t);  r = 1 - 2 / (e + 1);  the sign of y put back; every operation
rounded to float32 on its own (no fused multiply-add, IEEE division).  Its absolute error against tanh(a) = 1 - Q, Q = 2 / (exp(t) + 1) in (0, 1]:
    a and t are exact (a sign flip, a doubling).
    e = exp(t) (1 + d1), |d1| <= E.  The device library documents expf at 1 ulp and glibc's is below 1 ulp; E = 2 ulp = 2**-22 = 4 u is taken.
    e + 1 = (exp(t) + 1) (1 + d1 exp(t) / (exp(t) + 1)): a relative change of at most E; its float32 rounding adds d2, the division d3, |d2|, |d3| <= u.
    q = Q (1 + theta), |theta| <= E + 2 u + second-order terms below 1e-12 < 6.01 u, so |q - Q| <= 6.01 u Q <= 6.01 u.
    r = (1 - q) (1 + d4), |d4| <= u, |1 - q| <= 1: |r - (1 - Q)| <= 6.01 u + u = 7.01 u.
TANH_ABS = 8 u = 2**-21.  For t beyond float32's range e is +inf, q = 0 and r = 1: tanh's value to far below u."""
import numpy as np

from tests.linear_ref import U, check_close, to_bf16_bits, widen  # noqa: F401

UNITS = 60
ROWS = 32             # BG_POL_ROWS: rows of a workgroup
TANH_ABS = 8 * U
ACT = {None: 0, "relu": 1, "tanh": 2}

# the reference's main network behind its first layer (train_balatro_agent.py:54-82, 338-342): the three second layers as one block-diagonal
# 448 -> 224, combined_net 224 -> 512 -> 512, pi and vf 512 -> 256 -> 256 with tanh, action_net and value_net
REFERENCE = dict(in0=448, trunk=[(224, "relu"), (512, "relu"), (512, "relu")], pi=[(256, "tanh"), (256, "tanh")], vf=[(256, "tanh"), (256, "tanh")], value=True)
# the exact cases: an image swap, a layer order or a lane map that is wrong cannot pass them
EXACT = {
    "64-32|pi32|novf": dict(in0=64, trunk=[(32, "relu")], pi=[(32, None)], vf=[], value=False),
    "empty-sections-in512": dict(in0=512, trunk=[], pi=[], vf=[], value=True),
    "4+4+4x32": dict(in0=32, trunk=[(32, "relu"), (32, None), (32, "relu"), (32, "relu")], pi=[(32, "relu"), (32, "relu"), (32, None), (32, "relu")],
                     vf=[(32, None), (32, "relu"), (32, "relu"), (32, "relu")], value=True),
    "512-per-section": dict(in0=96, trunk=[(512, "relu")], pi=[(512, "relu")], vf=[(512, None)], value=True),
    # k-steps that end inside a batch of 8 behind the first batch (in 160: 10 steps, in 288: 18); tiles that give waves 0 and 1 two tiles and the others
    # one (out 288 over 8 waves x 32 units), and waves 3..7 none (out 96)
    "in160-288-96|pi288|vf96": dict(in0=160, trunk=[(288, "relu"), (96, None)], pi=[(288, "relu")], vf=[(96, "relu")], value=True),
}
MS = (1, 32, 64, 65, 130)   # 32, 64: the last workgroup is full (nrow == 32)


class Layer:
    def __init__(self, wb, bias, act):
        self.wb, self.bias, self.act = np.ascontiguousarray(wb, np.uint16), np.ascontiguousarray(bias, np.float32), act
        self.out, self.in_ = self.wb.shape


class Net:
    """in0; trunk / pi / vf: lists of Layer; action: Layer [60, latent_pi]; value: Layer [1, latent_vf] or None."""

    def hidden(self):
        return self.trunk + self.pi + self.vf

    def tap_cols(self):
        return sum(l.out for l in self.hidden())

    def tap_inputs(self, hb, taps):
        """-> [(layer, its input bits, its tapped output bits)] for the hidden layers in table order, then (action input bits, value input bits): every
        input is hb or a slice of `taps`, the kernel's own outputs."""
        offs, o = [], 0
        for l in self.hidden():
            offs.append((o, o + l.out))
            o += l.out
        piece = lambda k: taps[:, offs[k][0]:offs[k][1]]   # noqa: E731
        nt, npi = len(self.trunk), len(self.pi)
        trunk_out = piece(nt - 1) if nt else hb
        items = []
        for k, l in enumerate(self.hidden()):
            if k < nt:
                x = piece(k - 1) if k else hb
            elif k < nt + npi:
                x = piece(k - 1) if k > nt else trunk_out
            else:
                x = piece(k - 1) if k > nt + npi else trunk_out
            items.append((l, x, piece(k)))
        lat_pi = piece(nt + npi - 1) if npi else trunk_out
        lat_vf = piece(len(offs) - 1) if self.vf else trunk_out
        return items, lat_pi, lat_vf


def layer(xb, l):
    """-> (ref float64 [m, out], bound) of one layer (module docstring)."""
    return layer64(widen(xb), l)


def layer64(x, l):
    """`layer` over float64 activations x (the values, not bfloat16 bits)."""
    w, b = widen(l.wb), l.bias.astype(np.float64)
    s = x @ w.T + b
    bound = 2 * (x.shape[1] + 2) * U * (np.abs(x) @ np.abs(w).T + np.abs(b)) + U * np.abs(s)
    if l.act == "relu":
        return np.maximum(s, 0.0), bound
    if l.act == "tanh":
        return np.tanh(s), bound + TANH_ABS
    return s, bound


def rne_bits(v):
    """float64 -> float32 -> bfloat16 bits, both to nearest even."""
    return to_bf16_bits(np.asarray(v, np.float64).astype(np.float32))


def check_interval(got_bits, ref, bound, what):
    got, lo, hi = widen(got_bits), widen(rne_bits(ref - bound)), widen(rne_bits(ref + bound))
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    assert np.isfinite(got).all(), f"{what}: not finite"
    bad = (got < lo) | (got > hi)
    print(f"{what}: {int((got == widen(rne_bits(ref))).sum())} of {got.size} are the rounding of the reference itself")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {got.size} outside [rne(ref - bound), rne(ref + bound)]; first at {np.argwhere(bad)[0]}"


def check_taps(net, hb, taps, logits, values, what):
    """Every hidden layer's tapped output against its own tapped input; the logits and the values against their bounds."""
    items, lat_pi, lat_vf = net.tap_inputs(hb, taps)
    for k, (l, x, y) in enumerate(items):
        ref, bound = layer(x, l)
        check_interval(y, ref, bound, f"{what}: hidden layer {k} ({l.in_} -> {l.out}, {l.act})")
    ref, bound = layer(lat_pi, net.action)
    check_close(logits, ref, bound, what + ": logits")
    if net.value is not None:
        ref, bound = layer(lat_vf, net.value)
        check_close(values, ref[:, 0], bound[:, 0], what + ": values")


def chain64(net, hb):
    """-> (logits float64 [m, 60], values float64 [m] or None): `layer64` applied layer by layer to float64 activations, NO rounding between the
    layers -- the network itself, which both the kernel and the bfloat16 torch path approximate with one rounding to bfloat16 per layer."""
    x = widen(hb)
    for l in net.trunk:
        x = layer64(x, l)[0]
    p = v = x
    for l in net.pi:
        p = layer64(p, l)[0]
    for l in net.vf:
        v = layer64(v, l)[0]
    return layer64(p, net.action)[0], layer64(v, net.value)[0][:, 0] if net.value is not None else None


# ---------------------------------------------------------------------- the nets
def _build(spec, make):
    n = Net()
    n.in0 = spec["in0"]
    w = n.in0
    n.trunk = []
    for out, act in spec["trunk"]:
        n.trunk.append(make(out, w, act))
        w = out
    n.pi, n.vf = [], []
    wp = wv = w
    for out, act in spec["pi"]:
        n.pi.append(make(out, wp, act))
        wp = out
    for out, act in spec["vf"]:
        n.vf.append(make(out, wv, act))
        wv = out
    n.action = make(UNITS, wp, None)
    n.value = make(1, wv, None) if spec["value"] else None
    return n


def random_net(spec, seed):
    """Weights ~ N(0, 4 / in) rounded to bfloat16, biases ~ N(0, 1): tests/actor_ref.make_case's scaling, layer by layer."""
    rng = np.random.default_rng(seed)
    return _build(spec, lambda out, in_, act: Layer(to_bf16_bits((rng.standard_normal((out, in_)) * 2.0 / np.sqrt(in_)).astype(np.float32)),
                                                    rng.standard_normal(out).astype(np.float32), act))


def random_h(m, in0, seed):
    return to_bf16_bits(np.random.default_rng(seed).standard_normal((m, in0)).astype(np.float32))


def exact_net(spec, seed):
    """Weights in {-1, 0, 1} with at most two non-zeros per row at asymmetric places, biases in {-1, 0, 1, 2}."""
    rng = np.random.default_rng(seed)

    def make(out, in_, act):
        w = np.zeros((out, in_), np.float32)
        for j in range(out):
            for k in rng.choice(in_, size=rng.integers(1, 3), replace=False):
                w[j, k] = rng.choice((-1.0, 1.0))
        return Layer(to_bf16_bits(w), rng.integers(-1, 3, out).astype(np.float32), act)
    return _build(spec, make)


def exact_h(m, in0, seed):
    return to_bf16_bits((np.random.default_rng(seed).random((m, in0)) < 0.5).astype(np.float32))


def exact_forward(net, hb):
    """-> (taps bits [m, tap cols], logits float64 [m, 60], values float64 [m] or None).  Every activation is asserted to be an integer of magnitude
    <= 256: exact in bfloat16, and every partial sum exact in float32 in ANY order, so the kernel's outputs must EQUAL these."""
    def run(x, l):
        y = x @ widen(l.wb).T + l.bias.astype(np.float64)
        assert l.act in (None, "relu")
        y = np.maximum(y, 0.0) if l.act == "relu" else y
        assert (y == np.rint(y)).all() and np.abs(y).max() <= 256, "an exact case left the integers of magnitude <= 256"
        return y
    x = widen(hb)
    outs = []
    for l in net.trunk:
        x = run(x, l)
        outs.append(x)
    p = v = x
    for l in net.pi:
        p = run(p, l)
        outs.append(p)
    for l in net.vf:
        v = run(v, l)
        outs.append(v)
    taps = to_bf16_bits(np.concatenate(outs, 1).astype(np.float32)) if outs else np.zeros((len(hb), 0), np.uint16)
    return taps, run(p, net.action), run(v, net.value)[:, 0] if net.value is not None else None


def to_policy(net, device):
    """The net as a RowPolicy on `device`: float32 parameters that hold the bfloat16 values exactly."""
    import torch
    from balatro_gym_amd import RowActor, RowDense, RowPolicy

    def dense(l, cls=RowDense):
        d = cls(l.in_, l.out, l.act, device=device) if cls is RowDense else cls(l.in_, device=device)
        with torch.no_grad():
            d.weight.copy_(torch.from_numpy(widen(l.wb).astype(np.float32)))
            d.bias.copy_(torch.from_numpy(l.bias))
        return d
    return RowPolicy([dense(l) for l in net.trunk], [dense(l) for l in net.pi], [dense(l) for l in net.vf], dense(net.action, RowActor),
                     dense(net.value) if net.value is not None else None)


# ---------------------------------------------------------------------- the activations at their special values
# One hidden layer 64 -> 64 whose weight is the identity and whose bias is zero: unit j has ONE non-zero product, x[j] * 1, and every other product is
# x[k] * 0.  For finite x those are zeros of either sign, the accumulator starts at +0.0, and a float32 sum of x[j] with zeros is x[j] in any order:
# the pre-activation IS x[j] -- with one exception the contract itself makes: for x[j] = -0.0 the sum (+0.0) + (-0.0) is +0.0 in round-to-nearest, so
# the pre-activation of -0.0 is +0.0.  For a row that holds +-inf or NaN in column c the exact products inf * 0 and NaN * 0 are NaN: every unit but c
# is NaN (0x7fc0 behind bg_ppo_bf16), unit c is x[c] itself.  The action and value layers have zero weights and zero bias: a finite row's logits and
# value are 0.0, a non-finite row's are NaN (tap * 0), and the head answers such a row with action -1 and NaN (bg_head.h, "degenerate").
SPECIAL_FINITE = (0.0, 2.0 ** -126, 1e-3, 0.5, 1.0, 9.0, 44.0, 45.0, 88.0, 3e38)   # and their negatives; +-inf, NaN and the subnormal: rows of their own
SPECIAL_M = 33            # a full workgroup that holds every special row, and one row of a second
SPECIAL_ROWS = {"+inf": (20, 5, 0x7F80), "-inf": (21, 37, 0xFF80), "nan": (22, 11, 0x7FC0)}   # name -> (row, column, bits)
SPECIAL_SUB_ROW = 23      # +2**-130 (bits 0x0008) in column 3, -2**-130 (0x8008) in column 40, +0.0 elsewhere: a bfloat16 subnormal OPERAND
SPECIAL_SUB = ((3, 0x0008), (40, 0x8008))
QNAN = 0x7FC0


def special_case(act):
    """-> dict(net, hb [33, 64] bits, hb_finite (the three non-finite rows replaced by +0.0 rows), lo / hi (bits [33, 64]: the tap must lie in
    [lo, hi]; lo == hi: those bits exactly; QNAN in both: 0x7fc0 exactly), nonfinite (row indices), pairs (the (row, col), (row, col') places that hold
    x and -x for a finite non-zero x).  The expectation is the contract of csrc/bg_policy.h (comment above)."""
    assert act in ACT
    n = Net()
    n.in0 = 64
    n.trunk = [Layer(to_bf16_bits(np.eye(64, dtype=np.float32)), np.zeros(64, np.float32), act)]
    n.pi, n.vf = [], []
    n.action = Layer(np.zeros((UNITS, 64), np.uint16), np.zeros(UNITS, np.float32), None)
    n.value = Layer(np.zeros((1, 64), np.uint16), np.zeros(1, np.float32), None)
    pos = to_bf16_bits(np.array(SPECIAL_FINITE, np.float32))
    table = np.concatenate([pos, pos ^ 0x8000]).astype(np.uint16)   # 20 finite values, -0.0 among them
    assert np.isfinite(widen(table)).all() and len(table) == 20
    r, c = np.meshgrid(np.arange(SPECIAL_M), np.arange(64), indexing="ij")
    hb = table[(r + c) % len(table)]
    for row, col, bits in SPECIAL_ROWS.values():
        hb[row, col] = bits
    hb[SPECIAL_SUB_ROW] = 0
    for col, bits in SPECIAL_SUB:
        hb[SPECIAL_SUB_ROW, col] = bits
    nonfinite = sorted(row for row, _, _ in SPECIAL_ROWS.values())
    hb_finite = hb.copy()
    hb_finite[nonfinite] = 0
    # the expectation, element by element, from the pre-activation y = x (y = +0.0 for x = -0.0)
    y = hb.copy()
    y[y == 0x8000] = 0
    yv = widen(y)
    if act is None:
        lo = hi = y
    elif act == "relu":   # bg_lin_relu: v > 0 ? v : NaN kept : +0.0
        lo = hi = np.where(yv > 0, y, np.where(np.isnan(yv), QNAN, 0)).astype(np.uint16)
    else:
        with np.errstate(invalid="ignore"):
            t = np.tanh(yv)
            lo, hi = rne_bits(t - TANH_ABS), rne_bits(t + TANH_ABS)
        one = np.where(yv < 0, 0xBF80, 0x3F80).astype(np.uint16)
        sat = np.abs(yv) >= 45.0   # e = expf(2 |y|) is +inf from |y| > 44.4 on: r = 1 - 2 / inf = 1 exactly, and at inf
        lo, hi = np.where(sat, one, lo).astype(np.uint16), np.where(sat, one, hi).astype(np.uint16)
        zero = yv == 0   # t = 0, e = 1, r = 1 - 2 / 2 = +0.0 exactly
        lo, hi = np.where(zero, 0, lo).astype(np.uint16), np.where(zero, 0, hi).astype(np.uint16)
    lo, hi = lo.copy(), hi.copy()
    for row, col, bits in SPECIAL_ROWS.values():   # inf * 0 and NaN * 0 are NaN in every unit but `col`; a NaN in `col` stays one
        others = np.arange(64) != col
        lo[row, others] = hi[row, others] = QNAN
        if bits == QNAN:
            lo[row, col] = hi[row, col] = QNAN
    pairs = []
    for row in range(SPECIAL_M):
        if row in nonfinite or row == SPECIAL_SUB_ROW:
            continue
        for col in range(64 - 10):   # table[k] and table[k + 10] = -table[k] stand ten columns apart
            if (row + col) % 20 < 10 and (hb[row, col] & 0x7FFF) != 0:
                assert hb[row, col + 10] == hb[row, col] ^ 0x8000
                pairs.append((row, col, col + 10))
    return dict(net=n, hb=hb, hb_finite=hb_finite, lo=lo, hi=hi, nonfinite=nonfinite, pairs=np.array(pairs), act=act)


def check_special(case, taps, logits, values, actions, log_prob, what):
    """The taps of `special_case` against the contract, bit for bit where it fixes the bits; the logits / values / head of finite and non-finite rows."""
    taps, lo, hi = np.asarray(taps, np.uint16), case["lo"], case["hi"]
    assert taps.shape == lo.shape, f"{what}: shape {taps.shape}"
    exact = lo == hi
    bad = exact & (taps != lo)
    assert not bad.any(), (f"{what}: {int(bad.sum())} taps differ from the bits the contract fixes; first at {np.argwhere(bad)[0]}: "
                           f"got {taps[tuple(np.argwhere(bad)[0])]:#06x}, want {lo[tuple(np.argwhere(bad)[0])]:#06x}")
    with np.errstate(invalid="ignore"):
        g, l, h = widen(taps), widen(lo), widen(hi)
        out = ~exact & ~((g >= l) & (g <= h))
    assert not out.any(), f"{what}: {int(out.sum())} taps outside [rne(tanh - TANH_ABS), rne(tanh + TANH_ABS)]; first at {np.argwhere(out)[0]}"
    if case["act"] != "relu":   # tanh puts the sign of y back on r: an odd function to the bit (so is the identity)
        p = case["pairs"]
        odd = taps[p[:, 0], p[:, 1]] ^ 0x8000 != taps[p[:, 0], p[:, 2]]
        assert len(p) > 400 and not odd.any(), f"{what}: tap(-x) is not tap(x) with the sign flipped at {p[odd][:3]}"
    nf = np.zeros(len(taps), bool)
    nf[case["nonfinite"]] = True
    logits, values = np.asarray(logits), np.asarray(values)
    assert np.isnan(logits[nf]).all() and np.isnan(values[nf]).all(), f"{what}: a non-finite row's logits and value are NaN (tap * 0)"
    assert (logits[~nf] == 0).all() and (values[~nf] == 0).all(), f"{what}: a finite row's logits and value are 0"
    actions, log_prob = np.asarray(actions), np.asarray(log_prob)
    assert (actions[nf] == -1).all() and np.isnan(log_prob[nf]).all(), f"{what}: the head answers NaN logits with -1 and NaN"
    assert ((actions[~nf] >= 0) & (actions[~nf] < UNITS)).all() and np.isfinite(log_prob[~nf]).all()


def pitched(bits, pitch, fill):
    """-> (a [rows, pitch] uint16 array whose first columns are `bits` and whose padding is `fill`, 16-byte aligned; the storage that keeps it alive)."""
    bits = np.asarray(bits, np.uint16)
    storage = np.full(bits.shape[0] * pitch + 8, fill, np.uint16)
    off = (-storage.ctypes.data % 16) // 2
    a = storage[off:off + bits.shape[0] * pitch].reshape(bits.shape[0], pitch)
    a[:, :bits.shape[1]] = bits
    return a, storage
