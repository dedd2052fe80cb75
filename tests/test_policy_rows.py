"""bg_policy_forward (RowPolicy.act / .evaluate) on the MI355X, against tests/policy_ref.py.
  1  the exact cases: taps, logits and values EQUAL the integers, at m in {1, 32, 64, 65, 130} (a partial workgroup, full last workgroups, past two,
     past four); widths that give some waves two tiles and others one or none, k-steps that end inside a batch of 8;
  1a the activations at their special values (+-0, tanh's saturation, +-inf, NaN, a subnormal operand) against the contract, bit for bit;
  1b weights, h, taps and logits at pitches wider than their columns, through the C ABI: the integers, and every padding element keeps its fill;
  2  the reference's topology on random data, h a column slice of a wider tensor: every hidden layer's tapped output inside the interval around the
     float64 value of its own tapped input, logits and values inside their bounds;
  3  the head: actions / log_prob / entropy bit for bit sample_actions / evaluate_actions on the tapped logits, under the masks of real records and
     one all-masked row; deterministic mode returns the first valid maximum;
  4  shape independence: m = 200 in one call against rows [0:70] and [70:200] with index0 = 70, with and without the test outputs; two calls alike;
  5  a collection loop: 256 envs, 20 steps of RowExtractor -> policy.act -> env.step with every layer's bfloat16 copy attached to a RowOptimizer."""
import numpy as np
import pytest

from tests import policy_ref as pr

pytestmark = pytest.mark.gpu

_cache: dict = {}


def _bf16(bits):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits, np.uint16).view(np.int16)).cuda().view(torch.bfloat16)


def _bits(t):
    import torch
    t = t.contiguous()
    return (t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16)).cpu().numpy()


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {int((g != w).sum())} of {w.size} elements differ"


def _u16(t):
    return _bits(t).view(np.uint16)


def _reference():
    """The reference's topology, its policy on the device, 200 rows of h as a column slice (pitch 512 > in0 = 448), real masks with row 3 all-masked,
    and ONE call with every output: shared by tests 2, 3 and 4."""
    if "ref" not in _cache:
        import torch
        from tests.test_policy_head import _records
        net = pr.random_net(pr.REFERENCE, 3)
        policy = pr.to_policy(net, "cuda")
        m = 200
        hb = pr.random_h(m, net.in0, 4)
        wide = torch.full((m, 512), float("nan"), dtype=torch.bfloat16, device="cuda")
        h = wide[:, 32:32 + net.in0]
        h.copy_(_bf16(hb))
        rows = _records()[384][:m].clone()
        rows[3, 176:236] = 0
        mask = rows.cpu().numpy()[:, 176:236].view(np.int8).copy()
        assert (mask[3] == 0).all() and (mask != 0).any(1).sum() == m - 1
        out = policy.act(h, rows, seed=77, t=5, index0=1000, entropy=True, taps=True)
        _cache["ref"] = dict(net=net, policy=policy, hb=hb, h=h, rows=rows, mask=mask, out=out, m=m)
    return _cache["ref"]


@pytest.mark.parametrize("name", list(pr.EXACT))
def test_exact_cases_equal_the_integers(name):
    net = pr.exact_net(pr.EXACT[name], 11)
    policy = pr.to_policy(net, "cuda")
    for m in pr.MS:
        hb = pr.exact_h(m, net.in0, 5 + m)
        taps, logits, values = pr.exact_forward(net, hb)
        a, lp, v, _, tp, lg = policy.act(_bf16(hb), seed=1, t=m, taps=True)
        assert np.array_equal(_u16(tp), taps), f"{name} m {m}: taps"
        assert np.array_equal(lg.cpu().numpy().astype(np.float64), logits), f"{name} m {m}: logits"
        if values is None:
            assert v is None
        else:
            assert np.array_equal(v.cpu().numpy().astype(np.float64), values), f"{name} m {m}: values"
        assert ((a >= 0) & (a < 60)).all() and bool(lp.isfinite().all())


@pytest.mark.parametrize("act", ["tanh", "relu", None])
def test_activations_at_their_special_values(act):
    """policy_ref.special_case through an identity layer: +-0, the smallest normal, tanh's saturation (0x3f80 / 0xbf80 from |x| >= 45 on and at inf),
    tanh odd to the bit, +-inf and NaN in rows of their own (inf * 0 is NaN in every other unit of the row), one row with a bfloat16 SUBNORMAL operand
    (+-2**-130), whose tap the contract says is the operand itself under none / relu; and the finite rows of the same 32-row workgroup do not notice
    the non-finite rows beside them: every output bit for bit the run without them."""
    c = pr.special_case(act)
    policy = pr.to_policy(c["net"], "cuda")
    kw = dict(seed=3, t=1, entropy=True, taps=True)
    a, lp, v, en, tp, lg = policy.act(_bf16(c["hb"]), **kw)
    sub = _u16(tp)[pr.SPECIAL_SUB_ROW]
    print(f"{act}: the subnormal operands' taps {[f'{int(sub[col]):#06x}' for col, _ in pr.SPECIAL_SUB]} (operands {[f'{b:#06x}' for _, b in pr.SPECIAL_SUB]})")
    pr.check_special(c, _u16(tp), lg.cpu().numpy(), v.cpu().numpy(), a.cpu().numpy(), lp.cpu().numpy(), f"special values, {act}")
    assert bool(en[c["nonfinite"]].isnan().all())
    q = policy.act(_bf16(c["hb_finite"]), **kw)
    keep = np.setdiff1d(np.arange(pr.SPECIAL_M), c["nonfinite"])
    for k, name in enumerate(("actions", "log_prob", "values", "entropy", "taps", "logits")):
        g, w = _bits((a, lp, v, en, tp, lg)[k])[keep], _bits(q[k])[keep]
        assert np.array_equal(g, w), f"{act}: {name} of the finite rows beside the non-finite ones"
    assert bool(q[5].isfinite().all()) and bool((q[0] >= 0).all())


def test_pitched_weights_taps_and_logits_through_the_c_abi():
    """wpitch > in, h_stride > in0, taps_stride > tap cols, logits_out_stride > 60: the exact case 64-32|pi32|novf at m = 33 equals the integers, and
    every padding element and every element behind row m keeps its fill (the weights' and h's padding is NaN: a read of it would show)."""
    import torch
    from balatro_gym_amd import _native as nat
    from balatro_gym_amd.policy import _NET
    net, m = pr.exact_net(pr.EXACT["64-32|pi32|novf"], 11), 33
    hb = pr.exact_h(m, net.in0, 5 + m)
    taps, logits, values = pr.exact_forward(net, hb)
    tcols = net.tap_cols()
    assert values is None and tcols == 64
    nan, dev = float("nan"), "cuda"

    def pitched(bits, pitch):
        t = torch.full((bits.shape[0], pitch), nan, dtype=torch.bfloat16, device=dev)
        t[:, :bits.shape[1]] = _bf16(bits)
        return t
    t = np.zeros(1, _NET)
    n, keep = t[0], []
    n["n_trunk"], n["n_pi"], n["n_vf"], n["has_value"], n["in0"] = 1, 1, 0, 0, net.in0
    for k, l in enumerate(net.hidden() + [net.action]):
        w, b = pitched(l.wb, l.in_ + 8), torch.from_numpy(l.bias).to(dev)
        keep += [w, b]
        e = n["layer"][k]
        e["weight"], e["bias"], e["pitch"], e["in"], e["out"], e["act"] = w.data_ptr(), b.data_ptr(), l.in_ + 8, l.in_, l.out, pr.ACT[l.act]
    L = nat.load()
    assert L.bg_policy_check(t.ctypes.data) == 0 and L.bg_policy_tap_cols(t.ctypes.data) == tcols
    h = pitched(hb, net.in0 + 8)
    TS, LS, FILL = tcols + 8, 64, 0x7B7B
    tp = torch.full((m + 2, TS), FILL, dtype=torch.int16, device=dev)
    lg = torch.full((m + 2, LS), -777.0, device=dev)
    a = torch.full((m + 2,), 123, dtype=torch.int32, device=dev)
    lp, en = torch.full((m + 2,), -777.0, device=dev), torch.full((m + 2,), -777.0, device=dev)
    rc = L.bg_policy_forward(t.ctypes.data, h.data_ptr(), net.in0 + 8, None, 0, m, 0, 1, 0, m, a.data_ptr(), lp.data_ptr(), en.data_ptr(), None, tp.data_ptr(), TS,
                             lg.data_ptr(), LS, None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.bg_last_error(None)
    torch.cuda.synchronize()
    tpn, lgn = tp.cpu().numpy().view(np.uint16), lg.cpu().numpy()
    assert np.array_equal(tpn[:m, :tcols], taps), "taps at a pitch"
    assert np.array_equal(lgn[:m, :60].astype(np.float64), logits), "logits at a pitch"
    assert (tpn[:m, tcols:] == FILL).all() and (tpn[m:] == FILL).all(), "the taps' padding and the rows behind m keep their fill"
    assert (lgn[:m, 60:] == -777.0).all() and (lgn[m:] == -777.0).all(), "the logits' padding and the rows behind m keep their fill"
    assert bool((a[m:] == 123).all()) and bool((lp[m:] == -777.0).all()) and bool((en[m:] == -777.0).all()), "nothing is written behind row m"
    # the other outputs are those of the dense call on the same net
    wa, wlp, _, wen = pr.to_policy(net, dev).act(_bf16(hb), seed=1, t=m, entropy=True)
    _same(a[:m], wa, "actions"); _same(lp[:m], wlp, "log_prob"); _same(en[:m], wen, "entropy")
    assert bool(((wa >= 0) & (wa < 60)).all()) and bool(wlp.isfinite().all())


def test_reference_topology_is_inside_the_per_layer_intervals():
    r = _reference()
    n = 130
    a, lp, v, en, taps, logits = r["policy"].act(r["h"][:n], r["rows"][:n], seed=77, t=5, index0=1000, entropy=True, taps=True)
    pr.check_taps(r["net"], r["hb"][:n], _u16(taps), logits.cpu().numpy(), v.cpu().numpy(), "reference topology, m 130")
    assert tuple(taps.shape) == (n, r["net"].tap_cols()) and r["h"].stride(0) == 512 and r["net"].in0 == 448


def test_head_is_the_masked_head_on_the_tapped_logits():
    import torch
    from balatro_gym_amd import evaluate_actions, sample_actions
    r = _reference()
    policy, h, rows, mask = r["policy"], r["h"], r["rows"], r["mask"]
    a, lp, v, en, taps, logits = r["out"]
    wa, wlp, wen = sample_actions(logits, rows, seed=77, t=5, index0=1000)
    _same(a, wa, "actions"); _same(lp, wlp, "log_prob"); _same(en, wen, "entropy")
    assert int(a[3]) == -1 and bool(lp[3].isnan()) and bool(en[3].isnan()), "an all-masked row: -1, NaN"
    live = np.arange(r["m"]) != 3
    an = a.cpu().numpy()
    assert (mask[live, an[live]] != 0).all()
    # the same masks as a dense int8 matrix
    dense = torch.from_numpy(mask).cuda()
    a2, lp2, _, en2 = policy.act(h, dense, seed=77, t=5, index0=1000, entropy=True)
    _same(a2, a, "actions, int8 mask"); _same(lp2, lp, "log_prob, int8 mask"); _same(en2, en, "entropy, int8 mask")
    # deterministic: the first valid maximum
    ad, lpd, _, _ = policy.act(h, rows, seed=0, t=0, deterministic=True)
    wad, wlpd, _ = sample_actions(logits, rows, seed=0, t=0, deterministic=True)
    _same(ad, wad, "deterministic actions"); _same(lpd, wlpd, "deterministic log_prob")
    z = np.where(mask != 0, logits.cpu().numpy(), -np.inf)
    assert np.array_equal(ad.cpu().numpy()[live], z.argmax(1)[live])
    # evaluate: the given actions (one out of range, one masked)
    given = a.clone()
    given[9] = 60
    masked = int(np.flatnonzero(mask[5] == 0)[0])
    given[5] = masked
    elp, een, ev = policy.evaluate(h, given, rows)
    wlp2, wen2 = evaluate_actions(logits, given, rows)
    _same(elp, wlp2, "evaluate log_prob"); _same(een, wen2, "evaluate entropy"); _same(ev, v, "evaluate values")
    assert bool(elp[9].isnan()) and float(elp[5]) == -np.inf
    # no mask: every action valid
    a3, lp3, _, _ = policy.act(h, seed=4, t=2)
    wa3, wlp3, _ = sample_actions(logits, seed=4, t=2)
    _same(a3, wa3, "actions, no mask"); _same(lp3, wlp3, "log_prob, no mask")


def test_rows_do_not_depend_on_the_call_around_them():
    r = _reference()
    policy, h, rows = r["policy"], r["h"], r["rows"]
    kw = dict(seed=77, t=5, entropy=True)
    whole = r["out"]
    again = policy.act(h, rows, index0=1000, taps=True, **kw)
    lo = policy.act(h[:70], rows[:70], index0=1000, taps=True, **kw)
    hi = policy.act(h[70:], rows[70:], index0=1070, taps=True, **kw)
    import torch
    for k, name in enumerate(("actions", "log_prob", "values", "entropy", "taps", "logits")):
        _same(again[k], whole[k], name + ": two calls")
        _same(torch.cat([lo[k], hi[k]]), whole[k], name + ": [0:70] + [70:200]")
    plain = policy.act(h, rows, index0=1000, **kw)
    lo = policy.act(h[:70], rows[:70], index0=1000, **kw)
    hi = policy.act(h[70:], rows[70:], index0=1070, **kw)
    for k, name in enumerate(("actions", "log_prob", "values", "entropy")):
        _same(plain[k], whole[k], name + ": without the test outputs")
        _same(torch.cat([lo[k], hi[k]]), whole[k], name + ": [0:70] + [70:200] without the test outputs")


def test_refusals_are_bg_e_arg_with_the_call_s_name():
    import ctypes as C

    import torch
    from balatro_gym_amd import _native as nat
    r = _reference()
    policy = r["policy"]
    L = nat.load()
    net = policy._net().copy()
    assert L.bg_policy_check(net.ctypes.data) == 0 and L.bg_policy_tap_cols(net.ctypes.data) == policy.tap_cols
    bad = net.copy()
    bad[0]["layer"][1]["in"] = 256
    assert L.bg_policy_check(bad.ctypes.data) == -1 and b"bg_policy_check: a layer's in_features" in L.bg_last_error(None)
    m = 8
    h = torch.zeros((m, 448), dtype=torch.bfloat16, device="cuda")
    a = torch.full((m,), 123, dtype=torch.int32, device="cuda")
    lp = torch.full((m,), -777.0, device="cuda")
    call = lambda t, hp, pitch, flags, lp_ptr: L.bg_policy_forward(t.ctypes.data, hp, pitch, None, 0, m, flags, 1, 0, 0, a.data_ptr(), lp_ptr, None, None, None, 0, None, 0,   # noqa: E731
                                                                  None, torch.cuda.current_stream().cuda_stream)
    for args, text in (((bad, h.data_ptr(), 448, 0, lp.data_ptr()), b"in_features"), ((net, h.data_ptr() + 2, 448, 0, lp.data_ptr()), b"h_dev"),
                       ((net, h.data_ptr(), 444, 0, lp.data_ptr()), b"h_stride_elems"), ((net, h.data_ptr(), 448, 4, lp.data_ptr()), b"flags"),
                       ((net, h.data_ptr(), 448, 3, lp.data_ptr()), b"flags"), ((net, h.data_ptr(), 448, 0, a.data_ptr()), b"same pointer")):
        assert call(*args) == -1
        msg = L.bg_last_error(None)
        assert msg.startswith(b"bg_policy_forward: ") and text in msg, msg
    torch.cuda.synchronize()
    assert bool((a == 123).all()) and bool((lp == -777.0).all()), "a refused call writes nothing"
    assert call(net, h.data_ptr(), 448, 0, lp.data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool(((a >= 0) & (a < 60)).all()) and bool(lp.isfinite().all())
    assert C.sizeof(C.c_void_p) == 8


def test_collection_loop_over_records():
    """RowExtractor -> policy.act -> env.step: every action is valid under the live mask, no reward is the -1.0 invalid-action penalty, values are finite;
    the layers read the bfloat16 copies a RowOptimizer keeps.  The penalty is told by the step's info: error 1 (oracle/balatro_oracle.h,
    BO_ERR_INVALID_ACTION).  A reward of -1.0 is also what a boss blind answers a valid play it refuses with (errors 2..5) and a shop action that
    cannot be paid for or placed (6..8): every -1.0 must carry one of those, never error 0 or 1."""
    import torch
    from balatro_gym_amd import BalatroVecEnv, RowExtractor, RowOptimizer, RowPolicy
    torch.manual_seed(0)
    nn = torch.nn
    n, K = 256, 20
    ext = RowExtractor.from_linears(nn.Linear(416, 256), nn.Linear(10, 128), nn.Linear(21, 64)).cuda()
    second = RowPolicy.stack_blocks([nn.Linear(256, 128), nn.Linear(128, 64), nn.Linear(64, 32)], "relu")
    policy = RowPolicy.from_modules(trunk=[(nn.Linear(224, 512), "relu"), (nn.Linear(512, 512), "relu")], pi=[(nn.Linear(512, 256), "tanh"), (nn.Linear(256, 256), "tanh")],
                                    vf=[(nn.Linear(512, 256), "tanh"), (nn.Linear(256, 256), "tanh")], action_net=nn.Linear(256, 60), value_net=nn.Linear(256, 1))
    policy = RowPolicy([second] + list(policy.trunk), list(policy.pi), list(policy.vf), policy.action, policy.value).cuda()
    opt = RowOptimizer(list(ext.parameters()) + list(policy.parameters()))
    opt.attach(ext)
    opt.attach(policy)
    env = BalatroVecEnv(n, [7000 + i for i in range(n)], scorer_jokers=True, autoreset=True, obs_layout="rows")
    try:
        for t in range(K):
            rows = env.obs_rows
            mask = rows[:, 176:236].clone()
            with torch.no_grad():
                h = ext(rows)
            a, lp, v, _ = policy.act(h, rows, seed=9, t=t)
            assert policy._table_key is not None, "every layer reads its attached copy: the table is built once"
            assert bool(((a >= 0) & (a < 60)).all()) and bool((mask.gather(1, a.long()[:, None]) != 0).all()), f"step {t}: an action outside the mask"
            assert bool(v.isfinite().all()) and bool(lp.isfinite().all())
            _, reward, _, _, info = env.step(a)
            err = info["error"]
            assert not bool((err == 1).any()), f"step {t}: a step was answered with the invalid-action penalty"
            assert bool((err[reward == -1.0] > 1).all()), f"step {t}: a reward of -1.0 that no refusal of a VALID action explains"
        env.check()
    finally:
        env.close()
