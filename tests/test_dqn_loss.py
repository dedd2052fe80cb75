"""bg_dqn_loss, bg_sample_actions_eps and RowReplay on the MI355X: every load and store path of the loss kernel (q, q_next, q_next_online and dq
float32 / bfloat16, dense, at stride 64, from offset pointers; records the product wrote at stride 352 and 384 with hand-made fields written over them)
at sizes on each side of the workgroup's 64 rows and one with more workgroup partials than the finishing workgroup has lanes.  Everything is copied to
the host and held to tests/dqn_ref.py exactly as on the CPU (never to torch arithmetic on the GPU): dq, td, the excluded rows and their count bit for
bit on every row, the scalars within 2**-24 * |ref| + 2**-50 * (sum of |terms|).  Outputs sit between poisoned guards, padding columns and inputs stay
unwritten, two calls give the same bits, the bf16 gradient is the float32 call's rounded to nearest even, bad arguments are BG_E_ARG before any launch,
m == 0 zeroes the stats.  bg_sample_actions_eps is bit for bit the Python-integer restatement at the head test's sizes and mask kinds, whatever m or
index0.  Then end to end: a 256-env handle, a RowReplay of 6 slots that wraps, epsilon-greedy actions, encode_rows(index=) into a two-layer MLP and
its target copy, dqn_loss, backward and one SGD step against the float64 twin.

Largest observed share of a scalar bound on the MI355X: 0.98 (the final rounding to float32 alone can use all of 2**-24 * |ref|).  End to end: the largest
share of a propagated parameter-gradient bound 0.011; (a) against (b) there: td 0.34, dq 0.28, loss 0.014."""
import ctypes as C

import numpy as np
import pytest

from tests import dqn_ref, head_ref

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 65, 257, 4133)
BIG = 256 * 64 + 64 + 1   # 258 workgroup partials: the finishing workgroup's lanes fold two each
LAYOUTS = ("f32", "f32_s64", "f32_off4", "bf16", "bf16_s64", "bf16_off4", "bf16_off2")
GAMMA = 0.99
CONFIGS = [(f | l | dqn_ref.TIMEOUT_EXCLUDE * tmo, dbl, rew) for f in (dqn_ref.MASK_NEXT, 0) for l in (0, dqn_ref.MSE) for dbl in (False, True)
           for tmo, rew in ((1, False), (0, True))]
POISON = -1234.5

_cache: dict = {}
_worst = [0.0]


def _records_host(stride):
    key = ("rec", stride)
    if key not in _cache:
        from tests.test_policy_head import _records
        _cache[key] = _records()[stride].cpu().numpy()
    return _cache[key]


def _case(m, stride, bf16):
    key = ("case", m, stride, bf16)
    if key not in _cache:
        sigma = head_ref.SIGMAS[(m + stride // 32) % 4]
        _cache[key] = dqn_ref.synthetic(m * 5 + stride + bf16, m, sigma, bf16=bf16, stride=stride, base_rows=_records_host(stride))
    return _cache[key]


class _Call:
    """One bg_dqn_loss call through the C ABI with every output between poisoned guards; `.run()` launches, `.fetch()` copies back and checks the guards
    and that no input was written."""

    def __init__(self, c, layout, flags, double, rew, out_kind=None, with_td=True):
        import torch
        from balatro_gym_amd import _native as nat
        from tests.test_ppo_loss import _place
        self.L = nat.load()
        self.c, self.m, self.flags = c, c.m, flags
        self.bf16 = layout.startswith("bf16")
        kind = layout.split("_")[1] if "_" in layout else "dense"
        self.ins = {}
        for name, host in (("q", c.q), ("qn", c.q_next), ("qo", c.q_online if double else None)):
            self.ins[name] = None if host is None else _place(host, kind, self.bf16)
        self.dfill = POISON if not self.bf16 else -1232.0
        self.dflat, self.dview, self.doff, self.dstride = _place(None, out_kind or kind, self.bf16, poison=(self.dfill, c.m))
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
        self.rows, self.nx, self.rw = dev(c.rows), dev(c.next_index), dev(c.rewards) if rew else None
        assert self.rows.data_ptr() % 16 == 0
        self.before = {k: v[0].clone() for k, v in self.ins.items() if v is not None}
        self.before.update(rows=self.rows.clone(), nx=self.nx.clone(), rw=None if self.rw is None else self.rw.clone())
        g = lambda n: torch.full((n + 2,), POISON, dtype=torch.float32, device="cuda")   # noqa: E731
        self.td, self.stats = g(c.m) if with_td else None, g(8)
        need = int(self.L.bg_dqn_loss_workspace_bytes(C.c_int64(c.m)))
        self.need = need
        self.ws = torch.zeros(need + 32, dtype=torch.uint8, device="cuda")

    def run(self, **over):
        import torch
        vp = C.c_void_p
        p = lambda t, o=0: None if t is None else t.data_ptr() + o   # noqa: E731
        mat = lambda v: (None, 60) if v is None else (p(v[1]), v[3])   # noqa: E731
        (q, qs), (qn, ns), (qo, os_) = mat(self.ins["q"]), mat(self.ins["qn"]), mat(self.ins["qo"])
        a = dict(q=q, qs=qs, qn=qn, ns=ns, qo=qo, os=os_, dt=1 if self.bf16 else 0, rows=p(self.rows), rs=self.c.stride, store=self.c.store_rows, nx=p(self.nx),
                 rw=p(self.rw), m=self.m, gamma=GAMMA, flags=self.flags, dq=p(self.dview), ds=self.dstride, td=p(self.td, 4), stats=p(self.stats, 4), ws=p(self.ws),
                 wsb=self.need)
        a.update(over)
        return self.L.bg_dqn_loss(vp(a["q"]), C.c_uint64(a["qs"]), vp(a["qn"]), C.c_uint64(a["ns"]), vp(a["qo"]), C.c_uint64(a["os"]), a["dt"], vp(a["rows"]),
                                  C.c_uint64(a["rs"]), C.c_int64(a["store"]), vp(a["nx"]), vp(a["rw"]), C.c_int64(a["m"]), C.c_float(a["gamma"]),
                                  C.c_uint32(a["flags"]), vp(a["dq"]), C.c_uint64(a["ds"]), vp(a["td"]), vp(a["stats"]), vp(a["ws"]), C.c_uint64(a["wsb"]), None,
                                  vp(torch.cuda.current_stream().cuda_stream))

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return bool((self.dflat == self.dfill).all()) and bool((self.stats == POISON).all()) and (self.td is None or bool((self.td == POISON).all()))

    def fetch(self):
        """-> (dq [m, 60] float32 or bf16 bits, td or None, stats) on the host"""
        import torch
        from tests.test_ppo_loss import _outside_untouched
        torch.cuda.synchronize()
        assert _outside_untouched(self.dflat, self.doff, self.m, self.dstride, self.dfill), "dq: a guard or a padding column was written"
        for k, t in (("td", self.td), ("stats", self.stats)):
            assert t is None or (float(t[0]) == POISON and float(t[-1]) == POISON), f"{k}: a guard element was written"
        for k, v in self.ins.items():
            assert v is None or torch.equal(v[0].view(torch.int16), self.before[k].view(torch.int16)), f"input {k} was written"
        assert torch.equal(self.rows, self.before["rows"]) and torch.equal(self.nx, self.before["nx"]), "the records or the index were written"
        assert self.rw is None or torch.equal(self.rw.view(torch.int32), self.before["rw"].view(torch.int32))
        dq = self.dview.contiguous()
        dq = dq.view(torch.int16).cpu().numpy().view(np.uint16) if self.bf16 else dq.cpu().numpy()
        h = lambda t: None if t is None else t[1:-1].cpu().numpy()   # noqa: E731
        return dq, h(self.td), h(self.stats)


def _check_one(layout, stride, m, flags, double, rew, twice=False):
    bf16 = layout.startswith("bf16")
    c = _case(m, stride, bf16)
    what = f"{layout} / stride {stride} / m {m} / flags {flags} / double {double} / rewards {rew}"
    call = _Call(c, layout, flags, double, rew)
    assert call.run() == 0, call.L.bg_last_error(None)
    first = call.fetch()
    dq, td, st = first
    if bf16:   # the float32 call on the same (bf16-representable) values: its gradient rounded to nearest even is the bf16 call's, bit for bit
        f32 = _Call(c, "f32" + layout[4:].replace("_off2", "_off4"), flags, double, rew)
        assert f32.run() == 0
        dq32, td32, st32 = f32.fetch()
        assert np.array_equal(dq, head_ref.bf16_bits(dq32)), what + ": bf16 dq is not the rounding of the float32 call's"
        assert np.array_equal(td.view(np.uint32), td32.view(np.uint32)) and np.array_equal(st.view(np.uint32), st32.view(np.uint32)), what
        dq = dq32
    ct = dqn_ref.Contract(c, GAMMA, flags, double, rew)
    _worst[0] = max(_worst[0], ct.check(dq, td, st, what))
    if twice:
        again = _Call(c, layout, flags, double, rew)
        assert again.run() == 0
        for x, y in zip(first, again.fetch()):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), what + ": two calls differ"
    return ct, (dq, td, st)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_path_and_size(layout):
    """Both record strides at every size, the configuration (mask, loss, plain / double, timeout flag, reward source) rotating so that every one occurs
    with every layout.  The 4 133-row calls run twice and must give equal bits."""
    n = LAYOUTS.index(layout)
    for stride in (352, 384):
        for m in SIZES:
            flags, double, rew = CONFIGS[n % len(CONFIGS)]
            ct, _ = _check_one(layout, stride, m, flags, double, rew, twice=m == 4133)
            assert m <= dqn_ref.HAND_ROWS or ct.excluded.sum() >= 8
            n += 3
    print(f"{layout}: largest share of a scalar bound so far {_worst[0]:.3f}")


@pytest.mark.parametrize("layout", ["f32", "bf16"])
def test_more_partials_than_the_finishing_workgroup_has_lanes(layout):
    for flags, double, rew in ((5, True, False), (0, False, True)):
        ct, (dq, td, st) = _check_one(layout, 384, BIG, flags, double, rew, twice=True)
        assert st[7] == BIG and st[6] == ct.excluded.sum() > 0
    print(f"{layout}: largest share of a scalar bound so far {_worst[0]:.3f}")


def test_every_configuration_on_the_hand_made_rows():
    """All sixteen configurations at m = 257 (the hand-made rows in the fifth workgroup, one row), dense float32."""
    for flags, double, rew in CONFIGS:
        _check_one("f32", 384, 257, flags, double, rew)


def test_output_layout_is_independent_of_the_input_layout():
    base = {}
    for lin, lout in (("f32", "dense"), ("f32", "s64"), ("f32", "off4"), ("f32_s64", "dense"), ("f32_off4", "s64"), ("bf16", "off2"), ("bf16_off2", "dense"),
                      ("bf16", "s64"), ("bf16_s64", "off4")):
        bf16 = lin.startswith("bf16")
        call = _Call(_case(257, 384, bf16), lin, 5, True, False, out_kind=lout)
        assert call.run() == 0
        got = call.fetch()
        base.setdefault(bf16, got)
        for x, y in zip(base[bf16], got):
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (lin, lout)


def test_nullable_arguments_refused_arguments_and_m_zero():
    """td_dev may be NULL; every bad argument is BG_E_ARG with its text, before any launch (poison untouched); m == 0 writes zeros to stats only."""
    import torch
    c = _case(257, 384, False)
    full = _Call(c, "f32", 5, True, True)
    assert full.run() == 0
    want = full.fetch()
    notd = _Call(c, "f32", 5, True, True, with_td=False)
    assert notd.run() == 0
    got = notd.fetch()
    assert got[1] is None and np.array_equal(want[0].view(np.uint32), got[0].view(np.uint32)) and np.array_equal(want[2].view(np.uint32), got[2].view(np.uint32))
    call = _Call(c, "f32", 5, True, True)
    L = call.L
    p = lambda t, o=0: t.data_ptr() + o   # noqa: E731
    q, qn, qo, dq, st, ws, td = (p(call.ins["q"][1]), p(call.ins["qn"][1]), p(call.ins["qo"][1]), p(call.dview), p(call.stats, 4), p(call.ws), p(call.td, 4))
    need = call.need
    assert dq % 16 == 0 and need == 5 * 56
    inf, nan = float("inf"), float("nan")
    bad = [dict(q=0), dict(qn=0), dict(dq=0), dict(dt=2), dict(dt=-1), dict(qs=59), dict(ns=59), dict(os=59), dict(ds=59), dict(q=q + 2), dict(qn=qn + 1),
           dict(qo=qo + 2), dict(dq=dq + 2), dict(dt=1, q=q + 1), dict(dt=1, dq=dq + 1), dict(m=-1), dict(m=64 * 0x7fffffff + 1), dict(rows=0),
           dict(rows=p(call.rows, 8)), dict(rs=336), dict(rs=360), dict(rs=0), dict(store=-1), dict(store=2 ** 31), dict(nx=0), dict(nx=p(call.nx, 2)),
           dict(rw=p(call.rw, 2)), dict(td=td + 1), dict(stats=0), dict(stats=st + 2), dict(gamma=-0.01), dict(gamma=1.01), dict(gamma=nan), dict(gamma=inf),
           dict(gamma=-inf), dict(flags=8), dict(flags=0x80000001), dict(ws=0), dict(ws=ws + 8), dict(wsb=need - 1), dict(wsb=0),
           # aliasing: an output on an input, an output on another output
           dict(dq=q), dict(dq=qn), dict(dq=qo), dict(td=p(call.rw)), dict(td=p(call.nx)), dict(stats=p(call.rw)), dict(dq=p(call.rows)), dict(ws=dq),
           dict(td=st), dict(stats=td), dict(ws=p(call.rows))]
    for kw in bad:
        assert call.run(**kw) == -1, kw
        text = L.bg_last_error(None).decode()
        assert text.startswith("bg_dqn_loss: "), (kw, text)
    assert call.untouched(), "a refused call wrote an output"
    assert call.run(m=0, ws=0, wsb=0) == 0
    torch.cuda.synchronize()
    assert (call.stats[1:-1] == 0).all() and float(call.stats[0]) == POISON and float(call.stats[-1]) == POISON
    assert bool((call.dflat == call.dfill).all()) and bool((call.td == POISON).all())
    assert call.run() == 0
    for x, y in zip(want, call.fetch()):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_python_surface_shapes_timing_autograd_and_workspace_cache():
    """dqn_loss: leading shapes, a [C, N, stride] store, timing, DqnStats' scalar views, the cached workspace, an empty batch; q as an autograd leaf:
    loss.backward() leaves q.grad equal to stats.dq, a scaled loss scales it, without grad the loss carries no node."""
    import torch
    from balatro_gym_amd import dqn_loss, vec_env
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    for bf16 in (False, True):
        c = _case(300, 384, bf16)
        dt = torch.bfloat16 if bf16 else torch.float32
        assert c.store_rows == 303
        q, qn, qo, rows, nx, rw = t(c.q).to(dt), t(c.q_next).to(dt), t(c.q_online).to(dt), t(c.rows), t(c.next_index), t(c.rewards)
        for kw, flags, double, rew in ((dict(), 5, False, False), (dict(q_next_online=qo, rewards=rw, mask_next=False, loss="mse", timeouts="terminal"), 2, True, True),
                                       (dict(q_next_online=qo, loss="huber"), 5, True, False)):
            ct = dqn_ref.Contract(c, GAMMA, flags, double, rew)
            loss, st = dqn_loss(q, qn, rows, nx, gamma=GAMMA, **kw)
            dq = st.dq.float().cpu().numpy()
            if bf16:
                assert st.dq.dtype == torch.bfloat16 and np.array_equal(head_ref.bf16_bits(dq), head_ref.bf16_bits(ct.dq))
                ct.check(ct.dq, st.td.cpu().numpy(), st.raw.cpu().numpy(), "python bf16")
            else:
                ct.check(dq, st.td.cpu().numpy(), st.raw.cpu().numpy(), "python")
            assert loss.dim() == 0 and loss.dtype == torch.float32 and not loss.requires_grad and float(loss) == float(st.raw[0]) and st.kernel_ms is None
            for k, name in enumerate(dqn_ref.STATS):
                assert getattr(st, name).dim() == 0 and float(getattr(st, name)) == float(st.raw[k])
        # leading shapes [3, 100], the store as [3, 101, stride]
        l3, s3 = dqn_loss(q.view(3, 100, 60), qn.view(3, 100, 60), rows.view(3, 101, 384), nx.view(3, 100), gamma=GAMMA, timing=True)
        l1, s1 = dqn_loss(q, qn, rows, nx, gamma=GAMMA)
        assert torch.equal(s3.raw.view(torch.int32), s1.raw.view(torch.int32)) and tuple(s3.dq.shape) == (3, 100, 60) and tuple(s3.td.shape) == (3, 100)
        assert torch.equal(s3.dq.reshape(-1, 60).float(), s1.dq.float()) and s3.kernel_ms > 0.0
        before = dict(vec_env._dqn_workspaces)
        dqn_loss(q, qn, rows, nx)
        assert dict(vec_env._dqn_workspaces).keys() == before.keys() and all(vec_env._dqn_workspaces[k] is before[k] for k in before)
        e, se = dqn_loss(q[:0], qn[:0], rows, nx[:0])
        assert float(e) == 0.0 and tuple(se.dq.shape) == (0, 60) and (se.raw == 0).all()
        # autograd
        bits = torch.int16 if bf16 else torch.int32
        ql = q.clone().requires_grad_(True)
        loss, st = dqn_loss(ql, qn, rows, nx, q_next_online=qo, gamma=GAMMA)
        assert loss.requires_grad and loss.grad_fn is not None and float(loss.detach()) == float(st.loss)
        loss.backward()
        assert ql.grad.dtype == dt and torch.equal(ql.grad.view(bits), st.dq.view(bits)) and float(st.dq.float().abs().sum()) > 0.0
        ql2 = q.clone().requires_grad_(True)
        loss2, st2 = dqn_loss(ql2, qn, rows, nx, q_next_online=qo, gamma=GAMMA)
        (3.0 * loss2).backward()
        assert torch.equal(ql2.grad.view(bits), (st2.dq.float() * 3.0).to(dt).view(bits))
        with torch.no_grad():
            loss3, _ = dqn_loss(ql, qn, rows, nx, q_next_online=qo, gamma=GAMMA)
        assert not loss3.requires_grad and float(loss3) == float(loss.detach())


# ---------------------------------------------------------------- epsilon-greedy

def _eps_reference(bf16, mkind, eps):
    from tests import test_policy_head as th
    key = ("eps", bf16, mkind, eps)
    if key not in _cache:
        mk = th._mask(mkind)[1]
        _cache[key] = dqn_ref.eps_actions(th._logits_host(bf16), mk, th.SEED, th.INDEX0, th.T, eps)
    return _cache[key]


def _eps_call(lg, mk, m, eps, a0=0):
    import torch
    from balatro_gym_amd import sample_actions
    from tests import test_policy_head as th
    lgs, mks = lg[a0:a0 + m], None if mk is None else mk[a0:a0 + m]
    buf = torch.full((m + 2,), th.POISON_I, dtype=torch.int32, device="cuda")
    out = buf[1:m + 1]
    before = lgs.clone()
    res = sample_actions(lgs, mks, seed=th.SEED, t=th.T, index0=th.INDEX0 + a0, epsilon=eps, actions=out)
    assert res[0] is out and res[1] is None and res[2] is None
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert h[0] == th.POISON_I and h[-1] == th.POISON_I, "a guard element was written"
    bits = torch.int16 if lgs.dtype == torch.bfloat16 else torch.int32
    assert torch.equal(lgs.view(bits), before.view(bits))
    return h[1:-1].copy()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_epsilon_greedy_every_load_path_and_size(layout):
    """The head test's logit layouts, mask kinds and sizes at epsilon 0.5: every row is the restatement's, which is computed once over the 4 133-row set
    -- so changing m changes no row."""
    from tests import test_policy_head as th
    lg, _ = th._logits(layout)
    for mkind in th.MASK_KINDS:
        mk, _ = th._mask(mkind)
        want, explored = _eps_reference(layout.startswith("bf16"), mkind, 0.5)
        assert 0.45 < explored.mean() < 0.55
        for m in th.SIZES:
            got = _eps_call(lg, mk, m, 0.5)
            assert np.array_equal(got, want[:m]), (layout, mkind, m, np.flatnonzero(got != want[:m])[:5])


def test_epsilon_values_slices_and_the_deterministic_rule():
    """epsilon 0, 0.05 and 1 bit for bit; epsilon 0 is sample_actions(deterministic=True); a slice called with its global index0 equals the slice of the
    full call; env.act and RowBuffers.sample pass epsilon on; bad arguments are BG_E_ARG."""
    import torch
    from balatro_gym_amd import _native as nat, sample_actions
    from tests import test_policy_head as th
    for layout, mkind in (("f32", "rec384"), ("bf16", "dense"), ("f32_s64", None)):
        lg, _ = th._logits(layout)
        mk, _ = th._mask(mkind)
        for eps in (0.0, 0.05, 1.0):
            want, explored = _eps_reference(layout.startswith("bf16"), mkind, eps)
            got = _eps_call(lg, mk, th.M, eps)
            assert np.array_equal(got, want), (layout, mkind, eps)
            assert explored.all() == (eps == 1.0) and explored.any() == (eps > 0.0)
            for a0, b0 in ((64, 1000), (37, 613), (4001, 4133), (1, 2)):
                assert np.array_equal(_eps_call(lg, mk, b0 - a0, eps, a0), want[a0:b0]), (layout, mkind, eps, a0, b0)
        det = sample_actions(lg, mk, seed=th.SEED, t=th.T, index0=th.INDEX0, deterministic=True)[0].cpu().numpy()
        assert np.array_equal(_eps_call(lg, mk, th.M, 0.0), det)
    # the C ABI refuses what the contract excludes
    L = nat.load()
    lg, _ = th._logits("f32")
    out = torch.full((66,), th.POISON_I, dtype=torch.int32, device="cuda")
    fl = torch.zeros(64, dtype=torch.float32, device="cuda")
    vp = C.c_void_p

    def call(eps=0.5, flags=0, lp=None, en=None, logits=lg.data_ptr(), actions=out.data_ptr() + 4):
        return L.bg_sample_actions_eps(vp(logits), 0, C.c_uint64(60), None, C.c_uint64(0), C.c_int64(64), C.c_uint32(flags), C.c_uint64(1), C.c_uint64(0), C.c_uint64(0),
                                       C.c_float(eps), vp(actions), vp(lp), vp(en), None, vp(torch.cuda.current_stream().cuda_stream))
    for kw in (dict(eps=-0.01), dict(eps=1.01), dict(eps=float("nan")), dict(flags=1), dict(flags=2), dict(lp=fl.data_ptr()), dict(en=fl.data_ptr()), dict(logits=0),
               dict(actions=0), dict(actions=out.data_ptr() + 2), dict(actions=lg.data_ptr())):
        assert call(**kw) == -1, kw
        assert L.bg_last_error(None).decode().startswith("bg_sample_actions_eps: "), kw
    torch.cuda.synchronize()
    assert bool((out == th.POISON_I).all()), "a refused call wrote an output"
    assert call() == 0
    torch.cuda.synchronize()
    assert int(out[0]) == th.POISON_I and int(out[-1]) == th.POISON_I and bool((out[1:-1] >= 0).all())


# ---------------------------------------------------------------- end to end

def test_replay_epsilon_greedy_and_one_sgd_step_end_to_end():
    """256 envs, a RowReplay of 6 slots: start, then three step_many calls of K = 2 with masked epsilon-greedy actions (the ring wraps once).  The
    sampled (index, next_index) pairs are checked against the records' own bytes on the host; encode_rows(store, index=) feeds a two-layer float32
    MLP Q-network (153 -> 64 tanh -> 60) and its copy as target; dqn_loss (double DQN, masked), backward and one SGD step.  The parameters after the
    step equal before - lr * grad, and the gradients match the float64 twin built on the host from the same record bytes, with the kernel's dq replaced
    by SB3's loss under autograd (dqn_ref.sb3_statement), its Q values pinned to the GPU's float32 values (straight through).  Tolerance: the float32
    network's own, as test_mlp_takes_one_sgd_step_through_ppo_loss derives it -- dqn_ref's bound of every dq element carried through the absolute
    Jacobian, plus 2**-14 of the sum of absolute terms of each gradient element for the network's float32 passes, with the absolute error of the
    pre-activation (ppo_ref.mlp_gradient_bounds(forward_abs=True): the DQN gradient has ONE non-zero column per row, the case that form is for)."""
    import copy
    import torch
    from balatro_gym_amd import BalatroVecEnv, RowReplay, dqn_loss, encode_rows, sample_actions
    from balatro_gym_amd.vec_env import RowBuffers
    from tests import ppo_ref
    n, Cn, K, m = 256, 6, 2, 512
    env = BalatroVecEnv(n, [9000 + i for i in range(n)], scorer_jokers=True, autoreset=True, fused_steps=16, obs_layout="rows")
    dev = env.device
    torch.manual_seed(11)
    net = torch.nn.Sequential(torch.nn.Linear(153, 64), torch.nn.Tanh(), torch.nn.Linear(64, 60)).to(dev)
    target = copy.deepcopy(net).requires_grad_(False)
    with torch.no_grad():
        for p in target.parameters():
            p.mul_(0.9)   # (a target that is not the online network: double DQN's two maxima differ)
    squash = lambda x: x / (1.0 + x.abs())   # noqa: E731  (a fixed squashing of the raw features, the same on both sides)
    replay = RowReplay(Cn, n, dev)
    assert replay.store.data_ptr() % 128 == 0 and tuple(replay.store.shape) == (Cn, n, 384)
    replay.start(env.obs_rows)
    rb = RowBuffers(n, dev, steps=K, row_stride=384)
    last = env.obs_rows
    host_chain = [last.cpu().numpy().copy()]
    step = 0
    for call in range(3):
        with torch.no_grad():
            qv = net(squash(encode_rows(last, "produced")))
        a0 = env.act(qv, seed=5, t=step, epsilon=0.5) if call == 0 else rb.sample(qv, seed=5, t=step, epsilon=0.5)[0]
        a1 = sample_actions(qv, last, seed=5, t=step + 1, epsilon=0.5)[0]
        want0, _ = dqn_ref.eps_actions(qv.cpu().numpy(), last.cpu().numpy()[:, 176:236], 5, 0, step, 0.5)
        assert np.array_equal(a0.cpu().numpy(), want0) and (a0 >= 0).all()
        acts = torch.stack([a0, a1])
        env.step_many(acts, obs_buffers=rb)
        env.check()
        assert torch.equal(rb.action, acts)
        replay.add(rb.rows)
        host_chain += [rb.rows[k].cpu().numpy().copy() for k in range(K)]
        last = rb.rows[-1]
        step += K
    assert len(replay) == (Cn - 1) * n and step == 6
    # the ring against the chain: slot s holds chain record t with t % Cn == s, the newest Cn of them
    store_h = replay.store.cpu().numpy()
    for tstep in range(len(host_chain) - Cn, len(host_chain)):
        assert np.array_equal(store_h[tstep % Cn], host_chain[tstep])
    gen = torch.Generator(device=dev).manual_seed(3)
    index, next_index = replay.sample(m, generator=gen)
    assert index.dtype == torch.int32 and index.device == dev and tuple(next_index.shape) == (m,)
    ih, nh = index.cpu().numpy().astype(np.int64), next_index.cpu().numpy().astype(np.int64)
    flat = store_h.reshape(Cn * n, 384)
    newest = (len(host_chain) - 1) % Cn
    assert ((ih % n) == (nh % n)).all() and ((nh // n) == ((ih // n) + 1) % Cn).all() and ((ih // n) != newest).all() and len(set(ih // n)) == Cn - 1
    chain_pos = {t % Cn: t for t in range(len(host_chain) - Cn, len(host_chain))}
    for i in range(0, m, 37):   # the pair is (record t, record t + 1) of one env, bytes and all
        t0 = chain_pos[int(ih[i] // n)]
        assert np.array_equal(flat[ih[i]], host_chain[t0][ih[i] % n]) and np.array_equal(flat[nh[i]], host_chain[t0 + 1][nh[i] % n])
    # one update
    x, xn = squash(encode_rows(replay.store, "produced", index=index)), squash(encode_rows(replay.store, "produced", index=next_index))
    assert tuple(x.shape) == (m, 153)
    q = net(x)
    with torch.no_grad():
        q_next, q_next_online = target(xn), net(xn)
    lr = 0.1
    opt = torch.optim.SGD(net.parameters(), lr=lr)
    before = [p.detach().clone() for p in net.parameters()]
    loss, st = dqn_loss(q, q_next, replay.store, next_index, q_next_online=q_next_online, gamma=GAMMA)
    opt.zero_grad()
    loss.backward()
    grads = [p.grad.detach().cpu().numpy().astype(np.float64) for p in net.parameters()]
    opt.step()
    for p, b, g in zip(net.parameters(), before, grads):
        assert torch.allclose(p.detach(), b - lr * p.grad, rtol=1e-6, atol=1e-8) and not torch.equal(p.detach(), b) and np.abs(g).sum() > 0.0
    # the contract on the host, from the same record bytes
    c = dqn_ref.Case(q.detach().cpu().numpy(), q_next.cpu().numpy(), q_next_online.cpu().numpy(), flat, next_index.cpu().numpy(), np.zeros(Cn * n, np.float32))
    flags = dqn_ref.MASK_NEXT | dqn_ref.TIMEOUT_EXCLUDE
    ct = dqn_ref.Contract(c, GAMMA, flags, True)
    ct.check(st.dq.cpu().numpy(), st.td.cpu().numpy(), st.raw.cpu().numpy(), "end to end")
    assert ct.excluded.sum() == 0 and np.array_equal(ct.a, flat[nh, 172:176].copy().view(np.int32)[:, 0])
    sh = dqn_ref.check_contract_against_sb3(c, ct, "end to end")
    # the float64 twin, pinned to the GPU's Q values
    twin = torch.nn.Sequential(torch.nn.Linear(153, 64), torch.nn.Tanh(), torch.nn.Linear(64, 60)).double()
    twin.load_state_dict({k: v.detach().cpu().double() for k, v in zip(twin.state_dict().keys(), before)})
    x64 = x.detach().cpu().double()
    out64 = twin(x64)
    pinned = out64 + (torch.from_numpy(c.q).double() - out64).detach()
    loss64, _, _ = dqn_ref.sb3_statement(c, ct, ct.gamma32, params=pinned)
    loss64.backward()
    want = [p.grad.numpy() for p in twin.parameters()]
    _, dq64, _ = dqn_ref.sb3_statement(c, ct, ct.gamma32)
    scale = np.abs(ct.qa.astype(np.float64)) + np.abs(ct.r64) + float(ct.gamma32) * np.abs(ct.n)
    B = np.zeros((m, 60))
    B[np.arange(m), ct.a] = (4 * dqn_ref.ULP * scale + dqn_ref.ULP * np.abs(ct.g.astype(np.float64))) / m
    W1, b1, W2, b2 = (p.detach().numpy() for p in twin.parameters())
    worst = ppo_ref.check_mlp_gradients(grads, want, ppo_ref.mlp_gradient_bounds(B, np.abs(dq64), (W1, b1), W2, x64.numpy(), forward_abs=True))
    assert abs(float(loss64.detach()) - float(loss.detach())) <= 2.0 ** -20 * (1.0 + abs(float(loss64.detach())))
    print(f"end to end: largest share of a propagated bound {worst:.3f}; (a) against (b) {sh}")
    env.close()
