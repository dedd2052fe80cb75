"""RowOptimizer / bg_optim_step on the MI355X, held to tests/optim_ref.py BIT FOR BIT on every output and stat.
  base set      tensors of 1, 3, 4, 5, 60, 1 023, 1 024 and 1 025 elements, a RowExtractor weight [32, 447] with its pitch-448 shadow and a RowActor weight
                [60, 256] with a dense one; the 60-element tensor is a view that starts one float into its storage (the element path); three targets.
                Three consecutive steps from random state: Adam and RMSpropTFLike, clip active and inactive and off, wd 0 and 0.01, zero_grad on and off,
                tau in {0, 0.005, 1.0}; the second and third step write into the existing gradients, so the cached table is used.
  one more level  one tensor of 300 * 1024 + 7 elements behind the base set: 339 chunks, two per lane of the combining fold; two optimisers on equal
                inputs give equal bits.
  non-finite    one NaN and, separately, one Inf: skipped == 1, parameters, states, shadows and targets bitwise untouched, step not advanced,
                gradients zeroed under zero_grad; the following finite step is the reference's first step.
  grad is None  the parameter is left out and its state unchanged.
  attach        RowLinear, RowExtractor and RowActor with a shadow give bitwise the outputs without; after weight.copy_() the module casts again and is
                still correct; after refresh() it reads the shadow again (shown with a write through .data, which the version cannot see).
  end to end    five steps of a small MLP behind a RowActor against clip_grad_norm_ + torch.optim.Adam on the GPU: the parameters sit inside the k-step
                bound of optim_ref.py (`KStepBound`), against the float64 trajectory of torch's own gradients and against torch's float32 parameters.
                Largest observed shares: 0.92 and 0.85 (the end-to-end test's docstring)."""
import numpy as np
import pytest

from tests import optim_ref as R

pytestmark = pytest.mark.gpu

FOLD_SHAPES = R.BASE_SHAPES + [(300 * 1024 + 7,)]
CONFIGS = [(algo, max_norm, wd, zg, tau) for algo in (R.ADAM, R.RMSPROP_TF) for max_norm, wd, zg, tau in
           ((0.5, 0.0, True, 0.0), (0.0, 0.01, False, 0.005), (1e6, 0.01, True, 1.0), (0.5, 0.01, False, 1.0), (-1.0, 0.0, True, 0.005))]
_cache: dict = {}


def _np(t):
    return t.detach().contiguous().cpu().numpy()


def _u16(t):
    import torch
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


class Case:
    """The base set (or a longer one) as a RowOptimizer on the device and as optim_ref Tensors on the host, from the same random state."""

    def __init__(self, seed, algo, shapes=R.BASE_SHAPES, step0=3, targeted=R.TARGETED, **hyper):
        import torch
        from balatro_gym_amd import RowActor, RowExtractor, RowOptimizer
        self.algo, self.h = algo, R.Hyper(algo, **hyper)
        data = R.random_set(seed, shapes, algo)
        dev = "cuda"
        self.mods = {8: RowExtractor(32, device=dev), 9: RowActor(256, device=dev)}
        self.params = []
        for i, d in enumerate(data):
            x = torch.from_numpy(d["p"]).to(dev)
            if i in self.mods:
                p = self.mods[i].weight
                p.data.copy_(x.view(d["shape"]))
            elif i == R.OFFSET_TENSOR:
                store = torch.zeros(x.numel() + 1, device=dev)
                store[1:] = x
                p = store[1:].requires_grad_()
                assert p.data_ptr() % 16 == 4 and p.is_contiguous()
            else:
                p = x.view(d["shape"]).clone().requires_grad_()
            self.params.append(p)
        h = self.h
        self.opt = RowOptimizer(self.params, lr=h.lr, algorithm="adam" if algo == R.ADAM else "rmsprop_tf", betas=(h.beta1, h.beta2), eps=h.raw["eps"],
                                alpha=h.beta1, weight_decay=h.raw["weight_decay"], max_grad_norm=h.raw["max_norm"])
        for i, d in enumerate(data):
            self.opt.state1[i].copy_(torch.from_numpy(d["s1"]).to(dev).view(d["shape"]))
            if algo == R.ADAM:
                self.opt.state2[i].copy_(torch.from_numpy(d["s2"]).to(dev).view(d["shape"]))
        self.opt._set_carry(step0)
        for m in self.mods.values():
            self.opt.attach(m)
        self.targets = {i: torch.from_numpy(data[i]["target"]).to(dev).view(data[i]["shape"]).clone() for i in targeted}
        self.opt.set_target([self.params[i] for i in targeted], [self.targets[i] for i in targeted])
        self.rc = R.Carry.at(step0, h.beta1, h.beta2) if algo == R.ADAM else R.Carry(step0)
        self.ref = []
        for i, d in enumerate(data):
            sh = cols = pitch = 0
            if i in self.mods:
                store, cols, pitch, _ = self.opt._shadows[id(self.params[i])]
                sh = _u16(store).ravel().copy()
                assert R.same_bits(sh.reshape(-1, pitch)[:, :cols].ravel(), R.bf16_bits(d["p"])), "attach fills the shadow"
            self.ref.append(R.Tensor(d["p"].copy(), d["g"].copy(), d["s1"].copy(), d["s2"].copy() if algo == R.ADAM else None, sh if i in self.mods else None,
                                     cols, pitch, d["target"].copy() if i in targeted else None))
        self.set_grads([d["g"] for d in data])

    def set_grads(self, gs, skip=()):
        import torch
        for i, (p, g, t) in enumerate(zip(self.params, gs, self.ref)):
            if i in skip:
                p.grad = None
                continue
            x = torch.from_numpy(np.ascontiguousarray(g, np.float32)).to(p.device).view(p.shape)
            if p.grad is None:
                p.grad = x.clone()
            else:
                p.grad.copy_(x)   # the same memory: the cached table stays
            t.g[:] = g

    def step(self, active=None, **kw):
        st = self.opt.step(zero_grad=self.h.zero_grad, target_tau=self.h.raw["tau"], **kw)
        want = R.step(self.ref if active is None else [self.ref[i] for i in active], self.h, self.rc)
        return st, want

    def compare(self, st, want, what, active=None):
        import torch
        for i, (p, t) in enumerate(zip(self.params, self.ref)):
            got = {"p": _np(p).ravel(), "s1": _np(self.opt.state1[i]).ravel()}
            if p.grad is not None:
                got["g"] = _np(p.grad).ravel()
            if self.algo == R.ADAM:
                got["s2"] = _np(self.opt.state2[i]).ravel()
            if i in self.targets:
                got["target"] = _np(self.targets[i]).ravel()
            if i in self.mods:
                got["shadow"] = _u16(self.opt._shadows[id(p)][0]).ravel()
            for name, x in got.items():
                assert R.same_bits(x, getattr(t, name)), (what, i, name, int((x != getattr(t, name)).sum()))
        assert _np(st.grad_norm).tobytes() == np.float32(want["grad_norm"]).tobytes(), (what, float(st.grad_norm), want["grad_norm"])
        assert _np(st.clip_coef).tobytes() == np.float32(want["clip_coef"]).tobytes(), (what, float(st.clip_coef), want["clip_coef"])
        assert (int(st.skipped), int(st.nonfinite), int(st.step), int(st.raw[3])) == (want["skipped"], want["nonfinite"], want["step"], 0), what
        c = _np(self.opt._carry)
        assert (int(c.view(np.int64)[0]), float(c[1]), float(c[2])) == (self.rc.step, self.rc.b1pow, self.rc.b2pow), what
        assert isinstance(st.grad_norm, torch.Tensor) and st.grad_norm.is_cuda, "lazy device views"


@pytest.mark.parametrize("algo,max_norm,wd,zg,tau", CONFIGS)
def test_three_steps_of_the_base_set_bit_for_bit(algo, max_norm, wd, zg, tau):
    c = Case(5 + algo, algo, lr=3e-4 if algo == R.ADAM else 7e-4, beta1=0.9 if algo == R.ADAM else 0.99, weight_decay=wd, max_norm=max_norm, tau=tau, zero_grad=zg)
    rng = np.random.default_rng(99)
    for k in range(3):
        if k:
            c.set_grads([(rng.normal(0, 1, t.p.size) * 10.0 ** -k).astype(np.float32) for t in c.ref])
        table = c.opt._table
        st, want = c.step(lr=None if k < 2 else c.h.lr)
        assert k == 0 or c.opt._table is table, "no pointer changed: the table is not uploaded again"
        c.compare(st, want, f"step {k}")
        assert want["skipped"] == 0 and want["step"] == 4 + k
        for p in c.params:
            assert (not zg) or not bool(p.grad.any())
    clipped = float(st.clip_coef) < 1.0
    assert clipped == (max_norm == 0.5)
    store = c.opt._shadows[id(c.params[8])][0]
    assert not bool(store[:, 447].any()), "the padding column of the pitch-448 shadow is not written"
    for i, m in c.mods.items():
        import torch
        assert torch.equal(m.weight_bf16, m.weight.detach().to(torch.bfloat16)), "the shadow is the weight's bfloat16 rounding"


@pytest.mark.parametrize("algo", [R.ADAM, R.RMSPROP_TF])
def test_past_one_reduction_level_and_repeatable(algo):
    assert sum(R.chunks_of(np.prod(s)) for s in FOLD_SHAPES) == 339
    kw = dict(beta1=0.9 if algo == R.ADAM else 0.99, weight_decay=0.01, max_norm=0.5, tau=0.005)
    a = Case(21 + algo, algo, FOLD_SHAPES, step0=0, targeted=(5, 10), **kw)
    b = Case(21 + algo, algo, FOLD_SHAPES, step0=0, targeted=(5, 10), **kw)
    st, want = a.step()
    a.compare(st, want, "fold")
    assert float(want["clip_coef"]) < 1e-2 and want["step"] == 1
    st_b, _ = b.step()
    assert _np(st.raw).tobytes() == _np(st_b.raw).tobytes()
    for p, q, s, t in zip(a.params, b.params, a.opt.state1, b.opt.state1):
        assert R.same_bits(_np(p), _np(q)) and R.same_bits(_np(s), _np(t)), "two calls on equal inputs give equal bits"


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("zg", [True, False])
def test_a_non_finite_gradient_skips_the_step(bad, zg):
    kw = dict(weight_decay=0.01, max_norm=0.5, tau=1.0, zero_grad=zg)
    c = Case(31, R.ADAM, step0=5, **kw)
    fresh = Case(31, R.ADAM, step0=5, **kw)
    before = {k: [_np(x).copy() for x in v] for k, v in (("p", c.params), ("s1", c.opt.state1), ("s2", c.opt.state2))}
    before["target"] = {i: _np(t).copy() for i, t in c.targets.items()}
    before["shadow"] = {i: _u16(c.opt._shadows[id(c.params[i])][0]).copy() for i in c.mods}
    gs = [t.g.copy() for t in c.ref]
    gs[7][1024] = bad
    c.set_grads(gs)
    st, want = c.step()
    c.compare(st, want, "skip")
    assert int(st.skipped) == 1 and int(st.nonfinite) == 1 and int(st.step) == 5, "skipped, counted, and the step not advanced"
    for k, xs in (("p", c.params), ("s1", c.opt.state1), ("s2", c.opt.state2)):
        for x, y in zip(xs, before[k]):
            assert R.same_bits(_np(x), y), k
    for i, t in c.targets.items():
        assert R.same_bits(_np(t), before["target"][i])
    for i in c.mods:
        assert R.same_bits(_u16(c.opt._shadows[id(c.params[i])][0]), before["shadow"][i])
    for p in c.params:
        assert (not bool(p.grad.any())) if zg else True
    assert zg or not np.isfinite(_np(c.params[7].grad)[1024])
    # the following finite step is the first step of a run that never saw the bad gradient
    rng = np.random.default_rng(7)
    gs = [rng.normal(0, 1, t.p.size).astype(np.float32) for t in c.ref]
    c.set_grads(gs)
    fresh.set_grads(gs)
    st_a, _ = c.step()
    st_f, want_f = fresh.step()
    fresh.compare(st_f, want_f, "the reference's first step")
    assert _np(st_a.raw).tobytes() == _np(st_f.raw).tobytes() and int(st_a.step) == 6 and int(st_a.skipped) == 0
    for p, q in zip(c.params, fresh.params):
        assert R.same_bits(_np(p), _np(q))


def test_a_parameter_without_a_gradient_is_left_out():
    c = Case(41, R.ADAM, weight_decay=0.01, max_norm=0.5, tau=0.005)
    out = (2, 7, 9)
    keep = {i: (_np(c.params[i]).copy(), _np(c.opt.state1[i]).copy(), _np(c.opt.state2[i]).copy(), _np(c.targets[i]).copy() if i in c.targets else None) for i in out}
    c.set_grads([t.g for t in c.ref], skip=out)
    active = [i for i in range(len(c.params)) if i not in out]
    st, want = c.step(active=active)
    c.compare(st, want, "grad is None")
    for i, (p, s1, s2, tg) in keep.items():
        assert c.params[i].grad is None
        assert R.same_bits(_np(c.params[i]), p) and R.same_bits(_np(c.opt.state1[i]), s1) and R.same_bits(_np(c.opt.state2[i]), s2)
        assert tg is None or R.same_bits(_np(c.targets[i]), tg)
    # ... and is back in the next step, through a new table
    rng = np.random.default_rng(3)
    c.set_grads([rng.normal(0, 1, t.p.size).astype(np.float32) for t in c.ref])
    st, want = c.step()
    c.compare(st, want, "all of them again")


def _rows():
    if "rows" not in _cache:
        from balatro_gym_amd import BalatroVecEnv
        from balatro_gym_amd.vec_env import RowBuffers
        n, K = 96, 2
        env = BalatroVecEnv(n, [7000 + i for i in range(n)], autoreset=True)
        rb = RowBuffers(n, env.device, steps=K, row_stride=384)
        env.rollout(K, policy=0, policy_seed=3, obs_buffers=rb)
        env.check()
        _cache["rows"] = rb.rows.reshape(-1, 384)[:130].clone()
        env.close()
    return _cache["rows"]


@pytest.mark.parametrize("kind", ["linear", "extractor", "actor"])
def test_attach_gives_the_same_bits_and_follows_the_version(kind):
    import torch
    from balatro_gym_amd import RowActor, RowExtractor, RowLinear, RowOptimizer
    from balatro_gym_amd.rows import _live_shadow
    torch.manual_seed(11)
    rows = _rows()
    if kind == "actor":
        layer = RowActor(64, device="cuda")
        h = torch.randn((130, 64), device="cuda").to(torch.bfloat16)
        acts = torch.randint(0, 60, (130,), device="cuda", dtype=torch.int32)

        def run(l):
            lp, ent = l.evaluate(h, acts, rows)
            a, lp2, _ = l.act(h, rows, seed=5, t=1)
            loss, ps = l.ppo_loss(h, acts, torch.full((130,), -3.0, device="cuda"), torch.linspace(-1, 1, 130, device="cuda"), rows)
            return [lp, ent, a, lp2, loss, ps.dh, ps.dweight, ps.dbias]
    else:
        layer = RowLinear(64, "fixed", "relu", device="cuda") if kind == "linear" else RowExtractor(64, device="cuda")

        def run(l):
            return [l(rows)]

    def clone_of(l):   # an unattached layer with the same parameters: the cast path
        other = type(l)(64, device="cuda") if kind != "linear" else RowLinear(64, "fixed", "relu", device="cuda")
        other.load_state_dict(l.state_dict())
        assert other.weight_bf16 is None
        return other

    def same(xs, ys, what):
        bits = lambda t: t.detach().contiguous().reshape(-1).view(torch.uint8)   # noqa: E731
        for x, y in zip(xs, ys):
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(bits(x), bits(y)), what
    plain = run(layer)
    opt = RowOptimizer(layer.parameters(), lr=1e-2)
    opt.attach(layer)
    assert _live_shadow(layer) is layer.weight_bf16 and layer.weight_bf16.stride(0) == (448 if kind == "extractor" else layer.weight.shape[1])
    same(run(layer), plain, "with a shadow: the same bits")
    # a step: the update pass writes the shadow; the module reads it and agrees with an unattached layer of the same parameters
    out = run(layer)[-1] if kind != "actor" else run(layer)[4]
    layer.zero_grad()
    (out.float().square().mean() if kind != "actor" else out).backward()
    st = opt.step()
    assert int(st.skipped) == 0 and _live_shadow(layer) is not None, "the kernel's write does not bump the version"
    assert torch.equal(layer.weight_bf16, layer.weight.detach().to(torch.bfloat16))
    same(run(layer), run(clone_of(layer)), "behind a step")
    # a write through .data is invisible to the version: the module keeps reading the stale shadow -- which shows that the shadow IS what it reads
    stale = run(layer)
    layer.weight.data.mul_(1.5)
    same(run(layer), stale, "the stale shadow is read")
    opt.refresh()
    same(run(layer), run(clone_of(layer)), "behind refresh()")
    assert torch.equal(layer.weight_bf16, layer.weight.detach().to(torch.bfloat16))
    # a torch in-place write bumps the version: the module casts again and is still correct
    with torch.no_grad():
        layer.weight.copy_(layer.weight * 0.5)
    assert _live_shadow(layer) is None
    same(run(layer), run(clone_of(layer)), "fallen back to the cast")
    assert not torch.equal(layer.weight_bf16, layer.weight.detach().to(torch.bfloat16))
    opt.refresh()
    assert _live_shadow(layer) is layer.weight_bf16 and torch.equal(layer.weight_bf16, layer.weight.detach().to(torch.bfloat16))
    same(run(layer), run(clone_of(layer)), "the shadow again")


def test_five_steps_of_a_small_policy_against_torch_adam():
    """Two copies of Linear(40, 64) -> tanh -> RowActor(64): one stepped by RowOptimizer, one by clip_grad_norm_(0.5) + torch.optim.Adam(eps=1e-5) on the
    GPU, each from its own gradients.  X is the float64 trajectory (optim_ref.exact_step) of torch's gradients.  Ours against X: inside KStepBound fed
    with ours' float32 inputs and e_g = |g_ours - g_torch|.  Ours against torch's float32 parameters: inside that bound plus the same bound on torch's own
    values (its norm's float32 error measured and passed in).  Largest observed shares on the MI355X: 0.92 of the bound against X, 0.85 against torch's
    float32 Adam (the line printed below)."""
    import torch
    from balatro_gym_amd import RowActor, RowOptimizer
    torch.manual_seed(3)
    dev = "cuda"
    m, K = 256, 5

    def make():
        torch.manual_seed(17)
        return torch.nn.Linear(40, 64, device=dev), RowActor(64, device=dev)
    (l1, a1), (l2, a2) = make(), make()
    x = torch.randn((m, 40), device=dev)
    acts = torch.randint(0, 60, (m,), device=dev, dtype=torch.int32)
    old_lp = torch.full((m,), float(np.log(1 / 60)), device=dev)
    adv = torch.randn(m, device=dev)
    ours = list(l1.parameters()) + list(a1.parameters())
    theirs = list(l2.parameters()) + list(a2.parameters())
    h = R.Hyper(R.ADAM, lr=3e-3, eps=1e-5, max_norm=0.5)
    opt = RowOptimizer(ours, lr=h.lr, eps=1e-5, max_grad_norm=0.5)
    opt.attach(a1)
    adam = torch.optim.Adam(theirs, lr=h.lr, eps=1e-5)
    kb_ours, kb_torch = R.KStepBound(h, len(ours)), R.KStepBound(h, len(ours))
    X = [(_np(p).astype(np.float64).ravel(), np.zeros(p.numel()), np.zeros(p.numel())) for p in theirs]
    for k in range(K):
        for lin, act, ps in ((l1, a1, ours), (l2, a2, theirs)):
            for p in ps:
                if p.grad is not None:
                    p.grad.zero_()
            loss, _ = act.ppo_loss(torch.tanh(lin(x)).to(torch.bfloat16), acts, old_lp, adv, clip_range=0.2, ent_coef=0.01)
            loss.backward()
        g_o, g_t = [_np(p.grad).ravel() for p in ours], [_np(p.grad).ravel() for p in theirs]
        e_g = [np.abs(a.astype(np.float64) - b.astype(np.float64)) for a, b in zip(g_o, g_t)]
        zeros = [np.zeros(p.numel(), np.float32) for p in theirs]
        st_t = [(adam.state[p]["exp_avg"], adam.state[p]["exp_avg_sq"]) if adam.state.get(p) else None for p in theirs]
        P_o = kb_ours.advance([_np(p).ravel() for p in ours], g_o, [_np(s).ravel() for s in opt.state1], [_np(s).ravel() for s in opt.state2], e_g)
        norm64 = float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in g_t)))
        total = float(torch.nn.utils.clip_grad_norm_(theirs, 0.5))
        P_t = kb_torch.advance([_np(p).ravel() for p in theirs], g_t, [_np(s[0]).ravel() if s else z for s, z in zip(st_t, zeros)],
                               [_np(s[1]).ravel() if s else z for s, z in zip(st_t, zeros)],
                               [np.zeros(1)] * len(theirs), e_norm=abs(total - norm64))
        X = [R.exact_step(h, k + 1, xp, g, xm, xv, norm64) for (xp, xm, xv), g in zip(X, g_t)]
        st = opt.step()
        adam.step()
        assert int(st.skipped) == 0 and int(st.step) == k + 1
        assert abs(float(st.grad_norm) - float(np.sqrt(R.grad_norm(g_o)[0]))) <= 2.0 ** -23 * norm64
    share_x = share_t = 0.0
    for p, q, Po, Pt, (xp, _, _) in zip(ours, theirs, P_o, P_t, X):
        mine, other = _np(p).astype(np.float64).ravel(), _np(q).astype(np.float64).ravel()
        assert R.same_bits(Po.v, _np(p).ravel()), "the bound ran on the values of the steps it bounds"
        ex, et = np.abs(mine - xp), np.abs(mine - other)
        share_x, share_t = max(share_x, float((ex / Po.e).max())), max(share_t, float((et / (Po.e + Pt.e)).max()))
        assert (ex <= Po.e).all() and (et <= Po.e + Pt.e).all(), (float((ex / Po.e).max()), float((et / (Po.e + Pt.e)).max()))
    moved = float((ours[0].detach() - make()[0].weight.detach()).abs().max())
    assert moved > h.lr, "five steps moved the parameters"
    print(f"end to end, {K} steps: largest share of the bound against the float64 trajectory {share_x:.3f}, against torch's float32 Adam {share_t:.3f}")
