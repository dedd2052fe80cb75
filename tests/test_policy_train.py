"""RowPolicy under RowOptimizer steps, and act() against latent(), on the MI355X.
  attach        the statements of tests/test_optim_step.py::test_attach_gives_the_same_bits_and_follows_the_version for a RowDense, a masked RowDense and a
                whole RowPolicy, under Adam and RMSpropTFLike: with a shadow, behind a step (gradients from latent() -> action.ppo_loss), the stale
                read, behind refresh(), behind a version bump (the cast path: `_table_key is None`), behind a second refresh() -- every output of
                act() and evaluate() (actions, log_prob, values, entropy, taps, logits) bit for bit against an unattached clone with the same
                state_dict; the host table is ONE object across the step, so the cached table is what read the new parameters.
  block-diagonal  a stack_blocks layer under three device steps (Adam, Adam with weight decay, RMSpropTFLike): off-block weights stay exactly zero,
                the copy's off-block entries are +0.0 bits, the blocks move; a masked layer that started with non-zero off-block weights keeps
                copy == bfloat16(masked_weight()) behind every step.
  act / latent  the reference's topology, 200 rows: the kernel's logits and values against the float64 network (policy_ref.chain64) are no worse than
                1.5 x the bfloat16 torch path's (RMS), and the first PPO ratio is inside the clip range: |log_prob(act) - log_prob(latent)| <
                log(1.2) on every row.  Measured: the test's docstring."""
import numpy as np
import pytest

from tests import policy_ref as pr

pytestmark = pytest.mark.gpu

KINDS = ("dense", "dense_masked", "policy")


def _two_blocks():
    import torch
    mask = torch.zeros((64, 64))
    mask[:32, :32] = 1.0
    mask[32:, 32:] = 1.0
    return mask


def _make(kind):
    """dense / dense_masked: one layer driven through a one-layer RowPolicy; policy: a block-diagonal layer, a trunk layer, pi, vf, action, value."""
    import torch
    from balatro_gym_amd import RowActor, RowDense, RowPolicy
    dev = "cuda"
    if kind == "dense":
        return RowPolicy([RowDense(64, 96, "tanh", device=dev)], [], [], RowActor(96, device=dev), None)
    if kind == "dense_masked":   # left at its nn.Linear initialisation
        return RowPolicy([RowDense(64, 64, "relu", mask=_two_blocks(), device=dev)], [], [], RowActor(64, device=dev), None)
    blocks = RowPolicy.stack_blocks([torch.nn.Linear(32, 32, device=dev), torch.nn.Linear(32, 32, device=dev)])
    return RowPolicy([blocks, RowDense(64, 96, "relu", device=dev)], [RowDense(96, 64, "tanh", device=dev)], [RowDense(96, 32, "tanh", device=dev)],
                     RowActor(64, device=dev), RowDense(32, 1, device=dev))


def _inputs():
    import torch
    from tests.test_optim_step import _rows
    rows = _rows()
    assert tuple(rows.shape) == (130, 384) and bool((rows[:, 176:236] != 0).any(1).all()), "130 records, no all-masked row"
    g = torch.Generator().manual_seed(21)
    h = torch.randn((130, 64), generator=g).to(torch.bfloat16).cuda()
    acts = torch.randint(0, 60, (130,), generator=g, dtype=torch.int32).cuda()
    return rows, h, acts


def _backward(policy, h, rows):
    """The training path: latent() -> action.ppo_loss -> backward, on actions the policy itself drew (all valid)."""
    import torch
    a, lp, v, _ = policy.act(h, rows, seed=8, t=2)
    adv = torch.linspace(-1, 1, h.shape[0], device="cuda")
    for p in policy.parameters():
        p.grad = None
    lat, values = policy.latent(h)
    kw = dict(values=values, returns=torch.linspace(0, 2, h.shape[0], device="cuda")) if values is not None else {}
    loss, _ = policy.action.ppo_loss(lat, a, lp - 0.1, adv, rows, ent_coef=0.01, **kw)
    loss.backward()
    assert all(p.grad is not None and bool(p.grad.isfinite().all()) and bool(p.grad.any()) for p in policy.parameters())


@pytest.mark.parametrize("algo", ["adam", "rmsprop_tf"])
@pytest.mark.parametrize("kind", KINDS)
def test_attach_gives_the_same_bits_and_follows_the_version(kind, algo):
    import torch
    from balatro_gym_amd import RowOptimizer
    from balatro_gym_amd.rows import _live_shadow
    torch.manual_seed(11)
    rows, h, acts = _inputs()
    policy = _make(kind)
    layers = policy.layers()

    def run(p):
        out = p.act(h, rows, seed=5, t=1, entropy=True, taps=True) + p.evaluate(h, acts, rows, taps=True)
        assert len(out) == 11 and (out[2] is None) == (p.value is None)
        return [x for x in out if x is not None]   # (values: None without a value layer)

    def clone_of(p):   # an unattached policy with the same parameters: the cast path
        other = _make(kind)
        other.load_state_dict(p.state_dict())
        assert all(l.weight_bf16 is None for l in other.layers())
        return other

    def same(xs, ys, what):
        bits = lambda t: t.detach().contiguous().reshape(-1).view(torch.uint8)   # noqa: E731
        assert len(xs) == len(ys)
        for k, (x, y) in enumerate(zip(xs, ys)):
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(bits(x), bits(y)), f"{what}: output {k}"

    def w16(l):   # the bfloat16 weight an unattached layer would read
        return (l.masked_weight() if hasattr(l, "masked_weight") else l.weight).detach().to(torch.bfloat16)
    plain = run(policy)
    assert policy._table_key is None, "unattached: a cast per call, no cached table"
    opt = RowOptimizer(policy.parameters(), lr=1e-2, algorithm=algo)
    opt.attach(policy)
    assert all(_live_shadow(l) is l.weight_bf16 and l.weight_bf16.stride(0) == l.weight.shape[1] for l in layers)
    same(run(policy), plain, "with a shadow: the same bits")
    same(run(policy), run(clone_of(policy)), "with a shadow: the bits of an unattached clone")
    table = policy._table
    assert policy._table_key is not None and table is not None
    # a step: the update pass writes the shadows; the launch goes through the table built BEFORE the step and agrees with an unattached clone
    _backward(policy, h, rows)
    st = opt.step()
    assert int(st.skipped) == 0 and all(_live_shadow(l) is not None for l in layers), "the kernel's write does not bump the version"
    assert all(torch.equal(l.weight_bf16, w16(l)) for l in layers)
    behind = run(policy)
    assert policy._table is table, "behind a step the cached table is used"
    same(behind, run(clone_of(policy)), "behind a step")
    same(run(policy), behind, "behind a step: two calls")
    assert policy._table is table
    assert not torch.equal(behind[-1], plain[-1]), "the step moved the logits: the new parameters were read"
    # a write through .data is invisible to the version: the launch keeps reading the stale shadows -- which shows that the shadows ARE what it reads
    for l in layers:
        l.weight.data.mul_(1.5)
    same(run(policy), behind, "the stale shadows are read")
    opt.refresh()
    same(run(policy), run(clone_of(policy)), "behind refresh()")
    assert all(torch.equal(l.weight_bf16, w16(l)) for l in layers) and policy._table_key is not None
    # a torch in-place write bumps the version: the cast path, still correct -- a masked layer's cast is masked, whatever was written off-block
    with torch.no_grad():
        for l in layers:
            l.weight.copy_(l.weight * 0.5 + 0.01)
    assert all(_live_shadow(l) is None for l in layers)
    same(run(policy), run(clone_of(policy)), "fallen back to the cast")
    assert policy._table_key is None, "the cast path caches no table"
    assert not any(torch.equal(l.weight_bf16, w16(l)) for l in layers)
    opt.refresh()
    assert all(_live_shadow(l) is l.weight_bf16 and torch.equal(l.weight_bf16, w16(l)) for l in layers)
    same(run(policy), run(clone_of(policy)), "the shadows again")
    assert policy._table_key is not None, "the table is cached again"


@pytest.mark.parametrize("algo,wd", [("adam", 0.0), ("adam", 0.01), ("rmsprop_tf", 0.0)])
def test_a_block_diagonal_layer_stays_block_diagonal_under_the_device_optimiser(algo, wd):
    import torch
    from balatro_gym_amd import RowOptimizer
    torch.manual_seed(13)
    rows, h, _ = _inputs()
    bits = lambda t: t.detach().contiguous().view(torch.int16)   # noqa: E731
    policy, masked = _make("policy"), _make("dense_masked")
    blocks, dm = policy.trunk[0], masked.trunk[0]
    on = blocks.block_mask != 0
    assert torch.equal(on, dm.block_mask != 0) and int(on.sum()) == 2048
    dm.weight.data.copy_(torch.nn.Linear(64, 64, device="cuda").weight.detach())   # a masked layer whose raw off-block weights are not zero
    assert int((dm.weight[~on] != 0).sum()) == 2048
    want_dm = masked.act(h, rows, seed=5, t=1, taps=True)
    for p, layer in ((policy, blocks), (masked, dm)):
        opt = RowOptimizer(p.parameters(), lr=1e-2, algorithm=algo, weight_decay=wd)
        opt.attach(p)
        if layer is dm:
            got = masked.act(h, rows, seed=5, t=1, taps=True)
            assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(got, want_dm) if x is not None), "attach changes no bit"
        for k in range(3):
            before = layer.weight.detach().clone()
            _backward(p, h, rows)
            assert bool((layer.weight.grad[~on] == 0).all())
            st = opt.step()
            assert int(st.skipped) == 0 and int(st.step) == k + 1
            assert bool((layer.weight[~on] == 0).all()), f"step {k}: an off-block weight moved"
            assert bool((bits(layer.weight_bf16)[~on] == 0).all()), f"step {k}: the copy's off-block entries are +0.0 bits"
            assert not torch.equal(layer.weight[on], before[on]), f"step {k}: the blocks moved"
            assert torch.equal(layer.weight_bf16, layer.masked_weight().detach().to(torch.bfloat16)), f"step {k}: copy == bfloat16(masked_weight())"


def test_act_agrees_with_latent_and_is_as_accurate_as_the_torch_path():
    """The reference's topology (random_net(REFERENCE, 3), random_h(200, 448, 4), real masks without an all-masked row) against X, the float64 network
    without any rounding between layers.  Both paths round to bfloat16 once per layer, so their errors are of one kind: the kernel's RMS error must not
    exceed 1.5 x the torch path's (a margin for the scatter between two implementations of the same roundings, not a measurement), for the 200 x 60
    logits and for the 200 values (whose torch path also rounds the value itself to bfloat16).  The first ratio: |log_prob(act) - log_prob(latent ->
    action.evaluate)| < log(1.2) on every row -- 0.2 is the reference's clip_range.
    Measured on the MI355X (the lines this test prints): RMS logits kernel 0.01059, torch path 0.01131; values kernel 0.01181,
    torch path 0.01116; first log-ratio max 0.0385, median 0.0063 against log(1.2) = 0.1823."""
    import torch
    from balatro_gym_amd import actor_evaluate
    from tests.test_policy_head import _records
    from tests.test_policy_rows import _bf16, _reference
    r = _reference()
    net, policy, hb, h, m = r["net"], r["policy"], r["hb"], r["h"], r["m"]
    rows = _records()[384][:m]
    assert m == 200 and tuple(hb.shape) == (200, 448) and bool((rows[:, 176:236] != 0).any(1).all()), "no all-masked row"
    X_logits, X_values = pr.chain64(net, hb)
    a, lp_act, v, _, _, logits = policy.act(h, rows, seed=77, t=5, index0=1000, taps=True)
    with torch.no_grad():
        lat, v_train = policy.latent(_bf16(hb))
    lp_train, _ = policy.action.evaluate(lat, a, rows)
    train_logits = torch.empty((m, 60), dtype=torch.float32, device="cuda")
    lp_again, _ = actor_evaluate(lat, policy.action._w(), policy.action.bias.detach(), a, rows, logits_out=train_logits)
    assert torch.equal(lp_again.view(torch.int32), lp_train.view(torch.int32))
    rms = lambda got, want: float(np.sqrt(np.mean((got.cpu().numpy().astype(np.float64) - want) ** 2)))   # noqa: E731
    k_l, t_l, k_v, t_v = rms(logits, X_logits), rms(train_logits, X_logits), rms(v, X_values), rms(v_train, X_values)
    print(f"RMS error against the float64 network: logits kernel {k_l:.4g}, torch path {t_l:.4g}; values kernel {k_v:.4g}, torch path {t_v:.4g}")
    d = (lp_act - lp_train).abs().cpu().numpy().astype(np.float64)
    print(f"first log-ratio |log_prob(act) - log_prob(latent)|: max {d.max():.4g}, median {np.median(d):.4g} (log 1.2 = {np.log(1.2):.4g})")
    assert bool(lp_act.isfinite().all()) and bool(lp_train.isfinite().all()) and t_l > 0 and t_v > 0
    assert k_l <= 1.5 * t_l, (k_l, t_l)
    assert k_v <= 1.5 * t_v, (k_v, t_v)
    assert (d < np.log(1.2)).all(), f"{int((d >= np.log(1.2)).sum())} first ratios outside the clip range, max {d.max():.4g}"
