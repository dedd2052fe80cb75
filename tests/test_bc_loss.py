"""bg_bc_loss on the MI355X, through `bc_loss`: m in {1, 63, 64, 65, 257, 16 449} (the last has more workgroup partials than the finishing workgroup has
lanes), float32 and bfloat16, the mask from records at strides 352 and 384, dense int8 and none, the actions dense and read in place from the
records, with and without an index (a permutation, repeated indices, entries out of range), weights absent, random (zeros, one negative, one NaN),
0 / 1 and all zero.  Everything is copied to the host and held to the float64 closed form of tests/bc_ref.py by the bounds derived there (never to
torch arithmetic on the GPU); log_prob / entropy are bit for bit evaluate_actions', the bf16 gradient is the float32 call's rounded to nearest even,
two calls give the same bits, bad arguments are BG_E_ARG before any launch, m == 0 zeroes the stats.  Then autograd: logits.grad is dlogits, a
two-layer MLP matches its float64 twin within ppo_ref.mlp_gradient_bounds; and one gathered case whose records lie past 4 GiB of a store, the mask
and the action read in place.

Largest observed shares of the bounds on the MI355X (the device library's expf / logf): dlogits 0.25, nll_loss 0.061, entropy_loss 0.046, loss 0.061,
accuracy 0.46, weight_sum 0.36, log_prob 0.125, entropy 0.102; the MLP's parameter gradients 0.66 of their propagated bounds (dlogits 0.053 there);
past 4 GiB: dlogits 0.073, log_prob 0.041, entropy 0.026, loss 0.003, accuracy 0.044, weight_sum 0.34."""
import ctypes as C

import numpy as np
import pytest

from tests import bc_ref, head_ref, ppo_ref

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257, 256 * 64 + 64 + 1)
MASK_KINDS = ("rec384", "rec352", "dense", None)
INDEX_KINDS = (None, "perm", "repeat")
WEIGHT_KINDS = (None, "random", "filter", "zero")
MASK_OFF, ACT_OFF = 176, 172

_shares: dict = {}


def _note(sh):
    for k, v in sh.items():
        _shares[k] = max(_shares.get(k, 0.0), float(v))


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _records(c: bc_ref.Case, stride: int, seed: int = 1):
    """The case's masks and actions inside [store_rows, stride] records of random bytes, on the device -> (records, mask argument, actions argument)."""
    import torch
    rows = np.random.default_rng(seed).integers(0, 256, (c.store_rows, stride), dtype=np.uint8)
    rows[:, MASK_OFF:MASK_OFF + 60] = c.mask.view(np.uint8)
    rows[:, ACT_OFF:ACT_OFF + 4] = np.ascontiguousarray(c.actions).view(np.uint8).reshape(-1, 4)
    d = _dev(rows)
    return d, d, d[:, ACT_OFF:ACT_OFF + 4].view(torch.int32)[:, 0]


def _run(c: bc_ref.Case, mkind, ent, bf16=False, in_place=None, timing=False):
    """bc_loss on the device -> (dlogits float32 [m, 60] or bf16 bits, log_prob, entropy, stats) as host arrays, and the (loss, stats) pair."""
    import torch
    from balatro_gym_amd import bc_loss
    logits = _dev(c.logits)
    if bf16:
        logits = logits.to(torch.bfloat16)
    if mkind is not None and mkind.startswith("rec"):
        keep, mask, actions = _records(c, int(mkind[3:]))
        if in_place is False:
            actions = _dev(c.actions)
    else:
        keep, mask, actions = None, _dev(c.mask) if mkind == "dense" else None, _dev(c.actions)
    before = None if keep is None else keep.clone()
    loss, st = bc_loss(logits, actions, mask, weights=_dev(c.weights), index=_dev(c.index), ent_coef=ent, timing=timing)
    torch.cuda.synchronize()
    assert before is None or torch.equal(before, keep), "the records were written"
    dl = st.dlogits.view(torch.int16).cpu().numpy().view(np.uint16) if bf16 else st.dlogits.cpu().numpy()
    return (dl, st.log_prob.cpu().numpy(), st.entropy.cpu().numpy(), st.raw.cpu().numpy()), (loss, st)


@pytest.mark.parametrize("m", SIZES)
def test_sets_hold_the_bounds(m):
    from balatro_gym_amd import evaluate_actions
    k = 0
    for mkind in MASK_KINDS:
        for ikind in INDEX_KINDS:
            for wkind in WEIGHT_KINDS:
                k += 1
                masked = mkind is not None
                sigma = head_ref.SIGMAS[(m + k) % 4]
                bf16 = k % 2 == 0
                c = bc_ref.synthetic(m + 7 * k, m, sigma, masked, index=ikind, weights=wkind, bf16=bf16)
                ent = (0.0, 0.01)[k % 3 != 0]
                what = f"m {m} mask {mkind} index {ikind} weights {wkind} bf16 {bf16} ent {ent}"
                cf = bc_ref.ClosedForm(c, ent)
                first, (loss, st) = _run(c, mkind, ent)
                _note(cf.check(*first, what))
                raw = first[3]
                assert raw[6] == m and raw[5] == cf.excluded.sum() and float(loss) == raw[0]
                if cf.W == 0.0:
                    assert (raw[:5] == 0.0).all() and (first[0].view(np.uint32) == 0).all(), what + ": W == 0 gives loss 0 and an all-+0.0 gradient"
                second, _ = _run(c, mkind, ent, in_place=False)
                for x, y in zip(first, second):
                    assert np.array_equal(_bits(x), _bits(y)), what + ": two calls (actions in place and dense) differ"
                if bf16:   # the bfloat16 call: the float32 gradient rounded to nearest even, everything else the same bits
                    b16, _ = _run(c, mkind, ent, bf16=True)
                    assert np.array_equal(b16[0], head_ref.bf16_bits(first[0])), what + ": bf16 gradient"
                    for x, y in zip(first[1:], b16[1:]):
                        assert np.array_equal(_bits(x), _bits(y)), what + ": bf16 scalars"
                if ikind is None:   # log_prob / entropy are evaluate_actions', bit for bit
                    elp, een = evaluate_actions(_dev(c.logits), _dev(c.actions), _dev(c.mask))
                    assert np.array_equal(_bits(elp.cpu().numpy()), _bits(first[1])) and np.array_equal(_bits(een.cpu().numpy()), _bits(first[2])), what
    print(f"m {m}: largest shares so far {_shares}")


def test_hand_made_rows_and_timing():
    for mkind in ("rec384", None):
        c = bc_ref.synthetic(21 + (mkind is not None), 300, 1.0, mkind is not None, index="perm", weights="random")
        cf = bc_ref.ClosedForm(c, 0.01)
        (dl, lp, en, raw), (loss, st) = _run(c, mkind, 0.01, timing=True)
        cf.check(dl, lp, en, raw, f"hand-made {mkind}")
        want = {1, 2, 3, 4, 8, 9, 10, 12, 13}
        assert want <= set(np.flatnonzero(cf.excluded).tolist()) and raw[5] == cf.excluded.sum() and (dl[sorted(want)].view(np.uint32) == 0).all()
        assert dl[5, 11] < 0 < dl[5, 40] and dl[6, 40] < 0 < dl[6, 11], "ties of the maximum"
        assert st.kernel_ms > 0.0 and float(st.accuracy) == raw[3] and float(st.weight_sum) == raw[4]


def test_c_checks_refuse_before_any_launch_and_empty():
    import torch
    from balatro_gym_amd import _native as nat, bc_loss
    L = nat.load()
    m = 70
    lg = torch.zeros((m, 64), dtype=torch.float32, device="cuda")
    dl = torch.full((m, 64), 9.0, dtype=torch.float32, device="cuda")
    mask = torch.ones((m, 60), dtype=torch.int8, device="cuda")
    a = torch.zeros(m + 2, dtype=torch.int32, device="cuda")
    w = torch.ones(m + 2, dtype=torch.float32, device="cuda")
    ix = torch.zeros(m + 2, dtype=torch.int32, device="cuda")
    lp, en = torch.zeros(m + 2, device="cuda"), torch.zeros(m + 2, device="cuda")
    stats = torch.full((8,), 9.0, device="cuda")
    need = int(L.bg_bc_loss_workspace_bytes(C.c_int64(m)))
    assert need == 16 + 8 * 1 + 32 * 2
    ws = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    good = dict(lg=lg.data_ptr(), dt=0, ls=64, mask=mask.data_ptr(), ms=60, a=a.data_ptr(), astr=4, w=w.data_ptr(), ix=ix.data_ptr(), store=m, m=m, ent=0.01,
                dl=dl.data_ptr(), ds=64, lp=lp.data_ptr(), en=en.data_ptr(), st=stats.data_ptr(), ws=ws.data_ptr(), wsb=need)

    def call(**over):
        g = dict(good)
        g.update(over)
        vp = C.c_void_p
        return L.bg_bc_loss(vp(g["lg"]), g["dt"], C.c_uint64(g["ls"]), vp(g["mask"]), C.c_uint64(g["ms"]), vp(g["a"]), C.c_uint64(g["astr"]), vp(g["w"]), vp(g["ix"]),
                            C.c_int64(g["store"]), C.c_int64(g["m"]), C.c_float(g["ent"]), vp(g["dl"]), C.c_uint64(g["ds"]), vp(g["lp"]), vp(g["en"]), vp(g["st"]),
                            vp(g["ws"]), C.c_uint64(g["wsb"]), None, vp(torch.cuda.current_stream().cuda_stream))
    assert call() == 0
    torch.cuda.synchronize()
    dl.fill_(9.0)
    stats.fill_(9.0)
    bad = [dict(dt=2), dict(m=-1), dict(ent=float("nan")), dict(ent=float("inf")), dict(lg=None), dict(lg=lg.data_ptr() + 2), dict(ls=59), dict(dl=None),
           dict(dl=dl.data_ptr() + 2), dict(ds=59), dict(mask=mask.data_ptr() + 1), dict(ms=58), dict(ms=62), dict(a=None), dict(a=a.data_ptr() + 2),
           dict(astr=0), dict(astr=2), dict(astr=6), dict(astr=2 ** 32), dict(w=w.data_ptr() + 2), dict(ix=ix.data_ptr() + 2), dict(lp=lp.data_ptr() + 2),
           dict(en=en.data_ptr() + 2), dict(store=-1), dict(store=2 ** 31), dict(st=None), dict(st=stats.data_ptr() + 2), dict(ws=None),
           dict(ws=ws.data_ptr() + 8), dict(wsb=need - 1), dict(dl=lg.data_ptr()), dict(lp=en.data_ptr()), dict(lp=w.data_ptr()), dict(st=lp.data_ptr()),
           dict(en=a.data_ptr())]
    for over in bad:
        assert call(**over) == -1, over
        assert L.bg_last_error(None).decode().startswith("bg_bc_loss: "), over
    torch.cuda.synchronize()
    assert (dl == 9.0).all() and (stats == 9.0).all(), "a refused call wrote an output"
    # m == 0: zeros to the stats, nothing else; through the wrapper an empty tensor never reaches the library
    assert call(m=0, ws=None, wsb=0) == 0
    torch.cuda.synchronize()
    assert (stats[:7] == 0.0).all() and stats[7] == 9.0 and (dl == 9.0).all()
    loss, st = bc_loss(torch.zeros((0, 60), device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"))
    assert float(loss) == 0.0 and tuple(st.dlogits.shape) == (0, 60)


def test_autograd_and_mlp_step():
    """logits.grad is dlogits and a scaled loss scales it; then a two-layer MLP (153 -> 64 tanh -> 60 logits) on 256 rows of encode_rows output,
    float32 on the GPU, takes one SGD step through bc_loss.  Its twin runs in float64 on the CPU through bc_ref.torch_statement, its logits pinned to
    the GPU's float32 values, and the parameter gradients agree within ppo_ref.mlp_gradient_bounds of bc_ref's element bounds."""
    import torch
    from balatro_gym_amd import bc_loss, encode_rows
    from tests.test_policy_head import _records as head_records
    m = 256
    rows = head_records()[384][:m].contiguous()
    host_mask = rows.cpu().numpy()[:, MASK_OFF:MASK_OFF + 60].view(np.int8)
    c0 = bc_ref.synthetic(3, m, 1.0, True, hand_made=False, mask=host_mask, weights="filter")
    lg = _dev(c0.logits).requires_grad_(True)
    loss, st = bc_loss(lg, _dev(c0.actions), rows, weights=_dev(c0.weights), ent_coef=0.01)
    (3.0 * loss).backward()
    assert torch.equal(lg.grad, st.dlogits * 3.0) and loss.requires_grad
    with torch.no_grad():
        l2, _ = bc_loss(lg, _dev(c0.actions), rows, weights=_dev(c0.weights), ent_coef=0.01)
    assert not l2.requires_grad and float(l2) == float(loss.detach())
    # the MLP
    x = encode_rows(rows, "produced", torch.float32)
    x = x / (1.0 + x.abs())
    torch.manual_seed(7)
    net = torch.nn.Sequential(torch.nn.Linear(153, 64), torch.nn.Tanh(), torch.nn.Linear(64, 60))
    twin = torch.nn.Sequential(torch.nn.Linear(153, 64), torch.nn.Tanh(), torch.nn.Linear(64, 60)).double()
    twin.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    net = net.cuda()
    logits = net(x)
    lg_host = logits.detach().cpu().numpy().copy()
    r = head_ref.Reference(lg_host, host_mask, seed=11, index0=0, t=0)
    c = bc_ref.Case(lg_host, host_mask.copy(), r.action.astype(np.int32), c0.weights, None, m)
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    before = [p.detach().clone() for p in net.parameters()]
    loss, st = bc_loss(logits, _dev(c.actions), rows, weights=_dev(c.weights), ent_coef=0.01)
    opt.zero_grad()
    loss.backward()
    grads = [p.grad.detach().cpu().numpy().astype(np.float64) for p in net.parameters()]
    opt.step()
    for p, b, g in zip(net.parameters(), before, grads):
        assert torch.allclose(p.detach(), b - 0.1 * p.grad, rtol=1e-6, atol=1e-8) and not torch.equal(p.detach(), b) and np.abs(g).sum() > 0.0
    cf = bc_ref.ClosedForm(c, 0.01)
    assert cf.excluded.sum() == 0 and cf.W > 50
    dl = st.dlogits.cpu().numpy()
    sh = cf.check(dl, st.log_prob.cpu().numpy(), st.entropy.cpu().numpy(), st.raw.cpu().numpy(), "mlp")
    x64 = x.detach().cpu().double()
    out64 = twin(x64)
    pinned = out64 + (torch.from_numpy(lg_host).double() - out64).detach()
    scal, loss64 = bc_ref.torch_statement(c, 0.01, ~cf.excluded, cf.W, params=pinned)
    loss64.backward()
    want = [p.grad.numpy() for p in twin.parameters()]
    W1, b1, W2, b2 = (p.detach().numpy() for p in twin.parameters())
    worst = ppo_ref.check_mlp_gradients(grads, want, ppo_ref.mlp_gradient_bounds(cf.grad_bound(dl), np.abs(cf.dlogits), (W1, b1), W2, x64.numpy()))
    assert abs(scal["loss"] - float(loss.detach())) <= cf.stat_bounds["loss"]
    print(f"mlp: largest share of a propagated bound {worst:.3f}; dlogits share {sh['dlogits']:.3f}")


def test_gather_past_4_gib_of_a_store():
    """A store uint8 [2 731, 4 099, 384] (4 298 637 696 bytes; tests/test_large_store.py's shape) built on the device: zeros, and 128 planted
    OBSERVATION records (their action masks) at the first 32 records, the 32 around the record that straddles byte 2**31, the 32 around the one that
    straddles 2**32 and the last 32 observation records, with the demonstrated action of each planted one step later (record + N, the last of them the
    last records of the store).  bc_loss gathers them through an index with the mask of `store[:K - 1]` and the action view of `store[1:]` read in
    place, and with dense weights; a byte offset cut to 32 bits reads a zero record (an all-invalid mask: an excluded row) and fails the bounds."""
    import torch
    from balatro_gym_amd import bc_loss
    K, N, STRIDE = 2731, 4099, 384
    R = K * N
    S = (K - 1) * N   # observation records
    B31, B32 = 2 ** 31 // STRIDE, 2 ** 32 // STRIDE
    ranges = ((0, 32), (B31 - 16, B31 + 16), (B32 - 16, B32 + 16), (S - 32, S))
    planted = np.concatenate([np.arange(a, b) for a, b in ranges])
    assert R * STRIDE > 2 ** 32 and (planted + N).max() == R - 1 and ((planted + N) * STRIDE > 2 ** 32).sum() >= 32 + 15
    c = bc_ref.synthetic(77, 128, 3.0, True, hand_made=False, weights="random")   # a compact store of the 128 planted records
    torch.cuda.empty_cache()
    store = torch.zeros((K, N, STRIDE), dtype=torch.uint8, device="cuda")   # an allocation failure is an error of the test, never a skip
    flat = store.view(R, STRIDE)
    q = torch.from_numpy(planted).cuda()
    flat[q, MASK_OFF:MASK_OFF + 60] = _dev(c.mask.view(np.uint8))
    flat[q + N, ACT_OFF:ACT_OFF + 4] = _dev(np.ascontiguousarray(c.actions).view(np.uint8).reshape(-1, 4))
    weights = torch.zeros((K - 1, N), dtype=torch.float32, device="cuda")
    weights.view(-1)[q] = _dev(c.weights)
    rng = np.random.default_rng(9)
    order = rng.permutation(128)
    idx, src = planted[order].tolist(), order.tolist()
    for pos, bad in ((31, S), (64, 2 ** 31 - 1), (130, -1)):
        idx.insert(pos, bad)
        src.insert(pos, -1)
    src = np.array(src)
    case = bc_ref.Case(c.logits[np.where(src >= 0, src, 0)].copy(), c.mask, c.actions, c.weights, np.where(src >= 0, src, 128 + (src < 0)).astype(np.int32), 128)
    case.index[130] = -1
    cf = bc_ref.ClosedForm(case, 0.01)
    assert (~cf.src_ok).sum() == 3 and cf.W > 10
    actions = store[1:, :, ACT_OFF:ACT_OFF + 4].view(torch.int32)[:, :, 0]
    assert tuple(actions.shape) == (K - 1, N) and actions.stride() == (N * 96, 96)
    loss, st = bc_loss(_dev(case.logits), actions, store[:K - 1], weights=weights, index=_dev(np.array(idx, np.int64).astype(np.int32)), ent_coef=0.01)
    torch.cuda.synchronize()
    sh = cf.check(st.dlogits.cpu().numpy(), st.log_prob.cpu().numpy(), st.entropy.cpu().numpy(), st.raw.cpu().numpy(), "past 4 GiB")
    assert float(st.excluded) == cf.excluded.sum()
    print(f"past 4 GiB: shares {sh}")
    del store, flat, actions, weights
    torch.cuda.empty_cache()
