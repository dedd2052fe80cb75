"""The learner operators over ONE store of records that reaches past 2**31 and past 2**32 bytes, on the MI355X: uint8 [K = 2 731, N = 4 099, 384], that is
R = 11 194 369 records and 4 298 637 696 bytes -- the smallest shape class at which a byte offset held in 32 bits (signed or unsigned) wraps.  Every
`(size_t)record * stride` and every `index[i]` gather of bg_encode_rows_ex, bg_ppo_loss, bg_gae_rows(_ex), bg_episode_stats_rows and bg_norm_reward_rows
runs here on such offsets.  The store is built on the device (never 4 GB on the host): zeros, the reward field and the terminated byte of every record from
tests/gae_ref.py's synthetic arrays, and 128 PLANTED records -- tests/encode_ref.py's synthetic records (every dtype at its limits, random bytes; the action
mask reduced to the 0 / 1 the env writes) -- at the first 32 records, the 32 around the record that straddles byte 2**31, the 32 around the one that
straddles 2**32 and the last 32.  The planted records are read back once; that host copy is the reference's input.  Everything is compared on the host,
bit for bit with the numpy restatements (tests/encode_ref.py, norm_ref.py, gae_ref.py) or, for bg_ppo_loss, by tests/ppo_ref.py's bounds; a truncated
offset reads a zero record (or another planted one) and fails them.  Outputs sit between poisoned guards; the planted records are unchanged at the end
of every test.

Out of scope here, because their outputs alone would be many GB: the contiguous encode_rows, normalize_obs and the policy head over all R rows.

Largest observed shares of the bounds on the MI355X: the return moments of the 2 731 steps 0.0001 (mean) and 0.0006 (variance) of 4 N 2**-53; bg_ppo_loss
dlogits 0.021, dvalues 0.41, policy_loss 0.0009, approx_kl 0.00008, entropy_loss 0.007, value_loss 0.024, loss 0.0014, adv_mean 0.15, adv_std 0.16,
log_prob 0.055, entropy 0.029, clip_fraction 0.12.  Everything else is bit for bit."""
import numpy as np
import pytest

from tests import encode_ref, gae_ref, norm_ref, ppo_ref


K, N, STRIDE = 2731, 4099, 384
R = K * N
B31, B32 = 2 ** 31 // STRIDE, 2 ** 32 // STRIDE
RANGES = ((0, 32), (B31 - 16, B31 + 16), (B32 - 16, B32 + 16), (R - 32, R))
PLANTED = np.concatenate([np.arange(a, b) for a, b in RANGES])
MASK_OFF, MASK_END = 176, 236
KW = norm_ref.DEFAULTS


def test_the_shape_reaches_what_it_claims():
    assert R == 11194369 and R * STRIDE == 4298637696 > 2 ** 32
    assert B31 == 5592405 and B31 * STRIDE < 2 ** 31 < (B31 + 1) * STRIDE and B32 == 11184810 and B32 * STRIDE < 2 ** 32 < (B32 + 1) * STRIDE
    assert len(PLANTED) == 128 == len(set(PLANTED.tolist())) and PLANTED.max() == R - 1 < 2 ** 31 - 1
    # the low 32 bits of a byte offset past 2**32 are no multiple of the stride: a truncated offset reads no whole record, planted or not
    assert ((PLANTED[PLANTED > B32] * STRIDE) % 2 ** 32 % STRIDE == 128).all() and (PLANTED > B32).sum() == 15 + 32


@pytest.fixture(scope="module")
def big():
    import torch
    torch.cuda.empty_cache()
    store = torch.zeros((K, N, STRIDE), dtype=torch.uint8, device="cuda")   # an allocation failure is an error of the test, never a skip
    reward = gae_ref.synthetic_rewards(K, N, 4242)
    done = gae_ref.synthetic_done(K, N, "random", 4243)
    store[:, :, gae_ref.ROW_REWARD:gae_ref.ROW_REWARD + 8] = torch.from_numpy(reward).cuda().view(torch.uint8).view(K, N, 8)
    store[:, :, gae_ref.ROW_TERMINATED] = torch.from_numpy(done).cuda()
    planted = encode_ref.pack_records(encode_ref.synthetic_obs(n_random=128 - 17, seed=515), STRIDE).copy()
    assert planted.shape == (128, STRIDE)
    planted[:, MASK_OFF:MASK_END] &= 1   # the action mask as the env writes it: 0 / 1
    planted[:, gae_ref.ROW_REWARD:gae_ref.ROW_REWARD + 8] = np.ascontiguousarray(reward.reshape(-1)[PLANTED]).view(np.uint8).reshape(128, 8)
    planted[:, gae_ref.ROW_TERMINATED] = done.reshape(-1)[PLANTED]
    flat = store.view(R, STRIDE)
    pd = torch.from_numpy(planted).cuda()
    for i, (a, b) in enumerate(RANGES):
        flat[a:b] = pd[32 * i:32 * i + 32]
    torch.cuda.synchronize()
    host = torch.cat([flat[a:b] for a, b in RANGES]).cpu().numpy()
    assert np.array_equal(host, planted), "the planted records did not arrive where they were put"
    hr, hd = gae_ref.unpack_records(host[None])
    assert np.array_equal(gae_ref.bits64(hr[0]), gae_ref.bits64(reward.reshape(-1)[PLANTED])) and np.array_equal(hd[0], done.reshape(-1)[PLANTED] != 0)
    spot = np.array([33, B31 + 20, B32 - 40, R - 33, 7 * N + 5])   # records that are not planted: zeros but for the two fields
    got = flat[torch.from_numpy(spot).cuda()].cpu().numpy()
    sr, _ = gae_ref.unpack_records(got[None])
    assert np.array_equal(gae_ref.bits64(sr[0]), gae_ref.bits64(reward.reshape(-1)[spot])) and np.array_equal(got[:, gae_ref.ROW_TERMINATED], done.reshape(-1)[spot])
    assert not got[:, :gae_ref.ROW_REWARD].any() and not got[:, MASK_OFF:MASK_END].any()
    box = {"store": store, "host": host, "reward": reward, "done": done != 0}
    yield box
    box.pop("store")
    del store, flat
    torch.cuda.empty_cache()


def _unchanged(big):
    import torch
    flat = big["store"].view(R, STRIDE)
    now = torch.cat([flat[a:b] for a, b in RANGES]).cpu().numpy()
    assert np.array_equal(now, big["host"]), "the planted records of the store were written"


def _helpers():
    from tests import test_norm_rows as t
    return t._poisoned, t._guards_intact, t._raw


def _frozen_state():
    st = norm_ref.vecnormalize(norm_ref.synthetic_rows(9, 65, 384, 98), norm_ref.new_state(65))["state"]
    assert (st["obs_var"] != 1.0).any() and (st["obs_mean"] != 0.0).any()
    return st


def _gather_index(seed):
    """The planted record numbers, shuffled, plus R, 2**31 - 1 and -1 at positions inside the run -> (int64 [131] record numbers, rows of the host copy or -1)."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(128)
    idx = PLANTED[order].tolist()
    src = order.tolist()
    for pos, bad in ((31, R), (64, 2 ** 31 - 1), (130, -1)):
        idx.insert(pos, bad)
        src.insert(pos, -1)
    return np.array(idx, np.int64), np.array(src, np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["float32", "bfloat16"])
@pytest.mark.parametrize("layout", encode_ref.LAYOUTS)
def test_gather_across_the_boundaries(big, layout, dt):
    """encode_rows(index=) with and without frozen statistics: output row i is record index[i], bit for bit the numpy restatement on the host copy; a row
    whose index is out of range is +0.0."""
    import torch
    from balatro_gym_amd import RowNormalizer, encode_rows
    poisoned, guards_intact, raw = _helpers()
    idx, src = _gather_index(7)
    ok = src >= 0
    assert ((idx >= 0) & (idx < R)).tolist() == ok.tolist() and (~ok).sum() == 3
    index = torch.from_numpy(idx.astype(np.int32)).cuda()
    m, D = len(idx), encode_ref.COLS[layout]
    tdt = getattr(torch, dt)
    rows_host = big["host"][np.where(ok, src, 0)]
    cases = [(None, encode_ref.expected_bits(layout, encode_ref.unpack_records(rows_host)))]
    if layout != "extractor":
        st = _frozen_state()
        nm = RowNormalizer(N, "cuda", training=False)
        nm.obs_mean.copy_(torch.from_numpy(st["obs_mean"]))
        nm.obs_var.copy_(torch.from_numpy(st["obs_var"]))
        nm.obs_count.fill_(float(st["obs_count"]))
        with np.errstate(all="ignore"):
            want = norm_ref.from_moments(rows_host[None], None, st, training=False, **KW)
        cases.append((nm, norm_ref.obs_bits(want["obs"][0], layout)))
    for nm, want32 in cases:
        want32 = np.where(ok[:, None], want32, np.uint32(0))
        want = want32 if dt == "float32" else encode_ref.bf16_bits(want32)
        flat, out = poisoned(m * D, tdt)
        res = encode_rows(big["store"], layout, tdt, out=out.view(m, D), index=index, norm=nm)
        torch.cuda.synchronize()
        assert res.data_ptr() == out.data_ptr() and guards_intact(flat, m * D), f"{layout} {dt}: guard elements were written"
        got = raw(out).reshape(m, D)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (f"{layout} {dt} norm {nm is not None}: {len(bad)} elements differ, first (row, column) {tuple(bad[0])} of record {idx[bad[0][0]]}: "
                               f"{got[tuple(bad[0])]:#x} != {want[tuple(bad[0])]:#x}")
        assert not got[~ok].any()
        if nm is not None:
            assert np.array_equal(raw(nm.obs_mean), norm_ref.bits64(st["obs_mean"])) and np.array_equal(raw(nm.obs_var), norm_ref.bits64(st["obs_var"]))
    assert np.array_equal(index.cpu().numpy(), idx.astype(np.int32))
    _unchanged(big)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["f32", "bf16"])
def test_ppo_loss_gathers_across_the_boundaries(big, layout):
    """bg_ppo_loss with an index over the R stored rows: masks read in place from the store's records, actions / old log-probs / advantages / returns from
    [R] arrays that are zero but at the planted positions.  The reference is tests/ppo_ref.py's closed form over the compact 128-row store made of the
    host copy; the index repeats rows and holds one out-of-range entry."""
    import torch
    from balatro_gym_amd import evaluate_actions
    from tests.test_ppo_loss import COEF, _Call, _bits
    bf16 = layout == "bf16"
    m = 300
    host_mask = np.ascontiguousarray(big["host"][:, MASK_OFF:MASK_END]).view(np.int8)
    c = ppo_ref.synthetic(900 + bf16, m, 1.0, True, index="repeat", hand_made=False, bf16=bf16, mask=host_mask, store_rows=128)
    c.index[5] = 128                        # out of range in the compact store, R on the device
    assert np.array_equal(c.mask, host_mask) and len(set(c.index.tolist())) < m and all(((c.index >= 32 * i) & (c.index < 32 * i + 32)).any() for i in range(4))
    ok = c.index < 128
    dev_index = torch.from_numpy(np.where(ok, PLANTED[np.where(ok, c.index, 0)], R).astype(np.int32)).cuda()
    at = torch.from_numpy(PLANTED).cuda()
    stored = {}
    for name, a in (("actions", c.actions), ("old", c.old_log_prob), ("adv", c.advantages), ("returns", c.returns)):
        t = torch.zeros(R, dtype=torch.int32 if name == "actions" else torch.float32, device="cuda")
        t[at] = torch.from_numpy(a).cuda()
        stored[name] = t
    before = {k: v.clone() for k, v in stored.items()}
    call = _Call(c, None, 0, 60, layout)
    over = dict(mask=big["store"].data_ptr() + MASK_OFF, ms=STRIDE, index=dev_index.data_ptr(), store=R, **{k: v.data_ptr() for k, v in stored.items()})
    assert call.run(**over) == 0, call.L.bg_last_error(None)
    dl, dv, lp, en, st = call.fetch()
    what = f"ppo_loss over the large store {layout}"
    if bf16:
        f32 = _Call(c, None, 0, 60, "f32")
        assert f32.run(**over) == 0
        dl32, dv32, lp32, en32, st32 = f32.fetch()
        from tests import head_ref
        assert np.array_equal(dl, head_ref.bf16_bits(dl32)), what + ": bf16 dlogits is not the rounding of the float32 call's"
        for x, y in ((dv, dv32), (lp, lp32), (en, en32), (st, st32)):
            assert np.array_equal(_bits(x), _bits(y)), what
        dl = dl32
    cf = ppo_ref.ClosedForm(c, COEF[0], COEF[1], COEF[2], True, True)
    shares = cf.check(dl, dv, lp, en, st, what, cap=False)
    print(f"{what}: shares of the bounds {shares}")
    assert st[9] == m and st[8] == cf.excluded.sum() >= 1 and cf.excluded[5]
    gok, mk, a, _, _, _ = c.gathered()
    elp, een = evaluate_actions(torch.from_numpy(c.logits).cuda(), torch.from_numpy(a).cuda(), torch.from_numpy(mk).cuda())
    assert np.array_equal(_bits(lp)[gok], _bits(elp.cpu().numpy())[gok]) and np.array_equal(_bits(en)[gok], _bits(een.cpu().numpy())[gok]), what
    for k, v in stored.items():
        assert torch.equal(v.view(torch.int32), before[k].view(torch.int32)), f"{what}: stored {k} was written"
    _unchanged(big)


def _diff(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} elements differ, first (t, env) {tuple(bad[0])}: {got[tuple(bad[0])]:#x} != {want[tuple(bad[0])]:#x}"


@pytest.mark.gpu
def test_gae_over_the_whole_store(big):
    """gae_rows and gae_rows(rewards=) over all [K, N] records: bit for bit tests/gae_ref.py's loop."""
    import torch
    from balatro_gym_amd import gae_rows
    from tests.test_gae_rows import _guarded, _guards_intact, _ints
    values, last_values = gae_ref.synthetic_values(K, N, 77)
    v, lv = torch.from_numpy(values).cuda(), torch.from_numpy(last_values).cuda()
    other = gae_ref.synthetic_rewards(K, N, 4343)
    od = torch.from_numpy(other).cuda()
    for name, rewards, rd in (("records' rewards", big["reward"], None), ("rewards=", other, od)):
        want_a, want_r = gae_ref.gae(rewards, big["done"], values, last_values, 0.99, 0.95)
        fa, adv = _guarded(K, N, torch.float32)
        fr, ret = _guarded(K, N, torch.float32)
        gae_rows(big["store"], v, lv, 0.99, 0.95, advantages=adv, returns=ret, rewards=rd)
        _diff(_ints(adv), gae_ref.bits32(want_a), f"large store, {name}: advantages")
        _diff(_ints(ret), gae_ref.bits32(want_r), f"large store, {name}: returns")
        assert _guards_intact(fa, K, N) and _guards_intact(fr, K, N), f"{name}: guard elements were written"
    assert np.array_equal(_ints(v), gae_ref.bits32(values)) and np.array_equal(_ints(lv), gae_ref.bits32(last_values)) and np.array_equal(_ints(od), gae_ref.bits64(other))
    _unchanged(big)


@pytest.mark.gpu
def test_episode_stats_over_the_whole_store(big):
    """EpisodeStats.update in one call and split at K // 3: bit for bit tests/gae_ref.py's scan, carries included."""
    import torch
    from balatro_gym_amd import EpisodeStats
    from tests.test_gae_rows import _guarded, _guards_intact, _ints
    want_r, want_l, want_cr, want_cl = gae_ref.episode_stats(big["reward"], big["done"])
    for split in (None, K // 3):
        st = EpisodeStats(N, big["store"].device)
        fr, er = _guarded(K, N, torch.float64)
        fl, el = _guarded(K, N, torch.int32)
        if split is None:
            st.update(big["store"], ep_return=er, ep_len=el)
        else:
            st.update(big["store"][:split], ep_return=er[:split], ep_len=el[:split])
            st.update(big["store"][split:], ep_return=er[split:], ep_len=el[split:])
        what = f"large store, split {split}"
        _diff(_ints(er), gae_ref.bits64(want_r), what + ": ep_return")
        _diff(_ints(el).view(np.int32), want_l, what + ": ep_len")
        assert np.array_equal(_ints(st.ep_return_carry), gae_ref.bits64(want_cr)) and np.array_equal(st.ep_len_carry.cpu().numpy(), want_cl), what + ": carries"
        assert _guards_intact(fr, K, N) and _guards_intact(fl, K, N), what + ": guard elements were written"
        assert int(el.sum()) + int(st.ep_len_carry.sum()) == K * N
    _unchanged(big)


@pytest.mark.gpu
def test_reward_normaliser_over_the_whole_store(big):
    """bg_norm_reward_rows over all [K, N] records from the initial state: the device's moments of every step within the bound of numpy's and bit for bit
    the numpy statement of the fixed tree (65 waves: per = 2); the normalised rewards, the statistics and the carry bit for bit behind them."""
    import torch
    from tests.test_norm_rows import Dev, _raw
    s0 = norm_ref.new_state(N)
    d = Dev(s0, N)
    before = d.state_bits()
    rew, mr, ok = d.rew(big["store"])
    assert ok and d.guards(), "guard elements were written"
    with np.errstate(all="ignore"):
        rets, carry = norm_ref.returns_of(big["reward"], big["done"], s0["returns"], KW["gamma"])
    worst = [0.0, 0.0]
    for t in range(K):
        a, b = norm_ref.check_moments(mr[t, 0], mr[t, 1], rets[t], f"large store step {t} returns")
        worst = [max(worst[0], a), max(worst[1], b)]
    print(f"large store: worst |dmean| / bound {worst[0]:.4f}, worst |dvar| / bound {worst[1]:.4f}")
    tree = np.stack(norm_ref.tree_moments_ret(rets), axis=-1)
    _diff(norm_ref.bits64(mr), norm_ref.bits64(tree), "large store: return moments_out against the numpy statement of the fixed tree")
    want = norm_ref.reward_from_moments(big["reward"], big["done"], mr, s0, KW["gamma"], KW["epsilon"], KW["clip_reward"])
    _diff(rew, norm_ref.bits64(want["reward"]), "large store: normalised reward")
    got = d.state_bits()
    s = want["state"]
    assert np.array_equal(got["ret_stats"], norm_ref.bits64([s["ret_mean"], s["ret_var"], s["ret_count"]])), "large store: ret_stats"
    _diff(got["returns"], norm_ref.bits64(s["returns"]), "large store: returns carry")
    assert np.array_equal(norm_ref.bits64(carry), norm_ref.bits64(s["returns"]))
    for k in ("obs_mean", "obs_var", "obs_count"):
        assert np.array_equal(got[k], before[k]), f"the reward call wrote {k}"
    # RowNormalizer.normalize_reward is that call with the state it owns
    from balatro_gym_amd import RowNormalizer
    nm = RowNormalizer(N, "cuda")
    _diff(_raw(nm.normalize_reward(big["store"])), rew, "large store: RowNormalizer.normalize_reward")
    assert np.array_equal(_raw(nm.ret_stats), got["ret_stats"]) and np.array_equal(_raw(nm.returns), got["returns"])
    # a second, frozen pass reads the same records with the statistics as they stand
    rew0, _, ok = d.rew(big["store"], update=0)
    frozen = norm_ref.reward_from_moments(big["reward"], big["done"], None, s, KW["gamma"], KW["epsilon"], KW["clip_reward"], training=False)
    assert ok
    _diff(rew0, norm_ref.bits64(frozen["reward"]), "large store: normalised reward, update = 0")
    _unchanged(big)
