"""bg_norm_obs_rows / bg_norm_reward_rows / bg_gae_rows_ex on the MI355X: records the product writes (300 envs, 33 steps through step_many with valid random
actions at both strides, and a fused rollout) and the synthetic set of tests/test_norm_rows_host.py.  Everything is copied to the host and compared
there (never with torch arithmetic on the GPU):
  1  the device's batch moments against numpy.mean / numpy.var(x.astype(float64), axis=0): |dmean| <= 4 N 2**-53 mean(|x|), |dvar| <= 4 N 2**-53 var,
     exactly 0.0 for a constant column -- every case, every step, every column and the returns;
  2  everything behind the reduction bit for bit: tests/norm_ref.py's `from_moments` on the host copy of the records and the device's own moments.
Also: the carry across calls, determinism, update = 0, guards and arguments, gae_rows(rewards=), RowNormalizer.
  9  past one reduction level (tests/norm_ref.py's BIG_CASES: 4 097, 8 519, 4 160 and 65 536 envs): 1 and 2, and both entry points' moments_out bit for bit
     the numpy statement of the fixed tree (norm_ref.tree_moments_obs / tree_moments_ret).

Largest observed shares of bound 1 on the MI355X at the shapes of 9: mean 0.0002, variance 0.062 (N = 65 536; 0.047 at the three smaller ones)."""
import ctypes as C

import numpy as np
import pytest

from tests import gae_ref, norm_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64
POISON = {2: 0xA5A5, 4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}
KW = ref.DEFAULTS


def _torch():
    import torch
    return torch


def _poisoned(numel, dtype):
    """A poisoned flat device buffer of `numel` + 2 GUARD elements -> (flat, the [numel] view between the guards)."""
    torch = _torch()
    flat = torch.empty(numel + 2 * GUARD, dtype=dtype, device="cuda")
    flat.view(torch.uint8).fill_(0xA5)
    return flat, flat[GUARD:GUARD + numel]


def _raw(t):
    """Device tensor -> its bit patterns on the host (uint16 / uint32 / uint64)."""
    torch = _torch()
    size = t.element_size()
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[size]
    return t.contiguous().view(it).cpu().numpy().view({2: np.uint16, 4: np.uint32, 8: np.uint64}[size])


def _guards_intact(flat, numel):
    g = _raw(flat)
    p = g.dtype.type(POISON[g.dtype.itemsize])
    return bool((g[:GUARD] == p).all() and (g[GUARD + numel:] == p).all())


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} elements differ, first {tuple(bad[0])}: {got[tuple(bad[0])]:#x} != {want[tuple(bad[0])]:#x}"


class Dev:
    """The two entry points through bare ctypes calls, every output between poisoned guards."""

    def __init__(self, state, N):
        torch = _torch()
        from balatro_gym_amd import _native as nat
        self.L, self.N = nat.load(), N
        self.fm, self.mean = _poisoned(ref.COLS, torch.float64)
        self.fv, self.var = _poisoned(ref.COLS, torch.float64)
        self.fc, self.count = _poisoned(1, torch.float64)
        self.fs, self.ret_stats = _poisoned(3, torch.float64)
        self.fr, self.returns = _poisoned(N, torch.float64)
        self.load(state)

    def load(self, s):
        torch = _torch()
        self.mean.copy_(torch.from_numpy(np.array(s["obs_mean"])))
        self.var.copy_(torch.from_numpy(np.array(s["obs_var"])))
        self.count.copy_(torch.from_numpy(np.array([s["obs_count"]])))
        self.ret_stats.copy_(torch.from_numpy(np.array([s["ret_mean"], s["ret_var"], s["ret_count"]])))
        self.returns.copy_(torch.from_numpy(np.array(s["returns"])))

    def state_bits(self):
        return {"obs_mean": _raw(self.mean), "obs_var": _raw(self.var), "obs_count": _raw(self.count), "ret_stats": _raw(self.ret_stats), "returns": _raw(self.returns)}

    def guards(self):
        return all(_guards_intact(f, n) for f, n in ((self.fm, ref.COLS), (self.fv, ref.COLS), (self.fc, 1), (self.fs, 3), (self.fr, self.N)))

    def workspace(self, K):
        torch = _torch()
        need = int(self.L.bg_norm_workspace_bytes(K, C.c_int64(self.N)))
        return torch.empty(max(need, 16), dtype=torch.uint8, device="cuda"), need

    def obs(self, rows, layout="produced", dtype="float32", update=1, pitch=None, want_out=True, want_moments=True):
        """-> (out bits [K, N, pitch] | None, moments float64 [K, 2, 153] | None, out guards intact)"""
        torch = _torch()
        from balatro_gym_amd import _native as nat
        K, N, stride = rows.shape
        D = ref.COLS if layout == "produced" else ref.FIXED_COLS
        pitch = pitch or D
        tdt = torch.float32 if dtype == "float32" else torch.bfloat16
        fo, out = _poisoned(K * N * pitch, tdt)
        fq, mom = _poisoned(K * 2 * ref.COLS, torch.float64)
        ws, need = self.workspace(K)
        rc = self.L.bg_norm_obs_rows(C.c_void_p(rows.data_ptr()), C.c_uint64(stride), K, C.c_int64(N), nat.ENC_LAYOUTS[layout], nat.ENC_F32 if dtype == "float32" else nat.ENC_BF16,
                                     C.c_void_p(self.mean.data_ptr()), C.c_void_p(self.var.data_ptr()), C.c_void_p(self.count.data_ptr()), update, C.c_double(KW["epsilon"]),
                                     C.c_double(KW["clip_obs"]), C.c_void_p(out.data_ptr()) if want_out else None, C.c_uint64(pitch),
                                     C.c_void_p(mom.data_ptr()) if want_moments and update else None, C.c_void_p(ws.data_ptr()), C.c_uint64(need), None,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, self.L.bg_last_error(None).decode()
        torch.cuda.synchronize()
        ok = _guards_intact(fo, K * N * pitch) and _guards_intact(fq, K * 2 * ref.COLS)
        if not want_out:
            ok = ok and bool((_raw(fo) == POISON[fo.element_size()]).all())
        return (_raw(out).reshape(K, N, pitch) if want_out else None,
                mom.cpu().numpy().reshape(K, 2, ref.COLS) if want_moments and update else None, ok)

    def rew(self, rows, update=1, want_out=True, want_moments=True):
        torch = _torch()
        K, N, stride = rows.shape
        fo, out = _poisoned(K * N, torch.float64)
        fq, mom = _poisoned(K * 2, torch.float64)
        ws, need = self.workspace(K)
        rc = self.L.bg_norm_reward_rows(C.c_void_p(rows.data_ptr()), C.c_uint64(stride), K, C.c_int64(N), C.c_void_p(self.returns.data_ptr()), C.c_void_p(self.ret_stats.data_ptr()),
                                        update, C.c_double(KW["gamma"]), C.c_double(KW["epsilon"]), C.c_double(KW["clip_reward"]), C.c_void_p(out.data_ptr()) if want_out else None,
                                        C.c_void_p(mom.data_ptr()) if want_moments and update else None, C.c_void_p(ws.data_ptr()), C.c_uint64(need), None,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, self.L.bg_last_error(None).decode()
        torch.cuda.synchronize()
        ok = _guards_intact(fo, K * N) and _guards_intact(fq, K * 2)
        return (_raw(out).reshape(K, N) if want_out else None, mom.cpu().numpy().reshape(K, 2) if want_moments and update else None, ok)


def _want_state_bits(s):
    return {"obs_mean": ref.bits64(s["obs_mean"]), "obs_var": ref.bits64(s["obs_var"]), "obs_count": ref.bits64([s["obs_count"]]),
            "ret_stats": ref.bits64([s["ret_mean"], s["ret_var"], s["ret_count"]]), "returns": ref.bits64(s["returns"])}


def _check_moments(mo, mr, rows_host, state, what):
    """1: the device's batch moments against numpy's, every step, every column and the returns.  Prints the worst ratio to the bound."""
    K = rows_host.shape[0]
    x = ref.produced64(rows_host)
    reward, done = gae_ref.unpack_records(rows_host)
    ret = np.array(state["returns"], np.float64)
    worst = [0.0, 0.0]
    for t in range(K):
        a, b = ref.check_moments(mo[t, 0], mo[t, 1], x[t], f"{what} step {t} obs")
        ret = ret * KW["gamma"] + reward[t]
        c, d = ref.check_moments(mr[t, 0], mr[t, 1], ret, f"{what} step {t} returns")
        ret[done[t]] = 0
        worst = [max(worst[0], a, c), max(worst[1], b, d)]
    print(f"{what}: worst |dmean| / bound {worst[0]:.4f}, worst |dvar| / bound {worst[1]:.4f}")


def _check_call(rows_dev, state, what, layouts=(("produced", "float32"), ("produced", "bfloat16"), ("fixed", "float32"), ("fixed", "bfloat16"))):
    """One call of both entry points from `state` (every layout / dtype from the same state): checks 1 and 2, guards, inputs unchanged.  Returns the
    reference's result and the device's raw outputs of the first layout."""
    rows_host = rows_dev.cpu().numpy()
    K, N, _ = rows_host.shape
    d = Dev(state, N)
    first = None
    for layout, dtype in layouts:
        d.load(state)
        out, mo, ok = d.obs(rows_dev, layout, dtype)
        assert ok and d.guards(), f"{what} {layout} {dtype}: guard elements were written"
        if first is None:
            rew, mr, ok = d.rew(rows_dev)
            assert ok and d.guards(), f"{what} reward: guard elements were written"
            _check_moments(mo, mr, rows_host, state, what)
            want = ref.from_moments(rows_host, {"obs": mo, "ret": mr}, state, **KW)
            first = (out, mo, rew, mr)
            _same(rew, ref.bits64(want["reward"]), f"{what} normalised reward")
            got_state = d.state_bits()
            for k, w in _want_state_bits(want["state"]).items():
                _same(got_state[k], w, f"{what} {k}")
        else:
            _same(ref.bits64(mo), ref.bits64(first[1]), f"{what} {layout} {dtype}: moments differ between layouts")
        _same(out, ref.obs_bits(want["obs"], layout, dtype), f"{what} normalised {layout} {dtype}")
    assert np.array_equal(rows_dev.cpu().numpy(), rows_host), f"{what}: the records were written"
    return want, first


@pytest.mark.parametrize("K", ref.SYN_K)
def test_synthetic(K):
    """The synthetic set of the host test: N in {1, 2, 63, 65, 300}, both strides, from the initial state (count = 1e-4); then the second K steps from the
    state the first call left, and 2 K steps in ONE call: the same bits (3).  The same call twice: the same bits, moments included (4)."""
    torch = _torch()
    for _, N, stride, seed in [c for c in ref.synthetic_cases() if c[0] == K]:
        rows = torch.from_numpy(ref.synthetic_rows(2 * K, N, stride, seed)).cuda()
        s0 = ref.new_state(N)
        what = f"K {K} N {N} stride {stride}"
        w1, f1 = _check_call(rows[:K], s0, what + " first call")
        w2, f2 = _check_call(rows[K:], w1["state"], what + " second call", layouts=(("produced", "float32"),))
        w, f = _check_call(rows, s0, what + " one call of 2 K", layouts=(("produced", "float32"),))
        _same(f[0], np.concatenate([f1[0], f2[0]]), what + ": two calls differ from one (obs)")
        _same(f[2], np.concatenate([f1[2], f2[2]]), what + ": two calls differ from one (reward)")
        _same(ref.bits64(f[1]), ref.bits64(np.concatenate([f1[1], f2[1]])), what + ": two calls differ from one (obs moments)")
        _same(ref.bits64(f[3]), ref.bits64(np.concatenate([f1[3], f2[3]])), what + ": two calls differ from one (return moments)")
        for k, v in _want_state_bits(w["state"]).items():
            _same(v, _want_state_bits(w2["state"])[k], what + f": final {k}")
        # determinism
        d = Dev(s0, N)
        again = d.obs(rows, "produced", "float32")[:2] + d.rew(rows)[:2]
        for a, b, name in zip(again, f, ("obs", "obs moments", "reward", "return moments")):
            _same(ref.bits64(a) if a.dtype == np.float64 else a, ref.bits64(b) if b.dtype == np.float64 else b, what + f": a second identical call differs ({name})")


@pytest.mark.parametrize("case", ref.BIG_CASES, ids=lambda c: f"K{c[0]}-N{c[1]}")
def test_past_one_reduction_level(case):
    """9: N > 4 096, where bg_norm_ret_combine's lanes fold per >= 2 wave partials each before the tree (per = 2 with one part on lane 32 and none above;
    per = 3 with a ragged last lane and a last wave of 7; per = 2 across the 16-step batch; per = 16 at 65 536 envs) and bg_norm_obs_combine walks 17,
    34 and 256 chunks (a last chunk of one record, of two tiles and 7 records, full ones).  Checks 1 and 2 as everywhere, and the fixed tree itself: both
    entry points' moments_out are tests/norm_ref.py's numpy statement of the merge order BIT FOR BIT -- a merge with its operands swapped, or one part
    folded twice in place of its neighbour, can stay inside the bound of 1.  The same call twice gives the same bits; K split over two calls gives
    the bits of one call."""
    torch = _torch()
    K, N, stride, seed = case
    rows_host = ref.synthetic_rows(K, N, stride, seed)
    rows = torch.from_numpy(rows_host).cuda()
    s0 = ref.new_state(N)
    what = f"K {K} N {N} stride {stride}"
    w, f = _check_call(rows, s0, what, layouts=(("produced", "float32"), ("fixed", "bfloat16")))
    tree = ref.tree_moments(rows_host, s0, KW["gamma"])
    _same(ref.bits64(f[1]), ref.bits64(tree["obs"]), what + ": observation moments_out against the numpy statement of the fixed tree")
    _same(ref.bits64(f[3]), ref.bits64(tree["ret"]), what + ": return moments_out against the numpy statement of the fixed tree")
    d = Dev(s0, N)
    again = d.obs(rows, "produced", "float32")[:2] + d.rew(rows)[:2]
    names = ("obs", "obs moments", "reward", "return moments")
    for a, b, name in zip(again, f, names):
        _same(ref.bits64(a) if a.dtype == np.float64 else a, ref.bits64(b) if b.dtype == np.float64 else b, what + f": a second identical call differs ({name})")
    if K > 1 and N < 10000:
        k1 = K // 2
        d = Dev(s0, N)
        p1 = d.obs(rows[:k1], "produced", "float32")[:2] + d.rew(rows[:k1])[:2]
        p2 = d.obs(rows[k1:], "produced", "float32")[:2] + d.rew(rows[k1:])[:2]
        assert d.guards()
        for a1, a2, b, name in zip(p1, p2, f, names):
            a = np.concatenate([a1, a2])
            _same(ref.bits64(a) if a.dtype == np.float64 else a, ref.bits64(b) if b.dtype == np.float64 else b, what + f": two calls differ from one ({name})")
        got_state = d.state_bits()
        for k, v in _want_state_bits(w["state"]).items():
            _same(got_state[k], v, what + f": final {k} of two calls")


@pytest.fixture(scope="module")
def product_rows():
    """300 envs, 200 steps in: 33 steps through step_many(..., obs_buffers=RowBuffers) with a valid random action per env (drawn from the live action
    mask, so one step per call) at both strides, then a fused rollout of 33 steps: {name: uint8 [33, 300, stride] on the device}."""
    torch = _torch()
    from balatro_gym_amd import BalatroVecEnv
    from balatro_gym_amd.vec_env import RowBuffers
    n, K = 300, 33
    env = BalatroVecEnv(n, [900 + i for i in range(n)], scorer_jokers=True, autoreset=True, fused_steps=8, obs_layout="rows")
    env.rollout(200, policy=0, policy_seed=11, obs_buffers=RowBuffers(n, env.device, steps=1))
    out = {}
    g = torch.Generator().manual_seed(5)
    for stride in (384, 352):
        rb = RowBuffers(n, env.device, steps=K, row_stride=stride)
        one = RowBuffers(n, env.device, steps=1, row_stride=stride)
        for t in range(K):
            mask = env.obs["action_mask"] != 0
            u = torch.rand((n, 60), generator=g).to(env.device)
            acts = torch.where(mask, u, torch.full_like(u, -1.0)).argmax(1).to(torch.int32).view(1, n).contiguous()
            env.step_many(acts, obs_buffers=one)
            rb.rows[t].copy_(one.rows[0])
        env.check()
        out[f"step_many stride {stride}"] = rb.rows
    rb = RowBuffers(n, env.device, steps=K, row_stride=384)
    done = 0
    while done < K:   # the fused rollout, max_fused_steps at a time
        T = min(env.max_fused_steps, K - done)
        part = RowBuffers(n, env.device, steps=T, row_stride=384)
        env.rollout(T, policy=0, policy_seed=12 + done, obs_buffers=part)
        rb.rows[done:done + T].copy_(part.rows)
        done += T
    env.check()
    env.close()
    out["rollout"] = rb.rows
    return out


def test_product_records(product_rows):
    """Real records, both strides and a fused rollout, from the initial state: checks 1 and 2 over all four layout / dtype pairs."""
    for name, rows in product_rows.items():
        reward, done = gae_ref.unpack_records(rows.cpu().numpy())
        print(f"{name}: {int(done.sum())} terminated steps of {done.size}, {int((reward != 0).sum())} nonzero rewards")
        _check_call(rows.contiguous(), ref.new_state(rows.shape[1]), name)


def test_update_0_and_frozen_state():
    """5: update = 0 normalises with the statistics as given -- bit for bit the reference with frozen statistics -- and writes neither them nor the carry."""
    torch = _torch()
    K, N = 17, 65
    state = ref.vecnormalize(ref.synthetic_rows(9, N, 384, 98), ref.new_state(N))["state"]
    assert state["returns"].any()
    rows_host = ref.synthetic_rows(K, N, 352, 99)
    rows = torch.from_numpy(rows_host).cuda()
    want = ref.from_moments(rows_host, None, state, training=False, **KW)
    d = Dev(state, N)
    before = d.state_bits()
    for layout, dtype in (("produced", "float32"), ("produced", "bfloat16"), ("fixed", "float32"), ("fixed", "bfloat16")):
        out, _, ok = d.obs(rows, layout, dtype, update=0)
        assert ok and d.guards()
        _same(out, ref.obs_bits(want["obs"], layout, dtype), f"update 0 {layout} {dtype}")
    rew, _, ok = d.rew(rows, update=0)
    assert ok and d.guards()
    _same(rew, ref.bits64(want["reward"]), "update 0 reward")
    for k, v in d.state_bits().items():
        _same(v, before[k], f"update 0 wrote {k}")


def test_strides_null_outputs_and_bad_arguments():
    """6: out_stride_elems > cols keeps the poison in the extra columns (16-byte rows, odd rows, one element per lane), == cols is the dense matrix; out_dev / rewards_dev NULL update the
    statistics only; every bad argument returns BG_E_ARG with a message and writes nothing."""
    torch = _torch()
    from balatro_gym_amd import _native as nat
    K, N = 3, 65
    rows_host = ref.synthetic_rows(K, N, 384, 123)
    rows = torch.from_numpy(rows_host).cuda()
    s0 = ref.new_state(N)
    d = Dev(s0, N)
    out, mo, ok = d.obs(rows)
    rew, mr, ok2 = d.rew(rows)
    want = ref.from_moments(rows_host, {"obs": mo, "ret": mr}, s0, **KW)
    full = d.state_bits()
    for layout, dtype, pitch in (("produced", "float32", 156), ("produced", "float32", 155), ("produced", "bfloat16", 160), ("produced", "bfloat16", 157),
                                 ("fixed", "float32", 633), ("fixed", "bfloat16", 632),
                                 # dense: rows that are not 16-byte aligned run across row ends; [m, 628] float32 has 2 512-byte rows, so it is stored by rows
                                 ("produced", "bfloat16", 153), ("fixed", "float32", 628), ("fixed", "bfloat16", 628)):
        d.load(s0)
        wide, _, ok = d.obs(rows, layout, dtype, pitch=pitch)
        D = ref.COLS if layout == "produced" else ref.FIXED_COLS
        assert ok
        _same(wide[:, :, :D], ref.obs_bits(want["obs"], layout, dtype), f"pitch {pitch} {layout} {dtype}")
        assert (wide[:, :, D:] == POISON[wide.dtype.itemsize]).all(), f"pitch {pitch}: columns beyond the layout were written"
    # an output whose base is not 16-byte aligned: one element per lane
    d.load(s0)
    fo, o = _poisoned(K * N * ref.COLS + 1, torch.float32)
    ws, need = d.workspace(K)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def obs(rows_p=rows.data_ptr(), stride=384, k=K, n=N, layout=0, dt=0, mean_p=d.mean.data_ptr(), var_p=d.var.data_ptr(), count_p=d.count.data_ptr(), update=1,
            out_p=o.data_ptr() + 4, pitch=ref.COLS, mom_p=None, ws_p=ws.data_ptr(), ws_n=need, ms=None):
        return d.L.bg_norm_obs_rows(C.c_void_p(rows_p), C.c_uint64(stride), k, C.c_int64(n), layout, dt, C.c_void_p(mean_p), C.c_void_p(var_p), C.c_void_p(count_p), update,
                                    C.c_double(1e-8), C.c_double(10.0), C.c_void_p(out_p), C.c_uint64(pitch), C.c_void_p(mom_p), C.c_void_p(ws_p), C.c_uint64(ws_n), ms, st)
    assert obs() == 0
    torch.cuda.synchronize()
    _same(_raw(o[1:]).reshape(K, N, ref.COLS), ref.obs_bits(want["obs"]), "misaligned out_dev")
    assert _guards_intact(fo, K * N * ref.COLS + 1) and _raw(o[:1])[0] == POISON[4]
    # NULL outputs: the statistics only
    d.load(s0)
    assert d.obs(rows, want_out=False, want_moments=False)[2] and d.rew(rows, want_out=False, want_moments=False)[2]
    for k, v in d.state_bits().items():
        _same(v, full[k], f"NULL outputs: {k}")
    # bad arguments
    d.load(s0)
    before = d.state_bits()
    fo, o = _poisoned(K * N * ref.COLS, torch.float32)
    fq, mom = _poisoned(K * 2 * ref.COLS, torch.float64)
    ms = C.c_float(-1.0)
    good = dict(out_p=o.data_ptr(), ms=C.byref(ms))
    for kw in (dict(layout=nat.ENC_EXTRACTOR), dict(layout=7), dict(dt=2), dict(rows_p=rows.data_ptr() + 8), dict(rows_p=None), dict(stride=336), dict(stride=360), dict(stride=0),
               dict(k=-1), dict(n=-1), dict(ws_n=need - 1), dict(ws_p=None), dict(ws_p=ws.data_ptr() + 8), dict(update=0, mom_p=mom.data_ptr()), dict(mean_p=None),
               dict(var_p=d.var.data_ptr() + 4), dict(count_p=None), dict(out_p=o.data_ptr() + 2), dict(pitch=152), dict(mom_p=mom.data_ptr() + 4), dict(var_p=d.mean.data_ptr())):
        assert obs(**dict(good, **kw)) == -1, kw
        assert d.L.bg_last_error(None).decode().startswith("bg_norm_obs_rows: "), kw
    fr, r = _poisoned(K * N, torch.float64)

    def rew(rows_p=rows.data_ptr(), stride=384, k=K, n=N, carry_p=d.returns.data_ptr(), stats_p=d.ret_stats.data_ptr(), update=1, out_p=r.data_ptr(), mom_p=None,
            ws_p=ws.data_ptr(), ws_n=need):
        return d.L.bg_norm_reward_rows(C.c_void_p(rows_p), C.c_uint64(stride), k, C.c_int64(n), C.c_void_p(carry_p), C.c_void_p(stats_p), update, C.c_double(0.99), C.c_double(1e-8),
                                       C.c_double(10.0), C.c_void_p(out_p), C.c_void_p(mom_p), C.c_void_p(ws_p), C.c_uint64(ws_n), C.byref(ms), st)
    for kw in (dict(rows_p=rows.data_ptr() + 8), dict(stride=336), dict(stride=360), dict(k=-1), dict(n=-1), dict(ws_n=need - 1), dict(ws_p=None), dict(update=0, mom_p=mom.data_ptr()),
               dict(carry_p=None), dict(stats_p=None), dict(out_p=r.data_ptr() + 4), dict(out_p=d.returns.data_ptr())):
        assert rew(**kw) == -1, kw
        assert d.L.bg_last_error(None).decode().startswith("bg_norm_reward_rows: "), kw
    torch.cuda.synchronize()
    for f in (fo, fq, fr):
        assert bool((_raw(f) == POISON[f.element_size()]).all()), "a refused call wrote an output"
    for k, v in d.state_bits().items():
        _same(v, before[k], f"a refused call wrote {k}")
    assert ms.value == -1.0 and d.guards()
    # K == 0 / N == 0: no-ops; kernel_ms_out of a good call
    assert obs(**dict(good, k=0)) == 0 and ms.value == 0.0 and obs(**dict(good, n=0)) == 0 and rew(k=0) == 0 and rew(n=0) == 0
    torch.cuda.synchronize()
    assert bool((_raw(fo) == POISON[4]).all()) and bool((_raw(fr) == POISON[8]).all())
    for k, v in d.state_bits().items():
        _same(v, before[k], f"a no-op wrote {k}")
    assert obs(**good) == 0 and ms.value > 0.0
    ms.value = -1.0
    assert rew() == 0 and ms.value > 0.0
    torch.cuda.synchronize()
    _same(_raw(o).reshape(K, N, ref.COLS), ref.obs_bits(want["obs"]), "the good call behind the refused ones")
    _same(_raw(r).reshape(K, N), ref.bits64(want["reward"]), "the good reward call behind the refused ones")


def test_gae_rows_takes_the_normalised_rewards():
    """7: gae_rows(rewards=) is tests/gae_ref.py's loop fed those rewards, bit for bit; without the argument the result is what it was."""
    torch = _torch()
    from balatro_gym_amd import RowNormalizer, gae_rows
    from balatro_gym_amd.vec_env import RowBuffers
    for K, N, stride in ((33, 65, 352), (17, 300, 384), (1, 1, 384)):
        rows_host = ref.synthetic_rows(K, N, stride, 500 + K)
        rows = torch.from_numpy(rows_host).cuda()
        values, last_values = gae_ref.synthetic_values(K, N, 77)
        v, lv = torch.from_numpy(values).cuda(), torch.from_numpy(last_values).cuda()
        nr = RowNormalizer(N, "cuda").normalize_reward(rows)
        nr_host = nr.cpu().numpy()
        reward, done = gae_ref.unpack_records(rows_host)
        assert (nr_host != reward).any()
        want_a, want_r = gae_ref.gae(nr_host, done, values, last_values, 0.99, 0.95)
        a, r = gae_rows(rows, v, lv, 0.99, 0.95, rewards=nr)
        _same(_raw(a), gae_ref.bits32(want_a), f"K {K} N {N}: advantages from the normalised rewards")
        _same(_raw(r), gae_ref.bits32(want_r), f"K {K} N {N}: returns from the normalised rewards")
        want_a, want_r = gae_ref.gae(reward, done, values, last_values, 0.99, 0.95)
        a, r = gae_rows(rows, v, lv, 0.99, 0.95)
        _same(_raw(a), gae_ref.bits32(want_a), f"K {K} N {N}: advantages without the argument")
        _same(_raw(r), gae_ref.bits32(want_r), f"K {K} N {N}: returns without the argument")
        rb = RowBuffers(N, torch.device("cuda"), steps=K, row_stride=stride)
        rb.rows.copy_(rows)
        a2, r2 = rb.gae(v, lv, rewards=rb.normalize_reward(RowNormalizer(N, "cuda")))
        a3, _ = gae_rows(rows, v, lv, 0.99, 0.95, rewards=nr)
        assert torch.equal(a2.view(torch.int32), a3.view(torch.int32))
    # the raw call refuses rewards_dev that is misaligned or an output
    from balatro_gym_amd import _native as nat
    L = nat.load()
    adv, ret = torch.zeros((K, N), device="cuda"), torch.zeros((K, N), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for rp in (nr.data_ptr() + 4, adv.data_ptr()):
        assert L.bg_gae_rows_ex(C.c_void_p(rows.data_ptr()), C.c_uint64(stride), K, C.c_int64(N), C.c_void_p(v.data_ptr()), C.c_void_p(lv.data_ptr()), C.c_double(0.99),
                                C.c_double(0.95), C.c_void_p(adv.data_ptr()), C.c_void_p(ret.data_ptr()), C.c_void_p(rp), None, st) == -1
        assert L.bg_last_error(None).decode().startswith("bg_gae_rows_ex: ")


def test_row_normalizer():
    """8: RowNormalizer is the two calls with the state it owns; a state_dict round trip reproduces the next call's bits; training=False leaves the state
    untouched; [N, stride] rows are [1, N, stride]; RowBuffers.normalize / normalize_reward forward."""
    torch = _torch()
    from balatro_gym_amd import RowNormalizer
    from balatro_gym_amd.vec_env import RowBuffers
    K, N = 17, 65
    rows_host = ref.synthetic_rows(2 * K + 1, N, 384, 31)
    rows = torch.from_numpy(rows_host).cuda()
    nm = RowNormalizer(N, "cuda")
    o1, ms = nm.normalize_obs(rows[:K], timing=True)
    r1 = nm.normalize_reward(rows[:K])
    assert ms > 0.0 and tuple(o1.shape) == (K, N, 153) and o1.dtype == torch.float32 and tuple(r1.shape) == (K, N) and r1.dtype == torch.float64
    d = Dev(ref.new_state(N), N)
    out, mo, _ = d.obs(rows[:K])
    rew, mr, _ = d.rew(rows[:K])
    _same(_raw(o1), out, "RowNormalizer.normalize_obs")
    _same(_raw(r1), rew, "RowNormalizer.normalize_reward")
    want = ref.from_moments(rows_host[:K], {"obs": mo, "ret": mr}, ref.new_state(N), **KW)
    _same(_raw(nm.obs_mean), ref.bits64(want["state"]["obs_mean"]), "RowNormalizer.obs_mean")
    _same(_raw(nm.returns), ref.bits64(want["state"]["returns"]), "RowNormalizer.returns")
    # the round trip
    sd = nm.state_dict()
    other = RowNormalizer(N, "cuda")
    other.load_state_dict(sd)
    a = (nm.normalize_obs(rows[K:2 * K], "fixed", torch.bfloat16), nm.normalize_reward(rows[K:2 * K]))
    b = (other.normalize_obs(rows[K:2 * K], "fixed", torch.bfloat16), other.normalize_reward(rows[K:2 * K]))
    assert tuple(a[0].shape) == (K, N, 628) and a[0].dtype == torch.bfloat16
    _same(_raw(b[0]), _raw(a[0]), "after load_state_dict: obs")
    _same(_raw(b[1]), _raw(a[1]), "after load_state_dict: reward")
    for name in ("obs_mean", "obs_var", "obs_count", "ret_stats", "returns"):
        _same(_raw(getattr(other, name)), _raw(getattr(nm, name)), f"after load_state_dict: {name}")
    # [N, stride] is one step
    c1, c2 = RowNormalizer(N, "cuda"), RowNormalizer(N, "cuda")
    c1.load_state_dict(sd); c2.load_state_dict(sd)
    x1, x2 = c1.normalize_obs(rows[2 * K]), c2.normalize_obs(rows[2 * K:2 * K + 1])
    y1, y2 = c1.normalize_reward(rows[2 * K]), c2.normalize_reward(rows[2 * K:2 * K + 1])
    assert tuple(x1.shape) == (N, 153) and tuple(y1.shape) == (N,)
    _same(_raw(x1), _raw(x2[0]), "[N, stride] obs")
    _same(_raw(y1), _raw(y2[0]), "[N, stride] reward")
    _same(_raw(c1.obs_var), _raw(c2.obs_var), "[N, stride] state")
    # training=False
    frozen = RowNormalizer(N, "cuda", training=False)
    frozen.load_state_dict(dict(sd, training=False))
    state_now = {k: _raw(getattr(frozen, k)).copy() for k in ("obs_mean", "obs_var", "obs_count", "ret_stats", "returns")}
    rb = RowBuffers(N, torch.device("cuda"), steps=K, row_stride=384)
    rb.rows.copy_(rows[K:2 * K])
    out = torch.empty((K, N, 153), device="cuda")
    fo = rb.normalize(frozen, out=out)
    fr = rb.normalize_reward(frozen)
    assert fo.data_ptr() == out.data_ptr()
    st = {"obs_mean": sd["obs_mean"].numpy(), "obs_var": sd["obs_var"].numpy(), "obs_count": sd["obs_count"].numpy()[0], "ret_mean": sd["ret_stats"].numpy()[0],
          "ret_var": sd["ret_stats"].numpy()[1], "ret_count": sd["ret_stats"].numpy()[2], "returns": sd["returns"].numpy()}
    want = ref.from_moments(rows_host[K:2 * K], None, st, training=False, **KW)
    _same(_raw(fo), ref.obs_bits(want["obs"]), "training=False obs")
    _same(_raw(fr), ref.bits64(want["reward"]), "training=False reward")
    for k, v in state_now.items():
        _same(_raw(getattr(frozen, k)), v, f"training=False wrote {k}")
    frozen.reset_returns(torch.arange(N, device="cuda") % 2 == 0)
    assert not frozen.returns[0::2].any() and torch.equal(frozen.returns[1::2], nm.returns.new_tensor(sd["returns"].numpy()[1::2]))
