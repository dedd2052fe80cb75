"""bg_encode_rows on the MI355X: records the product writes (rollout at both strides, step_many) and the synthetic records of tests/encode_ref.py through
all three layouts and both dtypes; records and outputs are copied to the host and compared, bit pattern for bit pattern over every element, with the numpy
restatement (never with torch arithmetic on the GPU).  Then the store paths (aligned rows, dense-but-unaligned rows, element stores), the edges of m,
the argument checks of the C entry point, and BalatroSB3VecEnv(features="fixed") against the reference's own wrappers (sb3_fixed.npz)."""
import ctypes as C

import numpy as np
import pytest

from tests import encode_ref as ref

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "bfloat16")


def _bits(t):
    """A float32 / bfloat16 device tensor -> its bit patterns on the host (uint32 / uint16)."""
    import torch
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _want(layout, dtype, rows_host):
    w = ref.expected_bits(layout, ref.unpack_records(rows_host))
    return w if dtype == "float32" else ref.bf16_bits(w)


def _check_records(rows_dev, what):
    """rows_dev: uint8 [..., stride] on the device.  All layouts x dtypes against numpy over the host copy of the same bytes."""
    import torch
    from balatro_gym_amd import encode_rows
    host = rows_dev.cpu().numpy().reshape(-1, rows_dev.shape[-1])
    for layout in ref.LAYOUTS:
        for dt in DTYPES:
            got = encode_rows(rows_dev, layout, getattr(torch, dt))
            assert tuple(got.shape) == tuple(rows_dev.shape[:-1]) + (ref.COLS[layout],) and got.is_contiguous()
            g, w = _bits(got).reshape(len(host), -1), _want(layout, dt, host)
            bad = np.argwhere(g != w)
            assert bad.size == 0, f"{what} {layout} {dt}: {len(bad)} of {w.size} elements differ, first (record, column) {tuple(bad[0])}: {g[tuple(bad[0])]:#x} != {w[tuple(bad[0])]:#x}"


def _env(n, **kw):
    from balatro_gym_amd import BalatroVecEnv
    return BalatroVecEnv(n, [900 + i for i in range(n)], scorer_jokers=True, autoreset=True, **kw)


@pytest.mark.parametrize("stride", [384, 352])
def test_rollout_records(stride):
    """[max_fused_steps, 4096] records of a fused rollout, at the fast stride and densely packed."""
    from balatro_gym_amd.vec_env import RowBuffers
    n = 4096
    env = _env(n, fused_steps=8)
    T = env.max_fused_steps
    rb = RowBuffers(n, env.device, steps=T, row_stride=stride)
    env.rollout(T, policy=0, policy_seed=11, obs_buffers=rb)
    env.check()
    assert int(rb.action.max()) > 0
    _check_records(rb.rows, f"rollout stride {stride}")
    # RowBuffers.encode is the same call
    import torch
    from balatro_gym_amd import encode_rows
    assert torch.equal(rb.encode("extractor", torch.bfloat16).view(torch.int16), encode_rows(rb.rows, "extractor", torch.bfloat16).view(torch.int16))
    env.close()


def test_step_many_records_and_live_features():
    """A [K, N] buffer of step_many with the caller's actions; BalatroVecEnv.features equals encode_rows(env.obs_rows)."""
    import torch
    from balatro_gym_amd import encode_rows
    from balatro_gym_amd.vec_env import RowBuffers
    n, K = 1000, 12
    env = _env(n, fused_steps=16, obs_layout="rows")
    rb = RowBuffers(n, env.device, steps=K, row_stride=384)
    g = torch.Generator().manual_seed(5)
    acts = torch.randint(0, 60, (K, n), generator=g, dtype=torch.int32).to(env.device)
    env.step_many(acts, obs_buffers=rb)
    env.check()
    _check_records(rb.rows, "step_many")
    _check_records(env.obs_rows, "live records")
    for layout in ref.LAYOUTS:
        for dt in (torch.float32, torch.bfloat16):
            assert np.array_equal(_bits(env.features(layout, dt)), _bits(encode_rows(env.obs_rows, layout, dt))), (layout, dt)
    keys = _env(8)
    with pytest.raises(ValueError, match="obs_layout='rows'"):
        keys.features("fixed")
    keys.close()
    env.close()


def test_synthetic_records():
    """Every field at the limits of its dtype, chips_scored around 2**24 / 2**31 / 2**53 / int64 min and max, 10 000 records of random bytes."""
    import torch
    obs = ref.synthetic_obs()
    for stride in (384, 352):
        rows = torch.from_numpy(ref.pack_records(obs, stride)).cuda()
        _check_records(rows, f"synthetic stride {stride}")


def test_store_paths_and_edges_of_m():
    """`out` wider than D keeps its sentinel beyond column D; aligned rows (16-byte stores per row), dense unaligned rows (16-byte stores across rows) and
    an odd pitch (element stores) give the same values; m = 0, 1, 31, 32, 33 and a count that is no multiple of the workgroup's 32 records."""
    import torch
    from balatro_gym_amd import encode_rows
    obs = ref.synthetic_obs(n_random=300)
    rows_all = torch.from_numpy(ref.pack_records(obs, 384)).cuda()
    host_all = rows_all.cpu().numpy()
    for m in (0, 1, 31, 32, 33, 301):
        rows, host = rows_all[:m], host_all[:m]
        for layout in ref.LAYOUTS:
            D = ref.COLS[layout]
            for dt in DTYPES:
                tdt = getattr(torch, dt)
                want = _want(layout, dt, host) if m else np.zeros((0, D), np.uint32 if dt == "float32" else np.uint16)
                es = 4 if dt == "float32" else 2
                aligned = (D + 16 + 7) // 8 * 8                # row pitch a multiple of 16 bytes in both dtypes
                odd = D + 3 if (D + 3) * es % 16 else D + 5    # rows not 16-byte aligned, matrix not dense: element stores
                assert aligned * es % 16 == 0 and odd * es % 16 != 0
                sentinel = _bits(torch.full((1,), -7.0, dtype=tdt))[0]
                for pitch in (D, aligned, odd):
                    out = torch.full((m, pitch), -7.0, dtype=tdt, device="cuda")
                    res = encode_rows(rows, layout, tdt, out=out)
                    assert res.data_ptr() == out.data_ptr() and tuple(res.shape) == (m, D)
                    got = _bits(out)
                    assert np.array_equal(got[:, :D], want), (m, layout, dt, pitch)
                    assert (got[:, D:] == sentinel).all(), f"columns beyond {D} were written (m {m}, {layout}, {dt}, pitch {pitch})"
                # a matrix that starts 4 (f32) / 2 (bf16) bytes off a 16-byte boundary: dense, but element stores
                flat = torch.full((m * D + 8,), -7.0, dtype=tdt, device="cuda")
                out = flat[1:1 + m * D].view(m, D)
                encode_rows(rows, layout, tdt, out=out)
                got = _bits(flat)
                assert np.array_equal(got[1:1 + m * D].reshape(m, D), want) and (got[0] == sentinel) and (got[1 + m * D:] == sentinel).all(), (m, layout, dt, "offset")
    # [K, N, stride] rows with a [K, N, pitch] out: leading dimensions collapse to m = K * N
    rows3 = rows_all[:300].view(3, 100, 384)
    out3 = torch.zeros((3, 100, 160), device="cuda")
    r3 = encode_rows(rows3, "produced", out=out3)
    assert tuple(r3.shape) == (3, 100, 153) and np.array_equal(_bits(r3).reshape(300, 153), _want("produced", "float32", host_all[:300]))
    _, ms = encode_rows(rows_all, "fixed", timing=True)
    assert ms > 0.0


def test_bad_arguments_launch_nothing():
    """BG_E_ARG with a text for a bad layout, dtype, stride < 352, stride not a multiple of 16, misaligned rows_dev, out_stride_elems < D, misaligned
    out_dev, negative m and NULL pointers; `out` keeps its sentinel through all of them."""
    import torch
    from balatro_gym_amd import _native as nat
    L = nat.load()
    m = 64
    rows = torch.zeros((m + 1, 384), dtype=torch.uint8, device="cuda")
    out = torch.full((m, 640), -7.0, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rp, op = rows.data_ptr(), out.data_ptr()
    ms = C.c_float(-1.0)

    def call(rows_p=rp, stride=384, mm=m, layout=nat.ENC_FIXED, dt=nat.ENC_F32, out_p=op, pitch=640):
        return L.bg_encode_rows(C.c_void_p(rows_p), C.c_uint64(stride), C.c_int64(mm), layout, dt, C.c_void_p(out_p), C.c_uint64(pitch), C.byref(ms), st)
    bad = [dict(layout=3), dict(layout=-1), dict(dt=2), dict(dt=-1), dict(stride=336), dict(stride=360), dict(stride=0), dict(rows_p=rp + 8), dict(rows_p=None),
           dict(out_p=None), dict(pitch=627), dict(pitch=0), dict(out_p=op + 2), dict(dt=nat.ENC_BF16, out_p=op + 1), dict(mm=-1),
           dict(layout=nat.ENC_PRODUCED, pitch=152), dict(layout=nat.ENC_EXTRACTOR, pitch=446)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert L.bg_last_error(None).decode().startswith("bg_encode_rows: "), kw
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and ms.value == -1.0
    assert [L.bg_encode_cols(i) for i in (0, 1, 2, 3, -1)] == [153, 628, 447, -1, -1]
    assert call(mm=0) == 0 and ms.value == 0.0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert call() == 0 and ms.value > 0.0
    assert bool((out[:, :628] == 0).all()) and bool((out[:, 628:] == -7.0).all())


@pytest.mark.parametrize("as_torch", [False, True])
def test_sb3_features_fixed_vs_reference_wrappers(as_torch):
    """BalatroSB3VecEnv(features="fixed") replays sb3_fixed.npz (the reference's SafeBalatroEnv(BalatroEnvFixed(seed + rank)), as
    tests/test_gpu_parity.py::test_sb3_adapter_vs_reference_wrappers does for the dict path): every returned matrix equals the fixture's 51 keys flattened
    and concatenated; rewards, dones, the wrapper's info flags and the terminal observations as in the fixture."""
    from balatro_gym_amd.sb3_adapter import BalatroSB3VecEnv
    g = ref.sb3_fixture()
    S, T = g["actions"].shape
    want0 = ref.sb3_fixed_bits(g, "obs0_", (S,))
    want = ref.sb3_fixed_bits(g, "obs_", (S, T)).reshape(S, T, 628)
    term = ref.sb3_fixed_bits(g, "term_", (S, T)).reshape(S, T, 628)
    venv = BalatroSB3VecEnv(S, seed=int(g["seed0"]), max_invalid_actions=int(g["max_invalid_actions"]), max_episode_steps=int(g["max_episode_steps"]),
                            features="fixed", as_torch=as_torch)
    space = venv.observation_space
    assert tuple(getattr(space, "shape", None) or space[1]) == (628,)

    def host(x):
        if as_torch:
            assert x.is_cuda and x.dtype.is_floating_point
            x = x.cpu().numpy()
        assert x.dtype == np.float32 and x.shape == (S, 628)
        return x.view(np.uint32)
    assert np.array_equal(host(venv.reset()), want0)
    wrapper_ends = game_overs = 0
    for t in range(T):
        obs, rew, done, infos = venv.step(g["actions"][:, t])
        if as_torch:
            rew, done = rew.cpu().numpy(), done.cpu().numpy()
        ctx = f"t {t}"
        assert np.array_equal(host(obs), want[:, t]), ctx
        assert rew.dtype == np.float32 and np.array_equal(rew.view(np.uint32), g["rewards"][:, t].view(np.uint32)), ctx
        assert np.array_equal(done, g["dones"][:, t].astype(bool)), ctx
        for i in range(S):
            assert bool(infos[i].get("invalid_action_termination")) == bool(g["invalid_action_termination"][i, t]), (ctx, i)
            assert bool(infos[i].get("max_steps_reached")) == bool(g["max_steps_reached"][i, t]), (ctx, i)
            if done[i]:
                assert infos[i]["TimeLimit.truncated"] == bool(g["truncated"][i, t] and not g["invalid_action_termination"][i, t]), (ctx, i)
                if g["invalid_action_termination"][i, t] or (g["truncated"][i, t] and not g["terminated"][i, t]):
                    wrapper_ends += 1
                    tob = infos[i]["terminal_observation"]
                    assert tob.dtype == np.float32 and np.array_equal(tob.view(np.uint32), term[i, t]), f"{ctx} env {i}: terminal_observation"
                else:
                    game_overs += 1
                    assert "terminal_observation" not in infos[i]
    assert wrapper_ends > 100 and game_overs > 10, (wrapper_ends, game_overs)
    venv.close()
    # the other two layouts: one matrix of the right width from the same wrapper
    for layout in ("produced", "extractor"):
        v = BalatroSB3VecEnv(16, seed=3, features=layout)
        o = v.reset()
        assert o.shape == (16, ref.COLS[layout]) and o.dtype == np.float32
        assert np.array_equal(o.view(np.uint32), _want(layout, "float32", v.env.obs_rows.cpu().numpy()))
        v.close()
