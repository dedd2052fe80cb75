"""bg_get_states / bg_set_states / bg_copy_states on the GPU (csrc/bg_snapshot.h): many envs' state in one launch, the blobs on the device.
Blob bytes against bg_get_state with a sliced refill pending; restore with fan-out, fork across handles and a copy inside one handle at the
shallowest rings, each continued against the C oracle record byte for record byte (a forked env on its source's actions IS the unforked
trajectory; forks on other actions are fresh oracle envs replayed over the source's prefix); card states; every refusal.  200 and 70 envs,
the helpers and the shared oracle rollout of tests/test_state_layout_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from tests.helpers import OBS_KEYS
from tests.test_state_layout_gpu import ENV_INDEX0, N, POLICY, PSEED, _assert_records, _oracle, _setup, _vec

pytestmark = pytest.mark.gpu

NB = 70
KG, KS, KD = 8, 13, 12
L5, K4 = 5, 4
T0 = L5 * K4


def _shallow(monkeypatch):
    monkeypatch.setenv("BG_KG", str(KG)); monkeypatch.setenv("BG_KS", str(KS)); monkeypatch.setenv("BG_KD", str(KD))
    monkeypatch.setenv("BG_REFILL_SLICED", "1")


def _handle_a():
    """The 200-env handle of test_state_blob_between_handles_of_other_sizes_vs_oracle after four 5-step rollouts: the fourth asked for a refill,
    whose dense kernels are still to be issued in pieces."""
    from balatro_gym_amd.vec_env import RowBuffers
    seeds, jokers = _setup()
    A = _vec(N, seeds, scorer_jokers=True, autoreset=True, max_ante=4)
    assert L5 <= A.max_fused_steps // 2 and L5 * K4 > A.max_fused_steps, A.max_fused_steps
    A.inject(jokers=jokers, apply_now=True)
    rb = RowBuffers(N, A.device, steps=L5)
    for j in range(K4):
        A.rollout(L5, policy=POLICY, policy_seed=PSEED, env_index0=ENV_INDEX0, t0=L5 * j, obs_buffers=rb, zero_stats=(j == 0))
    return A


def _handle_b():
    return _vec(NB, [9 + i for i in range(NB)], scorer_jokers=True, autoreset=True, max_ante=4)


def _actions_for(wa, rows, cols_of, n, torch, device):
    """int32 [len(rows), n]: column c takes the oracle's recorded actions of env cols_of.get(c, c % N)."""
    a = np.stack([wa[rows, cols_of.get(c, c % N)] for c in range(n)], axis=1).astype(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def test_blob_bytes_with_a_refill_pending_vs_get_state(monkeypatch):
    import torch
    from balatro_gym_amd.vec_env import BalatroVecEnv, RowBuffers
    _shallow(monkeypatch)
    A = _handle_a()
    envs = [199, 0, 64, 63, 199]
    nb = int(A._L.bg_state_blob_bytes(A._h))
    stride = A.state_blob_stride
    assert stride % 16 == 0 and 0 <= stride - nb < 16
    out = torch.full((len(envs), stride), 0xA5, dtype=torch.uint8, device=A.device)
    got = A.get_states(envs, out=out)          # FIRST: it has to issue the pending pieces itself
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (len(envs), stride)
    got = got.cpu().numpy()
    for i, e in enumerate(envs):
        want = np.frombuffer(A.get_state(e), np.uint8)
        assert want.size == nb == 16 + 128 + 64 + 112 + 32 + KD * 64 + KG * 2560 + KS * 256 + 3 * 2560 + 128 * 4 + 4 + 4
        assert np.array_equal(got[i, :nb], want), f"blob {i} (env {e}) differs from bg_get_state at byte {int(np.argmax(got[i, :nb] != want))}"
        assert (got[i, nb:] == 0xA5).all(), f"blob {i}: padding written"
    parsed = BalatroVecEnv.parse_state_blob(A.get_states([64])[0])
    assert parsed["KD"] == KD and parsed["KS"] == KS and parsed["KG"] == KG and parsed["version"] == 7
    allb = A.get_states()
    assert tuple(allb.shape) == (N, stride) and not allb[:, nb:].any(), "get_states' own rows end in zero padding"
    assert np.array_equal(allb[199, :nb].cpu().numpy(), got[0, :nb]) and np.array_equal(allb[63, :nb].cpu().numpy(), got[3, :nb])
    M = 60
    rb = RowBuffers(N, A.device, steps=M)
    A.rollout(M, policy=POLICY, policy_seed=PSEED, env_index0=ENV_INDEX0, t0=T0, obs_buffers=rb, zero_stats=True)
    A.check()
    wobs, wr, wt, wa, _ = _oracle(T0 + M)
    _assert_records(rb, slice(None), (wobs, wr, wt, wa), slice(T0, T0 + M), slice(None), "the handle the blobs were taken from")
    A.close()


def test_restore_with_fan_out_vs_oracle(monkeypatch):
    import torch
    from balatro_gym_amd.vec_env import RowBuffers
    _shallow(monkeypatch)
    A = _handle_a()
    src = [199, 0, 64, 63, 199]
    blobs = A.get_states(src)
    nb = int(A._L.bg_state_blob_bytes(A._h))
    assert torch.equal(blobs[0], blobs[4]), "the two copies of env 199 differ"
    B, B2 = _handle_b(), _handle_b()
    before1 = B.get_state(1)
    dst, bidx = [0, 69, 5, 64], [0, 0, 2, 3]
    B.set_states(dst, blobs, blob_index=bidx)
    assert B.get_state(1) == before1, "an env that was not restored changed"
    for d, b in zip(dst, bidx):
        B2.set_state(d, bytes(blobs[b, :nb].cpu().numpy().tobytes()))
    assert torch.equal(B.get_states()[:, :nb], B2.get_states()[:, :nb]), "set_states and four set_state calls leave different handles"
    # the live observation follows (observe=True): the restored env shows its source's record
    A.observe()
    assert torch.equal(B.obs["hand"][0], A.obs["hand"][199]) and torch.equal(B.obs["money"][5], A.obs["money"][64])
    M = 60
    wobs, wr, wt, wa, _ = _oracle(T0 + M)
    source = {d: src[b] for d, b in zip(dst, bidx)}
    rb = RowBuffers(NB, B.device, steps=M)
    B.step_many(_actions_for(wa, slice(T0, T0 + M), source, NB, torch, B.device), obs_buffers=rb)
    B.check()
    for d, s in source.items():
        _assert_records(rb, d, (wobs, wr, wt, wa), slice(T0, T0 + M), s, f"env {d} restored from env {s}")
    assert torch.equal(rb.rows[:, 0], rb.rows[:, 69]), "two envs restored from one blob on the same actions diverge"
    A.close(); B.close(); B2.close()


def _replicas(e, prefix, first_actions, steps):
    """Fresh oracle envs replayed over env e's recorded prefix (resets and jokers as _oracle does them), then one step with first_actions[k],
    then `steps` steps of the oracle's own policy with env index ENV_INDEX0 + k.  Returns (obs, reward, terminated, actions) as [1 + steps, K]."""
    from oracle import pyoracle as po
    seeds, jokers = _setup()
    Kn, T = len(first_actions), 1 + steps
    rew, term, acts = np.zeros((T, Kn)), np.zeros((T, Kn), np.uint8), np.zeros((T, Kn), np.int32)
    cols = []
    for k in range(Kn):
        o = po.OracleEnv(seeds[e], scorer_jokers=True, max_ante=4)
        o.set_jokers(jokers[e])
        for a in prefix:
            if o.step(int(a))[2]:
                o.reset(); o.set_jokers(jokers[e])
        col = []
        for t in range(T):
            a = int(first_actions[k]) if t == 0 else o.policy_action(POLICY, PSEED, ENV_INDEX0 + k, T0 + t)
            _, r, tm, _, _ = o.step(a)
            if tm:
                o.reset(); o.set_jokers(jokers[e])
            col.append(o.obs())
            rew[t, k], term[t, k], acts[t, k] = r, tm, a
        cols.append(col)
    wobs = {key: np.stack([np.stack([cols[k][t][key] for k in range(Kn)]) for t in range(T)]) for key in OBS_KEYS}
    return wobs, rew, term, acts


def test_look_ahead_across_handles_vs_oracle(monkeypatch):
    import torch
    from balatro_gym_amd.vec_env import RowBuffers
    _shallow(monkeypatch)
    A = _handle_a()
    B = _handle_b()
    e, Kn, S = 64, 60, 30
    _, _, _, wa, _ = _oracle(T0)
    wobs, wr, wt, wact = _replicas(e, wa[:T0, e], list(range(Kn)), S)
    assert len(set(wr[0].tolist())) > 1 or len({tuple(wobs["hand"][0, k]) for k in range(Kn)}) > 1, "the 60 actions all lead to one state"
    assert len({tuple(wact[1:, k]) for k in range(Kn)}) > Kn // 2, "the branches do not draw differently"
    B.copy_states(range(Kn), [e] * Kn, source=A)
    A.observe()
    assert torch.equal(B.obs["hand"][:Kn], A.obs["hand"][e].expand(Kn, -1)), "observe=True: the forks show the source's hand"
    pad = np.zeros((1 + S, NB - Kn), np.int32)
    acts = torch.from_numpy(np.ascontiguousarray(np.concatenate([wact, pad], axis=1))).to(B.device)
    rb1, rbS = RowBuffers(NB, B.device, steps=1), RowBuffers(NB, B.device, steps=S)
    B.step_many(acts[:1], obs_buffers=rb1)
    _assert_records(rb1, slice(0, Kn), (wobs, wr, wt, wact), slice(0, 1), slice(None), "the 60 one-step branches")
    B.step_many(acts[1:], obs_buffers=rbS)
    B.check(); A.check()
    _assert_records(rbS, slice(0, Kn), (wobs, wr, wt, wact), slice(1, 1 + S), slice(None), "the 60 branches, 30 steps on")
    A.close(); B.close()


def test_copy_inside_one_handle_at_the_shallowest_rings_vs_oracle(monkeypatch):
    """BG_KD = 2, BG_KS = 3: a refill every 3 steps, an env's two ring slots written and consumed over and over.  No top-up is forced by a copy inside
    one handle, so the ring slots, the producer word in both buffers and the handle's own refill schedule all sit behind the 720 steps that follow
    (240 step_many calls of 3 steps: the length at which, by the oracle alone, enough envs have been through their ring several times)."""
    import torch
    from balatro_gym_amd.vec_env import RowBuffers
    kd, ks, T1, T2, H = 2, 3, 30, 720, 100
    monkeypatch.setenv("BG_KD", str(kd)); monkeypatch.setenv("BG_KS", str(ks))
    wobs, wr, wt, wa, _ = _oracle(T1 + T2)
    assert int((wt[T1:T1 + T2, :H].sum(axis=0) > 2 * kd).sum()) * 4 >= 3 * H, "too few envs consume their deck ring several times over"
    seeds, jokers = _setup()
    env = _vec(N, seeds, scorer_jokers=True, autoreset=True, max_ante=4)
    env.inject(jokers=jokers, apply_now=True)
    assert env.max_fused_steps == 3
    one = RowBuffers(N, env.device, steps=3)
    for t in range(0, T1, 3):
        env.rollout(3, policy=POLICY, policy_seed=PSEED, env_index0=ENV_INDEX0, t0=t, obs_buffers=one, zero_stats=(t == 0))
    env.copy_states(range(H, 2 * H), range(H))
    acts = _actions_for(wa, slice(T1, T1 + T2), {j + H: j for j in range(H)}, N, torch, env.device)
    rb = RowBuffers(N, env.device, steps=T2)
    for t in range(0, T2, 3):
        env.step_many(acts[t:t + 3], obs_buffers=one)
        rb.rows[t:t + 3].copy_(one.rows)
    env.check()
    want = (wobs, wr, wt, wa)
    _assert_records(rb, slice(0, H), want, slice(T1, T1 + T2), slice(0, H), "the sources")
    _assert_records(rb, slice(H, 2 * H), want, slice(T1, T1 + T2), slice(0, H), "the copies")
    env.close()


def test_card_states_bytes_and_fan_out():
    import random
    import torch
    from balatro_gym_amd.vec_env import BalatroVecEnv, RowBuffers
    n, T = 64, 20
    cards = [[(idx, random.Random(50 * i + idx).randrange(9), random.Random(70 * i + idx).randrange(4), random.Random(90 * i + idx).randrange(5))
              for idx in random.Random(i).sample(range(52), 12)] for i in range(n)]
    A = _vec(n, [4100 + 3 * i for i in range(n)], scorer_jokers=True, autoreset=True, max_ante=4, card_states=True, fused_steps=16)
    B = _vec(n, [77 + i for i in range(n)], scorer_jokers=True, autoreset=True, max_ante=4, card_states=True, fused_steps=16)
    A.inject_cards(cards)
    rbA = RowBuffers(n, A.device, steps=T)
    A.rollout(T, policy=POLICY, policy_seed=PSEED, env_index0=0, t0=0, obs_buffers=rbA)
    envs = [63, 0, 31, 63]
    nb, stride = int(A._L.bg_state_blob_bytes(A._h)), A.state_blob_stride + 128
    out = torch.full((len(envs), stride), 0xA5, dtype=torch.uint8, device=A.device)
    got = A.get_states(envs, out=out).cpu().numpy()
    for i, e in enumerate(envs):
        assert np.array_equal(got[i, :nb], np.frombuffer(A.get_state(e), np.uint8)), f"blob {i} (env {e}) differs from bg_get_state"
        assert (got[i, nb:] == 0xA5).all(), f"blob {i}: padding written"
    p = BalatroVecEnv.parse_state_blob(out[2])
    assert p["card_states"].size == 56 and p["card_template"].any() and p["KD"] == 12   # (the parser's "card_states" is the slice: 7 chunks of eight u16)
    dst, bidx = [3, 40, 63], [0, 0, 2]
    B.set_states(dst, out, blob_index=bidx)
    A.rollout(T, policy=POLICY, policy_seed=PSEED, env_index0=0, t0=T, obs_buffers=rbA)
    acts = rbA.action.clone()                      # B's column d takes the actions A's policy gave the source
    for d, b in zip(dst, bidx):
        acts[:, d] = rbA.action[:, envs[b]]
    rbB = RowBuffers(n, B.device, steps=T)
    B.step_many(acts.contiguous(), obs_buffers=rbB)
    A.check(); B.check()
    for d, b in zip(dst, bidx):
        assert torch.equal(rbB.rows[:, d], rbA.rows[:, envs[b]]), f"env {d} restored from env {envs[b]} leaves its source's trajectory"
    A.close(); B.close()


def test_refusals(monkeypatch):
    import torch
    from balatro_gym_amd import _native as nat
    A = _vec(NB, [300 + i for i in range(NB)], fused_steps=16)
    B = _vec(8, [500 + i for i in range(8)], fused_steps=16)
    monkeypatch.setenv("BG_KD", "14")   # (deeper: its blobs are larger, so they pass for their stride and fail for their header)
    D = _vec(8, [600 + i for i in range(8)], fused_steps=16)
    monkeypatch.delenv("BG_KD")
    stride, nb = A.state_blob_stride, int(A._L.bg_state_blob_bytes(A._h))
    blobs = A.get_states([0, 1, 2, 3])
    snap = lambda: A.get_states()[:, :nb]
    before = snap()

    def refused(prefix, call):
        with pytest.raises(nat.NativeError) as ei:
            call()
        assert prefix in str(ei.value), str(ei.value)
        assert torch.equal(snap(), before), f"{prefix} changed the handle although it refused"

    flat = torch.zeros(4 * stride + 16, dtype=torch.uint8, device=A.device)
    bad_magic = blobs.clone(); bad_magic[2, 0] ^= 0xFF
    bad_version = blobs.clone(); bad_version[1, 4] = 6
    other_depth = D.get_states([0])
    i32 = lambda *v: np.asarray(v, np.int32)
    raw = lambda f, *a: (lambda: A._check(f(*a), f.__name__))
    vp, idx4 = C.c_void_p, i32(0, 1, 2, 3)
    p4, pb = idx4.ctypes.data_as(vp), vp(blobs.data_ptr())
    for prefix, call in [
            ("bg_get_states: env_index[1] = 70 out of range", lambda: A.get_states([0, NB])),
            ("bg_get_states: env_index[0] = -1 out of range", lambda: A.get_states([-1])),
            ("bg_get_states: blob_stride_bytes", lambda: A.get_states([0], out=torch.zeros((1, stride - 16), dtype=torch.uint8, device=A.device))),
            ("bg_get_states: blob_stride_bytes", lambda: A.get_states([0], out=torch.zeros((1, stride + 8), dtype=torch.uint8, device=A.device))),
            ("bg_get_states: blobs_dev must be 16-byte aligned", lambda: A.get_states([0, 1], out=flat[8:8 + 2 * stride].view(2, stride))),
            ("bg_get_states: m = -1", raw(A._L.bg_get_states, A._h, p4, -1, pb, C.c_uint64(stride), None)),
            ("bg_get_states: null blobs_dev", raw(A._L.bg_get_states, A._h, p4, 4, None, C.c_uint64(stride), None)),
            ("bg_set_states: env_index[1] = 70 out of range", lambda: A.set_states([5, NB], blobs)),
            ("bg_set_states: env_index[2] = 5 is listed twice", lambda: A.set_states([5, 6, 5], blobs)),
            ("bg_set_states: blob_index[1] = 4 out of range", lambda: A.set_states([5, 6], blobs, blob_index=[0, 4])),
            ("bg_set_states: blob_index[0] = -1 out of range", lambda: A.set_states([5], blobs, blob_index=[-1])),
            ("bg_set_states: fewer blobs than envs", lambda: A.set_states([5, 6, 7, 8, 9], blobs)),
            ("bg_set_states: blob 2 is not a state blob", lambda: A.set_states([5, 6], bad_magic, blob_index=[0, 2])),
            ("bg_set_states: blob 1 has version 6", lambda: A.set_states([5, 6], bad_version, blob_index=[1, 0])),
            ("bg_set_states: blob 0 was saved with ring depths", lambda: A.set_states([5], other_depth)),
            ("bg_set_states: blob_stride_bytes", lambda: A.set_states([5], blobs[:, :stride - 16].contiguous())),
            ("bg_set_states: null index list", raw(A._L.bg_set_states, A._h, None, 4, pb, C.c_uint64(stride), 4, None, None)),
            ("bg_set_states: null blobs_dev", raw(A._L.bg_set_states, A._h, p4, 4, None, C.c_uint64(stride), 4, None, None)),
            ("bg_set_states: m = -2", raw(A._L.bg_set_states, A._h, p4, -2, pb, C.c_uint64(stride), 4, None, None)),
            ("bg_copy_states: dst_index[1] = 70 out of range", lambda: A.copy_states([5, NB], [0, 1])),
            ("bg_copy_states: src_index[0] = 8 out of range", lambda: A.copy_states([5], [8], source=B)),
            ("bg_copy_states: dst_index[1] = 5 is listed twice", lambda: A.copy_states([5, 5], [0, 1])),
            ("bg_copy_states: env 5 (src_index[1]) is written by another pair", lambda: A.copy_states([5, 6], [0, 5])),
            ("bg_copy_states: env 1 (src_index[0]) is written by another pair", lambda: A.copy_states([0, 1], [1, 0])),
            ("bg_copy_states: the source handle has ring depths", lambda: A.copy_states([5], [0], source=D)),
            ("bg_copy_states: null index list", raw(A._L.bg_copy_states, A._h, p4, A._h, None, 4, None)),
            ("bg_copy_states: null source handle", raw(A._L.bg_copy_states, A._h, p4, None, p4, 4, None)),
            ("bg_copy_states: m = -1", raw(A._L.bg_copy_states, A._h, p4, A._h, p4, -1, None))]:
        refused(prefix, call)
    # accepted edge cases: m == 0, a pair onto itself beside a fork of the same env, a source env of another handle with the same depths
    A.set_states([], blobs); A.copy_states([], []); assert tuple(A.get_states([]).shape) == (0, stride)
    A.copy_states([5, 6], [5, 5])
    after = snap()
    assert torch.equal(after[6], before[5]) and torch.equal(after[5], before[5]) and torch.equal(after[7:], before[7:]) and torch.equal(after[:5], before[:5])
    A.copy_states([9], [7], source=B)
    assert torch.equal(A.get_states([9])[0, :nb], B.get_states([7])[0, :nb])
    A.check(); A.close(); B.close(); D.close()
