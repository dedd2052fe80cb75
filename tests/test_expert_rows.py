"""bg_expert_actions on the MI355X, bit for bit against tests/expert_ref.py: the synthetic set of the host test tiled with records of a uniform-policy
rollout (selections in arbitrary states, shops, boss blinds) at m = 1, 63, 64, 65, 257 and 1025 (below, at and above a wave and a workgroup of every
lane mapping), strides 352 and 384, with and without an index (out-of-range, negative and repeated entries), with and without the detail word; a
collection loop of 300 steps of expert_act() -> step() over 256 envs, every action compared; the same actions again through step_many(limits=) into a
store, then episode_outcomes -> DemoBuffer.add -> bc_loss with one-hot logits, whose accuracy must be exactly 1; outputs poisoned before each call, the
records unchanged after it, two calls identical; every refusal of the C checks."""
import ctypes as C

import numpy as np
import pytest

from tests import expert_ref as ref
from tests.helpers import poison_

pytestmark = pytest.mark.gpu

N_ENVS, LOOP_STEPS, ROLLOUT_STEPS = 256, 300, 24
SIZES = (1, 63, 64, 65, 257, 1025)


def _dev(x):
    import torch
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.fixture(scope="module")
def pool():
    """uint8 [n, 384] records -- the synthetic set, then ROLLOUT_STEPS x 256 records of bg_rollout_rows under BG_POLICY_UNIFORM -- with the
    restatement's (actions, detail) on them, computed once."""
    import torch
    from balatro_gym_amd import BalatroVecEnv, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers
    names, synth, want_s = ref.synthetic_rows(384)
    env = BalatroVecEnv(N_ENVS, [9100 + i for i in range(N_ENVS)], scorer_jokers=True, autoreset=True, obs_layout="rows")
    rb = RowBuffers(N_ENVS, env.device, steps=ROLLOUT_STEPS, row_stride=384)
    env.rollout(ROLLOUT_STEPS, policy=nat.POLICY_UNIFORM, policy_seed=5, obs_buffers=rb)
    env.check()
    real = rb.rows.reshape(-1, 384).cpu().numpy()
    env.close()
    want_r = ref.expert_rows(real)
    phases = np.bincount(real[:, 339].astype(np.int8).astype(np.int64), minlength=4)
    selected = int((real[:, :64].reshape(-1, 8, 8).any(axis=2).sum(axis=1) > 0).sum())
    print(f"pool: {len(synth)} synthetic + {len(real)} rollout records; rollout phases {phases.tolist()}, {selected} with a selection, "
          f"{int((real[:, 340] != 0).sum())} under a boss blind")
    assert phases[0] > 0 and phases[1] > 0 and phases[2] > 0 and selected > 100
    rows = np.concatenate([synth, real])
    return {"rows": rows, "want": (np.concatenate([want_s[0], want_r[0]]), np.concatenate([want_s[1], want_r[1]])), "n_synth": len(synth)}


def _take(pool, m, stride):
    """m records of the pool, tiled in an order that puts synthetic and rollout records side by side -> (rows [m, stride], want actions, want detail)."""
    n = len(pool["rows"])
    pick = (np.arange(m, dtype=np.int64) * 7919 + m) % n
    rows = np.zeros((m, stride), np.uint8)
    rows[:, :352] = pool["rows"][pick, :352]
    if stride > 352:
        rows[:, 352:] = 0xEE   # bytes behind the record are not the record's
    return rows, pool["want"][0][pick], pool["want"][1][pick]


def _call(rows_d, **kw):
    """expert_actions on poisoned outputs, twice; the records untouched -> (actions, detail or None) as numpy."""
    import torch
    from balatro_gym_amd import expert_actions
    before = rows_d.clone()
    index = kw.get("index")
    shape = tuple(index.shape) if index is not None else tuple(rows_d.shape[:-1])
    outs = []
    for _ in range(2):
        out = torch.empty(shape, dtype=torch.int32, device=rows_d.device)
        det = torch.empty(shape, dtype=torch.int32, device=rows_d.device) if kw.get("detail") else None
        poison_(out, det)
        res = expert_actions(rows_d, index=index, out=out, detail=det, lanes=kw.get("lanes", 0))
        assert (res[0] if det is not None else res) is out
        outs.append((out.cpu().numpy(), None if det is None else det.cpu().numpy()))
    assert torch.equal(rows_d, before), "the records were written"
    assert np.array_equal(outs[0][0], outs[1][0]) and (outs[0][1] is None or np.array_equal(outs[0][1], outs[1][1])), "two calls differ"
    return outs[0]


@pytest.mark.parametrize("stride", [352, 384])
@pytest.mark.parametrize("m", SIZES)
def test_kernel_matches_the_restatement(pool, m, stride):
    rows, want_a, want_d = _take(pool, m, stride)
    rows_d = _dev(rows)
    for lanes in (0, 1, 8, 64):
        a, d = _call(rows_d, detail=True, lanes=lanes)
        assert np.array_equal(a, want_a), f"lanes {lanes}: actions differ at {np.flatnonzero(a != want_a)[:5]}"
        assert np.array_equal(d, want_d), f"lanes {lanes}: detail differs at {np.flatnonzero(d != want_d)[:5]}"
        a2, none = _call(rows_d, lanes=lanes)
        assert none is None and np.array_equal(a2, want_a)
    # through an index: a permutation with repeats, and entries outside the store
    rng = np.random.default_rng(m)
    index = rng.integers(0, m, m + 3).astype(np.int32)
    index[::5] = index[0]
    index[-3:] = [-1, m, -2 ** 31]
    if m > 1:
        index[1] = 2 ** 31 - 1
    inside = (index >= 0) & (index < m)
    wa = np.where(inside, want_a[np.where(inside, index, 0)], -1)
    wd = np.where(inside, want_d[np.where(inside, index, 0)], 0)
    for lanes in (0, 1, 8, 64):
        a, d = _call(rows_d, index=_dev(index), detail=True, lanes=lanes)
        assert np.array_equal(a, wa) and np.array_equal(d, wd), f"lanes {lanes}, indexed"
    a, _ = _call(rows_d, index=_dev(index))
    assert np.array_equal(a, wa)


@pytest.mark.parametrize("m", [8192, 8193, 131072, 131073])
def test_default_mapping_on_both_sides_of_its_thresholds(pool, m):
    """bg_expert_lanes(m): a wave per record up to 8 192 records, 8 lanes up to 131 072, one lane above (csrc/bg_expert.h).  The pool tiled to the
    last size of one mapping and the first of the next, with the library's choice."""
    import os
    import re
    from tests.helpers import ROOT
    hdr = open(os.path.join(ROOT, "balatro_gym_amd", "csrc", "bg_expert.h")).read()
    assert re.search(r"#define BG_EXPERT_WAVE_MAX 8192\b", hdr) and re.search(r"#define BG_EXPERT_GROUP_MAX 131072\b", hdr), "the test's sizes are the header's thresholds"
    rows, want_a, want_d = _take(pool, m, 384)
    a, d = _call(_dev(rows), detail=True)
    assert np.array_equal(a, want_a) and np.array_equal(d, want_d)


def test_whole_pool_and_three_dimensional_rows(pool):
    """Every record of the pool once, as [K, N, stride]: all named synthetic cases and all rollout records, in one launch."""
    import torch
    from balatro_gym_amd import expert_actions
    n = len(pool["rows"]) // 4 * 4
    rows_d = _dev(pool["rows"][:n].reshape(4, n // 4, 384))
    a, d = expert_actions(rows_d, detail=True)
    assert tuple(a.shape) == (4, n // 4) and a.dtype == torch.int32
    bad = np.flatnonzero(a.cpu().numpy().reshape(-1) != pool["want"][0][:n])
    assert bad.size == 0, f"actions differ on records {bad[:8]} (synthetic below {pool['n_synth']})"
    assert np.array_equal(d.cpu().numpy().reshape(-1), pool["want"][1][:n])
    assert expert_actions(rows_d[:, :0]).shape == (4, 0)


def test_collection_loop_and_chain_to_the_learner():
    import torch
    from balatro_gym_amd import BalatroVecEnv, DemoBuffer, EpisodeLimits, bc_loss, episode_outcomes, expert_actions
    from balatro_gym_amd.vec_env import RowBuffers
    n, K = N_ENVS, LOOP_STEPS
    seeds = [7000 + i for i in range(n)]
    # ---- the collection loop: expert_act() -> step(), the records kept on the device and compared at the end
    env = BalatroVecEnv(n, seeds, scorer_jokers=True, autoreset=True, max_ante=1, obs_layout="rows")   # (max_ante 1: episodes end inside the loop)
    dev = env.device
    seen = torch.zeros((K, n, 384), dtype=torch.uint8, device=dev)
    taken = torch.zeros((K, n), dtype=torch.int32, device=dev)
    for t in range(K):
        seen[t].copy_(env.obs_rows)
        a = env.expert_act(out=taken[t])
        assert a is taken[t] or a.data_ptr() == taken[t].data_ptr()
        env.step(a)
    env.check()
    env.close()
    want_a, _ = ref.expert_rows(seen.reshape(K * n, 384).cpu().numpy())
    got = taken.cpu().numpy().reshape(-1)
    bad = np.flatnonzero(got != want_a)
    assert bad.size == 0, f"{bad.size} actions of the loop differ from the restatement, first at step {bad[0] // n} env {bad[0] % n}: {got[bad[0]]} vs {want_a[bad[0]]}"
    mask = seen[:, :, 176:236].reshape(K * n, 60).cpu().numpy()
    assert (got >= 0).all() and (mask[np.arange(K * n), got] != 0).all(), "an action outside the record's mask"
    phases = set(np.unique(seen[:, :, 339].cpu().numpy()).tolist())
    print(f"collection loop: phases seen {sorted(phases)}, plays {int((got == 0).sum())}, discards {int((got == 1).sum())}, buys {int(((got >= 20) & (got < 30)).sum())}")
    assert {0, 1, 2} <= phases and (got == 0).any() and (got == 1).any()

    # ---- the same actions through step_many(limits=) one step per call, into a [K + 1, N] store
    env = BalatroVecEnv(n, seeds, scorer_jokers=True, autoreset=True, max_ante=1, obs_layout="rows")   # (max_ante 1: episodes end inside the loop)
    one = RowBuffers(n, dev, steps=1, row_stride=384)
    lim = EpisodeLimits(n, dev, max_invalid_actions=10 ** 9, max_episode_steps=10 ** 9, steps=1, row_stride=384, summary=True)   # (never reached: the chain is the step() loop)
    store = torch.zeros((K + 1, n, 384), dtype=torch.uint8, device=dev)
    store[0].copy_(env.obs_rows)
    for t in range(K):
        a = expert_actions(store[t])
        env.step_many(a[None], obs_buffers=one, limits=lim)
        store[t + 1].copy_(one.rows[0])
    env.check()
    env.close()
    actions = store[1:, :, 172:176].view(torch.int32)[:, :, 0]
    assert torch.equal(actions, taken), "the chunked chain took other actions than the step() loop"
    assert torch.equal(expert_actions(store[:K]), taken), "relabelling the finished store in one launch gives the actions taken"
    out = episode_outcomes(store)
    weights = (out.end_ante[1:] >= 1).float()
    kept_idx = torch.nonzero(weights.reshape(-1) > 0).reshape(-1).to(torch.int32)
    kept = int(kept_idx.numel())
    print(f"chain: {int((store[1:, :, 342] != 0).sum())} episodes ended, {kept} of {K * n} steps kept")
    assert kept > 0, "no episode ended inside the loop: the chain would be checked on nothing"
    demo = DemoBuffer(K * n, dev)
    demo.add(store, weights)
    assert len(demo) == kept
    assert torch.equal(demo.actions[:kept], taken.reshape(-1)[kept_idx.long()]), "the ring's actions are not the expert's"
    logits = torch.zeros((kept, 60), device=dev)
    logits[torch.arange(kept, device=dev), demo.actions[:kept].long()] = 20.0
    _, st = bc_loss(logits, demo.actions, demo.rows, weights=demo.weight, index=torch.arange(kept, dtype=torch.int32, device=dev))
    assert float(st.excluded) == 0.0 and float(st.weight_sum) == float(kept)
    assert float(st.accuracy) == 1.0


def test_c_checks_refuse_before_any_launch():
    import torch
    from balatro_gym_amd import _native as nat
    L = nat.load()
    m = 8
    rows = torch.zeros((m, 384), dtype=torch.uint8, device="cuda")
    out = torch.full((m + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    det = torch.full((m + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    idx = torch.zeros(m, dtype=torch.int32, device="cuda")
    good = dict(rows=rows.data_ptr(), stride=384, m=m, index=None, store=m, out=out.data_ptr(), det=det.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return L.bg_expert_actions(a["rows"], a["stride"], a["m"], a["index"], a["store"], a["out"], a["det"], None)

    assert call() == 0 and call(det=None) == 0 and call(index=idx.data_ptr()) == 0 and call(m=0) == 0 and call(m=0, store=0) == 0
    torch.cuda.synchronize()
    out.fill_(0x5A5A5A5A); det.fill_(0x5A5A5A5A)
    refusals = [dict(stride=336), dict(stride=360), dict(stride=0), dict(stride=-384), dict(rows=rows.data_ptr() + 8), dict(rows=None), dict(m=-1), dict(m=2 ** 31),
                dict(m=m + 1), dict(store=-1), dict(index=idx.data_ptr() + 2), dict(index=idx.data_ptr(), store=2 ** 31), dict(out=None), dict(out=out.data_ptr() + 2),
                dict(det=det.data_ptr() + 1), dict(out=rows.data_ptr()), dict(out=rows.data_ptr() + 384 * 3 + 172), dict(det=rows.data_ptr() + 16),
                dict(det=out.data_ptr()), dict(index=idx.data_ptr(), out=idx.data_ptr())]
    for kw in refusals:
        assert call(**kw) == -1, kw   # BG_E_ARG
        assert L.bg_last_error(None).decode().startswith("bg_expert_actions: "), kw
    assert L.bg_expert_actions_ex(rows.data_ptr(), 384, m, None, m, out.data_ptr(), None, 3, None, None) != 0
    torch.cuda.synchronize()
    assert (out == 0x5A5A5A5A).all() and (det == 0x5A5A5A5A).all(), "a refused call wrote an output"
