"""GPU tests of bg_step_many_rows (BalatroVecEnv.step_many with a RowBuffers): K steps per env with the CALLER's actions on the packed-record
engine (bg_engine3.h's action mode), every step kept as one record.  Everything is compared bit-exactly: the 31 observation keys, the reward's
bit pattern, the terminated byte and the action word of every record, against the CPU oracle or against the rollout that produced the actions."""
import random

import numpy as np
import pytest

from tests.helpers import OBS_KEYS, POISON, poison_
from tests.test_gpu_parity import SEED_OFFSET, _assert_obs, _obs_np, _oracle_envs, _oracle_rollout, _row_views, _vec

pytestmark = pytest.mark.gpu

R_REWARD, R_ACTION, R_TERM = 136, 172, 342   # BG_ROW_REWARD / BG_ROW_ACTION / BG_ROW_TERMINATED


def _assert_records(ctx, rows, res, want_obs, acts, stride):
    """One step's records (`rows`: CPU uint8 [n, stride]) against the oracle's results `res` of that step (OracleEnv.step tuples), the
    observations `want_obs` (stacked per key) and the actions as given."""
    _assert_obs(_row_views(rows), want_obs, ctx)
    r = rows.numpy()
    wr = np.array([x[1] for x in res], dtype=np.float64).view(np.uint64)
    wt = np.array([x[2] for x in res], dtype=np.uint8)
    gr = r[:, R_REWARD:R_REWARD + 8].copy().view(np.uint64)[:, 0]
    assert np.array_equal(gr, wr), f"{ctx}: reward bits differ for env {np.nonzero(gr != wr)[0][:4]}"
    assert np.array_equal(r[:, R_TERM], wt), f"{ctx}: terminated differs for env {np.nonzero(r[:, R_TERM] != wt)[0][:4]}"
    ga = r[:, R_ACTION:R_ACTION + 4].copy().view(np.int32)[:, 0]
    assert np.array_equal(ga, acts), f"{ctx}: the record's action word is not the caller's for env {np.nonzero(ga != acts)[0][:4]}"
    assert not r[:, R_TERM + 1:352].any(), f"{ctx}: record bytes 343..351"
    if stride == 384:
        assert not r[:, 352:].any(), f"{ctx}: bytes 352..383 of a whole-line record are not zero"
    elif stride > 352:
        assert (r[:, 352:] == POISON).all(), f"{ctx}: bytes 352.. of a record were written"


def _scenario_vs_oracle(monkeypatch, autoreset, stride, engine=None):
    """The scenario of tests/test_gpu_parity.py _step_many_vs_oracle through bg_step_many_rows: 333 envs (a partial last workgroup), scorer
    jokers, max_ante 4, the oracle's uniform policy, shallow rings (a 48-step call is eight or more launches with refills between them)."""
    import torch
    from balatro_gym_amd.vec_env import RowBuffers
    from oracle.gen_golden import IMPLEMENTED
    monkeypatch.setenv("BG_KG", "4"); monkeypatch.setenv("BG_KS", "5"); monkeypatch.setenv("BG_KD", "4")
    if engine is not None:
        monkeypatch.setenv("BG_ENGINE", str(engine))
    n, K, calls, spare = 333, 48, 3, 2
    seeds = [752_000 + SEED_OFFSET + 7 * i for i in range(n)]
    jokers = [random.Random(7300 + i).sample(IMPLEMENTED, i % 6) for i in range(n)]
    env = _vec(n, seeds, scorer_jokers=True, autoreset=autoreset, max_ante=4)
    env.inject(jokers=jokers, apply_now=True)
    orc = _oracle_envs(n, seeds, True, 4, jokers)
    rb = RowBuffers(n, env.device, steps=K + spare, row_stride=stride)
    assert env.max_fused_steps * 3 <= K
    env.set_profiling(True)
    plays = shops = episodes = 0
    for c in range(calls):
        acts = np.zeros((K, n), np.int32)
        res_k, want_k = [], []
        for j in range(K):
            t = c * K + j
            phase = [int(o.obs()["phase"]) for o in orc]
            acts[j] = [o.policy_action(0, 23, i, t) for i, o in enumerate(orc)]
            res = [o.step(int(a)) for o, a in zip(orc, acts[j])]
            plays += sum(r[4].hand_type >= 0 for r in res)
            shops += sum(p == 1 and r[1] != -1.0 for p, r in zip(phase, res))
            if autoreset:   # SAME_STEP auto-reset: the record shows the new episode
                for i, r in enumerate(res):
                    if r[2]:
                        episodes += 1
                        orc[i].reset(); orc[i].set_jokers(jokers[i])
            res_k.append(res)
            obs = [o.obs() for o in orc] if autoreset else [r[0] for r in res]
            want_k.append({k: np.stack([w[k] for w in obs]) for k in OBS_KEYS})
        poison_(rb.rows)
        out = env.step_many(torch.from_numpy(acts).to(env.device), obs_buffers=rb)
        assert out[0] is rb.tensors and out[1] is rb.reward and out[2] is rb.terminated and out[3] is None and out[4] is None
        prof = env.get_profile()
        ctx = f"engine {engine} autoreset {autoreset} stride {stride} call {c}"
        assert prof["rollout_launches"] >= 3, (ctx, prof)
        got = rb.rows.cpu()
        for j in range(K):
            _assert_records(f"{ctx} step {j}", got[j], res_k[j], want_k[j], acts[j], stride)
        assert (got[K:].numpy() == POISON).all(), f"{ctx}: rows past the call's last step were written"
        st = env.stats()
        assert st["steps"] == n * K, (ctx, st)
    env.check()
    env.close()
    assert plays > 0 and shops > 0, (plays, shops)   # the run contained service steps of both classes
    if autoreset:
        assert episodes > 0
    return plays, shops, episodes


@pytest.mark.parametrize("stride", [352, 384])
@pytest.mark.parametrize("autoreset", [False, True], ids=["autoreset_off", "autoreset_on"])
def test_every_step_vs_oracle(monkeypatch, autoreset, stride):
    """Every record of every step of three 48-step calls against the oracle, with auto-reset on and off (the oracle envs are stepped on after
    they terminate), on both record strides; rows past the call's last step keep their byte pattern."""
    _scenario_vs_oracle(monkeypatch, autoreset, stride)


def test_engine1_handle_gives_the_same_records(monkeypatch):
    """A BG_ENGINE=1 handle has no bg_engine3.h: the call runs on bg_engine.h (actions_in, copier wave) and writes the same records."""
    _scenario_vs_oracle(monkeypatch, True, 384, engine=1)


def test_cap_with_autoreset_off_vs_oracle():
    """Auto-reset off and per-env curriculum caps 1..3 (level-15 hands: antes rise fast): an env that has exceeded its cap is stepped on,
    with toggles, PLAY_HAND, shop-leave, blind selection and invalid actions -- every such step reports terminated = 1 (and the reward the
    action earns), which the owner waves' cheap steps alone would not.  Every record against the oracle."""
    import torch
    from balatro_gym_amd.vec_env import RowBuffers
    from oracle import pyoracle as po
    n, K, calls = 192, 30, 6
    seeds = [61_000 + SEED_OFFSET + 3 * i for i in range(n)]
    caps = [1 + i % 3 for i in range(n)]
    env = _vec(n, seeds, autoreset=False, max_ante=0)
    env.inject(levels=np.full((n, 12), 15, np.uint8), apply_now=True)
    env.set_max_ante(caps)
    orc = [po.OracleEnv(s, max_ante=c) for s, c in zip(seeds, caps)]
    for o in orc:
        for ht in range(12):
            o.set_hand_level(ht, 15)
    rb = RowBuffers(n, env.device, steps=K, row_stride=384)
    above = np.zeros(n, np.int64)
    kinds = {"toggle": 0, "play": 0, "leave": 0, "invalid": 0}
    for c in range(calls):
        acts = np.zeros((K, n), np.int32)
        res_k, want_k = [], []
        for j in range(K):
            t = c * K + j
            res = []
            for i, o in enumerate(orc):
                ob = o.obs()
                if int(ob["ante"]) > caps[i]:
                    m = (7 * i + t) % 6
                    a = [2 + t % 8, 0, 31, 60, 45, 2 + (t + 3) % 8][m]
                    above[i] += 1
                else:
                    a = o.policy_action(1, 21, i, t)
                acts[j, i] = a
                r = o.step(int(a))
                if int(ob["ante"]) > caps[i]:
                    assert r[2], "the oracle reports terminated on every step above the cap"
                    if r[1] == -1.0:
                        kinds["invalid"] += 1
                    elif a == 0:
                        kinds["play"] += 1
                    elif a == 31:
                        kinds["leave"] += 1
                    elif 2 <= a < 10:
                        kinds["toggle"] += 1
                res.append(r)
            res_k.append(res)
            want_k.append({k: np.stack([r[0][k] for r in res]) for k in OBS_KEYS})
        poison_(rb.rows)
        env.step_many(torch.from_numpy(acts).to(env.device), obs_buffers=rb)
        got = rb.rows.cpu()
        for j in range(K):
            _assert_records(f"call {c} step {j}", got[j], res_k[j], want_k[j], acts[j], 384)
    env.check()
    env.close()
    assert above.sum() >= 20 and above.max() >= 5, (int(above.sum()), int(above.max()))
    assert all(v > 0 for v in kinds.values()), kinds


def test_hostile_actions():
    """Rows of -1, 60, 1000, 32768 + 2, 65536, INT32_MIN, INT32_MAX for every env, interleaved with valid rows, on fresh envs and on envs made
    terminal (template ante 101, auto-reset off: they stay terminal and every step goes to a service wave): on a fresh env reward -1.0 and
    the state unchanged; on every env the record's action word is the input, and the records equal what bg_step_rows writes on a twin."""
    import torch
    from balatro_gym_amd._native import NativeError
    from balatro_gym_amd.vec_env import RowBuffers
    n = 333
    seeds = [4_400 + SEED_OFFSET + 5 * i for i in range(n)]
    hostile = [-1, 60, 1000, 32768 + 2, 65536, -2147483648, 2147483647]
    valid = [45, 2, 3, 4, 0, 5, 31]
    rows = []
    for h, v in zip(hostile, valid):
        rows += [h, v]
    K = len(rows)
    acts = torch.tensor(rows, dtype=torch.int32).view(K, 1).repeat(1, n).contiguous()
    term_mask = np.array([i % 3 == 1 for i in range(n)], np.uint8)

    def make(**kw):
        e = _vec(n, seeds, autoreset=False, **kw)
        try:
            e.inject(ante=[101] * n, mask=term_mask, apply_now=True)
            return e, True
        except NativeError:
            return e, False
    env, terminal = make()
    twin, terminal2 = make(obs_layout="rows")
    assert terminal == terminal2
    acts = acts.to(env.device)
    rb = RowBuffers(n, env.device, steps=K, row_stride=384)
    before = env.observe()
    before = {k: v.cpu().numpy().copy() for k, v in before.items()}
    poison_(rb.rows)
    env.step_many(acts, obs_buffers=rb)
    env.check()
    got = rb.rows.cpu()
    fresh = term_mask == 0 if terminal else np.ones(n, bool)
    prev = before
    for j in range(K):
        twin.step(acts[j])
        tw = twin.obs_rows.cpu().numpy()
        g = got[j].numpy()
        assert np.array_equal(g[:, :352], tw[:, :352]), f"row {j} (action {rows[j]}): records differ from bg_step_rows on a twin handle"
        assert np.array_equal(g[:, R_TERM], twin.terminated.cpu().numpy()), j
        assert np.array_equal(g[:, R_REWARD:R_REWARD + 8].copy().view(np.uint64)[:, 0], twin.reward.cpu().numpy().view(np.uint64)), j
        assert (g[:, R_ACTION:R_ACTION + 4].copy().view(np.int32)[:, 0] == rows[j]).all(), f"row {j}: action word"
        assert not g[:, 352:].any()
        cur = _row_views(got[j])
        if rows[j] in hostile:
            rw = g[:, R_REWARD:R_REWARD + 8].copy().view(np.float64)[:, 0]
            assert (rw[fresh] == -1.0).all() and not g[fresh, R_TERM].any(), f"row {j} (action {rows[j]}): not rejected"
            for k in OBS_KEYS:
                assert np.array_equal(cur[k][fresh], prev[k][fresh]), f"row {j} (action {rows[j]}): {k} changed"
        if terminal:
            assert g[term_mask == 1, R_TERM].all(), f"row {j}: an env above ante 100 is terminal on every step"
        prev = cur
    twin.check()
    fin = {k: v.cpu().numpy() for k, v in env.observe().items()}
    for k in OBS_KEYS:
        assert np.array_equal(fin[k], prev[k]), f"final state: {k}"
    env.close(); twin.close()


def _workload(n, cards=False):
    from oracle.gen_golden import IMPLEMENTED
    seeds = [1000 + SEED_OFFSET + i for i in range(n)]
    jokers = [random.Random(i).sample(IMPLEMENTED, 5) for i in range(n)]
    cs = [[(d, [0, 1, 4, 6, 8][(i + d) % 5], [0, 1, 3][d % 3], [0, 1, 2, 3, 4][(i // 3 + d) % 5]) for d in range(16)] if i % 3 == 0 else []
          for i in range(n)] if cards else None

    def make():
        e = _vec(n, seeds, autoreset=True, scorer_jokers=True, max_ante=4, card_states=cards)
        if cards:
            e.inject_cards(cs, apply_now=True)
        e.inject(jokers=jokers, apply_now=True)
        return e
    return seeds, jokers, cs, make


def _equals_rollout(n, policy, pseed, cards=False, pick=None):
    """Handle A: rollout(T) with packed records; its recorded actions through step_many on handle B as ONE call (T > max_fused_steps: chunks) and
    on handle C as calls of 20 (refill in pieces beside short launches): every byte of every record equal, and the stats.  `pick`: envs of B
    also compared with the oracle."""
    import torch
    from balatro_gym_amd.vec_env import RowBuffers
    seeds, jokers, cs, make = _workload(n, cards)
    a = make()
    T = a.max_fused_steps + 28
    rba = RowBuffers(n, a.device, steps=T, row_stride=384)
    a.rollout(T, policy=policy, policy_seed=pseed, obs_buffers=rba)
    sa = a.stats()
    a.close()
    acts = rba.action.contiguous()
    assert sa["steps"] == n * T and sa["plays"] > 0 and sa["episodes"] > 0
    rbb = RowBuffers(n, acts.device, steps=T, row_stride=384)
    b = make()
    b.set_profiling(True)
    b.step_many(acts, obs_buffers=rbb)
    assert b.get_profile()["rollout_launches"] >= 2
    sb = b.stats()
    b.close()
    assert torch.equal(rba.rows, rbb.rows), f"n {n}: one call differs from the rollout at step {int((rba.rows != rbb.rows).flatten(1).any(1).nonzero()[0])}"
    for k in ("steps", "episodes", "plays", "score_sum", "reward_bits"):
        assert sa[k] == sb[k], (k, sa[k], sb[k])
    sub = None
    if pick is not None:
        sub = rbb.rows[:, torch.from_numpy(pick).to(acts.device), :].cpu()
    rbb.rows.fill_(POISON)
    c = make()
    tot = {"steps": 0, "episodes": 0, "plays": 0, "score_sum": 0}
    for c0 in range(0, T, 20):
        k = min(20, T - c0)
        c.step_many(acts[c0:c0 + k], obs_buffers=_rows_slice(rbb, c0, k))
        s = c.stats()
        for key in tot:
            tot[key] += s[key]
    c.close()
    assert torch.equal(rba.rows, rbb.rows), f"n {n}: calls of 20 differ from the rollout"
    for key in tot:
        assert tot[key] == sa[key], (key, tot[key], sa[key])
    del rba, rbb
    if pick is not None:
        from balatro_gym_amd.vec_env import RowBuffers as RB
        w = RB(len(pick), torch.device("cpu"), steps=T, row_stride=384)
        w.rows.copy_(sub)
        wobs, wr, wt, wa, _ = _oracle_rollout(len(pick), [seeds[i] for i in pick], T, policy, pseed, True, 4, [jokers[i] for i in pick],
                                              cards=[cs[i] for i in pick] if cards else None, env_indexes=pick.tolist())
        assert np.array_equal(w.action.numpy(), wa)
        assert np.array_equal(w.terminated.numpy(), wt)
        assert np.array_equal(w.reward.contiguous().numpy().view(np.uint64), wr.view(np.uint64))
        for k in OBS_KEYS:
            assert np.array_equal(w.tensors[k].contiguous().numpy(), wobs[k]), f"record key {k} differs from the oracle"


def _rows_slice(rb, c0, k):
    """Rows c0 .. c0 + k of a RowBuffers as a RowBuffers of their own (same memory)."""
    from balatro_gym_amd.vec_env import RowBuffers
    v = RowBuffers.__new__(RowBuffers)
    v.n, v.steps, v.row_stride = rb.n, k, rb.row_stride
    v.rows = rb.rows[c0:c0 + k]
    v.tensors = {key: t[c0:c0 + k] for key, t in rb.tensors.items()}
    v.reward, v.action, v.terminated = rb.reward[c0:c0 + k], rb.action[c0:c0 + k], rb.terminated[c0:c0 + k]
    return v


def test_equals_the_rollout_full_size():
    """65 536 envs, configs[2] (256-env workgroups), T = max_fused_steps + 28: byte-equal to the rollout as one call and as calls of 20, equal
    stats; then 2 048 envs spread over all workgroups against the oracle."""
    pick = np.array([32 * j + (5 * j + j // 8) % 32 for j in range(2048)], dtype=np.int64)
    _equals_rollout(65536, 2, 20251001, pick=pick)


@pytest.mark.parametrize("n,cards", [(4096, False), (20000, False), (333, True)], ids=["4096_epw16", "20000_128env", "333_cards"])
def test_equals_the_rollout_other_shapes(n, cards):
    """The 64-env workgroup shape with 16 live envs per workgroup (4 096 envs), the 128-env shape (20 000 envs: a partial last workgroup) and
    card states (333 envs, uniform policy)."""
    _equals_rollout(n, 0 if cards else 2, 77, cards=cards, pick=np.arange(0, n, max(1, n // 128), dtype=np.int64)[:128] if not cards else np.arange(n, dtype=np.int64))


def test_long_run_small_job_vs_oracle():
    """160 envs, 900 steps in calls of 40 (more than two refill periods of the default rings), a get_state in the middle: every record
    against the oracle, and the final observe() equals the oracle's state."""
    import torch
    from balatro_gym_amd.vec_env import RowBuffers
    from oracle.gen_golden import IMPLEMENTED
    n, K, T = 160, 40, 900
    seeds = [33_000 + SEED_OFFSET + 11 * i for i in range(n)]
    jokers = [random.Random(900 + i).sample(IMPLEMENTED, 1 + i % 5) for i in range(n)]
    env = _vec(n, seeds, scorer_jokers=True, autoreset=True, max_ante=4)
    env.inject(jokers=jokers, apply_now=True)
    orc = _oracle_envs(n, seeds, True, 4, jokers)
    rb = RowBuffers(n, env.device, steps=K, row_stride=384)
    episodes = 0
    for c0 in range(0, T, K):
        k = min(K, T - c0)
        acts = np.zeros((k, n), np.int32)
        res_k, want_k = [], []
        for j in range(k):
            acts[j] = [o.policy_action(0, 5, i, c0 + j) for i, o in enumerate(orc)]
            res = [o.step(int(a)) for o, a in zip(orc, acts[j])]
            for i, r in enumerate(res):
                if r[2]:
                    episodes += 1
                    orc[i].reset(); orc[i].set_jokers(jokers[i])
            res_k.append(res)
            obs = [o.obs() for o in orc]
            want_k.append({key: np.stack([w[key] for w in obs]) for key in OBS_KEYS})
        poison_(rb.rows)
        env.step_many(torch.from_numpy(acts).to(env.device), obs_buffers=rb)
        if c0 == 440:
            assert len(env.get_state(7)) == env._L.bg_state_blob_bytes(env._h)
        got = rb.rows.cpu()
        for j in range(k):
            _assert_records(f"steps {c0}+{j}", got[j], res_k[j], want_k[j], acts[j], 384)
        assert (got[k:].numpy() == POISON).all()
    env.check()
    fin = {key: v.cpu().numpy() for key, v in env.observe().items()}
    _assert_obs(fin, {key: np.stack([o.obs()[key] for o in orc]) for key in OBS_KEYS}, "final observe()")
    env.close()
    assert episodes > 0


def test_gather_and_single_row():
    """World 1, own gather buffer [1, n, 352]: after step_many with records and a synchronize the buffer holds the call's last step.  A
    one-row RowBuffers (stride 0) holds the last step's record of a kept run."""
    import torch
    from balatro_gym_amd.vec_env import RowBuffers
    n, K = 333, 37
    seeds, jokers, _, make = _workload(n)
    a = make()
    rec = RowBuffers(n, a.device, steps=K, row_stride=384)
    a.rollout(K, policy=0, policy_seed=3, obs_buffers=rec)
    acts = rec.action.contiguous()
    a.close()
    b = make()
    gbuf = torch.zeros((1, n, 352), dtype=torch.uint8, device=b.device)
    b.set_gather_peers([gbuf], 0)
    rb = RowBuffers(n, b.device, steps=K, row_stride=384)
    b.step_many(acts, obs_buffers=rb)
    torch.cuda.synchronize(b.device)
    assert torch.equal(rb.rows, rec.rows)
    assert torch.equal(gbuf[0], rb.rows[K - 1][:, :352]), "gathered current records differ from the call's last row"
    b.check(); b.close()
    c = make()
    one = RowBuffers(n, c.device, steps=1, row_stride=384)
    poison_(one.rows)
    out = c.step_many(acts, obs_buffers=one)
    torch.cuda.synchronize(c.device)
    assert torch.equal(one.rows[0], rb.rows[K - 1])
    assert torch.equal(out[1][0].view(torch.int64), rb.reward[K - 1].view(torch.int64))
    c.check(); c.close()
