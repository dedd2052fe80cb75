"""tests/ppo_iter_ref.py without a GPU: the two statements of the transition driver agree; packed oracle observations unpack to themselves; and a DRY RUN of
tests/test_ppo_iteration.py's workload -- the same seeds and shapes, a float64 CPU twin of the network driving the oracle alone, head_ref.Reference as the
sampler, SB3-literal VecNormalize / GAE / loss -- meets every condition the GPU test asserts with at least twice the margin: terminated records per
iteration and their step positions, episodes across the iteration boundary, the share of undecidable head rows, and both mutation controls (the loss
reference fed mask[t + 1] excludes rows; GAE fed values shifted by one step differs).  The counts are printed."""
import numpy as np
import pytest

from tests import encode_ref, gae_ref, head_ref, helpers, norm_ref, ppo_iter_ref as ref, ppo_ref
from tests.helpers import OBS_KEYS

W = ref.WORKLOAD


def _workload(n=None):
    wl = helpers.sharded_workload("configs2", n or W["N"], seed0=W["seed0"])
    return wl, lambda: ref.make_oracles(wl["seeds"], wl["env_kwargs"]["scorer_jokers"], W["max_ante"], wl["jokers"])


def _valid_random_actions(make, K, seed):
    """[K, N] actions valid under the oracle's own masks (a throw-away set of envs is stepped to find them)."""
    vec = ref.OracleVec(make())
    rng = np.random.default_rng(seed)
    acts = []
    obs = vec.observe()
    for _ in range(K):
        u = rng.random(obs["action_mask"].shape)
        acts.append(np.where(obs["action_mask"] != 0, u, -1.0).argmax(axis=1).astype(np.int32))
        obs, _, _ = vec.step(acts[-1])
    return np.stack(acts), vec.transitions()


def test_the_two_transition_drivers_agree():
    """collect_literal (time-major, dict observations, Python lists) and collect_vectorised (env-major, one structured view) on the same actions, over two
    consecutive calls on the same envs (the second starts where the first ended); the step-at-a-time OracleVec gives the same arrays."""
    wl, make = _workload(40)
    K = 60
    acts, stepped = _valid_random_actions(make, 2 * K, 3)
    a, b = make(), make()
    for part in range(2):
        A = ref.collect_literal(a, acts[part * K:(part + 1) * K], wl["jokers"])
        B = ref.collect_vectorised(b, acts[part * K:(part + 1) * K], wl["jokers"])
        for k in OBS_KEYS:
            assert A["obs"][k].dtype == B["obs"][k].dtype and np.array_equal(A["obs"][k], B["obs"][k]), (part, k)
            assert np.array_equal(A["obs"][k], stepped["obs"][k][part * K:(part + 1) * K + 1]), (part, k)
        assert np.array_equal(A["mask"], B["mask"]) and A["mask"].dtype == np.int8
        assert np.array_equal(A["reward"].view(np.uint64), B["reward"].view(np.uint64)) and np.array_equal(A["done"], B["done"])
        assert np.array_equal(A["reward"].view(np.uint64), stepped["reward"][part * K:(part + 1) * K].view(np.uint64))
        assert np.array_equal(A["done"], stepped["done"][part * K:(part + 1) * K])
        if part:
            assert all(np.array_equal(A["obs"][k][0], first_last[k]) for k in OBS_KEYS), "the second call does not start where the first ended"
        first_last = {k: A["obs"][k][-1] for k in OBS_KEYS}
    assert stepped["done"].sum() >= 4, "the 120 steps end no episode: the reset path was not compared"
    assert np.take_along_axis(stepped["mask"][:-1], acts[:, :, None].astype(np.int64), axis=2).all()


def test_packed_oracle_observations_unpack_to_themselves():
    """encode_ref.pack_records / unpack_records over observations the oracle made (both strides), and the reward / action / terminated fields of
    ppo_iter_ref.step_records beside them."""
    _, make = _workload(40)
    acts, tr = _valid_random_actions(make, 30, 4)
    for stride in (384, 352):
        rows = ref.records(tr, acts, stride)
        assert rows.shape == (31, 40, stride) and rows.dtype == np.uint8
        obs, reward, action, term = ref.record_fields(rows)
        for k in OBS_KEYS:
            assert obs[k].dtype == tr["obs"][k].dtype and np.array_equal(obs[k], tr["obs"][k]), (stride, k)
        assert np.array_equal(reward[1:].view(np.uint64), tr["reward"].view(np.uint64)) and not reward[0].any()
        assert np.array_equal(action[1:], acts) and np.array_equal(term[1:] != 0, tr["done"]) and not term[0].any()
        r2, d2 = gae_ref.unpack_records(rows[1:])
        assert np.array_equal(r2.view(np.uint64), tr["reward"].view(np.uint64)) and np.array_equal(d2, tr["done"])


def test_monitor_literal_is_gae_refs_scan():
    """The per-env list statement of Monitor and gae_ref.episode_stats' forward scan agree, carry included."""
    rng = np.random.default_rng(8)
    reward = rng.uniform(-5, 20, (40, 17))
    done = rng.integers(0, 7, (40, 17)) == 0
    r1, l1, carry = ref.monitor_literal(reward[:25], done[:25])
    r2, l2, _ = ref.monitor_literal(reward[25:], done[25:], carry)
    er, el, _, _ = gae_ref.episode_stats(reward, done)
    assert np.array_equal(np.concatenate([r1, r2]).view(np.uint64), er.view(np.uint64)) and np.array_equal(np.concatenate([l1, l2]), el)


def _dry_run(layout, dtype):
    import torch
    N, K = W["N"], W["K"]
    wl, make = _workload()
    vec = ref.OracleVec(make(), wl["jokers"])
    net = ref.make_net(encode_ref.COLS[layout], W["net_seed"]).double()
    opt = torch.optim.SGD(net.parameters(), lr=W["lr"])
    feats = lambda obs_n: torch.from_numpy(ref.bits_to_float32(norm_ref.obs_bits(obs_n, layout, dtype), dtype)).double()   # noqa: E731
    rec0 = ref.step_records(vec.observe())
    state = norm_ref.new_state(N)
    obs_n, state = ref.norm_obs_step(rec0, norm_ref.numpy_moments(rec0[None])["obs"][0], state)   # VecNormalize.reset(): the observation half alone
    x = feats(obs_n)
    trs, und, mut_excluded, mut_gae, params0 = [], 0, [], [], [p.detach().clone() for p in net.parameters()]
    for it in range(W["iterations"]):
        actions, old_lp = np.zeros((K, N), np.int32), np.zeros((K, N), np.float32)
        values, rn = np.zeros((K, N), np.float32), np.zeros((K, N), np.float64)
        for t in range(K):
            with torch.no_grad():
                out = net(x).numpy()
            logits = out[:, :60].astype(np.float32)
            r = head_ref.Reference(logits, vec._obs[-1]["action_mask"], seed=W["act_seed"], index0=0, t=it * K + t)
            assert not r.degenerate.any()
            und += int((~r.decidable).sum())
            actions[t], old_lp[t], values[t] = r.action, r.log_prob(r.action).astype(np.float32), out[:, 60].astype(np.float32)
            obs, rew, done = vec.step(actions[t])
            rec = ref.step_records(obs, rew, actions[t], done)
            step = norm_ref.vecnormalize(rec[None], state)   # VecNormalize.step_wait, both halves
            state, rn[t] = step["state"], step["reward"][0]
            x = feats(step["obs"][0])
        with torch.no_grad():
            last_values = net(x).numpy()[:, 60].astype(np.float32)
        tr = vec.transitions()
        trs.append(tr)
        adv, ret = gae_ref.gae(rn, tr["done"], values, last_values, ref.GAMMA, ref.GAE_LAMBDA)
        shifted, _ = gae_ref.gae(rn, tr["done"], np.concatenate([values[1:], last_values[None]]), last_values, ref.GAMMA, ref.GAE_LAMBDA)
        mut_gae.append(int((gae_ref.bits32(shifted) != gae_ref.bits32(adv)).sum()))
        rec_obs = ref.records(tr, actions)[:K].reshape(K * N, ref.STRIDE)
        for b, idx in enumerate(ref.minibatch_indices(K, N, W["batch"], W["perm_seed"] + it)):
            ix = idx.numpy()
            x_mb = torch.from_numpy(ref.bits_to_float32(ref.frozen_features(rec_obs[ix], state, layout, dtype), dtype)).double()
            out = net(x_mb)
            lg, v = out[:, :60].detach().numpy().astype(np.float32), out[:, 60].detach().numpy().astype(np.float32)
            c = ref.make_case(lg, v, tr["mask"][:K], actions, old_lp, adv, ret, ix)
            cf = ppo_ref.ClosedForm(c, ref.CLIP, ref.ENT_COEF, ref.VF_COEF, True)
            assert cf.excluded.sum() == 0, "an action is invalid under the mask of its own observation"
            if b == 0:
                wrong = ppo_ref.ClosedForm(ref.make_case(lg, v, tr["mask"][1:], actions, old_lp, adv, ret, ix), ref.CLIP, ref.ENT_COEF, ref.VF_COEF, True)
                mut_excluded.append(int(wrong.excluded.sum()))
            _, loss = ppo_ref.torch_statement(c, ref.CLIP, ref.ENT_COEF, ref.VF_COEF, True, ~cf.excluded, params=(out[:, :60], out[:, 60]))
            opt.zero_grad()
            loss.backward()
            opt.step()
    moved = [float((p.detach() - q).abs().max()) for p, q in zip(net.parameters(), params0)]
    cond = ref.conditions(trs)
    cond.update(undecidable=und, rows=W["iterations"] * K * N, mask_shift_excluded=mut_excluded, value_shift_differs=mut_gae, moved=moved)
    return cond


@pytest.mark.parametrize("case", sorted(ref.CASES))
def test_dry_run_meets_every_condition_with_twice_the_margin(case):
    cond = _dry_run(*ref.CASES[case])
    print(f"{case}: {cond}")
    assert W["N"] % 32 and W["N"] % 64 and W["N"] % 256 and 32 <= W["K"] <= 64 and W["iterations"] * W["K"] * W["N"] <= 15000
    assert min(cond["terminated"]) >= 2 * 8 and min(cond["positions"]) >= 2 * 2, "too few terminated records"
    assert cond["spanning"] >= 2 * 1, "no episode spans the iteration boundary"
    assert cond["undecidable"] <= head_ref.UNDECIDABLE_CAP * cond["rows"] / 2, "too many undecidable head rows"
    assert min(cond["mask_shift_excluded"]) >= 2 and min(cond["value_shift_differs"]) >= 2, "the workload cannot see an off-by-one"
    assert min(cond["moved"]) > 0.0
