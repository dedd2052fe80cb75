"""One whole PPO iteration over packed records on the MI355X, then a second that carries all state over, through the product's operators alone, every
stage held to a reference that never reads a record the product wrote (tests/ppo_iter_ref.py: the C oracle stepped on the host with the GPU's actions, in
SB3's alignment, packed into reference records, and the single operators' references with their own bounds on top of those).

The recipe under test ("One PPO iteration over records"): ONE store uint8 [K + 1, N, 384]; store[0] the live record before the first
action, store[t + 1] the live record after action t; obs = store[:K] are the observation records (normalize_obs(index=), ppo_loss's mask), nxt = store[1:]
the reward records (gae_rows, EpisodeStats).  Per step: normalize_obs(live, update) -> network -> env.act(seed, t = global step) -> env.step ->
normalize_reward(live).  100 envs (no multiple of 32, 64 or 256), K = 48, max_ante = 1, minibatches of 1000 rows (the last has 800).

Each stage is PINNED: what the GPU produced is copied to the host and the next stage's reference starts from it, so every stage is held to its own bound.
  A  store[t]'s observation keys = the oracle's o[t]; store[t + 1]'s reward bits / action / terminated = reward[t] / a[t] / done[t]; bit for bit
  B  a[t] valid under the ORACLE's mask[t]; head_ref.Reference's action on decidable rows, log_prob / entropy within head_ref's bounds
  C  running mean / var / count, normalised rows, normalised rewards, the return carry after every call: the device's batch moments by
     norm_ref.check_moments, everything behind them bit for bit (norm_ref.from_moments over the oracle-made records); state_dict() after iteration 1
  D  advantages / returns = gae_ref.gae bit for bit            E  ep_return / ep_len = Monitor's per-episode sum and length, across the boundary
  F  minibatch features = the frozen-statistics features of o[t] at the index, bit for bit
  G  ppo_ref.ClosedForm over the oracle's mask[t]: every bound of ClosedForm.check, excluded == 0; G1: on an iteration's first minibatch
     |log_prob - old_log_prob| <= 2 max|dlogit| + both head_ref log-prob bounds
  H  p.grad against a float64 twin through ppo_ref.torch_statement within ppo_ref.mlp_gradient_bounds; the SGD step changed every parameter tensor
The device's batch moments are not an output of RowNormalizer: before each of its updating calls the test makes the same C call on a COPY of the state
with moments_out set (a second, side-effect-free launch); the product's own state is then held bit for bit to from_moments of those moments.

H's bound is ppo_ref.mlp_gradient_bounds with forward_abs=True: the relative slack alone misses an element of W2.grad whose logit column has a gradient on
ONE row of the minibatch with |h| = 6e-6 there (the float32 error of h is absolute); a float32 network on the CPU fed the exactly rounded gradient misses it
the same way, so that was the bound's mistake, not the kernel's (46 x the relative bound on the MI355X, 0.008 of the mended one).

Largest observed on the MI355X (produced float32 / fixed bfloat16): terminated records per iteration 65, 94 / 56, 74 at 30, 43 / 28, 38 step positions,
75 / 67 episodes across the boundary, 1 / 1 of 9 600 head rows undecidable; batch moments 0.009 (mean) and 0.21 (variance) of norm_ref's bounds; shares of
the head_ref / ppo_ref bounds: head log_prob 0.061, head entropy 0.052, dlogits 0.075, dvalues 0.48, loss 0.0022, policy_loss 0.0011, value_loss 0.067,
entropy_loss 0.021, approx_kl 0.0001, clip_fraction 0.26, adv_mean 0.45, adv_std 0.36, a propagated parameter bound 0.008.  G1: the logit difference
between the minibatch pass and the rollout pass (the normaliser's statistics moved in between, the policy did not) is at most 0.594 / 0.377 in iteration 1
and 0.138 / 0.118 in iteration 2; |log_prob - old_log_prob| reaches 0.70 of its bound.  Copies of this test with ppo_loss given nxt as the mask, gae_rows
given values shifted by one step or the observation records, and the statistics updated a second time at the iteration boundary each fail (191 rows
excluded; 4800, 2277 of 4800 advantages; obs_mean before step 0 of iteration 2)."""
import ctypes as C

import numpy as np
import pytest

from tests import encode_ref, gae_ref, head_ref, helpers, norm_ref, ppo_iter_ref as ref, ppo_ref
from tests.helpers import OBS_KEYS

pytestmark = pytest.mark.gpu

W = ref.WORKLOAD
_STATE = ("obs_mean", "obs_var", "obs_count", "ret_stats", "returns")


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {want.size} elements differ, first {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def _bits(t):
    """Device tensor -> its bit patterns on the host."""
    import torch
    it, nt = {2: (torch.int16, np.uint16), 4: (torch.int32, np.uint32), 8: (torch.int64, np.uint64)}[t.element_size()]
    return t.contiguous().view(it).cpu().numpy().view(nt)


def _state_bits(s):
    return {"obs_mean": norm_ref.bits64(s["obs_mean"]), "obs_var": norm_ref.bits64(s["obs_var"]), "obs_count": norm_ref.bits64([s["obs_count"]]),
            "ret_stats": norm_ref.bits64([s["ret_mean"], s["ret_var"], s["ret_count"]]), "returns": norm_ref.bits64(s["returns"])}


class _Probe:
    """The device's batch moments of the NEXT RowNormalizer update: the same C call on a copy of the state, moments_out set, no other output."""

    def __init__(self, norm):
        import torch
        from balatro_gym_amd import _native as nat
        self.L, self.nat, self.norm, self.N = nat.load(), nat, norm, norm.n
        self.need = int(self.L.bg_norm_workspace_bytes(1, C.c_int64(self.N)))
        self.ws = torch.empty(max(self.need, 16), dtype=torch.uint8, device=norm.device)

    def obs(self, live, mom):
        import torch
        n, p = self.norm, lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        mean, var, count = n.obs_mean.clone(), n.obs_var.clone(), n.obs_count.clone()
        rc = self.L.bg_norm_obs_rows(p(live), C.c_uint64(live.shape[-1]), 1, C.c_int64(self.N), self.nat.ENC_LAYOUTS["produced"], self.nat.ENC_F32, p(mean), p(var),
                                     p(count), 1, C.c_double(n.epsilon), C.c_double(n.clip_obs), None, C.c_uint64(norm_ref.COLS), p(mom), p(self.ws),
                                     C.c_uint64(self.need), None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, self.L.bg_last_error(None).decode()

    def reward(self, live, mom):
        import torch
        n, p = self.norm, lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        returns, stats = n.returns.clone(), n.ret_stats.clone()
        rc = self.L.bg_norm_reward_rows(p(live), C.c_uint64(live.shape[-1]), 1, C.c_int64(self.N), p(returns), p(stats), 1, C.c_double(n.gamma),
                                        C.c_double(n.epsilon), C.c_double(n.clip_reward), None, p(mom), p(self.ws), C.c_uint64(self.need), None,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, self.L.bg_last_error(None).decode()


def _snap(norm):
    return {k: getattr(norm, k).clone() for k in _STATE}


def _note(shares, new):
    for k, v in new.items():
        shares[k] = max(shares.get(k, 0.0), float(v))


@pytest.mark.parametrize("case", sorted(ref.CASES))
def test_two_ppo_iterations_against_the_oracle(case):
    import torch
    from balatro_gym_amd import BalatroVecEnv, EpisodeStats, RowNormalizer, gae_rows, ppo_loss
    layout, dtype = ref.CASES[case]
    tdt = torch.float32 if dtype == "float32" else torch.bfloat16
    N, K, D = W["N"], W["K"], encode_ref.COLS[layout]
    wl = helpers.sharded_workload("configs2", N, seed0=W["seed0"])
    env = BalatroVecEnv(N, wl["seeds"], obs_layout="rows", **dict(wl["env_kwargs"], max_ante=W["max_ante"]))
    helpers.apply_sharded_workload(env, wl, 0, N)
    orc = ref.make_oracles(wl["seeds"], wl["env_kwargs"]["scorer_jokers"], W["max_ante"], wl["jokers"])
    dev = env.device
    net = ref.make_net(D, W["net_seed"])
    twin = ref.make_net(D, W["net_seed"]).double()
    net = net.cuda()
    opt = torch.optim.SGD(net.parameters(), lr=W["lr"])
    norm, stats = RowNormalizer(N, dev), EpisodeStats(N, dev)
    probe = _Probe(norm)
    store = torch.zeros((K + 1, N, ref.STRIDE), dtype=torch.uint8, device=dev)
    obs, nxt = store[:K], store[1:]
    assert obs.is_contiguous() and nxt.is_contiguous() and env.obs_rows.shape == (N, ref.STRIDE)
    live = env.obs_rows

    state = norm_ref.new_state(N)          # the reference's VecNormalize, carried across the iterations
    carry, trs, shares, und_rows, last_store, x = None, [], {}, 0, None, None
    for it in range(W["iterations"]):
        # ------------------------------------------------------------------ the rollout: product calls only (and the probes beside them)
        logits_all = torch.zeros((K, N, 60), device=dev)
        actions, lp, en, values = (torch.zeros((K, N), dtype=d, device=dev) for d in (torch.int32, torch.float32, torch.float32, torch.float32))
        rn = torch.zeros((K, N), dtype=torch.float64, device=dev)
        x_all = torch.zeros((K + 1, N, D), dtype=tdt, device=dev)
        mo, mr = torch.zeros((K + 1, 2, norm_ref.COLS), dtype=torch.float64, device=dev), torch.zeros((K, 2), dtype=torch.float64, device=dev)
        snaps = [None] * (K + 1)
        store[0].copy_(live)
        if it == 0:   # VecNormalize.reset(): the reset observation updates the statistics
            probe.obs(live, mo[0])
            x = norm.normalize_obs(live, layout, tdt, update=True)
        x_all[0].copy_(x)
        snaps[0] = _snap(norm)
        for t in range(K):
            with torch.no_grad():
                out = net(x.float())
            logits_all[t].copy_(out[:, :60])
            values[t].copy_(out[:, 60])
            a = env.act(logits_all[t], seed=W["act_seed"], t=it * K + t, log_prob=lp[t], entropy=en[t])
            actions[t].copy_(a)
            env.step(a)
            store[t + 1].copy_(live)
            probe.reward(live, mr[t])
            rn[t].copy_(norm.normalize_reward(live))
            probe.obs(live, mo[t + 1])
            x = norm.normalize_obs(live, layout, tdt, update=True)
            x_all[t + 1].copy_(x)
            snaps[t + 1] = _snap(norm)
        with torch.no_grad():
            last_values = net(x.float())[:, 60].contiguous()
        adv, ret = gae_rows(nxt, values, last_values, ref.GAMMA, ref.GAE_LAMBDA, rewards=rn)
        ep_return, ep_len = stats.update(nxt)
        env.check()

        # ------------------------------------------------------------------ to the host; the oracle follows the GPU's actions
        store_h, actions_h, logits_h = store.cpu().numpy(), actions.cpu().numpy(), logits_all.cpu().numpy()
        lp_h, en_h, values_h, lastv_h, rn_h = lp.cpu().numpy(), en.cpu().numpy(), values.cpu().numpy(), last_values.cpu().numpy(), rn.cpu().numpy()
        x_bits, mo_h, mr_h = _bits(x_all), mo.cpu().numpy(), mr.cpu().numpy()
        snaps_h = [{k: _bits(v) for k, v in s.items()} for s in snaps]
        adv_h, ret_h = adv.cpu().numpy(), ret.cpu().numpy()
        tr = ref.collect_vectorised(orc, actions_h, wl["jokers"])
        trs.append(tr)
        rec = ref.records(tr, actions_h)
        what = f"{case} iteration {it}"

        # A: records and alignment
        got_obs, got_rew, got_act, got_term = ref.record_fields(store_h)
        for k in OBS_KEYS:
            _same(got_obs[k], tr["obs"][k], f"{what} A: store[t] key {k} against the oracle's o[t]")
        _same(got_rew[1:].view(np.uint64), tr["reward"].view(np.uint64), f"{what} A: store[t + 1] reward bits")
        _same(got_act[1:], actions_h, f"{what} A: store[t + 1] action")
        _same(got_term[1:], tr["done"].astype(np.uint8), f"{what} A: store[t + 1] terminated")
        if it == 0:
            assert not got_rew[0].any() and not got_act[0].any() and not got_term[0].any(), "the record of a reset carries a reward / action / terminated"
        else:
            _same(store_h[0], last_store, f"{what} A: store[0] against the previous iteration's store[K]")
        last_store = store_h[K].copy()

        # B: the head, against the oracle's mask of the observation the action was drawn from
        for t in range(K):
            r = head_ref.Reference(logits_h[t], tr["mask"][t], seed=W["act_seed"], index0=0, t=it * K + t)
            assert not r.degenerate.any()
            r.check_sampled(actions_h[t], f"{what} B step {t}", cap=False)
            und_rows += int((~r.decidable).sum())
            s_lp, s_en = r.check_stats(actions_h[t], lp_h[t], en_h[t], f"{what} B step {t}")
            _note(shares, {"head log_prob": s_lp, "head entropy": s_en})

        # C: the normaliser, call by call
        worst = [0.0, 0.0]
        def moments(got, batch, name):   # noqa: E306
            m, v = norm_ref.check_moments(got[0], got[1], batch, f"{what} C {name}")
            worst[0], worst[1] = max(worst[0], m), max(worst[1], v)
        def held(t, name):   # noqa: E306
            for k, w in _state_bits(state).items():
                _same(snaps_h[t][k], w, f"{what} C {name}: {k}")
        if it == 0:
            moments(mo_h[0], norm_ref.produced64(rec[0:1])[0], "reset observation")
            obs_n, state = ref.norm_obs_step(rec[0], mo_h[0], state)
            _same(x_bits[0], norm_ref.obs_bits(obs_n, layout, dtype), f"{what} C: normalised reset observation")
        held(0, "before step 0")
        for t in range(K):
            moments(mr_h[t], ref.returns_before_update(rec[t + 1], state), f"step {t} returns")
            rew_n, state = ref.norm_reward_step(rec[t + 1], mr_h[t], state)
            _same(rn_h[t].view(np.uint64), norm_ref.bits64(rew_n), f"{what} C step {t}: normalised reward")
            assert not state["returns"][tr["done"][t]].any(), "the return carry of a terminated env was not zeroed"
            moments(mo_h[t + 1], norm_ref.produced64(rec[t + 1:t + 2])[0], f"step {t} observation")
            obs_n, state = ref.norm_obs_step(rec[t + 1], mo_h[t + 1], state)
            _same(x_bits[t + 1], norm_ref.obs_bits(obs_n, layout, dtype), f"{what} C step {t}: normalised observation")
            held(t + 1, f"after step {t}")
        sd = norm.state_dict()
        for k, w in _state_bits(state).items():
            _same(sd[k].numpy().view(np.uint64), w, f"{what} C: state_dict()[{k}]")
        print(f"{what} C: worst |dmean| / bound {worst[0]:.4f}, worst |dvar| / bound {worst[1]:.4f}")

        # D: GAE (rn and values pinned, done from the oracle), and the off-by-one it must see
        want_a, want_r = gae_ref.gae(rn_h, tr["done"], values_h, lastv_h, ref.GAMMA, ref.GAE_LAMBDA)
        _same(gae_ref.bits32(adv_h), gae_ref.bits32(want_a), f"{what} D: advantages")
        _same(gae_ref.bits32(ret_h), gae_ref.bits32(want_r), f"{what} D: returns")
        shifted, _ = gae_ref.gae(rn_h, tr["done"], np.concatenate([values_h[1:], lastv_h[None]]), lastv_h, ref.GAMMA, ref.GAE_LAMBDA)
        assert (gae_ref.bits32(shifted) != gae_ref.bits32(adv_h)).any(), "values shifted by one step give the device's advantages: the workload cannot see it"

        # E: Monitor
        want_er, want_el, carry = ref.monitor_literal(tr["reward"], tr["done"], carry)
        _same(ep_return.cpu().numpy().view(np.uint64), want_er.view(np.uint64), f"{what} E: ep_return")
        _same(ep_len.cpu().numpy(), want_el, f"{what} E: ep_len")

        if it == 1:
            assert (logits_h.max(axis=-1) > logits_h.min(axis=-1)).all(), "iteration 2's logits are constant along a row"

        # ------------------------------------------------------------------ one epoch of minibatches
        rec_obs = rec[:K].reshape(K * N, ref.STRIDE)
        roll_logits, mask_flat = logits_h.reshape(K * N, 60), tr["mask"][:K].reshape(K * N, 60)
        for b, idx in enumerate(ref.minibatch_indices(K, N, W["batch"], W["perm_seed"] + it)):
            whatb = f"{what} minibatch {b}"
            ix, idx_dev = idx.numpy(), idx.to(dev)
            xm = norm.normalize_obs(obs, layout, tdt, index=idx_dev)
            out = net(xm.float())
            logits, v = out[:, :60], out[:, 60].contiguous()
            before = [p.detach().clone() for p in net.parameters()]
            loss, st = ppo_loss(logits, actions, lp, adv, obs, values=v, returns=ret, index=idx_dev, ent_coef=ref.ENT_COEF)
            opt.zero_grad()
            loss.backward()
            grads = [p.grad.detach().cpu().numpy().astype(np.float64) for p in net.parameters()]
            opt.step()
            for p, q in zip(net.parameters(), before):
                assert not torch.equal(p.detach(), q), f"{whatb} H: the SGD step left a parameter tensor unchanged"
            # F
            want_bits = ref.frozen_features(rec_obs[ix], state, layout, dtype)
            _same(_bits(xm), want_bits, f"{whatb} F: minibatch features")
            # G
            lg_h, v_h = logits.detach().cpu().numpy().copy(), v.detach().cpu().numpy()
            c = ref.make_case(lg_h, v_h, tr["mask"][:K], actions_h, lp_h, adv_h, ret_h, ix)
            cf = ppo_ref.ClosedForm(c, ref.CLIP, ref.ENT_COEF, ref.VF_COEF, True)
            raw, dl = st.raw.cpu().numpy(), st.dlogits.cpu().numpy()
            assert cf.excluded.sum() == 0 and raw[8] == 0.0, f"{whatb} G: {raw[8]} rows excluded: a stored action is invalid under the mask of its own observation"
            _note(shares, cf.check(dl, st.dvalues.cpu().numpy(), st.log_prob.cpu().numpy(), st.entropy.cpu().numpy(), raw, whatb + " G"))
            if b == 0:
                wrong = ppo_ref.ClosedForm(ref.make_case(lg_h, v_h, tr["mask"][1:], actions_h, lp_h, adv_h, ret_h, ix), ref.CLIP, ref.ENT_COEF, ref.VF_COEF, True)
                assert wrong.excluded.sum() > 0, "masks shifted by one step exclude no row: the workload cannot see it"
                # G1: the policy has not moved since the rollout; only the normaliser's statistics have
                roll = head_ref.Reference(roll_logits[ix], mask_flat[ix])
                rows = np.arange(c.m)
                dlog = np.where(cf.head.valid, np.abs(lg_h.astype(np.float64) - roll_logits[ix]), 0.0).max(axis=1)
                lpb = lambda r: 2.0 ** -17 + 2.0 ** -22 * np.abs(r.d[rows, cf.actions])   # noqa: E731
                gap = np.abs(st.log_prob.cpu().numpy().astype(np.float64) - lp_h.reshape(-1)[ix])
                print(f"{whatb} G1: largest logit difference between the minibatch pass and the rollout pass {dlog.max():.3e}; largest |log_prob - old_log_prob| "
                      f"{gap.max():.3e}, at most {(gap / (2.0 * dlog + lpb(cf.head) + lpb(roll))).max():.3f} of its bound")
                assert (gap <= 2.0 * dlog + lpb(cf.head) + lpb(roll)).all(), f"{whatb} G1"
                _note(shares, {"G1 logit difference": dlog.max()})
            # H: the float64 twin at the GPU's parameters, its outputs pinned to the GPU's
            twin.load_state_dict({k: q.double().cpu() for k, q in zip(twin.state_dict().keys(), before)})
            twin.zero_grad()
            x64 = torch.from_numpy(ref.bits_to_float32(want_bits, dtype)).double()
            out64 = twin(x64)
            pinned = out64 + (torch.from_numpy(np.concatenate([lg_h, v_h[:, None]], axis=1)).double() - out64).detach()
            _, loss64 = ppo_ref.torch_statement(c, ref.CLIP, ref.ENT_COEF, ref.VF_COEF, True, ~cf.excluded, params=(pinned[:, :60], pinned[:, 60]))
            loss64.backward()
            want = [p.grad.numpy() for p in twin.parameters()]
            W1, b1, W2, _ = (p.detach().numpy() for p in twin.parameters())
            B = np.concatenate([cf.grad_bound(cf.g, dl), (2.0 ** -22 * np.abs(cf.dvalues) + 1e-45)[:, None]], axis=1)
            und = ~cf.decidable   # (the contract lets such a row take either clip branch: both gradients are inside the row's bound)
            B[und, :60] += np.abs(cf.dlogits - cf.dlogits_other)[und]
            Dabs = np.abs(np.concatenate([cf.dlogits, cf.dvalues[:, None]], axis=1))
            _note(shares, {"H parameter gradient": ppo_ref.check_mlp_gradients(grads, want, ppo_ref.mlp_gradient_bounds(B, Dabs, (W1, b1), W2, x64.numpy(), forward_abs=True), whatb + " H ")})

    env.close()
    # ---------------------------------------------------------------------- what keeps all of the above from passing vacuously
    cond = ref.conditions(trs)
    total = W["iterations"] * K * N
    print(f"{case}: {cond}; {und_rows} of {total} head rows undecidable; largest shares of the bounds {({k: round(v, 4) for k, v in shares.items()})}")
    assert min(cond["terminated"]) >= 8 and min(cond["positions"]) >= 2, "too few terminated records"
    assert cond["spanning"] >= 1, "no episode spans the iteration boundary"
    assert und_rows <= head_ref.UNDECIDABLE_CAP * total, f"{und_rows} of {total} head rows undecidable"
