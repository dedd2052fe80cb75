"""GPU tests of envs ABOVE their curriculum cap on every step path.  The reference ends an episode on every step taken while state.ante >
current_max_ante (train_balatro_agent.py:147-152), whatever the action; a CHEAP step -- a toggle, a shop leave, a rejected action, settled on the
env's LDS image without a service wave -- has to send such an env to a service wave, which applies the rule (and the reset under auto-reset).
The scenario (tests/above_cap_ref.py; its contents are asserted by tests/test_above_cap_host.py): 300 envs, W warm-up steps, then the caps are
LOWERED below the ante of about half the envs, then K more steps -- with auto-reset on (one ending per lowered env) and off (the env stays above
its cap for all K steps, and further envs exceed their cap by play and are stepped on).  Every case holds every observation key or record byte,
the reward bits, the terminated bytes, the action word and (where the path has them) the info arrays against the CPU oracle, then the final
observe() and env.check().  The warm-up runs on the same handle through the path under test."""
import numpy as np
import pytest

from tests import above_cap_ref as ac
from tests import hash_ref
from tests.helpers import OBS_KEYS, POISON, assert_step_outputs, poison_, poison_env_outputs
from tests.test_gpu_parity import _StepBuffers, _assert_obs, _assert_poisoned, _obs_np, _vec
from tests.test_step_many_rows import _assert_records
from tests.test_step_many_safe import R_FLAGS, R_TERM, _diff, _terminal_sets

pytestmark = pytest.mark.gpu

N, W, K = ac.N, ac.W, ac.K
ONOFF = pytest.mark.parametrize("autoreset", [True, False], ids=["autoreset_on", "autoreset_off"])
STAT_KEYS = ("steps", "episodes", "plays", "score_sum", "reward_bits")


def _make(monkeypatch, autoreset, engine=None, cfg=None, **kw):
    """The scenario's handle: level-15 hands in the live state and the reset template, caps 3 + i % 2.  BG_ENGINE / BG_E3_CFG are read per handle."""
    if engine is not None:
        monkeypatch.setenv("BG_ENGINE", str(engine))
    if cfg is not None:
        monkeypatch.setenv("BG_E3_CFG", str(cfg))
    env = _vec(N, ac.seeds(), autoreset=autoreset, max_ante=0, **kw)
    env.inject(levels=np.full((N, 12), 15, np.uint8), apply_now=True)
    env.set_max_ante(ac.caps0())
    return env


def _finish(env, sc):
    _assert_obs({k: v.cpu().numpy() for k, v in env.observe().items()}, sc.final, "final observe()")
    env.check()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- one launch per step
@pytest.mark.parametrize("layout,autoreset,cards", [("keys", True, False), ("keys", False, False), ("keys", True, True), ("rows", True, False), ("rows", False, False)],
                         ids=["keys-autoreset_on", "keys-autoreset_off", "keys-autoreset_on-cards", "rows-autoreset_on", "rows-autoreset_off"])
def test_step_vs_oracle(monkeypatch, layout, autoreset, cards):
    """env.step, T = 1: the PROLOGUE of bg_engine_kernel<.., INFO> classifies the launch's only action (per key: bg_step; obs_layout="rows": bg_step_rows
    and its copiers).  Every output word of every step (tests/helpers.py assert_step_outputs: observation, reward bits, terminated, truncated, all 8
    info arrays with flags & 256 and BG_INFO_AUTORESET) in buffers poisoned before each call."""
    import torch
    sc = ac.scenario("caller", autoreset)
    env = _make(monkeypatch, autoreset, card_states=cards, **({"obs_layout": "rows"} if layout == "rows" else {}))
    for t in range(W + K):
        if t == W:
            env.set_max_ante(ac.caps1())
        poison_env_outputs(env)
        ob, reward, term, trunc, info = env.step(torch.from_numpy(np.array(sc.acts[t])).to(env.device))
        ctx = f"{layout} autoreset {autoreset} step {t}" + (" (the lowering)" if t == W else "")
        assert_step_outputs(ctx, sc.res[t], reward, term, trunc, info, obs=ob, autoreset=autoreset, want_obs=sc.want_obs[t])
        if layout == "rows":
            rows = env.obs_rows.cpu().numpy()
            assert not rows[:, 352:].any(), ctx
            assert np.array_equal(rows[:, 172:176].copy().view(np.int32)[:, 0], sc.acts[t]) and np.array_equal(rows[:, R_TERM], sc.terminated[t]), ctx
    _finish(env, sc)


# ---------------------------------------------------------------------------------------------------------------- bg_step_many, per key
@ONOFF
@pytest.mark.parametrize("keep", [True, False], ids=["per_step", "last_only"])
def test_step_many_keys_vs_oracle(monkeypatch, keep, autoreset):
    """bg_step_many through the C ABI (INFO, T > 1: cheap_step in the worker loop and in the further-cheap-steps loop), the warm-up as one call and
    the K steps behind the lowering as another: with [K, N, ...] buffers every step's outputs, with [N, ...] buffers the last step's."""
    sc = ac.scenario("caller", autoreset)
    env = _make(monkeypatch, autoreset)
    bufs = _StepBuffers(N, env.device, W if keep else 1)
    for lo, hi in ((0, W), (W, W + K)):
        if lo:
            env.set_max_ante(ac.caps1())
        bufs.poison()
        bufs.step_many(env, np.array(sc.acts[lo:hi]))
        for t in (range(lo, hi) if keep else [hi - 1]):
            ob, rw, tm, tr, info = bufs.row(t - lo if keep else 0)
            assert_step_outputs(f"keep {keep} autoreset {autoreset} step {t}", sc.res[t], rw, tm, tr, info, obs=ob, autoreset=autoreset, want_obs=sc.want_obs[t])
        if keep:
            _assert_poisoned(bufs.tensors()[1:] + list(bufs.ob.tensors.values()), hi - lo, f"steps {lo}..{hi}")
    _finish(env, sc)


# ---------------------------------------------------------------------------------------------------------------- bg_step_many_rows
def _step_many_rows(monkeypatch, autoreset, stride, engine, cfg):
    import torch
    from balatro_gym_amd.vec_env import RowBuffers
    sc = ac.scenario("caller", autoreset)
    env = _make(monkeypatch, autoreset, engine=engine, cfg=cfg)
    rb = RowBuffers(N, env.device, steps=W + 1, row_stride=stride)
    for lo, hi in ((0, W), (W, W + K)):
        if lo:
            env.set_max_ante(ac.caps1())
        poison_(rb.rows)
        env.step_many(torch.from_numpy(np.array(sc.acts[lo:hi])).to(env.device), obs_buffers=rb)
        got = rb.rows.cpu()
        for t in range(lo, hi):
            _assert_records(f"engine {engine} cfg {cfg} autoreset {autoreset} stride {stride} step {t}", got[t - lo], sc.res[t], sc.want_obs[t], sc.acts[t], stride)
        assert (got[hi - lo:].numpy() == POISON).all(), "rows past the call's last step were written"
        st, want = env.stats(), sc.stats(lo, hi)
        for key in STAT_KEYS:
            assert st[key] == want[key], (lo, key, st[key], want[key])
    _finish(env, sc)


@ONOFF
@pytest.mark.parametrize("stride", [352, 384])
def test_step_many_rows_engine1_vs_oracle(monkeypatch, stride, autoreset):
    """step_many with a RowBuffers on a BG_ENGINE=1 handle: bg_engine.h with actions_in and one copier wave, on both record strides."""
    _step_many_rows(monkeypatch, autoreset, stride, 1, None)


@ONOFF
@pytest.mark.parametrize("cfg", [113, 413])
def test_step_many_rows_engine3_vs_oracle(monkeypatch, cfg, autoreset):
    """The same on bg_engine3.h's action mode, whose owner waves load the cap (64 and 256 envs per workgroup): a control that passed before the
    other paths were mended."""
    _step_many_rows(monkeypatch, autoreset, 384, None, cfg)


# ---------------------------------------------------------------------------------------------------------------- rollouts (always auto-reset)
@pytest.mark.parametrize("hashed", [False, True], ids=["plain", "hash"])
def test_rollout_keys_engine1_vs_oracle(monkeypatch, hashed):
    """bg_rollout with one array per key (bg_engine.h, the policy on device, HASH off and on): W steps, the caps lowered, K steps -- every step's
    observation, reward bits, terminated byte and action, the stats, and the checksum against tests/hash_ref.py over the ORACLE's records."""
    import torch
    from balatro_gym_amd.vec_env import ObsBuffers
    sc = ac.scenario("policy", True)
    env = _make(monkeypatch, True)
    ob = ObsBuffers(N, env.device, steps=W)
    reward = torch.zeros((W, N), dtype=torch.float64, device=env.device)
    term = torch.zeros((W, N), dtype=torch.uint8, device=env.device)
    acts = torch.zeros((W, N), dtype=torch.int32, device=env.device)
    for lo, hi in ((0, W), (W, W + K)):
        if lo:
            env.set_max_ante(ac.caps1())
        poison_(ob.flat, reward, term, acts)
        env.rollout(hi - lo, policy=ac.POLICY | (0x100 if hashed else 0), policy_seed=ac.PSEED, t0=lo, obs_buffers=ob, reward=reward, terminated=term, actions=acts)
        k = hi - lo
        _diff(f"steps {lo}..: actions [step, env]", acts[:k].cpu().numpy(), sc.acts[lo:hi])
        _diff(f"steps {lo}..: terminated [step, env]", term[:k].cpu().numpy(), sc.terminated[lo:hi])
        _diff(f"steps {lo}..: reward bits [step, env]", reward[:k].cpu().numpy().view(np.uint64), sc.reward[lo:hi].view(np.uint64))
        for key in OBS_KEYS:
            _diff(f"steps {lo}..: obs[{key}]", ob.tensors[key][:k].cpu().numpy(), np.stack([sc.want_obs[t][key] for t in range(lo, hi)]))
        st, want = env.stats(), sc.stats(lo, hi, t0=lo)
        for key in STAT_KEYS:
            assert st[key] == want[key], (lo, key, st[key], want[key])
        if hashed:
            assert st["obs_hash"] == hash_ref.obs_hash(sc.records(lo, hi), t0=lo), f"steps {lo}..: obs_hash"
    _finish(env, sc)


def _rollout_rows(monkeypatch, engine, cfg, cards, hashed):
    from balatro_gym_amd.vec_env import RowBuffers
    sc = ac.scenario("policy", True)
    env = _make(monkeypatch, True, engine=engine, cfg=cfg, card_states=cards)
    rb = RowBuffers(N, env.device, steps=W + 1, row_stride=384)
    for lo, hi in ((0, W), (W, W + K)):
        if lo:
            env.set_max_ante(ac.caps1())
        poison_(rb.rows)
        env.rollout(hi - lo, policy=ac.POLICY | (0x100 if hashed else 0), policy_seed=ac.PSEED, t0=lo, obs_buffers=rb)
        k = hi - lo
        got, want = rb.rows.cpu().numpy(), sc.records(lo, hi)
        _diff(f"engine {engine} cfg {cfg} cards {cards} steps {lo}..: records [step, env, byte]", got[:k, :, :352], want)
        assert not got[:k, :, 352:].any() and (got[k:] == POISON).all()
        st, ws = env.stats(), sc.stats(lo, hi, t0=lo)
        for key in STAT_KEYS:
            assert st[key] == ws[key], (lo, key, st[key], ws[key])
        if hashed:
            assert st["obs_hash"] == hash_ref.obs_hash(want, t0=lo), f"steps {lo}..: obs_hash"
    _finish(env, sc)


@pytest.mark.parametrize("hashed", [False, True], ids=["plain", "hash"])
@pytest.mark.parametrize("cards", [False, True], ids=["nocards", "cards"])
@pytest.mark.parametrize("cfg", [113, 213, 413])
def test_rollout_rows_engine3_vs_oracle(monkeypatch, cfg, cards, hashed):
    """rollout with a RowBuffers on bg_engine3.h's POLICY mode, whose owner waves tested the ante against 100 alone: every workgroup shape, with and
    without card states, HASH off and on.  The caps are lowered between two launches; every record byte of both, the stats and the checksum."""
    _rollout_rows(monkeypatch, None, cfg, cards, hashed)


def test_rollout_rows_engine1_vs_oracle(monkeypatch):
    """The same on a BG_ENGINE=1 handle: bg_engine.h's policy mode with the copier wave."""
    _rollout_rows(monkeypatch, 1, None, False, True)


# ---------------------------------------------------------------------------------------------------------------- the wrappers of the record path
@pytest.mark.parametrize("cfg", [113, 413])
@pytest.mark.parametrize("progress", [False, True], ids=["safe", "progress"])
def test_step_many_rows_wrapped_vs_oracle(monkeypatch, progress, cfg):
    """step_many with EpisodeLimits (the SAFE instantiation) and with ProgressionRewards in front (PROG), the episode summary on, against OracleEnv +
    tests/safe_ref.py / tests/progress_ref.py: the ending a lowered cap forces is one the ENV made -- BG_END_GAME, the summary in bytes 344..351, the
    limits' counters and the progression carry back at their reset values -- on a toggle as on any other action.  Every record byte, the shaped
    reward bits, the terminal records, the counters and the carry of both calls."""
    import torch
    from balatro_gym_amd import EpisodeLimits, ProgressionRewards
    from balatro_gym_amd.vec_env import RowBuffers
    calls, cap_ended = ac.wrapped(progress)
    env = _make(monkeypatch, True, cfg=cfg)
    rb = RowBuffers(N, env.device, steps=W + 1, row_stride=384)
    lim = EpisodeLimits(N, env.device, *ac.WRAP_LIMITS, steps=W, row_stride=384, summary=True, progression=progress)
    prog = ProgressionRewards(N, env.device) if progress else None
    for gi, (acts, want, term, counters, carry) in enumerate(calls):
        if gi:
            env.set_max_ante(ac.caps1())
        k = len(acts)
        terminal = {(t, e): rec for t, e, rec in term}
        poison_(rb.rows); poison_(lim.terminal_rows); poison_(lim.terminal_step)
        env.step_many(torch.from_numpy(np.array(acts)).to(env.device), obs_buffers=rb, limits=lim, progression=prog)
        ctx = f"progress {progress} cfg {cfg} call {gi}"
        got = rb.rows.cpu().numpy()
        _diff(f"{ctx}: reward bits [step, env]", got[:k, :, 136:144].copy().view(np.uint64)[:, :, 0], want[:, :, 136:144].copy().view(np.uint64)[:, :, 0])
        _diff(f"{ctx}: end flags [step, env]", got[:k, :, R_FLAGS], want[:, :, R_FLAGS])
        _diff(f"{ctx}: records [step, env, byte]", got[:k, :, :352], want)
        assert not got[:k, :, 352:].any() and (got[k:] == POISON).all(), ctx
        sets, ts, trows = _terminal_sets(lim, N)
        assert set(sets) == set(terminal), (ctx, sorted(set(sets) ^ set(terminal))[:8])
        for key, rec in terminal.items():
            _diff(f"{ctx}: terminal record of (step, env) {key}", sets[key], rec)
        assert (trows[ts < 0] == POISON).all(), f"{ctx}: a terminal slot that was not used was written"
        cn = lim.counters.cpu().numpy()
        _diff(f"{ctx}: the limits' counters", cn[:, :2], counters)
        _diff(f"{ctx}: wrapper endings counted per env", cn[:, 2], np.bincount([e for _, e in terminal], minlength=N).astype(np.int32))
        if progress:
            _diff(f"{ctx}: the progression carry", prog.counters.cpu().numpy(), carry)
        st = env.stats()
        assert st["steps"] == N * k and st["episodes"] == int((want[:, :, R_TERM] != 0).sum()), (ctx, st)
    env.check()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- the route a user takes
def test_curriculum_checkpoint_lowers_caps_vs_oracle(monkeypatch):
    """RowCurriculum.load_state_dict(apply=True) with a checkpoint whose caps lie below the antes of running envs, followed by one step_many: the
    records equal the oracle's after set_max_ante to the same values."""
    import torch
    from balatro_gym_amd.vec_env import RowBuffers, RowCurriculum
    sc = ac.scenario("caller", True)
    monkeypatch.delenv("BG_ENGINE", raising=False)
    env = _vec(N, ac.seeds(), autoreset=True, max_ante=0)
    env.inject(levels=np.full((N, 12), 15, np.uint8), apply_now=True)
    cur = RowCurriculum(env, initial_max_ante=4)   # (sets one cap for every env: the scenario's per-env caps follow)
    env.set_max_ante(ac.caps0())
    cur.cap.copy_(torch.from_numpy(ac.caps0()).to(env.device))
    rb = RowBuffers(N, env.device, steps=W, row_stride=384)
    env.step_many(torch.from_numpy(np.array(sc.acts[:W])).to(env.device), obs_buffers=rb)
    _diff("warm-up: records", rb.rows[:W].cpu().numpy()[:, :, :352], sc.records(0, W))
    state = cur.state_dict()
    assert np.array_equal(state["cap"].numpy(), ac.caps0())
    state["cap"] = torch.from_numpy(ac.caps1())
    cur.load_state_dict(state, apply=True)
    assert np.array_equal(cur.cap.cpu().numpy(), ac.caps1())
    poison_(rb.rows)
    env.step_many(torch.from_numpy(np.array(sc.acts[W:])).to(env.device), obs_buffers=rb)
    got = rb.rows.cpu()
    for t in range(W, W + K):
        _assert_records(f"behind load_state_dict, step {t}", got[t - W], sc.res[t], sc.want_obs[t], sc.acts[t], 384)
    _finish(env, sc)
