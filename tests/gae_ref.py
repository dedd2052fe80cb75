"""Numpy restatement of bg_gae_rows / bg_episode_stats_rows, shared by the host and the GPU tests.

`gae` is SB3's `RolloutBuffer.compute_returns_and_advantage` (stable_baselines3/common/buffers.py) verbatim on float32 arrays, fed the way
`add()` feeds it on the rows path: rewards[t] = float32(record reward), episode_starts[0] = False (irrelevant: never read), episode_starts[t + 1] =
dones[t] = the record's terminated byte of step t, and the `dones` argument = the last step's terminated byte.  `episode_stats` is Monitor's
per-episode sum / length as a forward scan with one np.float64 addition per step."""
import numpy as np

ROW_BYTES, ROW_REWARD, ROW_TERMINATED = 352, 136, 342


def pack_records(reward, terminated, stride, seed=0):
    """reward float64 [K, N], terminated [K, N] (0 = not, any other byte = terminated) -> uint8 [K, N, stride] records whose every other byte is
    0xa5 noise or random, so a kernel that reads a wrong offset fails."""
    reward = np.ascontiguousarray(reward, dtype=np.float64)
    terminated = np.ascontiguousarray(terminated, dtype=np.uint8)
    K, N = reward.shape
    assert terminated.shape == (K, N) and stride >= ROW_BYTES and stride % 16 == 0
    rows = np.full((K, N, stride), 0xa5, np.uint8)
    rng = np.random.default_rng(seed)
    rows[:, :, 128:136] = rng.integers(0, 256, (K, N, 8), dtype=np.uint8)    # chips_scored, just below the reward
    rows[:, :, 144:152] = rng.integers(0, 256, (K, N, 8), dtype=np.uint8)    # just above it
    rows[:, :, 336:352] = rng.integers(0, 256, (K, N, 16), dtype=np.uint8)   # around the terminated byte
    rows[:, :, ROW_REWARD:ROW_REWARD + 8] = reward.view(np.uint8).reshape(K, N, 8)
    rows[:, :, ROW_TERMINATED] = terminated
    return rows


def unpack_records(rows):
    """uint8 [K, N, stride] -> (reward float64 [K, N], terminated bool [K, N])."""
    rows = np.ascontiguousarray(rows)
    K, N, _ = rows.shape
    reward = np.ascontiguousarray(rows[:, :, ROW_REWARD:ROW_REWARD + 8]).view(np.float64).reshape(K, N)
    return reward, rows[:, :, ROW_TERMINATED] != 0


def gae(reward, terminated, values, last_values, gamma, gae_lambda):
    """(advantages, returns) float32 [K, N]."""
    K, N = reward.shape
    gamma, gae_lambda = float(gamma), float(gae_lambda)   # Python floats, as PPO holds them
    rewards = np.zeros((K, N), dtype=np.float32)
    episode_starts = np.zeros((K, N), dtype=np.float32)
    advantages = np.zeros((K, N), dtype=np.float32)
    values = np.array(values, dtype=np.float32).reshape(K, N)
    last_values = np.array(last_values, dtype=np.float32).reshape(N)
    done = np.asarray(terminated) != 0
    with np.errstate(over="ignore", invalid="ignore"):   # the +-1e30 rewards overflow on purpose
        for t in range(K):   # RolloutBuffer.add: self.rewards[pos] = np.array(reward); self.episode_starts[pos] = np.array(episode_start)
            rewards[t] = np.array(reward[t])
            episode_starts[t] = np.array(done[t - 1] if t else np.zeros(N, bool))
        dones = done[K - 1] if K else np.zeros(N, bool)
        # compute_returns_and_advantage(last_values, dones), from here on verbatim
        last_gae_lam = 0
        for step in reversed(range(K)):
            if step == K - 1:
                next_non_terminal = 1.0 - dones.astype(np.float32)
                next_values = last_values
            else:
                next_non_terminal = 1.0 - episode_starts[step + 1]
                next_values = values[step + 1]
            delta = rewards[step] + gamma * next_values * next_non_terminal - values[step]
            last_gae_lam = delta + gamma * gae_lambda * next_non_terminal * last_gae_lam
            advantages[step] = last_gae_lam
        returns = advantages + values
    assert advantages.dtype == np.float32 and returns.dtype == np.float32
    return advantages, returns


def episode_stats(reward, terminated, carry_return=None, carry_len=None):
    """Forward scan -> (ep_return float64 [K, N], ep_len int32 [K, N], carry_return float64 [N], carry_len int32 [N])."""
    K, N = reward.shape
    cr = np.zeros(N, np.float64) if carry_return is None else np.array(carry_return, dtype=np.float64)
    cl = np.zeros(N, np.int32) if carry_len is None else np.array(carry_len, dtype=np.int32)
    ep_r, ep_l = np.zeros((K, N), np.float64), np.zeros((K, N), np.int32)
    done = np.asarray(terminated) != 0
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(K):
            cr = cr + reward[t].astype(np.float64)
            cl = cl + np.int32(1)
            ep_r[t] = np.where(done[t], cr, 0.0)
            ep_l[t] = np.where(done[t], cl, 0)
            cr = np.where(done[t], 0.0, cr)
            cl = np.where(done[t], 0, cl).astype(np.int32)
    return ep_r, ep_l, cr, cl


GAMMA_LAMBDA = [(0.99, 0.95), (0.99, 1.0), (1.0, 1.0), (0.95, 0.9), (0.0, 0.5)]
SYN_K = (1, 2, 17, 372)
SYN_N = (1, 63, 64, 65, 1000)
DONE_PATTERNS = ("last", "first", "always", "never", "random")


def _halfway(rng, n):
    """float64 values exactly halfway between two neighbouring float32 values: ties go to the even one, up for some, down for others."""
    lo = rng.uniform(-100.0, 100.0, n).astype(np.float32)
    hi = np.nextafter(lo, np.float32(np.inf))
    return (lo.astype(np.float64) + hi.astype(np.float64)) / 2.0


def synthetic_rewards(K, N, seed):
    """float64 [K, N]: ordinary rewards, float32 ties, +-2**-140 (a float32 subnormal), +-1e30, -1.0, -50.0."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(-50.0, 100.0, (K, N))
    kind = rng.integers(0, 10, (K, N))
    half = _halfway(rng, K * N).reshape(K, N)
    r = np.where(kind == 0, half, r)
    r = np.where(kind == 1, np.where(rng.integers(0, 2, (K, N)) == 0, 2.0 ** -140, -2.0 ** -140), r)
    r = np.where(kind == 2, np.where(rng.integers(0, 2, (K, N)) == 0, 1e30, -1e30) * (rng.integers(0, 40, (K, N)) == 0), r)
    r = np.where(kind == 3, -1.0, r)
    r = np.where(kind == 4, -50.0, r)
    if K * N >= 4:   # every special kind at least once, whatever the draw
        flat = r.reshape(-1)
        flat[0], flat[1], flat[2], flat[3] = half[0, 0], 2.0 ** -140, -2.0 ** -140, 1e30
        if K * N >= 6:
            flat[4], flat[5] = -1e30, _halfway(rng, 1)[0]
    return np.ascontiguousarray(r)


def synthetic_done(K, N, pattern, seed):
    d = np.zeros((K, N), np.uint8)
    if pattern == "last":
        d[K - 1] = 1
    elif pattern == "first":
        d[0] = 1
    elif pattern == "always":
        d[:] = 1
    elif pattern == "random":
        rng = np.random.default_rng(seed)
        d = (rng.integers(0, 6, (K, N)) == 0).astype(np.uint8) * rng.integers(1, 256, (K, N)).astype(np.uint8)   # any nonzero byte is "terminated"
    return d


def synthetic_values(K, N, seed):
    """float32 [K, N] and [N]: mostly unit scale, some up to 1e6, some subnormal / zero."""
    rng = np.random.default_rng(seed + 1)
    v = rng.standard_normal((K + 1, N)).astype(np.float32)
    kind = rng.integers(0, 8, (K + 1, N))
    v = np.where(kind == 0, (rng.uniform(-1e6, 1e6, (K + 1, N))).astype(np.float32), v)
    v = np.where(kind == 1, np.float32(0.0), v)
    v = np.where(kind == 2, np.float32(2.0 ** -135), v).astype(np.float32)
    return np.ascontiguousarray(v[:K]), np.ascontiguousarray(v[K])


def synthetic_cases():
    """(K, N, pattern, (gamma, gae_lambda), stride, seed): every K x N, the done patterns, discount pairs and strides cycling through them so that each
    appears with each K and with each N."""
    out, i = [], 0
    for K in SYN_K:
        for N in SYN_N:
            for p, pattern in enumerate(DONE_PATTERNS):
                out.append((K, N, pattern, GAMMA_LAMBDA[(i + p) % len(GAMMA_LAMBDA)], (384, 352)[(i + p) % 2], 1000 + i))
                i += 1
    return out


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
