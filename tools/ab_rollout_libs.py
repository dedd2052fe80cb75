#!/usr/bin/env python3
"""A/B of the headline path between two builds of the library: rollout() with packed records (RowBuffers, stride 384) at 65 536 envs, BASELINE
configs[2], T = 20 and T = 372, one child process per library and repetition (BALATRO_MI355X_LIB selects the library when it is loaded),
the two libraries alternating.  The driver itself never opens the GPU; it stops at the first child that fails or runs out of time.

    python tools/ab_rollout_libs.py name_a=/path/liba.so[:/path/of/that/checkout] name_b=/path/libb.so [--reps 4]

Prints p10 / median / p90 of the per-call env-steps/s (host clock around the call and a synchronize) per library and T, and whether the
second library's medians lie inside the first one's p10-p90."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if os.environ.get("AB_PACKAGE_ROOT"):   # a library of another commit goes with that commit's Python package (its binding lists other symbols)
    sys.path.insert(0, os.environ["AB_PACKAGE_ROOT"])


def child():
    import torch
    if not torch.cuda.is_available():
        print("ab_rollout_libs.py: no GPU is visible", file=sys.stderr)
        return 2
    import bench
    from balatro_gym_amd import BalatroVecEnv, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers
    n = 65536
    env = BalatroVecEnv(n, [1000 + g for g in range(n)], device=0, scorer_jokers=True, autoreset=True, max_ante=bench.MAX_ANTE)
    env.inject(jokers=[bench.jokers_for(g) for g in range(n)], apply_now=True)
    out = {"signature": nat.device_code_signature()}
    t0s = 0
    for T, calls in ((20, 40), (372, 6)):
        rb = RowBuffers(n, env.device, steps=T, row_stride=384)
        rates = []
        for c in range(calls + 2):   # (two warm-up calls per shape)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.rollout(T, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED, t0=t0s, obs_buffers=rb, zero_stats=False)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            t0s += T
            if c >= 2:
                rates.append(n * T / dt)
        out[str(T)] = rates
        del rb
    env.check()
    out["stats"] = env.stats()
    env.close()
    print("AB " + json.dumps(out))
    return 0


def main():
    if "--child" in sys.argv:
        return child()
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs=2, help="name=path of the two libraries (the first is the reference)")
    ap.add_argument("--reps", type=int, default=4)
    args = ap.parse_args()
    libs = [l.split("=", 1) for l in args.libs]
    res = {name: {"20": [], "372": []} for name, _ in libs}
    sig, stats = {}, {}
    for rep in range(args.reps):
        for name, path in libs:
            path, _, pkg = path.partition(":")
            env = dict(os.environ, BALATRO_MI355X_LIB=os.path.abspath(path))
            if pkg:
                env["AB_PACKAGE_ROOT"] = os.path.abspath(pkg)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=170)
            line = [l for l in p.stdout.splitlines() if l.startswith("AB ")]
            if p.returncode != 0 or not line:
                print(f"ab_rollout_libs.py: {name} repetition {rep} failed (exit {p.returncode}); stopping\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", file=sys.stderr)
                return 1
            r = json.loads(line[0][3:])
            sig[name] = r["signature"]
            stats.setdefault(name, r["stats"])
            if stats[name] != r["stats"]:
                print(f"ab_rollout_libs.py: {name} did not play the same games in every repetition", file=sys.stderr)
                return 1
            for T in ("20", "372"):
                res[name][T] += r[T]
    names = [n_ for n_, _ in libs]
    if stats[names[0]] != stats[names[1]]:
        print(f"ab_rollout_libs.py: the two libraries computed different rollouts: {stats}", file=sys.stderr)
        return 1
    print(f"rollout(T, RowBuffers stride 384), 65 536 envs, configs[2]; {args.reps} alternating processes per library; env-steps/s [G] p10 / median / p90")
    q = {}
    for name in names:
        for T in ("20", "372"):
            r = np.array(res[name][T]) / 1e9
            q[(name, T)] = (np.percentile(r, 10), np.median(r), np.percentile(r, 90))
            print(f"  {name:8s} {sig[name]}  T = {T:>3s}  {len(r):3d} calls  {q[(name, T)][0]:6.3f} / {q[(name, T)][1]:6.3f} / {q[(name, T)][2]:6.3f}")
    for T in ("20", "372"):
        lo, _, hi = q[(names[0], T)]
        m = q[(names[1], T)][1]
        print(f"  T = {T}: median of {names[1]} {m:.3f} is {'inside' if lo <= m <= hi else ('ABOVE' if m > hi else 'BELOW')} {names[0]}'s p10-p90 [{lo:.3f}, {hi:.3f}]")
    print(f"  identical rollout statistics on both: {stats[names[0]]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
