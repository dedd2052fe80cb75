#!/usr/bin/env python3
"""What does bg_step_many_rows (BalatroVecEnv.step_many with a RowBuffers) cost beside the two paths it sits between?

One process, 65 536 envs, BASELINE configs[2] set up as bench.py's `step_path` block does: 800 actions per env recorded from a policy rollout of a
twin handle (in pieces, with per-step buffers).  Three handles start from the same state and play the same games, each its own way:
  a  rollout(K, policy=POLICY_CYCLE3, t0=c, obs_buffers=RowBuffers)                      the engine's own rate (actions computed on the device)
  b  step_many(acts[c:c+K], obs_buffers=RowBuffers)                                      the caller's actions on the same engine
  c  step_many(acts[c:c+K], obs_buffers=ObsBuffers(steps=K), reward=..., terminated=...) the per-key path that keeps every step
At every position c the three are timed in turn (alternating: what else runs on the machine hits all three alike), at K = 100 and at K = 20 with
fresh handles, once by a host clock around the call and a synchronize with profiling off, once by the kernels' own events with profiling on.
At the end the three handles' observe() must be equal.  Prints min / p10 / median / p90 env-steps/s per mode and K and the ratios of medians."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=800)
    ap.add_argument("--ks", type=int, nargs="+", default=[100, 20])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("step_many_rows.py: no GPU is visible", file=sys.stderr)
        return 2
    import bench
    from balatro_gym_amd import BalatroVecEnv, _native as nat
    from balatro_gym_amd.vec_env import ObsBuffers, RowBuffers
    dev = torch.device("cuda:0")
    n, ks = args.envs, args.steps

    def make_env():
        e = BalatroVecEnv(n, [1000 + g for g in range(n)], device=0, scorer_jokers=True, autoreset=True, max_ante=bench.MAX_ANTE)
        e.inject(jokers=[bench.jokers_for(g) for g in range(n)], apply_now=True)
        return e

    twin = make_env()
    acts = torch.zeros((ks, n), dtype=torch.int32, device=dev)
    rec = 50
    rec_ob = ObsBuffers(n, dev, steps=rec)
    for c0 in range(0, ks, rec):
        twin.rollout(rec, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED, t0=c0, obs_buffers=rec_ob, actions=acts[c0:c0 + rec], zero_stats=c0 == 0)
    twin_stats = twin.stats()
    twin.close()
    del rec_ob
    print(f"build signature {nat.device_code_signature()}  library {os.path.basename(nat.lib_path())}")
    print(f"{n} envs, {ks} recorded steps (twin rollout: {twin_stats['plays']} plays, {twin_stats['episodes']} episodes), "
          f"{int((acts == 0).sum().item())} PLAY_HAND actions replayed; GPU {torch.cuda.get_device_name(0)}")

    def run(mode, env, c, K, bufs):
        if mode == "a":
            env.rollout(K, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED, t0=c, obs_buffers=bufs["a"])
        elif mode == "b":
            env.step_many(acts[c:c + K], obs_buffers=bufs["b"])
        else:
            env.step_many(acts[c:c + K], obs_buffers=bufs["c"], reward=bufs["rw"], terminated=bufs["tm"])

    def buffers(K):
        return {"a": RowBuffers(n, dev, steps=K, row_stride=384), "b": RowBuffers(n, dev, steps=K, row_stride=384), "c": ObsBuffers(n, dev, steps=K),
                "rw": torch.zeros((K, n), dtype=torch.float64, device=dev), "tm": torch.zeros((K, n), dtype=torch.uint8, device=dev)}

    # one warm-up pass of every shape (first-call costs: code object load, first touch of the buffers)
    for K in args.ks:
        bufs = buffers(K)
        for mode in "abc":
            e = make_env()
            run(mode, e, 0, K, bufs)
            torch.cuda.synchronize(dev)
            e.check()
            e.close()
        del bufs

    med = {}
    for K in args.ks:
        bufs = buffers(K)
        for profiled in (False, True):
            envs = {m: make_env() for m in "abc"}
            for e in envs.values():
                e.set_profiling(profiled)
            rates = {m: [] for m in "abc"}
            for c in range(0, ks - K + 1, K):
                for m in "abc":
                    e = envs[m]
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    run(m, e, c, K, bufs)
                    torch.cuda.synchronize(dev)
                    dt = time.perf_counter() - t0
                    if profiled:
                        p = e.get_profile()
                        dt = (p["step_ms"] if m == "c" else p["rollout_ms"]) * 1e-3
                    rates[m].append(n * K / dt)
            obs = {}
            for m, e in envs.items():
                e.check()
                obs[m] = {k: v.clone() for k, v in e.observe().items()}
                e.close()
            for m in "bc":
                for k in obs["a"]:
                    if not torch.equal(obs["a"][k], obs[m][k]):
                        print(f"step_many_rows.py: mode {m} ended in another state than the rollout (key {k})", file=sys.stderr)
                        return 1
            what = "kernel time (events)" if profiled else "wall clock (host)"
            print(f"\nK = {K}, {what}, {len(rates['a'])} calls per mode, env-steps/s [G]: min / p10 / median / p90")
            for m, name in (("a", "a rollout rows      "), ("b", "b step_many rows    "), ("c", "c step_many per-key ")):
                r = np.array(rates[m]) / 1e9
                q = (r.min(), np.percentile(r, 10), np.median(r), np.percentile(r, 90))
                med[(K, profiled, m)] = q
                print(f"  {name} {q[0]:7.3f} / {q[1]:7.3f} / {q[2]:7.3f} / {q[3]:7.3f}")
            ma, mb, mc = (med[(K, profiled, m)][2] for m in "abc")
            print(f"  median b / c = {mb / mc:.2f}   median b / a = {mb / ma:.3f}   (p10 of a = {med[(K, profiled, 'a')][1]:.3f}: b is "
                  f"{'inside' if mb >= med[(K, profiled, 'a')][1] else 'BELOW'} the spread of a)")
            print("  final observe() of the three handles: equal")
        del bufs
    return 0


if __name__ == "__main__":
    sys.exit(main())
