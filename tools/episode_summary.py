#!/usr/bin/env python3
"""What does the episode summary cost on bg_step_many_rows_ex, and what does bg_episode_ends_rows cost against what a user had before it?

    python tools/episode_summary.py --parent-tree DIR [--repeats 3] [--out profiles/episode_summary.txt]

tools/step_many_safe.py's method: every measurement is taken by WORKER processes (this file with --worker), the builds alternating, each worker on a
fresh handle: 65 536 envs, BASELINE configs[2] as bench.py sets it up, the uniform policy's actions recorded from a prior rollout of a twin handle
and replayed K steps per call under the limits 50 / 1000.
  safe workers   step_many(acts, obs_buffers=RowBuffers, limits=...) on the parent's tree, on this one with the switch off and with it on, one handle
                 per worker.  "Off" is judged against the spread of the parent's own workers; "on" is reported as a ratio of medians.
  scan worker    on records this build made with the switch on, [100, N] at N = 65 536 and 4 096: RowCurriculum.update (kernel time from the
                 library's events, and the whole call with its 8-byte synchronisation) against (a) a torch composite over the strided views --
                 mask, bincount, sums, maxima -- which gives the report only, and (b) sb3_adapter.CurriculumTracker.update fed step by step from
                 device-to-host copies of the two views, on a stand-in env.
--parent-tree: a built checkout of the parent commit (its own package and library)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = (50, 1000)


def _setup(tree):
    sys.path.insert(0, tree)
    import torch
    if not torch.cuda.is_available():
        print("episode_summary.py: no GPU is visible", file=sys.stderr)
        sys.exit(2)
    import bench
    from balatro_gym_amd import BalatroVecEnv, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers

    def make_env(n):
        e = BalatroVecEnv(n, [1000 + g for g in range(n)], device=0, scorer_jokers=True, autoreset=True, max_ante=bench.MAX_ANTE)
        e.inject(jokers=[bench.jokers_for(g) for g in range(n)], apply_now=True)
        return e

    def record(n, ks):
        twin = make_env(n)
        acts = torch.zeros((ks, n), dtype=torch.int32, device="cuda:0")
        rb = RowBuffers(n, torch.device("cuda:0"), steps=50, row_stride=384)
        for c0 in range(0, ks, 50):
            twin.rollout(50, policy=nat.POLICY_UNIFORM, policy_seed=bench.POLICY_SEED, t0=c0, obs_buffers=rb, zero_stats=c0 == 0)
            acts[c0:c0 + 50] = rb.action[:50]
        twin.close()
        return acts
    return torch, nat, RowBuffers, make_env, record


def safe_worker(args):
    tree = os.path.abspath(args.tree or ROOT)
    torch, nat, RowBuffers, make_env, record = _setup(tree)
    from balatro_gym_amd import EpisodeLimits
    n, ks = args.envs, args.steps
    acts = record(n, ks)
    out = {"signature": nat.device_code_signature(), "envs": n, "gpu": torch.cuda.get_device_name(0), "rates": {}}
    for K in args.ks:
        env = make_env(n)
        rb = RowBuffers(n, env.device, steps=K, row_stride=384)
        lim = EpisodeLimits(n, env.device, *LIMITS, steps=K) if args.summary < 0 else EpisodeLimits(n, env.device, *LIMITS, steps=K, summary=bool(args.summary))
        env.step_many(acts[:K], obs_buffers=rb, limits=lim)   # warm-up, not timed: the recording's first call
        torch.cuda.synchronize()
        rates = []
        for c in range(K, ks - K + 1, K):
            t0 = time.perf_counter()
            env.step_many(acts[c:c + K], obs_buffers=rb, limits=lim)
            torch.cuda.synchronize()
            rates.append(n * K / (time.perf_counter() - t0) / 1e9)
        env.check()
        q = {"median": float(np.median(rates)), "p10": float(np.percentile(rates, 10)), "p90": float(np.percentile(rates, 90)), "calls": len(rates),
             "ended_share": float((rb.terminated != 0).float().mean().item())}
        if args.summary > 0:
            q["summary_share"] = float((rb.end_ante != 0).float().mean().item())
        out["rates"][str(K)] = q
        env.close()
    print("RESULT " + json.dumps(out))
    return 0


class _StandIn:
    def __init__(self, n):
        self.num_envs, self.device = n, "cuda:0"

    def set_max_ante(self, max_ante, mask=None):
        pass


def scan_worker(args):
    torch, nat, RowBuffers, make_env, record = _setup(ROOT)
    from balatro_gym_amd import EpisodeLimits, RowCurriculum
    from balatro_gym_amd.sb3_adapter import CurriculumTracker
    K, out = 100, {"signature": nat.device_code_signature(), "gpu": torch.cuda.get_device_name(0), "scan": {}}
    for n in (65536, 4096):
        acts = record(n, 2 * K)
        env = make_env(n)
        rb = RowBuffers(n, env.device, steps=K, row_stride=384)
        lim = EpisodeLimits(n, env.device, *LIMITS, steps=K, summary=True)
        for c in (0, K):
            env.step_many(acts[c:c + K], obs_buffers=rb, limits=lim)
        env.check()
        env.close()
        cur = RowCurriculum(_StandIn(n), initial_max_ante=1, window=2)   # (a rule that fires on these records: caps rise, the apply path runs)
        kms, whole = [], []
        for r in range(args.reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rep, ms = cur.update(rb.rows, timing=True)
            torch.cuda.synchronize()
            if r >= 2:
                kms.append(ms); whole.append((time.perf_counter() - t0) * 1e3)
        whole_nt = []
        for r in range(args.reps + 2):   # without the timing events
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rep = cur.update(rb.rows)
            torch.cuda.synchronize()
            if r >= 2:
                whole_nt.append((time.perf_counter() - t0) * 1e3)

        def composite():
            ended = rb.terminated != 0
            fl = rb.end_flags[ended]
            ante = rb.end_ante[ended].to(torch.int64)
            chips = rb.end_chips.to(torch.int64)[ended]   # (torch indexes no uint32 tensor on the device: widen first)
            return torch.stack([ended.sum(), (fl & 1 != 0).sum(), (fl & 2 != 0).sum(), (fl == 4).sum(), ante.sum(), ante.max() if ante.numel() else ante.sum(),
                                chips.sum(), chips.max() if chips.numel() else chips.sum()]), torch.bincount(ante.clamp(max=15), minlength=16)
        comp = []
        for r in range(args.reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a, h = composite()
            torch.cuda.synchronize()
            if r >= 2:
                comp.append((time.perf_counter() - t0) * 1e3)
        agree = a.tolist() == rep[:8].tolist() and h[1:].tolist() == rep[17:32].tolist()
        trk = CurriculumTracker(_StandIn(n), initial_max_ante=1, window=2)
        t0 = time.perf_counter()
        for t in range(K):
            trk.update(rb.terminated[t].cpu().numpy() != 0, rb.end_ante[t].cpu().numpy())
        host = (time.perf_counter() - t0) * 1e3
        med = lambda x: float(np.median(x))   # noqa: E731
        out["scan"][str(n)] = {"kernel_ms": med(kms), "call_ms_timed": med(whole), "call_ms": med(whole_nt), "composite_ms": med(comp), "tracker_ms": host,
                               "ended": int(rep[0].item()), "raised": int(rep[8].item()), "composite_agrees": bool(agree), "records": n * K}
    print("RESULT " + json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=["safe", "scan"], default=None)
    ap.add_argument("--tree", default=None)
    ap.add_argument("--summary", type=int, default=-1, help="safe worker: -1 = the tree has no switch (the parent), 0 / 1 = off / on")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--ks", type=int, nargs="+", default=[100, 20])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "episode_summary.txt"))
    args = ap.parse_args()
    if args.worker:
        return safe_worker(args) if args.worker == "safe" else scan_worker(args)
    lines = []
    say = lambda s="": (lines.append(s), print(s, flush=True))   # noqa: E731
    results = {"parent": [], "off": [], "on": [], "scan": []}
    order = ((["parent"] if args.parent_tree else []) + ["off", "on"]) * args.repeats + ["scan"]
    for who in order:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "scan" if who == "scan" else "safe", "--envs", str(args.envs), "--steps", str(args.steps),
               "--ks", *map(str, args.ks), "--reps", str(args.reps)]
        if who == "parent":
            cmd += ["--tree", args.parent_tree, "--summary", "-1"]
        elif who != "scan":
            cmd += ["--summary", "1" if who == "on" else "0"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        res = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
            print(f"episode_summary.py: a {who} worker failed ({p.returncode}): nothing more is started", file=sys.stderr)
            return 1
        results[who].append(json.loads(res[-1][7:]))
        print(f"  ({who}: {res[-1][7:]})", flush=True)
    r0 = results["off"][0]
    say(f"tools/episode_summary.py: bg_step_many_rows_ex with limits {LIMITS[0]} / {LIMITS[1]}, {r0['envs']} envs, {args.steps} recorded steps of the uniform policy, GPU {r0['gpu']}")
    say(f"this build {r0['signature']}" + (f", parent build {results['parent'][0]['signature']}" if results["parent"] else "") +
        f"; {args.repeats} worker processes per variant, alternating, one handle each; host clock around call + synchronize; env-steps/s [G]")
    med = lambda who, K: [w["rates"][str(K)]["median"] for w in results[who]]   # noqa: E731
    for K in args.ks:
        say(f"\nK = {K} steps per call ({r0['rates'][str(K)]['calls']} timed calls per worker; ended steps {r0['rates'][str(K)]['ended_share']:.4f} of all)")
        for who, name in (("parent", "parent"), ("off", "this build, switch off"), ("on", "this build, switch on")):
            if results[who]:
                ms = med(who, K)
                say(f"  {name:24s} medians of the workers {' / '.join(f'{x:.3f}' for x in ms)}  -> median {np.median(ms):.3f}")
        if results["parent"]:
            pp, off = med("parent", K), np.median(med("off", K))
            lo, hi = min(pp), max(pp)
            say(f"  switch off against the parent: the parent's workers span {lo:.3f} .. {hi:.3f} ({100 * (hi - lo) / np.median(pp):.1f} % of their median); this build's median "
                f"{off:.3f} is {100 * (off / np.median(pp) - 1):+.1f} % of the parent's: {'inside' if lo <= off <= hi else 'above' if off > hi else 'BELOW'} that span")
        say(f"  switch on / switch off (medians): {np.median(med('on', K)) / np.median(med('off', K)):.3f}")
    say("\nbg_episode_ends_rows with a curriculum (window 2, so that caps rise), K = 100, records of stride 384 made with the switch on; medians of "
        f"{args.reps} calls, milliseconds")
    for n, s in results["scan"][0]["scan"].items():
        say(f"  N = {n}: {s['records']} records, {s['ended']} ended, {s['raised']} envs raised")
        say(f"    kernel {s['kernel_ms']:.3f} ms = {s['records'] * 128 / s['kernel_ms'] / 1e6:.0f} GB/s at one 128-byte line per record; whole RowCurriculum.update call "
            f"{s['call_ms']:.3f} ms ({s['call_ms_timed']:.3f} with the timing events)")
        say(f"    torch composite over the views (report only; agrees: {s['composite_agrees']}): {s['composite_ms']:.3f} ms = {s['composite_ms'] / s['call_ms']:.1f} x the call")
        say(f"    CurriculumTracker.update per step from device-to-host copies of terminated / end_ante: {s['tracker_ms']:.1f} ms = {s['tracker_ms'] / s['call_ms']:.0f} x the call")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
