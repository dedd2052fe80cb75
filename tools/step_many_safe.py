#!/usr/bin/env python3
"""What do SafeBalatroEnv's episode limits cost inside bg_step_many_rows_ex, and did adding them change bg_step_many_rows?

    python tools/step_many_safe.py [--parent-tree DIR] [--repeats 3] [--out profiles/step_many_safe.txt]

Every measurement is taken by WORKER processes (this file with --worker), several per build, the builds alternating, each worker on a fresh handle set:
65 536 envs, BASELINE configs[2] as bench.py sets it up, the uniform policy's actions recorded from a prior rollout of a twin handle (as
tools/step_many_rows.py does).  Handles that start from the same state then replay them, K steps per call, the modes in turn at every position (the
order of the turn rotating from one position to the next):
  p   step_many(acts, obs_buffers=RowBuffers)                          bg_step_many_rows, the unwrapped call
  s   step_many(acts, obs_buffers=RowBuffers, limits=50 / 1000)        the same masked actions under the limits
  pi  as p, with the out-of-range action 60 inserted in front of about every fifth step (drawn once, seeded; the recorded actions stay valid)
  si  as s, with those actions
  ad  BalatroSB3VecEnv(as_torch=True).step, one call per step           what a user has today for these semantics
--parent-tree: a built checkout of the parent commit (its own package and library).  "Unchanged" is judged between workers that run mode p ALONE, the
parent's and this build's alternating (a worker that times four handles in turn finds its state evicted from the caches by the other three, which a
worker with one handle does not); the ratios s / p and si / pi come from workers that run all modes.  The report states, per K, the median
env-steps/s of every worker, the spread of the parent's workers and where this build's median of medians lies in it; then the code-object metadata (VGPRs, SGPRs, scratch, LDS) of every bg_engine3_kernel instantiation of both libraries, the SAFE flag
stripped from the names so that the pre-existing instantiations pair up."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = (50, 1000)


def worker(args):
    tree = os.path.abspath(args.tree or ROOT)
    sys.path.insert(0, tree)
    import torch
    if not torch.cuda.is_available():
        print("step_many_safe.py: no GPU is visible", file=sys.stderr)
        return 2
    import bench
    from balatro_gym_amd import BalatroVecEnv, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers
    dev = torch.device("cuda:0")
    n, ks = args.envs, args.steps
    modes = args.modes.split(",")

    def make_env():
        e = BalatroVecEnv(n, [1000 + g for g in range(n)], device=0, scorer_jokers=True, autoreset=True, max_ante=bench.MAX_ANTE)
        e.inject(jokers=[bench.jokers_for(g) for g in range(n)], apply_now=True)
        return e

    twin = make_env()
    acts = torch.zeros((ks, n), dtype=torch.int32, device=dev)
    rec = 50
    rec_rb = RowBuffers(n, dev, steps=rec, row_stride=384)
    for c0 in range(0, ks, rec):
        twin.rollout(rec, policy=nat.POLICY_UNIFORM, policy_seed=bench.POLICY_SEED, t0=c0, obs_buffers=rec_rb, zero_stats=c0 == 0)
        acts[c0:c0 + rec] = rec_rb.action[:rec]
    twin.close()
    del rec_rb
    # the second action set: an out-of-range action (60) INSERTED in front of every fifth step or so (drawn once, seeded).  An invalid action leaves the
    # env as it was, so the recorded actions behind it meet the states they were recorded in and stay valid: about 20 % of the steps are invalid, no more
    gen = torch.Generator(device="cpu").manual_seed(20)
    ins = (torch.rand((ks, n), generator=gen) < 0.2).to(dev)
    src = ((~ins).cumsum(0) - 1).clamp_(min=0)
    acts_i = torch.where(ins, torch.full_like(acts, 60), acts.gather(0, src))
    del ins, src
    out = {"signature": nat.device_code_signature(), "tree": tree, "envs": n, "steps": ks, "gpu": torch.cuda.get_device_name(0), "rates": {}}

    for K in args.ks:
        use = [m for m in modes if m != "ad"]
        envs = {m: make_env() for m in use}
        bufs = {m: RowBuffers(n, dev, steps=K, row_stride=384) for m in use}
        lims = {}
        if any(m in ("s", "si") for m in use):
            from balatro_gym_amd import EpisodeLimits
            lims = {m: EpisodeLimits(n, dev, *LIMITS, steps=K) for m in use if m in ("s", "si")}

        def run(m, c):
            a = (acts_i if m in ("pi", "si") else acts)[c:c + K]
            if m in lims:
                envs[m].step_many(a, obs_buffers=bufs[m], limits=lims[m])
            else:
                envs[m].step_many(a, obs_buffers=bufs[m])
        for m in use:   # warm-up, not timed: code object load, first touch of the buffers.  It is the recording's first call; the timed ones go on from there
            run(m, 0)
        torch.cuda.synchronize(dev)
        rates = {m: [] for m in use}
        for c in range(K, ks - K + 1, K):
            first = (c // K) % len(use)   # the turn order rotates: the handle timed right behind another's 2.5 GB of records pays for it, and each is that one in turn
            for m in use[first:] + use[:first]:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                run(m, c)
                torch.cuda.synchronize(dev)
                rates[m].append(n * K / (time.perf_counter() - t0))
        for m in use:
            envs[m].check()
            r = np.array(rates[m]) / 1e9
            q = {"min": r.min(), "p10": np.percentile(r, 10), "median": np.median(r), "p90": np.percentile(r, 90), "calls": len(r)}
            if m in ("pi", "si"):
                q["invalid_share"] = float((bufs[m].reward == -1.0).float().mean().item())
            if m in lims:
                q["ended_share"] = float((bufs[m].terminated != 0).float().mean().item())
            out["rates"][f"{m}@{K}"] = {k: float(v) for k, v in q.items()}
            envs[m].close()
        del envs, bufs, lims
    if "ad" in modes:
        from balatro_gym_amd.sb3_adapter import BalatroSB3VecEnv
        venv = BalatroSB3VecEnv(n, seeds=[1000 + g for g in range(n)], max_invalid_actions=LIMITS[0], max_episode_steps=LIMITS[1], scorer_jokers=True,
                                max_ante=bench.MAX_ANTE, as_torch=True)
        venv.reset()
        T = min(ks, 200)
        for t in range(20):
            venv.step(acts[t])
        torch.cuda.synchronize(dev)
        per = []
        for t in range(20, T):
            t0 = time.perf_counter()
            venv.step(acts[t])
            torch.cuda.synchronize(dev)
            per.append(n / (time.perf_counter() - t0))
        r = np.array(per) / 1e9
        out["rates"]["ad@1"] = {"min": float(r.min()), "p10": float(np.percentile(r, 10)), "median": float(np.median(r)), "p90": float(np.percentile(r, 90)), "calls": len(r)}
        venv.close()
    print("RESULT " + json.dumps(out))
    return 0


def kernel_metadata(lib, pattern="bg_engine3_kernel"):
    """{kernel name: {vgpr, sgpr, scratch, lds, sgpr_spill, vgpr_spill}} of the gfx950 code object inside a built library (llvm-objcopy,
    clang-offload-bundler and llvm-readelf of the ROCm installation)."""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fatbin"), os.path.join(d, "co")
        subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fb])
        subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={fb}", f"--output={co}"])
        notes = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co], text=True)
    out = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if pattern in name:
            g = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))   # noqa: E731
            out[name] = {"vgpr": g("vgpr_count"), "sgpr": g("sgpr_count"), "scratch": g("private_segment_fixed_size"), "lds": g("group_segment_fixed_size"),
                         "sgpr_spill": g("sgpr_spill_count"), "vgpr_spill": g("vgpr_spill_count")}
    return out


def template_args(name):
    """bg_engine3_kernel<HASH, CARDS, NOW, KS, NSV, ACT[, SAFE]> from the mangled name: a tuple of ints, SAFE = 0 where the build has no such parameter."""
    args = re.search(r"bg_engine3_kernelI((?:L[bi]\d+E)+)E", name).group(1)
    v = [int(x) for x in re.findall(r"L[bi](\d+)E", args)]
    return tuple(v + [0] * (7 - len(v)))


def describe(targs):
    h, c, now, ks, nsv, act, safe = targs
    return f"{now}{ks}{nsv} {'hash ' if h else ''}{'cards ' if c else ''}{'SAFE' if safe else 'ACT' if act else 'policy'}".strip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=None)
    ap.add_argument("--modes", default="p,s,pi,si,ad")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=800)
    ap.add_argument("--ks", type=int, nargs="+", default=[100, 20])
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_many_safe.txt"))
    ap.add_argument("--metadata-only", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    lines = []
    say = lambda s="": (lines.append(s), print(s, flush=True))   # noqa: E731
    results = {"this": [], "parent": [], "this_p": []}
    if not args.metadata_only:
        order = (["parent", "this_p"] * args.repeats if args.parent_tree else []) + ["this"] * args.repeats
        for who in order:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--envs", str(args.envs), "--steps", str(args.steps), "--ks", *map(str, args.ks)]
            cmd += ["--tree", args.parent_tree, "--modes", "p"] if who == "parent" else ["--modes", "p" if who == "this_p" else args.modes]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            res = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not res:
                print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
                print(f"step_many_safe.py: a worker of the {who} build failed ({p.returncode}): nothing more is started", file=sys.stderr)
                return 1
            results[who].append(json.loads(res[-1][7:]))
        r0 = results["this"][0]
        say(f"tools/step_many_safe.py: {r0['envs']} envs, {r0['steps']} recorded steps of the uniform policy, limits {LIMITS[0]} / {LIMITS[1]}, GPU {r0['gpu']}")
        say(f"this build {r0['signature']}" + (f", parent build {results['parent'][0]['signature']}" if results["parent"] else "") +
            f"; {args.repeats} worker processes per build, alternating; host clock around call + synchronize; env-steps/s [G]")
        med = lambda who, key: [w["rates"][key]["median"] for w in results[who] if key in w["rates"]]   # noqa: E731
        for K in args.ks:
            say(f"\nK = {K} steps per call ({int(results['this'][0]['rates'][f'p@{K}']['calls'])} timed calls per mode and worker)")
            for who in ("parent", "this_p", "this"):
                for m, name in (("p", "bg_step_many_rows, policy's (masked) actions"), ("s", "  with limits"), ("pi", "bg_step_many_rows, 60 inserted at every fifth step"), ("si", "  with limits")):
                    ms = med(who, f"{m}@{K}")
                    if ms:
                        w0 = results[who][0]["rates"][f"{m}@{K}"]
                        extra = "".join(f", {k.replace('_', ' ')} {w0[k]:.3f}" for k in ("invalid_share", "ended_share") if k in w0)
                        say(f"  {who:6s} {m:2s} {name:45s} medians of the workers {' / '.join(f'{x:.3f}' for x in ms)}  -> median {np.median(ms):.3f}"
                            f"  (worker 1: min {w0['min']:.3f} p10 {w0['p10']:.3f} p90 {w0['p90']:.3f}{extra})")
            tp = med("this_p", f"p@{K}")
            if results["parent"]:
                pp = med("parent", f"p@{K}")
                lo, hi = min(pp), max(pp)
                say(f"  unchanged (workers with mode p alone)?  parent's workers span {lo:.3f} .. {hi:.3f} ({100 * (hi - lo) / np.median(pp):.1f} % of their median); this build's median "
                    f"{np.median(tp):.3f} is {100 * (np.median(tp) / np.median(pp) - 1):+.1f} % of the parent's: "
                    f"{'inside' if lo <= np.median(tp) <= hi else 'above' if np.median(tp) > hi else 'BELOW'} that span")
            for a, b, what in (("s", "p", "limits / unwrapped, masked actions"), ("si", "pi", "limits / unwrapped, about 20 % invalid actions")):
                ma, mb = med("this", f"{a}@{K}"), med("this", f"{b}@{K}")
                if ma and mb:
                    say(f"  {what}: {np.median(ma) / np.median(mb):.3f}")
        ad = med("this", "ad@1")
        if ad:
            say(f"\nBalatroSB3VecEnv(as_torch=True).step, one call per step: medians of the workers {' / '.join(f'{x:.4f}' for x in ad)} -> median {np.median(ad):.4f}")
            for K in args.ks:
                s = med("this", f"s@{K}")
                if s:
                    say(f"  step_many with limits at K = {K} is {np.median(s) / np.median(ad):.0f} x that")
    # code-object metadata
    libs = {"this": os.path.join(ROOT, "balatro_gym_amd", "libbalatro_mi355x.so")}
    if args.parent_tree:
        libs["parent"] = os.path.join(args.parent_tree, "balatro_gym_amd", "libbalatro_mi355x.so")
    meta = {who: {template_args(k): v for k, v in kernel_metadata(lib).items()} for who, lib in libs.items()}
    say("\ncode-object metadata of bg_engine3_kernel (VGPRs / SGPRs / scratch bytes per lane / LDS bytes / SGPR spills / VGPR spills)")
    fmt = lambda m: f"{m['vgpr']} / {m['sgpr']} / {m['scratch']} / {m['lds']} / {m['sgpr_spill']} / {m['vgpr_spill']}"   # noqa: E731
    same = True
    for targs in sorted(meta["this"]):
        line = f"  {describe(targs):24s} {fmt(meta['this'][targs])}"
        if "parent" in meta and not targs[6]:
            pm = meta["parent"].get(targs)
            eq = pm == meta["this"][targs]
            same = same and eq
            line += "   parent: equal" if eq else f"   parent: {fmt(pm) if pm else 'no such kernel'}  DIFFERENT"
        say(line)
    if "parent" in meta:
        say(f"  every pre-existing instantiation equal to the parent's: {'yes' if same and set(meta['parent']) <= set(meta['this']) else 'NO'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
