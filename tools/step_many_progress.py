#!/usr/bin/env python3
"""What does ProgressionRewardWrapper cost inside bg_step_many_rows_progress, and did adding it change bg_step_many_rows / bg_step_many_rows_ex?

    python tools/step_many_progress.py [--parent-tree DIR] [--repeats 3] [--out profiles/step_many_progress.txt]

As tools/step_many_safe.py: every measurement is taken by WORKER processes (this file with --worker), several per build, the builds alternating, each
worker on fresh handles: 65 536 envs, BASELINE configs[2] as bench.py sets it up, the uniform policy's actions recorded from a prior rollout of a twin
handle.  Handles that start from the same state then replay them, K steps per call, the modes in turn at every position (the order rotating):
  p   step_many(acts, obs_buffers=RowBuffers)                                            bg_step_many_rows
  s   step_many(acts, obs_buffers=RowBuffers, limits=50 / 1000)                          bg_step_many_rows_ex
  g   step_many(acts, obs_buffers=RowBuffers, limits=50 / 1000, progression=...)         bg_step_many_rows_progress
(under g an env is ended after 301 steps on ante 1, so from there on its recorded actions meet other states than they were recorded in: some become
invalid actions, which every mode handles; the share of ended steps is reported).
--parent-tree: a built checkout of the parent commit (its own package and library).  "Unchanged" is judged between workers that run mode p ALONE and
workers that run mode s ALONE, the parent's and this build's alternating; the ratio g / s comes from workers that run all three modes.  The report
states, per K, the median env-steps/s of every worker, the spread of the parent's workers and where this build's median of medians lies in it; then the
code-object metadata (VGPRs, SGPRs, scratch, LDS, spills -- the figures -Rpass-analysis=kernel-resource-usage prints) of every engine-3 kernel of both
libraries: the before / after table."""
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
MODES = {"p": "bg_step_many_rows", "s": "bg_step_many_rows_ex, limits", "g": "bg_step_many_rows_progress, limits + progression"}


def worker(args):
    tree = os.path.abspath(args.tree or ROOT)
    sys.path.insert(0, tree)
    import torch
    if not torch.cuda.is_available():
        print("step_many_progress.py: no GPU is visible", file=sys.stderr)
        return 2
    import bench
    import balatro_gym_amd
    from balatro_gym_amd import BalatroVecEnv, EpisodeLimits, _native as nat
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
    out = {"signature": nat.device_code_signature(), "tree": tree, "envs": n, "steps": ks, "gpu": torch.cuda.get_device_name(0), "rates": {}}
    for K in args.ks:
        envs = {m: make_env() for m in modes}
        bufs = {m: RowBuffers(n, dev, steps=K, row_stride=384) for m in modes}
        lims = {m: EpisodeLimits(n, dev, *LIMITS, steps=K, **({"progression": True} if m == "g" else {})) for m in modes if m != "p"}
        prog = balatro_gym_amd.ProgressionRewards(n, dev) if "g" in modes else None

        def run(m, c):
            a = acts[c:c + K]
            if m == "g":
                envs[m].step_many(a, obs_buffers=bufs[m], limits=lims[m], progression=prog)
            elif m == "s":
                envs[m].step_many(a, obs_buffers=bufs[m], limits=lims[m])
            else:
                envs[m].step_many(a, obs_buffers=bufs[m])
        for m in modes:   # warm-up, not timed: code object load, first touch of the buffers.  It is the recording's first call; the timed ones go on from there
            run(m, 0)
        torch.cuda.synchronize(dev)
        rates = {m: [] for m in modes}
        ended = {m: 0.0 for m in modes}
        for c in range(K, ks - K + 1, K):
            first = (c // K) % len(modes)
            for m in modes[first:] + modes[:first]:
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                run(m, c)
                torch.cuda.synchronize(dev)
                rates[m].append(n * K / (time.perf_counter() - t0))
                ended[m] += float((bufs[m].terminated != 0).float().mean().item())
        for m in modes:
            envs[m].check()
            r = np.array(rates[m]) / 1e9
            q = {"min": r.min(), "p10": np.percentile(r, 10), "median": np.median(r), "p90": np.percentile(r, 90), "calls": len(r), "ended_share": ended[m] / len(r)}
            if m == "g":
                q["stuck_share_last_call"] = float(((bufs[m].end_flags & nat.END_STUCK) != 0).float().mean().item())
            out["rates"][f"{m}@{K}"] = {k: float(v) for k, v in q.items()}
            envs[m].close()
        del envs, bufs, lims, prog
    print("RESULT " + json.dumps(out))
    return 0


def kernel_metadata(lib, pattern="bg_engine3_"):
    """{kernel name: {vgpr, agpr, sgpr, scratch, lds, sgpr_spill, vgpr_spill}} of the gfx950 code object inside a built library (llvm-objcopy,
    clang-offload-bundler and llvm-readelf of the ROCm installation; as tools/step_many_safe.py, with the AGPRs)."""
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fatbin"), os.path.join(d, "co")
        subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fb])
        subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={fb}", f"--output={co}"])
        notes = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co], text=True)
    out = {}
    for blk in re.split(r"\n\s*- (?=\.agpr_count:)", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if pattern in name:
            g = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))   # noqa: E731
            out[name] = {"vgpr": g("vgpr_count"), "agpr": g("agpr_count"), "sgpr": g("sgpr_count"), "scratch": g("private_segment_fixed_size"),
                         "lds": g("group_segment_fixed_size"), "sgpr_spill": g("sgpr_spill_count"), "vgpr_spill": g("vgpr_spill_count")}
    return out


def kernel_label(name):
    """'413 cards SAFE' and the like from a mangled engine-3 kernel name."""
    m = re.search(r"bg_engine3_progress_kernelILb(\d)ELi(\d)ELi(\d)ELi(\d)EE", name)
    if m:
        c, now, ks, nsv = map(int, m.groups())
        return f"{now}{ks}{nsv} {'cards ' if c else ''}PROG".strip()
    v = [int(x) for x in re.findall(r"L[bi](\d+)E", re.search(r"bg_engine3_kernelI((?:L[bi]\d+E)+)E", name).group(1))]
    h, c, now, ks, nsv, act, safe = v + [0] * (7 - len(v))
    return f"{now}{ks}{nsv} {'hash ' if h else ''}{'cards ' if c else ''}{'SAFE' if safe else 'ACT' if act else 'policy'}".strip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=None)
    ap.add_argument("--modes", default="p,s,g")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=800)
    ap.add_argument("--ks", type=int, nargs="+", default=[100, 20])
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_many_progress.txt"))
    ap.add_argument("--metadata-only", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    lines = []
    say = lambda s="": (lines.append(s), print(s, flush=True))   # noqa: E731
    results = {"this": [], "parent_p": [], "this_p": [], "parent_s": [], "this_s": []}
    if not args.metadata_only:
        order = (["parent_p", "this_p", "parent_s", "this_s"] * args.repeats if args.parent_tree else []) + ["this"] * args.repeats
        for who in order:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--envs", str(args.envs), "--steps", str(args.steps), "--ks", *map(str, args.ks)]
            cmd += ["--modes", args.modes if who == "this" else who[-1]] + (["--tree", args.parent_tree] if who.startswith("parent") else [])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            res = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not res:
                print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
                print(f"step_many_progress.py: a worker of {who} failed ({p.returncode}): nothing more is started", file=sys.stderr)
                return 1
            results[who].append(json.loads(res[-1][7:]))
            print(f"step_many_progress.py: worker {sum(len(v) for v in results.values())} of {len(order)} ({who}) done", file=sys.stderr, flush=True)
        r0 = results["this"][0]
        say(f"tools/step_many_progress.py: {r0['envs']} envs, {r0['steps']} recorded steps of the uniform policy, limits {LIMITS[0]} / {LIMITS[1]}, GPU {r0['gpu']}")
        say(f"this build {r0['signature']}" + (f", parent build {results['parent_p'][0]['signature']}" if results["parent_p"] else "") +
            f"; {args.repeats} worker processes per build and mode, alternating; host clock around call + synchronize; env-steps/s [G]")
        med = lambda who, key: [w["rates"][key]["median"] for w in results[who] if key in w["rates"]]   # noqa: E731
        for K in args.ks:
            say(f"\nK = {K} steps per call ({int(r0['rates'][f'p@{K}']['calls'])} timed calls per mode and worker)")
            for m in ("p", "s"):
                for who in (f"parent_{m}", f"this_{m}"):
                    ms = med(who, f"{m}@{K}")
                    if ms:
                        say(f"  {who:9s} alone  {MODES[m]:50s} medians of the workers {' / '.join(f'{x:.3f}' for x in ms)}  -> median {np.median(ms):.3f}")
                if results[f"parent_{m}"]:
                    pp, tp = med(f"parent_{m}", f"{m}@{K}"), med(f"this_{m}", f"{m}@{K}")
                    lo, hi = min(pp), max(pp)
                    say(f"    {MODES[m].split(',')[0]} unchanged?  parent's workers span {lo:.3f} .. {hi:.3f} ({100 * (hi - lo) / np.median(pp):.1f} % of their median); this build's "
                        f"median {np.median(tp):.3f} is {100 * (np.median(tp) / np.median(pp) - 1):+.1f} % of the parent's: "
                        f"{'inside' if lo <= np.median(tp) <= hi else 'above' if np.median(tp) > hi else 'BELOW'} that span")
            for m in ("p", "s", "g"):
                ms = med("this", f"{m}@{K}")
                if ms:
                    w0 = results["this"][0]["rates"][f"{m}@{K}"]
                    extra = "".join(f", {k.replace('_', ' ')} {w0[k]:.4f}" for k in ("ended_share", "stuck_share_last_call") if k in w0)
                    say(f"  this, all modes  {m}  {MODES[m]:50s} medians of the workers {' / '.join(f'{x:.3f}' for x in ms)}  -> median {np.median(ms):.3f}"
                        f"  (worker 1: min {w0['min']:.3f} p10 {w0['p10']:.3f} p90 {w0['p90']:.3f}{extra})")
            g, s, p = med("this", f"g@{K}"), med("this", f"s@{K}"), med("this", f"p@{K}")
            if g and s:
                say(f"  progression + limits / limits: {np.median(g) / np.median(s):.3f}" + (f"; / unwrapped: {np.median(g) / np.median(p):.3f}" if p else ""))
    # code-object metadata: the before / after table
    libs = {"this": os.path.join(ROOT, "balatro_gym_amd", "libbalatro_mi355x.so")}
    if args.parent_tree:
        libs["parent"] = os.path.join(args.parent_tree, "balatro_gym_amd", "libbalatro_mi355x.so")
    meta = {who: kernel_metadata(lib, "bg_engine3_") for who, lib in libs.items()}
    say("\ncode-object metadata of the engine-3 kernels: VGPRs / AGPRs / SGPRs / scratch bytes per lane / LDS bytes / SGPR spills / VGPR spills")
    say("(bg_engine3_kernel<HASH, CARDS, NOW, KS, NSV, ACT, SAFE> by shape and mode; PROG = bg_engine3_progress_kernel<CARDS, NOW, KS, NSV>)")
    fmt = lambda m: f"{m['vgpr']} / {m['agpr']} / {m['sgpr']} / {m['scratch']} / {m['lds']} / {m['sgpr_spill']} / {m['vgpr_spill']}"   # noqa: E731
    same, clean = True, True
    for name in sorted(meta["this"], key=lambda k: ("progress" in k, kernel_label(k))):
        new = "progress_kernel" in name
        line = f"  {kernel_label(name):24s} {fmt(meta['this'][name])}"
        if new:
            ok = meta["this"][name]["scratch"] == 0 and meta["this"][name]["vgpr_spill"] == 0
            clean = clean and ok
            line += "   new: no scratch, no VGPR spills" if ok else "   new: SCRATCH OR VGPR SPILLS"
        elif "parent" in meta:
            pm = meta["parent"].get(name)
            same = same and pm == meta["this"][name]
            line += "   parent: equal" if pm == meta["this"][name] else f"   parent: {fmt(pm) if pm else 'no such kernel'}  DIFFERENT"
        say(line)
    if "parent" in meta:
        say(f"  every pre-existing instantiation equal to the parent's: {'yes' if same and set(meta['parent']) <= set(meta['this']) else 'NO'}")
    say(f"  the new instantiations have no scratch and no VGPR spills: {'yes' if clean else 'NO'}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
