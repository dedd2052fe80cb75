#!/usr/bin/env python3
"""What does bg_encode_rows (vec_env.encode_rows) cost beside the torch composite a user writes without it?

One process.  65 536 envs (BASELINE configs[2], as bench.py sets them up) roll out 100 steps into a RowBuffers at stride 384; the records of 1, 20 and
100 steps (25 MB -- inside the 256 MiB Infinity Cache: the per-step latency figure --, 503 MB, 2.5 GB: the HBM figure) are encoded into each layout, in
float32 and bfloat16, two ways that alternate repeat by repeat in the same process:
  new       encode_rows(rows, layout, dtype, out=preallocated)                                    one launch
  baseline  what exists without it: per key `rb.tensors[k].to(dtype).reshape(m, -1)` + `torch.cat` (FIXED: plus a block of zeros); for EXTRACTOR the
            preprocessing of BalatroFeaturesExtractor.forward (train_balatro_agent.py:84-119) vectorised without its Python loop
Both are timed by device events around the call (>= 20 repeats after warm-up).  Bytes come from the shapes: m * 384 read + m * D * element size
written; "share of a measured copy" is that rate over what bg_bench_copy reaches in the same run (bench.py `roofline.peak_measured`; it is NOT a share of
the nominal 8 TB/s).  The float32 results of both ways are compared: PRODUCED / FIXED must be equal; EXTRACTOR may differ in the last bit where torch's
GPU kernel multiplies by a reciprocal (counted and printed)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, nargs="+", default=[1, 20, 100])
    ap.add_argument("--repeats", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("encode_rows.py: no GPU is visible", file=sys.stderr)
        return 2
    import bench
    from balatro_gym_amd import BalatroVecEnv, encode_rows, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers
    dev = torch.device("cuda:0")
    n, T = args.envs, max(args.steps)
    env = BalatroVecEnv(n, [1000 + g for g in range(n)], device=0, scorer_jokers=True, autoreset=True, max_ante=bench.MAX_ANTE, fused_steps=T)
    env.inject(jokers=[bench.jokers_for(g) for g in range(n)], apply_now=True)
    rb = RowBuffers(n, dev, steps=T, row_stride=nat.ROW_STRIDE_LINES)
    env.rollout(T, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED, obs_buffers=rb)
    st = env.stats()
    env.close()
    copy_gbps, fill_gbps = bench.measured_copy_gbps(dev)
    print(f"build signature {nat.device_code_signature()}  library {os.path.basename(nat.lib_path())}  GPU {torch.cuda.get_device_name(0)}")
    print(f"{n} envs x {T} steps of records at stride {rb.row_stride} ({st['plays']} plays, {st['episodes']} episodes); bg_bench_copy {copy_gbps:.0f} GB/s "
          f"(read + written), bg_bench_fill {fill_gbps:.0f} GB/s; {args.repeats} repeats after {args.warmup} warm-up, device events, new / baseline alternating")
    ar52 = torch.arange(52, dtype=torch.int8, device=dev)

    def baseline(steps, layout, dtype):
        m = steps * n
        t = {k: v[:steps] for k, v in rb.tensors.items()}
        if layout in ("produced", "fixed"):
            parts = [t[k].to(dtype).reshape(m, -1) for k in nat.OBS_KEYS]
            if layout == "fixed":
                parts.append(torch.zeros((m, nat.ENC_COLS[nat.ENC_FIXED] - nat.ENC_COLS[nat.ENC_PRODUCED]), dtype=dtype, device=dev))
            return torch.cat(parts, dim=1)
        one_hot = (t["hand"].reshape(m, 8, 1) == ar52).to(dtype).reshape(m, 416)   # hand >= 0 is implied: a card is 0..51
        f = lambda k, c: t[k].to(dtype).reshape(m, -1) / c
        return torch.cat([one_hot, t["joker_ids"].to(dtype).reshape(m, 10), f("chips_scored", 1e6), f("chips_needed", 1e5),
                          t["progress_ratio"].to(dtype).reshape(m, 1), f("money", 100), f("ante", 10), f("round", 3), f("hands_left", 10),
                          f("discards_left", 5), f("hand_levels", 10), f("phase", 3)], dim=1)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        del r
        return a.elapsed_time(b)

    def pct(x):
        return np.percentile(x, 10), np.median(x), np.percentile(x, 90)

    print(f"{'steps':>5} {'layout':>9} {'dtype':>8} {'MB read':>8} {'MB written':>10} | {'new p10':>8} {'median':>8} {'p90':>8} ms | {'base p10':>8} {'median':>8} {'p90':>8} ms | "
          f"{'speed-up':>8} {'GB/s':>6} {'share of a measured copy':>24} {'new p90 < base p10':>18}")
    worst_ok = True
    for steps in args.steps:
        rows = rb.rows[:steps]
        m = steps * n
        for layout in ("produced", "fixed", "extractor"):
            D = nat.ENC_COLS[nat.ENC_LAYOUTS[layout]]
            for dtype in (torch.float32, torch.bfloat16):
                out = torch.empty((steps, n, D), dtype=dtype, device=dev)
                new = lambda: encode_rows(rows, layout, dtype, out=out)
                base = lambda: baseline(steps, layout, dtype)
                if dtype == torch.float32:
                    g, w = new().reshape(m, D).view(torch.int32), base().view(torch.int32)
                    diff = int((g != w).sum().item())
                    if layout != "extractor" and diff:
                        print(f"encode_rows.py: {layout} differs from the torch composite in {diff} elements", file=sys.stderr)
                        return 1
                    if layout == "extractor":
                        print(f"      (extractor float32, {steps} steps: {diff} of {m * D} elements differ from the torch composite in the last bits -- its GPU division by a scalar)")
                    del g, w
                for _ in range(args.warmup):
                    timed(new), timed(base)
                tn, tb = [], []
                for _ in range(args.repeats):
                    tn.append(timed(new))
                    tb.append(timed(base))
                es = 4 if dtype == torch.float32 else 2
                rd, wr = m * rb.row_stride, m * D * es
                n10, n50, n90 = pct(tn)
                b10, b50, b90 = pct(tb)
                gbps = (rd + wr) / (n50 * 1e-3) / 1e9
                ok = n90 < b10
                worst_ok = worst_ok and ok
                print(f"{steps:>5} {layout:>9} {str(dtype).replace('torch.', ''):>8} {rd / 1e6:>8.1f} {wr / 1e6:>10.1f} | {n10:>8.4f} {n50:>8.4f} {n90:>8.4f}    | "
                      f"{b10:>8.3f} {b50:>8.3f} {b90:>8.3f}    | {b50 / n50:>7.1f}x {gbps:>6.0f} {gbps / copy_gbps:>24.2f} {'yes' if ok else 'NO':>18}")
                del out
                torch.cuda.empty_cache()
    print("new p90 below baseline p10 in every shape: " + ("yes" if worst_ok else "NO"))
    return 0 if worst_ok else 1


if __name__ == "__main__":
    sys.exit(main())
