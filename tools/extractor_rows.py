#!/usr/bin/env python3
"""What does the first layer behind BalatroFeaturesExtractor's input cost straight from the stored records (extractor_rows / extractor_rows_grad:
bg_extractor_rows, bg_extractor_rows_grad) beside the composite a user writes without it on the same commit?  Writes profiles/extractor_rows.txt (--out).

One process.  65 536 envs (BASELINE configs[2], as bench.py sets them up) roll out 100 steps into a RowBuffers at stride 384: a 2.5 GB store of
6 553 600 records.  Minibatches of 65 536 and 4 096 rows out of a shuffled permutation, H = 128, 448 (the reference's three first layers as one
block-structured weight), 512, 1024.  Every timed call takes the NEXT minibatch of the permutation, as an epoch does, so the records come from HBM.  The
ways alternate repeat by repeat in the same process:
  forward   ours       extractor_rows(rows, w[H, 447] bf16 at pitch 448, b, index=, activation="relu", dtype=bf16)                   one launch
            composite  encode_rows(rows, "extractor", bf16, index=) then relu(torch.nn.functional.linear(x, w, b_bf16))              [m, 447] goes through HBM
  backward  ours       extractor_rows_grad(rows, dout bf16, out=, index=, activation="relu", dweight=[H, 447] f32)                   two launches
            composite  (dout * (out > 0)).T @ x with x the [m, 447] bf16 matrix ALREADY in memory (kept from the forward: its cheapest form)
"kernel" is the library's own kernel_ms_out (ours; for the composite the encode kernel alone), "call" device events around the whole Python call
(median of >= 20 repeats after warm-up, p10 / p90 for ours).  Before timing the results are compared: forward within bf16 rounding of the composite's,
gradient within 1e-3 of the largest element.  Every ratio is reported as measured, those below 1 included.  --resources FILE appends the compiler's
resource lines for the new kernels (the remarks file `tools/isa_diff.py --save` keeps)."""
import argparse
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def resource_lines(path):
    """The per-kernel remarks of -Rpass-analysis=kernel-resource-usage for the bg_extractor kernels, one line per kernel."""
    out, cur = [], None
    for line in open(path):
        m = re.search(r"remark: (?:Function Name: (\S+)|\s+([A-Za-z ]+(?:\[[^\]]*\])?): (\d+))", line)
        if not m:
            continue
        if m.group(1):
            cur = [m.group(1)] if "bg_extractor" in m.group(1) else None
            if cur:
                out.append(cur)
        elif cur is not None:
            cur.append(f"{m.group(2).strip()} {m.group(3)}")
    return ["  " + c[0] + ": " + ", ".join(c[1:]) for c in out]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batches", type=int, nargs="+", default=[65536, 4096])
    ap.add_argument("--widths", type=int, nargs="+", default=[128, 448, 512, 1024])
    ap.add_argument("--repeats", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extractor_rows.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("extractor_rows.py: no GPU is visible", file=sys.stderr)
        return 2
    import bench
    from balatro_gym_amd import BalatroVecEnv, encode_rows, extractor_rows, extractor_rows_grad, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    dev = torch.device("cuda:0")
    n, T = args.envs, args.steps
    env = BalatroVecEnv(n, [1000 + g for g in range(n)], device=0, scorer_jokers=True, autoreset=True, max_ante=bench.MAX_ANTE, fused_steps=min(T, 100))
    env.inject(jokers=[bench.jokers_for(g) for g in range(n)], apply_now=True)
    rb = RowBuffers(n, dev, steps=T, row_stride=nat.ROW_STRIDE_LINES)
    done = 0
    while done < T:
        k = min(env.max_fused_steps, T - done)
        part = rb if k == T else RowBuffers(n, dev, steps=k, row_stride=nat.ROW_STRIDE_LINES)
        env.rollout(k, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED + done, obs_buffers=part)
        if part is not rb:
            rb.rows[done:done + k].copy_(part.rows)
        done += k
    env.close()
    store = n * T
    say(f"build signature {nat.device_code_signature()}  library {os.path.basename(nat.lib_path())}  GPU {torch.cuda.get_device_name(0)}")
    say(f"store: {n} envs x {T} steps = {store} records at stride {rb.row_stride}, {store * rb.row_stride / 1e6:.0f} MB; shuffled index; {args.repeats} repeats after "
        f"{args.warmup} warm-up, the ways alternating; device events; ms")
    perm = next(rb.minibatches(store, generator=torch.Generator().manual_seed(20240607)))
    turn = [0]

    def minibatch(m):
        turn[0] += 1
        lo = (turn[0] % (store // m)) * m
        return perm[lo:lo + m].contiguous()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), r

    def run(ways, m):
        """ways: name -> fn(index, timing) returning the library's kernel ms when timing (which synchronises, so the whole call is timed without it)."""
        call = {w: [] for w in ways}
        kern = {w: [] for w in ways}
        for rep in range(args.warmup + args.repeats):
            for w, fn in ways.items():
                index = minibatch(m)
                c, _ = timed(lambda: fn(index, False))
                index = minibatch(m)
                k = fn(index, True)
                if rep >= args.warmup:
                    call[w].append(c)
                    kern[w].append(k)
        return call, kern

    say(f"{'pass':>8} {'m':>6} {'H':>5} | {'ours kernel':>11} {'call p10':>9} {'median':>8} {'p90':>8} | {'composite encode kernel':>23} {'call median':>11} | "
        f"{'composite / ours (call)':>23}")
    slower = []
    for m in args.batches:
        x = torch.empty((m, nat.EXT_K), dtype=torch.bfloat16, device=dev)
        for H in args.widths:
            g = torch.Generator(device=dev).manual_seed(H)
            w = torch.zeros((H, nat.EXT_K + 1), dtype=torch.bfloat16, device=dev)[:, :nat.EXT_K]   # pitch 448, as RowExtractor stages it
            w.copy_(torch.randn((H, nat.EXT_K), device=dev, generator=g) * 0.05)
            wc = w.contiguous()
            b = torch.randn(H, device=dev, generator=g)
            b16 = b.to(torch.bfloat16)
            dout = torch.randn((m, H), device=dev, generator=g).to(torch.bfloat16)
            out = torch.empty((m, H), dtype=torch.bfloat16, device=dev)
            dweight = torch.zeros((H, nat.EXT_K), dtype=torch.float32, device=dev)
            index = minibatch(m)
            ours = extractor_rows(rb.rows, w, b, index=index, activation="relu", dtype=torch.float32)
            encode_rows(rb.rows, "extractor", torch.bfloat16, x, index=index)
            comp = torch.relu(torch.nn.functional.linear(x.float(), wc.float(), b))
            scale = float(comp.abs().max())
            if not float((ours - comp).abs().max()) <= 1e-3 * scale:
                print(f"extractor_rows.py: m {m} H {H}: forward differs from the composite by {float((ours - comp).abs().max())} of {scale}", file=sys.stderr)
                return 1
            gw, _ = extractor_rows_grad(rb.rows, dout, out=ours, index=index, activation="relu", dweight=dweight)
            ref = (dout.float() * (ours > 0)).T @ x.float()
            gscale = float(ref.abs().max())
            if not float((gw - ref).abs().max()) <= 1e-3 * gscale:
                print(f"extractor_rows.py: m {m} H {H}: gradient differs from the composite by {float((gw - ref).abs().max())} of {gscale}", file=sys.stderr)
                return 1
            del ours, comp, ref
            extractor_rows(rb.rows, w, b, index=index, activation="relu", out=out)

            def ours_fwd(index, t):
                r = extractor_rows(rb.rows, w, b, index=index, activation="relu", out=out, timing=t)
                return r[1] if t else 0.0

            def ours_bwd(index, t):
                r = extractor_rows_grad(rb.rows, dout, out=out, index=index, activation="relu", dweight=dweight, timing=t)
                return r[2] if t else 0.0

            def composite_fwd(index, t):
                r = encode_rows(rb.rows, "extractor", torch.bfloat16, x, index=index, timing=t)
                torch.relu(torch.nn.functional.linear(x, wc, b16))
                return r[1] if t else 0.0

            def composite_bwd(index, t):
                (dout * (out > 0)).T @ x
                return 0.0
            for name, ways in (("forward", {"ours": ours_fwd, "composite": composite_fwd}), ("backward", {"ours": ours_bwd, "composite": composite_bwd})):
                call, kern = run(ways, m)
                o, c = call["ours"], call["composite"]
                ratio = np.median(c) / np.median(o)
                if ratio < 1.0:
                    slower.append(f"{name} m {m} H {H}: ours {np.median(o):.4f} ms, composite {np.median(c):.4f} ms")
                say(f"{name:>8} {m:>6} {H:>5} | {np.median(kern['ours']):>11.4f} {np.percentile(o, 10):>9.4f} {np.median(o):>8.4f} {np.percentile(o, 90):>8.4f} | "
                    f"{np.median(kern['composite']):>23.4f} {np.median(c):>11.4f} | {ratio:>22.2f}x")
    say("ours faster than the composite (whole call) in every shape: " + ("yes" if not slower else "NO"))
    for s in slower:
        say("  " + s)
    if args.resources:
        say("the compiler's resource lines for the new kernels (-Rpass-analysis=kernel-resource-usage):")
        for s in resource_lines(args.resources):
            say(s)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
