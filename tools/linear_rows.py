#!/usr/bin/env python3
"""What does the network's first layer cost straight from the stored records (linear_rows / linear_rows_grad: bg_linear_rows, bg_linear_rows_grad) beside
the composite a user writes without it on the same commit?  Writes profiles/linear_rows.txt (--out).

One process.  65 536 envs (BASELINE configs[2], as bench.py sets them up) roll out 100 steps into a RowBuffers at stride 384: a 2.5 GB store of
6 553 600 records.  Minibatches of 4 096 and 65 536 rows out of a shuffled permutation, H = 128, 512, 1024, with and without frozen VecNormalize
statistics.  Every timed call takes the NEXT minibatch of the permutation, as an epoch does, so the records come from HBM.  The ways alternate repeat by
repeat in the same process:
  forward   ours       linear_rows(rows, w[H, 628] bf16, b, index=, norm=, dtype=bf16)                                   one launch
            composite  encode_rows(rows, "fixed", bf16, index=, norm=) then torch.nn.functional.linear(x, w, b_bf16)      the [m, 628] matrix goes through HBM
  backward  ours       linear_rows_grad(rows, dout bf16, index=, norm=, dweight=[H, 628] f32)                             two launches
            composite  dout.T @ x with x the [m, 628] bf16 matrix ALREADY in memory (kept from the forward: its cheapest form), bf16 result
"kernel" is the library's own kernel_ms_out (ours; for the composite the encode kernel alone), "call" device events around the whole Python call
(median of >= 20 repeats after warm-up, p10 / p90 for ours).  Before timing the results are compared: forward within bf16 rounding of the composite's,
gradient within the float32 bound of tests/linear_ref.py's kind.  --encode-only prints bg_encode_rows_ex's own medians ("fixed" bf16, with and without
statistics) and nothing else: run on the parent commit's library and on this one (BALATRO_MI355X_LIB) to see that the kernels beside the new header
did not move."""
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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batches", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--widths", type=int, nargs="+", default=[128, 512, 1024])
    ap.add_argument("--repeats", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--encode-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_rows.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("linear_rows.py: no GPU is visible", file=sys.stderr)
        return 2
    import bench
    from balatro_gym_amd import BalatroVecEnv, RowNormalizer, encode_rows, _native as nat
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
    stats = RowNormalizer(n, dev)
    stats.normalize_obs(rb.rows[:4])
    stats.training = False
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

    if args.encode_only:
        say(f"{'m':>6} {'norm':>4} | {'bg_encode_rows_ex kernel p10':>28} {'median':>8} {'p90':>8} | {'call median':>11}")
        for m in args.batches:
            out = torch.empty((m, 628), dtype=torch.bfloat16, device=dev)
            for normed in (False, True):
                call, kern = run({"encode": lambda index, t: encode_rows(rb.rows, "fixed", torch.bfloat16, out, index=index, norm=stats if normed else None, timing=True)[1] if t else
                                  encode_rows(rb.rows, "fixed", torch.bfloat16, out, index=index, norm=stats if normed else None)}, m)
                k = kern["encode"]
                say(f"{m:>6} {'yes' if normed else 'no':>4} | {np.percentile(k, 10):>28.4f} {np.median(k):>8.4f} {np.percentile(k, 90):>8.4f} | {np.median(call['encode']):>11.4f}")
        return finish(args, lines)

    from balatro_gym_amd import linear_rows, linear_rows_grad
    say(f"{'pass':>8} {'m':>6} {'H':>5} {'norm':>4} | {'ours kernel':>11} {'call p10':>9} {'median':>8} {'p90':>8} | {'composite encode kernel':>23} {'call median':>11} | "
        f"{'composite / ours (call)':>23}")
    slower = []
    for m in args.batches:
        x = torch.empty((m, 628), dtype=torch.bfloat16, device=dev)
        for H in args.widths:
            g = torch.Generator(device=dev).manual_seed(H)
            w = (torch.randn((H, 628), device=dev, generator=g) * 0.05).to(torch.bfloat16)
            b = torch.randn(H, device=dev, generator=g)
            b16 = b.to(torch.bfloat16)
            dout = torch.randn((m, H), device=dev, generator=g).to(torch.bfloat16)
            out = torch.empty((m, H), dtype=torch.bfloat16, device=dev)
            dweight = torch.zeros((H, 628), dtype=torch.float32, device=dev)
            ws = torch.empty(int(nat.load().bg_linear_rows_workspace_bytes(m, H)), dtype=torch.uint8, device=dev)
            for normed in (False, True):
                nm = stats if normed else None
                index = minibatch(m)
                ours = linear_rows(rb.rows, w, b, index=index, norm=nm, dtype=torch.float32)
                comp = torch.nn.functional.linear(encode_rows(rb.rows, "fixed", torch.float32, index=index, norm=nm).to(torch.bfloat16).float(), w.float(), b)
                scale = float(comp.abs().max())
                if not float((ours - comp).abs().max()) <= 1e-3 * scale:
                    print(f"linear_rows.py: m {m} H {H} norm {normed}: forward differs from the composite by {float((ours - comp).abs().max())} of {scale}", file=sys.stderr)
                    return 1
                encode_rows(rb.rows, "fixed", torch.bfloat16, x, index=index, norm=nm)
                gw, _ = linear_rows_grad(rb.rows, dout, index=index, norm=nm, dweight=dweight, workspace=ws)
                ref = dout.float().T @ x.float()
                gscale = float(ref.abs().max())
                if not float((gw - ref).abs().max()) <= 1e-3 * gscale:
                    print(f"linear_rows.py: m {m} H {H} norm {normed}: gradient differs from the composite by {float((gw - ref).abs().max())} of {gscale}", file=sys.stderr)
                    return 1
                del ours, comp, ref

                def ours_fwd(index, t):
                    r = linear_rows(rb.rows, w, b, index=index, norm=nm, out=out, timing=t)
                    return r[1] if t else 0.0

                def ours_bwd(index, t):
                    r = linear_rows_grad(rb.rows, dout, index=index, norm=nm, dweight=dweight, workspace=ws, timing=t)
                    return r[2] if t else 0.0

                def composite_fwd(index, t):
                    r = encode_rows(rb.rows, "fixed", torch.bfloat16, x, index=index, norm=nm, timing=t)
                    torch.nn.functional.linear(x, w, b16)
                    return r[1] if t else 0.0

                def composite_bwd(index, t):
                    dout.T @ x
                    return 0.0
                for name, ways in (("forward", {"ours": ours_fwd, "composite": composite_fwd}), ("backward", {"ours": ours_bwd, "composite": composite_bwd})):
                    call, kern = run(ways, m)
                    o, c = call["ours"], call["composite"]
                    ratio = np.median(c) / np.median(o)
                    if ratio < 1.0:
                        slower.append(f"{name} m {m} H {H} norm {'yes' if normed else 'no'}: ours {np.median(o):.4f} ms, composite {np.median(c):.4f} ms")
                    say(f"{name:>8} {m:>6} {H:>5} {'yes' if normed else 'no':>4} | {np.median(kern['ours']):>11.4f} {np.percentile(o, 10):>9.4f} {np.median(o):>8.4f} {np.percentile(o, 90):>8.4f} | "
                        f"{np.median(kern['composite']):>23.4f} {np.median(c):>11.4f} | {ratio:>22.2f}x")
    say("ours faster than the composite (whole call) in every shape: " + ("yes" if not slower else "NO"))
    for s in slower:
        say("  " + s)
    return finish(args, lines)


def finish(args, lines):
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
