#!/usr/bin/env python3
"""What does one minibatch's network input cost straight from the stored records (encode_rows(index=, norm=): bg_encode_rows_ex) beside its ceiling
and beside what a user writes without it?

One process.  65 536 envs (BASELINE configs[2], as bench.py sets them up) roll out 100 steps into a RowBuffers at stride 384: a 2.5 GB store of
6 553 600 records.  Minibatches of 4 096 and 65 536 rows; three cases -- "produced" float32, "produced" bfloat16, "fixed" bfloat16 with frozen VecNormalize
statistics (a RowNormalizer after a few real updates) --; three index patterns -- a slice of a random permutation (RowBuffers.minibatches), the same
slice sorted, a contiguous range passed through an index.  Every timed call takes the NEXT minibatch of the permutation (the next range for the contiguous ways), as
an epoch over the store does: 2.5 GB of other records pass before one is read again, so the records come from HBM and not from the 256 MiB Infinity
Cache.  Four ways, alternating repeat by repeat in the same process:
  gathered   encode_rows(rows, layout, dtype, out, index=index[, norm=])                                        one launch
  ceiling    the contiguous kernel on the same m: encode_rows / normalize_obs(update=False) of m consecutive records (bg_encode_rows / frozen bg_norm_obs_rows)
  torch u8   rows2d[index.long()] -- torch's advanced indexing of the 384-byte uint8 rows into a temporary --, then the contiguous call on the temporary
  torch i64  the same with the records viewed as int64 words before indexing: the fast way to do it in torch
"kernel" is the library's own kernel_ms_out, "call" device events around the whole Python call (>= 20 repeats after warm-up; p10 / median / p90 of the
call, median of the kernel).  Before timing, the gathered result is compared bit for bit with the torch composite's."""
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
    ap.add_argument("--repeats", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("minibatch_rows.py: no GPU is visible", file=sys.stderr)
        return 2
    import bench
    from balatro_gym_amd import BalatroVecEnv, RowNormalizer, encode_rows, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers
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
    st = env.stats()
    env.close()
    store = n * T
    rows2d = rb.rows.view(store, rb.row_stride)
    words = rows2d.view(torch.int64)
    stats = RowNormalizer(n, dev)
    stats.normalize_obs(rb.rows[:4])
    stats.training = False
    copy_gbps, fill_gbps = bench.measured_copy_gbps(dev)
    print(f"build signature {nat.device_code_signature()}  library {os.path.basename(nat.lib_path())}  GPU {torch.cuda.get_device_name(0)}")
    print(f"store: {n} envs x {T} steps = {store} records at stride {rb.row_stride}, {store * rb.row_stride / 1e6:.0f} MB ({st['plays']} plays, {st['episodes']} episodes); "
          f"bg_bench_copy {copy_gbps:.0f} GB/s (read + written), bg_bench_fill {fill_gbps:.0f} GB/s; {args.repeats} repeats after {args.warmup} warm-up, device events, "
          f"the four ways alternating; ms")

    def frozen(m):
        """A frozen normaliser of m envs with the statistics of `stats`: what normalize_obs of an [m, stride] temporary needs."""
        nm = RowNormalizer(m, dev, training=False)
        nm.obs_mean.copy_(stats.obs_mean), nm.obs_var.copy_(stats.obs_var), nm.obs_count.copy_(stats.obs_count)
        return nm

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), r[1]

    perm = next(rb.minibatches(store, generator=torch.Generator().manual_seed(20240607)))
    cases = (("produced", torch.float32, False), ("produced", torch.bfloat16, False), ("fixed", torch.bfloat16, True))
    print(f"{'m':>6} {'layout':>9} {'dtype':>8} {'norm':>4} {'index':>10} | {'gathered kernel':>15} {'call p10':>9} {'median':>8} {'p90':>8} | {'ceiling kernel':>14} {'call':>8} | "
          f"{'torch u8 call':>13} {'torch i64 call':>14} | {'gathered / ceiling (kernel)':>27} {'better composite / gathered (call)':>34}")
    slower = []
    turn = 0   # every timed call takes the NEXT minibatch of the permutation, as an epoch does: its records come from HBM, not from a cache an earlier repeat warmed
    for m in args.batches:
        m = min(m, store)
        nslices = store // m
        nm_m = frozen(m)

        def minibatch(name, k):
            """(index, first record of the contiguous range) of minibatch k under pattern `name`."""
            lo = (k % nslices) * m
            if name == "range":
                return torch.arange(lo, lo + m, dtype=torch.int32, device=dev), lo
            index = perm[lo:lo + m]
            return (index.sort().values if name == "sorted" else index).contiguous(), lo
        for layout, dtype, normed in cases:
            D = nat.ENC_COLS[nat.ENC_LAYOUTS[layout]]
            out = torch.empty((m, D), dtype=dtype, device=dev)
            out_c = torch.empty((m, D), dtype=dtype, device=dev)

            def contiguous(r2d):
                if normed:
                    return nm_m.normalize_obs(r2d, layout, dtype, out_c, timing=True)
                return encode_rows(r2d, layout, dtype, out_c, timing=True)
            ways = {"gathered": lambda index, lo: encode_rows(rb.rows, layout, dtype, out, index=index, norm=stats if normed else None, timing=True),
                    "ceiling": lambda index, lo: contiguous(rows2d[lo:lo + m]),
                    "torch u8": lambda index, lo: contiguous(rows2d[index.long()]),
                    "torch i64": lambda index, lo: contiguous(words[index.long()].view(torch.uint8))}
            for name in ("shuffled", "sorted", "range"):
                it = torch.int32 if dtype == torch.float32 else torch.int16
                index, lo = minibatch(name, 0)
                got = ways["gathered"](index, lo)[0].view(it).clone()
                for w in ("torch u8", "torch i64"):
                    if not torch.equal(got, ways[w](index, lo)[0].view(it)):
                        print(f"minibatch_rows.py: {layout} {dtype} {name} m {m}: the gathered result differs from the {w} composite", file=sys.stderr)
                        return 1
                del got
                call = {w: [] for w in ways}
                kern = {w: [] for w in ways}
                for rep in range(args.warmup + args.repeats):
                    for w, fn in ways.items():
                        turn += 1
                        index, lo = minibatch(name, turn)
                        torch.cuda.synchronize()
                        c, k = timed(lambda: fn(index, lo))
                        if rep >= args.warmup:
                            call[w].append(c)
                            kern[w].append(k)
                g10, g50, g90 = np.percentile(call["gathered"], 10), np.median(call["gathered"]), np.percentile(call["gathered"], 90)
                gk, ck = np.median(kern["gathered"]), np.median(kern["ceiling"])
                u8, i64 = np.median(call["torch u8"]), np.median(call["torch i64"])
                best = min(u8, i64)
                if g50 >= best:
                    slower.append(f"m {m} {layout} {str(dtype).replace('torch.', '')} {name}: gathered {g50:.4f} ms, better composite {best:.4f} ms")
                print(f"{m:>6} {layout:>9} {str(dtype).replace('torch.', ''):>8} {'yes' if normed else 'no':>4} {name:>10} | {gk:>15.4f} {g10:>9.4f} {g50:>8.4f} {g90:>8.4f} | "
                      f"{ck:>14.4f} {np.median(call['ceiling']):>8.4f} | {u8:>13.4f} {i64:>14.4f} | {gk / ck:>26.2f}x {best / g50:>33.2f}x")
            del out, out_c
    print("gathered call faster than the better torch composite in every shape: " + ("yes" if not slower else "NO"))
    for s in slower:
        print("  " + s)
    return 0


if __name__ == "__main__":
    sys.exit(main())
