#!/usr/bin/env python3
"""What do bg_norm_obs_rows / bg_norm_reward_rows (vec_env.RowNormalizer) cost beside bg_encode_rows and beside the torch composite a user writes without them?

One process.  65 536 envs (BASELINE configs[2], as bench.py sets them up) and 4 096 envs are run 400 steps, then roll out 100 steps into a RowBuffers at
stride 384.  Shapes (envs x steps): 65 536 x 100, 4 096 x 100, 65 536 x 1.  Per shape, layout "produced", float32 and bf16, update = 1 (training) and
update = 0 (frozen statistics), each way alternating repeat by repeat in the same process (p10 / median / p90 over the repeats after warm-up):
  kernel ms   the library's own kernel_ms_out (device events around the call's launches)
  wall ms     time.perf_counter around the Python call and a device synchronisation
Partners in the same run:
  encode      bg_encode_rows of the same layout and dtype: the update = 0 pass writes the same bytes, so that is its floor
  torch       the composite: encode_rows, then per step mean / var over the envs in float64, RunningMeanStd's merge, (x - mean) / sqrt(var + eps), clip,
              convert (update = 0: the normalisation alone); for the reward the per-step loop over rb.reward with a float64 carry
Before timing, the composite's float32 result is compared with the kernel's (largest absolute difference; torch's reduction order differs, so equality
is not expected; the bit-exact claims rest on tests/test_norm_rows.py)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GAMMA, EPS, CLIP = 0.99, 1e-8, 10.0


def records(n, T, dev):
    """[T, n] records at stride 384 of a real rollout after 400 steps of warm-up."""
    import bench
    from balatro_gym_amd import BalatroVecEnv, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers
    env = BalatroVecEnv(n, [1000 + g for g in range(n)], device=0, scorer_jokers=True, autoreset=True, max_ante=bench.MAX_ANTE, fused_steps=min(T, 100))
    env.inject(jokers=[bench.jokers_for(g) for g in range(n)], apply_now=True)
    env.rollout(400, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED, obs_buffers=RowBuffers(n, dev, steps=1))
    rb = RowBuffers(n, dev, steps=T, row_stride=nat.ROW_STRIDE_LINES)
    env.rollout(T, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED + 1, obs_buffers=rb)
    st = env.stats()
    env.close()
    return rb, st


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("norm_rows.py: no GPU is visible", file=sys.stderr)
        return 2
    import bench
    from balatro_gym_amd import RowNormalizer, encode_rows, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers
    dev = torch.device("cuda:0")
    copy_gbps, fill_gbps = bench.measured_copy_gbps(dev)
    print(f"build signature {nat.device_code_signature()}  library {os.path.basename(nat.lib_path())}  GPU {torch.cuda.get_device_name(0)}")
    print(f"bg_bench_copy {copy_gbps:.0f} GB/s (read + written), bg_bench_fill {fill_gbps:.0f} GB/s; gamma {GAMMA} epsilon {EPS} clip {CLIP}; layout produced, stride 384; "
          f"{args.repeats} repeats after {args.warmup} warm-up, the ways alternating; p10 median p90")

    def merge(mean, var, count, bm, bv, n):
        delta = bm - mean
        tot = count + n
        m2 = var * count + bv * n + delta.square() * count * n / tot
        return mean + delta * n / tot, m2 / tot, tot

    def torch_obs(rows, dtype, update, mean, var, count):
        K, n = rows.shape[:2]
        x = encode_rows(rows, "produced", torch.float32).double()
        if not update:
            return ((x - mean) / (var + EPS).sqrt()).clamp(-CLIP, CLIP).to(dtype)
        out = torch.empty((K, n, 153), dtype=dtype, device=rows.device)
        for t in range(K):
            mean, var, count = merge(mean, var, count, x[t].mean(0), x[t].var(0, unbiased=False), n)
            out[t] = ((x[t] - mean) / (var + EPS).sqrt()).clamp(-CLIP, CLIP).to(dtype)
        return out

    def torch_reward(rb, K, update, ret, mean, var, count):
        reward, term = rb.reward[:K], rb.terminated[:K]
        n = reward.shape[1]
        if not update:
            return (reward / (var + EPS).sqrt()).clamp(-CLIP, CLIP)
        out = torch.empty((K, n), dtype=torch.float64, device=reward.device)
        for t in range(K):
            ret = ret * GAMMA + reward[t]
            mean, var, count = merge(mean, var, count, ret.mean(), ret.var(unbiased=False), n)
            out[t] = (reward[t] / (var + EPS).sqrt()).clamp(-CLIP, CLIP)
            ret = torch.where(term[t] != 0, 0.0, ret)
        return out

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        del r
        return (time.perf_counter() - t0) * 1e3

    def pct(x):
        return f"{np.percentile(x, 10):9.4f} {np.median(x):9.4f} {np.percentile(x, 90):9.4f}"

    def run(ways):
        """ways: name -> (fn returning kernel ms or None, fn for the wall clock).  Alternating; returns name -> (kernel list, wall list)."""
        res = {k: ([], []) for k in ways}
        for i in range(args.warmup + args.repeats):
            for k, (kfn, wfn) in ways.items():
                ms = kfn() if kfn else None
                w = wall(wfn)
                if i >= args.warmup:
                    if ms is not None:
                        res[k][0].append(ms)
                    res[k][1].append(w)
        return res

    for n, K in ((65536, 100), (4096, 100), (65536, 1)):
        rb, st = records(n, K, dev)
        rows = rb.rows
        mb_in = K * n * 384 / 1e6
        print(f"\n{n} envs x {K} steps: records after 400 steps of warm-up ({st['plays']} plays, {st['episodes']} episodes in the window); {mb_in:.0f} MB of records")
        f64 = dict(dtype=torch.float64, device=dev)
        for dtype, name in ((torch.float32, "float32"), (torch.bfloat16, "bf16")):
            out = torch.empty((K, n, 153), dtype=dtype, device=dev)
            enc = torch.empty((K, n, 153), dtype=dtype, device=dev)
            mb_out = out.numel() * out.element_size() / 1e6
            # ---- the two ways agree to rounding
            nm = RowNormalizer(n, dev)
            nm.normalize_obs(rows, "produced", dtype, out=out)
            ref = torch_obs(rows, dtype, 1, torch.zeros(153, **f64), torch.ones(153, **f64), torch.tensor(1e-4, **f64))
            print(f"  ({name}, update 1: largest |kernel - torch composite| {float((out.float() - ref.float()).abs().max()):.3g} over {out.numel()} elements in [-{CLIP}, {CLIP}])")
            del ref
            trained = nm.state_dict()
            for update in (1, 0):
                nm = RowNormalizer(n, dev, training=bool(update))
                nm.load_state_dict(dict(trained, training=bool(update)))
                m0, v0, c0 = nm.obs_mean.clone(), nm.obs_var.clone(), nm.obs_count.clone()[0]
                ways = {"norm": (lambda: nm.normalize_obs(rows, "produced", dtype, out=out, timing=True)[1], lambda: nm.normalize_obs(rows, "produced", dtype, out=out)),
                        "encode": (lambda: encode_rows(rows, "produced", dtype, out=enc, timing=True)[1], lambda: encode_rows(rows, "produced", dtype, out=enc)),
                        "torch": (None, lambda: torch_obs(rows, dtype, update, m0, v0, c0))}
                res = run(ways)
                kn, ke = np.median(res["norm"][0]), np.median(res["encode"][0])
                print(f"  obs {name:>7} update {update} | norm kernel {pct(res['norm'][0])} ms  wall {pct(res['norm'][1])} ms | encode kernel {pct(res['encode'][0])} ms  wall "
                      f"{pct(res['encode'][1])} ms | torch wall {pct(res['torch'][1])} ms | norm / encode (kernel) {kn / ke:.2f}x, torch / norm (wall) "
                      f"{np.median(res['torch'][1]) / np.median(res['norm'][1]):.1f}x | {(mb_in * (2 if update else 1) + mb_out) / kn:.0f} GB/s of records read + output written")
            del out, enc
        # ---- reward
        rew = torch.empty((K, n), **f64)
        nm = RowNormalizer(n, dev)
        nm.normalize_reward(rows, out=rew)
        ref = torch_reward(rb, K, 1, torch.zeros(n, **f64), torch.tensor(0.0, **f64), torch.tensor(1.0, **f64), torch.tensor(1e-4, **f64))
        print(f"  (reward, update 1: largest |kernel - torch composite| {float((rew - ref).abs().max()):.3g})")
        del ref
        trained = nm.state_dict()
        for update in (1, 0):
            nm = RowNormalizer(n, dev, training=bool(update))
            nm.load_state_dict(dict(trained, training=bool(update)))
            r0, s0 = nm.returns.clone(), nm.ret_stats.clone()
            ways = {"norm": (lambda: nm.normalize_reward(rows, out=rew, timing=True)[1], lambda: nm.normalize_reward(rows, out=rew)),
                    "torch": (None, lambda: torch_reward(rb, K, update, r0, s0[0], s0[1], s0[2]))}
            res = run(ways)
            print(f"  reward          update {update} | norm kernel {pct(res['norm'][0])} ms  wall {pct(res['norm'][1])} ms | torch wall {pct(res['torch'][1])} ms | torch / norm (wall) "
                  f"{np.median(res['torch'][1]) / np.median(res['norm'][1]):.1f}x")
        del rb, rows, rew
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
