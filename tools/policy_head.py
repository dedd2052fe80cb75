#!/usr/bin/env python3
"""What do bg_sample_actions / bg_evaluate_actions cost beside the torch composite a user writes without them?

One process.  65 536 envs (set up as bench.py's) are run 400 steps, then roll out 100 steps into a RowBuffers at stride 384: the masks.  Logits are
N(0, 2^2).  Shapes (rows): 65 536 and 4 096 for sampling -- float32 and bf16 logits, masked from the last step's records and unmasked -- and
65 536 x 100 for evaluating given actions.  Per shape the ways alternate repeat by repeat in the same process (p10 / median / p90 after warm-up):
  kernel ms   the library's own kernel_ms_out (device events around the launch)
  event ms    device events around the whole Python call (for the composite: around its seven to nine launches)
Partners in the same run:
  composite   masked_fill -> log_softmax -> exp -> cumsum -> compare / argmax with the SAME u (precomputed, which favours it) -> gather -> entropy
  multinomial the same with torch.multinomial drawing the action
  evaluate    masked_fill -> log_softmax -> gather -> entropy
and bg_bench_copy, whose bytes per second the kernel's useful bytes (logits + 60 mask bytes + outputs per row) are set against.
Before timing, the composite's actions are compared with the kernel's (torch's cumsum adds in another order, so equality on every row is not expected;
the claims rest on tests/test_policy_head.py)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED, T = 20240611, 5


def hash_u(seed, n, t):
    """u of rows 0..n-1: the counter hash of bg_sample_actions (splitmix64 finaliser, high 32 bits), 24 bits as a float32 in [0, 1)."""
    m64 = (1 << 64) - 1
    with np.errstate(over="ignore"):
        x = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (np.arange(n, dtype=np.uint64) + np.uint64(1)) + np.uint64((0xD1B54A32D192ED03 * (t + 1)) & m64)
        x ^= x >> np.uint64(30); x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27); x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return ((x >> np.uint64(40)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_head.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("policy_head.py: no GPU is visible", file=sys.stderr)
        return 2
    import bench
    from balatro_gym_amd import BalatroVecEnv, evaluate_actions, sample_actions, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    copy_gbps, fill_gbps = bench.measured_copy_gbps(dev)
    say(f"build signature {nat.device_code_signature()}  library {os.path.basename(nat.lib_path())}  GPU {torch.cuda.get_device_name(0)}")
    say(f"bg_bench_copy {copy_gbps:.0f} GB/s (read + written), bg_bench_fill {fill_gbps:.0f} GB/s; logits N(0, 4); masks from records at stride 384; "
        f"{args.repeats} repeats after {args.warmup} warm-up, the ways alternating; p10 median p90")

    N, K = 65536, 100
    env = BalatroVecEnv(N, [1000 + g for g in range(N)], device=0, scorer_jokers=True, autoreset=True, max_ante=bench.MAX_ANTE, fused_steps=K)
    env.inject(jokers=[bench.jokers_for(g) for g in range(N)], apply_now=True)
    env.rollout(400, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED, obs_buffers=RowBuffers(N, dev, steps=1))
    rb = RowBuffers(N, dev, steps=K, row_stride=nat.ROW_STRIDE_LINES)
    env.rollout(K, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED + 1, obs_buffers=rb)
    env.check()
    env.close()
    valid_share = float((rb.tensors["action_mask"][-1] != 0).float().mean())
    say(f"records of {N} envs x {K} steps after 400 steps of warm-up; {valid_share * 60:.1f} of 60 actions valid on average in the last step")

    def pct(x):
        return f"{np.percentile(x, 10):8.4f} {np.median(x):8.4f} {np.percentile(x, 90):8.4f}"

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        del r
        return a.elapsed_time(b)

    def run(ways):
        """ways: name -> (fn returning kernel ms or None, fn for the events).  Alternating; returns name -> (kernel list, event list)."""
        res = {k: ([], []) for k in ways}
        for i in range(args.warmup + args.repeats):
            for k, (kfn, efn) in ways.items():
                ms = kfn() if kfn else None
                e = events(efn)
                if i >= args.warmup:
                    if ms is not None:
                        res[k][0].append(ms)
                    res[k][1].append(e)
        return res

    ninf = float("-inf")

    def valid_of(mask_rows):
        return None if mask_rows is None else mask_rows[..., 176:236] != 0

    def entropy_of(lp, p, valid):
        return -(p * (lp if valid is None else lp.masked_fill(~valid, 0.0))).sum(-1)

    def composite(logits, mask_rows, u):
        valid = valid_of(mask_rows)
        x = logits.float()
        lp = torch.log_softmax(x if valid is None else x.masked_fill(~valid, ninf), -1)
        p = lp.exp()
        a = (p.cumsum(-1) > u[:, None]).to(torch.uint8).argmax(-1)
        return a.int(), lp.gather(-1, a[:, None])[:, 0], entropy_of(lp, p, valid)

    def multinomial(logits, mask_rows):
        valid = valid_of(mask_rows)
        x = logits.float()
        lp = torch.log_softmax(x if valid is None else x.masked_fill(~valid, ninf), -1)
        p = lp.exp()
        a = torch.multinomial(p, 1)
        return a[:, 0].int(), lp.gather(-1, a)[:, 0], entropy_of(lp, p, valid)

    def evaluate(logits, mask_rows, actions):
        valid = valid_of(mask_rows)
        x = logits.float()
        lp = torch.log_softmax(x if valid is None else x.masked_fill(~valid, ninf), -1)
        return lp.gather(-1, actions.long()[..., None])[..., 0], entropy_of(lp, lp.exp(), valid)

    g = torch.Generator(device=dev).manual_seed(7)
    for n in (65536, 4096):
        u = torch.from_numpy(hash_u(SEED, n, T)).to(dev)
        say(f"\nsample, {n} rows x 1")
        for dtype, name in ((torch.float32, "float32"), (torch.bfloat16, "bf16")):
            logits = (torch.randn((n, 60), generator=g, device=dev) * 2.0).to(dtype)
            for masked in (True, False):
                mrows = rb.rows[-1][:n] if masked else None
                a = torch.empty(n, dtype=torch.int32, device=dev)
                lp, en = torch.empty(n, device=dev), torch.empty(n, device=dev)
                kw = dict(seed=SEED, t=T, actions=a, log_prob=lp, entropy=en)
                sample_actions(logits, mrows, **kw)
                ca, clp, cen = composite(logits, mrows, u)
                same = a == ca
                say(f"  ({name}, {'masked' if masked else 'unmasked'}: composite draws the kernel's action on {float(same.float().mean()) * 100:.3f} % of rows; there, largest "
                    f"|log_prob difference| {float((lp - clp)[same].abs().max()):.3g}, |entropy difference| {float((en - cen)[same].abs().max()):.3g})")
                ways = {"kernel": (lambda: sample_actions(logits, mrows, timing=True, **kw)[3], lambda: sample_actions(logits, mrows, **kw)),
                        "composite": (None, lambda: composite(logits, mrows, u)),
                        "multinomial": (None, lambda: multinomial(logits, mrows))}
                res = run(ways)
                km = np.median(res["kernel"][0])
                useful = n * (60 * logits.element_size() + (60 if masked else 0) + 12) / 1e6
                cp10 = np.percentile(res["composite"][1], 10)
                say(f"  {name:>7} {'masked  ' if masked else 'unmasked'} | kernel {pct(res['kernel'][0])} ms  events {pct(res['kernel'][1])} ms | composite events {pct(res['composite'][1])} ms | "
                    f"multinomial events {pct(res['multinomial'][1])} ms | composite p10 / kernel events median {cp10 / np.median(res['kernel'][1]):.1f}x | "
                    f"{useful / km:.0f} GB/s useful = {useful / km / copy_gbps * 100:.0f} % of the copy")
    say(f"\nevaluate, {N} rows x {K}")
    for dtype, name in ((torch.float32, "float32"), (torch.bfloat16, "bf16")):
        logits = (torch.randn((K, N, 60), generator=g, device=dev) * 2.0).to(dtype)
        actions = sample_actions(logits, rb.rows, seed=SEED, t=T)[0]
        lp, en = torch.empty((K, N), device=dev), torch.empty((K, N), device=dev)
        for masked in (True, False):
            mrows = rb.rows if masked else None
            evaluate_actions(logits, actions, mrows, log_prob=lp, entropy=en)
            clp, cen = evaluate(logits, mrows, actions)
            say(f"  ({name}, {'masked' if masked else 'unmasked'}: largest |log_prob difference| {float((lp - clp).abs().max()):.3g}, |entropy difference| {float((en - cen).abs().max()):.3g})")
            del clp, cen
            ways = {"kernel": (lambda: evaluate_actions(logits, actions, mrows, log_prob=lp, entropy=en, timing=True)[2], lambda: evaluate_actions(logits, actions, mrows, log_prob=lp, entropy=en)),
                    "composite": (None, lambda: evaluate(logits, mrows, actions))}
            res = run(ways)
            km = np.median(res["kernel"][0])
            useful = K * N * (60 * logits.element_size() + (60 if masked else 0) + 12) / 1e6
            say(f"  {name:>7} {'masked  ' if masked else 'unmasked'} | kernel {pct(res['kernel'][0])} ms  events {pct(res['kernel'][1])} ms | composite events {pct(res['composite'][1])} ms | "
                f"composite p10 / kernel events median {np.percentile(res['composite'][1], 10) / np.median(res['kernel'][1]):.1f}x | "
                f"{useful / km:.0f} GB/s useful = {useful / km / copy_gbps * 100:.0f} % of the copy")
        del logits, actions
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
