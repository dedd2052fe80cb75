#!/usr/bin/env python3
"""What does bg_ppo_loss cost beside the torch composite a learner writes without it?

One process.  65 536 envs (set up as bench.py's) are run 400 steps, then roll out 100 steps into a RowBuffers at stride 384: the masks and the stored
side of a rollout.  Logits are N(0, 2^2), actions are drawn by bg_sample_actions under the records' masks, old_log_prob is their log-prob plus
N(0, 0.15^2), advantages / values / returns N(0, 1); clip_range 0.2, ent_coef 0.01, vf_coef 0.5, advantages normalised.  Shapes (rows): 65 536 and 4 096
-- float32 and bf16 logits, masked from the records and unmasked, with and without an index (a random permutation of the first step's rows, read in
place) -- and one 65 536 x 100 call.  Per shape the ways alternate repeat by repeat in the same process (p10 / median / p90 after warm-up):
  kernel ms   the library's own kernel_ms_out (device events around its two to four launches)
  event ms    device events around the whole Python call, forward plus loss.backward() into logits.grad / values.grad
Partner in the same run:
  composite   SB3's loss as tests/ppo_ref.py states it, on the GPU in float32 under autograd: (index_select ->) masked_fill -> log_softmax -> gather ->
              exp -> clamp -> min -> mean, the entropy and mse terms, then backward() into the same leaves
and bg_bench_copy, whose bytes per second the kernel's useful bytes (logits read + gradient written + 60 mask bytes + 28 bytes of row scalars) are set
against.  Before timing, the composite's loss and gradient are compared with the kernel's (the claims rest on tests/test_ppo_loss.py)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED, T = 20240611, 5
CLIP, ENT, VF = 0.2, 0.01, 0.5


def main():
    import torch
    import torch.nn.functional as F
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-large", action="store_true", help="leave out the 65 536 x 100 call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_loss.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("ppo_loss.py: no GPU is visible", file=sys.stderr)
        return 2
    import bench
    from balatro_gym_amd import BalatroVecEnv, ppo_loss, sample_actions, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    copy_gbps, fill_gbps = bench.measured_copy_gbps(dev)
    say(f"build signature {nat.device_code_signature()}  library {os.path.basename(nat.lib_path())}  GPU {torch.cuda.get_device_name(0)}")
    say(f"bg_bench_copy {copy_gbps:.0f} GB/s (read + written), bg_bench_fill {fill_gbps:.0f} GB/s; logits N(0, 4); masks from records at stride 384; clip {CLIP} "
        f"ent_coef {ENT} vf_coef {VF}, advantages normalised; {args.repeats} repeats after {args.warmup} warm-up, the ways alternating; p10 median p90")

    N, K = 65536, 100
    env = BalatroVecEnv(N, [1000 + g for g in range(N)], device=0, scorer_jokers=True, autoreset=True, max_ante=bench.MAX_ANTE, fused_steps=K)
    env.inject(jokers=[bench.jokers_for(g) for g in range(N)], apply_now=True)
    env.rollout(400, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED, obs_buffers=RowBuffers(N, dev, steps=1))
    rb = RowBuffers(N, dev, steps=K, row_stride=nat.ROW_STRIDE_LINES)
    env.rollout(K, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED + 1, obs_buffers=rb)
    env.check()
    env.close()

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

    def composite(logits, values, mask_rows, actions, old_lp, adv, returns, index):
        """ppo_ref.torch_statement's operations, float32 on the device; forward and backward."""
        logits.grad = None
        values.grad = None
        if index is not None:
            ix = index.long()
            mask_rows = None if mask_rows is None else mask_rows.index_select(0, ix)
            actions, old_lp, adv, returns = actions[ix], old_lp[ix], adv[ix], returns[ix]
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        x = logits.float()
        if mask_rows is not None:
            x = x.masked_fill(mask_rows[..., 176:236] == 0, ninf)
        lp_all = F.log_softmax(x, dim=-1)
        log_prob = lp_all.gather(-1, actions.long()[..., None])[..., 0]
        p = lp_all.exp()
        entropy = -(p * torch.where(p > 0, lp_all, torch.zeros_like(lp_all))).sum(-1)
        ratio = torch.exp(log_prob - old_lp)
        policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - CLIP, 1 + CLIP)).mean()
        value_loss = F.mse_loss(returns, values)
        loss = policy_loss + ENT * (-entropy.mean()) + VF * value_loss
        loss.backward()
        return loss.detach()

    def fused(logits, values, mask_rows, actions, old_lp, adv, returns, index, timing=False):
        logits.grad = None
        values.grad = None
        loss, st = ppo_loss(logits, actions, old_lp, adv, mask_rows, values=values, returns=returns, index=index, clip_range=CLIP, ent_coef=ENT, vf_coef=VF,
                            timing=timing)
        loss.backward()
        return st.kernel_ms if timing else loss.detach()

    g = torch.Generator(device=dev).manual_seed(7)

    def shape(lead, dtype, masked, indexed, name):
        """lead: (n,) or (K, N).  The stored side is the records of step 0 (n rows of it) or of all K steps."""
        n = int(np.prod(lead))
        store_rows = rb.rows[0][:n] if len(lead) == 1 else rb.rows
        logits = (torch.randn(lead + (60,), generator=g, device=dev) * 2.0).to(dtype)
        actions, lp, _ = sample_actions(logits, store_rows, seed=SEED, t=T)
        if not masked:
            actions, lp, _ = sample_actions(logits, None, seed=SEED, t=T)
        old_lp = lp + 0.15 * torch.randn(lead, generator=g, device=dev)
        adv, returns, values = (torch.randn(lead, generator=g, device=dev) for _ in range(3))
        index = None
        if indexed:   # the learner's rows arrive permuted: logits row i belongs to stored row index[i]
            index = torch.randperm(n, generator=g, device=dev).int()
            logits = logits[index.long()].contiguous()
        logits.requires_grad_(True)
        values.requires_grad_(True)
        mrows = store_rows if masked else None
        a = (logits, values, mrows, actions, old_lp, adv, returns, index)
        lf = float(fused(*a))
        gf = logits.grad.float().clone()
        lc = float(composite(*a))
        gdiff = float((gf - logits.grad.float()).abs().max())
        gmax = float(gf.abs().max())
        del gf
        ways = {"kernel": (lambda: fused(*a, timing=True), lambda: fused(*a)), "composite": (None, lambda: composite(*a))}
        res = run(ways)
        km = np.median(res["kernel"][0])
        useful = n * (2 * 60 * logits.element_size() + (60 if masked else 0) + 28) / 1e6
        say(f"  {name:>7} {'masked  ' if masked else 'unmasked'} {'index' if indexed else 'dense'} | kernel {pct(res['kernel'][0])} ms  fwd+bwd events {pct(res['kernel'][1])} ms | "
            f"composite fwd+bwd events {pct(res['composite'][1])} ms | composite p10 / fused events median {np.percentile(res['composite'][1], 10) / np.median(res['kernel'][1]):.1f}x | "
            f"{useful / km:.0f} GB/s useful = {useful / km / copy_gbps * 100:.0f} % of the copy | loss {lf:.6f} vs {lc:.6f}, largest |gradient difference| {gdiff:.3g} of {gmax:.3g}")
        logits.grad = None
        values.grad = None

    for n in (65536, 4096):
        say(f"\n{n} rows x 1")
        for dtype, name in ((torch.float32, "float32"), (torch.bfloat16, "bf16")):
            for masked in (True, False):
                for indexed in (False, True):
                    shape((n,), dtype, masked, indexed, name)
    if not args.skip_large:
        say(f"\n{N} rows x {K}")
        for dtype, name in ((torch.float32, "float32"), (torch.bfloat16, "bf16")):
            shape((K, N), dtype, True, False, name)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
