#!/usr/bin/env python3
"""What does bg_dqn_loss cost beside the same loss written in torch?

One process, one commit.  65 536 envs (set up as bench.py's) are run 400 steps, then 16 steps go into a RowReplay of 16 slots at stride 384: a ring of
65 536 x 16 records (403 MB), full.  A minibatch is `replay.sample(m)`; Q values are N(0, 2^2) float32 (no network: the loss alone is measured), gamma
0.99, Huber, step-limit endings as ordinary done rows (there are none without limits).  Shapes: 32, 4 096 and 65 536 rows; masked by the next record's
action mask and unmasked; plain and double DQN.  Per shape the two ways alternate repeat by repeat (p10 / median / p90 after warm-up):
  kernel ms   the library's own kernel_ms_out (device events around its two launches)
  event ms    device events around the whole Python call, forward plus loss.backward() into q.grad
Partner in the same run:
  composite   the loss in torch float32 under autograd: gather of the action, the reward, the terminated byte (and the mask) from the ring at
              next_index -> masked_fill + max (double: argmax + gather) -> where(done) -> smooth_l1_loss -> backward() into the same leaf
Both timed calls do the whole job from the ring on every call: the composite gathers its actions, rewards, done flags and masks from the records each
time, as the kernel reads them in place.  Before timing, the composite's action and target are drawn on every included row and compared with the
kernel's: the largest |td difference| over the included rows and the two losses are printed with each line (the claims rest on tests/test_dqn_loss.py).
The kernel's useful bytes (q_next (+ online) read, dq written, 60 mask bytes, 24 bytes of fields and index per row) are set against bg_bench_copy.
No ratio is demanded of either side; what comes out is written down, the small shapes included, where the Python wrapper is most of the call."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GAMMA = 0.99


def main():
    import torch
    import torch.nn.functional as F
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dqn_loss.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("dqn_loss.py: no GPU is visible", file=sys.stderr)
        return 2
    import bench
    from balatro_gym_amd import BalatroVecEnv, RowReplay, dqn_loss, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    copy_gbps, fill_gbps = bench.measured_copy_gbps(dev)
    say(f"build signature {nat.device_code_signature()}  library {os.path.basename(nat.lib_path())}  GPU {torch.cuda.get_device_name(0)}")
    say(f"bg_bench_copy {copy_gbps:.0f} GB/s (read + written), bg_bench_fill {fill_gbps:.0f} GB/s; Q values N(0, 4) float32; a full ring of {args.envs} x 16 records at "
        f"stride 384; gamma {GAMMA}, Huber; {args.repeats} repeats after {args.warmup} warm-up, the ways alternating; p10 median p90")

    N, Cn = args.envs, 16
    env = BalatroVecEnv(N, [1000 + g for g in range(N)], device=0, scorer_jokers=True, autoreset=True, max_ante=bench.MAX_ANTE, fused_steps=Cn)
    env.inject(jokers=[bench.jokers_for(g) for g in range(N)], apply_now=True)
    one = RowBuffers(N, dev, steps=1, row_stride=nat.ROW_STRIDE_LINES)
    env.rollout(400, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED, obs_buffers=one)
    replay = RowReplay(Cn, N, dev)
    replay.start(one.rows[0])
    rb = RowBuffers(N, dev, steps=Cn - 1, row_stride=nat.ROW_STRIDE_LINES)
    env.rollout(Cn - 1, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED + 1, obs_buffers=rb)
    replay.add(rb.rows)
    env.rollout(1, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED + 2, obs_buffers=one)
    replay.add(one.rows)   # the ring wraps: slot 0 holds the newest record
    env.check()
    env.close()
    del rb, one
    torch.cuda.empty_cache()
    assert len(replay) == (Cn - 1) * N
    store = replay.store
    flat = store.view(-1, store.shape[-1])
    # the fields of every record as strided views of the ring (what RowBuffers exposes)
    f_action = flat[:, 172:176].view(torch.int32)[:, 0]
    f_reward = flat[:, 136:144].view(torch.float64)[:, 0]
    f_done = flat[:, 342]
    f_mask = flat[:, 176:236]

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

    def composite(q, q_next, q_online, next_index, masked, backward=True):
        """dqn_ref.sb3_statement's operations, float32 on the device; forward and backward.  -> (loss, td)"""
        q.grad = None
        nx = next_index.long()
        a = f_action[nx].long()
        r = f_reward[nx].float()
        done = f_done[nx] != 0
        sel = q_next if q_online is None else q_online
        if masked:
            sel = sel.masked_fill(f_mask[nx] == 0, ninf)
        n = sel.max(1).values if q_online is None else q_next.gather(1, sel.argmax(1, keepdim=True))[:, 0]
        y = torch.where(done, r, r + GAMMA * n)
        cur = q.gather(1, a[:, None])[:, 0]
        loss = F.smooth_l1_loss(cur, y)
        if backward:
            loss.backward()
        return loss.detach(), (cur - y).detach()

    def fused(q, q_next, q_online, next_index, masked, timing=False):
        q.grad = None
        loss, st = dqn_loss(q, q_next, store, next_index, q_next_online=q_online, gamma=GAMMA, mask_next=masked, timeouts="terminal", timing=timing)
        loss.backward()
        return st.kernel_ms if timing else loss.detach()

    g = torch.Generator(device=dev).manual_seed(7)

    def shape(m, masked, double):
        index, next_index = replay.sample(m, generator=g)
        q = (torch.randn((m, 60), generator=g, device=dev) * 2.0).requires_grad_(True)
        q_next = torch.randn((m, 60), generator=g, device=dev) * 2.0
        q_online = q_next + torch.randn((m, 60), generator=g, device=dev) if double else None
        a = (q, q_next, q_online, next_index, masked)
        lf, st = dqn_loss(q, q_next, store, next_index, q_next_online=q_online, gamma=GAMMA, mask_next=masked, timeouts="terminal")
        lc, tdc = composite(*a, backward=False)
        inc = ~torch.isnan(st.td)
        tdiff = float((st.td[inc] - tdc[inc]).abs().max())
        excluded = int(st.excluded)
        lf = float(lf.detach())
        fused(*a)
        gf = q.grad.clone()
        composite(*a)
        gdiff = float((gf - q.grad).abs().max())
        ways = {"kernel": (lambda: fused(*a, timing=True), lambda: fused(*a)), "composite": (None, lambda: composite(*a)[0])}
        res = run(ways)
        km = np.median(res["kernel"][0])
        useful = m * (60 * 4 * (3 if double else 2) + (60 if masked else 0) + 24) / 1e6
        say(f"  {m:>6} rows {'masked  ' if masked else 'unmasked'} {'double' if double else 'plain '} | kernel {pct(res['kernel'][0])} ms  fwd+bwd events {pct(res['kernel'][1])} ms | "
            f"composite fwd+bwd events {pct(res['composite'][1])} ms | composite median / fused events median {np.median(res['composite'][1]) / np.median(res['kernel'][1]):.1f}x | "
            f"{useful / km:.0f} GB/s useful = {useful / km / copy_gbps * 100:.0f} % of the copy | loss {lf:.6f} vs {float(lc):.6f}; {int(inc.sum())} included rows "
            f"({excluded} excluded), largest |td difference| {tdiff:.3g}, largest |gradient difference| {gdiff:.3g} of {float(gf.abs().max()):.3g}")
        q.grad = None

    for m in (32, 4096, 65536):
        say(f"\n{m} rows out of {N} x {Cn}")
        for masked in (True, False):
            for double in (False, True):
                shape(m, masked, double)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
