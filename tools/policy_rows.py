#!/usr/bin/env python3
"""What does RowPolicy.act (bg_policy_forward: every hidden layer, action_net, the masked draw and value_net in one launch) cost beside the torch
composite it replaces on the same commit?  Writes profiles/policy_rows.txt (--out).

A fresh process per case (--case TOPOLOGY M is what a child runs; the parent starts them one after the other and stops at the first that fails).
m envs (set up as bench.py's) are run 64 steps and 4 more into a RowBuffers at stride 384; the last step's records are the input.
  agent   train_balatro_agent.py:54-82, 338-342: h = RowExtractor.from_linears(416->256, 10->128, 21->64)(records) bfloat16 [m, 448];
          second layers 256->128, 128->64, 64->32 (ReLU), combined_net 224->512->512 (ReLU), pi and vf 512->256->256 (Tanh), action_net, value_net
  fixed   train_balatro_fixed.py:361-364: net_arch pi [512, 512, 256] / vf [512, 512, 256], ReLU.  h = RowLinear(512)(records) bfloat16 [m, 512] stands for
          the first layer; pi and vf 512->512->256, action_net, value_net.  (The script's vf has a first layer of its own; here both branches read the one
          h: the same arithmetic per row, see README.)
  ours       policy.act(h, records, seed=, t=)                                                                    one launch
  composite  the same nn.Linear modules after .to(bfloat16) on h (slices, cat, F.linear + activation), values = value_net(latent_vf).float(),
             RowActor.act(latent_pi, records, seed=, t=)                                                          ~20 launches
"call" is device events around the whole Python call, the two ways alternating repeat by repeat (p10 / median / p90 of --repeats after warm-up);
"kernel" is the library's kernel_ms_out of ours alone, in repeats of their own (asking for it synchronises).  The MFMA floor: the launch's count of
v_mfma_f32_32x32x16_bf16 (per workgroup of 32 rows: sum over layers of ceil(out / 32) * in / 16) at 32 cycles each over the device's 4 SIMDs per CU at
its clock (2.4 GHz where torch reports none)."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED, T = 20240611, 5
TOPOLOGIES = ("agent", "fixed")


def child(args):
    import torch
    if not torch.cuda.is_available():
        print("policy_rows.py: no GPU is visible", file=sys.stderr)
        return 2
    import bench
    from balatro_gym_amd import BalatroVecEnv, RowActor, RowDense, RowExtractor, RowLinear, RowOptimizer, RowPolicy, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers
    topo, m = args.case[0], int(args.case[1])
    dev = torch.device("cuda:0")
    nn = torch.nn
    torch.manual_seed(7)
    env = BalatroVecEnv(m, [1000 + g for g in range(m)], device=0, scorer_jokers=True, autoreset=True, max_ante=bench.MAX_ANTE, fused_steps=64)
    env.inject(jokers=[bench.jokers_for(g) for g in range(m)], apply_now=True)
    env.rollout(64, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED, obs_buffers=RowBuffers(m, dev, steps=1))
    rb = RowBuffers(m, dev, steps=4, row_stride=nat.ROW_STRIDE_LINES)
    env.rollout(4, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED + 1, obs_buffers=rb)
    env.check()
    env.close()
    records = rb.rows[-1]

    if topo == "agent":
        first = RowExtractor.from_linears(nn.Linear(416, 256), nn.Linear(10, 128), nn.Linear(21, 64)).to(dev)
        second = [nn.Linear(256, 128), nn.Linear(128, 64), nn.Linear(64, 32)]
        combined = [nn.Linear(224, 512), nn.Linear(512, 512)]
        pi, vf, act = [nn.Linear(512, 256), nn.Linear(256, 256)], [nn.Linear(512, 256), nn.Linear(256, 256)], "tanh"
        trunk = [RowPolicy.stack_blocks(second, "relu")] + [RowDense.from_linear(l, "relu") for l in combined]
    else:
        first = RowLinear(512, activation="relu").to(dev)
        second, combined = [], []
        pi, vf, act = [nn.Linear(512, 512), nn.Linear(512, 256)], [nn.Linear(512, 512), nn.Linear(512, 256)], "relu"
        trunk = []
    action_net, value_net = nn.Linear(256, 60), nn.Linear(256, 1)
    policy = RowPolicy(trunk, [RowDense.from_linear(l, act) for l in pi], [RowDense.from_linear(l, act) for l in vf], RowActor.from_linear(action_net),
                       RowDense.from_linear(value_net)).to(dev)
    opt = RowOptimizer(list(policy.parameters()))
    opt.attach(policy)   # every layer reads its bfloat16 copy: the table is built once
    with torch.no_grad():
        h = first(records)
    b16 = lambda ls: [l.to(dev).to(torch.bfloat16) for l in ls]   # noqa: E731
    second, combined, pi, vf = b16(second), b16(combined), b16(pi), b16(vf)
    value16 = value_net.to(dev).to(torch.bfloat16)
    fn = torch.tanh if act == "tanh" else torch.relu
    splits = (256, 128, 64)

    @torch.no_grad()
    def composite():
        x = h
        if second:
            x = torch.cat([torch.relu(l(p)) for l, p in zip(second, x.split(splits, dim=1))], 1)
        for l in combined:
            x = torch.relu(l(x))
        p = v = x
        for l in pi:
            p = fn(l(p))
        for l in vf:
            v = fn(l(v))
        values = value16(v).float()[:, 0]
        a, lp, _ = policy.action.act(p, records, seed=SEED, t=T)
        return a, lp, values

    def ours(timing=False):
        return policy.act(h, records, seed=SEED, t=T, timing=timing)

    def events(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = f()
        b.record()
        b.synchronize()
        del r
        return a.elapsed_time(b)

    o, c = ours(), composite()
    torch.cuda.synchronize()
    dv = float((o[2] - c[2]).abs().max())
    same = float((o[0] == c[0]).float().mean())
    res = {"ours": [], "composite": []}
    for i in range(args.warmup + args.repeats):
        for k, f in (("ours", ours), ("composite", composite)):
            e = events(f)
            if i >= args.warmup:
                res[k].append(e)
    kern = [ours(True)[-1] for _ in range(args.warmup + args.repeats)][args.warmup:]
    layers = policy.layers()
    mfma = sum(-(-l.out_features // 32) * (l.in_features // 16) for l in layers) * -(-m // 32)
    prop = torch.cuda.get_device_properties(0)
    ghz = getattr(prop, "clock_rate", 2.4e6) / 1e6   # kHz; 2.4 GHz (the MI355X's peak engine clock) where torch does not report one
    floor_ms = mfma * 32 / (prop.multi_processor_count * 4) / (ghz * 1e9) * 1e3
    pct = lambda x: f"{np.percentile(x, 10):8.4f} {np.median(x):8.4f} {np.percentile(x, 90):8.4f}"   # noqa: E731
    ratio = np.median(res["composite"]) / np.median(res["ours"])
    print(f"RESULT {topo:>6} {m:>6} | {np.median(kern):>11.4f} {pct(res['ours'])} | {pct(res['composite'])} | {ratio:>6.2f}x | {mfma:>9} {floor_ms:>8.4f} {100 * floor_ms / np.median(kern):>5.1f}% | "
          f"{dv:.3g} {100 * same:.1f}%", flush=True)
    print(f"INFO build signature {nat.device_code_signature()}  GPU {torch.cuda.get_device_name(0)}  {prop.multi_processor_count} CUs at {ghz:.2f} GHz", flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--case", nargs=2, default=None, metavar=("TOPOLOGY", "M"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_rows.txt"))
    args = ap.parse_args()
    if args.case:
        return child(args)
    lines, info = [], None
    for topo in TOPOLOGIES:
        for m in args.batches:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", topo, str(m), "--repeats", str(args.repeats), "--warmup", str(args.warmup)],
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
                print(f"policy_rows.py: the case {topo} {m} failed ({r.returncode}): nothing more is started", file=sys.stderr)
                return 1
            for ln in r.stdout.splitlines():
                if ln.startswith("RESULT "):
                    lines.append(ln[7:])
                    print(ln[7:], flush=True)
                elif ln.startswith("INFO "):
                    info = ln[5:]
    head = [info or "", f"h from the first layer over records at stride 384, every layer's bfloat16 copy attached; {args.repeats} repeats after {args.warmup} warm-up, the ways "
            "alternating, a fresh process per case; device events; ms",
            f"{'net':>6} {'m':>6} | {'ours kernel':>11} {'call p10':>8} {'median':>8} {'p90':>8} | {'composite call p10':>8} {'median':>8} {'p90':>8} | composite / ours | "
            f"{'MFMAs':>9} {'floor ms':>8} {'rate':>6} | max |values - composite's|, share of equal actions"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(head + lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
