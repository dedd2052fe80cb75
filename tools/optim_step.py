#!/usr/bin/env python3
"""What does RowOptimizer.step (bg_optim_step) cost beside what a user writes without it, on the same commit?  Writes profiles/optim_step.txt (--out).

Every case runs in a FRESH process (this script starts itself with --case); a case warms up, then times --repeats calls with device events around the
whole Python call and reports p10 / median / p90 in milliseconds.  Gradients are random; timing does not depend on their values.
  (a) the parameter set of train_balatro_fixed.py: pi and vf [512, 512, 256] over 628 inputs, action_net, value_net (16 tensors, 1.45 M elements)
  (b) train_balatro_agent.py's DQN network: the extractor (its three first layers stacked as one RowExtractor weight [448, 447]), 224 -> 512 -> 512, and
      q_net 512 -> 512 -> 512 -> 60, with a target copy of every tensor
  ours          opt.step()                      clip + Adam + shadows (attach) + zero_grad: three launches
  ours+target   opt.step(target_tau=1.0)        (b) only: DQN's hard target update in the same pass
  torch         clip_grad_norm_(params, 0.5); torch.optim.Adam(fused=True, eps=1e-5).step(); zero_grad(set_to_none=False)
  torch+casts   the same plus the per-call casts `attach` removes: (a) two `weight.to(bfloat16)` of [512, 628]; (b) the pitch-448 bfloat16 buffer and its copy
  torch+target  (b) only: torch plus torch._foreach_copy_ of the parameters into the target network
  (a2c) train_balatro_agent.py's A2C network (extractor, pi / vf [256, 256], action_net, value_net):
  ours          RowOptimizer(algorithm="rmsprop_tf").step()
  loop          clip_grad_norm_ + SB3's RMSpropTFLike written as its per-tensor torch loop + zero_grad(set_to_none=False)
  (c) one tensor of 64 M elements: the library's own kernel time (kernel_ms_out, all three launches) and the bytes the call must move -- 4 read by the
      norm pass, 16 read and 16 written by the update pass per element -- against bg_bench_copy on 1 GiB in the same process."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = ["a:ours", "a:torch", "a:torch+casts", "b:ours", "b:ours+target", "b:torch", "b:torch+casts", "b:torch+target", "a2c:ours", "a2c:loop", "c:ours"]


def _mlp(sizes):
    import torch
    return [torch.nn.Linear(i, o, device="cuda") for i, o in zip(sizes[:-1], sizes[1:])]


def _network(which):
    """-> (modules whose parameters are stepped, the record layers to attach, extra (weight, cast) pairs of the torch+casts way)"""
    import torch
    from balatro_gym_amd import RowActor, RowExtractor, RowLinear
    if which == "a":
        pi0, vf0 = RowLinear(512, "fixed", "relu", device="cuda"), RowLinear(512, "fixed", "relu", device="cuda")
        actor = RowActor(256, device="cuda")
        mods = [pi0, vf0] + _mlp([512, 512, 256]) + _mlp([512, 512, 256]) + [actor, torch.nn.Linear(256, 1, device="cuda")]
        return mods, [pi0, vf0, actor], [lambda: pi0.weight.detach().to(torch.bfloat16), lambda: vf0.weight.detach().to(torch.bfloat16)]
    ext = RowExtractor(448, device="cuda")

    def cast():
        wb = torch.empty((448, 448), dtype=torch.bfloat16, device="cuda")[:, :447]
        wb.copy_(ext.weight.detach())
        return wb
    tail = _mlp([256, 128]) + _mlp([128, 64]) + _mlp([64, 32]) + _mlp([224, 512, 512])
    if which == "b":
        return [ext] + tail + _mlp([512, 512, 512, 60]), [ext], [cast]
    actor = RowActor(256, device="cuda")
    return [ext] + tail + _mlp([512, 256, 256]) + _mlp([512, 256, 256]) + [actor, torch.nn.Linear(256, 1, device="cuda")], [ext, actor], [cast]


def run_case(case, repeats, warmup):
    import torch
    from balatro_gym_amd import RowOptimizer, _native as nat
    torch.manual_seed(1)
    which, way = case.split(":")

    def events(fn, n):
        out = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return out
    if which == "c":
        n = 64 * 1024 * 1024
        p = torch.randn(n, device="cuda").requires_grad_()
        p.grad = torch.randn(n, device="cuda")
        opt = RowOptimizer([p], lr=3e-4, max_grad_norm=0.5)
        for _ in range(warmup):
            opt.step()
        ks = [opt.step(timing=True).kernel_ms for _ in range(repeats)]   # the gradients are zero from the first call on: the time does not depend on values
        L = nat.load()
        src, dst = torch.empty(1 << 30, dtype=torch.uint8, device="cuda"), torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
        gbps = C.c_double(0.0)
        rates = []
        for _ in range(5):
            assert L.bg_bench_copy(src.data_ptr(), dst.data_ptr(), C.c_uint64(1 << 30), 20, C.byref(gbps), None) == 0
            rates.append(gbps.value)
        return dict(case=case, tensors=1, elements=n, kernel_ms=ks, bytes=36 * n, copy_gbps=float(np.median(rates)))
    mods, attach, casts = _network(which)
    params = [q for m in mods for q in m.parameters()]
    for q in params:
        q.grad = torch.randn_like(q) * 0.01
    targets = [q.detach().clone() for q in params]
    if way.startswith("ours"):
        opt = RowOptimizer(params, lr=3e-4, algorithm="rmsprop_tf" if which == "a2c" else "adam", eps=1e-5, max_grad_norm=0.5)
        for m in attach:
            opt.attach(m)
        tau = 0.0
        if way == "ours+target":
            opt.set_target(params, targets)
            tau = 1.0
        fn = lambda: opt.step(target_tau=tau)   # noqa: E731
    elif which == "a2c":
        sq = [torch.ones_like(q) for q in params]

        def fn():   # SB3's RMSpropTFLike.step: one loop iteration per tensor
            torch.nn.utils.clip_grad_norm_(params, 0.5)
            with torch.no_grad():
                for q, s in zip(params, sq):
                    g = q.grad
                    s.mul_(0.99).addcmul_(g, g, value=0.01)
                    q.addcdiv_(g, s.add(1e-5).sqrt_(), value=-7e-4)
            torch._foreach_zero_([q.grad for q in params])
    else:
        adam = torch.optim.Adam(params, lr=3e-4, eps=1e-5, fused=True)

        def fn():
            torch.nn.utils.clip_grad_norm_(params, 0.5)
            adam.step()
            adam.zero_grad(set_to_none=False)
            if way == "torch+casts":
                for cast in casts:
                    cast()
            if way == "torch+target":
                with torch.no_grad():
                    torch._foreach_copy_(targets, params)
    events(fn, warmup)
    torch.cuda.synchronize()
    return dict(case=case, tensors=len(params), elements=int(sum(q.numel() for q in params)), call_ms=events(fn, repeats))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--case", default=None, help="(internal) run one case in this process and print its JSON line")
    ap.add_argument("--cases", nargs="+", default=CASES)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("optim_step.py: no GPU is visible", file=sys.stderr)
        return 2
    if args.case:
        rep = 20 if args.case.startswith("c:") else args.repeats
        print("RESULT " + json.dumps(run_case(args.case, rep, 3 if args.case.startswith("c:") else args.warmup)), flush=True)
        return 0
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    from balatro_gym_amd import _native as nat
    say(f"tools/optim_step.py --repeats {args.repeats} --warmup {args.warmup}: one fresh process per case, device events around the whole call, milliseconds")
    say(f"device code {nat.device_code_signature()}, {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    say(f"{'case':<16}{'tensors':>8}{'elements':>12}{'p10':>10}{'median':>10}{'p90':>10}")
    med = {}
    for case in args.cases:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--repeats", str(args.repeats), "--warmup", str(args.warmup)],
                           capture_output=True, text=True, timeout=600)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not got:
            say(f"{case:<16} FAILED (exit {r.returncode}): {r.stderr.strip()[-400:]}")
            return 1   # a failed case ends the run: nothing more is started on the GPU
        d = json.loads(got[0][7:])
        x = d.get("call_ms") or d["kernel_ms"]
        med[case] = float(np.median(x))
        say(f"{case:<16}{d['tensors']:>8}{d['elements']:>12}{np.percentile(x, 10):>10.4f}{np.median(x):>10.4f}{np.percentile(x, 90):>10.4f}")
        if "copy_gbps" in d:
            rate = d["bytes"] / (med[case] * 1e-3) / 1e9
            say(f"  (c) kernel time of the three launches; {d['bytes'] / 2 ** 30:.2f} GiB moved -> {rate:.0f} GB/s; bg_bench_copy {d['copy_gbps']:.0f} GB/s; "
                f"share {rate / d['copy_gbps']:.2f}")
    say()
    for a, b in (("a:ours", "a:torch"), ("a:ours", "a:torch+casts"), ("b:ours", "b:torch"), ("b:ours", "b:torch+casts"), ("b:ours+target", "b:torch+target"),
                 ("a2c:ours", "a2c:loop")):
        if a in med and b in med:
            say(f"{b} / {a}: {med[b] / med[a]:.2f}x  ({med[b] - med[a]:+.4f} ms per step)")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
