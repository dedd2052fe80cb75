#!/usr/bin/env python3
"""What do bg_episode_outcome_rows and bg_bc_loss cost beside the same work written in torch, and did the calls next to them move?

One commit.  A [K = 100, N] store of records at stride 384 is built on the device (N = 65 536 and 4 096): random bytes, a terminated byte set with
probability 0.05, end flags, end antes 1..8, N(0, 1) rewards, action masks with 60 % of the actions valid and a stored action that is valid under the
mask of the record one step earlier.  Medians (p10 / median / p90 after warm-up), by the library's own kernel_ms_out (device events around its
launches) and by device events around the whole Python call:
  outcome scan   episode_outcomes(store, 0.99), all four outputs, and end_ante alone (the filter: no reward line is read)
      against    the loop of K iterations over the strided views (reward, terminated, end_flags, end_ante) in torch, all four outputs
  bc loss        bc_loss forward plus loss.backward() into logits.grad over a minibatch of m = 65 536 and 4 096 rows (the first m observation
                 records): mask and action read in place from the records, weights = (end_ante >= 5) of the scan, ent_coef 0.01
      against    the torch composite under autograd (mask bytes and actions gathered from the strided views on every call, masked_fill, log_softmax,
                 gather, weighted mean, entropy, backward())
      against    the two-launch route: evaluate_actions for old_log_prob, then ppo_loss at ratio 1 with the weights as advantages, plus backward()
  neighbours     the contiguous medians of gae_rows (K x N) and ppo_loss (m rows) on this library and, with --baseline-root, on another checkout
                 with its own built library (the parent commit's) in a child process of its own: they should not have moved.
No ratio is promised; what comes out is written down.  --notes FILE is appended verbatim (the compiler's resource lines, tools/isa_diff.py's finding)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("BC_ROWS_PACKAGE_ROOT") or ROOT)   # (the child process of --baseline-root imports the other checkout's package)
K, STRIDE, GAMMA = 100, 384, 0.99
SIZES = (65536, 4096)


def pct(xs):
    a = np.sort(np.asarray(xs, np.float64))
    return f"{a[int(0.1 * (len(a) - 1))]:.4f} {np.median(a):.4f} {a[int(round(0.9 * (len(a) - 1)))]:.4f}"


def timed(torch, fn, repeats, warmup):
    """-> (event ms of the whole call, what fn returned last) per repeat after warm-up."""
    out, ms = None, []
    for r in range(warmup + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        if r >= warmup:
            ms.append(a.elapsed_time(b))
    return ms, out


def build_store(torch, N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    store = torch.randint(0, 256, (K + 1, N, STRIDE), dtype=torch.uint8, device="cuda", generator=g)
    done = torch.rand((K + 1, N), device="cuda", generator=g) < 0.05
    store[:, :, 342] = done.to(torch.uint8)
    store[:, :, 343] = torch.where(done, torch.randint(1, 8, (K + 1, N), device="cuda", generator=g), 0).to(torch.uint8)
    store[:, :, 344:346] = torch.randint(1, 9, (K + 1, N), device="cuda", generator=g).to(torch.int16).view(torch.uint8).view(K + 1, N, 2)
    store[:, :, 136:144] = torch.randn((K + 1, N), dtype=torch.float64, device="cuda", generator=g).view(torch.uint8).view(K + 1, N, 8)
    mask = (torch.rand((K + 1, N, 60), device="cuda", generator=g) < 0.6)
    mask[:, :, 0] = True
    store[:, :, 176:236] = mask.to(torch.uint8)
    # the action stored in record t + 1 is valid under the mask of record t
    pick = torch.multinomial(mask[:K].reshape(-1, 60).float(), 1, generator=g).view(K, N).to(torch.int32)
    store[1:, :, 172:176] = pick.view(torch.uint8).view(K, N, 4)
    return store


def torch_outcome_loop(torch, store, gamma):
    Kn, N = store.shape[0], store.shape[1]
    reward = store[:, :, 136:144].view(torch.float64)[:, :, 0]
    done = store[:, :, 342]
    flags = store[:, :, 343]
    ante = store[:, :, 344:346].view(torch.int16)[:, :, 0]
    steps_o = torch.empty((Kn, N), dtype=torch.int32, device=store.device)
    ante_o, flags_o = torch.empty_like(steps_o), torch.empty((Kn, N), dtype=torch.uint8, device=store.device)
    ret_o = torch.empty((Kn, N), dtype=torch.float64, device=store.device)
    s = torch.full((N,), -1, dtype=torch.int32, device=store.device)
    a, f, r = s.clone(), torch.zeros(N, dtype=torch.uint8, device=store.device), torch.zeros(N, dtype=torch.float64, device=store.device)
    for t in range(Kn - 1, -1, -1):
        d = done[t] != 0
        s = torch.where(d, 0, torch.where(s < 0, -1, s + 1)).to(torch.int32)
        a = torch.where(d, ante[t].to(torch.int32), a)
        f = torch.where(d, flags[t], f)
        r = torch.where(d, reward[t], reward[t] + gamma * r)
        steps_o[t], ante_o[t], flags_o[t], ret_o[t] = s, a, f, r
    return steps_o, ante_o, flags_o, ret_o


def neighbours(torch, repeats, warmup):
    """The contiguous medians of gae_rows and ppo_loss on whatever library this process loads -> dict."""
    from balatro_gym_amd import gae_rows, ppo_loss, _native as nat
    out = {"signature": nat.device_code_signature(), "library": nat.lib_path()}
    for N in SIZES:
        store = build_store(torch, N, 5)
        rows = store[1:]
        values = torch.randn((K, N), device="cuda")
        last = torch.randn(N, device="cuda")
        ker = [gae_rows(rows, values, last, timing=True)[2] for _ in range(warmup + repeats)][warmup:]
        ev, _ = timed(torch, lambda: gae_rows(rows, values, last), repeats, warmup)
        out[f"gae_rows {K} x {N}"] = {"kernel": pct(ker), "event": pct(ev)}
        m = N
        logits = torch.randn((m, 60), device="cuda") * 2.0
        mask = store[0]
        acts = store[1, :, 172:176].view(torch.int32)[:, 0].contiguous()
        olp, adv = torch.randn(m, device="cuda") * 0.1 - 2.0, torch.randn(m, device="cuda")
        ker = [ppo_loss(logits, acts, olp, adv, mask, ent_coef=0.01, timing=True)[1].kernel_ms for _ in range(warmup + repeats)][warmup:]
        ev, _ = timed(torch, lambda: ppo_loss(logits, acts, olp, adv, mask, ent_coef=0.01), repeats, warmup)
        out[f"ppo_loss {m} rows"] = {"kernel": pct(ker), "event": pct(ev)}
        del store, rows
        torch.cuda.empty_cache()
    return out


def main():
    import torch
    import torch.nn.functional as F
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-root", default=None, help="another checkout with its built library (the parent commit's): its gae_rows / ppo_loss medians, from a child process")
    ap.add_argument("--neighbours-only", action="store_true", help="print the neighbours' medians as one JSON line and stop (what the child process runs)")
    ap.add_argument("--notes", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc_rows.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bc_rows.py: no GPU is visible", file=sys.stderr)
        return 2
    if args.neighbours_only:
        print("NEIGHBOURS " + json.dumps(neighbours(torch, args.repeats, args.warmup)), flush=True)
        return 0
    from balatro_gym_amd import bc_loss, episode_outcomes, evaluate_actions, ppo_loss, _native as nat
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"build signature {nat.device_code_signature()}  library {os.path.basename(nat.lib_path())}  GPU {torch.cuda.get_device_name(0)}")
    say(f"synthetic records, K = {K}, stride {STRIDE}, gamma {GAMMA}; {args.repeats} repeats after {args.warmup} warm-up; milliseconds: p10 median p90")
    for N in SIZES:
        store = build_store(torch, N, 5)
        rows = store[1:]           # the K step records; store[:K] are their observation records
        say()
        say(f"== {N} x {K} records ({rows.numel() / 1e6:.0f} MB)")
        ker = [episode_outcomes(rows, GAMMA, timing=True).kernel_ms for _ in range(args.warmup + args.repeats)][args.warmup:]
        ev, o = timed(torch, lambda: episode_outcomes(rows, GAMMA), args.repeats, args.warmup)
        say(f"outcome scan, four outputs      kernel {pct(ker)}   call {pct(ev)}")
        ker = [episode_outcomes(rows, GAMMA, want=("end_ante",), timing=True).kernel_ms for _ in range(args.warmup + args.repeats)][args.warmup:]
        ev, _ = timed(torch, lambda: episode_outcomes(rows, GAMMA, want=("end_ante",)), args.repeats, args.warmup)
        say(f"outcome scan, end_ante alone    kernel {pct(ker)}   call {pct(ev)}")
        ev, ref = timed(torch, lambda: torch_outcome_loop(torch, rows, GAMMA), max(3, args.repeats // 4), 1)
        say(f"torch loop of {K} iterations     call {pct(ev)}")
        same = all(torch.equal(x, y) for x, y in zip(ref, (o.steps_to_end, o.end_ante, o.end_flags, o.returns)))
        say(f"  the loop's four outputs equal the kernel's: {same}")
        del ref
        weights_all = (o.end_ante >= 5).float()   # [K, N]: the outcome of the step taken from observation record t stands at t
        for m in sorted({N, 4096}, reverse=True):
            if m > N:
                continue
            logits = (torch.randn((m, 60), device="cuda") * 2.0).requires_grad_(True)
            obs = store[:K].view(-1, STRIDE)[:m]
            act = store[1:].view(-1, STRIDE)[:m, 172:176].view(torch.int32)[:, 0]
            w = weights_all.view(-1)[:m].contiguous()

            def ours():
                logits.grad = None
                loss, st = bc_loss(logits, act, obs, weights=w, ent_coef=0.01)
                loss.backward()
                return loss, st

            def composite():
                logits.grad = None
                valid = obs[:, 176:236] != 0
                a = act.long()
                logp = F.log_softmax(logits.masked_fill(~valid, float("-inf")), dim=-1)
                lp = logp.gather(1, a[:, None])[:, 0]
                p = logp.exp()
                ent = -(p * torch.where(p > 0, logp, torch.zeros_like(logp))).sum(-1)
                W = w.sum()
                loss = (-(lp * w).sum() - 0.01 * (ent * w).sum()) / W
                loss.backward()
                return loss

            def two_launch():
                logits.grad = None
                dense = act.contiguous()
                olp, _ = evaluate_actions(logits.detach(), dense, obs)
                loss, st = ppo_loss(logits, dense, olp, w, obs, ent_coef=0.01, normalize_advantage=False)
                loss.backward()
                return loss

            ker = [bc_loss(logits.detach(), act, obs, weights=w, ent_coef=0.01, timing=True)[1].kernel_ms for _ in range(args.warmup + args.repeats)][args.warmup:]
            ev, (loss, st) = timed(torch, ours, args.repeats, args.warmup)
            g_ours = logits.grad.clone()
            say(f"bc_loss + backward, m = {m:<6}   kernel {pct(ker)}   call {pct(ev)}   loss {float(loss.detach()):.6f} accuracy {float(st.accuracy):.4f} "
                f"weight_sum {float(st.weight_sum):.0f} excluded {int(st.excluded)}")
            ev, closs = timed(torch, composite, args.repeats, args.warmup)
            say(f"torch composite + backward        call {pct(ev)}   loss {float(closs.detach()):.6f}   largest |gradient difference| {float((logits.grad - g_ours).abs().max()):.3e}")
            ev, _ = timed(torch, two_launch, args.repeats, args.warmup)
            say(f"evaluate_actions + ppo_loss       call {pct(ev)}   (its loss value is a constant and its divisor m: the gradient differs by W / m)")
        del store, rows, o, weights_all
        torch.cuda.empty_cache()
    say()
    say("== the neighbours: contiguous medians of gae_rows and ppo_loss, kernel / whole call")
    res = [("this library", neighbours(torch, args.repeats, args.warmup))]
    if args.baseline_root:
        env = dict(os.environ, BC_ROWS_PACKAGE_ROOT=os.path.abspath(args.baseline_root))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--neighbours-only", "--repeats", str(args.repeats), "--warmup", str(args.warmup)],
                           env=env, capture_output=True, text=True, timeout=600)
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("NEIGHBOURS ")]
        if r.returncode != 0 or not got:
            say(f"baseline checkout: the child process failed ({r.returncode}): {r.stderr[-400:]}")
        else:
            res.append(("baseline checkout", json.loads(got[0][len("NEIGHBOURS "):])))
    for name, d in res:
        say(f"{name}: signature {d['signature']} ({os.path.basename(d['library'])})")
        for k, v in d.items():
            if isinstance(v, dict):
                say(f"  {k:<24} kernel {v['kernel']}   call {v['event']}")
    if args.notes and os.path.exists(args.notes):
        say()
        lines.extend(open(args.notes).read().rstrip("\n").split("\n"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
