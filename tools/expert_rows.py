#!/usr/bin/env python3
"""What does bg_expert_actions cost, which lane mapping should it use, and what does it cost beside the calls it stands next to?

Records: N envs (scorer jokers, auto-reset) run bg_rollout_rows under BG_POLICY_UNIFORM into a [K, N] store at stride 384 -- K = 100 for the relabel
shape, the last of 20 steps for the K = 1 shapes -- so the store holds what a learner's own early states look like: selections in arbitrary states,
shops, boss blinds.  The share of play-phase records (the ones that pay for the subset search) is printed.  Per shape, in a child process of its own
(p10 / median / p90 after warm-up):
  the mappings   bg_expert_actions_ex with lanes_per_record 1 (one lane per record, the plain walk of the masks), 8 and 64 (a lane group per record,
                 the masks dealt across its lanes, the argmax by __shfl_xor): kernel time by the library's own kernel_ms_out (device events around
                 the launch), the three alternating within each repeat; all three give the same bytes (checked)
  the call       expert_actions(rows) with the library's choice: the whole Python call by device events
      against    sample_actions(zero logits, rows) on the same records: the head the call replaces in a collection loop
      against    one env.step() of N envs (bg_step_rows; the K = 1 shapes): what share of a collection step the expert is
      against    a torch composite that yields the same actions (einsum histograms over a [218, 8] membership table, argmax, argsort), in chunks of
                 65 536 records; its actions are compared with the call's
  the crossovers kernel medians of the three mappings and of the library's choice at m = 1 024 .. 1 048 576 records of one store, in one process: where
                 bg_expert_lanes' thresholds sit
      against    bg_bench_copy in the same process: bytes per second of records read (352 per record; play-phase records read every line) beside
                 what a plain copy sustains -- which says whether the kernel is bound by instructions or by bandwidth
A child process that fails -- a non-zero exit, no result line, its time limit -- ends the run: what was gathered is written, the exit status is 1 and
nothing more is started on the GPU.  --notes FILE is appended verbatim (the compiler's resource lines, tools/isa_diff.py's finding, the CPU closed-loop
totals of tests/test_expert_rows_host.py)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STRIDE = 384
SHAPES = {"4096x1": (4096, 1), "65536x1": (65536, 1), "65536x100": (65536, 100)}
LANES = (1, 8, 64)
CHUNK = 65536


def pct(xs):
    a = np.sort(np.asarray(xs, np.float64))
    return f"{a[int(0.1 * (len(a) - 1))]:.4f} {np.median(a):.4f} {a[int(round(0.9 * (len(a) - 1)))]:.4f}"


def timed(torch, fn, repeats, warmup):
    ms = []
    for r in range(warmup + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if r >= warmup:
            ms.append(a.elapsed_time(b))
    return ms


# ---------------------------------------------------------------------------------------------------------------- the torch composite
def _tables(torch, dev):
    masks = [m for m in range(1, 256) if bin(m).count("1") <= 5]
    M = torch.tensor([[(m >> i) & 1 for i in range(8)] for m in masks], dtype=torch.bool, device=dev)   # [218, 8], ascending mask value
    bc = torch.tensor([5, 10, 20, 30, 30, 35, 40, 60, 100], device=dev)
    bm = torch.tensor([1, 2, 2, 3, 4, 4, 4, 7, 8], device=dev)
    fb = torch.tensor([45, 46, 47, 31, 55, 0] + list(range(1, 60)), device=dev)
    return M, torch.tensor(masks, device=dev), bc, bm, fb


def _first(torch, x):
    return x.to(torch.uint8).argmax(1)


def torch_expert(torch, rows, T):
    """The rule of csrc/bg_expert.h in torch ops over rows uint8 [m, stride] -> int64 [m] actions."""
    M, mval, bc, bm, fb = T
    m = rows.shape[0]
    i8 = rows.view(torch.int8)
    mask = rows[:, 176:236] != 0
    phase = i8[:, 339].long()
    hand = i8[:, 310:318].long()
    sel = rows[:, 0:64].view(torch.int64) != 0
    down = rows[:, 64:128].view(torch.int64) != 0
    levels = i8[:, 318:330].long().clamp(1, 15)
    live = (hand >= 0) & (hand <= 51)
    up = live & ~down
    V = torch.where(up.any(1, keepdim=True), up, live)
    rank, suit = (hand >> 2).clamp(0, 12), hand & 3
    r2 = rank + 2
    chips = torch.where(r2 <= 10, r2, torch.where(r2 == 14, torch.full_like(r2, 11), torch.full_like(r2, 10)))
    Mf = M.float()
    valid = ~((M[None] & ~V[:, None]).any(-1))                                   # [m, 218]: the subset lies within V
    roh = torch.nn.functional.one_hot(rank, 13).float() * live[..., None]
    soh = torch.nn.functional.one_hot(suit, 4).float() * live[..., None]
    hist = torch.einsum("sk,mkr->msr", Mf, roh)
    suits = torch.einsum("sk,mkr->msr", Mf, soh)
    n = M.sum(1)[None]                                                           # [1, 218]
    top = hist.topk(2, dim=-1).values
    c0, c1 = top[..., 0], top[..., 1]
    flush = ((suits > 0).sum(-1) == 1) & (n >= 5)
    pres = hist > 0
    run = torch.stack([pres[..., i:i + 5].all(-1) for i in range(9)], -1).any(-1) | (pres[..., 12] & pres[..., :4].all(-1))
    straight = run & (n >= 5)
    ht = torch.zeros_like(c0, dtype=torch.long)
    for cond, t in ((c0 == 2, 1), ((c0 == 2) & (c1 == 2), 2), (c0 == 3, 3), (straight, 4), (flush, 5), ((c0 == 3) & (c1 == 2), 6), (c0 == 4, 7), (straight & flush, 8)):
        ht = torch.where(cond, torch.full_like(ht, t), ht)
    L = levels.gather(1, ht)
    value = (bc[ht] + (L - 1) * 10 + torch.einsum("sk,mk->ms", Mf, chips.float()).long()) * (bm[ht] + L - 1)
    key = value * 2048 + (5 - n) * 256 + (255 - mval)[None]
    key = torch.where(valid, key, torch.full_like(key, -1))
    best = key.argmax(1)
    P = M[best]
    valueP = value.gather(1, best[:, None])[:, 0]
    needed = rows[:, 156:160].view(torch.int32)[:, 0].long()
    scored = rows[:, 144:148].view(torch.int32)[:, 0].long()
    remaining = (needed - scored).clamp(min=0)
    hl, dl = i8[:, 333].long(), i8[:, 334].long()
    play = (dl <= 0) | (hl <= 1) | (valueP * hl >= remaining) | ~(live & ~P).any(1)
    cand = live & ~P
    kd = torch.where(cand, chips * 8 + torch.arange(8, device=rows.device)[None], torch.full_like(chips, 1 << 20))
    pos = torch.empty_like(kd).scatter_(1, kd.argsort(1), torch.arange(8, device=rows.device)[None].expand(m, 8))
    D = cand & (pos < 5)
    Tm = torch.where(play[:, None], P, D)
    off, on = sel & ~Tm, Tm & ~sel
    a0 = torch.where(off.any(1), 2 + _first(torch, off), torch.where(on.any(1), 2 + _first(torch, on), (~play).long()))
    a0 = torch.where(live.any(1), a0, torch.full_like(a0, -1))
    b = mask[:, 45:48]
    a2 = torch.where(b.any(1), 45 + _first(torch, b), torch.full_like(a0, -1))
    items, costs = rows[:, 256:276].view(torch.int16).long(), rows[:, 276:296].view(torch.int16).long()
    cj = (items == 3) & mask[:, 20:30]
    ks = torch.where(cj, costs * 16 + torch.arange(10, device=rows.device)[None], torch.full_like(costs, 1 << 30))
    a1 = torch.where(cj.any(1), 20 + ks.argmin(1), torch.full_like(a0, 31))
    a = torch.where(phase == 0, a0, torch.where(phase == 1, a1, torch.where(phase == 2, a2, torch.where(phase == 3, torch.full_like(a0, 55), torch.full_like(a0, -1)))))
    ok = (a >= 0) & mask.gather(1, a.clamp(min=0)[:, None])[:, 0]
    fm = mask[:, fb]
    fa = torch.where(fm.any(1), fb[_first(torch, fm)], torch.full_like(a0, -1))
    return torch.where(ok, a, fa)


def torch_expert_chunked(torch, rows, T, out):
    flat = rows.reshape(-1, rows.shape[-1])
    for s in range(0, flat.shape[0], CHUNK):
        out[s:s + CHUNK] = torch_expert(torch, flat[s:s + CHUNK], T)
    return out


# ---------------------------------------------------------------------------------------------------------------- one shape, one process
def child(name, repeats, warmup):
    import torch
    from balatro_gym_amd import BalatroVecEnv, _native as nat, expert_actions, sample_actions
    from balatro_gym_amd.vec_env import RowBuffers
    N, K = SHAPES[name]
    env = BalatroVecEnv(N, [31000 + i for i in range(N)], scorer_jokers=True, autoreset=True, obs_layout="rows")
    dev = env.device
    steps = K if K > 1 else 20
    rb = RowBuffers(N, dev, steps=steps, row_stride=STRIDE)
    env.rollout(steps, policy=nat.POLICY_UNIFORM, policy_seed=3, obs_buffers=rb)
    env.check()
    rows = rb.rows if K > 1 else rb.rows[steps - 1:steps]
    rows = rows.contiguous()
    m = N * K
    res = {"shape": name, "records": m, "play_share": float((rows[:, :, 339] == 0).float().mean())}
    out = {g: torch.empty((K, N), dtype=torch.int32, device=dev) for g in LANES}
    det = {g: torch.empty((K, N), dtype=torch.int32, device=dev) for g in LANES}
    kernel = {g: [] for g in LANES}
    for r in range(warmup + repeats):
        for g in LANES:
            ms = expert_actions(rows, out=out[g], detail=det[g], lanes=g, timing=True)[-1]
            if r >= warmup:
                kernel[g].append(ms)
    res["same_bytes"] = all(torch.equal(out[g], out[1]) and torch.equal(det[g], det[1]) for g in LANES)
    for g in LANES:
        res[f"kernel_lanes{g}"] = pct(kernel[g])
    a = torch.empty((K, N), dtype=torch.int32, device=dev)
    res["kernel_default_no_detail"] = pct([expert_actions(rows, out=a, timing=True)[-1] for _ in range(warmup + repeats)][warmup:])
    res["call"] = pct(timed(torch, lambda: expert_actions(rows, out=a), repeats, warmup))
    med = float(res["kernel_default_no_detail"].split()[1])
    res["records_gbps"] = m * 352 / (med * 1e-3) / 1e9
    logits = torch.zeros((K, N, 60), device=dev)
    sa = torch.empty((K, N), dtype=torch.int32, device=dev)
    res["sample_actions_call"] = pct(timed(torch, lambda: sample_actions(logits, rows, seed=1, t=0, actions=sa), repeats, warmup))
    res["sample_actions_kernel"] = pct([sample_actions(logits, rows, seed=1, t=0, actions=sa, timing=True)[-1] for _ in range(warmup + repeats)][warmup:])
    if K == 1:
        zeros = torch.zeros(N, dtype=torch.int32, device=dev)   # PLAY_HAND with whatever is selected: valid or not, one bg_step_rows launch either way
        res["step_rows_call"] = pct(timed(torch, lambda: env.step(zeros), repeats, warmup))
        res["expert_act_call"] = pct(timed(torch, lambda: env.expert_act(out=a[0]), repeats, warmup))
    T = _tables(torch, dev)
    ta = torch.empty(m, dtype=torch.int64, device=dev)
    comp_rep = max(3, repeats // 10) if K > 1 else repeats
    res["torch_composite_call"] = pct(timed(torch, lambda: torch_expert_chunked(torch, rows, T, ta), comp_rep, 2))
    res["torch_composite_equal_share"] = float((ta == out[1].reshape(-1).long()).float().mean())
    L = nat.load()
    nbytes = min(m * STRIDE, 1 << 30) // 16 * 16
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    gbps = C.c_double(0.0)
    rc = L.bg_bench_copy(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), C.c_uint64(nbytes), 20, C.byref(gbps), None)
    res["copy_gbps_read_plus_written"] = gbps.value if rc == 0 else None
    res["copy_bytes"] = nbytes
    env.close()
    print("RESULT " + json.dumps(res), flush=True)


SWEEP = (1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072, 262144, 524288, 1048576)


def sweep(repeats, warmup):
    """Where the three mappings cross: kernel medians at m records of one store, the mappings (and the library's choice, lanes 0) alternating."""
    import torch
    from balatro_gym_amd import BalatroVecEnv, _native as nat, expert_actions
    from balatro_gym_amd.vec_env import RowBuffers
    N, steps = 65536, 16
    env = BalatroVecEnv(N, [31000 + i for i in range(N)], scorer_jokers=True, autoreset=True, obs_layout="rows")
    rb = RowBuffers(N, env.device, steps=steps, row_stride=STRIDE)
    env.rollout(steps, policy=nat.POLICY_UNIFORM, policy_seed=3, obs_buffers=rb)
    env.check()
    flat = rb.rows.reshape(-1, STRIDE).flip(0).contiguous()   # (the last steps first: the first step of a rollout is all blind select)
    res = {}
    for m in SWEEP:
        rows = flat[:m]
        out = torch.empty(m, dtype=torch.int32, device=env.device)
        ms = {g: [] for g in (0,) + LANES}
        for r in range(warmup + repeats):
            for g in ms:
                t = expert_actions(rows, out=out, lanes=g, timing=True)[-1]
                if r >= warmup:
                    ms[g].append(t)
        res[m] = {str(g): float(np.median(v)) for g, v in ms.items()}
        res[m]["play_share"] = float((rows[:, 339] == 0).float().mean())
    env.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", default=None)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expert_rows.txt"))
    ap.add_argument("--notes", default=None)
    ap.add_argument("--timeout", type=int, default=420)
    args = ap.parse_args()
    if args.child == "sweep":
        sweep(args.repeats, args.warmup)
        return 0
    if args.child:
        child(args.child, args.repeats, args.warmup)
        return 0
    lines = [f"tools/expert_rows.py --repeats {args.repeats} --warmup {args.warmup}: milliseconds as p10 median p90, each shape in a process of its own", ""]
    status = 0
    for name in args.shapes.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--repeats", str(args.repeats), "--warmup", str(args.warmup)],
                               capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            lines.append(f"{name}: the child process ran into its time limit of {args.timeout} s: stopped here")
            status = 1
            break
        got = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not got:
            lines.append(f"{name}: the child process failed (exit {p.returncode}): stopped here\n{p.stderr[-2000:]}")
            status = 1
            break
        r = json.loads(got[-1][7:])
        lines.append(f"{name}: {r['records']} records at stride {STRIDE}, {100 * r['play_share']:.1f} % in the play phase; the three mappings give the same bytes: {r['same_bytes']}")
        for g in LANES:
            lines.append(f"  kernel, {g:2d} lane(s) per record, with detail      {r[f'kernel_lanes{g}']}")
        lines.append(f"  kernel, the library's choice, without detail   {r['kernel_default_no_detail']}   = {r['records_gbps']:.0f} GB/s of records read")
        lines.append(f"  expert_actions, whole call                     {r['call']}")
        lines.append(f"  sample_actions on the same records: kernel     {r['sample_actions_kernel']}")
        lines.append(f"  sample_actions, whole call                     {r['sample_actions_call']}")
        if "step_rows_call" in r:
            lines.append(f"  env.step() (bg_step_rows), whole call          {r['step_rows_call']}")
            lines.append(f"  env.expert_act(), whole call                   {r['expert_act_call']}")
        lines.append(f"  torch composite, whole call                    {r['torch_composite_call']}   (actions equal to the kernel's on {100 * r['torch_composite_equal_share']:.3f} % of the records)")
        if r["copy_gbps_read_plus_written"]:
            lines.append(f"  bg_bench_copy of {r['copy_bytes'] / 1e6:.0f} MB in the same process: {r['copy_gbps_read_plus_written']:.0f} GB/s read + written")
        lines.append("")
    if status == 0:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "sweep", "--repeats", str(args.repeats), "--warmup", str(args.warmup)],
                               capture_output=True, text=True, timeout=args.timeout)
            got = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        except subprocess.TimeoutExpired:
            p, got = None, []
        if not got:
            lines.append(f"sweep: the child process failed or ran into its time limit: stopped here\n{p.stderr[-2000:] if p else ''}")
            status = 1
        else:
            r = json.loads(got[-1][7:])
            lines.append("where the mappings cross: kernel medians (no detail) at m records, ms; `choice` is lanes 0 = bg_expert_lanes(m)")
            lines.append("        m    1 lane   8 lanes  64 lanes    choice   play share")
            for m, v in r.items():
                lines.append(f"{int(m):9d}  {v['1']:8.4f}  {v['8']:8.4f}  {v['64']:8.4f}  {v['0']:8.4f}   {100 * v['play_share']:.1f} %")
            lines.append("")
    if args.notes and os.path.exists(args.notes):
        lines.append(open(args.notes).read().rstrip())
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return status


if __name__ == "__main__":
    sys.exit(main())
