#!/usr/bin/env python3
"""What do the fused actor calls (actor_sample / actor_ppo_loss: bg_actor_sample, bg_actor_ppo_loss) cost beside the composite a user writes without them
on the same commit?  Writes profiles/actor_rows.txt (--out).

One process.  65 536 envs (set up as bench.py's) are run 64 steps and then 4 more into a RowBuffers at stride 384; the last step's records give the
masks.  h ~ N(0, 1) bfloat16 [m, Hin], weight ~ N(0, 4 / Hin) float32 [60, Hin], bias N(0, 1); m = 4 096 and 65 536, Hin = 256 and 512; actions are drawn
by the head under the records' masks, old_log_prob is their log-prob plus N(0, 0.15^2), advantages / values / returns N(0, 1); clip_range 0.2, ent_coef
0.01, vf_coef 0.5, advantages normalised.  The ways alternate repeat by repeat in the same process:
  collect   ours       actor_sample(h, weight, bias, rows, seed=, t=)                                                  one launch
            composite  logits = F.linear(h, w_bf16, b_bf16); sample_actions(logits, rows, seed=, t=)                      a GEMM and a launch
  train     ours       loss, _ = actor_ppo_loss(h, weight, bias, ...); loss.backward()      -> h.grad, weight.grad, bias.grad, values.grad
            composite  logits = F.linear(h, w_bf16, b_bf16); loss, _ = ppo_loss(logits, ...); loss.backward()   -> the same leaves (bfloat16 parameters)
"kernel" is the library's own kernel_ms_out (ours: every launch of the call; composite: the head / loss launches alone), "call" device events around
the whole Python call (p10 / median / p90 after warm-up).  Before timing, ours is compared with the same arithmetic in torch on its own logits (logits,
dh, dweight to 1e-4 of the largest element) and its loss with the composite's: the composite rounds its logits to bfloat16, which moves rows across the
clip boundary, so its gradient is not comparable row by row (the claims rest on tests/test_actor_rows.py).

--base-only --lib PATH: bg_ppo_loss' and bg_sample_actions' own kernel medians (float32 logits, masked, m = 4 096 and 65 536) through the C ABI of the
library at PATH: run on the parent commit's library and on this one to see that the kernels beside the new header did not move."""
import argparse
import ctypes as C
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
    ap.add_argument("--repeats", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--widths", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--base-only", action="store_true")
    ap.add_argument("--lib", default=None, help="--base-only: the library to measure (default: the tree's)")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actor_rows.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("actor_rows.py: no GPU is visible", file=sys.stderr)
        return 2
    import bench
    from balatro_gym_amd import BalatroVecEnv, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    N = max(args.batches)
    env = BalatroVecEnv(N, [1000 + g for g in range(N)], device=0, scorer_jokers=True, autoreset=True, max_ante=bench.MAX_ANTE, fused_steps=64)
    env.inject(jokers=[bench.jokers_for(g) for g in range(N)], apply_now=True)
    env.rollout(64, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED, obs_buffers=RowBuffers(N, dev, steps=1))
    rb = RowBuffers(N, dev, steps=4, row_stride=nat.ROW_STRIDE_LINES)
    env.rollout(4, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED + 1, obs_buffers=rb)
    env.check()
    env.close()
    records = rb.rows[-1]

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
        """ways: name -> (call returning kernel ms or None, call to put between events) -> name -> (kernel ms list, event ms list)"""
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

    g = torch.Generator(device=dev).manual_seed(7)

    if args.base_only:
        path = args.lib or nat.lib_path()
        L = C.CDLL(path)
        vp, u64, i64, f32 = C.c_void_p, C.c_uint64, C.c_int64, C.c_float
        L.bg_sample_actions.argtypes = [vp, C.c_int, u64, vp, u64, i64, C.c_uint32, u64, u64, u64, vp, vp, vp, C.POINTER(f32), vp]
        L.bg_ppo_loss_workspace_bytes.restype = u64
        L.bg_ppo_loss_workspace_bytes.argtypes = [i64]
        L.bg_ppo_loss.argtypes = [vp, C.c_int, u64, vp, u64, vp, vp, vp, vp, vp, vp, i64, i64, f32, f32, f32, C.c_uint32, vp, u64, vp, vp, vp, vp, vp, u64, C.POINTER(f32), vp]
        say(f"[{args.label or os.path.basename(path)}] library {os.path.basename(path)} signature {nat.device_code_signature(path)}  GPU {torch.cuda.get_device_name(0)}; "
            f"float32 logits N(0, 4), masks from records; {args.repeats} repeats after {args.warmup} warm-up; kernel ms p10 median p90")
        for m in args.batches:
            logits = torch.randn((m, 60), generator=g, device=dev) * 2.0
            mask = records[:m]
            acts = torch.empty(m, dtype=torch.int32, device=dev)
            lp, en, dv = (torch.empty(m, device=dev) for _ in range(3))
            adv, ret, val = (torch.randn(m, generator=g, device=dev) for _ in range(3))
            dl = torch.empty((m, 60), device=dev)
            st = torch.empty(10, device=dev)
            ws = torch.empty(int(L.bg_ppo_loss_workspace_bytes(m)), dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream().cuda_stream
            ms = f32(0.0)

            def sample():
                rc = L.bg_sample_actions(logits.data_ptr(), 0, 60, mask.data_ptr() + 176, 384, m, 0, SEED, 0, T, acts.data_ptr(), lp.data_ptr(), en.data_ptr(), C.byref(ms), stream)
                assert rc == 0
                return float(ms.value)
            sample()
            old = lp + 0.15 * torch.randn(m, generator=g, device=dev)
            old = torch.where(torch.isfinite(old), old, torch.zeros_like(old))

            def loss():
                rc = L.bg_ppo_loss(logits.data_ptr(), 0, 60, mask.data_ptr() + 176, 384, acts.data_ptr(), old.data_ptr(), adv.data_ptr(), val.data_ptr(), ret.data_ptr(), None, m, m,
                                   CLIP, ENT, VF, 1, dl.data_ptr(), 60, dv.data_ptr(), lp.data_ptr(), en.data_ptr(), st.data_ptr(), ws.data_ptr(), ws.numel(), C.byref(ms), stream)
                assert rc == 0
                return float(ms.value)
            ks, kl = [], []
            for i in range(args.warmup + args.repeats):
                a, b = sample(), loss()
                if i >= args.warmup:
                    ks.append(a)
                    kl.append(b)
            say(f"  m {m:>6} | bg_sample_actions {pct(ks)} | bg_ppo_loss {pct(kl)}")
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
        return 0

    from balatro_gym_amd import actor_ppo_loss, actor_sample, ppo_loss, sample_actions
    say(f"build signature {nat.device_code_signature()}  library {os.path.basename(nat.lib_path())}  GPU {torch.cuda.get_device_name(0)}")
    say(f"h N(0, 1) bfloat16, weight N(0, 4 / Hin) float32, masks from records at stride 384; clip {CLIP} ent_coef {ENT} vf_coef {VF}, advantages normalised; "
        f"{args.repeats} repeats after {args.warmup} warm-up, the ways alternating; device events; ms")
    say(f"{'pass':>8} {'m':>6} {'Hin':>5} | {'ours kernel':>11} {'call p10':>9} {'median':>8} {'p90':>8} | {'composite head/loss kernel':>26} {'call p10':>9} {'median':>8} {'p90':>8} | composite / ours (call medians)")
    lost = []
    for m in args.batches:
        mask = records[:m]
        for Hin in args.widths:
            h = torch.randn((m, Hin), generator=g, device=dev).to(torch.bfloat16)
            w = (torch.randn((60, Hin), generator=g, device=dev) * 2.0 / Hin ** 0.5)
            b = torch.randn(60, generator=g, device=dev)
            w16, b16 = w.to(torch.bfloat16), b.to(torch.bfloat16)
            acts, lp, _ = actor_sample(h, w, b, mask, seed=SEED, t=T)
            old = lp + 0.15 * torch.randn(m, generator=g, device=dev)
            old = torch.where(torch.isfinite(old), old, torch.zeros_like(old))
            adv, ret = (torch.randn(m, generator=g, device=dev) for _ in range(2))
            hp, vp_ = h.clone().requires_grad_(True), torch.randn(m, generator=g, device=dev).requires_grad_(True)
            wp, bp = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
            w16p, b16p = w16.clone().requires_grad_(True), b16.clone().requires_grad_(True)
            kw = dict(values=vp_, returns=ret, clip_range=CLIP, ent_coef=ENT, vf_coef=VF)

            def zero():
                for p in (hp, vp_, wp, bp, w16p, b16p):
                    p.grad = None

            def ours_train(timing=False):
                zero()
                loss, st = actor_ppo_loss(hp, wp, bp, acts, old, adv, mask, timing=timing, **kw)
                loss.backward()
                return st.kernel_ms if timing else loss.detach()

            def comp_train(timing=False):
                zero()
                loss, st = ppo_loss(F.linear(hp, w16p, b16p), acts, old, adv, mask, timing=timing, **kw)
                loss.backward()
                return st.kernel_ms if timing else loss.detach()

            def ours_collect(timing=False):
                r = actor_sample(h, w, b, mask, seed=SEED, t=T, timing=timing)
                return r[3] if timing else r

            def comp_collect(timing=False):
                r = sample_actions(F.linear(h, w16, b16), mask, seed=SEED, t=T, timing=timing)
                return r[3] if timing else r

            # ours against the same arithmetic in torch on ITS logits (the composite's logits are rounded to bfloat16, which moves rows across the clip
            # boundary: its gradient is not comparable row by row), and the two losses against each other
            lg, dlg = torch.empty((m, 60), device=dev), torch.empty((m, 60), device=dev)
            loss_o, st = actor_ppo_loss(h, w, b, acts, old, adv, mask, values=vp_.detach(), returns=ret, clip_range=CLIP, ent_coef=ENT, vf_coef=VF,
                                        dh_dtype=torch.float32, logits_out=lg, dlogits_out=dlg)
            dp = dlg.to(torch.bfloat16).float()
            rel = lambda x, y: float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))   # noqa: E731
            r_lg, r_dh, r_dw = rel(lg, F.linear(h.float(), w16.float(), b)), rel(st.dh, dp @ w16.float()), rel(st.dweight, dp.T @ h.float())
            lo, lc = float(loss_o), float(comp_train())
            if max(r_lg, r_dh, r_dw) > 1e-4 or abs(lo - lc) > 2e-2 * max(1.0, abs(lc)):
                say(f"m {m} Hin {Hin}: ours differs from torch on its own logits: logits {r_lg:.3g}, dh {r_dh:.3g}, dweight {r_dw:.3g} (relative to the largest "
                    f"element); loss {lo} vs the composite's {lc}")
                return 1
            del lg, dlg, dp, st
            for name, ours, comp in (("collect", ours_collect, comp_collect), ("train", ours_train, comp_train)):
                res = run({"ours": (lambda: ours(True), ours), "composite": (lambda: comp(True), comp)})
                o, c = res["ours"], res["composite"]
                ratio = np.median(c[1]) / np.median(o[1])
                say(f"{name:>8} {m:>6} {Hin:>5} | {np.median(o[0]):>11.4f} {pct(o[1])} | {np.median(c[0]):>26.4f} {pct(c[1])} | {ratio:>6.2f}x")
                if ratio < 1.0:
                    lost.append(f"  {name} m {m} Hin {Hin}: ours {np.median(o[1]):.4f} ms, composite {np.median(c[1]):.4f} ms")
            zero()
    say(f"ours faster than the composite (whole call) in every shape: {'NO' if lost else 'yes'}")
    for s in lost:
        say(s)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
