#!/usr/bin/env python3
"""What do bg_gae_rows (vec_env.gae_rows) and bg_episode_stats_rows (vec_env.EpisodeStats) cost beside the torch composite a user writes without them?

One process.  65 536 envs (BASELINE configs[2], as bench.py sets them up) and 4 096 envs are run 400 steps, then roll out 100 steps into a RowBuffers at
stride 384; the same record bytes are also laid out at stride 352.  Shapes: 65 536 x {20, 100} and 4 096 x 100, both strides.  Two ways alternate repeat by
repeat in the same process, each timed by device events around the call (>= 20 repeats after warm-up; p10 / median / p90):
  new       gae_rows(rows, values, last_values, 0.99, 0.95, advantages=, returns=) / EpisodeStats.update(rows, ep_return=, ep_len=): one launch each
  baseline  what exists without them: `rb.reward.float()`, `rb.terminated.float()` (strided views of the records) and SB3's reversed loop over the K steps
            with torch operations on [N] device tensors; for the episode statistics the forward loop with torch.where and a float64 carry
Before timing, the baseline's advantages are compared with the kernel's: torch's GPU arithmetic may contract a multiply-add, so the count of differing
elements and the largest difference relative to the largest |advantage| are printed and held to float32 rounding; the bit-exact claim rests on the numpy
comparison in tests/test_gae_rows.py, not on this.  The episode statistics (float64 additions in the same order) must be equal.
When tools/micro/libgae_variants.so is built (tools/micro/gae_variants.hip: the LDS-tile shape of both kernels), those kernels are the A/B partners: each
must give the library kernel's bits and is timed in the same alternation -- both sides of the A/B through bare C calls, so that neither carries the
Python wrapper's argument checks between its events.
"Share of a measured copy": bytes over the median time, over what bg_bench_copy reaches in the same process -- with bytes = what the shapes make
unavoidable at the HBM's 64-byte sector: two sectors per record (reward; terminated byte) plus the dense arrays read and written.  What is actually
fetched per record (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, one run each) is not measured by this tool."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VARIANTS_LIB = os.path.join(ROOT, "tools", "micro", "libgae_variants.so")
GAMMA, LAMBDA = 0.99, 0.95


def records(n, T, dev):
    """[T, n] records at stride 384 of a real rollout after 400 steps of warm-up, and the same bytes at stride 352."""
    import bench
    from balatro_gym_amd import BalatroVecEnv, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers
    env = BalatroVecEnv(n, [1000 + g for g in range(n)], device=0, scorer_jokers=True, autoreset=True, max_ante=bench.MAX_ANTE, fused_steps=T)
    env.inject(jokers=[bench.jokers_for(g) for g in range(n)], apply_now=True)
    env.rollout(400, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED, obs_buffers=RowBuffers(n, dev, steps=1))
    rb = RowBuffers(n, dev, steps=T, row_stride=nat.ROW_STRIDE_LINES)
    env.rollout(T, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED + 1, obs_buffers=rb)
    st = env.stats()
    env.close()
    rb352 = RowBuffers(n, dev, steps=T, row_stride=nat.ROW_BYTES)
    rb352.rows.copy_(rb.rows[:, :, :nat.ROW_BYTES])
    return {384: rb, 352: rb352}, st


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("gae_rows.py: no GPU is visible", file=sys.stderr)
        return 2
    import bench
    from balatro_gym_amd import EpisodeStats, gae_rows, _native as nat
    dev = torch.device("cuda:0")
    copy_gbps, fill_gbps = bench.measured_copy_gbps(dev)
    part = C.CDLL(VARIANTS_LIB) if os.path.exists(VARIANTS_LIB) else None
    if part:
        part.gae_tiles.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        part.eps_tiles.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L = nat.load()
    print(f"build signature {nat.device_code_signature()}  library {os.path.basename(nat.lib_path())}  GPU {torch.cuda.get_device_name(0)}")
    print(f"bg_bench_copy {copy_gbps:.0f} GB/s (read + written), bg_bench_fill {fill_gbps:.0f} GB/s; gamma {GAMMA} gae_lambda {LAMBDA}; {args.repeats} repeats after "
          f"{args.warmup} warm-up, device events, new / baseline" + (" / A/B pair" if part else "") + " alternating")

    def base_gae(rb, K, values, last_values):
        rewards, dones = rb.reward[:K].float(), rb.terminated[:K].float()
        adv = torch.empty_like(values)
        last = 0
        for step in reversed(range(K)):
            nnt = 1.0 - dones[step]   # = 1 - episode_starts[step + 1]; for the last step 1 - dones
            nv = last_values if step == K - 1 else values[step + 1]
            delta = rewards[step] + GAMMA * nv * nnt - values[step]
            last = delta + GAMMA * LAMBDA * nnt * last
            adv[step] = last
        return adv, adv + values

    def base_eps(rb, K, cr, cl):
        reward, term = rb.reward[:K], rb.terminated[:K]
        n = reward.shape[1]
        er, el = torch.empty((K, n), dtype=torch.float64, device=dev), torch.empty((K, n), dtype=torch.int32, device=dev)
        for t in range(K):
            cr = cr + reward[t]
            cl = cl + 1
            d = term[t] != 0
            er[t] = torch.where(d, cr, 0.0)
            el[t] = torch.where(d, cl, 0)
            cr = torch.where(d, 0.0, cr)
            cl = torch.where(d, 0, cl)
        return er, el, cr, cl

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        del r
        return a.elapsed_time(b)

    def pct(x):
        return np.percentile(x, 10), np.median(x), np.percentile(x, 90)

    hdr = (f"{'op':>8} {'envs':>6} {'steps':>5} {'stride':>6} | {'new p10':>8} {'median':>8} {'p90':>8} ms | {'base p10':>8} {'median':>8} {'p90':>8} ms | {'speed-up':>8} "
           f"{'MB min':>7} {'GB/s':>6} {'share of a measured copy':>24} {'new p90 < base p10':>18}")
    all_ok = True
    ab_lines = []
    for n, shapes in ((65536, (20, 100)), (4096, (100,))):
        T = max(shapes)
        rbs, st = records(n, T, dev)
        print(f"{n} envs: {T} steps of records after 400 steps of warm-up ({st['plays']} plays, {st['episodes']} episodes in the window)")
        print(hdr)
        g = torch.Generator(device=dev).manual_seed(n)
        for K in shapes:
            values, last_values = torch.randn((K, n), device=dev, generator=g), torch.randn(n, device=dev, generator=g)
            adv, ret = torch.empty_like(values), torch.empty_like(values)
            er, el = torch.empty((K, n), dtype=torch.float64, device=dev), torch.empty((K, n), dtype=torch.int32, device=dev)
            for stride in (384, 352):
                rb = rbs[stride]
                rows = rb.rows[:K]
                stats = EpisodeStats(n, dev)
                # ---- the two ways agree
                gae_rows(rows, values, last_values, GAMMA, LAMBDA, advantages=adv, returns=ret)
                ba, br = base_gae(rb, K, values, last_values)
                diff = int((ba.view(torch.int32) != adv.view(torch.int32)).sum().item())
                rel = float(((ba - adv).abs().max() / adv.abs().max()).item())
                print(f"      (gae {n} x {K}, stride {stride}: {diff} of {K * n} advantages differ in bits from the torch composite, largest difference {rel:.2e} of the "
                      f"largest |advantage| {float(adv.abs().max()):.1f})")
                if not rel < 1e-5:
                    print("gae_rows.py: the torch composite and the kernel differ by more than float32 rounding", file=sys.stderr)
                    return 1
                stream = torch.cuda.current_stream(dev).cuda_stream
                if part:
                    la, lr = torch.full_like(adv, -7.0), torch.full_like(ret, -7.0)
                    assert part.gae_tiles(rows.data_ptr(), stride, K, n, values.data_ptr(), last_values.data_ptr(), GAMMA, LAMBDA, la.data_ptr(), lr.data_ptr(), stream) == 0
                    if not (torch.equal(la.view(torch.int32), adv.view(torch.int32)) and torch.equal(lr.view(torch.int32), ret.view(torch.int32))):
                        print("gae_rows.py: the LDS-tile partner differs from the library's GAE kernel", file=sys.stderr)
                        return 1
                stats.reset()
                stats.update(rows, ep_return=er, ep_len=el)
                ber, bel, bcr, bcl = base_eps(rb, K, torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
                if not (torch.equal(ber.view(torch.int64), er.view(torch.int64)) and torch.equal(bel, el) and torch.equal(bcr.view(torch.int64), stats.ep_return_carry.view(torch.int64))
                        and torch.equal(bcl.to(torch.int32), stats.ep_len_carry)):
                    print("gae_rows.py: the torch composite and the episode kernel differ", file=sys.stderr)
                    return 1
                pcr, pcl = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
                if part:
                    per, pel = torch.full_like(er, -7.0), torch.full_like(el, -7)
                    assert part.eps_tiles(rows.data_ptr(), stride, K, n, pcr.data_ptr(), pcl.data_ptr(), per.data_ptr(), pel.data_ptr(), stream) == 0
                    if not (torch.equal(per.view(torch.int64), er.view(torch.int64)) and torch.equal(pel, el) and torch.equal(pcr.view(torch.int64), stats.ep_return_carry.view(torch.int64))
                            and torch.equal(pcl, stats.ep_len_carry)):
                        print("gae_rows.py: the LDS-tile partner differs from the library's episode kernel", file=sys.stderr)
                        return 1
                del ba, br, ber, bel
                zr, zl = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
                ways = {"gae": (lambda: gae_rows(rows, values, last_values, GAMMA, LAMBDA, advantages=adv, returns=ret), lambda: base_gae(rb, K, values, last_values),
                                K * n * (128 + 4 + 8) + n * 4),
                        "episodes": (lambda: stats.update(rows, ep_return=er, ep_len=el), lambda: base_eps(rb, K, zr, zl), K * n * (128 + 12) + n * 24)}
                # the A/B pair: the library's entry point and the partner's, both called bare
                pair = {"gae": (lambda: L.bg_gae_rows(rows.data_ptr(), stride, K, n, values.data_ptr(), last_values.data_ptr(), GAMMA, LAMBDA, adv.data_ptr(), ret.data_ptr(), None, stream),
                                lambda: part.gae_tiles(rows.data_ptr(), stride, K, n, values.data_ptr(), last_values.data_ptr(), GAMMA, LAMBDA, la.data_ptr(), lr.data_ptr(), stream)),
                        "episodes": (lambda: L.bg_episode_stats_rows(rows.data_ptr(), stride, K, n, pcr.data_ptr(), pcl.data_ptr(), er.data_ptr(), el.data_ptr(), None, stream),
                                     lambda: part.eps_tiles(rows.data_ptr(), stride, K, n, pcr.data_ptr(), pcl.data_ptr(), per.data_ptr(), pel.data_ptr(), stream))} if part else {}
                for op, (new, base, nbytes) in ways.items():
                    ab = pair.get(op)
                    for _ in range(args.warmup):
                        timed(new), timed(base)
                        if ab:
                            timed(ab[0]), timed(ab[1])
                    tn, tb, ta, tp = [], [], [], []
                    for _ in range(args.repeats):
                        tn.append(timed(new))
                        tb.append(timed(base))
                        if ab:
                            ta.append(timed(ab[0]))
                            tp.append(timed(ab[1]))
                    n10, n50, n90 = pct(tn)
                    b10, b50, b90 = pct(tb)
                    gbps = nbytes / (n50 * 1e-3) / 1e9
                    ok = n90 < b10
                    all_ok = all_ok and ok
                    print(f"{op:>8} {n:>6} {K:>5} {stride:>6} | {n10:>8.4f} {n50:>8.4f} {n90:>8.4f}    | {b10:>8.3f} {b50:>8.3f} {b90:>8.3f}    | {b50 / n50:>7.1f}x "
                          f"{nbytes / 1e6:>7.1f} {gbps:>6.0f} {gbps / copy_gbps:>24.2f} {'yes' if ok else 'NO':>18}")
                    if ab:
                        a10, a50, a90 = pct(ta)
                        p10, p50, p90 = pct(tp)
                        ab_lines.append(f"{op:>8} {n:>6} {K:>5} {stride:>6} | library (lane = env, 16 steps in registers) {a10:.4f} {a50:.4f} {a90:.4f} ms | partner (LDS tiles) "
                                        f"{p10:.4f} {p50:.4f} {p90:.4f} ms | partner median / library median {p50 / a50:.2f}")
        del rbs, rb, rows
        torch.cuda.empty_cache()
    if ab_lines:
        print("A/B: the library's kernels against the LDS-tile kernels of tools/micro/gae_variants.hip, both through bare C calls (same per-step text, bit-identical "
              "results; p10 median p90):")
        print("\n".join(ab_lines))
    print("new p90 below baseline p10 in every shape: " + ("yes" if all_ok else "NO"))
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
