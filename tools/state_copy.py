"""What bg_copy_states / bg_get_states / bg_set_states cost (csrc/bg_snapshot.h) -> profiles/state_copy.txt.

Two shapes: 65 536 envs with fused_steps=16 (26 KB blobs) and 4 096 envs at full ring depth.  Per shape, alternating repeat by repeat in one process, timed
by device events around the Python call (p10 / median / p90 after warm-up):
  copy   copy_states of the first half of the handle onto the second half      (m = N / 2 envs)
  get    get_states of all envs into a preallocated tensor                     (m = N)
  set    set_states of all envs from it (includes its read-back of 64 bytes per env and the wait for it)
  bench  bg_bench_copy of the same byte count (m blobs), the plain 16-byte-per-lane streaming copy of this library (its rate is its own kernel's)
  copy_b2b / get_b2b   eight calls inside one pair of events, per call: the host's part of a call (checking and uploading the index lists; none for
         get_b2b, which names no envs) then runs beside the previous call's kernel, so this is what the kernel sustains
Each is reported as moved bytes per second, read + written (2 x m x blob bytes over the median), beside the bench copy's.  Then: the 60-way fork as a call
time (device events, and the host's time inside the call); on 64 envs the only way there was before -- a loop of get_state / set_state, by the host's
clock, since it synchronises -- against get_states / set_states of the same 64, per env; and the first 16-step launch after a forced top-up (behind a
set_states of one env) against the same launch without one."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_copy.txt"))
    args = ap.parse_args()
    import torch
    import bench
    from balatro_gym_amd import BalatroVecEnv, _native as nat
    from balatro_gym_amd.vec_env import RowBuffers
    dev = torch.device("cuda:0")
    L = nat.load()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        return a.elapsed_time(b)

    def alternate(ways):
        ms = {k: [] for k in ways}
        for r in range(args.warmup + args.repeats):
            for k, fn in ways.items():
                t = events(fn)
                if r >= args.warmup:
                    ms[k].append(t)
        return {k: np.percentile(v, [10, 50, 90]) for k, v in ms.items()}

    copy_gbps, fill_gbps = bench.measured_copy_gbps(dev)
    say(f"build signature {nat.device_code_signature()}  library {os.path.basename(nat.lib_path())}  GPU {torch.cuda.get_device_name(0)}")
    say(f"bg_bench_copy {copy_gbps:.0f} GB/s at 1 GiB (read + written), bg_bench_fill {fill_gbps:.0f} GB/s; {args.repeats} repeats after {args.warmup} warm-up, "
        f"device events around the call, the ways alternating; ms as p10 median p90; GB/s = 2 x m x blob bytes / median")

    for n, fused, name in ((65536, 16, "65 536 envs, fused_steps=16"), (4096, 0, "4 096 envs, full ring depth")):
        env = BalatroVecEnv(n, [1000 + i for i in range(n)], device=0, fused_steps=fused)
        rb = RowBuffers(n, dev, steps=1)
        env.rollout(min(16, env.max_fused_steps), policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED, obs_buffers=rb)
        nb, stride = int(L.bg_state_blob_bytes(env._h)), env.state_blob_stride
        half = n // 2
        dst, src, every = np.arange(half, n, dtype=np.int32), np.arange(half, dtype=np.int32), np.arange(n, dtype=np.int32)
        blobs = torch.empty((n, stride), dtype=torch.uint8, device=dev)
        scratch = torch.empty((2, n * stride), dtype=torch.uint8, device=dev)
        g, own = C.c_double(), {}

        def bench_copy(nbytes):
            rc = L.bg_bench_copy(C.c_void_p(scratch[0].data_ptr()), C.c_void_p(scratch[1].data_ptr()), C.c_uint64(nbytes & ~15), 1, C.byref(g),
                                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            assert rc == 0
            own.setdefault(nbytes, []).append(g.value)
        env.get_states(out=blobs)
        B2B = 8   # calls inside one pair of events: the host's part of call k + 1 (checking and uploading the index lists) runs beside the kernel of call k

        def times(fn):
            def run():
                for _ in range(B2B):
                    fn()
            return run
        res = alternate({"copy": lambda: env.copy_states(dst, src, observe=False), "bench_half": lambda: bench_copy(half * nb),
                         "get": lambda: env.get_states(every, out=blobs), "set": lambda: env.set_states(every, blobs, observe=False),
                         "bench_all": lambda: bench_copy(n * nb),
                         "copy_b2b": times(lambda: env.copy_states(dst, src, observe=False)), "get_b2b": times(lambda: env.get_states(None, out=blobs))})
        for k in ("copy_b2b", "get_b2b"):
            res[k] = res[k] / B2B
        say()
        say(f"{name}: blob {nb} bytes (stride {stride}), handle {env.state_bytes() / 1e9:.2f} GB, refill period {env.max_fused_steps} steps")
        for k, m in (("copy", half), ("copy_b2b", half), ("bench_half", half), ("get", n), ("get_b2b", n), ("set", n), ("bench_all", n)):
            p = res[k]
            rate = np.median(own[m * nb][args.warmup:]) if k.startswith("bench") else 2 * m * nb / p[1] / 1e6   # (the bench copy times its own kernel)
            say(f"  {k:<11} m {m:>6}  {2 * m * nb / 1e6:8.1f} MB moved  {p[0]:8.3f} {p[1]:8.3f} {p[2]:8.3f} ms  {rate:7.0f} GB/s")
        if n == 65536:
            forks = np.arange(1, 61, dtype=np.int32)
            host = []

            def fork():
                t = time.perf_counter(); env.fork(0, forks, observe=False); host.append((time.perf_counter() - t) * 1e6)
            p = alternate({"fork": fork})["fork"]
            say(f"  60-way fork (env 0 -> envs 1..60): {p[0] * 1e3:.1f} {p[1] * 1e3:.1f} {p[2] * 1e3:.1f} us by device events around the call, "
                f"{np.median(host[args.warmup:]):.1f} us of host time inside it ({60 * nb / 1e6:.2f} MB read + written)")
            # the first launch after a forced top-up: set_states of ONE env forces the whole handle's rings to be topped up before the next step
            one = env.get_states([0])
            T = min(16, env.max_fused_steps)
            rbT = RowBuffers(n, dev, steps=T)
            roll = lambda: env.rollout(T, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED, obs_buffers=rbT)

            def forced():
                env.set_states([0], one, observe=False)
                return events(roll)
            plain, topped = [], []
            for r in range(args.warmup + args.repeats):
                a, b = events(roll), forced()
                if r >= args.warmup:
                    plain.append(a); topped.append(b)
            say(f"  a {T}-step launch: {np.median(plain):.3f} ms as the schedule runs it, {np.median(topped):.3f} ms as the first launch behind a forced top-up "
                f"(set_states of one env; copy_states inside one handle forces none)")
            env.check()
        env.close()
        del blobs, scratch

    n = 64
    env = BalatroVecEnv(n, [7 + i for i in range(n)], device=0, fused_steps=16)
    nb = int(L.bg_state_blob_bytes(env._h))
    every = np.arange(n, dtype=np.int32)
    blobs = env.get_states()
    loop_get, loop_set, new_get, new_set = [], [], [], []
    for r in range(args.warmup + args.repeats):
        torch.cuda.synchronize(); t = time.perf_counter(); host = [env.get_state(i) for i in range(n)]; loop_get.append(time.perf_counter() - t)
        t = time.perf_counter()
        for i in range(n):
            env.set_state(i, host[i])
        loop_set.append(time.perf_counter() - t)
        t = time.perf_counter(); env.get_states(every, out=blobs); torch.cuda.synchronize(); new_get.append(time.perf_counter() - t)
        t = time.perf_counter(); env.set_states(every, blobs, observe=False); torch.cuda.synchronize(); new_set.append(time.perf_counter() - t)
    med = lambda v: float(np.median(v[args.warmup:])) * 1e6
    say()
    say(f"64 envs, fused_steps=16 (blob {nb} bytes), host clock to completion, per env: get_state loop {med(loop_get) / n:.1f} us, get_states {med(new_get) / n:.2f} us "
        f"({med(loop_get) / med(new_get):.0f}x); set_state loop {med(loop_set) / n:.1f} us, set_states {med(new_set) / n:.2f} us ({med(loop_set) / med(new_set):.0f}x)  "
        f"(the loop's blobs end on the host, the batch's on the device)")
    env.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
