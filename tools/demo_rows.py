#!/usr/bin/env python3
"""What does bg_demo_append_rows cost beside the same bytes produced in torch and beside a plain copy, which loads should its scatter use, and did the
calls next to it move?

One commit.  A [K + 1 = 101, N] store of records at stride 384 is built on the device (N = 65 536 and 4 096: random bytes), with float32 weights that
keep 1 %, 10 % and 100 % of the K * N candidate rows, float64 returns, and a ring of K * N slots at stride 384 (so nothing is dropped and every call
writes what it keeps).  Medians (p10 / median / p90 after warm-up):
  the call       DemoBuffer.add(store, weights, returns=): the kernel time of its three launches by the library's own kernel_ms_out (device events
                 around them) and the whole Python call by device events
      against    the torch composite that produces the same bytes: nonzero() of the keep test (the host waits for the count), two index_selects of
                 the record rows, the patch copies, the ring / weight / source writes with wrap; whole call by device events, the wait included.
                 Its ring is compared with the call's, once per shape.
      against    (100 % keep) bg_bench_copy of the same number of bytes read + written, in the same process: per row 352 + 4 + 4 + 8 read (the
                 observation record, its weight in both passes, its return; the 32 bytes of the next record are lines another row reads) and
                 352 + 4 + 4 written
  the loads      --ab-lib NAME=LIB (repeatable): a library built from the same sources with -DBG_DEMO_NT=1 (non-temporal loads of the store's
                 records) or -DBG_DEMO_NT_ST=0 (plain stores to the ring); the call's medians on each and the time of the learner's first read
                 behind the call (encode_rows of 65 536 drawn slots), in child processes of their own, alternating
  neighbours     --baseline-root DIR: another checkout with its own built library (the parent commit's); the kernel / call medians of
                 episode_outcomes (K x N) and bc_loss (m = N rows) on both, in child processes of their own, alternating: they should not have moved.
A child process that fails -- a non-zero exit, no result line, its time limit -- ends the run: what was gathered is written, the exit status is 1 and
nothing more is started on the GPU.  No ratio is promised; what comes out is written down, the shapes where the composite wins included.  --notes FILE is appended verbatim (the
compiler's resource lines, tools/isa_diff.py's finding)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("DEMO_ROWS_PACKAGE_ROOT") or ROOT)   # (a child process of --baseline-root imports the other checkout's package)
K, STRIDE = 100, 384
SIZES = (65536, 4096)
SHARES = (0.01, 0.10, 1.0)
ROW_READ, ROW_WRITTEN = 352 + 4 + 4 + 8, 352 + 4 + 4


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


def inputs(torch, N, share, seed=7):
    g = torch.Generator(device="cuda").manual_seed(seed)
    store = torch.randint(0, 256, (K + 1, N, STRIDE), dtype=torch.uint8, device="cuda", generator=g)
    u = torch.rand((K, N), device="cuda", generator=g)
    weights = torch.where(u < share, u + 0.25, torch.zeros_like(u)) if share < 1.0 else u + 0.25
    returns = torch.randn((K, N), dtype=torch.float64, device="cuda", generator=g)
    return store, weights.contiguous(), returns


class Composite:
    """The same bytes in torch.  The cursor lives on the host: nonzero() has to wait for the count anyway."""

    def __init__(self, torch, capacity, stride):
        self.torch, self.C, self.total = torch, capacity, 0
        self.rows = torch.zeros((capacity, stride), dtype=torch.uint8, device="cuda")
        self.weight = torch.zeros(capacity, dtype=torch.float32, device="cuda")
        self.source = torch.full((capacity,), -1, dtype=torch.int32, device="cuda")

    def add(self, store, weights, returns):
        torch = self.torch
        N = store.shape[1]
        w = weights.reshape(-1)
        idx = torch.nonzero(torch.isfinite(w) & (w > 0)).reshape(-1)   # the host synchronises here
        kept = int(idx.numel())
        r0 = max(kept - self.C, 0)
        idx = idx[r0:]
        n = kept - r0
        flat = store.view(-1, store.shape[2])
        rec = flat.index_select(0, idx)
        nxt = flat.index_select(0, idx + N)
        rec[:, 172:176] = nxt[:, 172:176]
        rec[:, 342:352] = nxt[:, 342:352]
        rec[:, 136:144] = returns.reshape(-1)[idx].view(torch.uint8).view(n, 8)
        start = (self.total + r0) % self.C
        first = min(n, self.C - start)
        for dst, src in ((self.rows[:, :352], rec[:, :352]), (self.weight, w[idx]), (self.source, idx.to(torch.int32))):
            dst[start:start + first] = src[:first]
            if first < n:
                dst[:n - first] = src[first:]
        self.total += kept


def append_medians(torch, repeats, warmup, say=None, with_composite=False):
    """DemoBuffer.add on whatever library this process loads, per (N, share) -> dict; with_composite: the torch composite and the copy beside it."""
    from balatro_gym_amd import DemoBuffer, encode_rows, _native as nat
    L = nat.load()
    out = {"signature": nat.device_code_signature(), "library": nat.lib_path()}
    for N in SIZES:
        M = K * N
        for share in SHARES:
            store, weights, returns = inputs(torch, N, share)
            demo = DemoBuffer(M, torch.device("cuda", 0))
            ker = [demo.add(store, weights, returns=returns, timing=True) for _ in range(warmup + repeats)][warmup:]
            ev = timed(torch, lambda: demo.add(store, weights, returns=returns), repeats, warmup)
            kept = int(demo.cursor[1])
            # the learner's first read behind an add: a minibatch of 65 536 drawn slots encoded straight from the ring, timed right after the call
            back = []
            for r in range(warmup + repeats):
                demo.add(store, weights, returns=returns)
                index = demo.sample(65536, seed=3, t=r)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                encode_rows(demo.rows, "produced", index=index)
                b.record()
                b.synchronize()
                back.append(a.elapsed_time(b))
            back = back[warmup:]
            out[f"{N} x {K} keep {share:.2f}"] = {"kernel": pct(ker), "event": pct(ev), "kept": kept, "back": pct(back)}
            if say:
                say(f"== {N} x {K} candidate rows, keep share {share:.2f}: {kept} rows kept ({kept * 352 / 1e6:.1f} MB of records)")
                say(f"bg_demo_append_rows               kernel {pct(ker)}   call {pct(ev)}   encode_rows of 65 536 drawn slots right behind it {pct(back)}")
            if with_composite:
                comp = Composite(torch, M, STRIDE)
                fresh = DemoBuffer(M, torch.device("cuda", 0))
                fresh.add(store, weights, returns=returns)
                comp.add(store, weights, returns)
                same = torch.equal(comp.rows, fresh.rows) and torch.equal(comp.weight, fresh.weight) and torch.equal(comp.source, fresh.source) \
                    and comp.total == int(fresh.cursor[0])
                cev = timed(torch, lambda: comp.add(store, weights, returns), max(5, repeats // 2), 2)
                say(f"torch composite (nonzero, gathers)  call {pct(cev)}   its ring, weights and sources equal the call's: {same}")
                del comp, fresh
                if share == 1.0:
                    nbytes = (M * (ROW_READ + ROW_WRITTEN) // 2) // 16 * 16
                    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
                    gbps = C.c_double(0.0)
                    rc = L.bg_bench_copy(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), C.c_uint64(nbytes), 20, C.byref(gbps),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
                    med = float(np.median(ker))
                    say(f"bg_bench_copy of {2 * nbytes / 1e6:.0f} MB read + written: rc {rc}, {gbps.value:.0f} GB/s = {2 * nbytes / gbps.value / 1e6:.4f} ms;"
                        f"  the call's three launches move the same bytes at {2 * nbytes / med / 1e6:.0f} GB/s")
                    del src, dst
            del store, weights, returns, demo
            torch.cuda.empty_cache()
    return out


def neighbours(torch, repeats, warmup):
    """The medians of episode_outcomes and bc_loss on whatever checkout and library this process loads -> dict."""
    from balatro_gym_amd import bc_loss, episode_outcomes, _native as nat
    out = {"signature": nat.device_code_signature(), "library": nat.lib_path()}
    for N in SIZES:
        store, _, _ = inputs(torch, N, 1.0)
        store[:, :, 342] = (store[:, :, 342] < 13).to(torch.uint8)
        store[:, :, 176:236] = (store[:, :, 176:236] < 154).to(torch.uint8)
        store[:, :, 176] = 1
        rows = store[1:]
        ker = [episode_outcomes(rows, 0.99, timing=True).kernel_ms for _ in range(warmup + repeats)][warmup:]
        ev = timed(torch, lambda: episode_outcomes(rows, 0.99), repeats, warmup)
        out[f"episode_outcomes {K} x {N}"] = {"kernel": pct(ker), "event": pct(ev)}
        m = N
        logits = torch.randn((m, 60), device="cuda") * 2.0
        obs = store[0]
        act = (store[1, :, 172:176].view(torch.int32)[:, 0] % 60).abs().contiguous()
        w = torch.rand(m, device="cuda")
        ker = [bc_loss(logits, act, obs, weights=w, ent_coef=0.01, timing=True)[1].kernel_ms for _ in range(warmup + repeats)][warmup:]
        ev = timed(torch, lambda: bc_loss(logits, act, obs, weights=w, ent_coef=0.01), repeats, warmup)
        out[f"bc_loss {m} rows"] = {"kernel": pct(ker), "event": pct(ev)}
        del store, rows
        torch.cuda.empty_cache()
    return out


def child(mode, repeats, warmup, env_over):
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--repeats", str(repeats), "--warmup", str(warmup)],
                           env=dict(os.environ, **env_over), capture_output=True, text=True, timeout=900)
    except subprocess.TimeoutExpired:
        return None, "the child process did not end within its time limit and was killed"
    got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not got:
        return None, f"the child process failed ({r.returncode}): {r.stderr[-400:]}"
    return json.loads(got[0][len("RESULT "):]), None


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="how often each side of an alternating comparison runs")
    ap.add_argument("--mode", default="main", choices=("main", "append", "neighbours"), help="append / neighbours: print one RESULT line of JSON and stop (the child processes)")
    ap.add_argument("--ab-lib", action="append", default=[], metavar="NAME=LIB", help="a library of the same sources built with another -DBG_DEMO_NT / -DBG_DEMO_NT_ST (repeatable)")
    ap.add_argument("--baseline-root", default=None, help="another checkout with its built library (the parent commit's)")
    ap.add_argument("--notes", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demo_rows.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("demo_rows.py: no GPU is visible", file=sys.stderr)
        return 2
    if args.mode == "append":
        print("RESULT " + json.dumps(append_medians(torch, args.repeats, args.warmup)), flush=True)
        return 0
    if args.mode == "neighbours":
        print("RESULT " + json.dumps(neighbours(torch, args.repeats, args.warmup)), flush=True)
        return 0
    from balatro_gym_amd import _native as nat
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"build signature {nat.device_code_signature()}  library {os.path.basename(nat.lib_path())}  GPU {torch.cuda.get_device_name(0)}")
    say(f"synthetic records, K = {K}, stride {STRIDE}, ring of K * N slots; {args.repeats} repeats after {args.warmup} warm-up; milliseconds: p10 median p90")
    say()
    def finish(rc):
        """Write what was gathered.  rc != 0: a child process failed -- that ends the run, nothing more is started on the GPU."""
        if rc == 0 and args.notes and os.path.exists(args.notes):
            say()
            lines.extend(open(args.notes).read().rstrip("\n").split("\n"))
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return rc

    append_medians(torch, args.repeats, args.warmup, say=say, with_composite=True)
    for title, mode, sides in (
            ("the scatter's loads of the store and stores to the ring: plain loads and non-temporal stores (this library) against the other builds, kernel / whole call", "append",
             [("plain loads, non-temporal stores", {})] + [(s.split("=", 1)[0], {"BALATRO_MI355X_LIB": os.path.abspath(s.split("=", 1)[1])}) for s in args.ab_lib]),
            ("the neighbours: medians of episode_outcomes and bc_loss, kernel / whole call", "neighbours",
             [("this commit", {})] + ([("baseline checkout", {"DEMO_ROWS_PACKAGE_ROOT": os.path.abspath(args.baseline_root)})] if args.baseline_root else []))):
        if len(sides) < 2:
            continue
        say()
        say(f"== {title}; child processes, alternating")
        for rnd in range(args.rounds):
            for name, env_over in sides:
                d, err = child(mode, args.repeats, args.warmup, env_over)
                if err:
                    say(f"{name}, round {rnd}: {err}")
                    say("the run ends here: after a failed child process nothing more is started on the GPU")
                    return finish(1)
                say(f"{name}, round {rnd}: signature {d['signature']} ({os.path.basename(d['library'])})")
                for k, v in d.items():
                    if isinstance(v, dict):
                        say(f"  {k:<30} kernel {v['kernel']}   call {v['event']}" + (f"   read behind it {v['back']}" if "back" in v else ""))
    return finish(0)


if __name__ == "__main__":
    sys.exit(main())
