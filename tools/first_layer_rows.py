"""What tools/linear_rows.py and tools/extractor_rows.py share: the store of records they measure on, the minibatches of its shuffled permutation, the
alternating timed repeats, the comparison with the composite, and the lines of the table.  The two scripts state their layer's calls and composites."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parser(batches, widths, out):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batches", type=int, nargs="+", default=batches)
    ap.add_argument("--widths", type=int, nargs="+", default=widths)
    ap.add_argument("--repeats", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out))
    return ap


class Session:
    """The rolled-out store `rb` on `dev` and everything that is measured on it; `lines` is what `finish` writes to --out."""

    def __init__(self, args, who):
        import torch
        import bench
        from balatro_gym_amd import BalatroVecEnv, _native as nat
        from balatro_gym_amd.vec_env import RowBuffers
        self.args, self.who, self.torch, self.lines, self.slower, self.turn = args, who, torch, [], [], 0
        self.dev = dev = torch.device("cuda:0")
        n, T = args.envs, args.steps
        env = BalatroVecEnv(n, [1000 + g for g in range(n)], device=0, scorer_jokers=True, autoreset=True, max_ante=bench.MAX_ANTE, fused_steps=min(T, 100))
        env.inject(jokers=[bench.jokers_for(g) for g in range(n)], apply_now=True)
        self.rb = rb = RowBuffers(n, dev, steps=T, row_stride=nat.ROW_STRIDE_LINES)
        done = 0
        while done < T:
            k = min(env.max_fused_steps, T - done)
            part = rb if k == T else RowBuffers(n, dev, steps=k, row_stride=nat.ROW_STRIDE_LINES)
            env.rollout(k, policy=bench.POLICY_CYCLE3, policy_seed=bench.POLICY_SEED + done, obs_buffers=part)
            if part is not rb:
                rb.rows[done:done + k].copy_(part.rows)
            done += k
        env.close()
        self.store = n * T

    def describe(self):
        """The two opening lines; the permutation is drawn behind them."""
        from balatro_gym_amd import _native as nat
        torch, rb, args = self.torch, self.rb, self.args
        self.say(f"build signature {nat.device_code_signature()}  library {os.path.basename(nat.lib_path())}  GPU {torch.cuda.get_device_name(0)}")
        self.say(f"store: {args.envs} envs x {args.steps} steps = {self.store} records at stride {rb.row_stride}, {self.store * rb.row_stride / 1e6:.0f} MB; shuffled index; "
                 f"{args.repeats} repeats after {args.warmup} warm-up, the ways alternating; device events; ms")
        self.perm = next(rb.minibatches(self.store, generator=torch.Generator().manual_seed(20240607)))

    def say(self, s):
        print(s, flush=True)
        self.lines.append(s)

    def minibatch(self, m):
        self.turn += 1
        lo = (self.turn % (self.store // m)) * m
        return self.perm[lo:lo + m].contiguous()

    def timed(self, fn):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), r

    def run(self, ways, m):
        """ways: name -> fn(index, timing) returning the library's kernel ms when timing (which synchronises, so the whole call is timed without it)."""
        call = {w: [] for w in ways}
        kern = {w: [] for w in ways}
        for rep in range(self.args.warmup + self.args.repeats):
            for w, fn in ways.items():
                index = self.minibatch(m)
                c, _ = self.timed(lambda: fn(index, False))
                index = self.minibatch(m)
                k = fn(index, True)
                if rep >= self.args.warmup:
                    call[w].append(c)
                    kern[w].append(k)
        return call, kern

    def differs(self, case, what, got, want):
        """got against the composite's want within 1e-3 of its largest element; says so on stderr and returns True when it is not."""
        scale = float(want.abs().max())
        off = float((got - want).abs().max())
        if not off <= 1e-3 * scale:
            print(f"{self.who}: {case}: {what} differs from the composite by {off} of {scale}", file=sys.stderr)
            return True
        return False

    def header(self, extra=""):
        self.say(f"{'pass':>8} {'m':>6} {'H':>5}{extra} | {'ours kernel':>11} {'call p10':>9} {'median':>8} {'p90':>8} | {'composite encode kernel':>23} {'call median':>11} | "
                 f"{'composite / ours (call)':>23}")

    def measure(self, name, m, H, ways, cell="", label=""):
        """One line of the table: ways {"ours", "composite"} over minibatches of m; cell / label: the script's extra column and its words for the summary."""
        call, kern = self.run(ways, m)
        o, c = call["ours"], call["composite"]
        ratio = np.median(c) / np.median(o)
        if ratio < 1.0:
            self.slower.append(f"{name} m {m} H {H}{label}: ours {np.median(o):.4f} ms, composite {np.median(c):.4f} ms")
        self.say(f"{name:>8} {m:>6} {H:>5}{cell} | {np.median(kern['ours']):>11.4f} {np.percentile(o, 10):>9.4f} {np.median(o):>8.4f} {np.percentile(o, 90):>8.4f} | "
                 f"{np.median(kern['composite']):>23.4f} {np.median(c):>11.4f} | {ratio:>22.2f}x")

    def summary(self):
        self.say("ours faster than the composite (whole call) in every shape: " + ("yes" if not self.slower else "NO"))
        for s in self.slower:
            self.say("  " + s)

    def finish(self):
        out = self.args.out
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(self.lines) + "\n")
        return 0


def open_session(args, who):
    """-> a Session, or None with a line on stderr where no GPU is visible."""
    import torch
    if not torch.cuda.is_available():
        print(f"{who}: no GPU is visible", file=sys.stderr)
        return None
    return Session(args, who)
