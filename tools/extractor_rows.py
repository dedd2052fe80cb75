#!/usr/bin/env python3
"""What does the first layer behind BalatroFeaturesExtractor's input cost straight from the stored records (extractor_rows / extractor_rows_grad:
bg_extractor_rows, bg_extractor_rows_grad) beside the composite a user writes without it on the same commit?  Writes profiles/extractor_rows.txt (--out).

One process.  65 536 envs (BASELINE configs[2], as bench.py sets them up) roll out 100 steps into a RowBuffers at stride 384: a 2.5 GB store of
6 553 600 records.  Minibatches of 65 536 and 4 096 rows out of a shuffled permutation, H = 128, 448 (the reference's three first layers as one
block-structured weight), 512, 1024.  Every timed call takes the NEXT minibatch of the permutation, as an epoch does, so the records come from HBM.  The
ways alternate repeat by repeat in the same process:
  forward   ours       extractor_rows(rows, w[H, 447] bf16 at pitch 448, b, index=, activation="relu", dtype=bf16)                   one launch
            composite  encode_rows(rows, "extractor", bf16, index=) then relu(torch.nn.functional.linear(x, w, b_bf16))              [m, 447] goes through HBM
  backward  ours       extractor_rows_grad(rows, dout bf16, out=, index=, activation="relu", dweight=[H, 447] f32)                   two launches
            composite  (dout * (out > 0)).T @ x with x the [m, 447] bf16 matrix ALREADY in memory (kept from the forward: its cheapest form)
"kernel" is the library's own kernel_ms_out (ours; for the composite the encode kernel alone), "call" device events around the whole Python call
(median of >= 20 repeats after warm-up, p10 / p90 for ours).  Before timing the results are compared: forward within bf16 rounding of the composite's,
gradient within 1e-3 of the largest element.  Every ratio is reported as measured, those below 1 included.  --resources FILE appends the compiler's
resource lines for the new kernels (the remarks file `tools/isa_diff.py --save` keeps)."""
import re
import sys

import first_layer_rows as flr


def resource_lines(path):
    """The per-kernel remarks of -Rpass-analysis=kernel-resource-usage for the bg_extractor kernels, one line per kernel."""
    out, cur = [], None
    for line in open(path):
        m = re.search(r"remark: (?:Function Name: (\S+)|\s+([A-Za-z ]+(?:\[[^\]]*\])?): (\d+))", line)
        if not m:
            continue
        if m.group(1):
            cur = [m.group(1)] if "bg_extractor" in m.group(1) else None
            if cur:
                out.append(cur)
        elif cur is not None:
            cur.append(f"{m.group(2).strip()} {m.group(3)}")
    return ["  " + c[0] + ": " + ", ".join(c[1:]) for c in out]


def main():
    ap = flr.parser(batches=[65536, 4096], widths=[128, 448, 512, 1024], out="extractor_rows.txt")
    ap.add_argument("--resources", default=None)
    args = ap.parse_args()
    S = flr.open_session(args, "extractor_rows.py")
    if S is None:
        return 2
    torch, rb, dev = S.torch, S.rb, S.dev
    from balatro_gym_amd import encode_rows, extractor_rows, extractor_rows_grad, _native as nat
    S.describe()
    S.header()
    for m in args.batches:
        x = torch.empty((m, nat.EXT_K), dtype=torch.bfloat16, device=dev)
        for H in args.widths:
            g = torch.Generator(device=dev).manual_seed(H)
            w = torch.zeros((H, nat.EXT_K + 1), dtype=torch.bfloat16, device=dev)[:, :nat.EXT_K]   # pitch 448, as RowExtractor stages it
            w.copy_(torch.randn((H, nat.EXT_K), device=dev, generator=g) * 0.05)
            wc = w.contiguous()
            b = torch.randn(H, device=dev, generator=g)
            b16 = b.to(torch.bfloat16)
            dout = torch.randn((m, H), device=dev, generator=g).to(torch.bfloat16)
            out = torch.empty((m, H), dtype=torch.bfloat16, device=dev)
            dweight = torch.zeros((H, nat.EXT_K), dtype=torch.float32, device=dev)
            case = f"m {m} H {H}"
            index = S.minibatch(m)
            ours = extractor_rows(rb.rows, w, b, index=index, activation="relu", dtype=torch.float32)
            encode_rows(rb.rows, "extractor", torch.bfloat16, x, index=index)
            if S.differs(case, "forward", ours, torch.relu(torch.nn.functional.linear(x.float(), wc.float(), b))):
                return 1
            gw, _ = extractor_rows_grad(rb.rows, dout, out=ours, index=index, activation="relu", dweight=dweight)
            if S.differs(case, "gradient", gw, (dout.float() * (ours > 0)).T @ x.float()):
                return 1
            del ours
            extractor_rows(rb.rows, w, b, index=index, activation="relu", out=out)

            def ours_fwd(index, t):
                r = extractor_rows(rb.rows, w, b, index=index, activation="relu", out=out, timing=t)
                return r[1] if t else 0.0

            def ours_bwd(index, t):
                r = extractor_rows_grad(rb.rows, dout, out=out, index=index, activation="relu", dweight=dweight, timing=t)
                return r[2] if t else 0.0

            def composite_fwd(index, t):
                r = encode_rows(rb.rows, "extractor", torch.bfloat16, x, index=index, timing=t)
                torch.relu(torch.nn.functional.linear(x, wc, b16))
                return r[1] if t else 0.0

            def composite_bwd(index, t):
                (dout * (out > 0)).T @ x
                return 0.0
            S.measure("forward", m, H, {"ours": ours_fwd, "composite": composite_fwd})
            S.measure("backward", m, H, {"ours": ours_bwd, "composite": composite_bwd})
    S.summary()
    if args.resources:
        S.say("the compiler's resource lines for the new kernels (-Rpass-analysis=kernel-resource-usage):")
        for s in resource_lines(args.resources):
            S.say(s)
    return S.finish()


if __name__ == "__main__":
    sys.exit(main())
