#!/usr/bin/env python3
"""What does the network's first layer cost straight from the stored records (linear_rows / linear_rows_grad: bg_linear_rows, bg_linear_rows_grad) beside
the composite a user writes without it on the same commit?  Writes profiles/linear_rows.txt (--out).

One process.  65 536 envs (BASELINE configs[2], as bench.py sets them up) roll out 100 steps into a RowBuffers at stride 384: a 2.5 GB store of
6 553 600 records.  Minibatches of 4 096 and 65 536 rows out of a shuffled permutation, H = 128, 512, 1024, with and without frozen VecNormalize
statistics.  Every timed call takes the NEXT minibatch of the permutation, as an epoch does, so the records come from HBM.  The ways alternate repeat by
repeat in the same process:
  forward   ours       linear_rows(rows, w[H, 628] bf16, b, index=, norm=, dtype=bf16)                                   one launch
            composite  encode_rows(rows, "fixed", bf16, index=, norm=) then torch.nn.functional.linear(x, w, b_bf16)      the [m, 628] matrix goes through HBM
  backward  ours       linear_rows_grad(rows, dout bf16, index=, norm=, dweight=[H, 628] f32)                             two launches
            composite  dout.T @ x with x the [m, 628] bf16 matrix ALREADY in memory (kept from the forward: its cheapest form), bf16 result
"kernel" is the library's own kernel_ms_out (ours; for the composite the encode kernel alone), "call" device events around the whole Python call
(median of >= 20 repeats after warm-up, p10 / p90 for ours).  Before timing the results are compared: forward within bf16 rounding of the composite's,
gradient within the float32 bound of tests/linear_ref.py's kind.  --encode-only prints bg_encode_rows_ex's own medians ("fixed" bf16, with and without
statistics) and nothing else: run on the parent commit's library and on this one (BALATRO_MI355X_LIB) to see that the kernels beside the new header
did not move."""
import sys

import numpy as np

import first_layer_rows as flr


def main():
    ap = flr.parser(batches=[4096, 65536], widths=[128, 512, 1024], out="linear_rows.txt")
    ap.add_argument("--encode-only", action="store_true")
    args = ap.parse_args()
    S = flr.open_session(args, "linear_rows.py")
    if S is None:
        return 2
    torch, rb, dev = S.torch, S.rb, S.dev
    from balatro_gym_amd import RowNormalizer, encode_rows, linear_rows, linear_rows_grad, _native as nat
    stats = RowNormalizer(args.envs, dev)
    stats.normalize_obs(rb.rows[:4])
    stats.training = False
    S.describe()

    if args.encode_only:
        S.say(f"{'m':>6} {'norm':>4} | {'bg_encode_rows_ex kernel p10':>28} {'median':>8} {'p90':>8} | {'call median':>11}")
        for m in args.batches:
            out = torch.empty((m, 628), dtype=torch.bfloat16, device=dev)
            for normed in (False, True):
                call, kern = S.run({"encode": lambda index, t: encode_rows(rb.rows, "fixed", torch.bfloat16, out, index=index, norm=stats if normed else None, timing=True)[1] if t else
                                    encode_rows(rb.rows, "fixed", torch.bfloat16, out, index=index, norm=stats if normed else None)}, m)
                k = kern["encode"]
                S.say(f"{m:>6} {'yes' if normed else 'no':>4} | {np.percentile(k, 10):>28.4f} {np.median(k):>8.4f} {np.percentile(k, 90):>8.4f} | {np.median(call['encode']):>11.4f}")
        return S.finish()

    S.header(f" {'norm':>4}")
    for m in args.batches:
        x = torch.empty((m, 628), dtype=torch.bfloat16, device=dev)
        for H in args.widths:
            g = torch.Generator(device=dev).manual_seed(H)
            w = (torch.randn((H, 628), device=dev, generator=g) * 0.05).to(torch.bfloat16)
            b = torch.randn(H, device=dev, generator=g)
            b16 = b.to(torch.bfloat16)
            dout = torch.randn((m, H), device=dev, generator=g).to(torch.bfloat16)
            out = torch.empty((m, H), dtype=torch.bfloat16, device=dev)
            dweight = torch.zeros((H, 628), dtype=torch.float32, device=dev)
            ws = torch.empty(int(nat.load().bg_linear_rows_workspace_bytes(m, H)), dtype=torch.uint8, device=dev)
            for normed in (False, True):
                nm = stats if normed else None
                case = f"m {m} H {H} norm {normed}"
                index = S.minibatch(m)
                ours = linear_rows(rb.rows, w, b, index=index, norm=nm, dtype=torch.float32)
                comp = torch.nn.functional.linear(encode_rows(rb.rows, "fixed", torch.float32, index=index, norm=nm).to(torch.bfloat16).float(), w.float(), b)
                if S.differs(case, "forward", ours, comp):
                    return 1
                encode_rows(rb.rows, "fixed", torch.bfloat16, x, index=index, norm=nm)
                gw, _ = linear_rows_grad(rb.rows, dout, index=index, norm=nm, dweight=dweight, workspace=ws)
                if S.differs(case, "gradient", gw, dout.float().T @ x.float()):
                    return 1
                del ours, comp

                def ours_fwd(index, t):
                    r = linear_rows(rb.rows, w, b, index=index, norm=nm, out=out, timing=t)
                    return r[1] if t else 0.0

                def ours_bwd(index, t):
                    r = linear_rows_grad(rb.rows, dout, index=index, norm=nm, dweight=dweight, workspace=ws, timing=t)
                    return r[2] if t else 0.0

                def composite_fwd(index, t):
                    r = encode_rows(rb.rows, "fixed", torch.bfloat16, x, index=index, norm=nm, timing=t)
                    torch.nn.functional.linear(x, w, b16)
                    return r[1] if t else 0.0

                def composite_bwd(index, t):
                    dout.T @ x
                    return 0.0
                yn = "yes" if normed else "no"
                S.measure("forward", m, H, {"ours": ours_fwd, "composite": composite_fwd}, f" {yn:>4}", f" norm {yn}")
                S.measure("backward", m, H, {"ours": ours_bwd, "composite": composite_bwd}, f" {yn:>4}", f" norm {yn}")
    S.summary()
    return S.finish()


if __name__ == "__main__":
    sys.exit(main())
