#!/usr/bin/env python3
"""Time per launch of the fused attention with 4 heads x 64 channels against 8 heads x 32 channels at d_model = 256 (the same flops
and bytes), forward and backward, fp32 and bf16, at the decoder's shapes; and the error of both against float64 attention on the same
inputs.  Device events around a queue of launches after a warm-up, the median of repeated windows, narrow and wide alternating.

    python tools/attention_heads_bench.py [--out FILE.md]           (needs the GPU; prints markdown)"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from attention_heads_case import attention64, case, views  # noqa: E402

SHAPES = [(200, 3000, 2), (3000, 3000, 2), (200, 301, 1)]                  # (Lq, Lk, score sources)
ERR_SHAPES = [(33, 31, 1), (70, 65, 2), (200, 301, 2), (40, 1030, 2)]


def window(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches                             # us per launch


def measure(fns, launches, repeats):
    """fns: {name: callable}; windows of the callables alternate -> {name: (median us, min, max)}"""
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(window(fn, launches))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def setup(Lq, Lk, H, D, nsrc, d):
    c = case(Lq, Lk, H, D, nsrc, True, tag="ahb")
    pq, pk = c["pack_q"].to(d), c["pack_k"].to(d)
    return c, pq, pk, c["bits"].to(d), c["dy"].to(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    from segdino3d_amd import ops, train_dec as T
    if not torch.cuda.is_available():
        raise SystemExit("attention_heads_bench: needs a HIP device")
    d = torch.device("cuda:0")
    lines = ["### Wide against narrow at equal work (us per launch: median [min - max] of %d windows, narrow and wide alternating)" % args.repeats, "",
             "| Lq x Lk | sources | pass | dtype | 8 x 32 | 4 x 64 | wide / narrow | (waves, split) 8 x 32 | (waves, split) 4 x 64 |", "|---|---|---|---|---|---|---|---|---|"]
    for Lq, Lk, nsrc in SHAPES:
        launches = 20 if Lq * Lk > 1_000_000 else 200
        for bf16 in (False, True):
            fwd, bwd = {}, {}
            for name, H, D in (("narrow", 8, 32), ("wide", 4, 64)):
                c, pq, pk, bits, dy = setup(Lq, Lk, H, D, nsrc, d)
                q, k, v, q2, k2 = views(pq, pk, c["C"], nsrc)

                def f(q=q, k=k, v=v, q2=q2, k2=k2, H=H, s=c["scale"], bits=bits):
                    if bf16:
                        with ops.bf16_decoder_scope():
                            return ops.attention(q, k, v, H, s, mask_bits=bits, q2=q2, k2=k2)
                    return ops.attention(q, k, v, H, s, mask_bits=bits, q2=q2, k2=k2)
                fwd[name] = f
                if not bf16:                                             # the backward kernels are fp32 in both modes
                    rq, rk = pq.clone().requires_grad_(True), pk.clone().requires_grad_(True)
                    o = T.attention(*views(rq, rk, c["C"], nsrc)[:3], H, c["scale"], mask_bits=bits,
                                    q2=views(rq, rk, c["C"], nsrc)[3], k2=views(rq, rk, c["C"], nsrc)[4])
                    bwd[name] = lambda o=o, dy=dy, rq=rq, rk=rk: torch.autograd.grad(o, (rq, rk), dy, retain_graph=True)
            for what, fns in (("forward", fwd), ("backward", bwd)):
                if not fns:
                    continue
                r = measure(fns, launches, args.repeats)
                cell = lambda x: f"{x[0]:.1f} [{x[1]:.1f} - {x[2]:.1f}]"  # noqa: E731
                lines.append(f"| {Lq} x {Lk} | {nsrc} | {what} | {'bf16' if bf16 else 'fp32'} | {cell(r['narrow'])} | {cell(r['wide'])} | "
                             f"{r['wide'][0] / r['narrow'][0]:.2f} | {ops.attention_launch_config(Lq, Lk, 8, 32)} | {ops.attention_launch_config(Lq, Lk, 4, 64)} |")
    lines += ["", "(backward = torch.autograd.grad through the attention node: both backward kernels plus the packing of the gradients torch does around them)", "",
              "### Error against float64 attention (max abs error / max |ref|), same Lq, Lk, sources and mask; 2 H heads of 32 against H heads of 64", "",
              "| Lq x Lk | sources | fp32 8 x 32 | fp32 4 x 64 | bf16 8 x 32 | bf16 4 x 64 |", "|---|---|---|---|---|---|"]
    for Lq, Lk, nsrc in ERR_SHAPES:
        row = {}
        for name, H, D in (("narrow", 8, 32), ("wide", 4, 64)):
            c, pq, pk, bits, _ = setup(Lq, Lk, H, D, nsrc, d)
            q, k, v, q2, k2 = views(c["pack_q"], c["pack_k"], c["C"], nsrc)
            ref = attention64(q, k, v, H, c["scale"], c["blocked"], q2=q2, k2=k2)
            q, k, v, q2, k2 = views(pq, pk, c["C"], nsrc)
            row[name, "fp32"] = float((ops.attention(q, k, v, H, c["scale"], mask_bits=bits, q2=q2, k2=k2).cpu().double() - ref).abs().max() / ref.abs().max())
            with ops.bf16_decoder_scope():
                row[name, "bf16"] = float((ops.attention(q, k, v, H, c["scale"], mask_bits=bits, q2=q2, k2=k2).cpu().double() - ref).abs().max() / ref.abs().max())
        lines.append(f"| {Lq} x {Lk} | {nsrc} | {row['narrow', 'fp32']:.2e} | {row['wide', 'fp32']:.2e} | {row['narrow', 'bf16']:.2e} | {row['wide', 'bf16']:.2e} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
