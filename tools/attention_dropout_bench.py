#!/usr/bin/env python3
"""Time per launch and peak memory of attention with dropout on the probabilities at the decoder's shapes (two score sources, bit mask),
8 heads x 32 channels and 4 x 64: the fused kernels at p = 0 (the plain instantiations), the fused kernels at p = 0.1 (mask generated
inside them) and the explicit route at p = 0.1 (`train_dec.attention_dropout` without `keep`: [H, Lq, Lk] probabilities, torch's
softmax, dropout, matmuls and autograd - the statements every p > 0 ran before the kernels had a random stream).  fp32 and bf16 forward,
fp32 backward.  Device events around a queue of launches after a warm-up, the median of repeated windows, the arms alternating.

    python tools/attention_dropout_bench.py [--out FILE.md] [--passes forward,backward]          (needs the GPU; prints markdown)"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from attention_heads_bench import measure, setup  # noqa: E402
from attention_heads_case import views  # noqa: E402

SHAPES = [(200, 3000), (3000, 3000)]
LAYOUTS = [(8, 32), (4, 64)]
NSRC = 2
P = 0.1
ARMS = ["fused p=0", "fused p=0.1", "explicit p=0.1"]


def peak(step):
    """bytes by which the allocator's peak rises over one call of step()"""
    step()                                                                # workspaces and caches of the first call
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--passes", default="forward,backward")
    args = ap.parse_args()
    from segdino3d_amd import _lib, ops, train_dec as T
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("attention_dropout_bench: needs a HIP device")
    d = torch.device("cuda:0")
    key = torch.tensor([0x243F6A88, -0x7A5CF72D], dtype=torch.int32, device=d)
    cell = lambda x: f"{x[0]:.1f} [{x[1]:.1f} - {x[2]:.1f}]"  # noqa: E731
    lines = ["### Attention with dropout on the probabilities (us per launch: median [min - max] of %d windows, arms alternating)" % args.repeats, "",
             "| Lq x Lk | heads | pass | dtype | " + " | ".join(ARMS) + " | fused p=0.1 / fused p=0 | fused p=0.1 median < explicit min |", "|---|---|---|---|---|---|---|---|---|"]
    mem = ["", "### Peak memory of one forward + backward (MiB the allocator's peak rises by; one fp32 [H, Lq, Lk] tensor for scale)", "",
           "| Lq x Lk | heads | fused p=0.1 | explicit p=0.1 | one probability tensor |", "|---|---|---|---|---|"]
    for Lq, Lk in SHAPES:
        launches = 20 if Lq * Lk > 1_000_000 else 100
        for H, D in LAYOUTS:
            c, pq, pk, bits, dy = setup(Lq, Lk, H, D, NSRC, d)
            kw = dict(mask_bits=bits)
            calls = {"fused p=0": lambda q, k, v, q2, k2: T.attention(q, k, v, H, c["scale"], q2=q2, k2=k2, **kw),
                     "fused p=0.1": lambda q, k, v, q2, k2: T.attention(q, k, v, H, c["scale"], q2=q2, k2=k2, dropout_p=P, key=key, call=1, **kw),
                     "explicit p=0.1": lambda q, k, v, q2, k2: T.attention_dropout(q, k, v, H, c["scale"], q2=q2, k2=k2, p=P, **kw)}
            rows = []
            if "forward" in args.passes:
                # the fused arms call the C entry points as the training node does (lse kept, full split workspace) without the node's host
                # work, which at 200 queries is as long as the kernel; the explicit arm is the Python route itself
                q, k, v, q2, k2 = views(pq, pk, c["C"], NSRC)
                out, lse = torch.empty(Lq, H * D, device=d), torch.empty(H, Lq, device=d)
                ws = torch.empty(lib.sd3d_attention_ws_bytes(Lq, H, D), dtype=torch.uint8, device=d)
                ld, st = pq.stride(0), pk.stride(0)
                head = lambda bf16: (q.data_ptr(), ld, q2.data_ptr(), ld, k.data_ptr(), st, k2.data_ptr(), st, v.data_ptr(), st, bits.data_ptr(), Lq, Lk, H, D,  # noqa: E731
                                     c["scale"], out.data_ptr(), H * D, lse.data_ptr(), int(bf16), ws.data_ptr(), ws.numel())
                for bf16 in (False, True):
                    def explicit(bf16=bf16):
                        with torch.no_grad():
                            if bf16:
                                with ops.bf16_decoder_scope():
                                    return calls[ARMS[2]](q, k, v, q2, k2)
                            return calls[ARMS[2]](q, k, v, q2, k2)
                    rows.append(("forward", "bf16" if bf16 else "fp32",
                                 {ARMS[0]: lambda a=head(bf16): _lib.check(lib.sd3d_attention(*a, None, 0, 0.0, ops._stream()), "attention"),
                                  ARMS[1]: lambda a=head(bf16): _lib.check(lib.sd3d_attention(*a, key.data_ptr(), 1, P, ops._stream()), "attention"),
                                  ARMS[2]: explicit}))
            if "backward" in args.passes:
                bwd = {}
                for n, f in calls.items():
                    rq, rk = pq.clone().requires_grad_(True), pk.clone().requires_grad_(True)
                    o = f(*views(rq, rk, c["C"], NSRC))
                    bwd[n] = lambda o=o, rq=rq, rk=rk: torch.autograd.grad(o, (rq, rk), dy, retain_graph=True)
                rows.append(("backward", "fp32", bwd))
            for what, dtype, fns in rows:
                r = measure(fns, launches, args.repeats)
                lines.append(f"| {Lq} x {Lk} | {H} x {D} | {what} | {dtype} | " + " | ".join(cell(r[n]) for n in ARMS) +
                             f" | {r[ARMS[1]][0] / r[ARMS[0]][0]:.2f} | {'yes' if r[ARMS[1]][0] < r[ARMS[2]][1] else 'NO'} |")
                del fns
            rows.clear()

            def step(f):
                rq, rk = pq.clone().requires_grad_(True), pk.clone().requires_grad_(True)
                f(*views(rq, rk, c["C"], NSRC)).backward(dy)
            mib = lambda b: f"{b / 2 ** 20:.1f}"  # noqa: E731
            mem.append(f"| {Lq} x {Lk} | {H} x {D} | {mib(peak(lambda: step(calls[ARMS[1]])))} | {mib(peak(lambda: step(calls[ARMS[2]])))} | {mib(H * Lq * Lk * 4)} |")
            torch.cuda.empty_cache()
    text = "\n".join(lines + ["", "(forward = the C entry point as the training node calls it: kernel with lse, key-split merge; the explicit route, under no_grad, is fp32 whatever the decoder's dtype;",
                              " backward = torch.autograd.grad through the node: both backward kernels plus the packing of the gradients torch does around them)"] + mem) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
