#!/usr/bin/env python3
"""Outputs of `ops.attention` with 32-channel heads, recorded on the commit BEFORE the head width became a kernel parameter:
tests/test_gpu_attention_heads.py::test_narrow_heads_are_bitwise_unchanged compares today's kernels against them bit by bit.

    python tests/golden/make_golden_attention32.py [OUT_DIR]          (needs the GPU; OUT_DIR defaults to tests/golden)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from attention_heads_case import case, views  # noqa: E402

SHAPES = [(33, 311, 8, 1), (200, 3000, 8, 2)]


def run(Lq, Lk, H, nsrc, bf16, device="cuda:0"):
    from segdino3d_amd import ops
    c = case(Lq, Lk, H, 32, nsrc, True, tag="a32")
    q, k, v, q2, k2 = views(c["pack_q"].to(device), c["pack_k"].to(device), c["C"], nsrc)
    if bf16:
        with ops.bf16_decoder_scope():
            return ops.attention(q, k, v, H, c["scale"], mask_bits=c["bits"].to(device), q2=q2, k2=k2).cpu()
    return ops.attention(q, k, v, H, c["scale"], mask_bits=c["bits"].to(device), q2=q2, k2=k2).cpu()


def name(Lq, Lk, nsrc, bf16):
    return f"{Lq}x{Lk}_s{nsrc}_{'bf16' if bf16 else 'fp32'}"


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else HERE
    os.makedirs(out, exist_ok=True)
    arrays = {name(Lq, Lk, nsrc, bf16): run(Lq, Lk, H, nsrc, bf16).numpy() for Lq, Lk, H, nsrc in SHAPES for bf16 in (False, True)}
    np.savez_compressed(os.path.join(out, "attention32.npz"), **arrays)
    print("wrote attention32.npz:", ", ".join(arrays))


if __name__ == "__main__":
    main()
