#!/usr/bin/env python3
"""Device outputs of the attention recorded on the commit BEFORE the 32- and 64-channel kernels became one body per pass: the forward
with 64-channel heads (fp32 and bf16) and the fp32 backward through `train_dec.attention` at both widths.
tests/test_gpu_attention_heads.py::test_attention_bits_are_unchanged compares today's kernels against them bit by bit.

    python tests/golden/make_golden_attention_bits.py [OUT_DIR]       (needs the GPU; OUT_DIR defaults to tests/golden)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from attention_heads_case import case, views  # noqa: E402

# (Lq, Lk, H, nsrc), all masked.  Forward: one key past a tile; keys split four ways and merged
FWD = [(70, 65, 2, 2), (40, 1030, 2, 2)]
# Backward: one source, ten key tiles (four waves in the q kernel); two sources; 33 query tiles (the kv kernel's 96 KiB paths: 8 waves
# at 32 channels, 4 at 64) - of that one only pack_k.grad is kept, the kernel under test there writes dk, dk1 and dv
BWD = [((33, 311, 3, 1), True), ((70, 65, 2, 2), True), ((1030, 40, 1, 2), False)]
WIDTHS = (32, 64)


def forward(Lq, Lk, H, nsrc, bf16, device="cuda:0"):
    from segdino3d_amd import ops
    c = case(Lq, Lk, H, 64, nsrc, True, tag="ab")
    q, k, v, q2, k2 = views(c["pack_q"].to(device), c["pack_k"].to(device), c["C"], nsrc)
    if bf16:
        with ops.bf16_decoder_scope():
            return ops.attention(q, k, v, H, c["scale"], mask_bits=c["bits"].to(device), q2=q2, k2=k2).cpu().numpy()
    return ops.attention(q, k, v, H, c["scale"], mask_bits=c["bits"].to(device), q2=q2, k2=k2).cpu().numpy()


def backward(Lq, Lk, H, nsrc, D, device="cuda:0"):
    """-> (pack_q.grad, pack_k.grad) of train_dec.attention under the output gradient c["dy"]"""
    from segdino3d_amd import train_dec as T
    c = case(Lq, Lk, H, D, nsrc, True, tag="ab")
    pq, pk = c["pack_q"].to(device).requires_grad_(True), c["pack_k"].to(device).requires_grad_(True)
    q, k, v, q2, k2 = views(pq, pk, c["C"], nsrc)
    T.attention(q, k, v, H, c["scale"], mask_bits=c["bits"].to(device), q2=q2, k2=k2).backward(c["dy"].to(device))
    return pq.grad.cpu().numpy(), pk.grad.cpu().numpy()


def fwd_name(Lq, Lk, nsrc, bf16):
    return f"fwd64_{Lq}x{Lk}_s{nsrc}_{'bf16' if bf16 else 'fp32'}"


def bwd_name(Lq, Lk, nsrc, D, which):
    return f"bwd{D}_{Lq}x{Lk}_s{nsrc}_{which}"


# kept as the SHA-256 of shape and bytes instead of the array: the 64-channel gradients of the ten-key-tile shape are 0.5 MB of incompressible
# floats (pack_k.grad alone 311 x 576), with them the file passes the 1 MiB a committed file may have; a digest pins the same bits
DIGEST = {bwd_name(33, 311, 1, 64, "dpack_q"), bwd_name(33, 311, 1, 64, "dpack_k")}


def outputs():
    """Every pinned output of today's kernels, as stored in attention_bits.npz: {name: array, or name + '.sha256': uint8[32]}"""
    import hashlib
    arrays = {fwd_name(Lq, Lk, nsrc, bf16): forward(Lq, Lk, H, nsrc, bf16) for Lq, Lk, H, nsrc in FWD for bf16 in (False, True)}
    for (Lq, Lk, H, nsrc), keep_q in BWD:
        for D in WIDTHS:
            gq, gk = backward(Lq, Lk, H, nsrc, D)
            if keep_q:
                arrays[bwd_name(Lq, Lk, nsrc, D, "dpack_q")] = gq
            arrays[bwd_name(Lq, Lk, nsrc, D, "dpack_k")] = gk
    for name in DIGEST:
        a = np.ascontiguousarray(arrays.pop(name))
        arrays[name + ".sha256"] = np.frombuffer(hashlib.sha256(repr(a.shape).encode() + a.tobytes()).digest(), dtype=np.uint8)
    return arrays


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else HERE
    os.makedirs(out, exist_ok=True)
    arrays = outputs()
    path = os.path.join(out, "attention_bits.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote attention_bits.npz ({os.path.getsize(path)} bytes):", ", ".join(arrays))


if __name__ == "__main__":
    main()
