"""Inputs and the float64 reference shared by the attention tests of the head widths (test_decoder_heads.py,
test_gpu_attention_heads.py) and by tests/golden/make_golden_attention32.py.

Inputs are `det_randn` packed projections (queries [Lq, 2 H D] = [q | q2], keys [Lk, 3 H D] = [k | k2 | v]) whose column blocks
are taken as strided views, the mask is the one of test_gpu_decoder.py::test_attention_matches_oracle: the leading key tile(s)
blocked for every query, query 0 with a single open key (the last), an open diagonal, at least one open key per row."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from _det import det_randn  # noqa: E402


def pack_bits(blocked):
    """bool [Lq, Lk] (True = blocked) -> int32 words [Lq, ceil(Lk / 32)], bits past Lk set."""
    Lq, Lk = blocked.shape
    nw = (Lk + 31) // 32
    pad = torch.ones(Lq, nw * 32, dtype=torch.bool)
    pad[:, :Lk] = blocked
    words = (pad.view(Lq, nw, 32).long() << torch.arange(32)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def case(Lq, Lk, H, D, nsrc, masked, tag="ah"):
    """-> dict(pack_q [Lq, 2 H D], pack_k [Lk, 3 H D], dy [Lq, H D], blocked | None, bits | None, scale)"""
    C = H * D
    pack_q = det_randn(f"{tag}.q{Lq}.{C}", (Lq, 2 * C))
    pack_k = det_randn(f"{tag}.k{Lk}.{C}", (Lk, 3 * C))
    dy = det_randn(f"{tag}.dy{Lq}.{C}", (Lq, C))
    blocked = bits = None
    if masked:
        blocked = det_randn(f"{tag}.m{Lq}.{Lk}", (Lq, Lk)) > 0.3
        blocked[:, : min(40, Lk - 1)] = True
        blocked[0] = True
        blocked[0, Lk - 1] = False
        blocked[torch.arange(Lq), torch.arange(Lq) % Lk] = False
        bits = pack_bits(blocked)
    return dict(pack_q=pack_q, pack_k=pack_k, dy=dy, blocked=blocked, bits=bits, scale=(D * nsrc) ** -0.5, C=C)


def views(pack_q, pack_k, C, nsrc):
    """(q, k, v, q2 | None, k2 | None) as column views of the packed tensors."""
    two = nsrc == 2
    return pack_q[:, :C], pack_k[:, :C], pack_k[:, 2 * C:], pack_q[:, C:] if two else None, pack_k[:, C:2 * C] if two else None


def attention64(q, k, v, H, scale, blocked=None, q2=None, k2=None, rnd=None):
    """Float64 masked softmax attention, heads = equal column slices.  rnd: operand rounding applied to scale * q, k and v."""
    Lq, Lk = q.shape[0], k.shape[0]
    r = rnd or (lambda t: t.double())
    hv = lambda t, L: t.reshape(L, H, -1)  # noqa: E731
    s = torch.einsum("qhc,khc->hqk", r(hv(q * scale, Lq)), r(hv(k, Lk)))
    if q2 is not None:
        s = s + torch.einsum("qhc,khc->hqk", r(hv(q2 * scale, Lq)), r(hv(k2, Lk)))
    if blocked is not None:
        s = s.masked_fill(blocked.unsqueeze(0), float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.einsum("hqk,khc->qhc", p, r(hv(v, Lk))).reshape(Lq, -1)
