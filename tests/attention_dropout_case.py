"""The keep mask of attention dropout restated in numpy (csrc/attention.h is the definition the kernels share), and the
float64 reference of attention with that mask applied to the probabilities.

Element (head, q, k) of attention number `call`: Philox4x32-10 keyed by two uint32 words with the counter (k >> 2, q, head, call);
the element takes output word k & 3 and is kept iff that word >= floor(p 2^32).  Kept probabilities are scaled by 1 / (1 - p)."""
import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
# the key of the statistical checks and of the GPU tests (two uint32 words; int32 on the device)
KEY = (0x243F6A88, 0x85A308D3)


def philox4x32_10(counter, key):
    """counter: four arrays (or scalars) of uint32 values, key: two -> four uint64 arrays holding the uint32 output words."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)        # 32 x 32 -> 64 bit, exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def threshold(p):
    return int(float(np.float32(p)) * 2.0 ** 32)


def keep_mask(key, call, H, Lq, Lk, p):
    """bool [H, Lq, Lk]: True = kept."""
    nblk = (Lk + 3) // 4
    head, q, kblk = np.meshgrid(np.arange(H), np.arange(Lq), np.arange(nblk), indexing="ij")
    words = philox4x32_10((kblk, q, head, np.full_like(kblk, call)), key)
    w = np.stack(words, axis=-1).reshape(H, Lq, nblk * 4)[:, :, :Lk]
    return w >= np.uint64(threshold(p))


def key_tensor(key, device):
    """two uint32 words -> the int32 tensor the library reads"""
    return torch.tensor(np.array(key, dtype=np.uint32).view(np.int32), dtype=torch.int32, device=device)


def attention64_dropout(q, k, v, H, scale, keep, p, blocked=None, q2=None, k2=None, rnd=None):
    """`attention_heads_case.attention64` with the keep mask applied to its probabilities: softmax first (normalised before the drop),
    then c K o P with c = 1 / (1 - p) as the kernels form it in fp32.  rnd: operand rounding applied to scale * q, k and v."""
    Lq, Lk = q.shape[0], k.shape[0]
    r = rnd or (lambda t: t.double())
    hv = lambda t, L: t.reshape(L, H, -1)  # noqa: E731
    s = torch.einsum("qhc,khc->hqk", r(hv(q * scale, Lq)), r(hv(k, Lk)))
    if q2 is not None:
        s = s + torch.einsum("qhc,khc->hqk", r(hv(q2 * scale, Lq)), r(hv(k2, Lk)))
    if blocked is not None:
        s = s.masked_fill(blocked.unsqueeze(0), float("-inf"))
    c = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    pr = torch.softmax(s, dim=-1) * (torch.as_tensor(keep).to(torch.float64) * c)
    return torch.einsum("hqk,khc->qhc", pr, r(hv(v, Lk))).reshape(Lq, -1)
