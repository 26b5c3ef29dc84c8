"""Inputs for the direct tests of the row-chain executor (`segdino3d_amd/csrc/rowchain.hip`, `csrc/rowchain_narrow.hip`,
`csrc/rowchain_ops.h`; tests/test_gpu_rowchain_ops.py), the float64 reference of LINEAR, ATTN, MERGE and BITS2D written out from the
kernels' header comments, and Python twins of the two LINEAR dispatches (which instantiation of `rc_linear<NT, GB, NB>` the 16-row
tiles run, how `rcn_linear` splits a Linear over its waves on 4-row tiles).  LN, PE and BOX take their references, planted rows and
scale functions from tests/decoder_kernel_cases.py.  Nothing here needs a GPU; tests/test_rowchain_cases.py checks the references, the
reach of the case lists and that the fp32 evaluation of every reference passes the tolerance rule on its own.

Every reference is a function of tensors of any float dtype and computes in that dtype (float64 = the reference, float32 = the same
reference in fp32, whose error sets the bound).

Tolerance rule (`check_float`, the rule of tests/loss_kernel_cases.py and tests/decoder_kernel_cases.py): the error of an entry is
measured in units of the entry's own scale, the bound is max(8 ulp, 4 x e32) of that scale (e32: the error of the fp32 evaluation of the
reference), and no entry may be further than 2e-5 of the largest reference entry from the reference.  The kernel's output never enters
the bound.  Scales: LINEAR - the largest of |x_k w_k|, |b|, |res| summed into the entry (through the activation: `linear_scale`);
ATTN and MERGE - the largest |v| among the entry's open keys.

Exact LINEAR cases hold integers (x, w in -7 .. 7, b and res in -15 .. 15): every partial sum of any summation order is an integer
below 2^24 (the CPU test asserts it), fp32 accumulation is exact and the float64 reference is the only right answer, bit for bit
(the device of tests/conv_forward_cases.py).

ATTN logit spread: `ATTN_SPREAD` natural-log units between a row's largest and smallest logit - the largest of 8, 16, 32, 64 at which
the fp32 reference alone stays inside the rule, cap included, on every case (`spread_passes`, asserted by the CPU test)."""
import math
from functools import lru_cache

import torch

from tests import decoder_kernel_cases as K
from tests.loss_kernel_cases import CAP, FLOOR, _arr, float_bound, scaled_error

F64, F32 = torch.float64, torch.float32
PREFIX = "[rowchain-error]"
RECORDS = []
EXACT_LIMIT = 2.0 ** 24
H, DH, D = 8, 32, 256               # heads, channels of a head, d_model
ATTN_SCALE = DH ** -0.5
SPREADS = (64, 32, 16, 8)
gen = K.gen


def record(line):
    line = f"{PREFIX} {line}"
    print(line)
    RECORDS.append(line)


def check_float(family, case, got, ref64, ref32, scale=None):
    """Assert the tolerance rule and print / record the `[rowchain-error]` line.  `scale` defaults to the largest reference entry."""
    got, r64, r32 = _arr(got), _arr(ref64), _arr(ref32)
    assert got.shape == r64.shape == r32.shape, (family, case, got.shape, r64.shape, r32.shape)
    assert bool(torch.isfinite(r64).all()), (family, case, "reference not finite")
    top = float(r64.abs().max()) if r64.numel() else 0.0
    sc = torch.full_like(r64, top) if scale is None else _arr(scale).expand_as(r64) if _arr(scale).numel() == 1 else _arr(scale)
    assert sc.shape == r64.shape, (family, case, sc.shape, r64.shape)
    bound, e32 = float_bound(r64, r32, sc)
    kerr = scaled_error(got, r64, sc)
    worst = float((got - r64).abs().max()) if r64.numel() else 0.0
    record(f"{family} | {case} | kernel {kerr:.3e} | e32 {e32:.3e} | bound {bound:.3e} | abs {worst:.3e} | cap {CAP * top:.3e}")
    assert bool(torch.isfinite(got).all()), (family, case, "not finite")
    assert bool(((got - r64).abs() <= bound * sc + FLOOR).all()), (family, case, kerr, bound)
    assert worst <= CAP * top + FLOOR, (family, case, worst, CAP * top)
    return kerr, e32, bound


reference_passes = K.reference_passes


# ---- slots --------------------------------------------------------------------------------------------------------------------------------
MAX_SLOTS = 9


def nslots(width):
    """LDS slots a buffer of `width` columns spans (a slot is [rows][260] floats; wider rows have a stride of width + 4)."""
    ld = 260 if width <= 256 else width + 4
    return (16 * ld + 4159) // 4160


# ---- LINEAR: twins of the dispatches --------------------------------------------------------------------------------------------------------
INSTANTIATIONS = [(1, 4, 4), (1, 4, 8), (1, 4, 16), (1, 2, 3), (1, 4, 0), (1, 2, 0), (1, 1, 0), (2, 2, 0), (2, 1, 0), (3, 1, 32), (3, 1, 0),
                  (4, 1, 16), (4, 1, 0)]
GENERIC = [i for i in INSTANTIATIONS if i[2] == 0]


def linear_dispatch16(k, cout):
    """Twin of `rc_linear_dispatch` (csrc/rowchain.hip): -> ((NT, GB, NB), nb), nb the number of 16-MFMA blocks the body walks."""
    ct = (cout + 15) >> 4
    nt = (ct + 15) >> 4
    ng = k >> 4
    if nt <= 1:
        if ng in (16, 32, 64):
            inst = (1, 4, ng // 4)
        elif ng == 6:
            inst = (1, 2, 3)
        elif ng & 3 == 0:
            inst = (1, 4, 0)
        elif ng & 1 == 0:
            inst = (1, 2, 0)
        else:
            inst = (1, 1, 0)
    elif nt == 2:
        inst = (2, 2, 0) if ng & 1 == 0 else (2, 1, 0)
    elif nt == 3:
        inst = (3, 1, 32) if ng == 32 else (3, 1, 0)
    else:
        inst = (4, 1, 16) if ng == 16 else (4, 1, 0)
    return inst, (inst[2] if inst[2] else ng // inst[1])


def possible_nb(inst):
    """The block counts a generic instantiation can be asked for at K <= 1024 (the dispatch sends the others to another body)."""
    out = set()
    for k in range(16, 1025, 16):
        for cout in (1, 257, 513, 769):
            got, nb = linear_dispatch16(k, cout)
            if got == inst:
                out.add(nb)
    return out


def narrow_split(k, cout):
    """Twin of `rcn_linear`'s task split (csrc/rowchain_narrow.hip): -> dict(kp = K parts, pq = channel quads of a part, ntiles,
    rounds = the sizes of the `rcn_round<RQ>` calls of one task, scratch = floats of the partial sums)."""
    nq, ntiles = k >> 2, (cout + 63) >> 6
    kp = 1 if ntiles >= 8 else 2 if ntiles >= 4 else 4 if ntiles >= 2 else 8
    while nq % kp:
        kp >>= 1
    pq = nq // kp
    rounds, q = [], 0
    while pq - q >= 32:
        rounds.append(32)
        q += 32
    for rq in (16, 8, 4):
        if pq - q >= rq:
            rounds.append(rq)
            q += rq
    rounds += [1] * (pq - q)
    return dict(kp=kp, pq=pq, ntiles=ntiles, rounds=rounds, scratch=kp * 4 * ntiles * 64)


# ---- LINEAR: cases ----------------------------------------------------------------------------------------------------------------------------
# (k0, k1, cout, rows of the two scenes, res, act, option); option: None | "nodst" (dst=None, global copy only) | "inplace" (dst = src0's
# slot) | "prog4" (the same op in program 0 and program 3 of a four-program launch).  k1 > 0: two sources; k0 != k1 is built through
# Program._op.  The list reaches all 13 instantiations of the 16-row dispatch and, per generic one, every block count mod 3 it can be
# asked for plus nb = 1 and nb = 2 where the dispatch admits them (tests/test_rowchain_cases.py proves both).  A residual is a LOAD (a
# multiple of 4 columns) into a slot whose row stride is that of the Linear's output: with more than 256 columns the two agree only
# when cout itself is a multiple of 4, so the wide cases with a residual are.
LINEAR_EXACT = [
    # <1,4,4> / <1,4,8> / <1,4,16> / <1,2,3>: the decoder's own bodies
    (256, 0, 256, (17, 37), True, None, None), (256, 0, 199, (1, 16), False, "relu", None), (256, 0, 3, (15, 1), False, None, "nodst"),
    (256, 0, 1, (16, 17), False, None, None), (128, 128, 256, (37, 15), False, None, None), (256, 256, 256, (16, 1), True, "relu", None),
    (512, 0, 15, (17, 16), False, None, None), (1024, 0, 256, (37, 1), True, None, None), (1024, 0, 17, (1, 15), False, None, "prog4"),
    (96, 0, 256, (15, 17), False, "relu", None), (256, 0, 256, (37, 16), False, None, "inplace"),
    # <1,4,0>: nb = 1, 2, 3, 5
    (64, 0, 16, (1, 37), False, None, None), (128, 0, 17, (16, 15), True, None, None), (192, 0, 256, (17, 1), False, "relu", None),
    (160, 160, 199, (15, 16), False, None, None), (64, 0, 100, (17, 15), False, None, "inplace"),
    # <1,2,0>: nb = 1, 5, 7, 9 (nb is odd here: an even count of 32-channel blocks is a multiple of 64 channels)
    (32, 0, 15, (37, 1), False, None, None), (160, 0, 199, (16, 17), True, None, None), (224, 0, 256, (1, 15), False, None, None),
    (144, 144, 3, (15, 37), False, "relu", None),
    # <1,1,0>: nb = 1, 3, 5, 7
    (16, 0, 1, (17, 16), False, None, None), (48, 0, 32, (1, 37), True, None, None), (80, 0, 3, (16, 15), False, None, "nodst"),
    (64, 48, 256, (37, 17), False, None, None),
    # <2,2,0>: nb = 1, 2, 3, 5, 8
    (32, 0, 257, (15, 1), False, None, None), (64, 0, 272, (17, 37), True, "relu", None), (96, 0, 400, (16, 16), False, None, None),
    (160, 0, 512, (1, 17), False, None, "prog4"), (256, 0, 512, (37, 15), True, None, None), (96, 32, 400, (15, 17), False, None, None),
    # <2,1,0>: nb = 1, 3, 5 (odd by the dispatch)
    (16, 0, 512, (16, 37), False, None, None), (48, 0, 257, (17, 1), False, None, None), (80, 0, 400, (1, 16), True, "relu", None),
    (272, 0, 272, (15, 15), False, None, "inplace"),
    # <3,1,32> and <3,1,0>: nb = 1, 2, 3, 5, 16, 64
    (256, 256, 768, (37, 17), False, None, None), (512, 0, 513, (1, 15), False, None, None), (16, 0, 513, (16, 1), False, None, None),
    (32, 0, 768, (15, 37), True, "relu", None), (48, 0, 600, (17, 16), True, None, None), (80, 0, 513, (1, 17), False, None, "nodst"),
    (256, 0, 768, (16, 15), False, None, None), (1024, 0, 768, (17, 1), False, None, None),
    # <4,1,16> and <4,1,0>: nb = 1, 2, 3, 5, 32, 64
    (256, 0, 1024, (15, 16), True, "relu", None), (256, 0, 769, (37, 1), False, None, None), (16, 0, 769, (1, 37), False, None, None),
    (32, 0, 1024, (17, 15), True, None, None), (48, 0, 769, (16, 17), False, None, None), (80, 0, 1024, (15, 1), False, None, "prog4"),
    (512, 0, 1024, (1, 16), False, None, None), (1024, 0, 1024, (37, 17), False, None, None), (128, 0, 1024, (16, 37), False, None, None),
]
# float cases under `check_float`: every activation; row 1 of scene 0 is scaled by 1e3 next to rows of scale 1
LINEAR_FLOAT = [
    (256, 0, 256, (17, 5), True, "gelu", None), (96, 0, 199, (5, 16), False, "sigmoid", None), (48, 0, 260, (16, 3), True, "relu", None),
    (128, 128, 272, (3, 17), False, None, None), (160, 0, 17, (17, 4), False, "gelu", "inplace"), (512, 0, 64, (5, 5), True, "sigmoid", None),
    (80, 0, 513, (4, 17), False, "gelu", None), (64, 0, 769, (17, 2), False, None, None),
]
LINEAR_K = [16, 32, 48, 64, 80, 96, 128, 160, 256, 512, 1024]
LINEAR_COUT = [1, 3, 15, 16, 17, 199, 256, 257, 272, 400, 512, 513, 768, 769, 1024]
LINEAR_ROWS = [1, 15, 16, 17, 37]
ACTS = [None, "relu", "gelu", "sigmoid"]


def linear_id(c):
    k0, k1, cout, rows, res, act, opt = c
    return f"k{k0}+{k1}-c{cout}-r{rows[0]}+{rows[1]}" + ("-res" if res else "") + (f"-{act}" if act else "") + (f"-{opt}" if opt else "")


def linear_slots(c):
    """Slot plan of a case: dict(src0, src1, res, dst, n_slots); fails when the shape does not fit the 9 slots of a workgroup."""
    k0, k1, cout, _, res, _, opt = c
    at, plan = 0, {}
    plan["src0"] = at
    at += nslots(k0)
    plan["src1"] = None
    if k1:
        plan["src1"] = at
        at += nslots(k1)
    plan["res"] = None
    if res:
        plan["res"] = at
        at += nslots(cout)
    if opt == "inplace":
        plan["dst"] = plan["src0"]
        at = max(at, nslots(cout))
    elif opt == "nodst":
        plan["dst"] = None
    else:
        plan["dst"] = at
        at += nslots(cout)
    assert at <= MAX_SLOTS, (linear_id(c), at)
    plan["n_slots"] = max(at, 1)
    return plan


@lru_cache(maxsize=None)
def linear_case(c, exact):
    k0, k1, cout, rows, res, act, opt = c
    n, k = sum(rows), k0 + k1
    g = gen(71, k0, k1, cout, rows[0], rows[1], int(exact))
    if exact:
        ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()  # noqa: E731
        x, w, b = ri(-7, 7, n, k), ri(-7, 7, cout, k), ri(-15, 15, cout)
        r = ri(-15, 15, n, cout) if res else None
    else:
        x, w, b = torch.randn(n, k, generator=g), torch.randn(cout, k, generator=g) / math.sqrt(k), torch.randn(cout, generator=g)
        r = torch.randn(n, cout, generator=g) if res else None
        if n > 1:
            x[1] *= 1e3
            if r is not None:
                r[1] *= 1e3
    return dict(x=x, w=w, b=b, res=r, k0=k0, k1=k1, cout=cout, rows=rows, act=act, opt=opt, n=n)


def act_ref(t, act):
    if act == "relu":
        return torch.relu(t)
    if act == "gelu":
        return 0.5 * t * (1 + torch.erf(t / math.sqrt(2.0)))
    if act == "sigmoid":
        return 1 / (1 + torch.exp(-t))
    return t


def linear_ref(x, w, b, res, act):
    """act([x0 | x1] W^T + b + res); x holds the concatenated sources."""
    y = x @ w.T
    if b is not None:
        y = y + b
    if res is not None:
        y = y + res
    return act_ref(y, act)


def linear_scale(x, w, b, res, act):
    """The largest of |x_k w_k|, |b|, |res| summed into the entry.  Through an activation: relu and gelu pass an error of their
    argument on with a slope of at most 1.13 and round their own value (max with |y|); sigmoid's slope is s (1 - s) and its value s."""
    x, w = x.double(), w.double()
    top = torch.stack([(x[i].abs()[None, :] * w.abs()).amax(1) for i in range(x.shape[0])])
    if b is not None:
        top = torch.maximum(top, b.double().abs().expand_as(top))
    if res is not None:
        top = torch.maximum(top, res.double().abs())
    if act == "sigmoid":
        s = linear_ref(x, w, None if b is None else b.double(), None if res is None else res.double(), "sigmoid")
        return torch.maximum(s, s * (1 - s) * top)
    if act == "gelu":
        return 1.13 * top
    return top


def exact_magnitude(c):
    """Upper bound of every partial sum of an exact case, whatever the order: sum |x| |w| + |b| + |res|."""
    m = c["x"].double().abs() @ c["w"].double().abs().T + c["b"].double().abs()
    if c["res"] is not None:
        m = m + c["res"].double().abs()
    return float(m.max())


# ---- ATTN ---------------------------------------------------------------------------------------------------------------------------------------
def attn_ref(q, k, v, scale, open_=None):
    """Masked softmax per head: q [n, 256] (q * scale first, the kernel's operand convention), k / v [Lk, 256], open_ bool [n, Lk]
    (None: every key open) - blocked keys get -inf.  Every row has an open key."""
    n, Lk = q.shape[0], k.shape[0]
    s = torch.einsum("qhc,khc->hqk", (q * scale).view(n, H, DH), k.view(Lk, H, DH))
    if open_ is not None:
        s = s.masked_fill(~open_[None], float("-inf"))
    p = torch.softmax(s, -1)
    return torch.einsum("hqk,khc->qhc", p, v.view(Lk, H, DH)).reshape(n, D)


def attn_scale(v, open_, n):
    """The largest |v| among the entry's open keys -> [n, 256]."""
    a = v.double().abs()
    if open_ is None:
        return a.amax(0)[None, :].expand(n, D).contiguous()
    return torch.stack([a[open_[i]].amax(0) for i in range(n)])


def logits(q, k, scale):
    n, Lk = q.shape[0], k.shape[0]
    return torch.einsum("qhc,khc->hqk", (q.double() * scale).view(n, H, DH), k.double().view(Lk, H, DH))


ATTN_LK = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129]
ATTN_NQ = [1, 3, 4, 5, 16, 17]
ATTN_LK_MAX = 1024                  # decoder.FUSED_SA_MAX_KEYS
# masked 2D path: two scenes (nq, Lk = nm) per launch; every Lk of ATTN_LK, every nq of ATTN_NQ, Lk = 1024 once
ATTN_2D = [((1, 1), (17, 15)), ((3, 16), (16, 17)), ((4, 31), (5, 32)), ((5, 33), (1, 63)), ((16, 64), (3, 65)), ((17, 129), (4, 17)),
           ((17, ATTN_LK_MAX), (5, 33))]
# self-attention: Lk = nq, the scene's own rows
ATTN_SELF = [(1, 15), (16, 17), (31, 32), (33, 63), (64, 65), (129, 3), (4, 5)]


def rescale_spread(q, k, scale, open_, spread):
    """Scale q so that the widest row (largest minus smallest OPEN logit over heads and rows) spans `spread` natural-log units."""
    s = logits(q, k, scale)
    if open_ is not None:
        hi = s.masked_fill(~open_[None], float("-inf")).amax(-1)
        lo = s.masked_fill(~open_[None], float("inf")).amin(-1)
    else:
        hi, lo = s.amax(-1), s.amin(-1)
    width = float((hi - lo).max())
    return q * (spread / width) if width > 0 else q


def plant_open(nq, Lk, g):
    """bool [nq, Lk] with the dummy key Lk - 1 always open, random elsewhere, and the planted rows (as many as fit): row 0 - only the dummy
    key; row 1 - a whole 64-key tile (keys 64 .. 127) and a whole 16-key tile (16 .. 31) blocked between open ones; row 2 - every open
    key in the first half of the 16-key tiles; row 3 - every open key (but the dummy) in the second half."""
    o = torch.rand(nq, Lk, generator=g) < 0.5
    o[:, Lk - 1] = True
    ntiles = (Lk + 15) // 16
    mid = ((ntiles + 1) // 2) * 16
    o[0, :Lk - 1] = False
    if nq > 1:
        o[1, :16] = True
        o[1, 16:32] = False
        o[1, 64:128] = False
        if Lk > 128:
            o[1, 128:] = True
    if nq > 2 and mid < Lk - 1:
        o[2, mid:Lk - 1] = False
        o[2, 0] = True
    if nq > 3 and mid < Lk - 1:
        o[3, :mid] = False
        o[3, mid] = True
    o[:, Lk - 1] = True                                         # (the blocked tiles of row 1 may hold it)
    return o


@lru_cache(maxsize=None)
def attn_case(nq, Lk, masked, spread, seed=0):
    """One scene: q [nq, 256], k, v [Lk, 256], open_ (masked) or None.  Planted logits: row nq - 1, head 0 is dominated by key 0 (first
    tile), head 1 by the last key (last tile of the second half) - 4 units above the runner-up of unit-variance logits; THEN q is
    scaled so that the widest row of the case spans exactly `spread`: no row spans more."""
    g = gen(83, nq, Lk, int(masked), seed)
    q, k, v = (torch.randn(n, D, generator=g) for n in (nq, Lk, Lk))
    v[:, ::7] *= 50.0                                           # columns of unequal size: the scale of an entry is its own column's
    open_ = plant_open(nq, Lk, g) if masked else None
    r = nq - 1
    for head, key in ((0, 0), (1, Lk - 1)):
        if open_ is not None:
            open_[r, key] = True
        sl = slice(head * DH, (head + 1) * DH)
        qr = q[r, sl].double()
        nrm = float(qr.norm())
        s = logits(q[r:r + 1], k, ATTN_SCALE)[head, 0]
        if open_ is not None:
            s = s.masked_fill(~open_[r], float("-inf"))
        others = torch.cat([s[:key], s[key + 1:]])
        want = (float(others.max()) if others.numel() and bool(torch.isfinite(others).any()) else 0.0) + 4.0
        kk = k[key, sl].double()
        kk = kk + (want - float(s[key])) / (ATTN_SCALE * nrm * nrm) * qr       # moves this key's logit of row r, head `head` to `want`
        k[key, sl] = kk.float()
    q = rescale_spread(q, k, ATTN_SCALE, open_, spread).float()
    return dict(q=q, k=k, v=v, open=open_, nq=nq, Lk=Lk)


def spread_passes(spread, cases):
    """Does the fp32 reference alone pass the rule (cap included) on every (nq, Lk, masked) of `cases` at this spread?"""
    for nq, Lk, masked in cases:
        c = attn_case(nq, Lk, masked, spread)
        r64 = attn_ref(c["q"].double(), c["k"].double(), c["v"].double(), ATTN_SCALE, c["open"])
        r32 = attn_ref(c["q"], c["k"], c["v"], ATTN_SCALE, c["open"])
        try:
            reference_passes(r64, r32, attn_scale(c["v"], c["open"], nq))
        except AssertionError:
            return False
    return True


def attn_shapes():
    out = [(nq, Lk, True) for pair in ATTN_2D for nq, Lk in pair]
    out += [(n, n, False) for pair in ATTN_SELF for n in pair]
    return sorted(set(out))


ATTN_SPREAD = 64                  # chosen by tests/test_rowchain_cases.py::test_attention_spread_is_the_largest_the_fp32_reference_passes


# ---- BITS2D -------------------------------------------------------------------------------------------------------------------------------------
def bits2d_ref(open_, near):
    """open_ bool [Q, S] (superpoint open for the query), near bool [Mq, S] -> blocked bool [Q, Mq + 1]: bit m is blocked when no
    superpoint is both open for the query and near key m; the appended dummy key Mq is always open."""
    hit = (open_.double() @ near.double().T) > 0 if near.shape[0] else torch.zeros(open_.shape[0], 0, dtype=torch.bool)
    return torch.cat([~hit, torch.zeros(open_.shape[0], 1, dtype=torch.bool)], 1)


def pack_bits(m, words, fill):
    """bool [R, S] -> int32 words [R, words], little-endian bits, padding bits = fill (blocked rows: 1, near rows: 0, as in
    tests/test_gpu_decoder.py::test_dinox_mask_bits_sizes)."""
    full = torch.full((m.shape[0], words * 32), bool(fill), dtype=torch.bool)
    full[:, :m.shape[1]] = m
    w = (full.view(m.shape[0], words, 32).long() << torch.arange(32)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


BITS_NW = [1, 63, 64, 65, 127, 128, 129, 130, 200]
BITS_NM = [1, 2, 16, 17, 32, 33, 48, 65]
# two scenes (nq, nw, nm) per launch; S = 32 nw (the last bit of the last word is a superpoint) in scene 0, 32 nw - 5 in scene 1
BITS_LAUNCHES = [((5, 1, 1), (18, 63, 2)), ((18, 64, 16), (5, 65, 17)), ((6, 127, 32), (17, 128, 33)), ((17, 129, 48), (6, 130, 65)),
                 ((5, 200, 65), (18, 128, 17)), ((18, 129, 2), (5, 1, 33)), ((4, 130, 17), (9, 200, 48))]


@lru_cache(maxsize=None)
def bits_case(nq, nw, nm, full_last_word, seed=0):
    """open_ [nq, S], near [nm - 1, S] with, as far as they fit: query 0 - nothing open; query 1 / key 0 - a hit carried only by the last
    superpoint (the last bit of the last word when S = 32 nw); query 2 / key 1 - only by a bit of word 64; query 3 / key 2 - only
    by a bit of word 128.  Each planted key is near its planted superpoint alone and no other query opens that superpoint, so the hit
    is in exactly one (query, key) entry."""
    S = 32 * nw - (0 if full_last_word else 5)
    Mq = nm - 1
    g = gen(97, nq, nw, nm, seed)
    open_ = torch.rand(nq, S, generator=g) < 0.03
    near = torch.rand(Mq, S, generator=g) < 0.02
    open_[0] = False
    planted = []
    spots = [(1, 0, S - 1)] + ([(2, 1, 64 * 32 + 3)] if nw > 64 else []) + ([(3, 2, 128 * 32 + 30)] if nw > 128 else [])
    for qi, mi, s in spots:
        if qi < nq and mi < Mq and s < S:
            open_[:, s] = False
            near[:, s] = False
            open_[qi] = False
            near[mi] = False
            open_[qi, s] = True
            near[mi, s] = True
            planted.append((qi, mi, s))
    return dict(open=open_, near=near, S=S, nw=nw, nm=nm, nq=nq, planted=planted)


def key_table(nm, shift=0):
    """V [nm, 256] with V[key, (key + shift) % 256] = 1: head h's 32 channels show keys 32 h .. 32 h + 31 (nm <= 256), so with equal logits
    the attention output of a query is 1 / (its open keys) exactly at its open keys and 0 elsewhere."""
    assert nm <= D
    v = torch.zeros(nm, D)
    v[torch.arange(nm), (torch.arange(nm) + shift) % D] = 1.0
    return v


# ---- MERGE ------------------------------------------------------------------------------------------------------------------------------------
PART = 64 + 32 * DH                 # floats of one partial state: m [32], l [32], O [32 dv][32 queries]


def merge_ref(m, l, o):
    """m, l [Z, n, H] (log2 domain), o [Z, n, H, 32] -> [n, 256]: sum_z O_z 2^(m_z - M) / sum_z l_z 2^(m_z - M), M = max_z m_z; a split
    with m_z = -inf (every key blocked) contributes nothing."""
    M = m.amax(0, keepdim=True)
    f = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - M))
    L = (l * f).sum(0)
    return ((o * f[..., None]).sum(0) / L[..., None]).reshape(m.shape[1], D)


@lru_cache(maxsize=None)
def merge_case(nq, Lk, ksplit, seed=0):
    """Partial softmax states of a masked attention whose Lk keys are cut into `ksplit` runs, computed in float64 and rounded to fp32
    (m, l, O as attention.hip's key splits leave them).  Row 0 has every key of split 0 blocked (m_0 = -inf, l_0 = 0, O_0 = 0)."""
    g = gen(101, nq, Lk, ksplit, seed)
    q, k, v = (torch.randn(n, D, generator=g) for n in (nq, Lk, Lk))
    v[:, ::5] *= 20.0
    open_ = torch.rand(nq, Lk, generator=g) < 0.6
    open_[:, Lk - 1] = True
    run = -(-Lk // ksplit)
    if ksplit > 1:
        open_[0, :run] = False
    s = logits(q, k, ATTN_SCALE) * math.log2(math.e)
    s = s.masked_fill(~open_[None], float("-inf")).permute(1, 0, 2)                    # [n, H, Lk]
    vv = v.double().view(Lk, H, DH)
    ms, ls, os_ = [], [], []
    for z in range(ksplit):
        sz = s[:, :, z * run:(z + 1) * run]
        mz = sz.amax(-1)
        p = torch.where(torch.isinf(sz), torch.zeros_like(sz), torch.exp2(sz - torch.where(torch.isinf(mz), torch.zeros_like(mz), mz)[..., None]))
        ms.append(mz)
        ls.append(p.sum(-1))
        os_.append(torch.einsum("nhk,khc->nhc", p, vv[z * run:(z + 1) * run]))
    m, l, o = torch.stack(ms).float(), torch.stack(ls).float(), torch.stack(os_).float()
    return dict(m=m, l=l, o=o, v=v, open=open_, nq=nq, ksplit=ksplit)


def merge_pack(c):
    """The workspace layout MERGE reads: [32-query block][head][split][m 32 | l 32 | O dv x 32 queries] floats; the queries past the
    scene's end in its last block hold NaN (never read)."""
    nq, Z = c["nq"], c["ksplit"]
    nb = (nq + 31) // 32
    ws = torch.full((nb, H, Z, PART), float("nan"))
    for z in range(Z):
        for bx in range(nb):
            rows = slice(bx * 32, min(nq, bx * 32 + 32))
            n = rows.stop - rows.start
            ws[bx, :, z, :n] = c["m"][z, rows].T
            ws[bx, :, z, 32:32 + n] = c["l"][z, rows].T
            ws[bx, :, z, 64:].view(H, DH, 32)[:, :, :n] = c["o"][z, rows].permute(1, 2, 0)
    return ws.reshape(-1)


# ---- LN / PE / BOX: the planted cases of tests/decoder_kernel_cases.py laid over two scenes ------------------------------------------------------
SMALL_ROWS = [1, 4, 5, 16, 17, 45]
SECOND_SCENE_ROWS = 6


def scene_rows(rows):
    """Two scenes: `rows` rows of scene 0 and SECOND_SCENE_ROWS rows of scene 1 -> (n, rng_rows [n, 6], ranges [2, 6])."""
    n = rows + SECOND_SCENE_ROWS
    which = torch.cat([torch.zeros(rows, dtype=torch.long), torch.ones(SECOND_SCENE_ROWS, dtype=torch.long)])
    return n, K.SCENE_RANGES[which].contiguous(), K.SCENE_RANGES[:2].contiguous()


def pe_rows(rows):
    """`pe_case(n)` with each row moved into its own scene's range (the same position relative to it, points outside the range included)."""
    n, rng_rows, ranges = scene_rows(rows)
    p = dict(K.pe_case(n))
    u = (p["xyz"] - p["rng_rows"][:, :3]) / (p["rng_rows"][:, 3:] - p["rng_rows"][:, :3])
    p["xyz"] = (rng_rows[:, :3] + u * (rng_rows[:, 3:] - rng_rows[:, :3])).contiguous()
    p["rng_rows"], p["ranges"] = rng_rows, ranges
    return p


def box_rows(rows):
    n, rng_rows, ranges = scene_rows(rows)
    c = dict(K.box_case(n))
    c["rng_rows"], c["ranges"] = rng_rows, ranges
    return c
