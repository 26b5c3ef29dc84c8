"""Inputs for the direct tests of the decoder's small kernels in `segdino3d_amd/csrc/dense.hip` and `csrc/train_dec.hip`
(tests/test_gpu_decoder_kernels.py) and the float64 reference of every one of them, written out from the formula in the kernel's header
comment: LayerNorm forward / backward, the activation derivatives, column sums, the sine and Fourier positional encodings (one scene and
the rows of several), the box modulation's gradient, box refinement forward / backward, the batched transpose.

Inputs are seeded fp32 CPU tensors, so their float64 copies are exact; every reference takes tensors of any float dtype and computes in
that dtype (float64 = the reference, float32 = the same reference evaluated in fp32, whose error sets the bound).  The PE references and
`inverse_sigmoid` are cross-checked against `oracle/decoder_ref.py`, the others against float64 autograd, by
tests/test_decoder_kernel_cases.py on the CPU; nothing here needs a GPU.

Tolerance rule (`check_float`, the rule of tests/loss_kernel_cases.py): an error is measured in units of the entry's own scale - the
largest magnitude among the terms that are summed into it, taken from the float64 reference (each `*_scale` function says which terms).
The bound is max(8 ulp of fp32, 4 x e32) of that scale, e32 being the error of the same reference evaluated in fp32 on the CPU; on top
of it no entry may be further than 2e-5 of the largest reference entry from the reference.  The kernel's own output never enters.
Column sums have a derived bound instead (`col_sum_bound`).

Scene ranges have a positive extent in every axis; a zero extent (division by zero in the normalisation) is out of scope here."""
import math
from functools import lru_cache

import torch

from oracle import decoder_ref as D
from tests.loss_kernel_cases import CAP, FLOOR, _arr, float_bound, scaled_error

F64, F32 = torch.float64, torch.float32
U = 2.0 ** -24                      # unit roundoff of fp32
DENORM = 2.0 ** -149                # smallest positive fp32 denormal
TEMPERATURE = 10000.0               # ScanNetQueryDecoder's default
RECORDS = []


def gen(*seed):
    v = 0
    for s in seed:
        v = (v * 1000003 + int(s)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(v)


# ---- the tolerance rule -----------------------------------------------------------------------------------------------------------------
def check_float(family, case, got, ref64, ref32, scale=None):
    """Assert the tolerance rule and print / record the `[decoder-kernel-error]` line.  `scale` defaults to the largest reference entry."""
    got, r64, r32 = _arr(got), _arr(ref64), _arr(ref32)
    assert got.shape == r64.shape == r32.shape, (family, case, got.shape, r64.shape, r32.shape)
    assert bool(torch.isfinite(r64).all()), (family, case, "reference not finite")
    top = float(r64.abs().max()) if r64.numel() else 0.0
    sc = torch.full_like(r64, top) if scale is None else _arr(scale).expand_as(r64) if _arr(scale).numel() == 1 else _arr(scale)
    assert sc.shape == r64.shape, (family, case, sc.shape, r64.shape)
    bound, e32 = float_bound(r64, r32, sc)
    kerr = scaled_error(got, r64, sc)
    worst = float((got - r64).abs().max()) if r64.numel() else 0.0
    line = f"[decoder-kernel-error] {family} | {case} | kernel {kerr:.3e} | e32 {e32:.3e} | bound {bound:.3e} | abs {worst:.3e} | cap {CAP * top:.3e}"
    print(line)
    RECORDS.append(line)
    assert bool(torch.isfinite(got).all()), (family, case, "not finite")
    assert bool(((got - r64).abs() <= bound * sc + FLOOR).all()), (family, case, kerr, bound)      # entries of scale 0: exact
    assert worst <= CAP * top + FLOOR, (family, case, worst, CAP * top)
    return kerr, e32, bound


def reference_passes(ref64, ref32, scale=None):
    """The fp32 evaluation of the reference against the rule (CPU test: the reference alone passes) -> (e32, largest abs error, cap)."""
    r64, r32 = _arr(ref64), _arr(ref32)
    top = float(r64.abs().max()) if r64.numel() else 0.0
    sc = torch.full_like(r64, top) if scale is None else _arr(scale).expand_as(r64) if _arr(scale).numel() == 1 else _arr(scale)
    bound, e32 = float_bound(r64, r32, sc)
    worst = float((r32 - r64).abs().max()) if r64.numel() else 0.0
    assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all())
    assert bool(((r32 - r64).abs() <= bound * sc + FLOOR).all())
    assert worst <= CAP * top + FLOOR, (worst, CAP * top)
    return e32, worst, CAP * top


def check_bound(family, case, got, ref64, bound):
    """Derived absolute bound per entry (column sums)."""
    got, r64, b = _arr(got), _arr(ref64), _arr(bound)
    err = (got - r64).abs()
    ratio = float((err / b.clamp(min=1e-300)).max())
    line = f"[decoder-kernel-error] {family} | {case} | abs {float(err.max()):.3e} | derived bound {float(b[err.argmax()]):.3e} | error / bound {ratio:.3e}"
    print(line)
    RECORDS.append(line)
    assert bool(torch.isfinite(got).all()) and bool((err <= b).all()), (family, case, ratio)
    return ratio


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------------
LN_M = [1, 3, 4, 5, 201]            # one wave per row, 4 rows per workgroup
LN_D = [4, 96, 252, 256, 260, 1020, 1024]      # 4 x 64 lanes x float4
LN_M_SUMS = [8191, 8192, 8193]      # at D = 8: the column sums of dw / db switch paths at 8192 rows
EPS = 1e-5


@lru_cache(maxsize=None)
def ln_case(M, D, planted=True):
    """x, res, w, b, dy [M, D] / [D]; with `planted`: the last row of x (and of x + res) has mean 1e3 and spread 1 - the variance must
    not cancel - and row 0 is constant (x = 1.75, x + res = 3: variance 0, x - mean exactly 0 in fp32 too, so the output is b).
    The big row is 1000 +- k / 8 in shuffled pairs: fp32 holds x + res, every partial sum of the row and its mean (1000) exactly, so
    what the row tests is the variance - a one-pass E[x^2] - mean^2 loses it entirely (x^2 needs 26 bits).  A generic 1000 + randn row
    tests something else: x + res and the mean are then rounded to ulp(1000) / 2 = 3e-5 by ANY fp32 LayerNorm, which by itself is
    outside the 2e-5 cap on O(1) outputs (this reference in fp32: 5.3e-5 against a cap of 4.9e-5 at M = 5, D = 96)."""
    g = gen(11, M, D)
    c = dict(M=M, D=D, x=torch.randn(M, D, generator=g), res=torch.randn(M, D, generator=g), w=1 + 0.1 * torch.randn(D, generator=g),
             b=0.1 * torch.randn(D, generator=g), dy=torch.randn(M, D, generator=g))
    c["big"], c["const"] = None, None
    if planted:
        c["big"] = M - 1
        for key, base, spread in (("x", 1000.0, 1.0), ("res", 0.0, 0.25)):
            half = torch.round(8 * spread * torch.randn(D // 2, generator=g)) / 8
            c[key][M - 1] = base + torch.cat([half, -half])[torch.randperm(D, generator=g)]
        if M >= 3:
            c["const"] = 0
            c["x"][0] = 1.75
            c["res"][0] = 1.25                                  # x + res = 3 exactly; x alone = 1.75
    return c


def layernorm_ref(x, res, w, b, eps=EPS, relu=False):
    """y = act(LN(x + res) * w + b): mean and (biased) variance over the row, two passes."""
    v = x if res is None else x + res
    mean = v.mean(1, keepdim=True)
    var = ((v - mean) ** 2).mean(1, keepdim=True)
    y = (v - mean) / torch.sqrt(var + eps) * w + b
    return torch.relu(y) if relu else y


def layernorm_scale(x, res, w, b, eps=EPS):
    """Terms summed into an entry: x, res and the row mean, each times rstd |w|, and b."""
    x, w, b = x.double(), w.double(), b.double()
    v = x if res is None else x + res.double()
    mean = v.mean(1, keepdim=True)
    k = w.abs() / torch.sqrt(((v - mean) ** 2).mean(1, keepdim=True) + eps)
    top = torch.maximum(x.abs(), mean.abs())
    if res is not None:
        top = torch.maximum(top, res.double().abs())
    return torch.maximum(top * k, b.abs().expand_as(x))


def plant_relu_mask(y):
    """A forward output for the backward's ReLU mask with +0, -0 and the smallest denormal in it (when the row is long enough):
    only the denormal lets the gradient through."""
    y = y.clone()
    flat = y.view(-1)
    spots = {}
    for i, (name, v) in enumerate((("zero", 0.0), ("minus_zero", -0.0), ("denormal", DENORM))):
        if i < flat.numel():
            flat[i] = v
            spots[name] = i
    return y, spots


def layernorm_bwd_ref(dy, y, x, res, w, eps=EPS):
    """-> (dxin, dw, db, g, g * xhat); y (the forward output) masks dy where the fused ReLU was off: y > 0 passes."""
    v = x if res is None else x + res
    g = dy if y is None else torch.where(y > 0, dy, torch.zeros_like(dy))
    mean = v.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(((v - mean) ** 2).mean(1, keepdim=True) + eps)
    xh = (v - mean) * rstd
    gw = g * w
    a, bb = gw.mean(1, keepdim=True), (gw * xh).mean(1, keepdim=True)
    dxin = rstd * (gw - a - xh * bb)
    return dxin, (g * xh).sum(0), g.sum(0), g, g * xh


def layernorm_bwd_scale(dy, y, x, res, w, eps=EPS):
    """dxin: the terms g w (its own and the row mean's) and xhat times the row mean's terms g w xhat, each times rstd."""
    dy, x, w = dy.double(), x.double(), w.double()
    v = x if res is None else x + res.double()
    g = dy if y is None else torch.where(y.double() > 0, dy, torch.zeros_like(dy))
    mean = v.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(((v - mean) ** 2).mean(1, keepdim=True) + eps)
    xh = (v - mean) * rstd
    gw = (g * w).abs()
    return rstd * torch.maximum(gw.amax(1, keepdim=True).expand_as(x), xh.abs() * (gw * xh.abs()).amax(1, keepdim=True))


def layernorm_sums_bound(dy, y, x, res, w, eps=EPS):
    """Derived bounds of (dw, db): column sums over M rows through `sd3d_col_sums` (chain `col_sum_chain(M)`) of addends that are exact
    (g, for db) or carry the fp32 rounding of xhat = (v - mean) rstd (g xhat, for dw): at most 8 roundings of the row's largest
    |v| rstd - the subtraction of the mean is where they are absolute, not relative."""
    dy, x = dy.double(), x.double()
    v = x if res is None else x + res.double()
    g = dy if y is None else torch.where(y.double() > 0, dy, torch.zeros_like(dy))
    mean = v.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(((v - mean) ** 2).mean(1, keepdim=True) + eps)
    xh = (v - mean) * rstd
    big = torch.maximum(v.abs().amax(1, keepdim=True), mean.abs()) * rstd
    L = col_sum_chain(x.shape[0])
    dw = U * (L * (g * xh).abs().sum(0) + 8 * (g.abs() * torch.maximum(xh.abs(), big)).sum(0))
    db = U * L * g.abs().sum(0)
    return dw + FLOOR, db + FLOOR


# ---- activation derivatives -------------------------------------------------------------------------------------------------------------
ACTS = [None, "relu", "gelu", "sigmoid"]
ACT_SHAPES = [(1, 1, 32), (5, 3, 32), (37, 199, 224), (200, 256, 256), (3, 33, 64)]        # (M, C, C_pad); 256 threads over M x C_pad
GELU_Z = [0.0, 1e-4, -1e-4, 1.0, -1.0, 5.0, -5.0, 10.0, -10.0, 40.0, -40.0]
SIGMOID_Y = [0.0, 1.0, 1e-7, 1.0 - 2.0 ** -24]
RELU_REF = [0.0, -0.0, DENORM]


@lru_cache(maxsize=None)
def act_case(act, M, C):
    """dy, ref [M, C]; ref is what `sd3d_act_backward` wants per activation (forward output for relu / sigmoid, pre-activation for
    gelu) with the decisive values planted at the front (as many as fit)."""
    g = gen(23, ACTS.index(act), M, C)
    dy = torch.randn(M, C, generator=g)
    z = 2.0 * torch.randn(M, C, generator=g)
    if act == "relu":
        ref, plant = torch.relu(z), RELU_REF
    elif act == "sigmoid":
        ref, plant = torch.sigmoid(z), SIGMOID_Y
    else:
        ref, plant = z, GELU_Z if act == "gelu" else []
    flat = ref.view(-1)
    n = min(len(plant), flat.numel())
    flat[:n] = torch.tensor(plant[:n], dtype=F32)
    return dict(M=M, C=C, dy=dy, ref=ref, planted=n)


def act_backward_ref(dy, ref, act):
    """g = dy * act'(.)."""
    if act is None:
        return dy.clone()
    if act == "relu":
        return torch.where(ref > 0, dy, torch.zeros_like(dy))
    if act == "gelu":                                           # d/dz [z Phi(z)] = Phi(z) + z phi(z), erf form
        return dy * (0.5 * (1 + torch.erf(ref / math.sqrt(2.0))) + ref * torch.exp(-0.5 * ref * ref) / math.sqrt(2.0 * math.pi))
    return dy * ref * (1 - ref)


def act_backward_scale(dy, ref, act):
    """gelu: the terms 1/2, erf / 2 and z phi(z) (the first is the largest but for |z| phi(z) <= 0.25); sigmoid: y and y^2."""
    dy, ref = dy.double(), ref.double()
    if act == "gelu":
        return dy.abs() * torch.maximum(torch.full_like(ref, 0.5), (ref * torch.exp(-0.5 * ref * ref) / math.sqrt(2.0 * math.pi)).abs())
    if act == "sigmoid":
        return dy.abs() * torch.maximum(ref.abs(), ref * ref)
    return dy.abs()


# ---- column sums ------------------------------------------------------------------------------------------------------------------------
CSUM_M = [1, 15, 16, 17, 63, 64, 65, 8191, 8192, 8193, 8192 + 65]
CSUM_C = [1, 63, 64, 65, 260]
CSUM_SMALL_MAX = 8192


def col_sum_chain(M):
    """Longest chain of fp32 roundings behind one column sum, read from csrc/train_dec.hip.  Up to 8192 rows: 16 row lanes, each adds
    its ceil(M / 16) rows (four at a time as a tree, then the rest) - at most that many roundings with the final one to fp32 - and the
    16 lanes meet in double.  Above: 64-row chunks on 4 row lanes of 16 rows; the chunks meet in double.  (The 4 lanes of a chunk meet
    in fp32, two more roundings than the 16 asserted here; the bound holds with room to spare all the same.)"""
    return -(-M // 16) if M <= CSUM_SMALL_MAX else 16


@lru_cache(maxsize=None)
def csum_case(M, C):
    return 1000.0 + torch.randn(M, C, generator=gen(31, M, C))


def col_sum_bound(x):
    return col_sum_chain(x.shape[0]) * U * x.double().abs().sum(0)


# ---- positional encodings ---------------------------------------------------------------------------------------------------------------
PE_N = [1, 17, 200]
SINE_D = [6, 96, 256]               # 17 x 6, 17 x 96, 200 x 6 ... are no multiples of the 256 threads of a workgroup
FOURIER_D = [2, 96, 256]
TWO_PI = 2 * math.pi


def pe_tables(d_pos, temperature=TEMPERATURE):
    """(dim_t [d_pos] fp32, axis [d_pos] int8) from the oracle's channel plan and divisors."""
    dim_t, axis = [], []
    for a, cdim in enumerate(D.pe_channel_plan(d_pos, 3)):
        dim_t.append(D.pe_dim_t(cdim, temperature))
        axis.append(torch.full((cdim,), a, dtype=torch.int8))
    return torch.cat(dim_t).float().contiguous(), torch.cat(axis).contiguous()


SCENE_RANGES = torch.tensor([[-1.5, -2.0, 0.0, 4.5, 3.0, 2.75],          # (lo, hi) of three scenes, every extent positive
                             [0.25, 0.5, -0.5, 8.0, 7.25, 2.5],
                             [-10.0, -12.0, -1.0, -3.5, 4.0, 1.25]])


@lru_cache(maxsize=None)
def pe_case(n, seed=0):
    """n points of three scenes (scene 1 owns no row, the scene of a row is not sorted), each up to half an extent outside its scene's
    range, as columns 0-2 of an [n, 6] tensor; modulation numerators [n, 3] in (0, 1), denominators [3] and [n, 3]."""
    g = gen(41, n, seed)
    row_scene = torch.where(torch.rand(n, generator=g) < 0.5, 2, 0).to(torch.int32)
    if n > 1:
        row_scene[0], row_scene[1] = 2, 0
    rng = SCENE_RANGES[row_scene.long()]
    u = torch.rand(n, 3, generator=g) * 2 - 0.5
    u[0, 0] = 1.5
    if n > 1:
        u[1, 1], u[1, 2] = -0.5, 0.0
    pts = torch.zeros(n, 6)
    pts[:, :3] = rng[:, :3] + u * (rng[:, 3:] - rng[:, :3])
    pts[:, 3:] = torch.randn(n, 3, generator=g)
    return dict(n=n, pts=pts, xyz=pts[:, :3], row_scene=row_scene, rng_rows=rng, mod_num=torch.rand(n, 3, generator=g) * 0.9 + 0.05,
                den1=torch.rand(3, generator=g) * 0.4 + 0.05, den2=torch.rand(n, 3, generator=g) * 0.4 + 0.05)


@lru_cache(maxsize=None)
def pe_case_one_scene(n, s=2):
    """`pe_case(n)` with every row moved into scene s (the same position relative to the range): n rows for the one-scene entries."""
    p = dict(pe_case(n))
    u = (p["xyz"] - p["rng_rows"][:, :3]) / (p["rng_rows"][:, 3:] - p["rng_rows"][:, :3])
    p["rng_rows"] = SCENE_RANGES[s].expand(n, 6).contiguous()
    p["pts"] = p["pts"].clone()
    p["pts"][:, :3] = SCENE_RANGES[s, :3] + u * (SCENE_RANGES[s, 3:] - SCENE_RANGES[s, :3])
    p["xyz"], p["row_scene"], p["scene"] = p["pts"][:, :3], torch.full((n,), s, dtype=torch.int32), s
    return p


def _normalised(xyz, rng_rows):
    return (xyz - rng_rows[:, :3]) * 1.0 / (rng_rows[:, 3:] - rng_rows[:, :3]) + 0.0


def sine_pe_ref(xyz, rng_rows, dim_t, axis, mod_num=None, mod_den=None):
    """out[r, c] = f_c(((x - lo) / (hi - lo))[axis c] * 2 pi / dim_t[c]) * (mod_num / mod_den)[r, axis c]; f = sin on even channels,
    cos on odd ones; rng_rows [n, 6] = each row's own (lo, hi)."""
    a = axis.long()
    pos = _normalised(xyz, rng_rows)[:, a] * TWO_PI / dim_t.to(xyz.dtype)[None, :]
    even = (torch.arange(a.numel()) % 2 == 0)[None, :]
    out = torch.where(even, pos.sin(), pos.cos())
    if mod_num is not None:
        out = out * (mod_num / mod_den.expand_as(mod_num))[:, a]
    return out


def sine_pe_scale(xyz, rng_rows, dim_t, axis, mod_num=None, mod_den=None):
    """One product: sin / cos carry the absolute rounding of their argument, so max(1, |argument|), times the modulation."""
    a = axis.long()
    pos = _normalised(xyz.double(), rng_rows.double())[:, a] * TWO_PI / dim_t.double()[None, :]
    sc = pos.abs().clamp(min=1.0)
    if mod_num is not None:
        sc = sc * (mod_num.double() / mod_den.double().expand_as(mod_num)).abs()[:, a]
    return sc


def sine_pe_mod_bwd_ref(d_out, xyz, rng_rows, dim_t, axis, mod_den):
    """d mod_num [n, 3]: sum over the channels of an axis of d_out * pe / mod_den (positions and denominators carry no gradient)."""
    pe = sine_pe_ref(xyz, rng_rows, dim_t, axis)
    onehot = torch.stack([axis.long() == k for k in range(3)], 1).to(xyz.dtype)           # [d, 3]
    return (d_out * pe) @ onehot / mod_den.expand(xyz.shape[0], 3)


def sine_pe_mod_bwd_scale(d_out, xyz, rng_rows, dim_t, axis, mod_den):
    """The largest term d_out * pe / mod_den of the axis (pe with the scale of `sine_pe_scale`)."""
    sc = (d_out.double().abs() * sine_pe_scale(xyz, rng_rows, dim_t, axis))
    per_axis = torch.stack([torch.where((axis.long() == k)[None, :], sc, torch.zeros_like(sc)).amax(1) for k in range(3)], 1)
    return per_axis / mod_den.double().expand(xyz.shape[0], 3).abs()


@lru_cache(maxsize=None)
def gauss_b(d_pos):
    """[3, d_pos / 2 + 5]: wider than the kernel reads."""
    return torch.randn(3, d_pos // 2 + 5, generator=gen(43, d_pos))


def fourier_pe_ref(xyz, rng_rows, gb, d_pos):
    """[sin | cos] of sum_a (normalised x_a * 2 pi) * B[a, c], c < d_pos / 2."""
    p = _normalised(xyz, rng_rows) * TWO_PI
    proj = (p[:, :, None] * gb.to(xyz.dtype)[None, :, :d_pos // 2]).sum(1)
    return torch.cat([proj.sin(), proj.cos()], 1)


def fourier_pe_scale(xyz, rng_rows, gb, d_pos):
    """The argument of sin / cos is a sum of three products: max(1, the largest of them)."""
    p = _normalised(xyz.double(), rng_rows.double()) * TWO_PI
    t = (p[:, :, None] * gb.double()[None, :, :d_pos // 2]).abs().amax(1).clamp(min=1.0)
    return torch.cat([t, t], 1)


# ---- box refinement ---------------------------------------------------------------------------------------------------------------------
BOX_Q = [1, 85, 86, 200]            # 85 x 3 = 255 and 86 x 3 = 258 elements straddle one workgroup
SIZE_PREV = [0.0, 1e-6, 1e-5, 0.5, 1 - 1e-6, 1.0, -0.2, 1.3]               # the clamp and both eps branches of inverse_sigmoid
D_SIZE = [0.0, 1.0, -1.0, 30.0, -30.0, 100.0, -100.0]


@lru_cache(maxsize=None)
def box_case(Q):
    """ref_points, d_center, d_size [Q, 3], size_prev [3] and [Q, 3], per-row scenes as in `pe_case`, gradients of the outputs.  The
    grid SIZE_PREV x D_SIZE is planted over the first 56 elements (as many as fit) of the [Q, 3] arrays."""
    g = gen(53, Q)
    p = pe_case(Q, seed=1)
    c = dict(Q=Q, ref=p["xyz"].contiguous(), dc=0.3 * torch.randn(Q, 3, generator=g), ds=torch.randn(Q, 3, generator=g),
             sp1=torch.tensor([0.11, 0.5, 0.93]), sp2=torch.rand(Q, 3, generator=g), row_scene=p["row_scene"], rng_rows=p["rng_rows"],
             g_center=torch.randn(Q, 3, generator=g), g_metric=torch.randn(Q, 3, generator=g))
    grid = [(s, d) for s in SIZE_PREV for d in D_SIZE]
    n = min(len(grid), 3 * Q)
    c["sp2"].view(-1)[:n] = torch.tensor([s for s, _ in grid[:n]], dtype=F32)
    c["ds"].view(-1)[:n] = torch.tensor([d for _, d in grid[:n]], dtype=F32)
    c["planted"] = n
    if Q == 1:
        c["sp1"] = torch.tensor([1e-6, 1.0, 0.4])              # one ordinary entry: the largest reference entry carries the cap
        c["ds"][0] = torch.tensor([-100.0, 100.0, 0.5])
        c["sp2"][0] = torch.tensor([0.0, 1e-5, 0.7])
    return c


def box_case_one_scene(Q, s=2):
    """`box_case(Q)` with every row in scene s: Q rows for the one-scene entries (the points need not lie inside the range)."""
    c = dict(box_case(Q))
    c["rng_rows"], c["row_scene"], c["scene"] = SCENE_RANGES[s].expand(Q, 6).contiguous(), torch.full((Q,), s, dtype=torch.int32), s
    return c


def inverse_sigmoid(x, eps=1e-5):
    x = x.clamp(0, 1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


def box_refine_ref(ref, dc, size_prev, ds, rng_rows, normalize):
    """-> (center, size, size_metric); size_prev [3] or [Q, 3]; ds None: no sizes."""
    center = ref + dc
    if ds is None:
        return center, None, None
    sp = size_prev.expand_as(ds)
    if normalize:
        size = torch.sigmoid(inverse_sigmoid(sp) + ds)
        return center, size, size * (rng_rows[:, 3:] - rng_rows[:, :3])
    size = sp + ds
    return center, size, size


def box_size_scale(size_prev, ds, rng_rows):
    """Normalised size s = sigmoid(z), z = inverse_sigmoid(size_prev) + d_size: s itself, and the two terms of z through
    ds / dz = s (1 - s).  -> (scale of size, scale of size_metric)."""
    ds = ds.double()
    logit = inverse_sigmoid(size_prev.double().expand_as(ds))
    s = torch.sigmoid(logit + ds)
    sc = torch.maximum(s, s * (1 - s) * torch.maximum(logit.abs(), ds.abs()))
    return sc, sc * (rng_rows.double()[:, 3:] - rng_rows.double()[:, :3])


def box_refine_bwd_ref(g_center, g_metric, size, rng_rows, normalize, has_size=True):
    """-> (d d_center, d d_size): the centre passes its gradient on; the size takes the metric size's times (hi - lo) s (1 - s) when
    normalised.  Absent output gradients are zeros."""
    zero = torch.zeros_like(rng_rows[:, :3])
    d_dc = zero if g_center is None else g_center.clone()
    if not has_size:
        return d_dc, None
    gm = zero if g_metric is None else g_metric
    if normalize:
        return d_dc, gm * (rng_rows[:, 3:] - rng_rows[:, :3]) * size * (1 - size)
    return d_dc, gm.clone()


def box_refine_bwd_scale(g_metric, size, rng_rows):
    """d d_size = g (hi - lo) (s - s^2): the larger of the two terms is s."""
    return g_metric.double().abs() * (rng_rows.double()[:, 3:] - rng_rows.double()[:, :3]) * size.double().abs()


def box_refine_chain_scale(g_metric, size_prev, ds, rng_rows):
    """Forward and backward in one (the autograd node): d d_size = g (hi - lo) s (1 - s) with s = sigmoid(z), z = inverse_sigmoid(size_prev)
    + d_size - the scale of `box_refine_bwd_scale`, and the two terms of z through d [s (1 - s)] / dz = s (1 - s) (1 - 2 s)."""
    ds = ds.double()
    logit = inverse_sigmoid(size_prev.double().expand_as(ds))
    s = torch.sigmoid(logit + ds)
    sc = torch.maximum(s, s * (1 - s) * (1 - 2 * s).abs() * torch.maximum(logit.abs(), ds.abs()))
    return g_metric.double().abs() * (rng_rows.double()[:, 3:] - rng_rows.double()[:, :3]) * sc


# ---- batched transpose ------------------------------------------------------------------------------------------------------------------
TRANSPOSE_JOBS = [(1, 1, 1, 1), (31, 33, 32, 1), (32, 32, 32, 1), (33, 31, 64, 1), (3, 256, 32, 1), (256, 1024, 256, 1), (27, 5, 32, 4)]
TB_MAX = 112                        # jobs per launch


def small_jobs(n):
    """n small (rows, cols, ld_dst, batch) of mixed shapes."""
    g = gen(61, n)
    out = []
    for i in range(n):
        rows, cols = int(torch.randint(1, 41, (1,), generator=g)), int(torch.randint(1, 41, (1,), generator=g))
        ld = rows + (0, 1, 32 - rows % 32)[i % 3]
        out.append((rows, cols, ld, 1 if i % 5 else 2))
    return out


def transpose_src(rows, cols, batch, seed):
    return torch.randn(batch, rows, cols, generator=gen(67, rows, cols, batch, seed))


def transpose_ref(src, ld_dst):
    """[batch, rows, cols] -> [batch, cols, ld_dst], columns rows.. zero."""
    b, rows, cols = src.shape
    out = torch.zeros(b, cols, ld_dst, dtype=src.dtype)
    out[:, :, :rows] = src.transpose(1, 2)
    return out
