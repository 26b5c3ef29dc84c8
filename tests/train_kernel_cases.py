"""Inputs for the direct tests of the sparse U-Net's training kernels in `segdino3d_amd/csrc/pair_wgrad.hip` and `csrc/train.hip`
(tests/test_gpu_train_kernels.py) and the float64 reference of every one of them, written out from the formula in the kernel's header
comment: the weight gradient over a pair list (with its output-row list), the gather + matmul model of the sparse convolution behind
the input gradient, batch-statistics BatchNorm forward / backward with its running statistics, and the backward of the superpoint mean.

Inputs are seeded fp32 / integer CPU tensors, so their float64 copies are exact; every reference takes tensors of any float dtype and
computes in that dtype (float64 = the reference, float32 = the same reference evaluated in fp32, whose error sets the bound).
tests/test_train_kernel_cases.py cross-checks the references against float64 autograd on the CPU; nothing here needs a GPU.

Tolerance rules.
* Weight gradient: integer inputs are compared bit for bit (every partial sum is an integer below 2^24, so no summation order can
  change it); float inputs against the derived bound of `wgrad_bound`.
* BatchNorm and the pooling backward: `check_float`, the rule of tests/decoder_kernel_cases.py - an error is measured in units of the
  entry's own scale (the largest magnitude among the terms summed into it, from the float64 reference); the bound is
  max(8 ulp of fp32, 4 x e32) of that scale, e32 being the error of the same reference evaluated in fp32 on the CPU, and no entry may
  be further than 2e-5 of the largest reference entry from the reference.  The margin of 4 over e32 is the figure of the decoder
  tests; no family here needs another one (profiles/train_kernel_errors.md).  The kernel's own output never enters a bound."""
from functools import lru_cache

import numpy as np
import torch

from tests.loss_kernel_cases import CAP, FLOOR, ULP32, _arr, scaled_error

F64, F32 = torch.float64, torch.float32
U = 2.0 ** -24                      # unit roundoff of fp32
PT = 128                            # pairs per tile of the pair lists
RECORDS = []
PREFIX = "[train-kernel-error]"


def gen(*seed):
    v = 0
    for s in seed:
        v = (v * 1000003 + int(s)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(v)


def record(line):
    line = f"{PREFIX} {line}"
    print(line)
    RECORDS.append(line)


# ---- the tolerance rule -----------------------------------------------------------------------------------------------------------------
def _scale_of(scale, r64):
    top = float(r64.abs().max()) if r64.numel() else 0.0
    if scale is None:
        return torch.full_like(r64, top), top
    s = _arr(scale)
    return (s.expand_as(r64) if s.numel() == 1 else s), top


def float_bound(r64, r32, sc):
    e32 = scaled_error(r32, r64, sc)
    return max(8 * ULP32, 4 * e32), e32


def check_float(family, case, got, ref64, ref32, scale=None):
    """Assert the tolerance rule and print / record the `[train-kernel-error]` line.  `scale` defaults to the largest reference entry."""
    got, r64, r32 = _arr(got), _arr(ref64), _arr(ref32)
    assert got.shape == r64.shape == r32.shape, (family, case, got.shape, r64.shape, r32.shape)
    assert bool(torch.isfinite(r64).all()), (family, case, "reference not finite")
    sc, top = _scale_of(scale, r64)
    assert sc.shape == r64.shape, (family, case, sc.shape, r64.shape)
    bound, e32 = float_bound(r64, r32, sc)
    kerr = scaled_error(got, r64, sc)
    worst = float((got - r64).abs().max()) if r64.numel() else 0.0
    record(f"{family} | {case} | kernel {kerr:.3e} | e32 {e32:.3e} | bound {bound:.3e} | abs {worst:.3e} | cap {CAP * top:.3e}")
    assert bool(torch.isfinite(got).all()), (family, case, "not finite")
    assert bool(((got - r64).abs() <= bound * sc + FLOOR).all()), (family, case, kerr, bound)      # entries of scale 0: exact
    assert worst <= CAP * top + FLOOR, (family, case, worst, CAP * top)
    return kerr, e32, bound


def reference_passes(family, ref64, ref32, scale=None):
    """The fp32 evaluation of the reference against the rule (CPU test: the reference alone passes) -> (e32, largest abs error, cap)."""
    r64, r32 = _arr(ref64), _arr(ref32)
    sc, top = _scale_of(scale, r64)
    bound, e32 = float_bound(r64, r32, sc)
    worst = float((r32 - r64).abs().max()) if r64.numel() else 0.0
    assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all())
    assert bool(((r32 - r64).abs() <= bound * sc + FLOOR).all()), (family, e32, bound)
    assert worst <= CAP * top + FLOOR, (family, worst, CAP * top)
    return e32, worst, CAP * top


def check_bound(family, case, got, ref64, bound):
    """Derived absolute bound per entry (the weight gradient)."""
    got, r64, b = _arr(got), _arr(ref64), _arr(bound)
    assert got.shape == r64.shape == b.shape, (family, case, got.shape, r64.shape, b.shape)
    err = (got - r64).abs()
    ratio = float((err / b.clamp(min=1e-300)).max()) if err.numel() else 0.0
    worst = int(err.argmax()) if err.numel() else 0
    record(f"{family} | {case} | abs {float(err.max()) if err.numel() else 0.0:.3e} | derived bound {float(b[worst]) if err.numel() else 0.0:.3e} | "
           f"error / bound {ratio:.3e}")
    assert bool(torch.isfinite(got).all()) and bool((err <= b).all()), (family, case, ratio)
    return ratio


# ---- neighbour tables -------------------------------------------------------------------------------------------------------------------
# name -> (K, M, V_in, pairs per offset planted at the front; the other offsets get seeded counts).  Between them: an offset with no pair,
# offsets with exactly 1, 127, 128 and 129 pairs (a tile is 128 pairs, staged in two steps of 64), K = 1 / 3 / 27 / 125.
TABLES = {
    "k1_m1": (1, 1, 1, [1]),
    "k1_m5": (1, 5, 4, [4]),
    "k1_m130": (1, 130, 131, [129]),
    "k3_m150": (3, 150, 97, [127, 0, 128]),
    "k27_m40": (27, 40, 43, [0, 1, 39, 0]),
    "k27_m600": (27, 600, 577, [129, 0, 128, 1, 127, 599, 64, 65, 63, 256, 257]),
    "k125_m20": (125, 20, 23, [0, 1, 19, 0, 0, 2]),
}
HOT = 0                             # the input row many pairs read (about a third of all pairs, when the input has more than one row)


@lru_cache(maxsize=None)
def table_case(name):
    """-> dict(nbr int32 [K, M], n_pairs, V_in, counts [K], dead = the output row no pair writes (None at M = 1)).  A pair's input row
    is row HOT with probability 0.3 and any row otherwise; the rows of an offset are a seeded subset of the output rows but `dead`."""
    K, M, V_in, planted = TABLES[name]
    g = gen(71, K, M)
    dead = None if M == 1 else int(torch.randint(0, M, (1,), generator=g))
    rows_ok = torch.tensor([r for r in range(M) if r != dead], dtype=torch.long)
    counts = list(planted) + [int(torch.randint(0, len(rows_ok) + 1, (1,), generator=g)) for _ in range(K - len(planted))]
    nbr = torch.full((K, M), -1, dtype=torch.int32)
    for k, c in enumerate(counts):
        rows = rows_ok[torch.randperm(len(rows_ok), generator=g)[:c]]
        src = torch.randint(0, V_in, (c,), generator=g)
        src[torch.rand(c, generator=g) < 0.3] = HOT
        nbr[k, rows] = src.to(torch.int32)
    return dict(name=name, nbr=nbr, K=K, M=M, V_in=V_in, counts=counts, n_pairs=int(sum(counts)), dead=dead)


def tile_counts(counts):
    """(real tiles, tiles of the capacity `ops.pair_lists` allots: the pairs + 127 of padding per offset, rounded up to a tile)."""
    real = sum(-(-c // PT) for c in counts)
    p_cap = (sum(counts) + 127 * len(counts) + 127) // PT * PT
    return real, p_cap // PT


def symmetric_table(K, M, seed=0, fill=0.5):
    """A stride-1 table of a voxel set onto itself: nbr[K - 1 - k][i] = r <=> nbr[k][r] = i, the centre offset is the identity.  Each
    offset below the centre is a seeded partial one-to-one map of about fill * M rows (one row, at least)."""
    assert K % 2 == 1
    g = gen(73, K, M, seed)
    nbr = torch.full((K, M), -1, dtype=torch.int32)
    nbr[K // 2] = torch.arange(M, dtype=torch.int32)
    for k in range(K // 2):
        n = max(1, int(fill * M * float(torch.rand(1, generator=g))))
        r, i = torch.randperm(M, generator=g)[:n], torch.randperm(M, generator=g)[:n]
        nbr[k, r] = i.to(torch.int32)
        nbr[K - 1 - k, i] = r.to(torch.int32)
    return nbr


def stride_tables(Mc, seed=0):
    """(down [8, Mc] with fine rows, up [8, Mf] with coarse rows, Mf): a k = 2, s = 2 pair - every coarse row owns a seeded non-empty
    subset of its eight children, fine rows numbered in a seeded order; down[k][p] = f <=> up[k][f] = p."""
    g = gen(79, Mc, seed)
    own = torch.rand(8, Mc, generator=g) < 0.4
    own[torch.randint(0, 8, (Mc,), generator=g), torch.arange(Mc)] = True
    ks, ps = own.nonzero(as_tuple=True)
    Mf = int(ks.numel())
    f = torch.randperm(Mf, generator=g).to(torch.int32)
    down = torch.full((8, Mc), -1, dtype=torch.int32)
    up = torch.full((8, Mf), -1, dtype=torch.int32)
    down[ks, ps] = f
    up[ks, f.long()] = ps.to(torch.int32)
    return down, up, Mf


def tiny_scene_points(seed=5):
    """[N, 6]: a few far-apart points, one tight cluster and a straight line (tests/test_gpu_pair_paths.py::test_chained_lists_edge_cases)."""
    g = torch.Generator().manual_seed(seed)
    iso = torch.rand(40, 3, generator=g) * 50.0
    cluster = 0.5 + 0.05 * torch.rand(300, 3, generator=g)
    line = torch.stack([torch.arange(200) * 0.02 + 10.0, torch.full((200,), 3.0), torch.full((200,), 3.0)], 1)
    pts = torch.cat([iso, cluster, line]).float()
    return torch.cat([pts, torch.zeros(pts.shape[0], 3)], 1)


# ---- weight gradient --------------------------------------------------------------------------------------------------------------------
CHANNELS = [4, 36, 68, 96, 100, 128, 160, 260]
# (Cout, Cin): every pair of {4, 36, 68, 100} - one, two, three and four 32-wide tiles per block, each with a ragged last tile - covers
# the 16 instantiations; behind them the full blocks (96, 128) and the channel counts of more than one block (160 = 96 + 64, 260 = 96 +
# 96 + 68).
CHANNEL_PAIRS = [(a, b) for a in (4, 36, 68, 100) for b in (4, 36, 68, 100)] + [(96, 128), (128, 96), (128, 128), (160, 260), (260, 160), (4, 260), (160, 36)]


def sub_tiles(C):
    """32-wide tiles per block of `sd3d_pair_wgrad` for C channels: C split evenly over its ceil(C / 128) blocks."""
    n32 = (C + 31) // 32
    nb = (n32 + 3) // 4
    return (n32 + nb - 1) // nb


def wgrad_waves(nco, nci):
    return 4 if nco * nci < 8 else nco * nci


def wgrad_ranges(K, Cin, Cout, p_cap):
    """Tile ranges of `sd3d_pair_wgrad` (`wgrad_ranges` in csrc/pair_wgrad.hip); the launch has this many + K partial slots."""
    blocks = -(-Cout // 128) * -(-Cin // 128)
    total = 256 if (Cin * Cout > 96 * 96 or (Cin >= 96 and Cout >= 96)) else (512 if K > 27 else 768)
    r = max(32, total // blocks)
    tiles = p_cap // PT
    return (tiles if tiles > 0 else 1) if tiles < r else r


def int_operands(M, V_in, Cout, Cin, seed=0, ones=False):
    """(dy [M, Cout], x [V_in, Cin]) of integers in -2 .. 2 (or all ones: the gradient is then the pair count of the offset)."""
    if ones:
        return torch.ones(M, Cout), torch.ones(V_in, Cin)
    g = gen(83, M, V_in, Cout, Cin, seed)
    return torch.randint(-2, 3, (M, Cout), generator=g).float(), torch.randint(-2, 3, (V_in, Cin), generator=g).float()


CARRY = 1.99609375                  # 0x3FFF8000: a tie on the odd bf16 mantissa 0x7F rounds up, the carry runs into the exponent -> 2.0
CARRY2 = -0.998046875 - 2.0 ** -12  # just above the tie of the mantissa 0x7F below 1: -> -1.0


def float_operands(M, V_in, Cout, Cin, seed=0):
    """Seeded normal operands; their first entries round to bf16 with a carry into the exponent."""
    g = gen(89, M, V_in, Cout, Cin, seed)
    dy, x = torch.randn(M, Cout, generator=g), torch.randn(V_in, Cin, generator=g)
    dy.view(-1)[0], x.view(-1)[0] = CARRY, CARRY2
    if dy.numel() > 1:
        dy.view(-1)[1] = CARRY2
    return dy, x


def round_bf16(t):
    """fp32 -> the nearest bf16 value (ties to even) as fp32, by the integer arithmetic of `round_to_bf16` in csrc/pair_wgrad.hip."""
    u = t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    u = torch.where(u >= 2 ** 31, u - 2 ** 32, u)
    return u.to(torch.int32).view(torch.float32).reshape(t.shape)


def wgrad_ref(dy, x, nbr, bf16=False):
    """dw[k][co][ci] = sum over the rows r of offset k of dy[r][co] * x[nbr[k][r]][ci], in the dtype of dy; -> (dw [K, Cout, Cin],
    the same sum over |dy| |x|).  bf16: both operands rounded to bf16 first (the products are then exact in fp32)."""
    if bf16:
        dy, x = round_bf16(dy.float()).to(dy.dtype), round_bf16(x.float()).to(x.dtype)
    K = nbr.shape[0]
    dw = torch.zeros(K, dy.shape[1], x.shape[1], dtype=dy.dtype)
    mag = torch.zeros_like(dw)
    for k in range(K):
        rows = (nbr[k] >= 0).nonzero(as_tuple=True)[0]
        if rows.numel():
            a, b = dy[rows], x[nbr[k][rows].long()]
            dw[k] = a.t() @ b
            mag[k] = a.abs().t() @ b.abs()
    return dw, mag


def wgrad_bound(mag64, counts, n_slots, old=None):
    """|err| <= (P_k + n_slots) * 2^-24 * sum_p |dy[out(p), co]| |x[in(p), ci]| per entry of offset k.

    Chain: every product of two fp32 operands is rounded once, and an entry's products are added one after the other into the MFMA
    accumulator of the workgroup that owns the tile range (the instruction's contraction index is the pair index) - at most P_k
    additions of at most P_k rounded products, each with a relative error of 2^-24 on a partial sum that |.|-sums bound; to first order
    that is (P_k + 1) * 2^-24 of sum |dy| |x| when one range holds the whole offset and less when several share it.  Pass 2 adds the
    partial blocks of the offset's slots in fp32: fewer than n_slots additions.  (P_k + n_slots) covers both with one rounding to
    spare; the padding rows of a tile are zeros and add nothing.  `old` (accumulate): one more addition, of the old value."""
    P = torch.tensor(counts, dtype=F64)[:, None, None]
    b = (P + n_slots) * U * mag64
    if old is not None:
        b = b + U * (old.double().abs() + mag64)
    return b + FLOOR


def out_rows_ref(pos, p_cap):
    """numpy: out_idx[pos[k][r]] = r for every entry >= 0, -1 everywhere else."""
    pos = np.asarray(pos)
    out = np.full(int(p_cap), -1, dtype=np.int32)
    k, r = np.nonzero(pos >= 0)
    out[pos[k, r]] = r.astype(np.int32)
    return out


# ---- the sparse convolution as gather + matmul ------------------------------------------------------------------------------------------------
def conv_model(x, w, nbr, res=None):
    """y[r] = sum_k w[k] @ x[nbr[k][r]] (+ res[r]); x [V_in, Cin], w [K, Cout, Cin], nbr [K, M]; differentiable."""
    y = torch.zeros(nbr.shape[1], w.shape[1], dtype=x.dtype) if res is None else res.clone()
    for k in range(nbr.shape[0]):
        rows = (nbr[k] >= 0).nonzero(as_tuple=True)[0]
        if rows.numel():
            y = y.index_add(0, rows, x[nbr[k][rows].long()] @ w[k].t())
    return y


def conv_grads(x, w, nbr, dy, res=None):
    """float64 autograd of `conv_model` -> (y, dx, dw, dres or None)."""
    x = x.double().clone().requires_grad_(True)
    w = w.double().clone().requires_grad_(True)
    r = None if res is None else res.double().clone().requires_grad_(True)
    y = conv_model(x, w, nbr, r)
    y.backward(dy.double())
    return y.detach(), x.grad, w.grad, None if r is None else r.grad


ROW_TOL = 2e-6                      # of the row's largest entry: the figure of tests/test_gpu_pair_paths.py for `pair_conv`


def row_error(got, ref64):
    return float(((got.double() - ref64).abs() / ref64.abs().amax(dim=1, keepdim=True).clamp_min(1e-3)).max()) if ref64.numel() else 0.0


# ---- BatchNorm --------------------------------------------------------------------------------------------------------------------------
BN_M = [1, 2, 255, 256, 257, 513]   # 256 rows per block of the column reductions
BN_C = [4, 12, 96, 100, 256, 1024]  # 256 / (C / 4) row lanes: 256, 85, 10 (16 idle threads), 10 (6 idle), 4, 1
EPS = float(np.float32(1e-5))       # the kernels take eps as a float
MOMENTA = [float(np.float32(0.02)), 1.0]
COL_BIG, COL_CONST, COL_OUT = 0, 1, 2


@lru_cache(maxsize=None)
def bn_case(M, C):
    """x, res, dy [M, C]; gamma, beta, running mean / var [C].  Planted columns of x (M >= 2): COL_BIG has mean 1e3 and spread 1 -
    1000 +- k / 8 in shuffled pairs (and one 1000 when M is odd), so fp32 holds the values, every partial sum and the mean exactly and
    what the column tests is the variance; COL_CONST is 1.75 in every row (variance exactly 0); row 0 of COL_OUT is its largest
    outlier, 8 spreads above the mean of the others - the kernel subtracts row 0 from every row before it sums."""
    g = gen(97, M, C)
    c = dict(M=M, C=C, x=torch.randn(M, C, generator=g), res=torch.randn(M, C, generator=g), dy=torch.randn(M, C, generator=g),
             gamma=1 + 0.1 * torch.randn(C, generator=g), beta=0.1 * torch.randn(C, generator=g),
             run_mean=0.5 * torch.randn(C, generator=g), run_var=0.5 + torch.rand(C, generator=g))
    c["x"] += 0.5 * torch.randn(C, generator=g)                 # column means of the order of the spread
    half = torch.round(8 * torch.randn(M // 2, generator=g)) / 8
    col = torch.cat([half, -half, torch.zeros(M % 2)])
    c["x"][:, COL_BIG] = 1000.0 + col[torch.randperm(M, generator=g)]
    c["x"][:, COL_CONST] = 1.75
    if M >= 2:
        c["x"][0, COL_OUT] = float(c["x"][1:, COL_OUT].mean()) + 8.0
    return c


def bn_stats_ref(x, eps=EPS):
    """-> (mean, biased variance, rstd = 1 / sqrt(var + eps)) over the rows, two passes."""
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return mean, var, 1 / torch.sqrt(var + eps)


def bn_stats_scale(x):
    """mean: the column's largest |x|; variance: the largest of its terms (x - mean)^2; rstd is one term, itself.
    -> (scale of mean, of var, of rstd)."""
    x = x.double()
    mean, var, rstd = bn_stats_ref(x)
    return x.abs().amax(0), ((x - mean) ** 2).amax(0), rstd


def bn_running_ref(run_mean, run_var, mean, var, M, momentum):
    """nn.BatchNorm1d: running = (1 - momentum) running + momentum * batch, the variance unbiased (M / (M - 1), 1 at M = 1)."""
    unb = M / max(M - 1, 1)
    return (1 - momentum) * run_mean + momentum * mean, (1 - momentum) * run_var + momentum * var * unb


def bn_apply_ref(x, mean, rstd, gamma, beta, res=None, relu=False):
    """y = act((x - mean) rstd gamma + beta + res) -> (y, pre-activation)."""
    z = (x - mean) * rstd * gamma + beta
    if res is not None:
        z = z + res
    return (torch.relu(z) if relu else z), z


def bn_apply_scale(x, mean, rstd, gamma, beta, res=None):
    """Terms summed into an entry: x and the mean, each times rstd |gamma|; beta; res."""
    x, mean, k = x.double(), mean.double(), (rstd.double() * gamma.double()).abs()
    top = torch.maximum(torch.maximum(x.abs(), mean.abs().expand_as(x)) * k, beta.double().abs().expand_as(x))
    return top if res is None else torch.maximum(top, res.double().abs())


def bn_backward_ref(dy, y, x, mean, rstd, gamma):
    """-> (dx, dres, dgamma, dbeta); y (the forward output) masks dy where the fused ReLU was off: y > 0 passes; None: no ReLU.
    dbeta = sum g, dgamma = sum g xhat, dx = gamma rstd (g - dbeta / M - xhat dgamma / M), dres = g."""
    M = x.shape[0]
    g = dy if y is None else torch.where(y > 0, dy, torch.zeros_like(dy))
    xh = (x - mean) * rstd
    dbeta, dgamma = g.sum(0), (g * xh).sum(0)
    return gamma * rstd * (g - dbeta / M - xh * dgamma / M), g, dgamma, dbeta


def bn_backward_scale(dy, y, x, mean, rstd, gamma):
    """dx: the terms g, dbeta / M and xhat dgamma / M, each times |gamma| rstd - the sums taken term by term (a column's largest |g|
    and |g xhat|); dgamma / dbeta: the column's largest |g xhat| / |g|.  -> (scale of dx, of dgamma, of dbeta)."""
    dy, x, mean, rstd = dy.double(), x.double(), mean.double(), rstd.double()
    g = dy if y is None else torch.where(y.double() > 0, dy, torch.zeros_like(dy))
    xh = (x - mean) * rstd
    gm, gxm = g.abs().amax(0), (g * xh).abs().amax(0)
    dx = (gamma.double() * rstd).abs() * torch.maximum(torch.maximum(g.abs(), gm.expand_as(g)), xh.abs() * gxm)
    return dx, gxm, gm


# ---- backward of the superpoint mean ----------------------------------------------------------------------------------------------------------
POOL_V = [1, 7, 8, 9, 100]          # eight voxels per workgroup
POOL_C = [4, 32, 96, 128]           # half a wave per voxel, lanes over float4 pieces: 1, 8, 24 and 32 of 32 lanes


@lru_cache(maxsize=None)
def pool_case(V, pow2=False):
    """Points sorted into V voxels and grouped into superpoints: superpoints int64 [N] (per point), sidx uint32-valued [N] (point ids
    in voxel order), seg_start int32 [V + 1], sp_start int32 [S + 1], voxel_of [N].  Voxel 0 has about 50 points (V = 1) or one point
    (V >= 2, voxel 1 then has the 50); superpoints are chunks of a seeded shuffle of the points, so a voxel's points fall into
    different ones; superpoint 0 has one point and the last id has none.  pow2: every superpoint has 1, 2, 4 or 8 points."""
    g = gen(101, V, int(pow2))
    sizes = [50] if V == 1 else [1, 50] + [int(torch.randint(1, 7, (1,), generator=g)) for _ in range(V - 2)]
    N = sum(sizes)
    sidx = torch.randperm(N, generator=g)
    seg_start = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int32)
    voxel_of = torch.empty(N, dtype=torch.long)
    voxel_of[sidx] = torch.repeat_interleave(torch.arange(V), torch.tensor(sizes))
    menu = [1, 2, 4, 8] if pow2 else [1, 2, 3, 5, 7]
    chunks, left = [1], N - 1
    while left > 0:
        s = menu[int(torch.randint(0, len(menu), (1,), generator=g))]
        while s > left:
            s = max(m for m in menu if m <= left) if pow2 else left
        chunks.append(s)
        left -= s
    order = torch.randperm(N, generator=g)
    sp = torch.empty(N, dtype=torch.int64)
    sp[order] = torch.repeat_interleave(torch.arange(len(chunks)), torch.tensor(chunks))
    S = len(chunks) + 1                                         # the last id: no point
    sp_start = torch.tensor([0] + list(np.cumsum(chunks)) + [N], dtype=torch.int32)
    return dict(V=V, N=N, S=S, sizes=sizes, sp_sizes=chunks + [0], superpoints=sp, sidx=sidx, seg_start=seg_start, sp_start=sp_start,
                voxel_of=voxel_of)


def pool_dout(S, C, seed=0, integer=False):
    g = gen(103, S, C, seed)
    return torch.randint(-8, 9, (S, C), generator=g).float() if integer else torch.randn(S, C, generator=g)


def pool_backward_ref(dout, c):
    """dfeat[v] = sum over the points p of voxel v of dout[sp[p]] / |sp[p]| -> (dfeat [V, C], the largest |term| of each entry)."""
    cnt = torch.tensor(c["sp_sizes"], dtype=dout.dtype).clamp(min=1)
    term = dout[c["superpoints"]] / cnt[c["superpoints"]][:, None]                       # [N, C], per point
    dfeat = torch.zeros(c["V"], dout.shape[1], dtype=dout.dtype).index_add(0, c["voxel_of"], term)
    top = torch.zeros(c["V"], dout.shape[1], dtype=dout.dtype)
    top = top.scatter_reduce(0, c["voxel_of"][:, None].expand_as(term), term.abs(), "amax", include_self=True)
    return dfeat, top


def pool_forward_model(feat, c):
    """The pooled mean the kernel is the backward of: out[s] = mean over the points p of superpoint s of feat[voxel(p)]."""
    cnt = torch.tensor(c["sp_sizes"], dtype=feat.dtype).clamp(min=1)
    return torch.zeros(c["S"], feat.shape[1], dtype=feat.dtype).index_add(0, c["superpoints"], feat[c["voxel_of"]]) / cnt[:, None]


class StubPairs:
    """What the host wrappers look at before they call the library (`ops.PairLists` without a device)."""

    def __init__(self, center=-1, pos=None, out_idx=None, K=3, M=5, p_cap=512):
        self.center, self.pos, self.out_idx, self.K, self.M, self.p_cap = center, pos, out_idx, K, M, p_cap
        self.in_idx = self.tile_k = None
