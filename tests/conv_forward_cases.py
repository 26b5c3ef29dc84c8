"""Inputs for the direct tests of the forward convolution kernels - the pair-major sparse convolution (`segdino3d_amd/csrc/pair_gemm.hip`),
its dense twin `launch_pair_dense`, the output-stationary gather-GEMM (`csrc/gather_gemm.hip`) and the split-bf16 one
(`csrc/gather_gemm_split.hip`) - in tests/test_gpu_conv_forward.py, and the float64 reference of the one operation all of them
evaluate, written from the formula in `ops.gather_gemm`'s docstring:

    out[r, n] = act(scale[n] * sum_k sum_c x[nbr[k, r], c] * w[k, n, c] + shift[n] + res[r, n])

Nothing here needs a GPU; tests/test_conv_forward_cases.py checks the reference, the planted tables, the case lists and the Python
twins of the launchers' kernel selection on the CPU.

Tables.  The hand-built tables of tests/train_kernel_cases.py (an empty offset, offsets of exactly 1 / 127 / 128 / 129 pairs, a dead
output row, a hot input row, K = 1 / 3 / 27 / 125), its symmetric and stride tables, and what the forward needs on top:
  * `sym27_planted`  a symmetric 3^3 table (chained lists need one) whose offsets below the centre start with 0 / 1 / 127 / 128 / 129
                     pairs, and `up_planted`, a one-pair-per-row table (direct epilogue) with the same planted counts;
  * `big27_m6000`    the planted counts and 22 full offsets, 1062 tiles of capacity: the two-group 256-column kernel wants 1024;
  * `up_big`, `sym27_m12000`  the planted direct and symmetric tables again with more than a thousand tiles.  A pass-1 launch has up to
                     CUs x 2 .. 4 workgroups and never more than the capacity has tiles (`pass1_grid`), so on a small table every
                     workgroup multiplies ONE tile: only on these three and on `full27_m15200` does a workgroup walk from one offset's tiles into the
                     next one's (W[k] restaged between runs, the lock-step stream crossing a tile boundary);
  * `long_run`       one offset of 26 real tiles and four short ones behind it: a run of one offset longer than WS_RANGE_TILES;
  * `full27_m15200`  3213 real tiles.  A weight-stationary workgroup walks tiles [b n / g, (b + 1) n / g) of n real tiles on a grid of
                     g = min(CUs x resident workgroups, capacity tiles) workgroups (`ws_grid`), so ONE workgroup's range exceeds
                     WS_RANGE_TILES = 24 only when n > 24 g.  The smallest such launch on 256 CUs is the two-group kernel at
                     Cin = 288 (one workgroup per CU, g = 128): more than 3072 tiles.  `long_run` alone cannot reach that piece loop.

Operands.  Integer: x and w in -2 .. 2, scale in {1, 2, 3}, shift and res in -3 .. 3.  Every partial sum of any summation order is
then an integer below 2^24 (tests/test_conv_forward_cases.py asserts it from the reference's magnitude), fp32 accumulation is exact,
and the float64 reference cast to fp32 is the only right answer: these cases are compared bit for bit.  Integers in -2 .. 2 are
exact in bf16 as well, so the split-bf16 kernel has to give the same bits.  Float: seeded normals, the rows of x and res spread
by exp(randn).

Tolerance rule of the float cases (`check_conv`), two assertions, neither of which looks at the kernel's output for its bound:
  * the rule of `train_kernel_cases.check_float` with the per-entry magnitude |scale| sum |x| |w| + |shift| + |res| of `conv_ref`
    as scale: |error| <= max(8 ulp, MARGIN x e32) of that magnitude, e32 being the error of `conv_ref` evaluated in fp32 on the CPU, and
    no entry further than CAP of the largest reference entry from the reference.  MARGIN is 4, the figure of the decoder and training
    families, for every family here: profiles/conv_forward_errors.md holds the measured kernel / e32 ratios, none of which asks for more;
  * the project's row figure: `row_error` < ROW_TOL = 2e-6 of the row's largest entry (tests/test_gpu_pair_paths.py)."""
from collections import namedtuple
from functools import lru_cache

import torch

from tests.loss_kernel_cases import CAP, FLOOR, ULP32, _arr, scaled_error
from tests.train_kernel_cases import (HOT, PT, ROW_TOL, TABLES, gen, row_error, stride_tables, symmetric_table, table_case,  # noqa: F401
                                      tile_counts)

F64, F32 = torch.float64, torch.float32
PREFIX = "[conv-forward-error]"
RECORDS = []
MARGIN = 4                          # x e32 (see the module docstring)
EXACT_LIMIT = 2.0 ** 24
WS_RANGE_TILES = 24                 # csrc/pair_gemm.hip
DENSE_MIN_ROWS = 16384              # GG_PAIR_DENSE_MIN_ROWS, csrc/gather_gemm.hip
N_CU = 256                          # MI355X


def record(line):
    line = f"{PREFIX} {line}"
    print(line)
    RECORDS.append(line)


# ---- neighbour tables -------------------------------------------------------------------------------------------------------------------
PLANTED = [0, 1, 127, 128, 129]
SYM_TABLES = ("sym27_m300", "sym27_planted", "sym27_m12000")
DIRECT_TABLES = ("up_c40", "up_planted", "up_big")
BIG_TABLES = ("big27_m6000", "full27_m15200")
BOTH_PLANTED = ("k27_m600", "sym27_planted", "up_planted", "big27_m6000", "up_big", "sym27_m12000")      # an empty offset and the 127 / 128 / 129 boundary
TABLE_NAMES = tuple(TABLES) + SYM_TABLES + ("down_c40",) + DIRECT_TABLES + ("long_run",) + BIG_TABLES


def _counted(nbr, planted, g, V_in, dead):
    """Fill nbr [K, M] offset by offset with planted[k] pairs on seeded rows (never `dead`), a third of them reading row HOT."""
    M = nbr.shape[1]
    rows_ok = torch.tensor([r for r in range(M) if r != dead], dtype=torch.long)
    for k, c in enumerate(planted):
        rows = rows_ok[torch.randperm(len(rows_ok), generator=g)[:c]]
        src = torch.randint(0, V_in, (c,), generator=g)
        src[torch.rand(c, generator=g) < 0.3] = HOT
        nbr[k, rows] = src.to(torch.int32)


def _sym_planted(K, M):
    """`symmetric_table` with planted pair counts below the centre: PLANTED, then seeded ones."""
    g = gen(113, K, M)
    nbr = torch.full((K, M), -1, dtype=torch.int32)
    nbr[K // 2] = torch.arange(M, dtype=torch.int32)
    for k in range(K // 2):
        n = PLANTED[k] if k < len(PLANTED) else int(torch.randint(1, M + 1, (1,), generator=g))
        r, i = torch.randperm(M, generator=g)[:n], torch.randperm(M, generator=g)[:n]
        nbr[k, r] = i.to(torch.int32)
        nbr[K - 1 - k, i] = r.to(torch.int32)
    return nbr


def _up_planted(counts, V_in):
    """A one-pair-per-row table [K, sum(counts)]: offset k owns counts[k] rows, scattered by a seeded shuffle."""
    g = gen(127, len(counts), sum(counts))
    M = sum(counts)
    order = torch.randperm(M, generator=g)
    nbr = torch.full((len(counts), M), -1, dtype=torch.int32)
    at = 0
    for k, c in enumerate(counts):
        src = torch.randint(0, V_in, (c,), generator=g)
        src[torch.rand(c, generator=g) < 0.3] = HOT
        nbr[k, order[at:at + c]] = src.to(torch.int32)
        at += c
    return nbr


@lru_cache(maxsize=None)
def table(name):
    """-> dict(name, nbr int32 [K, M], K, M, V_in, counts [K], n_pairs, dead = an output row without any pair or None,
    kind = "plain" | "sym" (a stride-1 table onto itself: chained lists may be built) | "direct" (one pair per output row))."""
    if name in TABLES:
        return dict(table_case(name), kind="plain")
    dead, kind = None, "plain"
    if name == "sym27_m300":
        nbr, V_in, kind = symmetric_table(27, 300), 300, "sym"
    elif name == "sym27_planted":
        nbr, V_in, kind = _sym_planted(27, 300), 300, "sym"
    elif name in ("down_c40", "up_c40"):
        down, up, Mf = stride_tables(40)
        nbr, V_in, kind = (down, Mf, "plain") if name == "down_c40" else (up, 40, "direct")
    elif name == "up_planted":
        nbr, V_in, kind = _up_planted(PLANTED + [300, 64, 5], 97), 97, "direct"
    elif name == "sym27_m12000":
        nbr, V_in, kind = _sym_planted(27, 12000), 12000, "sym"
    elif name == "up_big":
        nbr, V_in, kind = _up_planted(PLANTED + [35000, 45000, 52000], 5000), 5000, "direct"
    elif name == "long_run":
        M, V_in, dead = 3400, 211, 1234
        nbr = torch.full((5, M), -1, dtype=torch.int32)
        _counted(nbr, [(WS_RANGE_TILES + 1) * PT + 1, 1, 127, 128, 129], gen(131, M), V_in, dead)
    elif name == "big27_m6000":
        M = V_in = 6000
        nbr = torch.full((27, M), -1, dtype=torch.int32)
        _counted(nbr, PLANTED + [M] * 22, gen(133, M), V_in, None)
    elif name == "full27_m15200":
        M = 15200
        nbr, V_in = torch.randint(0, M, (27, M), generator=gen(137, M), dtype=torch.int32), M
    else:
        raise KeyError(name)
    counts = (nbr >= 0).sum(1).tolist()
    return dict(name=name, nbr=nbr, K=nbr.shape[0], M=nbr.shape[1], V_in=V_in, counts=counts, n_pairs=int(sum(counts)), dead=dead, kind=kind)


def capacity_tiles(t):
    """Tiles of the capacity `ops.pair_lists_batch` allots to the table's plain lists (its `p_cap` formula) = `n_tiles` of the launch."""
    return tile_counts(t["counts"])[1]


# ---- the launchers' kernel selection, restated ------------------------------------------------------------------------------------------
def pg_col_tiles(Cout):
    """`pg_col_tiles` (csrc/pair_gemm.hip): (32-column tiles per workgroup, column groups)."""
    sub = (Cout + 31) // 32
    nt = 4 if sub >= 4 else sub
    if sub > 4 and sub % 4:
        nt = next(c for c in (4, 3, 2, 1) if sub % c == 0)
    return nt, -(-sub // nt)


def _ws_flags(Cin, Cout, chained, crowded, n_tiles):
    """`ws_one` / `ws_two` of `launch_pair_conv` (csrc/pair_gemm.hip, the lines under "weight-stationary variant")."""
    nt, cgs = pg_col_tiles(Cout)
    w_lds = Cout * (Cin + 4) * 4
    w_lds_cg = 32 * nt * (Cin + 4) * 4
    ws_one = not chained and not (crowded and nt >= 3) and cgs == 1 and Cout == 32 * nt and w_lds <= 68 * 1024
    ws_two = (not chained and not crowded and cgs == 2 and nt == 4 and Cout == 256 and n_tiles >= 1024
              and w_lds_cg + WS_RANGE_TILES * PT * 4 + 256 <= 160 * 1024)
    return nt, cgs, ws_one, ws_two, (w_lds_cg if ws_two else w_lds)


def pass1_variant(Cin, Cout, chained, direct, crowded, n_tiles):
    """The pass-1 kernel `launch_pair_conv` launches: ("ws2",) the two-group weight-stationary kernel, ("ws", nt, direct) the
    weight-stationary one, ("chained", nt) the lock-step kernel over chained lists, ("lockstep", nt, direct) the lock-step one.
    crowded = several scenes in flight; n_tiles = p_cap / 128."""
    nt, _cgs, ws_one, ws_two, _w = _ws_flags(Cin, Cout, chained, crowded, n_tiles)
    if ws_two:
        return ("ws2",)
    if ws_one:
        return ("ws", nt, bool(direct))
    return ("chained", nt) if chained else ("lockstep", nt, bool(direct))


def dense_variant(Cout):
    """`launch_pair_dense`: k_dense[nt - 1]."""
    return ("dense", pg_col_tiles(Cout)[0])


def takes_dense(M, Cout, ld_out=None, ld_res=0, nt=0):
    """The condition of `launch_gather_gemm` (csrc/gather_gemm.hip) under which a plain Linear goes to `launch_pair_dense`."""
    ld_out = Cout if ld_out is None else ld_out
    return nt == 0 and M >= DENSE_MIN_ROWS and Cout % 4 == 0 and ld_out % 4 == 0 and ld_res % 4 == 0


def ws_grid(Cin, Cout, n_tiles, n_cu=N_CU):
    """gridDim.x of a weight-stationary launch (`launch_pair_conv`, the lines under "resident workgroups per CU") or None."""
    nt, _cgs, ws_one, ws_two, w_need = _ws_flags(Cin, Cout, False, False, n_tiles)
    if not (ws_one or ws_two):
        return None
    per_cu = 4 if nt == 1 else (3 if nt == 3 else 2)
    per_cu = min(per_cu, (160 * 1024) // (w_need + WS_RANGE_TILES * PT * 4 + 256))
    return max(1, min(n_cu * per_cu // (2 if ws_two else 1), n_tiles))


def pass1_grid(Cin, Cout, chained, direct, crowded, n_tiles, n_cu=N_CU):
    """gridDim.x of the pass-1 launch: `ws_grid`, or `pg_lockstep_grid` (csrc/pair_gemm.hip) for the lock-step kernels."""
    if pass1_variant(Cin, Cout, chained, direct, crowded, n_tiles)[0] in ("ws", "ws2"):
        return ws_grid(Cin, Cout, n_tiles, n_cu)
    nt, cgs = pg_col_tiles(Cout)
    return max(1, min(n_cu * (3 if nt == 1 else 2) // cgs, n_tiles))


def dense_plan_code(rows, Cin, Cout):
    """`sd3d_dense_plan_code` (csrc/gather_gemm.hip)."""
    sub, tiles, steps = (Cout + 31) // 32, -(-rows // 32), Cin // 32
    if tiles >= 64 and steps >= 2:
        return 0
    if sub <= 0:
        return 1
    nt = 4 if sub >= 4 else sub
    while nt > 1 and tiles * -(-sub // nt) < 2048:
        nt -= 1
    if sub % nt:
        nt = next(c for c in range(nt, 0, -1) if sub % c == 0)
    return -1 if tiles * -(-sub // nt) < 1024 and steps >= 8 else nt


def lds_column_tiles(sub, tiles, gathered):
    """`lds_column_tiles` (csrc/gather_gemm.hip): column tiles per workgroup of the lock-step gather-GEMM."""
    nt = 4 if sub >= 4 else sub
    while nt > 2 and -(-tiles // 4) * -(-sub // nt) < 256:
        nt -= 1
    if nt == 2 and -(-tiles // 4) * -(-sub // 2) < 192:
        nt = 1
    if sub % nt:
        nt = next(c for c in range(nt, 0, -1) if sub % c == 0)
    if not gathered and tiles < 1024:
        nt = 2 if sub % 2 == 0 and -(-tiles // 4) * (sub // 2) >= 512 else 1
    return nt


def lds_ksplit(M, Cout, K, nt, ws_bytes):
    """gridDim.z of the lock-step gather-GEMM on a table (`launch_gather_gemm`: "slice the offsets over gridDim.z")."""
    wgs = -(-(-(-M // 32)) // 4) * -(-Cout // (32 * nt))
    if K < 8 or wgs >= 384:
        return 1
    ksp = 8 if wgs < 96 else (4 if wgs < 256 else 2)
    return ksp if ksp * M * Cout * 4 <= ws_bytes else 1


# ---- channel lists (from the launchers' rules) --------------------------------------------------------------------------------------------
COUT_RAGGED = [4, 36, 68, 100]      # one to four column tiles, the last one ragged: never weight-stationary
COUT_FULL = [32, 64, 96, 128]       # full tiles: the weight-stationary sizes
COUT_GROUPS = [160, 192, 256, 260]  # column groups: nt 1 x 5, 3 x 2, 4 x 2, 3 x 3
COUT_PAIR = COUT_RAGGED + COUT_FULL + COUT_GROUPS
COUT_GG_ONLY = [3, 199]             # `pair_conv` and the dense kernel refuse Cout % 4 != 0
# (Cin, split): one source, or x = [x1 | x2] with x1 `split` channels wide
CIN = [(32, 0), (96, 0), (160, 0), (256, 0), (288, 256)]
CIN_SPLITS = [(160, s) for s in (32, 64, 96, 128)]

PairCase = namedtuple("PairCase", "table mode cin split cout act")       # mode: plain | chained | direct


def _pc(table_name, mode, cin, cout, i):
    c, s = cin if isinstance(cin, tuple) else (cin, 0)
    return PairCase(table_name, mode, c, s, cout, "relu" if i % 2 else None)


def _pair_cases():
    out = []
    # every pass-1 variant on the tables that hold an empty offset AND the 127 / 128 / 129 boundary
    for i, cout in enumerate(COUT_PAIR):
        out.append(_pc("k27_m600", "plain", CIN[i % len(CIN)], cout, i))
    for i, cout in enumerate(COUT_RAGGED + COUT_FULL + [160, 256]):
        out.append(_pc("up_planted", "direct", CIN[(i + 1) % len(CIN)], cout, i))
    for i, cout in enumerate([32, 36, 64, 96, 128, 260]):
        out.append(_pc("sym27_planted", "chained", CIN[(i + 2) % len(CIN)], cout, i))
        out.append(_pc("sym27_planted", "plain", CIN[(i + 2) % len(CIN)], cout, i + 1))
    # W[k] too large for the weight-stationary kernel at a weight-stationary width: lock-step
    out += [_pc("k27_m600", "plain", 256, 128, 0), _pc("k27_m600", "plain", 128, 128, 1), _pc("up_planted", "direct", 96, 128, 1)]
    # every other table
    for i, name in enumerate(["k1_m1", "k1_m5", "k1_m130", "k3_m150", "k27_m40", "k125_m20", "down_c40", "long_run"]):
        out += [_pc(name, "plain", 32, 32, i), _pc(name, "plain", 96, 68, i + 1)]
    out += [_pc("long_run", "plain", 128, 128, 0), _pc("long_run", "plain", 160, 96, 1)]
    out += [_pc("sym27_m300", "chained", 64, 64, 0), _pc("sym27_m300", "plain", 64, 100, 1), _pc("sym27_m300", "chained", 288, 192, 1)]
    out += [_pc("up_c40", "direct", 32, 64, 0), _pc("up_c40", "direct", 96, 100, 1)]
    # a two-source split at every multiple of 32 of one width
    out += [_pc("k3_m150", "plain", cs, 64, i) for i, cs in enumerate(CIN_SPLITS)]
    # the two-group 256-column kernel: 1024 tiles of capacity or more
    out.append(_pc("big27_m6000", "plain", 32, 256, 1))
    # more tiles than workgroups: every variant walks from one offset's tiles into the next one's
    out += [_pc("big27_m6000", "plain", 32, cout, i) for i, cout in enumerate(COUT_RAGGED + COUT_FULL + [160])]
    out += [_pc("big27_m6000", "plain", 96, 128, 0)]
    out += [_pc("up_big", "direct", 64 if cout == 4 else 32, cout, i) for i, cout in enumerate(COUT_RAGGED + COUT_FULL)]
    out += [_pc("sym27_m12000", "chained", 32, cout, i) for i, cout in enumerate(COUT_FULL)]
    return out


PAIR_CASES = _pair_cases()
PAIR_FLOAT_CASES = [PairCase("k27_m600", "plain", 96, 0, 96, "relu"), PairCase("k27_m600", "plain", 288, 256, 260, "gelu"),
                    PairCase("k27_m600", "plain", 32, 0, 36, "sigmoid"), PairCase("k125_m20", "plain", 160, 0, 4, None),
                    PairCase("sym27_planted", "chained", 128, 0, 128, "relu"), PairCase("sym27_planted", "chained", 256, 0, 100, None),
                    PairCase("up_planted", "direct", 96, 0, 64, "gelu"), PairCase("up_planted", "direct", 160, 96, 68, "sigmoid"),
                    PairCase("long_run", "plain", 64, 0, 32, None), PairCase("big27_m6000", "plain", 32, 0, 256, "relu")]
RANGE_CASE = PairCase("full27_m15200", "plain", 288, 256, 256, "relu")    # a workgroup's range of more than WS_RANGE_TILES tiles


def case_id(c):
    return "-".join(str(v) for v in c)


def tiles_per_workgroup(c, crowded):
    """Real tiles per workgroup of the case's pass-1 launch (a chained table's from below: a sub-tile holds at most 128 entries)."""
    t = table(c.table)
    real, cap = tile_counts(t["counts"])
    if c.mode == "chained":
        real = -(-t["n_pairs"] // PT)
        cap = (t["n_pairs"] + 127 * (11 * (t["K"] // 2) + 1) + 127) // PT
    return real / pass1_grid(c.cin, c.cout, c.mode == "chained", c.mode == "direct", crowded, cap)


def pair_variants(c):
    """The pass-1 labels a case reaches: alone on the device and with several scenes in flight."""
    t = table(c.table)
    return {pass1_variant(c.cin, c.cout, c.mode == "chained", c.mode == "direct", crowded, capacity_tiles(t)) for crowded in (False, True)}


DENSE_ROWS = [16383, 16384, 16385, 16511]                       # 16384 = 128 tiles of 128 rows; 16385 and 16511: a last tile of 1 and 127 rows
DenseCase = namedtuple("DenseCase", "M cin split cout act")


def _dense_cases():
    out = []
    for m_i, M in enumerate((16384, 16511)):
        for i, cout in enumerate(COUT_PAIR + COUT_GG_ONLY):
            out.append(DenseCase(M, (32, 96)[(i + m_i) % 2], 0, cout, "relu" if i % 2 else None))
    for M in (16383, 16385):
        for i, cout in enumerate([4, 100, 160, 260, 199]):
            out.append(DenseCase(M, (32, 96)[i % 2], 0, cout, "relu" if i % 2 else None))
    out += [DenseCase(16385, 96, 32, 96, "relu"), DenseCase(16511, 96, 64, 260, None)]      # two sources
    return out


DENSE_CASES = _dense_cases()
# (rows, Cin, Cout) below the dense threshold: the 63 / 64 row-tile switch, the split over the four waves (steps >= 8), ragged widths
LINEAR_SHAPES = [(2016, 32, 64), (2017, 32, 64), (2016, 64, 64), (2017, 64, 64), (2016, 64, 199), (2017, 96, 160), (200, 256, 256),
                 (200, 256, 199), (200, 224, 256), (513, 32, 160), (33, 96, 36), (1, 32, 4), (5000, 32, 192), (1, 256, 3)]
LINEAR_ROWS = 5000                  # rows of the operands the shapes above cut their rows from
GG_NT = (0, 1, 2, 3, 4, -1, -11, -12, -13, -14)


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
def int_operands(V_in, M, K, Cin, Cout, seed=0):
    """-> dict(x [V_in, Cin], w [K, Cout, Cin], scale, shift [Cout], res [M, Cout]) of small integers (see the module docstring)."""
    g = gen(139, V_in, M, K, Cin, Cout, seed)
    return dict(x=torch.randint(-2, 3, (V_in, Cin), generator=g).float(), w=torch.randint(-2, 3, (K, Cout, Cin), generator=g).float(),
                scale=torch.randint(1, 4, (Cout,), generator=g).float(), shift=torch.randint(-3, 4, (Cout,), generator=g).float(),
                res=torch.randint(-3, 4, (M, Cout), generator=g).float())


def float_operands(V_in, M, K, Cin, Cout, seed=0):
    """Seeded normals; the rows of x and res spread by exp(randn), the weights scaled to keep the sums of the order of the terms."""
    g = gen(149, V_in, M, K, Cin, Cout, seed)
    return dict(x=torch.randn(V_in, Cin, generator=g) * torch.exp(torch.randn(V_in, 1, generator=g)),
                w=torch.randn(K, Cout, Cin, generator=g) * (3.0 / (max(K, 1) * Cin) ** 0.5),
                scale=0.5 + torch.rand(Cout, generator=g), shift=0.1 * torch.randn(Cout, generator=g),
                res=torch.randn(M, Cout, generator=g) * torch.exp(torch.randn(M, 1, generator=g)))


def identity_table(M):
    return torch.arange(M, dtype=torch.int32).view(1, M)


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
def act_ref(y, act):
    if act in (None, "none"):
        return y
    if act == "relu":
        return torch.relu(y)
    if act == "gelu":
        return 0.5 * y * (1 + torch.erf(y * 0.70710678118654752440))
    if act == "sigmoid":
        return 1 / (1 + torch.exp(-y))
    raise ValueError(act)


def conv_ref(x, w, nbr, scale=None, shift=None, res=None, act=None, dtype=F64, want_mag=True):
    """act(scale * sum_k w[k] @ x[nbr[k]] + shift + res) evaluated in `dtype` -> (out [M, Cout], the per-entry magnitude
    |scale| * sum |x| |w| + |shift| + |res| or None).  nbr None: the identity (a plain Linear), w [Cout, Cin] or [1, Cout, Cin].
    An entry -1 of the table gathers a row of zeros."""
    x, w = x.to(dtype), w.to(dtype)
    if w.dim() == 2:
        w = w[None]
    if nbr is None:
        nbr = identity_table(x.shape[0])
    K, M = nbr.shape
    hit = (nbr >= 0)
    src = nbr.long().clamp_min(0)
    acc = torch.zeros(M, w.shape[1], dtype=dtype)
    mag = torch.zeros(M, w.shape[1], dtype=dtype) if want_mag else None
    for k in range(K):
        g = x[src[k]] * hit[k][:, None].to(dtype)
        acc += g @ w[k].t()
        if want_mag:
            mag += g.abs() @ w[k].abs().t()
    if scale is not None:
        acc = acc * scale.to(dtype)
        mag = mag * scale.to(dtype).abs() if want_mag else None
    if shift is not None:
        acc = acc + shift.to(dtype)
        mag = mag + shift.to(dtype).abs() if want_mag else None
    if res is not None:
        acc = acc + res.to(dtype)
        mag = mag + res.to(dtype).abs() if want_mag else None
    return act_ref(acc, act), mag


def conv_pairs_ref(x, w, nbr, scale=None, shift=None, res=None, act=None):
    """The independent formulation in float64: an explicit loop over the offsets' pairs with index_add (`train_kernel_cases.conv_model`)."""
    from tests.train_kernel_cases import conv_model
    y = conv_model(x.double(), w.double(), nbr)
    if scale is not None:
        y = y * scale.double()
    if shift is not None:
        y = y + shift.double()
    if res is not None:
        y = y + res.double()
    return act_ref(y, act)


@lru_cache(maxsize=None)
def pair_int_case(c, seed=0):
    """-> (operands, float64 reference cast to fp32, magnitude) of an integer PairCase; computed once, never written to."""
    t = table(c.table)
    o = int_operands(t["V_in"], t["M"], t["K"], c.cin, c.cout, seed)
    ref, mag = conv_ref(o["x"], o["w"], t["nbr"], o["scale"], o["shift"], o["res"], c.act)
    return o, ref.float(), mag


@lru_cache(maxsize=None)
def pair_float_case(c, seed=0):
    """-> (operands, ref64, ref32 = the reference evaluated in fp32, magnitude)."""
    t = table(c.table)
    o = float_operands(t["V_in"], t["M"], t["K"], c.cin, c.cout, seed)
    r64, mag = conv_ref(o["x"], o["w"], t["nbr"], o["scale"], o["shift"], o["res"], c.act)
    r32, _ = conv_ref(o["x"], o["w"], t["nbr"], o["scale"], o["shift"], o["res"], c.act, dtype=F32, want_mag=False)
    return o, r64, r32, mag


@lru_cache(maxsize=None)
def linear_operands(Cin, Cout, rows=DENSE_ROWS[-1], kind="int", seed=0):
    """Operands of a plain Linear on up to `rows` rows (a case takes the first M rows of x and res)."""
    return (int_operands if kind == "int" else float_operands)(rows, rows, 1, Cin, Cout, seed)


def linear_ref(o, M, scale=False, shift=True, res=True, act=None, dtype=F64, want_mag=True):
    return conv_ref(o["x"][:M], o["w"], None, o["scale"] if scale else None, o["shift"] if shift else None, o["res"][:M] if res else None,
                    act, dtype=dtype, want_mag=want_mag)


# ---- the tolerance rule of the float cases --------------------------------------------------------------------------------------------------
def float_bound(r64, r32, mag, margin=MARGIN):
    e32 = scaled_error(r32, r64, mag)
    return max(8 * ULP32, margin * e32), e32


def check_conv(family, case, label, got, ref64, ref32, mag, margin=MARGIN):
    """Both assertions of the module docstring; prints / records the `[conv-forward-error]` line."""
    rerr = row_error(torch.as_tensor(got).detach().cpu(), ref64)
    got, r64, r32, sc = _arr(got), _arr(ref64), _arr(ref32), _arr(mag)
    assert got.shape == r64.shape == r32.shape == sc.shape, (family, case, got.shape, r64.shape, r32.shape, sc.shape)
    assert bool(torch.isfinite(r64).all()), (family, case, "reference not finite")
    top = float(r64.abs().max()) if r64.numel() else 0.0
    bound, e32 = float_bound(r64, r32, sc, margin)
    kerr = scaled_error(got, r64, sc)
    worst = float((got - r64).abs().max()) if r64.numel() else 0.0
    record(f"{family} | {case} | {label} | kernel {kerr:.3e} | e32 {e32:.3e} | bound {bound:.3e} | row {rerr:.3e} | row bound {ROW_TOL:.1e} | "
           f"abs {worst:.3e} | cap {CAP * top:.3e}")
    assert bool(torch.isfinite(got).all()), (family, case, "not finite")
    assert bool(((got - r64).abs() <= bound * sc + FLOOR).all()), (family, case, kerr, bound)
    assert worst <= CAP * top + FLOOR, (family, case, worst, CAP * top)
    assert rerr < ROW_TOL, (family, case, rerr)
    return kerr, e32, bound


def record_exact(family, case, label, same):
    """The line of an integer case: the error is 0 or the case fails."""
    record(f"{family} | {case} | {label} | kernel {'0.000e+00 (bit-equal)' if same else 'DIFFERS'} | e32 0.000e+00 | bound 0.000e+00 (exact)")


def reference_passes(family, ref64, ref32, mag, margin=MARGIN):
    """The fp32 evaluation of the reference against the rule (the CPU test: the reference alone passes) -> e32."""
    rerr = row_error(ref32, ref64)
    r64, r32, sc = _arr(ref64), _arr(ref32), _arr(mag)
    top = float(r64.abs().max()) if r64.numel() else 0.0
    bound, e32 = float_bound(r64, r32, sc, margin)
    worst = float((r32 - r64).abs().max()) if r64.numel() else 0.0
    assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all())
    assert bool(((r32 - r64).abs() <= bound * sc + FLOOR).all()), (family, e32, bound)
    assert worst <= CAP * top + FLOOR, (family, worst, CAP * top)
    assert rerr < ROW_TOL, (family, rerr)
    return e32
