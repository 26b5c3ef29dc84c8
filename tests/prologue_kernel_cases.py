"""Inputs for the direct tests of the prologue kernels in `segdino3d_amd/csrc/voxel.hip` (tests/test_gpu_prologue_kernels.py) and the
reference of every one of them: scene statistics, voxel keys, the run-length unique per level (with and without spconv's output-extent
clip), the stride-2 maps, per-voxel feature means, segment starts and superpoint pooling - and of the superpoint ids' key builder
`sd3d_keys_from_i64` in `csrc/sort_scan.hip`.

Inputs are seeded CPU arrays.  Integer work (quantised coordinates, keys, unique, parents, segment starts, neighbour tables, error
flags) is numpy and is compared exactly; `voxel_keys_ref` performs the kernel's fp32 operations in the same order in numpy float32.
Float work is float64; every float reference takes a dtype and can be evaluated in fp32 too.  tests/test_prologue_kernel_cases.py
checks on the CPU that the integer references agree with `oracle/sparse_ref.py`, that the fp32 evaluations stay inside their bounds, and
that a reference with one member of the largest segment dropped or counted twice does not.  Nothing here needs a GPU.

Bounds (the kernel's own output never enters one):
  * a mean of n fp32 terms x_i, added in ANY order and divided once: |error| <= (n - 1) u sum|x_i| / n + u |mean|, u = 2^-24
    (`mean_bound`).  Terms that are themselves rounded once before they are added (icoords * voxel_size in the pooled positions, x - centre
    in mode 2 of `voxel_mean`) add u sum|x_i| / n; the centre of mode 2 adds its own bound (`centre_bound`).
  * the sums of `scene_stats`: depth x u x sum|x_i| with the depth of the kernel's addition tree (`stats_chain`), as
    `decoder_kernel_cases.col_sum_bound` does for the column sums.
  * min / max and everything integer: exact.
No float output of these kernels is a purely elementwise result (each is a sum or a mean, at the least of one term), so the elementwise
rule of `loss_kernel_cases.float_bound` has nothing to apply to here: a voxel or superpoint of one point falls under `mean_bound` with
n = 1, which allows the one rounding of the division and is stricter than that rule."""
from functools import lru_cache

import numpy as np
import torch

from oracle import sparse_ref as R
from tests.decoder_kernel_cases import gen
from tests.helpers import morton_decode_np

F64, F32 = torch.float64, torch.float32
U = 2.0 ** -24                      # unit roundoff of fp32
MORTON_BITS = 48
MORTON_MASK = (1 << MORTON_BITS) - 1
VS = float(np.float32(0.02))        # the voxel size as the kernels receive it
RECORDS = []
TAG = "[prologue-kernel-error]"


def _a64(t):
    return torch.as_tensor(t).detach().cpu().double()


def check_bound(family, case, got, ref64, ref32, bound):
    """Derived absolute bound per entry: print / record the `[prologue-kernel-error]` line (largest kernel error, largest error of the
    fp32 evaluation of the reference, the bound at the worst entry) and assert."""
    got, r64, r32, b = _a64(got), _a64(ref64), _a64(ref32), _a64(bound)
    assert got.shape == r64.shape == r32.shape == b.shape, (family, case, got.shape, r64.shape, r32.shape, b.shape)
    assert bool(torch.isfinite(r64).all()), (family, case, "reference not finite")
    err, e32 = (got - r64).abs(), (r32 - r64).abs()
    ratio = err / b.clamp(min=1e-300)
    worst = int(ratio.argmax()) if ratio.numel() else 0
    line = (f"{TAG} {family} | {case} | kernel {float(err.max()) if err.numel() else 0.0:.3e} | fp32 reference {float(e32.max()) if e32.numel() else 0.0:.3e}"
            f" | bound {float(b.reshape(-1)[worst]) if b.numel() else 0.0:.3e} | error / bound {float(ratio.max()) if ratio.numel() else 0.0:.3e}")
    print(line)
    RECORDS.append(line)
    assert bool(torch.isfinite(got).all()), (family, case, "not finite")
    assert bool((err <= b).all()), (family, case, float(ratio.max()))
    return float(ratio.max()) if ratio.numel() else 0.0


def inside(ref_other, ref64, bound):
    """Every entry of `ref_other` within `bound` of `ref64` (CPU self-checks)."""
    return bool(((_a64(ref_other) - _a64(ref64)).abs() <= _a64(bound)).all())


# ---- Z-order keys ------------------------------------------------------------------------------------------------------------------------
def morton_encode_np(r):
    """[n, 3] non-negative integers below 2^16 -> Z-order code, bit 0 = x, 1 = y, 2 = z (the inverse of `helpers.morton_decode_np`)."""
    r = np.asarray(r).astype(np.int64)
    m = np.zeros(r.shape[0], dtype=np.int64)
    for b in range(16):
        for a in range(3):
            m |= ((r[:, a] >> b) & 1) << (3 * b + a)
    return m


def level_key(k, shift):
    """Key of the level `shift / 3` levels up: the Z-order part shifted, the scene bits kept."""
    k = np.asarray(k, dtype=np.int64)
    return ((k & MORTON_MASK) >> shift) | (k & ~np.int64(MORTON_MASK))


# ---- scene_stats -------------------------------------------------------------------------------------------------------------------------
STATS_N = [1, 255, 256, 257, 65536, 65537]     # 256 workgroups of 256 threads: the last value takes the grid-stride loop a second step
STATS_BLOCKS = 256


@lru_cache(maxsize=None)
def stats_case(n, width):
    """[n, width] fp32 rows, xyz in columns 0-2: far from the origin, one axis negative; the extremes sit in the last rows."""
    g = gen(101, n, width)
    p = torch.randn(n, width, generator=g)
    p[:, :3] = torch.tensor([-1500.0, 30.0, 2000.0]) + 5.0 * torch.randn(n, 3, generator=g)
    p[n - 1, 0], p[n - 1, 1] = -1600.0, 90.0                   # min x, max y in the last row (the grid-stride loop's second step at 65537)
    p[n // 2, 2] = -3.5                                        # min z of another sign than the rest
    return p


def stats_ref(xyz, dtype=F64):
    """-> [9]: min xyz, max xyz (exact in any dtype), sum xyz in `dtype`."""
    x = xyz[:, :3]
    return torch.cat([x.min(0)[0].to(dtype), x.max(0)[0].to(dtype), x.to(dtype).sum(0)])


def stats_chain(n):
    """Roundings behind one sum of `scene_stats`, read from csrc/voxel.hip: a thread adds its ceil(n / 65536) rows, the wave's butterfly
    has 6 steps, the 4 waves of a workgroup meet in 3 additions; the final kernel's lanes add up to 4 workgroup partials each and meet
    in 6 more steps.  One more for the terms of second order."""
    blocks = min(STATS_BLOCKS, -(-n // 256))
    return -(-n // (STATS_BLOCKS * 256)) + 6 + 3 + -(-blocks // 64) + 6 + 1


def stats_sum_bound(xyz):
    n = xyz.shape[0]
    return min(stats_chain(n), max(n - 1, 0)) * U * xyz[:, :3].double().abs().sum(0)


# ---- voxel_keys --------------------------------------------------------------------------------------------------------------------------
INV_VOXELS = [50.0, float(np.float32(1.0) / np.float32(0.03))]


@lru_cache(maxsize=None)
def keys_case(inv_voxel):
    """[n, 6] points whose coordinates are the exact fp32 multiples k * voxel of the voxel size, k = -300 .. 300, and `nextafter` on
    either side of each, shuffled per axis; 0.0 and -0.0 are among them (k = 0 and its negation)."""
    vox = np.float32(1.0) / np.float32(inv_voxel)
    k = np.arange(-300, 301).astype(np.float32)
    m = (k * vox).astype(np.float32)
    vals = np.concatenate([m, np.nextafter(m, np.float32(np.inf)), np.nextafter(m, np.float32(-np.inf)), np.array([-0.0], np.float32)])
    rng = np.random.default_rng(int(inv_voxel * 7) + 3)
    xyz = np.stack([rng.permutation(vals) for _ in range(3)], 1).astype(np.float32)
    return torch.from_numpy(np.concatenate([xyz, np.zeros_like(xyz)], 1))


def voxel_keys_ref(xyz, inv_voxel, stats, shift_to_min, batch_index):
    """The kernel's fp32 operations in its order, in numpy float32: c = floor((x - min) * inv_voxel) (min = 0 without shift_to_min),
    origin = floor(cmin / 16) * 16 - 32, key = Z-order code of (c - origin) & 0xFFFF | batch << 48.
    -> dict(icoords int32 [n, 3], origin int32 [3], keys int64 [n], flag: 1 = a coordinate outside [origin + 32, origin + 65536 - 64),
    2 = a Z-order code that needs more than 32 bits)."""
    x = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32)[:, :3])
    st = np.asarray(stats, dtype=np.float32)
    inv = np.float32(inv_voxel)
    mn = st[:3].copy() if shift_to_min else np.zeros(3, np.float32)
    c = np.floor(((x - mn[None, :]).astype(np.float32) * inv).astype(np.float32)).astype(np.int64)
    cmin = np.floor(((st[:3] - mn).astype(np.float32) * inv).astype(np.float32)).astype(np.int64)
    origin = (cmin // 16) * 16 - 32
    rel = c - origin[None, :]
    bad = bool(((rel < 32) | (rel >= 65536 - 64)).any())
    m = morton_encode_np(rel & 0xFFFF)
    flag = (1 if bad else 0) | (2 if bool((m >> 32).any()) else 0)
    keys = m | (np.int64(batch_index & 0xFF) << MORTON_BITS)
    return dict(icoords=c.astype(np.int32), origin=origin.astype(np.int32), keys=keys, flag=flag)


def flag_case(rel, axis):
    """Two points, unit voxels, shift_to_min: the scene's minimum at the origin (so the key origin is -32) and one point whose
    coordinate `axis` sits `rel` voxels above the key origin."""
    p = np.zeros((2, 6), np.float32)
    p[1, axis] = float(rel - 32) + 0.5
    return torch.from_numpy(p)


# ---- keys_from_i64 -----------------------------------------------------------------------------------------------------------------------
KEYS64_N = [0, 1, 63, 64, 65, 255, 256, 257, 1025]             # around a wave, a 256-thread workgroup (one atomic each for the maximum), five of them
KEYS64_ADD = [0, 5 << 32]
KEYS64_BITS = [16, 64]
KEYS64_FLAG_PRESET, KEYS64_FLAG_VALUE = 16, 4                  # the flag word is OR-ed into: an overwrite loses the 16
KEYS64_MAX_PRESETS = [0, 7]                                    # the maximum only grows
KEYS64_IDS = {"zeros": 0, "fits16": 65535, "over16": 65536, "below_limit": 0x7FFFFFFE, "limit": 0x7FFFFFFF, "negative": -1}
INT32_MAX = 0x7FFFFFFF


def keys64_positions(n):
    """First, one interior and last position of n ids (fewer when they coincide)."""
    return sorted({0, n // 2, n - 1}) if n > 0 else []


def keys64_case(n, name, pos):
    """int64 [n]: small random ids (below 100) with KEYS64_IDS[name] at position `pos`; `zeros`: every id 0."""
    x = np.random.default_rng(7000 + n).integers(0, 100, n).astype(np.int64)
    if name == "zeros":
        x[:] = 0
    elif n:
        x[pos] = KEYS64_IDS[name]
    return x


def keys_from_i64_ref(x, add, bits, flag_value, flag, max_out):
    """The contract of `sd3d_keys_from_i64` in include/segdino3d_hip.h: keys[i] = x[i] + add (mod 2^64); on the ids x[i], read as
    unsigned: flag |= flag_value when one does not fit `bits` bits (bits = 64: no check), flag |= 8 when one is negative or above
    INT32_MAX - 1, max_out = max(max_out, largest id clamped to INT32_MAX).  -> (keys uint64 [n], flag, max_out)"""
    u = np.asarray(x, dtype=np.int64).view(np.uint64)
    keys = u + np.uint64(add % (1 << 64))
    if len(u):
        top = int(u.max())
        if bits < 64 and top >> bits:
            flag |= flag_value
        if top > INT32_MAX - 1:
            flag |= 8
        max_out = max(max_out, min(top, INT32_MAX))
    return keys, flag, max_out


# ---- run-length unique, levels -----------------------------------------------------------------------------------------------------------
def levels_ref(skeys, sidx, n_levels):
    """Sorted keys [n] (int64), the points they came from [n] | None -> dict(ukeys [L x [V_l]], seg_start [V_0 + 1], inverse [n],
    parents [(L - 1) x [V_{l-1}]], counts [L])."""
    skeys = np.asarray(skeys, dtype=np.int64)
    n = len(skeys)
    ids, ukeys = [], []
    for l in range(n_levels):
        k = level_key(skeys, 3 * l)
        head = np.concatenate([[True], k[1:] != k[:-1]])
        ids.append(np.cumsum(head) - 1)
        ukeys.append(k[head])
        if l == 0:
            seg_start = np.concatenate([np.nonzero(head)[0], [n]]).astype(np.int32)
    inverse = np.empty(n, dtype=np.int32)
    inverse[np.arange(n) if sidx is None else np.asarray(sidx, dtype=np.int64)] = ids[0]
    parents = []
    for l in range(1, n_levels):
        par = np.empty(len(ukeys[l - 1]), dtype=np.int32)
        par[ids[l - 1]] = ids[l]
        parents.append(par)
    return dict(ukeys=ukeys, seg_start=seg_start, inverse=inverse, parents=parents, counts=np.array([len(u) for u in ukeys], np.int32))


@lru_cache(maxsize=None)
def sorted_keys_case(kind):
    """-> (sorted keys int64 [n], src_idx int32 [n]).  `runs`: 1400 voxels with 1 - 9 points each and runs of 300 and 600 equal keys, so
    that runs cross the boundaries of the 256-thread workgroups; `one`; `equal`: 700 equal keys; `distinct`: 700 different ones.  Z-order
    codes below 2^20 with two scene indices: five levels merge them step by step."""
    rng = np.random.default_rng({"runs": 1, "one": 2, "equal": 3, "distinct": 4}[kind])
    if kind == "one":
        keys = np.array([0x2F3A7], dtype=np.int64)
    elif kind == "equal":
        keys = np.full(700, 0x51C33 | (1 << MORTON_BITS), dtype=np.int64)
    elif kind == "distinct":
        keys = np.sort(rng.choice(1 << 20, 700, replace=False).astype(np.int64))
    else:
        v = np.sort(rng.choice(1 << 20, 1400, replace=False).astype(np.int64))
        v[700:] |= np.int64(1) << MORTON_BITS                  # the second scene of a batch
        v = np.sort(v)
        reps = rng.integers(1, 10, 1400)
        reps[100], reps[900] = 300, 600
        keys = np.repeat(v, reps)
    return keys, rng.permutation(len(keys)).astype(np.int32)


@lru_cache(maxsize=None)
def level_scene(n=4000):
    """[n, 6] points of a 0.3 x 0.4 x 0.2 m box around (-1, 2, 0.5): a few points per 2 cm voxel, negative coordinates on one axis."""
    g = gen(131, n)
    p = torch.zeros(n, 6)
    p[:, :3] = torch.tensor([-1.0, 2.0, 0.5]) + torch.rand(n, 3, generator=g) * torch.tensor([0.3, 0.4, 0.2])
    return p


# ---- spconv's output-extent clip ---------------------------------------------------------------------------------------------------------
CLIP_MIN = 128
CLIP_LEVELS = 4
# extents per axis -> what happens to the voxels of the trailing slice: D < 128 is clamped to 128 (nothing dropped); 129 -> 64: x = 128
# dropped at level 1; 130 -> 65 -> 32: x = 129 dropped at level 2; 132 -> 66 -> 33 -> 16: x = 131 dropped at level 3; 136 -> 68 -> 34 -> 17:
# wider than 128 and nothing dropped
CLIP_GRIDS = {"narrow": (100, 90, 60), "level1": (129, 40, 40), "level2": (40, 130, 40), "level3": (40, 40, 132), "all": (129, 130, 132),
              "even": (136, 136, 136)}


@lru_cache(maxsize=None)
def clip_grid(name):
    """Unique integer voxel coordinates [V, 3] int32 (in `pack` order, like `unique_voxels`) inside the box of `CLIP_GRIDS[name]`: 900
    random ones, the two corners, and 40 in the trailing slice (the last two planes) of every axis."""
    D = np.array(CLIP_GRIDS[name], dtype=np.int64)
    rng = np.random.default_rng(sum(CLIP_GRIDS[name]))
    c = [rng.integers(0, D, (900, 3)), np.zeros((1, 3), np.int64), (D - 1)[None, :]]
    for a in range(3):
        t = rng.integers(0, D, (40, 3))
        t[:, a] = D[a] - 1 - rng.integers(0, 2, 40)
        t[:3, a] = D[a] - 1
        c.append(t)
    return R.unique_voxels(np.concatenate(c).astype(np.int32))[0]


def grid_points(coords, voxel_size, offset=(0.0, 0.0, 0.0), seed=0):
    """One to three points per voxel at its centre (the corner voxel's at its lower corner: it is the scene's minimum, and the other
    points then sit half a voxel clear of every boundary after the shift), shuffled.  -> ([n, 6] fp32, voxel of every point)."""
    rng = np.random.default_rng(seed + 17)
    vox = np.repeat(np.arange(len(coords)), rng.integers(1, 4, len(coords)))
    vox = rng.permutation(vox)
    xyz = (coords[vox].astype(np.float64) + 0.5) * voxel_size
    xyz[(coords[vox] == 0).all(1)] = 0.0
    p = np.zeros((len(vox), 6), np.float32)
    p[:, :3] = (xyz + np.asarray(offset)[None, :]).astype(np.float32)
    return torch.from_numpy(p), vox


def clipped_levels_ref(coords0, n_levels, min_shape=CLIP_MIN, key_offset=32):
    """Integer model of spconv's SparseConv3d(k = 2, s = 2, p = 0) levels on unique level-0 coordinates (any order): a child c has the
    parent c // 2 if that lies inside the output extent (D - 2) // 2 + 1, D_0 = max(cmax + 1, min_shape), and none otherwise.
    -> (coords per level, parent index per level pair, -1 = dropped).  The rows of a level are in the device's order: the Z-order of
    c + (key_offset >> level), the key origin of shift_to_min coordinates lying `key_offset` level-0 voxels below the scene's minimum."""
    c0 = np.asarray(coords0, dtype=np.int64)
    coords = [c0[np.argsort(morton_encode_np(c0 + key_offset), kind="stable")]]
    shape = np.maximum(coords[0].max(0) + 1, min_shape)
    parents = []
    for level in range(1, n_levels):
        c = coords[-1]
        shape = (shape - 2) // 2 + 1
        o = c // 2
        valid = (o < shape[None, :]).all(1)
        code = morton_encode_np(o + (key_offset >> level))
        uc = np.unique(code[valid])
        par = np.full(len(c), -1, dtype=np.int32)
        par[valid] = np.searchsorted(uc, code[valid])
        parents.append(par)
        coords.append(morton_decode_np(uc) - (key_offset >> level))
    return coords, parents


def stride_tables_ref(fine, coarse, parent, order):
    """(down [8, V_coarse], up [8, V_fine]) int32 of the k = 2 s = 2 convolution and its transpose: child j of parent p sits at kernel
    offset (c_j - 2 c_p), enumerated x-fastest or z-fastest; a dropped child has no entry."""
    down = np.full((8, len(coarse)), -1, dtype=np.int32)
    up = np.full((8, len(fine)), -1, dtype=np.int32)
    for j in np.nonzero(parent >= 0)[0]:
        p = parent[j]
        r = fine[j] - 2 * coarse[p]
        assert ((r >= 0) & (r < 2)).all()
        k = r[0] + 2 * r[1] + 4 * r[2] if order == "x_fastest" else (r[0] * 2 + r[1]) * 2 + r[2]
        down[k, p], up[k, j] = j, p
    return down, up


def conv_ref(x, w, nbr, scale, shift, res, relu=True):
    """float64 model of the sparse convolution: out[r] = relu(scale * sum_k x[nbr[k][r]] . w[k]^T + shift + res[r])."""
    K, M = nbr.shape
    acc = torch.zeros(M, w.shape[1], dtype=F64)
    xd, wd = x.double(), w.double()
    for k in range(K):
        rows = np.nonzero(nbr[k] >= 0)[0]
        if len(rows):
            acc[rows] += xd[nbr[k][rows]] @ wd[k].t()
    out = acc * scale.double() + shift.double() + res.double()
    return torch.relu(out) if relu else out


# ---- means -------------------------------------------------------------------------------------------------------------------------------
def mean_bound(terms64, index, n_seg, rounded_terms=False):
    """Per entry of `segment_mean(terms, index, n_seg)`: (n - 1) u sum|x_i| / n + u |mean| for any order of the additions; terms that
    were rounded once before they were added (`rounded_terms`) add u sum|x_i| / n."""
    t = terms64.double()
    cnt = torch.bincount(torch.from_numpy(np.asarray(index, dtype=np.int64)), minlength=n_seg).clamp(min=1).double()[:, None]
    mabs = R.segment_mean(t.abs(), index, n_seg)               # sum|x_i| / n
    mean = R.segment_mean(t, index, n_seg)
    return ((cnt - 1) * U * mabs + U * mean.abs() + (U * mabs if rounded_terms else 0.0))


VM_POPULATIONS = [1, 2, 3, 4, 5, 7, 8, 9, 64, 700] + [1] * 9 + [2, 3]       # points per voxel of one scene; the largest is voxel 9
VM_SHAPES = [(1, 0), (0, 61), (2, 59), (0, 256), (2, 256), (0, 317)]        # (mode, F): C = 3, 64, 65, 259, 262, 320
VM_GENERIC = (0, 768)                                                       # C = 771 on the path for ld_out > 320
VM_BRANCH = [((2, 256), 320), ((2, 256), 352), ((0, 317), 352)]             # the same C on either side of the branch at ld_out = 320


def vm_channels(mode, F):
    return 3 if mode == 1 else (3 + F if mode == 0 else 6 + F)


def round_up(v, m):
    return -(-v // m) * m


@lru_cache(maxsize=None)
def vm_scene(seed=0, populations=tuple(VM_POPULATIONS)):
    """Points [n, 6] about 30 m from the origin (xyz, rgb), the voxel of every point (shuffled), sorted_idx (the points voxel by voxel,
    ascending inside a voxel, like a stable sort) and seg_start."""
    g = gen(211, seed)
    pop = np.array(populations)
    n = int(pop.sum())
    vox = np.repeat(np.arange(len(pop)), pop)[torch.randperm(n, generator=g).numpy()]
    pts = torch.cat([torch.tensor([30.0, -28.0, 31.0]) + 3.0 * torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)], 1)
    sidx = np.argsort(vox, kind="stable").astype(np.int32)
    seg = np.concatenate([[0], np.cumsum(pop)]).astype(np.int32)
    return dict(n=n, n_vox=len(pop), pts=pts, vox=vox, sidx=sidx, seg_start=seg, largest=int(pop.argmax()))


@lru_cache(maxsize=None)
def vm_feats(n, F, seed=0):
    """2D features with a large common mean."""
    return 50.0 + 4.0 * torch.randn(n, F, generator=gen(223, n, F, seed))


def vm_rows(pts, f2d, mode, dtype=F64, centre=None):
    """The assembled feature row of every point: mode 0 [rgb | f2d], 1 [rgb], 2 [rgb | xyz - centre | f2d]; centre = the scene's mean
    position in `dtype` unless given."""
    p = pts.to(dtype)
    if mode == 1:
        return p[:, 3:6].clone()
    if mode == 0:
        return torch.cat([p[:, 3:6], f2d.to(dtype)], 1)
    c = p[:, :3].mean(0) if centre is None else centre.to(dtype)
    return torch.cat([p[:, 3:6], p[:, :3] - c, f2d.to(dtype)], 1)


def vm_centre32(pts):
    """The centre as the kernel forms it, in fp32: sum * (1 / n)."""
    return pts[:, :3].float().sum(0) * torch.tensor(1.0 / pts.shape[0], dtype=F32)


def centre_bound(pts):
    """|fp32 centre - mean xyz|: the bound of the statistics' sum over n, the rounding of 1 / n and of the product."""
    return stats_sum_bound(pts) / pts.shape[0] + 3 * U * pts[:, :3].double().mean(0).abs()


def vm_ref(sc, f2d, mode, dtype=F64):
    rows = vm_rows(sc["pts"], f2d, mode, dtype, centre=vm_centre32(sc["pts"]) if dtype == F32 else None)
    return R.segment_mean(rows, sc["vox"], sc["n_vox"])


def vm_bound(sc, f2d, mode):
    rows = vm_rows(sc["pts"], f2d, mode)
    b = mean_bound(rows, sc["vox"], sc["n_vox"])
    if mode == 2:                                               # x - centre: rounded once per term, and the centre's own error
        b[:, 3:6] += U * R.segment_mean(rows[:, 3:6].abs(), sc["vox"], sc["n_vox"]) + centre_bound(sc["pts"])[None, :]
    return b


def drop_or_double(terms, index, n_seg, seg, double):
    """`segment_mean` with one member of segment `seg` left out (the count with it) or counted twice: what a wrong lane mask or an
    off-by-one at a pass boundary computes.  -> the row of `seg`."""
    members = np.nonzero(np.asarray(index) == seg)[0]
    victim = members[len(members) // 2]
    keep = np.concatenate([members, [victim]]) if double else members[members != victim]
    return terms[keep].double().sum(0) / len(keep)


# ---- segment starts ----------------------------------------------------------------------------------------------------------------------
def segment_starts_ref(dense_ids, S):
    """start[s] = first position whose (sorted) id is >= s, s = 0 .. S: an id above S is as good as S."""
    return np.searchsorted(np.asarray(dense_ids, dtype=np.int64), np.arange(S + 1), side="left").astype(np.int32)


@lru_cache(maxsize=None)
def seg_ids_case(n, S, seed=0):
    """n sorted ids below S with leading and trailing unused ids and long gaps (S >= 40), or all of them 0 (S = 1)."""
    rng = np.random.default_rng(1000 * n + S + seed)
    if S == 1:
        return np.zeros(n, dtype=np.int64)
    used = np.sort(rng.choice(np.arange(7, S - 9), size=min(n, max(1, (S - 16) // 5)), replace=False))
    return np.sort(used[rng.integers(0, len(used), n)]).astype(np.int64)


# ---- superpoint pooling ------------------------------------------------------------------------------------------------------------------
POOL_SIZES = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513, 700]
POOL_ORDER = [5, 0, 13, 2, 9, 1, 12, 4, 0, 8, 3, 11, 6, 10, 7, 0]          # indices into POOL_SIZES: empty segments first, inside and last
POOL_C = [4, 32, 64, 96]
POOL_VOX = 600


@lru_cache(maxsize=None)
def pool_case(C):
    """feat [V, C]; per point: its voxel (`inverse`), quantised coordinates (negative too), its segment; sorted_idx / start as
    `segment_starts` leaves them.  Half of the points of the largest segment share one voxel."""
    g = gen(307, C)
    sizes = np.array([POOL_SIZES[i] for i in POOL_ORDER])
    n, S = int(sizes.sum()), len(sizes)
    seg_sorted = np.repeat(np.arange(S), sizes)
    sidx = torch.randperm(n, generator=g).numpy().astype(np.int32)           # sorted position -> point
    seg = np.empty(n, dtype=np.int64)
    seg[sidx] = seg_sorted
    inverse = torch.randint(0, POOL_VOX, (n,), generator=g).numpy().astype(np.int32)
    largest = int(sizes.argmax())
    members = np.nonzero(seg == largest)[0]
    inverse[members[::2]] = 17
    icoords = torch.randint(-150, 151, (n, 3), generator=g).numpy().astype(np.int32)
    icoords[:, 2] += 400                                        # one axis with a common offset
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return dict(C=C, n=n, S=S, feat=torch.randn(POOL_VOX, C, generator=g), inverse=inverse, icoords=icoords, seg=seg, sidx=sidx, start=start,
                sizes=sizes, largest=largest)


def pool_terms(c, dtype=F64):
    """-> (feature row of every point, position term of every point) in `dtype`."""
    f = c["feat"].to(dtype)[torch.from_numpy(c["inverse"].astype(np.int64))]
    pos = torch.from_numpy(c["icoords"]).to(dtype) * torch.tensor(VS, dtype=dtype)
    return f, pos


def pool_ref(c, dtype=F64):
    f, pos = pool_terms(c, dtype)
    return R.segment_mean(f, c["seg"], c["S"]), R.segment_mean(pos, c["seg"], c["S"])


def pool_bound(c):
    f, pos = pool_terms(c)
    return mean_bound(f, c["seg"], c["S"]), mean_bound(pos, c["seg"], c["S"], rounded_terms=True)
