"""The rule of segdino3d_amd/fuse_views.py (include/segdino3d_hip.h, "Fusion of posed RGB-D frames") restated in numpy: what
csrc/fuse_views.hip is tested against, bit for bit, since the reference ships no code that makes `points`.

Steps 1-3 and 5-7 are integer decisions or single rounded fp32 operations and are written once; only the back-projection of step 4
runs in `dtype`: float32 is what the kernels must EQUAL, float64 gives the share of pixels whose cell the fp32 arithmetic moves.

  1. Depth pixel (vi, ui) takes part iff vi % stride == 0 and ui % stride == 0; it reads colour pixel
     (((2 vi + 1) Hc) // (2 Hd), ((2 ui + 1) Wc) // (2 Wd)).
  2. d = (float)raw * depth_scale, one rounded fp32 multiply (fp32 depth as it is); valid iff d > 0, d >= near, d <= far in fp32.
  3. Unless edge_rel is None: each of the 4 neighbours inside the image, whatever the stride, with depth dn by step 2, is a jump iff
     !(dn > 0) or |dn - d| > edge_abs + edge_rel * d (one rounded multiply, one rounded add, one rounded subtract); any jump drops.
  4. x = (ui - cx) * d / fx, y likewise, w_i = ((R_i0 x + R_i1 y) + R_i2 d) + R_i3, every operation rounded on its own in `dtype`;
     unless all w_i are finite with |w_i| < 2^14 the pixel is dropped and counted in out_of_range.
  5. c_i = floorf(w_i * inv_voxel), inv_voxel = float32(1.0 / voxel); unless -2^20 <= c_i < 2^20 on all axes (as floats) the pixel is
     dropped and counted in out_of_range; key = ((c_x + 2^20) << 42) | ((c_y + 2^20) << 21) | (c_z + 2^20).
  6. Per cell: n += 1, S_i += (int64) rint((double) w_i * 2^20), C_j += colour byte j.
  7. The cells with n >= min_obs in ascending key order: xyz_i = float32((double) S_i / (double) n / 2^20),
     rgb_j = float32((double) C_j / (double) n), obs = n."""
from collections import namedtuple

import numpy as np

FIXED_BITS = 20                   # SD3D_FUSE_FIXED_BITS
WORLD_BITS = 14                   # SD3D_FUSE_WORLD_BITS
CELL_BITS = 20                    # SD3D_FUSE_CELL_BITS
TILE_H, TILE_W = 8, 32            # the kernel's tile of participating pixels: only `tile_stats` uses it
RULE_DEFAULTS = dict(voxel=0.02, near=0.1, far=6.0, stride=1, edge_abs=0.02, edge_rel=0.02, min_obs=2)

State = namedtuple("State", "keys n S C pixels_used out_of_range")
State.__doc__ = """The integer state of a fusion: keys uint64 [M] ascending and unique, n int64 [M], S int64 [M, 3], C int64 [M, 3], and the
counters pixels_used (observations added to a cell) and out_of_range (dropped at steps 4 and 5)."""


def rule(**kw):
    bad = set(kw) - set(RULE_DEFAULTS)
    assert not bad, bad
    return {**RULE_DEFAULTS, **kw}


def cam_to_world(poses):
    """poses float64 [V, 4, 4] -> (fp32 [K, 3, 4], kept int64 [K]): views with a non-finite pose are dropped."""
    poses = np.asarray(poses, dtype=np.float64)
    kept = np.flatnonzero(np.isfinite(poses).all(axis=(1, 2)))
    return np.ascontiguousarray(poses[kept][:, :3, :].astype(np.float32)), kept


def depth_metres(depth, depth_scale):
    """Step 2's conversion -> fp32, the shape of `depth`."""
    if depth.dtype == np.uint16:
        return depth.astype(np.float32) * np.float32(depth_scale)
    assert depth.dtype == np.float32 and depth_scale is None
    return depth


def valid_pixels(d, near, far, edge_abs, edge_rel):
    """Steps 2 and 3 for one view: d fp32 [Hd, Wd] -> bool [Hd, Wd] (before the stride)."""
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (d > np.float32(0)) & (d >= np.float32(near)) & (d <= np.float32(far))
        if edge_rel is not None:
            thr = np.float32(edge_abs) + np.float32(edge_rel) * d                     # one rounded multiply, one rounded add
            H, W = d.shape
            for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                dn = np.full_like(d, np.float32(1))
                inside = np.zeros((H, W), dtype=bool)
                ys, yd = (slice(0, H - 1), slice(1, H)) if dy < 0 else (slice(1, H), slice(0, H - 1)) if dy > 0 else (slice(0, H), slice(0, H))
                xs, xd = (slice(0, W - 1), slice(1, W)) if dx < 0 else (slice(1, W), slice(0, W - 1)) if dx > 0 else (slice(0, W), slice(0, W))
                dn[yd, xd] = d[ys, xs]                                                # pixel (yd, xd) sees its neighbour (ys, xs)
                inside[yd, xd] = True
                jump = ~(dn > np.float32(0)) | (np.abs(dn - d) > thr)
                ok &= ~(inside & jump)
    return ok


def observations(depth, depth_scale, intr, c2w, colors, dtype=np.float32, **kw):
    """Steps 1-5 for kept views: depth uint16 / fp32 [V, Hd, Wd], intr fp32 [V, 4], c2w fp32 [V, 3, 4], colors uint8 [V, Hc, Wc, 3] ->
    dict(key uint64 [P], w fp32 [P, 3], rgb uint8 [P, 3], view / vi / ui int64 [P], out_of_range int)."""
    r = rule(**kw)
    V, Hd, Wd = depth.shape
    Hc, Wc = colors.shape[1:3]
    assert colors.shape[0] == V and colors.shape[3] == 3 and colors.dtype == np.uint8
    s = int(r["stride"])
    inv_voxel = np.float32(1.0 / float(r["voxel"]))
    f = dtype
    out = dict(key=[], w=[], rgb=[], view=[], vi=[], ui=[])
    out_of_range = 0
    for v in range(V):
        d = depth_metres(depth[v], depth_scale)
        ok = valid_pixels(d, r["near"], r["far"], r["edge_abs"], r["edge_rel"])
        take = np.zeros_like(ok)
        take[::s, ::s] = True                                                         # step 1
        vi, ui = np.nonzero(ok & take)
        z = d[vi, ui].astype(f)
        fx, fy, cx, cy = (f(x) for x in intr[v])
        R = c2w[v].astype(f)
        with np.errstate(all="ignore"):                                               # step 4, every operation in `dtype`, left to right
            x = (ui.astype(f) - cx) * z / fx
            y = (vi.astype(f) - cy) * z / fy
            w = np.stack([((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z) + R[i, 3] for i in range(3)], axis=1)
            fine = (np.isfinite(w) & (np.abs(w) < f(2 ** WORLD_BITS))).all(axis=1)
            w32 = w.astype(np.float32)                                                # steps 5-7 are written once, on fp32
            c = np.floor(w32 * inv_voxel)                                             # step 5: one rounded fp32 multiply
            fine &= ((c >= np.float32(-2 ** CELL_BITS)) & (c < np.float32(2 ** CELL_BITS))).all(axis=1)
        out_of_range += int((~fine).sum())
        vi, ui, w32, c = vi[fine], ui[fine], w32[fine], c[fine]
        ci = (c.astype(np.int64) + (1 << CELL_BITS)).astype(np.uint64)
        out["key"].append((ci[:, 0] << np.uint64(42)) | (ci[:, 1] << np.uint64(21)) | ci[:, 2])
        out["w"].append(w32)
        out["rgb"].append(colors[v][((2 * vi + 1) * Hc) // (2 * Hd), ((2 * ui + 1) * Wc) // (2 * Wd)])
        out["view"].append(np.full(len(vi), v, dtype=np.int64))
        out["vi"].append(vi)
        out["ui"].append(ui)
    empty = dict(key=np.zeros(0, np.uint64), w=np.zeros((0, 3), np.float32), rgb=np.zeros((0, 3), np.uint8), view=np.zeros(0, np.int64),
                 vi=np.zeros(0, np.int64), ui=np.zeros(0, np.int64))
    res = {k: (np.concatenate(a) if len(a) else empty[k]) for k, a in out.items()}
    res["out_of_range"] = out_of_range
    return res


def _reduce(keys, n, S, C):
    uk, inv = np.unique(keys, return_inverse=True)
    n2, S2, C2 = np.zeros(len(uk), np.int64), np.zeros((len(uk), 3), np.int64), np.zeros((len(uk), 3), np.int64)
    np.add.at(n2, inv, n)
    np.add.at(S2, inv, S)
    np.add.at(C2, inv, C)
    return uk, n2, S2, C2


def accumulate(obs):
    """Step 6 over the observations of `observations` -> State."""
    fixed = np.rint(obs["w"].astype(np.float64) * 2.0 ** FIXED_BITS).astype(np.int64)
    P = len(obs["key"])
    return State(*_reduce(obs["key"], np.ones(P, np.int64), fixed, obs["rgb"].astype(np.int64)), P, obs["out_of_range"])


def merge(a, b):
    """The state after both `a` and `b`: integer sums, so the order and the cut cannot matter."""
    return State(*_reduce(np.concatenate([a.keys, b.keys]), np.concatenate([a.n, b.n]), np.concatenate([a.S, b.S]), np.concatenate([a.C, b.C])),
                 a.pixels_used + b.pixels_used, a.out_of_range + b.out_of_range)


def emit(state, min_obs=2):
    """Step 7 -> dict(points fp32 [N, 6], obs int32 [N], keys uint64 [N], cells, pixels_used, out_of_range)."""
    keep = state.n >= min_obs
    n = state.n[keep].astype(np.float64)
    xyz = (state.S[keep].astype(np.float64) / n[:, None] / 2.0 ** FIXED_BITS).astype(np.float32)
    rgb = (state.C[keep].astype(np.float64) / n[:, None]).astype(np.float32)
    return dict(points=np.concatenate([xyz, rgb], axis=1), obs=state.n[keep].astype(np.int32), keys=state.keys[keep], cells=len(state.keys),
                pixels_used=state.pixels_used, out_of_range=state.out_of_range)


def fuse_kept(depth, depth_scale, intr, c2w, colors, dtype=np.float32, **kw):
    """The whole rule for kept views with the fp32 cam_to_world [V, 3, 4] given."""
    r = rule(**kw)
    return emit(accumulate(observations(depth, depth_scale, intr, c2w, colors, dtype, **kw)), r["min_obs"])


def fuse(depth, depth_scale, intr, poses, colors, dtype=np.float32, **kw):
    """The whole rule for one batch of GIVEN views (float64 poses [V, 4, 4]; colours per given view)."""
    c2w, kept = cam_to_world(poses)
    return fuse_kept(depth[kept], depth_scale, intr[kept], c2w, colors[kept], dtype, **kw)


def tile_stats(obs, stride=1):
    """(cells, observations per cell, observations per (view, tile, cell)): what the kernel's on-chip combining saves."""
    P = len(obs["key"])
    if P == 0:
        return 0, 0.0, 0.0
    cells = len(np.unique(obs["key"]))
    ty, tx = (obs["vi"] // stride) // TILE_H, (obs["ui"] // stride) // TILE_W
    tile = (obs["view"] << 40) | (ty << 20) | tx
    pairs = len(np.unique(np.stack([tile.astype(np.uint64), obs["key"]], axis=1), axis=0))
    return cells, P / cells, P / pairs
