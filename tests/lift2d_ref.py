"""Numpy restatement of the multi-view lifting rule of segdino3d_amd/lift2d.py (include/segdino3d_hip.h states it in full).  The
reference project has no code that makes `points_2dfeats`, so THIS file is what the kernels are pinned against; tests/test_lift2d_ref.py
pins it in turn (torch's `grid_sample` on the CPU, analytic fields, hand-made edge cases).

Everything is evaluated in `dtype` (float64 by default).  `dtype=np.float32` evaluates the same expressions in single precision: the
deviation between the two is the yardstick of the value tolerance in tests/test_gpu_lift2d.py.  Inputs are the fp32 / fp16 / uint16
values the device sees (the world-to-camera matrices are inverted in float64 and rounded to fp32 first, as the wrapper does)."""
import numpy as np

RULE = dict(near=0.05, border=0, tol_abs=0.05, tol_rel=0.0)

# outcome of a (point, view) pair, in the order the rule decides it
BEHIND, OUTSIDE, NO_DEPTH, OCCLUDED, VISIBLE = 0, 1, 2, 3, 4


def world_to_cam(cam_to_world):
    """[V, 4, 4] -> (fp32 [K, 3, 4], kept [K]): poses with a non-finite entry are dropped, the others inverted in float64."""
    pose = np.asarray(cam_to_world, dtype=np.float64)
    kept = np.flatnonzero(np.isfinite(pose).all(axis=(1, 2)))
    inv = np.linalg.inv(pose[kept]) if len(kept) else np.zeros((0, 4, 4))
    return np.ascontiguousarray(inv[:, :3, :].astype(np.float32)), kept


def depth_metres(depth, depth_scale, dtype=np.float64):
    depth = np.asarray(depth)
    if depth.dtype == np.uint16:
        return depth.astype(dtype) * dtype(np.float32(depth_scale))
    assert depth.dtype == np.float32 and depth_scale is None
    return depth.astype(dtype)


def project(points, w2c, intr, dtype=np.float64):
    """-> z, u, v [N, V]"""
    with np.errstate(all="ignore"):
        p = np.asarray(points)[:, :3].astype(dtype)
        m = np.asarray(w2c).astype(dtype)
        k = np.asarray(intr).astype(dtype)
        cam = np.einsum("vij,nj->nvi", m[:, :, :3], p) + m[None, :, :, 3]
        z = cam[..., 2]
        u = k[None, :, 0] * cam[..., 0] / z + k[None, :, 2]
        v = k[None, :, 1] * cam[..., 1] / z + k[None, :, 3]
    return z, u, v


def outcomes(points, w2c, intr, depth, depth_scale=None, near=0.05, border=0, tol_abs=0.05, tol_rel=0.0, dtype=np.float64, margins=False):
    """Outcome code [N, V] of every pair; with `margins` also the distance [N, V] of the closest decision the pair REACHES from its
    boundary (pixels for the rounding, metres for `near` and the depth test; inf where a non-finite value decides)."""
    d_all = depth_metres(depth, depth_scale, dtype)
    V, Hd, Wd = d_all.shape
    z, u, v = project(points, w2c, intr, dtype)
    half = dtype(0.5)
    with np.errstate(all="ignore"):
        front = z > dtype(near)
        uf, vf = np.floor(u + half), np.floor(v + half)
        inside = front & (uf >= border) & (uf < Wd - border) & (vf >= border) & (vf < Hd - border)
        ui = np.where(inside, uf, 0).astype(np.int64)
        vi = np.where(inside, vf, 0).astype(np.int64)
        d = d_all[np.arange(V)[None, :], vi, ui]
        has = inside & (d > 0)
        err = np.abs(d - z) - (dtype(tol_abs) + dtype(tol_rel) * d)
        vis = has & (err <= 0)
    out = np.full(z.shape, BEHIND, dtype=np.int8)
    out[front] = OUTSIDE
    out[inside] = NO_DEPTH
    out[has] = OCCLUDED
    out[vis] = VISIBLE
    if not margins:
        return out
    with np.errstate(all="ignore"):
        big = np.inf
        m = np.where(np.isfinite(z), np.abs(z - near), big)

        def rounding(t, size):                 # distance of t + 0.5 from the nearest integer: where the pixel, or the bound, changes
            s = t + 0.5                        # (bounds are integers for every border; far outside the image nothing can change)
            return np.where(np.isfinite(s) & (s > -border - 3) & (s < size + border + 3), np.abs(s - np.round(s)), big)
        m = np.where(front, np.minimum(m, np.minimum(rounding(u, Wd), rounding(v, Hd))), m)
        m = np.where(has, np.minimum(m, np.abs(err)), m)
    return out, m


def pack_bits(vis):
    """bool [N, V] -> int32 [N, ceil(V / 32)], bit v % 32 of word v // 32."""
    N, V = vis.shape
    W = (V + 31) // 32
    pad = np.zeros((N, W * 32), dtype=np.uint64)
    pad[:, :V] = vis
    words = (pad.reshape(N, W, 32) << np.arange(32, dtype=np.uint64)[None, None, :]).sum(axis=2)
    return words.astype(np.uint32).view(np.int32)


def sample(fmap, xf, yf, dtype=np.float64):
    """Bilinear samples of one channels-last map [Hf, Wf, C] at map coordinates xf, yf [M] with the tap indices clamped to the map."""
    Hf, Wf, _ = fmap.shape
    xf, yf = xf.astype(dtype), yf.astype(dtype)
    x0, y0 = np.floor(xf), np.floor(yf)
    wx, wy = (xf - x0)[:, None], (yf - y0)[:, None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb = np.clip(x0, 0, Wf - 1), np.clip(x0 + 1, 0, Wf - 1)
    ya, yb = np.clip(y0, 0, Hf - 1), np.clip(y0 + 1, 0, Hf - 1)
    f = fmap.astype(dtype)
    one = dtype(1.0)
    return (one - wy) * (one - wx) * f[ya, xa] + (one - wy) * wx * f[ya, xb] + wy * (one - wx) * f[yb, xa] + wy * wx * f[yb, xb]


def lift(points, w2c, intr, depth_hw, maps, vis, dtype=np.float64):
    """`maps`: list over the scales of [V, Hf, Wf, C]; `vis` bool [N, V] -> (out [N, C], [mean_s], count [N]) in `dtype`."""
    Hd, Wd = depth_hw
    N, V = vis.shape
    _, u, v = project(points, w2c, intr, dtype)
    count = vis.sum(axis=1).astype(np.int32)
    half = dtype(0.5)
    means = []
    for fm in maps:
        _, Hf, Wf, C = fm.shape
        total = np.zeros((N, C), dtype=dtype)
        for j in range(V):                                            # ascending view order
            idx = np.flatnonzero(vis[:, j])
            if len(idx) == 0:
                continue
            xf = (u[idx, j] + half) * dtype(Wf) / dtype(Wd) - half
            yf = (v[idx, j] + half) * dtype(Hf) / dtype(Hd) - half
            total[idx] += sample(fm[j], xf, yf, dtype)
        mean = np.zeros_like(total)
        seen = count > 0
        mean[seen] = total[seen] / count[seen, None].astype(dtype)
        means.append(mean)
    out = means[0].copy()
    for m in means[1:]:
        out = out + m
    return out / dtype(len(maps)), means, count


def lift_point_features(points, cam_to_world, intr, depth, maps, depth_scale=None, dtype=np.float64, **rule):
    """The whole step from the raw inputs: -> (out, means, count, kept)."""
    w2c, kept = world_to_cam(cam_to_world)
    intr, depth = np.asarray(intr)[kept], np.asarray(depth)[kept]
    maps = [np.asarray(m)[kept] for m in maps]
    vis = outcomes(points, w2c, intr, depth, depth_scale, dtype=dtype, **{**RULE, **rule}) == VISIBLE
    return lift(points, w2c, intr, depth.shape[1:], maps, vis, dtype) + (kept,)
