"""Test cases of the multi-view lifting, built on the CPU: a small analytic room (floor z = 0, back wall y = 4, one box in front of the
wall), depth maps ray-cast analytically in float64, points sampled on the surfaces plus a few behind the cameras, far outside every
frustum and at non-finite / 1e30 coordinates.

`build_case` drops every point for which ANY decision of ANY view (under every rule variant and depth format the tests use) lies within
`MARGIN` = 1e-3 (pixels or metres) of its boundary, so that an fp32 evaluation and the float64 restatement cannot decide differently,
and asserts that fewer than 20 % of the points go and that every outcome class still occurs."""
import functools

import numpy as np

import lift2d_ref as R

MARGIN = 1e-3
DEV32 = 8.979e-06        # largest deviation of the float32 restatement from the float64 one over VALUE_CASES (`python tests/lift2d_case.py`)
WALL_Y = 4.0
BOX = np.array([[1.2, 2.5, 0.0], [2.2, 3.3, 1.0]])                 # min, max corner
DEPTH_SCALE = 0.001
MAX_DEPTH = 60.0                                                   # beyond this a ray counts as a miss (uint16 millimetres end at 65.5 m)
RULES = [dict(border=0, tol_rel=0.0), dict(border=2, tol_rel=0.0), dict(border=0, tol_rel=0.25), dict(border=2, tol_rel=0.25)]


def look_at_pose(eye, yaw, pitch):
    """cam_to_world [4, 4] of a camera at `eye` (x right, y down, z forward) looking along `yaw` (0 = +y of the world, radians) and
    `pitch` radians below the horizon."""
    fwd = np.array([np.sin(yaw) * np.cos(pitch), np.cos(yaw) * np.cos(pitch), -np.sin(pitch)])
    right = np.array([np.cos(yaw), -np.sin(yaw), 0.0])
    down = np.cross(fwd, right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, down, fwd, eye
    return pose


def ray_cast(pose, intr, H, W):
    """Depth (camera z, float64 metres, 0 = nothing hit within MAX_DEPTH) of every pixel centre of one view."""
    fx, fy, cx, cy = intr
    vi, ui = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d_cam = np.stack([(ui - cx) / fx, (vi - cy) / fy, np.ones_like(ui)], axis=-1)   # z component 1: the ray parameter is the depth
    d = d_cam @ pose[:3, :3].T
    o = pose[:3, 3]
    best = np.full((H, W), np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -o[2] / d[..., 2]                                                        # floor
        best = np.where((t > 0) & np.isfinite(t), np.minimum(best, t), best)
        t = (WALL_Y - o[1]) / d[..., 1]                                              # back wall
        best = np.where((t > 0) & np.isfinite(t), np.minimum(best, t), best)
        ta, tb = (BOX[0] - o) / d, (BOX[1] - o) / d                                  # box: slabs
        tmin, tmax = np.nanmax(np.minimum(ta, tb), axis=-1), np.nanmin(np.maximum(ta, tb), axis=-1)
        hit = (tmax >= tmin) & (tmin > 0)
        best = np.where(hit, np.minimum(best, tmin), best)
    return np.where(best < MAX_DEPTH, best, 0.0)


def room_points(rng, n):
    """n points on the floor, the wall and the faces of the box (in about equal parts)."""
    k = rng.integers(0, 5, n)
    a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    lo, hi = BOX
    floor = np.stack([a * 4.0, b * 4.0, np.zeros(n)], 1)
    wall = np.stack([a * 4.0, np.full(n, WALL_Y), b * 2.5], 1)
    top = np.stack([lo[0] + a * (hi[0] - lo[0]), lo[1] + b * (hi[1] - lo[1]), np.full(n, hi[2])], 1)
    front = np.stack([lo[0] + a * (hi[0] - lo[0]), np.full(n, lo[1]), b * hi[2]], 1)
    side = np.stack([np.where(a < 0.5, lo[0], hi[0]), lo[1] + b * (hi[1] - lo[1]), rng.uniform(0, 1, n) * hi[2]], 1)
    return np.choose(k[:, None], [floor, wall, top, front, side])


def make_views(rng, V, H, W, n_bad_poses=0):
    """V random cameras inside the room: any yaw, 5 - 30 degrees below the horizon -> poses [V, 4, 4], intrinsics fp32 [V, 4],
    depth float64 [V, H, W] with some pixels zeroed.  The last `n_bad_poses` poses get a non-finite entry (their depth is unused)."""
    poses, intr, depth = [], [], []
    for j in range(V):
        eye = np.array([rng.uniform(0.4, 3.6), rng.uniform(0.2, 2.2), rng.uniform(1.0, 1.7)])
        yaw = rng.uniform(-np.pi, np.pi) if j % 4 else rng.uniform(-0.5, 0.5)      # a quarter of them face the wall and the box
        pose = look_at_pose(eye, yaw, rng.uniform(0.08, 0.5))
        f = rng.uniform(0.85, 1.25) * W
        k = np.array([f, f * rng.uniform(0.97, 1.03), (W - 1) / 2 + rng.uniform(-1, 1), (H - 1) / 2 + rng.uniform(-1, 1)], dtype=np.float32)
        d = ray_cast(pose, k.astype(np.float64), H, W)
        d[rng.uniform(size=d.shape) < 0.06] = 0.0                                  # sensor drop-outs
        poses.append(pose), intr.append(k), depth.append(d)
    poses = np.stack(poses)
    for j in range(n_bad_poses):
        poses[V - 1 - j, j % 3, 3] = np.nan if j % 2 == 0 else np.inf
    return poses, np.stack(intr), np.stack(depth)


def special_points():
    """Points no view may see: non-finite, huge, far outside every frustum."""
    return np.array([[np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [-np.inf, 0.0, np.nan], [1e30, 1e30, 1e30], [-1e30, 2.0, 1.0], [2.0, 3e30, 0.5],
                     [2.0, -500.0, 1.0], [900.0, 2.0, 1.0], [2.0, 2.0, 400.0], [2.0, 2.0, -300.0]], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def build_case(seed=10, n_points=1400, n_views=70, H=24, W=32, n_bad_poses=0):
    """-> dict(points fp32 [N, 3], poses float64 [V, 4, 4], intr fp32 [V, 4], depth_u16 [V, H, W], depth_f32 [V, H, W], w2c, kept,
    dropped = the share of sampled points the margin rule removed).  Shared by the tests: treat it as read-only."""
    rng = np.random.default_rng(seed)
    poses, intr, depth = make_views(rng, n_views, H, W, n_bad_poses)
    depth_u16 = np.round(depth / DEPTH_SCALE).astype(np.uint16)
    depth_f32 = (depth_u16.astype(np.float32) * np.float32(DEPTH_SCALE)).astype(np.float32)
    pts = np.concatenate([room_points(rng, n_points), special_points()]).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    w2c, kept = R.world_to_cam(poses)
    worst = np.full(len(pts), np.inf)
    for d, scale in ((depth_u16, DEPTH_SCALE), (depth_f32, None)):
        for tol_rel in (0.0, 0.25):
            _, m = R.outcomes(pts, w2c, intr[kept], d[kept], scale, tol_rel=tol_rel, margins=True)
            worst = np.minimum(worst, m.min(axis=1))
    keep = worst >= MARGIN
    dropped = 1.0 - keep.mean()
    assert dropped < 0.20, f"the margin rule drops {dropped:.1%} of the points: choose another seed"
    pts = np.ascontiguousarray(pts[keep])
    assert (~np.isfinite(pts)).any() and (np.abs(pts[np.isfinite(pts)]) >= 1e30).any(), "the special points must survive"
    out = R.outcomes(pts, w2c, intr[kept], depth_u16[kept], DEPTH_SCALE)
    for code, name in ((R.BEHIND, "behind camera"), (R.OUTSIDE, "outside image"), (R.NO_DEPTH, "zero depth"), (R.OCCLUDED, "occluded"),
                       (R.VISIBLE, "visible")):
        assert (out == code).any(), f"no pair is '{name}': choose another seed"
    assert ((out == R.VISIBLE).sum(axis=1) == 0).any(), "no point is visible in no view"
    for a in (pts, poses, intr, depth_u16, depth_f32, w2c, kept):
        a.setflags(write=False)
    return dict(points=pts, poses=poses, intr=intr, depth_u16=depth_u16, depth_f32=depth_f32, w2c=w2c, kept=kept, dropped=dropped, H=H, W=W)


def make_maps(seed, V, sizes, C, dtype):
    """One random channels-last map per scale: [V, Hf, Wf, C] in `dtype` (values the dtype holds exactly, |x| <= 2)."""
    rng = np.random.default_rng(seed)
    return [rng.uniform(-2, 2, (V, hf, wf, C)).astype(dtype) for hf, wf in sizes]


# (name, C, map dtype, [(Hf, Wf) per scale], output dtype name, number of views): the value cases of tests/test_gpu_lift2d.py.
# Between them: every lane-group width of the accumulate kernel (8, 16, 32, 64 lanes) and its channel chunks (C = 320 / 1024 in fp32),
# 1 x 1 maps (every tap clamped), maps coarser than the depth image (taps clamped at the border), one and three scales.
VALUE_CASES = [
    ("c64_f16_1x1", 64, np.float16, [(1, 1)], "float32", 70),
    ("c128_f16_7x9", 128, np.float16, [(7, 9)], "float32", 70),
    ("c256_f16_7x9", 256, np.float16, [(7, 9)], "float32", 70),
    ("c320_f16_15x20", 320, np.float16, [(15, 20)], "float32", 70),
    ("c320_f32_15x20", 320, np.float32, [(15, 20)], "float32", 70),
    ("c64_f32_3scales", 64, np.float32, [(15, 20), (7, 9), (1, 1)], "float32", 70),
    ("c256_f16_3scales_f16out", 256, np.float16, [(15, 20), (7, 9), (1, 1)], "float16", 70),
    ("c1024_f32_7x9", 1024, np.float32, [(7, 9)], "float32", 33),
]


@functools.lru_cache(maxsize=None)
def value_case(name):
    """-> dict(maps = list of arrays, vis bool [N, V], ref = float64 (out, means, count), dev32 = the largest deviation of the float32
    evaluation of the restatement from the float64 one, over the output and the per-scale means)."""
    _, C, dt, sizes, out_dtype, V = next(c for c in VALUE_CASES if c[0] == name)
    c = build_case()
    maps = make_maps(sum(map(ord, name)), V, sizes, C, dt)
    w2c, intr = c["w2c"][:V], c["intr"][:V]
    vis = R.outcomes(c["points"], w2c, intr, c["depth_u16"][:V], DEPTH_SCALE) == R.VISIBLE
    hw = (c["H"], c["W"])
    ref = R.lift(c["points"], w2c, intr, hw, maps, vis)
    f32 = R.lift(c["points"], w2c, intr, hw, maps, vis, dtype=np.float32)
    dev32 = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip([f32[0]] + f32[1], [ref[0]] + ref[1]))
    return dict(C=C, maps=maps, vis=vis, ref=ref, dev32=dev32, out_dtype=out_dtype, V=V)


if __name__ == "__main__":                     # the figures of profiles/lift_2d.md, "tolerance"
    worst = 0.0
    for case in VALUE_CASES:
        d = value_case(case[0])["dev32"]
        worst = max(worst, d)
        print(f"{case[0]:28s} float32 restatement vs float64: {d:.3e}")
    print(f"largest {worst:.3e}; bound of the value comparisons = 4 x that = {4 * worst:.3e}")
