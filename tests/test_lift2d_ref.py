"""Pins the float64 restatement of the multi-view lifting (tests/lift2d_ref.py) - the only thing the lifting kernels can be compared
with, since the reference has no code that makes `points_2dfeats` - and the host-side checks of `lift2d.Views`.  No GPU."""
import numpy as np
import pytest
import torch

import lift2d_case as K
import lift2d_ref as R


def _front_camera(H=24, W=32, f=24.0):
    """One camera at (2, 0.5, 1.2) looking straight at the wall: world x -> u, world -z -> v, world y -> depth."""
    pose = K.look_at_pose(np.array([2.0, 0.5, 1.2]), 0.0, 0.0)
    intr = np.array([[f, f, (W - 1) / 2, (H - 1) / 2]], dtype=np.float32)
    return pose[None], intr


def test_case_builder_keeps_every_outcome_and_most_points():
    c = K.build_case()
    assert c["dropped"] < 0.20 and len(c["points"]) >= 1000
    out, m = R.outcomes(c["points"], c["w2c"], c["intr"], c["depth_u16"], K.DEPTH_SCALE, margins=True)
    assert m.min() >= K.MARGIN
    assert set(np.unique(out)) == {R.BEHIND, R.OUTSIDE, R.NO_DEPTH, R.OCCLUDED, R.VISIBLE}
    # float32 evaluation decides every pair as float64 does: what the margin is for
    for d, s in ((c["depth_u16"], K.DEPTH_SCALE), (c["depth_f32"], None)):
        for rule in K.RULES:
            a = R.outcomes(c["points"], c["w2c"], c["intr"], d, s, **rule)
            b = R.outcomes(c["points"], c["w2c"], c["intr"], d, s, dtype=np.float32, **rule)
            assert np.array_equal(a, b)
    bad = ~np.isfinite(c["points"]).all(axis=1) | (np.abs(c["points"]) >= 1e30).any(axis=1)
    assert bad.sum() >= 6 and not (out[bad] == R.VISIBLE).any()


def test_sampling_equals_grid_sample_border():
    rng = np.random.default_rng(0)
    Hf, Wf, C, M = 7, 9, 5, 400
    fmap = rng.normal(size=(Hf, Wf, C))
    xf, yf = rng.uniform(-1.0, Wf, M), rng.uniform(-1.0, Hf, M)                     # includes taps on and beyond the border
    got = R.sample(fmap, xf, yf)
    gx, gy = (2 * xf + 1) / Wf - 1, (2 * yf + 1) / Hf - 1                             # align_corners=False pixel -> normalised
    grid = torch.from_numpy(np.stack([gx, gy], -1)).reshape(1, 1, M, 2)
    want = torch.nn.functional.grid_sample(torch.from_numpy(fmap).permute(2, 0, 1)[None], grid, mode="bilinear", padding_mode="border",
                                           align_corners=False)[0, :, 0].T.numpy()
    assert np.abs(got - want).max() < 1e-12


def test_linear_field_is_reproduced_at_interior_points():
    """Map texel (i, j) holds a*X + b*Y + c at its centre in depth-image pixels, X = (j + 0.5) Wd / Wf - 0.5: bilinear interpolation
    of a linear field is exact, so a visible interior point returns a*u + b*v + c."""
    H, W, Hf, Wf = 24, 32, 12, 16
    poses, intr = _front_camera(H, W)
    w2c, _ = R.world_to_cam(poses)
    jj, ii = np.meshgrid(np.arange(Wf), np.arange(Hf))
    X, Y = (jj + 0.5) * W / Wf - 0.5, (ii + 0.5) * H / Hf - 0.5
    coef = np.array([[0.25, -0.5, 1.0], [-1.0, 0.125, 3.0]])
    fmap = np.stack([a * X + b * Y + c for a, b, c in coef], -1)[None]                # [1, Hf, Wf, 2]
    fmap = np.concatenate([fmap] * 32, -1)                                            # 64 channels
    rng = np.random.default_rng(1)
    pts = np.stack([rng.uniform(1.2, 2.8, 200), np.full(200, K.WALL_Y), rng.uniform(0.7, 1.7, 200)], 1).astype(np.float32)
    depth = np.full((1, H, W), np.float32(K.WALL_Y - 0.5))                            # the wall, seen head-on: constant depth
    z, u, v = R.project(pts, w2c, intr)
    inner = (u[:, 0] > 1.5) & (u[:, 0] < W - 2.5) & (v[:, 0] > 1.5) & (v[:, 0] < H - 2.5)
    assert inner.sum() > 50
    out, means, count, _ = R.lift_point_features(pts, poses, intr, depth, [fmap])
    assert (count[inner] == 1).all()
    for ch, (a, b, c) in enumerate(coef):
        assert np.abs(out[inner, ch] - (a * u[inner, 0] + b * v[inner, 0] + c)).max() < 1e-9


def test_round_half_up():
    """u = k + 0.5 reads pixel k + 1 for odd AND even k (half rounds up, not to even)."""
    H, W = 4, 8
    w2c = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None].astype(np.float32)
    intr = np.array([[2.0, 2.0, 0.0, 0.0]], dtype=np.float32)
    depth = np.zeros((1, H, W), dtype=np.float32)
    depth[0, 1, 2] = depth[0, 1, 3] = 1.0                                              # only pixels (row 1, cols 2 and 3) are valid
    # z = 1: u = 2 x, v = 2 y.  u = 1.5 -> pixel 2, u = 2.5 -> pixel 3, u = 0.5 -> pixel 1 (invalid), u = 3.5 -> pixel 4 (invalid)
    pts = np.array([[0.75, 0.5, 1.0], [1.25, 0.5, 1.0], [0.25, 0.5, 1.0], [1.75, 0.5, 1.0], [0.75, 0.25, 1.0], [0.75, 0.75, 1.0]], dtype=np.float32)
    out = R.outcomes(pts, w2c, intr, depth)
    assert out[:, 0].tolist() == [R.VISIBLE, R.VISIBLE, R.NO_DEPTH, R.NO_DEPTH, R.VISIBLE, R.NO_DEPTH]   # v = 0.5 -> row 1, v = 1.5 -> row 2
    # the image bounds follow the rounded pixel: u = -0.5 -> pixel 0 is inside, u just below is outside
    edge = np.array([[-0.25, 0.5, 1.0], [-0.2501, 0.5, 1.0], [3.7499, 0.5, 1.0], [3.75, 0.5, 1.0]], dtype=np.float32)
    assert R.outcomes(edge, w2c, intr, depth)[:, 0].tolist() == [R.NO_DEPTH, R.OUTSIDE, R.NO_DEPTH, R.OUTSIDE]
    assert R.outcomes(edge, w2c, intr, depth, border=1)[:, 0].tolist() == [R.OUTSIDE] * 4


def test_box_occludes_the_wall_behind_it():
    H, W = 24, 32
    poses, intr = _front_camera(H, W)
    depth = K.ray_cast(poses[0], intr[0].astype(np.float64), H, W).astype(np.float32)[None]
    w2c, _ = R.world_to_cam(poses)
    lo, hi = K.BOX
    behind = np.array([[1.7, K.WALL_Y, 0.5], [1.5, K.WALL_Y, 0.8]], dtype=np.float32)       # wall points in the box's shadow
    free = np.array([[0.5, K.WALL_Y, 1.2], [3.2, K.WALL_Y, 1.5]], dtype=np.float32)         # wall points beside it
    front = np.array([[1.7, lo[1], 0.5]], dtype=np.float32)                                 # on the box's front face
    out = R.outcomes(np.concatenate([behind, free, front]), w2c, intr, depth, tol_abs=0.2)  # 0.2: half a coarse pixel of slant
    assert out[:, 0].tolist() == [R.OCCLUDED, R.OCCLUDED, R.VISIBLE, R.VISIBLE, R.VISIBLE]
    # tol_rel widens the test with the depth READ (d = 2 m at the box's front, the wall lies 1.5 m behind it): 0.05 + 0.8 * 2 >= 1.5
    assert R.outcomes(behind, w2c, intr, depth, tol_rel=0.1)[:, 0].tolist() == [R.OCCLUDED] * 2
    assert R.outcomes(behind, w2c, intr, depth, tol_rel=0.8)[:, 0].tolist() == [R.VISIBLE] * 2


def test_invalid_poses_are_dropped():
    c = K.build_case(n_bad_poses=3)
    w2c, kept = R.world_to_cam(c["poses"])
    assert kept.tolist() == list(range(67)) and w2c.shape == (67, 3, 4) and w2c.dtype == np.float32
    full = np.concatenate([w2c[0].astype(np.float64), [[0, 0, 0, 1]]]) @ c["poses"][0]
    assert np.abs(full - np.eye(4)).max() < 1e-6
    from segdino3d_amd import lift2d
    w2c_b, kept_b = lift2d.world_to_cam(torch.from_numpy(c["poses"].copy()))
    assert np.array_equal(kept, kept_b) and w2c.tobytes() == w2c_b.tobytes()
    assert len(R.world_to_cam(np.full((2, 4, 4), np.nan))[1]) == 0


def test_pack_bits():
    vis = np.zeros((3, 70), dtype=bool)
    vis[0, [0, 31, 32, 69]] = True
    vis[2, :] = True
    bits = R.pack_bits(vis).view(np.uint32)
    assert bits.shape == (3, 3) and bits[0].tolist() == [0x80000001, 1, 1 << 5] and bits[1].tolist() == [0, 0, 0]
    assert bits[2].tolist() == [0xFFFFFFFF, 0xFFFFFFFF, (1 << 6) - 1]


def test_views_validation_errors():
    """`Views` checks dtypes, shapes and the poses before it touches the device or the library."""
    from segdino3d_amd import lift2d
    V, H, W = 3, 4, 6
    depth16, depth32 = torch.zeros(V, H, W, dtype=torch.uint16), torch.zeros(V, H, W)
    intr, poses = torch.ones(V, 4), np.stack([np.eye(4)] * V)
    with pytest.raises(ValueError, match="depth_scale"):
        lift2d.Views(depth16, intr, poses)
    with pytest.raises(ValueError, match="depth_scale"):
        lift2d.Views(depth32, intr, poses, depth_scale=0.001)
    with pytest.raises(TypeError, match="uint16 or fp32"):
        lift2d.Views(depth32.double(), intr, poses)
    with pytest.raises(ValueError, match=r"\[V, Hd, Wd\]"):
        lift2d.Views(depth32[0], intr, poses)
    with pytest.raises(ValueError, match=r"\[V, 4, 4\]"):
        lift2d.Views(depth32, intr, poses[:, :3])
    with pytest.raises(ValueError, match="poses"):
        lift2d.Views(depth32, intr, poses[:2])
    with pytest.raises(ValueError, match="intrinsics"):
        lift2d.Views(depth32, torch.ones(V, 3), poses)
    with pytest.raises(ValueError, match="intrinsics"):
        lift2d.Views(depth32, intr.double(), poses)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lift2d.Views(depth32, intr, poses)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lift2d.PointFeatureAccumulator(torch.zeros(5, 3), 64)
    with pytest.raises(TypeError, match="unknown visibility parameter"):
        lift2d.PointFeatureAccumulator(torch.zeros(5, 3), 64, tolerance=1.0)


def test_recorded_float32_deviation_is_the_measured_one():
    """The value tolerance of tests/test_gpu_lift2d.py is 4 x `DEV32`: the figure recorded there is what the restatement gives."""
    worst = max(K.value_case(case[0])["dev32"] for case in K.VALUE_CASES)
    assert abs(worst - K.DEV32) <= 1e-9, worst
