"""csrc/fuse_views.hip + segdino3d_amd/fuse_views.py against the numpy restatement tests/fuse_views_ref.py (the reference has no
counterpart) on the synthetic room and the hand-built scenes of tests/fuse_views_case.py.

Bounds.  None: `N`, the keys, `obs`, the counters and the BITS of `points` must EQUAL the float32 restatement.  Every decision of the
rule is an integer one or a single rounded fp32 operation, the per-cell state is integer sums, and every emitted float is one
rounding of a quotient of identical integers.  The composition test's one exception is explained where it stands."""
import numpy as np
import pytest
import torch

import fuse_views_case as K
import fuse_views_ref as R

pytestmark = pytest.mark.gpu

SMALL = 1 << 18                      # slots: three times the room's cells, and quicker to empty and sort than the default 2^21


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _t(a, d):
    return torch.from_numpy(np.array(a)).to(d)                   # a copy: the shared cases are read-only


def _views(c, d, kind="u16", idx=None):
    from segdino3d_amd import lift2d
    idx = slice(None) if idx is None else idx
    depth = (c["depth_u16"] if kind == "u16" else c["depth_f32"])[idx]
    return lift2d.Views(_t(depth, d), _t(c["intr"][idx], d), c["poses"][idx], c.get("scale", K.DEPTH_SCALE) if kind == "u16" else None)


def _ref(c, kind="u16", **kw):
    depth, scale = (c["depth_u16"], c.get("scale", K.DEPTH_SCALE)) if kind == "u16" else (c["depth_f32"], None)
    return R.fuse(depth, scale, c["intr"], c["poses"], c["colors"], **kw)


def _fuse(c, d, kind="u16", voxel=0.02, capacity=SMALL, **rule):
    from segdino3d_amd import fuse_views as fuse
    return fuse.fuse_views(_views(c, d, kind), _t(c["colors"], d), voxel=voxel, capacity=capacity, return_obs=True, return_info=True,
                           return_keys=True, **rule)


def _equal(got, want, what):
    points, obs, info, keys = got
    assert points.dtype == torch.float32 and obs.dtype == torch.int32 and keys.dtype == torch.int64 and points.is_contiguous(), what
    assert tuple(points.shape) == (len(want["obs"]), 6) and tuple(obs.shape) == (len(want["obs"]),), (what, points.shape, len(want["obs"]))
    assert np.array_equal(keys.cpu().numpy().view(np.uint64), want["keys"]), what
    assert np.array_equal(obs.cpu().numpy(), want["obs"]), what
    assert np.array_equal(points.cpu().numpy().view(np.uint32), want["points"].view(np.uint32)), what
    assert (info.n, info.cells, info.pixels_used, info.out_of_range, info.overflow) == \
        (len(want["obs"]), want["cells"], want["pixels_used"], want["out_of_range"], 0), (what, info)


def _check(c, d, kind="u16", what="", capacity=SMALL, **kw):
    want = _ref(c, kind, **kw)
    _equal(_fuse(c, d, kind, capacity=capacity, **kw), want, (what, kind, kw))
    return want


def _with(c, **over):
    return {**c, **over}


# ---------------------------------------------------------------------------------------------- nothing to fuse
def test_no_views_one_pixel_and_no_depth():
    from segdino3d_amd import fuse_views as fuse, lift2d
    d = dev()
    none = lift2d.Views(torch.zeros(0, 4, 6, dtype=torch.uint16).to(d), np.zeros((0, 4), np.float32), np.zeros((0, 4, 4)), K.DEPTH_SCALE)
    points, obs, info = fuse.fuse_views(none, torch.zeros(0, 4, 6, 3, dtype=torch.uint8, device=d), return_obs=True, return_info=True)
    assert tuple(points.shape) == (0, 6) and points.is_cuda and tuple(obs.shape) == (0,) and info == fuse.FuseInfo(0, 0, 0, 0, 0)
    one = K.wall(1, 1, 1.0)
    want = _check(one, d, min_obs=1, what="1 x 1")
    assert len(want["obs"]) == 1 and want["points"][0, :3].tolist() == [1.0, 0.0, 0.0]
    assert _check(one, d, what="1 x 1, min_obs 2")["points"].shape == (0, 6)
    wall = K.wall(9, 11, 1.0)
    dark = _with(wall, depth_u16=np.zeros_like(wall["depth_u16"]), depth_f32=np.zeros_like(wall["depth_f32"]))
    for kind in ("u16", "f32"):
        assert _check(dark, d, kind, min_obs=1, what="all depth 0")["pixels_used"] == 0


# ---------------------------------------------------------------------------------------------- tile edges and the halo of the edge test
@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("hw", [(5, 7), (9, 63), (9, 64), (9, 65), (17, 33)])
def test_small_and_odd_images(hw, kind):
    d = dev()
    c = K.noisy(hw[0], hw[1], V=2, seed=hw[1], color_hw=(hw[0] + 2, hw[1] - 3))
    want = _check(c, d, kind, min_obs=1, what=hw)
    assert 0 < want["pixels_used"] < 2 * hw[0] * hw[1]                               # some pixels pass, holes and steps drop others
    assert _check(c, d, kind, min_obs=1, edge_rel=None, what=hw)["pixels_used"] > want["pixels_used"]


def test_depth_straddles_near_and_far_exactly():
    d = dev()
    raw = np.array([[99, 100, 101, 5999], [6000, 6001, 199, 200], [201, 11999, 12000, 12001]], np.uint16)[None]
    for scale, near, far in ((0.001, 0.1, 6.0), (0.0005, 0.1, 6.0), (0.0005, 0.05, 3.0)):
        c = _with(K.wall(3, 4, 1.0), depth_u16=raw, depth_f32=raw.astype(np.float32) * np.float32(scale), scale=scale)
        for kind in ("u16", "f32"):
            want = _check(c, d, kind, min_obs=1, edge_rel=None, near=near, far=far, what=(scale, near, far))
            dm = raw[0].astype(np.float32) * np.float32(scale)
            assert want["pixels_used"] == int(((dm >= np.float32(near)) & (dm <= np.float32(far))).sum()) and 0 < want["pixels_used"] < 12


# ---------------------------------------------------------------------------------------------- how many pixels share a cell
def test_wall_many_pixels_per_cell():
    """0.5 m in front of a 48 x 64 camera with 0.25 m cells: hundreds of pixels of one tile share a cell; on-chip combining decides."""
    d = dev()
    c = K.wall(48, 64, 0.5, color_hw=(48, 64))
    want = _check(c, d, voxel=0.25, what="wall 0.5 m")
    assert want["obs"].max() >= 300 and len(want["obs"]) <= 16
    _check(c, d, "f32", what="wall 0.5 m, 2 cm")


def test_wall_one_pixel_per_cell():
    d = dev()
    c = K.wall(48, 64, 5.0)
    want = _check(c, d, voxel=2.0 ** -6, min_obs=1, what="wall 5 m")
    assert want["obs"].max() == 1 and len(want["obs"]) == 48 * 64


def test_wall_on_a_cell_boundary_at_a_negative_coordinate():
    d = dev()
    c = K.wall(16, 40, 0.5, plane_x=-1.0)
    c = _with(c, depth_f32=np.full((1, 16, 40), 0.5, np.float32))
    want = _check(c, d, "f32", voxel=2.0 ** -5, min_obs=1, what="boundary")
    assert (want["points"][:, 0] == -1.0).all()                                       # w_x = 0.5 - 1.5 exactly: the cell that begins at -1
    assert ((want["keys"] >> np.uint64(42)) == np.uint64((1 << 20) - 32)).all()
    assert (want["points"][:, 1] < 0).any() and (want["points"][:, 2] < 0).any()


def test_one_cell_from_eight_views_and_several_tiles():
    d = dev()
    c = K.wall(48, 64, 0.5, V=8)
    want = _check(c, d, voxel=1.0, what="8 views, 1 m cells")
    assert len(want["obs"]) <= 8 and want["obs"].max() > 8 * 48 * 64 // 8            # a cell sums over all views and over many tiles of each


# ---------------------------------------------------------------------------------------------- the room
@pytest.mark.parametrize("color_hw", [(60, 80), (97, 131)])
def test_room(color_hw):
    d = dev()
    c = K.room_case(color_hw)
    want = _check(c, d, capacity=1 << 21, what=("room", color_hw))
    assert len(want["obs"]) > 3000 and want["obs"].max() > 8
    _check(c, d, "f32", what=("room f32", color_hw))


@pytest.mark.parametrize("kw", [dict(stride=2), dict(stride=3, min_obs=1), dict(min_obs=1), dict(min_obs=3), dict(edge_rel=None),
                                dict(voxel=0.05, near=0.8, far=2.5, edge_abs=0.0, edge_rel=0.01)])
def test_room_rule_parameters(kw):
    d = dev()
    assert len(_check(K.room_case(), d, what="room", **kw)["obs"]) > 500


def test_nan_pose_is_dropped():
    from segdino3d_amd import fuse_views as fuse
    d = dev()
    c = K.room_case()
    poses = c["poses"].copy()
    poses[3, 1, 2] = np.nan
    bad = _with(c, poses=poses)
    want = _check(bad, d, what="NaN pose")
    keep = np.array([0, 1, 2, 4, 5, 6, 7])
    # colours per KEPT view give the same cloud as colours per given view
    views = _views(bad, d)
    assert len(views) == 7 and views.n_given == 8
    again = fuse.fuse_views(views, _t(c["colors"][keep], d), capacity=SMALL)
    assert np.array_equal(again.cpu().numpy().view(np.uint32), want["points"].view(np.uint32))


# ---------------------------------------------------------------------------------------------- out of range
def test_points_beyond_the_world_are_counted_not_written():
    d = dev()
    c = K.wall(9, 20, 1.0, V=2)
    poses = c["poses"].copy()
    poses[1, 0, 3] = 2.0 ** 14                                                         # view 1 lands at x >= 2^14 m
    want = _check(_with(c, poses=poses), d, min_obs=1, what="2^14")
    assert want["out_of_range"] == 9 * 20 and want["pixels_used"] == 9 * 20
    poses[0, 1, 3] = -3.0e38                                                           # and view 0 at the end of fp32
    want = _check(_with(c, poses=poses), d, min_obs=1, what="inf")
    assert want["out_of_range"] == 2 * 9 * 20 and want["cells"] == 0 and len(want["obs"]) == 0


def test_cells_beyond_21_bits_through_a_small_voxel():
    """|c| >= 2^20 needs a voxel below 2^-6, which PointCloudFuser refuses: through the operator layer."""
    from segdino3d_amd import ops
    d = dev()
    c = K.wall(9, 20, 1.0, V=2)
    poses = c["poses"].copy()
    poses[0, 0, 3], poses[1, 0, 3] = 1100.0, -1100.0                                   # 1 mm cells: |c| > 2^20; view 1 at the negative end
    poses = np.concatenate([poses, c["poses"][:1]])                                    # and one view inside
    cc = {k: np.concatenate([c[k], c[k][:1]]) for k in ("depth_u16", "intr", "colors")}
    c2w, _ = R.cam_to_world(poses)
    want = R.fuse_kept(cc["depth_u16"], K.DEPTH_SCALE, cc["intr"], c2w, cc["colors"], voxel=2.0 ** -10, min_obs=1)
    assert want["out_of_range"] == 2 * 9 * 20 and want["pixels_used"] == 9 * 20
    ws = ops.fuse_workspace(SMALL, d)
    ops.fuse_accumulate(_t(cc["depth_u16"], d), K.DEPTH_SCALE, _t(cc["intr"], d), _t(c2w, d), _t(cc["colors"], d), ws, SMALL, 2.0 ** 10)
    points, obs, keys, info = ops.fuse_emit(ws, SMALL, 1, 3 * 9 * 20, want_keys=True)
    info = info.tolist()
    assert info == [len(want["obs"]), want["cells"], want["pixels_used"], want["out_of_range"], 0]
    n = info[0]
    assert np.array_equal(keys[:n].cpu().numpy().view(np.uint64), want["keys"]) and np.array_equal(obs[:n].cpu().numpy(), want["obs"])
    assert np.array_equal(points[:n].cpu().numpy().view(np.uint32), want["points"].view(np.uint32))


# ---------------------------------------------------------------------------------------------- a function of the set of observations
def test_cut_order_and_stream_do_not_change_a_bit():
    from segdino3d_amd import fuse_views as fuse, ops
    d = dev()
    c = K.room_case()
    base, base_obs, _, _ = _fuse(c, d)
    colors = _t(c["colors"], d)
    for order in (list(range(8)), list(range(7, -1, -1)), [5, 2, 7, 0, 3, 6, 1, 4]):
        fuser = fuse.PointCloudFuser(capacity=SMALL)
        for i in order:                                                               # one add per view
            fuser.add(_views(c, d, idx=slice(i, i + 1)), colors[i:i + 1])
        points, obs = fuser.result(return_obs=True)
        assert torch.equal(points, base) and torch.equal(obs, base_obs), order
    fuser = fuse.PointCloudFuser(capacity=SMALL)
    rev = np.arange(7, -1, -1)
    fuser.add(_views(c, d, idx=rev[:3]), colors[torch.from_numpy(rev[:3].copy()).to(d)])
    half = fuser.result()                                                             # a result in between does not disturb the state
    fuser.add(_views(c, d, idx=rev[3:]), colors[torch.from_numpy(rev[3:].copy()).to(d)])
    points, obs = fuser.result(return_obs=True)
    assert torch.equal(points, base) and torch.equal(obs, base_obs) and half.shape[0] < base.shape[0]
    assert torch.equal(fuser.result(), base)                                          # twice
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with ops.use_stream(side):
        got = _fuse(c, d)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(got[0], base) and torch.equal(got[1], base_obs)


def test_overflow_is_an_error_not_a_thinner_cloud():
    from segdino3d_amd import fuse_views as fuse
    d = dev()
    c = K.room_case()
    fuser = fuse.PointCloudFuser(capacity=64)
    fuser.add(_views(c, d), _t(c["colors"], d))
    with pytest.raises(RuntimeError, match=r"overflow = \d+ .* capacity = 64"):
        fuser.result()
    assert fuser.info.overflow > 0 and fuser.info.cells <= 64 and fuser.info.pixels_used + fuser.info.overflow == _ref(c)["pixels_used"]
    _equal(_fuse(c, d, capacity=1 << 21), _ref(c), "after an overflow")


# ---------------------------------------------------------------------------------------------- the chain
def test_fused_points_feed_superpoints_and_lifting():
    """Views -> points -> superpoints and 2D features.  Labels must EQUAL tests/point_superpoints_ref.py on the fused xyz.  Visibility
    counts must equal tests/lift2d_ref.py on every point whose closest decision is at least `lift2d_case.MARGIN` (1e-3 px / m) from
    its boundary in the float64 restatement - the rule by which tests/lift2d_case.py chooses its points, since an fp32 evaluation may
    decide a closer call differently; fused points are not chosen, so the test applies the rule itself and requires that it keeps
    most points."""
    import lift2d_case as K2
    import lift2d_ref as R2
    import point_superpoints_ref as P
    from segdino3d_amd import fuse_views as fuse, lift2d, superpoints
    d = dev()
    c = K.room_case()
    views = _views(c, d)
    points = fuse.fuse_views(views, _t(c["colors"], d), voxel=0.1, capacity=SMALL)          # 10 cm: a few thousand points keep the numpy side quick
    want = _ref(c, voxel=0.1)
    assert np.array_equal(points.cpu().numpy().view(np.uint32), want["points"].view(np.uint32))
    xyz = np.ascontiguousarray(want["points"][:, :3])
    labels, info = superpoints.point_superpoints(points[:, :3].contiguous(), radius=0.25, return_info=True)
    ref = P.point_superpoints(xyz, radius=0.25)
    assert np.array_equal(labels.cpu().numpy(), ref.labels) and info.count == ref.count and ref.count > 1
    maps = _t(np.random.default_rng(0).standard_normal((8, 15, 20, 64)).astype(np.float16), d)
    feats, counts = lift2d.lift_point_features(points, views, maps, return_counts=True)
    w2c, _ = R2.world_to_cam(c["poses"])
    out, margin = R2.outcomes(xyz, w2c, c["intr"], c["depth_u16"], K.DEPTH_SCALE, margins=True)
    sure = margin.min(axis=1) >= K2.MARGIN
    assert sure.mean() > 0.8, sure.mean()
    ref_count = (out == R2.VISIBLE).sum(axis=1)
    assert np.array_equal(counts.cpu().numpy()[sure], ref_count[sure]) and ref_count[sure].mean() >= 1     # the views that made a point see it
    assert tuple(feats.shape) == (len(xyz), 64) and bool(torch.isfinite(feats).all())


# ---------------------------------------------------------------------------------------------- arguments
def test_device_argument_errors():
    from segdino3d_amd import fuse_views as fuse, ops
    d = dev()
    c = K.wall(9, 20, 1.0)
    views, colors = _views(c, d), _t(c["colors"], d)
    fuser = fuse.PointCloudFuser(capacity=SMALL)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fuser.add(views, colors.cpu())
    with pytest.raises(TypeError, match="uint8"):
        fuser.add(views, colors.float())
    with pytest.raises(ValueError, match="one colour image per view"):
        fuser.add(views, colors.repeat(2, 1, 1, 1))
    with pytest.raises(ValueError, match=r"\[V, Hc, Wc, 3\]"):
        fuser.add(views, colors[..., :2])
    with pytest.raises(TypeError, match="lift2d.Views"):
        fuser.add(c["depth_u16"], colors)
    ws = ops.fuse_workspace(SMALL, d)
    with pytest.raises(RuntimeError, match="workspace too small"):
        ops.fuse_emit(ws[:4096], SMALL, 1, 16)
    with pytest.raises(ValueError, match="capacity"):
        ops.fuse_workspace(1000, d)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fuse_workspace(SMALL, "cpu")
    assert tuple(fuser.result().shape) == (0, 6)                                      # nothing was added by the refused calls
