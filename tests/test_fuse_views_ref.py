"""The numpy restatement of the fusion rule (tests/fuse_views_ref.py) against cases small enough to write out by hand, and its own
invariances: what keeps the yardstick of tests/test_gpu_fuse_views.py honest.  No GPU."""
import numpy as np

import fuse_views_case as K
import fuse_views_ref as R

OFF = 1 << R.CELL_BITS


def key(cx, cy, cz):
    return np.uint64(((cx + OFF) << 42) | ((cy + OFF) << 21) | (cz + OFF))


def identity_view(depth, colors=None, intr=(1.0, 1.0, 0.0, 0.0)):
    depth = np.asarray(depth, dtype=np.float32)[None]
    if colors is None:
        colors = np.zeros(depth.shape + (3,), np.uint8)
    return depth, np.array([intr], np.float32), np.eye(4)[None], np.asarray(colors, np.uint8).reshape((1,) + np.shape(colors)[-3:])


def test_hand_computed_case():
    """fx = fy = 1, cx = cy = 0, identity pose: pixel (vi, ui) of depth d is the point (ui d, vi d, d).  voxel = 2."""
    colors = np.zeros((2, 3, 3), np.uint8)
    colors[..., 0] = 10 * np.arange(6).reshape(2, 3)
    colors[..., 1] = 255
    depth, intr, poses, col = identity_view([[1.0, 1.0, 0.0], [0.25, 1.0, 2.0]], colors)
    out = R.fuse(depth, None, intr, poses, col, voxel=2.0, edge_rel=None, min_obs=1)
    # (0,0,1), (1,0,1), (0,.25,.25), (1,1,1) share cell (0,0,0); (4,2,2) is alone in cell (2,1,1); the pixel of depth 0 is invalid
    assert out["keys"].tolist() == [key(0, 0, 0), key(2, 1, 1)]
    assert out["obs"].tolist() == [4, 1] and out["cells"] == 2 and out["pixels_used"] == 5 and out["out_of_range"] == 0
    assert out["points"].dtype == np.float32
    assert out["points"].tolist() == [[0.5, 0.3125, 0.8125, 20.0, 255.0, 0.0], [4.0, 2.0, 2.0, 50.0, 255.0, 0.0]]
    assert R.fuse(depth, None, intr, poses, col, voxel=2.0, edge_rel=None, min_obs=2)["obs"].tolist() == [4]
    assert R.fuse(depth, None, intr, poses, col, voxel=2.0, edge_rel=None, min_obs=5)["points"].shape == (0, 6)
    # the edge test: every pixel has a neighbour that is a hole or a jump
    assert R.fuse(depth, None, intr, poses, col, voxel=2.0, min_obs=1)["points"].shape == (0, 6)
    # uint16 depth with a scale gives the same cloud where the product is exact
    d16 = np.array([[[4, 4, 0], [1, 4, 8]]], np.uint16)
    again = R.fuse(d16, 0.25, intr, poses, col, voxel=2.0, edge_rel=None, min_obs=1)
    assert np.array_equal(again["points"], out["points"]) and np.array_equal(again["keys"], out["keys"])


def test_near_far_and_nan_depth():
    depth, intr, poses, col = identity_view([[0.1, 6.0, np.nan, -1.0, np.inf, 6.0000005, 0.099999994]])
    obs = R.observations(depth, None, intr, R.cam_to_world(poses)[0], col, edge_rel=None)
    assert sorted(obs["ui"].tolist()) == [0, 1]                       # near and far themselves are inside; a NaN fails everything


def test_edge_rule_by_hand():
    # a step of 3 cm at 1 m is within 0.02 + 0.02 * d; a step of 5 cm is a jump for both of its sides; a hole drops its neighbours
    depth, intr, poses, col = identity_view([[1.0, 1.03, 1.06, 1.11, 1.11, 0.0, 1.11, 1.11]])
    ok = R.valid_pixels(depth[0], 0.1, 6.0, 0.02, 0.02)
    assert ok[0].tolist() == [True, True, False, False, False, False, False, True]
    assert R.valid_pixels(depth[0], 0.1, 6.0, 0.02, None)[0].tolist() == [True, True, True, True, True, False, True, True]
    # the neighbours count whatever the stride: pixel 4 is dropped although pixel 5 does not take part
    obs = R.observations(depth, None, intr, R.cam_to_world(poses)[0], col, stride=2)
    assert obs["ui"].tolist() == [0]


def test_negative_coordinates_take_the_floor_cell():
    # cx = 2: pixel 0 is the point (-2 d, 0, d) = (-0.75, 0, 0.375); voxel 0.5 -> floor gives cell -2, truncation would give -1
    depth, intr, poses, col = identity_view([[0.375]], intr=(1.0, 1.0, 2.0, 0.0))
    out = R.fuse(depth, None, intr, poses, col, voxel=0.5, edge_rel=None, min_obs=1)
    assert out["keys"].tolist() == [key(-2, 0, 0)] and out["points"][0, :3].tolist() == [-0.75, 0.0, 0.375]
    # exactly on a boundary: -1.0 belongs to the cell that begins there
    depth, intr, poses, col = identity_view([[0.5]], intr=(1.0, 1.0, 2.0, 0.0))
    assert R.fuse(depth, None, intr, poses, col, voxel=0.5, edge_rel=None, min_obs=1)["keys"].tolist() == [key(-2, 0, 1)]


def test_out_of_range_is_counted():
    depth, intr, poses, col = identity_view([[1.0, 1.0]])
    poses = poses.copy()
    poses[0, 0, 3] = 2.0 ** 14                                                         # |w| < 2^14 fails
    out = R.fuse(depth, None, intr, poses, col, edge_rel=None, min_obs=1)
    assert out["points"].shape == (0, 6) and out["out_of_range"] == 2 and out["pixels_used"] == 0
    poses[0, 0, 3] = 1100.0                                                            # inside the world, outside 21 bits of 1 mm cells
    out = R.fuse(depth, None, intr, poses, col, voxel=2.0 ** -10, edge_rel=None, min_obs=1)
    assert out["points"].shape == (0, 6) and out["out_of_range"] == 2
    poses[0, 0, 3] = 1000.0
    assert R.fuse(depth, None, intr, poses, col, voxel=2.0 ** -10, edge_rel=None, min_obs=1)["obs"].tolist() == [1, 1]


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("points", "obs", "keys")) and \
        (a["cells"], a["pixels_used"], a["out_of_range"]) == (b["cells"], b["pixels_used"], b["out_of_range"])


def test_set_invariance():
    c = K.room_case()
    c2w, kept = R.cam_to_world(c["poses"])
    args = lambda idx: (c["depth_u16"][idx], K.DEPTH_SCALE, c["intr"][idx], c2w[idx], c["colors"][idx])   # noqa: E731
    whole = R.accumulate(R.observations(*args(np.arange(8))))
    assert len(whole.keys) > 3000 and whole.n.max() > 8
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    two = R.merge(R.accumulate(R.observations(*args(perm[:3]))), R.accumulate(R.observations(*args(perm[3:]))))
    assert _same(R.emit(whole), R.emit(two)) and _same(R.emit(whole), R.emit(R.accumulate(R.observations(*args(perm)))))
    assert np.array_equal(whole.S, two.S) and np.array_equal(whole.C, two.C)


def test_stride_min_obs_nan_pose_and_odd_colour_size():
    c = K.room_case((97, 131))
    base = R.fuse(c["depth_u16"], K.DEPTH_SCALE, c["intr"], c["poses"], c["colors"])
    # stride: exactly the observations on the stride's grid
    c2w, _ = R.cam_to_world(c["poses"])
    o1 = R.observations(c["depth_u16"], K.DEPTH_SCALE, c["intr"], c2w, c["colors"])
    o2 = R.observations(c["depth_u16"], K.DEPTH_SCALE, c["intr"], c2w, c["colors"], stride=2)
    on_grid = (o1["vi"] % 2 == 0) & (o1["ui"] % 2 == 0)
    assert 0 < len(o2["key"]) < len(o1["key"]) and np.array_equal(o2["key"], o1["key"][on_grid]) and np.array_equal(o2["rgb"], o1["rgb"][on_grid])
    # the colour pixel is the one under the depth pixel's centre
    Hd, Wd, Hc, Wc = 120, 160, 97, 131
    vi, ui = o1["vi"][:1000], o1["ui"][:1000]
    yc, xc = np.floor((vi + 0.5) * Hc / Hd).astype(int), np.floor((ui + 0.5) * Wc / Wd).astype(int)
    assert np.array_equal(o1["rgb"][:1000], c["colors"][o1["view"][:1000], yc, xc])
    # min_obs only filters
    one = R.fuse(c["depth_u16"], K.DEPTH_SCALE, c["intr"], c["poses"], c["colors"], min_obs=1)
    three = R.fuse(c["depth_u16"], K.DEPTH_SCALE, c["intr"], c["poses"], c["colors"], min_obs=3)
    assert len(three["obs"]) < len(base["obs"]) < len(one["obs"]) and one["obs"].min() == 1 and three["obs"].min() == 3
    assert np.array_equal(one["points"][one["obs"] >= 2], base["points"])
    # a NaN pose drops its view, whatever its depth holds
    poses = c["poses"].copy()
    poses[3, 1, 2] = np.nan
    keep = np.array([0, 1, 2, 4, 5, 6, 7])
    assert _same(R.fuse(c["depth_u16"], K.DEPTH_SCALE, c["intr"], poses, c["colors"]),
                 R.fuse(c["depth_u16"][keep], K.DEPTH_SCALE, c["intr"][keep], c["poses"][keep], c["colors"][keep]))
    # without the edge test more pixels take part
    assert R.fuse(c["depth_u16"], K.DEPTH_SCALE, c["intr"], c["poses"], c["colors"], edge_rel=None)["pixels_used"] > base["pixels_used"]


def test_room_is_a_room():
    """The synthetic scene is what it claims: every fused point lies on a face of the room or of a box, to the depth quantisation."""
    c = K.room_case()
    out = R.fuse(c["depth_u16"], K.DEPTH_SCALE, c["intr"], c["poses"], c["colors"])
    p = out["points"][:, :3].astype(np.float64)
    dist = np.minimum(np.abs(p - K.ROOM_LO), np.abs(p - K.ROOM_HI)).min(axis=1)
    for lo, hi in K.BOXES:
        inside = ((p >= lo - 0.01) & (p <= hi + 0.01)).all(axis=1)
        dist = np.where(inside, np.minimum(dist, np.minimum(np.abs(p - lo), np.abs(p - hi)).min(axis=1)), dist)
    # a point is a mean of surface points of one cell, so it is within a cell's diagonal of a surface; away from the room's edges it
    # is on one, to the millimetre quantisation of the depth
    assert len(p) > 2000 and dist.max() < 0.02 * 3 ** 0.5 and np.median(dist) < 0.002, (dist.max(), np.median(dist))
    assert (p < 0).any(axis=0).all()                                                   # negative coordinates on every axis


def test_float32_cell_shift_share_is_recorded():
    """A figure for profiles/fuse_views.md, not a bound: the share of observations whose cell the fp32 back-projection moves."""
    share, P = K.cell_shift_share()
    print(f"room: {P} observations, cells moved by the float32 back-projection: {share:.4%}")
    assert P > 50000 and 0.0 <= share <= 1.0
