"""csrc/tsdf.hip + segdino3d_amd/tsdf.py against the numpy restatement tests/tsdf_ref.py (the reference has no counterpart) on the
synthetic room and the hand-built scenes of tests/fuse_views_case.py and tests/tsdf_case.py.

Bounds.  None: the block keys, the sorted voxel state (key, W, T, C), the BITS of the vertices, the cell keys, the faces and every
counter must EQUAL the float32 restatement.  Every decision of the rule is an integer one or a single rounded fp32 operation, the
per-voxel state is integer sums, and every emitted float is a fixed sequence of rounded fp32 operations on identical integers."""
import numpy as np
import pytest
import torch

import fuse_views_case as K
import tsdf_case as C
import tsdf_ref as R

pytestmark = pytest.mark.gpu

SMALL = 1 << 12                      # blocks: several times what the largest case here touches; 48 MB of state


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _t(a, d):
    return torch.from_numpy(np.array(a)).to(d)                   # a copy: the shared cases are read-only


def _views(c, d, kind="u16", idx=None):
    from segdino3d_amd import lift2d
    idx = slice(None) if idx is None else idx
    depth, scale = C.depth_of(c, kind)
    return lift2d.Views(_t(depth[idx], d), _t(c["intr"][idx], d), c["poses"][idx], scale)


def _volume(c, d, kind="u16", capacity=SMALL, **kw):
    from segdino3d_amd import tsdf
    vol = tsdf.TsdfVolume(capacity=capacity, **kw)
    vol.add(_views(c, d, kind), _t(c["colors"], d))
    return vol


def _equal_state(vol, want, what):
    keys, W, T, Cs = (x.cpu().numpy() for x in vol.state())
    assert np.array_equal(keys.view(np.uint64), want.keys), what
    assert np.array_equal(W, want.W) and np.array_equal(T, want.T) and np.array_equal(Cs, want.C), what


def _equal_mesh(got, want, what):
    vertices, faces, info, keys = got
    assert vertices.dtype == torch.float32 and faces.dtype == torch.int32 and keys.dtype == torch.int64 and vertices.is_contiguous(), what
    assert tuple(vertices.shape) == want.vertices.shape and tuple(faces.shape) == want.faces.shape, (what, vertices.shape, faces.shape)
    assert np.array_equal(keys.cpu().numpy().view(np.uint64), want.keys), what
    assert np.array_equal(vertices.cpu().numpy().view(np.uint32), want.vertices.view(np.uint32)), what
    assert np.array_equal(faces.cpu().numpy(), want.faces), what
    assert tuple(info) == (len(want.vertices), len(want.faces), want.blocks, want.voxels_observed, want.updates, want.out_of_range, 0), \
        (what, info)


def _check(c, d, kind="u16", what="", capacity=SMALL, **kw):
    want_vol, want = C.ref(c, kind, **kw)
    vol = _volume(c, d, kind, capacity, **kw)
    _equal_state(vol, want_vol, (what, kind, kw))
    _equal_mesh(vol.mesh(return_info=True, return_keys=True), want, (what, kind, kw))
    return want_vol, want


def _with(c, **over):
    return {**c, **over}


# ---------------------------------------------------------------------------------------------- nothing to fuse
def test_no_views_one_pixel_and_no_depth():
    from segdino3d_amd import lift2d, tsdf
    d = dev()
    none = lift2d.Views(torch.zeros(0, 4, 6, dtype=torch.uint16).to(d), np.zeros((0, 4), np.float32), np.zeros((0, 4, 4)), K.DEPTH_SCALE)
    vertices, faces, info = tsdf.tsdf_mesh(none, torch.zeros(0, 4, 6, 3, dtype=torch.uint8, device=d), return_info=True)
    assert tuple(vertices.shape) == (0, 6) and vertices.is_cuda and tuple(faces.shape) == (0, 3) and info == tsdf.TsdfInfo(0, 0, 0, 0, 0, 0, 0)
    vol, mesh = _check(K.wall(1, 1, 1.0), d, min_weight=1, what="1 x 1")
    assert len(vol.keys) > 0 and vol.updates > 0 and len(mesh.vertices) > 0            # fx = 1: the one pixel is a frustum a metre wide
    wall = K.wall(9, 11, 1.0)
    dark = _with(wall, depth_u16=np.zeros_like(wall["depth_u16"]), depth_f32=np.zeros_like(wall["depth_f32"]))
    for kind in ("u16", "f32"):
        vol, _ = _check(dark, d, kind, min_weight=1, what="all depth 0")
        assert len(vol.keys) == 0 and vol.updates == 0


# ---------------------------------------------------------------------------------------------- tile and image edges
@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("hw", [(5, 7), (9, 63), (9, 64), (9, 65), (17, 33)])
def test_small_and_odd_images(hw, kind):
    d = dev()
    c = K.noisy(hw[0], hw[1], V=2, seed=hw[1], color_hw=(hw[0] + 2, hw[1] - 3))
    vol, mesh = _check(c, d, kind, min_weight=1, what=hw)
    assert vol.updates > 0 and len(vol.keys) > 4
    if hw[0] > 5:
        assert len(mesh.vertices) > 20 and len(mesh.faces) > 10


def test_wall_on_a_block_face_at_a_negative_coordinate():
    d = dev()
    vol, mesh = _check(C.block_face_wall(), d, "f32", what="block face", **C.BLOCK_FACE_RULE)
    assert (mesh.vertices[:, 0] == -1.0).all() and len(mesh.faces) > 50 and R.block_coords(vol.keys)[:, 0].min() == -5
    vol, mesh = _check(C.block_face_wall(on_centres=True), d, "f32", what="voxel centres", **C.BLOCK_FACE_RULE)
    assert ((vol.W > 0) & (vol.T == 0)).sum() > 50 and len(mesh.faces) > 50


@pytest.mark.parametrize("kw", [dict(voxel=0.05, trunc=0.05), dict(voxel=0.05, trunc=0.4), dict(voxel=0.05, min_weight=1),
                                dict(voxel=0.05, min_weight=3), dict(voxel=0.05, edge_rel=None),
                                dict(voxel=0.0625, trunc=0.1, near=0.8, far=2.5, edge_abs=0.0, edge_rel=0.01)])
def test_room_rule_parameters(kw):
    d = dev()
    _, mesh = _check(K.room_case(), d, what="room", **kw)
    assert len(mesh.vertices) > 200 and len(mesh.faces) > 300


def test_depth_straddles_near_and_far_exactly():
    d = dev()
    raw = np.array([[99, 100, 101, 5999], [6000, 6001, 199, 200], [201, 11999, 12000, 12001]], np.uint16)[None]
    for scale, near, far in ((0.001, 0.1, 6.0), (0.0005, 0.1, 6.0), (0.0005, 0.05, 3.0)):
        c = _with(K.wall(3, 4, 1.0), depth_u16=raw, depth_f32=raw.astype(np.float32) * np.float32(scale), scale=scale)
        for kind in ("u16", "f32"):
            vol, _ = _check(c, d, kind, min_weight=1, edge_rel=None, near=near, far=far, voxel=0.05, what=(scale, near, far))
            assert vol.updates > 0


def test_nan_pose_is_dropped():
    from segdino3d_amd import tsdf
    d = dev()
    c = K.room_case()
    poses = c["poses"].copy()
    poses[3, 1, 2] = np.nan
    bad = _with(c, poses=poses)
    _, want = _check(bad, d, what="NaN pose", **C.ROOM_RULE)
    keep = np.array([0, 1, 2, 4, 5, 6, 7])
    views = _views(bad, d)                                                            # colours per KEPT view give the same mesh
    assert len(views) == 7 and views.n_given == 8
    vertices, faces = tsdf.tsdf_mesh(views, _t(c["colors"][keep], d), capacity=SMALL, **C.ROOM_RULE)
    assert np.array_equal(vertices.cpu().numpy().view(np.uint32), want.vertices.view(np.uint32)) and np.array_equal(faces.cpu().numpy(), want.faces)


def test_samples_beyond_the_world_are_counted_not_written():
    d = dev()
    c = K.wall(9, 20, 1.0, V=2)
    poses = c["poses"].copy()
    poses[1, 0, 3] = 2.0 ** 14                                                         # view 1 lands at x >= 2^14 m
    vol, mesh = _check(_with(c, poses=poses), d, min_weight=1, what="2^14")
    assert vol.out_of_range == 5 * 9 * 20 and len(mesh.vertices) > 0
    poses[0, 1, 3] = -3.0e38                                                           # and view 0 at the end of fp32
    vol, mesh = _check(_with(c, poses=poses), d, min_weight=1, what="inf")
    assert vol.out_of_range == 2 * 5 * 9 * 20 and len(vol.keys) == 0 and len(mesh.vertices) == 0


# ---------------------------------------------------------------------------------------------- the room
@pytest.mark.parametrize("color_hw", [(60, 80), (97, 131)])
def test_room(color_hw):
    d = dev()
    want_vol, want = C.room_ref(color_hw)
    vol = _volume(K.room_case(color_hw), d, **C.ROOM_RULE)
    _equal_state(vol, want_vol, ("room", color_hw))
    _equal_mesh(vol.mesh(return_info=True, return_keys=True), want, ("room", color_hw))
    assert len(want.vertices) > 3000 and len(want.faces) > 5000
    _check(K.room_case(color_hw), d, "f32", what=("room f32", color_hw), **C.ROOM_RULE)


def test_more_views_than_one_call_takes():
    """70 views: two touch / integrate pairs, the second with 6 views."""
    d = dev()
    c = K.wall(9, 20, 1.0, V=70)
    vol, mesh = _check(c, d, voxel=0.05, what="70 views")
    assert vol.W.max() > 64 and len(mesh.vertices) > 0


# ---------------------------------------------------------------------------------------------- a function of the set of frames
def test_cut_order_and_stream_do_not_change_a_bit():
    from segdino3d_amd import ops, tsdf
    d = dev()
    c = K.room_case()
    whole = _volume(c, d, **C.ROOM_RULE)
    base_v, base_f = whole.mesh()
    base_state = whole.state()
    assert base_v.shape[0] == len(C.room_ref()[1].vertices)
    colors = _t(c["colors"], d)

    def same(vol, what):
        v, f = vol.mesh()
        assert torch.equal(v, base_v) and torch.equal(f, base_f), what
        assert all(torch.equal(a, b) for a, b in zip(vol.state(), base_state)), what

    for order in (list(range(8)), list(range(7, -1, -1)), [5, 2, 7, 0, 3, 6, 1, 4]):
        vol = tsdf.TsdfVolume(capacity=SMALL, **C.ROOM_RULE)
        for i in order:                                                               # one add per view
            vol.add(_views(c, d, idx=slice(i, i + 1)), colors[i:i + 1])
        same(vol, order)
    vol = tsdf.TsdfVolume(capacity=SMALL, **C.ROOM_RULE)
    rev = np.arange(7, -1, -1)
    vol.add(_views(c, d, idx=rev[:3]), colors[torch.from_numpy(rev[:3].copy()).to(d)])
    half_v, _ = vol.mesh()                                                            # a mesh in between does not disturb the state
    vol.add(_views(c, d, idx=rev[3:]), colors[torch.from_numpy(rev[3:].copy()).to(d)])
    same(vol, "after a mesh in between")
    same(vol, "twice")
    assert 0 < half_v.shape[0] < base_v.shape[0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with ops.use_stream(side):
        got = _volume(c, d, **C.ROOM_RULE)
        v, f = got.mesh()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(v, base_v) and torch.equal(f, base_f)


def test_overflow_is_an_error_not_a_thinner_mesh():
    d = dev()
    c = K.room_case()
    vol = _volume(c, d, capacity=64, **C.ROOM_RULE)
    with pytest.raises(RuntimeError, match=r"overflow = \d+ .* capacity = 64 \(\d+ blocks held, \d+ updates"):
        vol.mesh()
    assert vol.info.overflow > 0 and vol.info.blocks <= 64
    want_vol, want = C.room_ref()
    fresh = _volume(c, d, capacity=1 << 12, **C.ROOM_RULE)
    _equal_state(fresh, want_vol, "after an overflow")
    _equal_mesh(fresh.mesh(return_info=True, return_keys=True), want, "after an overflow")
    with pytest.raises(RuntimeError, match=r"vertices = \d+, more than max_vertices = 100"):
        fresh.mesh(max_vertices=100)
    _equal_mesh(fresh.mesh(return_info=True, return_keys=True, max_vertices=len(want.vertices)), want, "max_vertices exactly")


# ---------------------------------------------------------------------------------------------- the chain
def test_mesh_feeds_superpoints_and_lifting():
    """Views -> mesh -> mesh_superpoints: labels and count EQUAL tests/superpoints_ref.py on the same mesh.  The vertices go through
    lift2d.lift_point_features with the room's views: shape and finiteness only, lift2d's own tests cover its values."""
    import superpoints_ref as S
    from segdino3d_amd import lift2d, superpoints, tsdf
    d = dev()
    c = K.room_case()
    views = _views(c, d)
    vertices, faces = tsdf.tsdf_mesh(views, _t(c["colors"], d), capacity=SMALL, **C.ROOM_RULE)
    _, want = C.room_ref()
    assert np.array_equal(vertices.cpu().numpy().view(np.uint32), want.vertices.view(np.uint32)) and np.array_equal(faces.cpu().numpy(), want.faces)
    labels, info = superpoints.mesh_superpoints(vertices[:, :3].contiguous(), faces, return_info=True)
    ref = S.mesh_superpoints(np.ascontiguousarray(want.vertices[:, :3]), want.faces)
    assert np.array_equal(labels.cpu().numpy(), ref.labels) and info.count == ref.count and ref.count > 1 and info.bad_faces == 0
    maps = _t(np.random.default_rng(0).standard_normal((8, 15, 20, 64)).astype(np.float16), d)
    feats = lift2d.lift_point_features(vertices, views, maps)
    assert tuple(feats.shape) == (len(want.vertices), 64) and bool(torch.isfinite(feats).all())


# ---------------------------------------------------------------------------------------------- arguments
def test_device_argument_errors():
    from segdino3d_amd import ops, tsdf
    d = dev()
    c = K.wall(9, 20, 1.0)
    views, colors = _views(c, d), _t(c["colors"], d)
    vol = tsdf.TsdfVolume(capacity=SMALL)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vol.add(views, colors.cpu())
    with pytest.raises(TypeError, match="uint8"):
        vol.add(views, colors.float())
    with pytest.raises(ValueError, match="one colour image per view"):
        vol.add(views, colors.repeat(2, 1, 1, 1))
    with pytest.raises(ValueError, match=r"\[V, Hc, Wc, 3\]"):
        vol.add(views, colors[..., :2])
    with pytest.raises(TypeError, match="lift2d.Views"):
        vol.add(c["depth_u16"], colors)
    ws = ops.tsdf_workspace(SMALL, d)
    with pytest.raises(RuntimeError, match="workspace too small"):
        ops.tsdf_mesh(ws[:4096], SMALL, 1, 0.02, 64)
    with pytest.raises(RuntimeError, match="workspace too small"):
        ops.tsdf_touch(views.depth, views.depth_scale, views.intrinsics, views.cam_to_world, ws[:4096], SMALL, 50.0, 0.04)
    with pytest.raises(ValueError, match="at most 64 views"):
        ops.tsdf_touch(views.depth.repeat(65, 1, 1), views.depth_scale, views.intrinsics.repeat(65, 1), views.cam_to_world.repeat(65, 1, 1),
                       ws, SMALL, 50.0, 0.04)
    with pytest.raises(ValueError, match="capacity"):
        ops.tsdf_workspace(1000, d)
    vertices, faces = vol.mesh()
    assert tuple(vertices.shape) == (0, 6) and tuple(faces.shape) == (0, 3)           # nothing was added by the refused calls


# ---------------------------------------------------------------------------------------------- steps 2 and 3 of the pixel rule, directly
@pytest.mark.parametrize("edges", C.PIXEL_RULE_EDGES, ids=("edges", "no-edges"))
@pytest.mark.parametrize("kind", ("u16", "f32"))
@pytest.mark.parametrize("H, W", C.PIXEL_RULE_SIZES)
def test_touch_vdepth_equals_the_pixel_rule(H, W, kind, edges):
    """`vdepth` of ops.tsdf_touch is the front end every depth-pixel stage shares (csrc/depth_pixel.h): d where the pixel is valid by
    steps 2 and 3, else 0.  Bit for bit against valid_pixels of tests/fuse_views_ref.py on images with a zero, a NaN (fp32), a pixel
    exactly at `near` and one exactly at `far`, and a step edge; tests/test_tsdf_ref.py checks that each image has pixels of both
    kinds."""
    from segdino3d_amd import ops
    d = dev()
    c = C.pixel_rule_case(H, W, kind)
    ok = C.pixel_rule_valid(c, **edges)
    assert ok.any() and not ok.all()
    want = np.where(ok, c["metres"], np.float32(0))
    c2w, _ = K.R.cam_to_world(c["poses"])
    ws = ops.tsdf_workspace(1 << 10, d)
    got = ops.tsdf_touch(_t(c["depth"], d), c["scale"], _t(c["intr"], d), _t(c2w, d), ws, 1 << 10, 50.0, 0.04, c["near"], c["far"], **edges)
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, H, W)
    assert np.array_equal(got.cpu().numpy()[0].view(np.uint32), want.view(np.uint32)), (H, W, kind, edges)
