"""csrc/raster.hip + segdino3d_amd/raster.py against the numpy restatement tests/raster_ref.py (the reference has no counterpart) on the
inputs of tests/raster_case.py and hand-built ones.

Bounds.  None: the BITS of depth, face, vertex, the label images and all six counters must EQUAL the restatement.  Every decision of
the rule is a comparison of single rounded fp32 / fp64 operations or of int64 edge functions, and the image is a minimum over a set of
integer keys."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fuse_views_ref as FR
import raster_case as K
import raster_ref as R
import transfer_case as TC
import transfer_ref as T

pytestmark = pytest.mark.gpu

F32 = np.float32


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _t(a, d):
    return torch.from_numpy(np.array(a)).to(d)                   # a copy: the shared cases are read-only


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _same(res, want, what=""):
    """A `RenderResult` against the restatement's dict: everything that was asked for."""
    from segdino3d_amd import ops
    assert list(res.kept) == list(want["kept"]), what
    k = len(want["kept"])
    for name in ("depth", "face", "vertex"):
        got = _np(getattr(res, name))
        if got is None:
            continue
        assert got.shape == want[name].shape and got.shape[0] == k, (what, name, got.shape)
        if name == "depth":
            assert got.dtype == F32 and np.array_equal(_bits(got), _bits(want[name])), (what, name, int((_bits(got) != _bits(want[name])).sum()))
        else:
            assert got.dtype == np.int32 and np.array_equal(got, want[name]), (what, name, int((got != want[name]).sum()))
    for name in ("face_label_images", "vertex_label_images"):
        got = _np(getattr(res, name))
        assert (got is None) == (want[name] is None), (what, name)
        if got is not None:
            assert got.dtype == np.int32 and got.shape == want[name].shape and np.array_equal(got, want[name]), (what, name)
    info = res.read_info()
    assert tuple(info) == ops.RASTER_INFO == R.INFO and info == want["info"], (what, info, want["info"])


def _run(d, vertices, faces, intr, poses, H, W, face_labels=None, vertex_labels=None, fill=-1, near=0.1, far=6.0, what="", **kw):
    """render_mesh on the device with every image asked for, held against the restatement -> (RenderResult, the restatement's dict)."""
    from segdino3d_amd import raster
    want = R.render_mesh(vertices, faces, intr, poses, H, W, near=near, far=far, face_labels=face_labels, vertex_labels=vertex_labels, fill=fill)
    res = raster.render_mesh(_t(vertices, d), _t(faces, d), intr, poses, H, W, near=near, far=far, fill=fill, return_vertex=True,
                             face_labels=None if face_labels is None else _t(face_labels, d),
                             vertex_labels=None if vertex_labels is None else _t(vertex_labels, d), **kw)
    _same(res, want, what)
    return res, want


def _run_px(d, corners_px, H, W, what="", z=2.0, f=64.0, cx=0.0, cy=0.0, **kw):
    v, fc, intr = K.pixel_mesh(corners_px, z=z, f=f, cx=cx, cy=cy)
    return _run(d, v, fc, intr, K.IDENTITY, H, W, what=what, **kw)


ONE = [[[0, 0], [9, 0], [0, 9]]]                                  # a triangle in pixels that covers the top left corner


# ---------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("case", ["F0", "Nv0", "V0", "K0"])
def test_nothing_to_draw_launches_nothing_and_returns_the_fills(case, monkeypatch):
    from segdino3d_amd import ops, raster
    d = dev()
    v, f, intr = K.pixel_mesh(ONE)
    poses = np.stack([np.eye(4)] * 2)
    intr = np.repeat(intr, 2, axis=0)
    if case == "F0":
        f = f[:0]
    elif case == "Nv0":
        v = v[:0]
    elif case == "V0":
        poses, intr = poses[:0], intr[:0]
    else:
        poses = poses.copy()
        poses[:, 0, 0] = np.nan
    flab, vlab = np.arange(len(f), dtype=np.int32), np.arange(2 * len(v), dtype=np.int32).reshape(2, -1)

    def boom(*a, **kw):
        raise AssertionError("a launch")
    monkeypatch.setattr(ops, "raster_views", boom)
    res, want = _run(d, v, f, intr, poses, 5, 7, face_labels=flab, vertex_labels=vlab, fill=-7, what=case)
    k = 0 if case in ("V0", "K0") else 2
    assert res.n_given == len(poses) and len(res.kept) == k and res.depth.shape == (k, 5, 7) and res.vertex_label_images.shape == (2, k, 5, 7)
    assert res.face_label_images.shape == (k, 5, 7)
    if k:
        assert (res.depth == 0).all() and (res.face == -1).all() and (res.vertex == -1).all() and (res.vertex_label_images == -7).all()
        assert res.read_info()["bad"] == (2 if case == "Nv0" else 0)
    views = raster.rendered_views(_t(v, d), _t(f, d), intr, poses, 5, 7)
    assert len(views) == k and views.n_given == len(poses) and views.depth.shape == (k, 5, 7)


def test_one_view_of_one_pixel():
    res, want = _run_px(dev(), [[[-1, -1], [3, -1], [-1, 3]]], 1, 1)
    assert want["info"]["pixels"] == 1 and want["depth"][0, 0, 0] == 2.0 and want["vertex"][0, 0, 0] == 0


def test_an_image_that_is_a_multiple_of_no_tile_or_wave_width():
    c = K.soup()
    intr = np.array([[32, 32, 26, 18], [30.5, 31.25, 25.3, 17.9]], dtype=F32)
    res, want = _run(dev(), c["vertices"], c["faces"], intr, c["poses"][[0, 2]], 37, 53, face_labels=c["face_labels"][:1])
    assert want["info"]["pixels"] > 0.8 * 2 * 37 * 53 and want["info"]["drawn"] > 500


# ---------------------------------------------------------------------------------------------- the edges of the image
def test_triangles_across_and_beyond_the_image_edges():
    H, W = 24, 40
    tris = [[[-6, 5], [5, 3], [-2, 12]],                                             # across the left edge
            [[35, 2], [47, 6], [37, 11]],                                            # the right
            [[12, -7], [22, -3], [15, 4]],                                           # the top
            [[20, 20], [30, 29], [17, 31]],                                          # the bottom
            [[-9, -9], [-2, -8], [-5, -1]], [[41, 30], [50, 26], [45, 40]],          # fully outside: two corners of the plane
            [[W - 1 + 0.5, 3], [W + 4, 3], [W + 2, 9]],                              # just beyond the last column
            [[-100, -100], [300, -100], [-100, 300]]]                                # the whole image and far more: the large path
    res, want = _run_px(dev(), tris, H, W, z=4.0)
    assert want["info"] == dict(drawn=5, near=0, guard=0, empty=3, bad=0, pixels=H * W)
    assert all((want["face"][0] == i).any() for i in range(4)) and (want["face"][0] == 7).sum() > H * W // 2


# ---------------------------------------------------------------------------------------------- thresholds
def test_near_is_inclusive_at_the_corner():
    """Identity pose: z_c IS the vertex's z.  A corner at z_c == near stays; the next float below drops the face under `near`."""
    d = dev()
    for z0, drawn in ((F32(0.5), 1), (np.nextafter(F32(0.5), F32(1)), 1), (np.nextafter(F32(0.5), F32(0)), 0)):
        v = np.array([[0, 0, z0], [0.5, 0, 1.0], [0, 0.5, 1.0]], dtype=F32)
        res, want = _run(d, v, np.array([[0, 1, 2]], np.int32), np.array([[16, 16, 0, 0]], F32), K.IDENTITY, 12, 12, near=0.5, far=0.5 * 4,
                         what=repr(z0))
        assert want["info"]["drawn"] == drawn and want["info"]["near"] == 1 - drawn and (want["info"]["pixels"] > 0) == bool(drawn)


def test_far_is_inclusive_at_the_plane():
    """A camera-facing plane at z_c = 4 renders d == 4.0 exactly: kept with far == 4.0, dropped (though drawn) with the next float
    below as `far`; and the plane one float beyond 4 is dropped with far == 4.0.  From the other side a plane AT `near` is kept, and
    one float nearer its corners fail step 2: the face is not drawn at all."""
    d = dev()
    four, above, below = F32(4.0), np.nextafter(F32(4.0), F32(5)), np.nextafter(F32(4.0), F32(0))
    for z, near, far, drawn, hit in ((four, 0.1, four, 1, True), (four, 0.1, below, 1, False), (above, 0.1, four, 1, False),
                                     (above, 0.1, above, 1, True), (four, four, four, 1, True), (four, above, 6.0, 0, False),
                                     (below, four, 6.0, 0, False)):
        v = np.array([[0, 0, z], [1, 0, z], [0, 1, z]], F32)
        res, want = _run(d, v, np.array([[0, 1, 2]], np.int32), np.array([[32, 32, 0, 0]], F32), K.IDENTITY, 12, 12, near=float(near),
                         far=float(far), what=f"{z!r} {near!r} {far!r}")
        assert want["info"]["drawn"] == drawn and want["info"]["near"] == 1 - drawn and (want["info"]["pixels"] > 0) == hit, (z, near, far)
        if hit:
            assert set(np.unique(want["depth"]).tolist()) == {0.0, float(z)}


def test_the_projection_guard_on_both_sides():
    """fx = 2, z_c = 1, cx = 0: u = 2 x exactly.  x = 8192 projects onto 2^14 and drops the face under `guard` (the coordinate itself
    is far below its own limit); the float below 8192 stays inside and the face is drawn."""
    d = dev()
    for x, guard in ((F32(8192.0), 1), (np.nextafter(F32(8192.0), F32(0)), 0), (F32(-8192.0), 1), (np.nextafter(F32(-8192.0), F32(0)), 0)):
        for axis in (0, 1):
            v = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1]], dtype=F32)
            v[0, axis], v[1, 1 - axis] = x, 5.0                                        # the other two corners: (0, 0) and 10 px along the other axis
            res, want = _run(d, v, np.array([[0, 1, 2]], np.int32), np.array([[2, 2, 0, 0]], F32), K.IDENTITY, 8, 8, what=f"{x!r} {axis}")
            assert want["info"]["guard"] == guard and want["info"]["drawn"] == 1 - guard and (want["info"]["pixels"] > 0) == (not guard)


def test_a_face_of_zero_area_after_the_snap():
    """(1, 1), (3, 1), (5, 1 + 1/1024): the third corner snaps onto the line of the other two, A == 0, `empty`.  One sub-pixel step
    further it is a (thin) triangle and is drawn."""
    d = dev()
    res, want = _run_px(d, [[[1, 1], [3, 1], [5, 1 + 1 / 1024]]], 8, 8)
    assert want["info"] == dict(drawn=0, near=0, guard=0, empty=1, bad=0, pixels=0)
    res, want = _run_px(d, [[[1, 1], [3, 1], [5, 1 + 1 / 256]]], 8, 8)
    assert want["info"]["drawn"] == 1 and want["info"]["pixels"] == 3


def test_bad_faces():
    d = dev()
    v = np.array([[0, 0, 1], [0.1, 0, 1], [0, 0.1, 1], [np.nan, 0, 1], [0, 16384.0, 1], [0, 0, -np.inf], [0, np.nextafter(F32(16384), F32(0)), 1]], F32)
    f = np.array([[0, 1, -1], [0, 1, 2], [7, 1, 2], [0, 3, 2], [4, 1, 2], [0, 1, 5], [0, 1, 6], [-2147483648, 2147483647, 0]], dtype=np.int32)
    res, want = _run(d, v, f, np.array([[64, 64, 4, 4]], F32), K.IDENTITY, 16, 16, vertex_labels=np.arange(7, dtype=np.int32))
    assert list(want["classes"][0]) == [R.BAD, R.DRAWN, R.BAD, R.BAD, R.BAD, R.BAD, R.GUARD, R.BAD] and want["info"]["pixels"] > 0


# ---------------------------------------------------------------------------------------------- the two draw kernels
def _box(area):
    bw = max(b for b in range(1, int(area ** 0.5) + 1) if area % b == 0)
    return bw, area // bw


def test_size_classes_straddle_the_threshold():
    """Triangles whose clamped bounding box holds S - 1, S and S + 1 pixels (S = ops.RASTER_SMALL_MAX_PIXELS): the first two are drawn
    one lane each, the third by a wave; alone and all together (on top of each other) they equal the restatement, which has no such
    classes.  Then the S + 1 triangle pushed across the image corner until its CLAMPED box is small again."""
    from segdino3d_amd import ops
    d = dev()
    S = ops.RASTER_SMALL_MAX_PIXELS
    boxes = [_box(S - 1), _box(S), _box(S + 1)]
    side = max(max(b) for b in boxes) + 6
    tris = [K.box_triangle(2, 3, bw, bh) for bw, bh in boxes]
    v, f, intr = K.pixel_mesh(tris)
    w2c, _ = R.world_to_cam(K.IDENTITY)
    assert list(R.box_pixels(R.setup(v, f, w2c[0], intr[0], 0.1, side, side))) == [S - 1, S, S + 1]
    for i in range(3):
        _run_px(d, tris[i:i + 1], side, side, what=f"area {S - 1 + i}")
    res, want = _run_px(d, tris, side, side, what="together")
    assert want["samples"] > want["info"]["pixels"] > 0
    bw, bh = boxes[2]
    shifted = [[[x - 3, y - 4] for x, y in K.box_triangle(2, 3, bw, bh)]]
    v, f, intr = K.pixel_mesh(shifted)
    assert 0 < R.box_pixels(R.setup(v, f, w2c[0], intr[0], 0.1, side, side))[0] <= S
    _run_px(d, shifted, side, side, what="clamped")


# ---------------------------------------------------------------------------------------------- ties
def test_depth_ties_go_to_the_lower_face_index():
    """The soup's coincident walls tie on every pixel they show on: preferring the higher index changes more than 1 500 faces."""
    fwd, rev = K.soup_ref(), K.soup_ref(reverse_ties=True)
    assert (fwd["face"] != rev["face"]).sum() > 1500 and np.array_equal(_bits(fwd["depth"]), _bits(rev["depth"]))
    c = K.soup()
    res, _ = _run(dev(), c["vertices"], c["faces"], c["intr"], c["poses"], c["H"], c["W"])
    assert not np.array_equal(_np(res.face), rev["face"])
    # coincident duplicates of one triangle: face 0 everywhere
    tri = [[1, 1], [9, 1], [1, 9]]
    res, want = _run_px(dev(), [tri, tri, tri], 12, 12)
    assert set(np.unique(want["face"]).tolist()) == {-1, 0} and want["samples"] == 3 * want["info"]["pixels"]


def test_vertex_ties_go_to_the_lowest_corner():
    """w1 == w2 > w0 at (4, 4) and w0 > w1 == w2 at (2, 2) of the first triangle, all three equal at (2, 2) of the others, and
    w0 == w1 > w2 at (3, 3) of the last (tests/test_raster_ref.py holds the restatement's values against the hand count)."""
    d = dev()
    res, want = _run_px(d, [[[0, 0], [8, 0], [0, 8]]], 10, 10)
    assert want["vertex"][0, 4, 4] == 1 and want["vertex"][0, 2, 2] == 0
    res, want = _run_px(d, [[[0, 0], [6, 0], [0, 6]]], 10, 10)
    assert want["vertex"][0, 2, 2] == 0
    res, want = _run_px(d, [[[6, 0], [0, 6], [0, 0]]], 10, 10)
    assert want["vertex"][0, 2, 2] == 0 and want["vertex"][0, 3, 3] == 0


# ---------------------------------------------------------------------------------------------- the soup, labels, cuts and streams
def test_soup():
    c, want = K.soup(), K.soup_ref()
    res, again = _run(dev(), c["vertices"], c["faces"], c["intr"], c["poses"], c["H"], c["W"], face_labels=c["face_labels"],
                      vertex_labels=c["vertex_labels"])
    _same(res, want, "the cached restatement")
    assert res.n_given == 3 and list(res.kept) == [0, 2] and want["info"]["near"] > 0 and want["info"]["empty"] > 0
    assert want["samples"] > 2 * want["info"]["pixels"]                               # overdraw: the minimum is what decides


@pytest.mark.parametrize("which", ["face", "vertex", "both", "fill", "int64", "uint8", "bool", "rows"])
def test_labels(which):
    from segdino3d_amd import raster
    d = dev()
    c = K.soup()
    fl, vl = c["face_labels"], c["vertex_labels"]
    args = (c["vertices"], c["faces"], c["intr"], c["poses"], c["H"], c["W"])
    if which == "face":
        _run(d, *args, face_labels=fl)
    elif which == "vertex":
        _run(d, *args, vertex_labels=vl)
    elif which == "both":
        res, want = _run(d, *args, face_labels=fl, vertex_labels=vl)                  # 3 + 5 = 8
        assert res.face_label_images.shape == (3, 2, 64, 80) and res.vertex_label_images.shape == (5, 2, 64, 80)
    elif which == "fill":
        res, want = _run(d, *args, face_labels=fl[:2], vertex_labels=vl[:1], fill=-7)
        assert (want["face_label_images"] == -7).any() and not (want["face_label_images"] == -1).all()
    elif which == "rows":                                                             # one row given alone comes back without the channel axis
        res, want = _run(d, *args, face_labels=fl[0], vertex_labels=vl[1])
        assert res.face_label_images.shape == res.vertex_label_images.shape == (2, 64, 80)
    else:
        dtype = dict(int64=np.int64, uint8=np.uint8, bool=np.bool_)[which]
        f2, v2 = (fl[:2] % 7 + 1).astype(dtype), (vl[:2] % 2).astype(dtype)
        res, want = _run(d, *args, face_labels=f2, vertex_labels=v2, fill=0)
        assert res.face_label_images.dtype == torch.int32 and want["vertex_label_images"].max() == 1


def test_the_cut_into_passes_and_calls_and_the_stream_do_not_matter():
    from segdino3d_amd import ops, raster
    d = dev()
    c, want = K.soup(), K.soup_ref()
    poses = np.stack([c["poses"][0], c["poses"][2], c["poses"][1], c["poses"][2], c["poses"][0]])      # 5 views, the third NaN
    intr = c["intr"][[0, 2, 1, 2, 0]]
    v, f = _t(c["vertices"], d), _t(c["faces"], d)
    fl, vl = _t(c["face_labels"], d), _t(c["vertex_labels"], d)
    kw = dict(face_labels=fl, vertex_labels=vl, return_vertex=True)
    names = ("depth", "face", "vertex", "face_label_images", "vertex_label_images")

    def images(res):
        return {n: _np(getattr(res, n)) for n in names}
    one = raster.render_mesh(v, f, intr, poses, 64, 80, **kw)
    base = images(one)
    assert list(one.kept) == [0, 1, 3, 4]
    for n in names:                                                                   # views 0 and 1 ARE the soup's two kept views
        assert np.array_equal(base[n][..., :2, :, :].view(np.uint32), want[n].view(np.uint32)), n
        assert np.array_equal(base[n][..., 2:, :, :], base[n][..., 1::-1, :, :]), n
    for vpp in (1, 3):
        res = raster.render_mesh(v, f, intr, poses, 64, 80, views_per_pass=vpp, **kw)
        assert res.read_info() == one.read_info()
        for n, a in images(res).items():
            assert np.array_equal(a.view(np.uint32), base[n].view(np.uint32)), (vpp, n)
    halves = [raster.render_mesh(v, f, intr[s], poses[s], 64, 80, **kw) for s in (slice(0, 2), slice(2, 5))]
    assert [list(h.kept) for h in halves] == [[0, 1], [1, 2]]
    for n in names:
        both = np.concatenate([images(h)[n] for h in halves], axis=-3)
        assert np.array_equal(both.view(np.uint32), base[n].view(np.uint32)), n
    total = {k: sum(h.read_info()[k] for h in halves) for k in ops.RASTER_INFO}
    assert total == one.read_info()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with ops.use_stream(side):
        res = raster.render_mesh(v, f, intr, poses, 64, 80, views_per_pass=2, **kw)
    torch.cuda.current_stream().wait_stream(side)
    for n, a in images(res).items():
        assert np.array_equal(a.view(np.uint32), base[n].view(np.uint32)), ("side stream", n)
    assert res.read_info() == one.read_info()


# ---------------------------------------------------------------------------------------------- the chain
def test_the_tsdf_room_mesh_in_two_of_its_own_poses():
    c, want = K.room(), K.room_ref()
    res, again = _run(dev(), c["vertices"], c["faces"], c["intr"], c["poses"], c["H"], c["W"])
    _same(res, want, "the cached restatement")
    assert want["info"]["drawn"] > 1000 and want["info"]["pixels"] > 10000


def test_rendered_views_feed_the_stages_that_take_views():
    from segdino3d_amd import fuse_views, lift2d, raster, transfer
    d = dev()
    c, want = K.room(), K.room_ref()
    v, f = _t(c["vertices"], d), _t(c["faces"], d)
    views = raster.rendered_views(v, f, c["intr"], c["poses"], c["H"], c["W"])
    assert isinstance(views, lift2d.Views) and len(views) == 2 and views.depth_scale is None and views.depth.dtype == torch.float32
    assert np.array_equal(_bits(_np(views.depth)), _bits(want["depth"]))
    bits, count = lift2d.visibility(v, views)
    assert bits.shape == (len(c["vertices"]), 1) and int(count.max()) >= 1 and int((count > 0).sum()) > 500   # the mesh sees itself
    idx = transfer.PointIndex(v, 0.1).nearest_pixels(views)
    c2w, kept = FR.cam_to_world(c["poses"])
    want_idx, _ = T.nearest_pixels(c["vertices"], want["depth"], None, c["intr"], c2w, 0.1)
    assert np.array_equal(_np(idx), want_idx) and (want_idx >= 0).sum() > 0.9 * want["info"]["pixels"]
    colors = torch.full((2, 60, 80, 3), 128, dtype=torch.uint8, device=d)
    points = fuse_views.fuse_views(views, colors, voxel=0.05, capacity=1 << 16, min_obs=1)
    assert points.shape[1] == 6 and points.shape[0] > 500
    # a dropped pose: the kept views are those of the poses handed in
    poses = np.concatenate([c["poses"][:1], np.full((1, 4, 4), np.nan), c["poses"][1:]])
    views3 = raster.rendered_views(v, f, c["intr"][[0, 0, 1]], poses, c["H"], c["W"], views_per_pass=1)
    assert list(views3.kept) == [0, 2] and views3.n_given == 3 and np.array_equal(_bits(_np(views3.depth)), _bits(want["depth"]))
    maps = torch.arange(3, device=d).view(3, 1, 1, 1).expand(3, 2, 2, 1)
    assert views3.select_maps(maps)[:, 0, 0, 0].tolist() == [0, 2]


def _prediction(n, d, container):
    host = TC.prediction_case(n)
    pred = {k: ([_t(x, d) for x in v] if isinstance(v, list) else _t(v, d)) for k, v in host.items()}
    if container != "dict":
        pred = SimpleNamespace(**pred)
    if container == "output":
        pred = SimpleNamespace(pred_pts_seg=pred)
    return host, pred


@pytest.mark.parametrize("container", ["dict", "output"])
def test_render_prediction_mesh(container):
    """The five images equal the restatement's vertex map read through the five channels built by transfer_ref's instance-map rule."""
    from segdino3d_amd import raster, transfer
    d = dev()
    c, want = K.room(), K.room_ref()
    host, pred = _prediction(len(c["vertices"]), d, container)
    for thr, fill in ((0.0, -1), (0.5, -3)):
        got = raster.render_prediction_mesh(_t(c["vertices"], d), _t(c["faces"], d), c["intr"], c["poses"], c["H"], c["W"], pred, score_thr=thr,
                                            fill=fill)
        imap = T.instance_map(host["pts_instance_mask"][0], host["instance_scores"], thr)
        chans = dict(semantic=host["pts_semantic_mask"][0], panoptic_semantic=host["pts_semantic_mask"][1],
                     panoptic_instance=host["pts_instance_mask"][1], instance=imap, instance_label=T.take_labels(host["instance_labels"], imap, fill))
        assert tuple(got) == transfer.PREDICTION_IMAGES == tuple(chans)
        for name, chan in chans.items():
            assert got[name].dtype == torch.int32 and np.array_equal(_np(got[name]), R.take(chan, want["vertex"], fill)), (name, thr)
    assert (_np(got["instance"]) >= 0).any() and (_np(got["instance"]) == -3).any()
    with pytest.raises(ValueError, match="render_prediction_mesh: the prediction covers"):
        raster.render_prediction_mesh(_t(c["vertices"][:-1], d), _t(c["faces"], d), c["intr"], c["poses"], c["H"], c["W"], pred)


def test_render_prediction_keeps_its_bits():
    """`transfer.render_prediction` builds its channels through the helper it now shares with `render_prediction_mesh`: the same
    images as tests/transfer_ref.py on the case of tests/test_gpu_transfer.py."""
    from segdino3d_amd import transfer
    from segdino3d_amd.lift2d import Views
    d = dev()
    c = TC.broken_pose_case("u16")
    w, ok = T.pixel_queries(c["depth"][c["kept"]], c["scale"], c["intr"][c["kept"]], c["c2w"])
    pts = np.ascontiguousarray(w[ok][::3])
    host, pred = _prediction(len(pts), d, "object")
    views = Views(_t(c["depth"], d), c["intr"], c["poses"], depth_scale=c["scale"])
    kd, ki = c["depth"][c["kept"]], c["intr"][c["kept"]]
    for thr, fill in ((0.0, -1), (0.5, -3)):
        got = transfer.render_prediction(views, _t(pts, d), pred, 0.1, score_thr=thr, fill=fill)
        want = T.render_prediction(pts, host, kd, c["scale"], ki, c["c2w"], 0.1, score_thr=thr, fill=fill)
        assert tuple(got) == transfer.PREDICTION_IMAGES == tuple(want)
        for name in want:
            assert got[name].dtype == torch.int32 and np.array_equal(_np(got[name]), want[name]), (name, thr)
    assert (want["instance"] >= 0).any() and (want["instance"] == -3).any()
    with pytest.raises(RuntimeError, match="render_prediction: pts_semantic_mask: expected tensors on the HIP device"):
        transfer.render_prediction(views, _t(pts, d), dict(host, pts_semantic_mask=[torch.zeros(len(pts))] * 2), 0.1)
