"""csrc/transfer.hip + segdino3d_amd/transfer.py against the numpy restatement tests/transfer_ref.py (the reference has no counterpart)
on the inputs of tests/transfer_case.py and a few hand-built ones.

Bounds.  None: indices, the BITS of d2, label images and instance maps must EQUAL the restatement.  Every decision of the rule is a
comparison of single rounded fp32 operations, and the answer is a minimum over a set of integer keys."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fuse_views_case as FK
import fuse_views_ref as FR
import transfer_case as K
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


def _check(p, q, r, d, labels=None, fill=-1, what=""):
    """The point form against the restatement: idx, the bits of d2 and the gathered labels -> the restatement's (idx, d2)."""
    from segdino3d_amd import transfer
    want_idx, want_d2 = T.nearest(p, q, r)
    index = transfer.PointIndex(_t(p, d), r)
    got = index.nearest(_t(q, d), labels=None if labels is None else _t(labels, d), fill=fill, return_d2=True)
    idx, d2 = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert idx.dtype == np.int32 and d2.dtype == F32 and idx.shape == d2.shape == (len(q),), what
    assert np.array_equal(idx, want_idx), (what, int((idx != want_idx).sum()))
    assert np.array_equal(_bits(d2), _bits(want_d2)), what
    if labels is not None:
        out = got[2].cpu().numpy()
        assert out.dtype == np.int32 and np.array_equal(out, T.take_labels(labels, want_idx, fill)), what
    return want_idx, want_d2


def _views(depth, scale, intr, poses, d):
    from segdino3d_amd import lift2d
    return lift2d.Views(_t(depth, d), _t(intr, d), poses, scale)


# ---------------------------------------------------------------------------------------------- sizes
def test_no_points_no_queries_one_point():
    from segdino3d_amd import transfer
    d = dev()
    q = np.array([[0.5, -0.25, 2.0], [0.0, 0.0, 0.0]], dtype=F32)
    idx, d2 = _check(np.zeros((0, 3), F32), q, 0.5, d, labels=np.zeros((2, 0), np.int32), fill=-7, what="N = 0")
    assert idx.tolist() == [-1, -1]
    _check(q, np.zeros((0, 3), F32), 0.5, d, labels=np.array([[4, 5]], np.int32), what="M = 0")
    idx, d2 = _check(q[:1], q[:1], 0.5, d, what="N = 1, the query on the point")
    assert idx.tolist() == [0] and d2.tolist() == [0.0]
    # [N, 6] clouds (xyz, rgb) and a single label row pass as they are
    index = transfer.PointIndex(torch.cat([_t(q, d), torch.full((2, 3), 1.0e9, device=d)], dim=1), 0.5)
    idx, out = index.nearest(_t(q[::-1].copy(), d), labels=torch.tensor([7, 9], device=d))
    assert idx.tolist() == [1, 0] and out.tolist() == [9, 7] and out.dtype == torch.int32


# ---------------------------------------------------------------------------------------------- the radius
@pytest.mark.parametrize("radius", [0.1, 0.125, 4.0, 2.0 ** -9])
def test_radius_boundary(radius):
    """A source point at squared distance exactly r2 is a hit, the next float beyond is a miss: along each axis, in both directions.
    Pair k is 50 away from the others and differs in one coordinate only, which is 0 for the query and +-r (or the next float) for the
    point, so dx is exact and d2 = fl(r r) = r2 (or the square of the next float, which lies above r2)."""
    d = dev()
    r = F32(radius)
    beyond = np.nextafter(r, F32(np.inf))
    r2 = F32(r * r)
    assert F32(beyond * beyond) > r2
    q = np.zeros((12, 3), F32)
    for k in range(12):
        q[k] = [50.0 * k, -50.0 * k, 50.0 * k - 300.0]
        q[k, k % 3] = 0.0
    p = q.copy()
    for k in range(12):
        p[k, k % 3] = (1 - 2 * ((k // 3) % 2)) * (r if k < 6 else beyond)
    idx, d2 = _check(p, q, radius, d, what=f"r = {radius}")
    assert idx.tolist() == list(range(6)) + [-1] * 6
    assert np.all(d2[:6] == r2) and np.all(np.isinf(d2[6:]))


# ---------------------------------------------------------------------------------------------- cells
def test_lattice_ties_and_cell_boundaries():
    d = dev()
    p, q, r = K.lattice_case()
    idx, d2 = _check(p, q, r, d, labels=K.labels_for(len(p), 3), what="lattice")
    assert (idx >= 0).sum() > 2000 and (d2 == F32(r) * F32(r)).sum() > 10 and (q < 0).any()
    assert (T.nearest(p, q, r, reverse_ties=True)[0] != idx).sum() > 100             # the ties are there, and the device broke them downwards


def test_agreement_case():
    d = dev()
    p, q, r = K.agreement_case()
    _check(p, q, r, d, what="uniform")


# ---------------------------------------------------------------------------------------------- validity
def test_duplicates_and_invalid_points():
    d = dev()
    rng = np.random.default_rng(5)
    p = rng.uniform(-1, 1, (300, 3)).astype(F32)
    p[100:200] = p[:100]                                                              # duplicated: the lower index wins
    p[250] = [np.nan, 0, 0]
    p[251] = [0, np.inf, 0]
    p[252] = [0, 0, -np.inf]
    p[253] = [16384.0, 0, 0]
    p[254] = [0, -16384.0, 0]
    p[255] = [16383.0, 16383.0, -16383.0]
    q = np.concatenate([p[100:260], rng.uniform(-1, 1, (100, 3)).astype(F32),
                        np.array([[16383.5, 16383.0, -16383.0], [16383.5, 0, 0], [np.nan, np.nan, np.nan], [0, 0, np.inf], [16384.0, 0, 0],
                                  [-16384.0, 0, 0], [3.0e38, 0, 0]], dtype=F32)])
    idx, d2 = _check(p, q, 0.75, d, labels=K.labels_for(len(p), 2), what="validity")
    assert np.array_equal(idx[:100], np.arange(100)) and np.all(d2[:100] == 0)
    assert idx[150:155].tolist() == [-1] * 5 and idx[155] == 255                      # invalid sources as queries; the corner point
    assert idx[260] == 255 and d2[260] == 0.25 and idx[261:].tolist() == [-1] * 6     # the query at 16383.5 is valid and finds the corner


# ---------------------------------------------------------------------------------------------- bucket shapes
def test_one_long_bucket():
    d = dev()
    rng = np.random.default_rng(6)
    p = rng.uniform(0.01, 0.09, (3000, 3)).astype(F32)                                # one cell of the grid at r = 0.1 (cells of 105 / 1024)
    q = rng.uniform(-0.1, 0.2, (500, 3)).astype(F32)
    idx, _ = _check(p, q, 0.1, d, what="one cell")
    assert 50 < (idx >= 0).sum() < 500


@pytest.mark.parametrize("N", [2048, 2049, 3000])
def test_scattered_points_share_buckets(N):
    """Far more cells than points share the buckets, on either side of the size at which the table doubles (2 N > 2^12)."""
    d = dev()
    rng = np.random.default_rng(N)
    p = rng.uniform(-8000, 8000, (N, 3)).astype(F32)
    q = (p[rng.integers(0, N, 2000)] + rng.uniform(-0.08, 0.08, (2000, 3)).astype(F32)).astype(F32)
    idx, _ = _check(p, q, 0.1, d, what=f"scattered {N}")
    assert 500 < (idx >= 0).sum() < 2000


# ---------------------------------------------------------------------------------------------- labels
@pytest.mark.parametrize("L", [1, 3, 8])
def test_label_channels(L):
    from segdino3d_amd import transfer
    d = dev()
    p, q, r = K.agreement_case()
    p, q = p[:1000], q[:1500]
    lab = K.labels_for(len(p), L, seed=L)
    assert (lab == -1).any()
    idx, _ = _check(p, q, 2 * r, d, labels=lab, fill=-7, what=f"L = {L}")
    assert (idx < 0).any() and (idx >= 0).any()
    index = transfer.PointIndex(_t(p, d), 2 * r)
    for dtype, values in ((torch.int64, lab.astype(np.int64)), (torch.bool, lab > 10), (torch.uint8, (lab & 0xFF).astype(np.uint8))):
        got = index.nearest(_t(q, d), labels=_t(values, d).to(dtype), fill=-7)[1]
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), T.take_labels(values, idx, -7)), dtype
    one = transfer.transfer_labels(_t(p, d), _t(lab[0], d), _t(q, d), 2 * r)
    assert tuple(one.shape) == (len(q),) and np.array_equal(one.cpu().numpy(), T.take_labels(lab[0], idx))


# ---------------------------------------------------------------------------------------------- the pixel form
def _pixel_check(index, views, ref_points, depth, scale, intr, c2w, r, d, labels=None, fill=-1, what="", **rule):
    want_idx, want_d2 = T.nearest_pixels(ref_points, depth, scale, intr, c2w, r, **rule)
    got = index.nearest_pixels(views, labels=None if labels is None else _t(labels, d), fill=fill, return_d2=True, **rule)
    idx, d2 = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert idx.shape == d2.shape == depth.shape and idx.dtype == np.int32, what
    assert np.array_equal(idx, want_idx), (what, int((idx != want_idx).sum()))
    assert np.array_equal(_bits(d2), _bits(want_d2)), what
    if labels is not None:
        assert np.array_equal(got[2].cpu().numpy(), T.take_labels(labels, want_idx, fill)), what
    return want_idx


@functools.lru_cache(maxsize=None)
def _noisy_cloud():
    c = K.broken_pose_case("u16")
    fused = FR.fuse_kept(c["depth"][c["kept"]], c["scale"], c["intr"][c["kept"]], c["c2w"], FK.noisy(24, 32, V=3)["colors"][c["kept"]],
                         voxel=0.05, min_obs=1, edge_rel=None)
    pts = np.ascontiguousarray(fused["points"][:, :3])
    pts.setflags(write=False)
    return pts


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_pixels_of_small_views_with_a_dropped_pose(kind):
    from segdino3d_amd import transfer
    d = dev()
    c, pts = K.broken_pose_case(kind), _noisy_cloud()
    views = _views(c["depth"], c["scale"], c["intr"], c["poses"], d)
    assert views.n_given == 3 and views.kept.tolist() == [0, 2]
    kd, ki = c["depth"][c["kept"]], c["intr"][c["kept"]]
    index = transfer.PointIndex(_t(pts, d), 0.1)
    lab = K.labels_for(len(pts), 3, seed=9)
    first = idx = _pixel_check(index, views, pts, kd, c["scale"], ki, c["c2w"], 0.1, d, labels=lab, fill=-7, what=kind)
    holes = kd == 0
    assert holes.any() and np.all(idx[holes] == -1) and np.all(idx[~holes] >= 0)     # every pixel with depth made a cell of this cloud
    idx = _pixel_check(index, views, pts, kd, c["scale"], ki, c["c2w"], 0.1, d, what=kind + " far", near=0.95, far=1.2)
    metres = FR.depth_metres(kd, c["scale"])
    assert np.all(idx[metres > F32(1.2)] == -1) and np.all(idx[metres < F32(0.95)] == -1) and (idx >= 0).any()
    one = transfer.render_labels(views, _t(pts, d), _t(lab[1], d), 0.1)
    assert tuple(one.shape) == kd.shape and np.array_equal(one.cpu().numpy(), T.take_labels(lab[1], first))


@pytest.mark.parametrize("n_points", [1000, 4000])
def test_pixels_against_a_dense_cloud(n_points):
    """A wall seen from 1 m with r = 0.5: the box of a tile has a few dozen cells; 1 000 points fit the tile's on-chip copy and
    4 000 do not, so the two counts take the two paths that read bucket ranges from the tile's table.  Odd image extents: partial
    tiles in both directions, more than one tile per row."""
    from segdino3d_amd import transfer
    d = dev()
    c = FK.wall(11, 45, 1.0, V=2)
    rng = np.random.default_rng(n_points)
    pts = np.stack([rng.uniform(0.6, 1.4, n_points), rng.uniform(-0.9, 0.9, n_points), rng.uniform(-0.6, 0.6, n_points)], axis=1).astype(F32)
    c2w, kept = FR.cam_to_world(c["poses"])
    views = _views(c["depth_u16"], FK.DEPTH_SCALE, c["intr"], c["poses"], d)
    idx = _pixel_check(transfer.PointIndex(_t(pts, d), 0.5), views, pts, c["depth_u16"], FK.DEPTH_SCALE, c["intr"], c2w, 0.5, d,
                       labels=K.labels_for(n_points, 1), what=f"wall {n_points}")
    assert np.all(idx >= 0)


@functools.lru_cache(maxsize=None)
def _room_reference(r=0.1):
    pts, _ = K.room_cloud(0.05)
    depth, intr, c2w = K.room_views()
    idx, d2 = T.nearest_pixels(pts, depth, FK.DEPTH_SCALE, intr, c2w, r)
    idx.setflags(write=False)
    d2.setflags(write=False)
    return idx, d2


def _room(d):
    """The room's views, the cloud `fuse_views` makes of them on the device, its counters, and the restatement's cloud."""
    from segdino3d_amd import fuse_views as fuse
    c = FK.room_case()
    views = _views(c["depth_u16"], FK.DEPTH_SCALE, c["intr"], c["poses"], d)
    points, info = fuse.fuse_views(views, _t(c["colors"], d), voxel=0.05, capacity=1 << 18, min_obs=1, edge_rel=None, return_info=True)
    return c, views, points, info


def test_room_against_its_own_cloud():
    from segdino3d_amd import transfer
    d = dev()
    c, views, points, info = _room(d)
    pts, fused = K.room_cloud(0.05)
    assert np.array_equal(_bits(points[:, :3].cpu().numpy()), _bits(pts))             # the cloud the restatement searched
    want_idx, want_d2 = _room_reference()
    lab = K.labels_for(len(pts), 2, seed=11)
    idx, d2, out = transfer.PointIndex(points, 0.1).nearest_pixels(views, labels=_t(lab, d), return_d2=True)
    idx = idx.cpu().numpy()
    assert np.array_equal(idx, want_idx) and np.array_equal(_bits(d2.cpu().numpy()), _bits(want_d2))
    assert np.array_equal(out.cpu().numpy(), T.take_labels(lab, want_idx))
    # coverage: no -1 where fuse_views counted a used pixel (no edge test, nothing out of range: every pixel with a valid depth)
    valid = T.pixel_queries(*((c["depth_u16"], FK.DEPTH_SCALE) + K.room_views()[1:]))[1]
    assert info.out_of_range == 0 and info.pixels_used == int(valid.sum()) > 100000
    assert int((idx[valid] < 0).sum()) == 0 and np.all(idx[~valid] == -1)


def test_cuts_streams_and_a_second_index_give_the_same_bits():
    from segdino3d_amd import transfer
    d = dev()
    c, views, points, info = _room(d)
    lab = _t(K.labels_for(points.shape[0], 3, seed=12), d)
    index = transfer.PointIndex(points, 0.1)
    whole = index.nearest_pixels(views, labels=lab, return_d2=True)

    def part(ix, sel):
        v = _views(c["depth_u16"][sel], FK.DEPTH_SCALE, c["intr"][sel], c["poses"][sel], d)
        return ix.nearest_pixels(v, labels=lab, return_d2=True)

    def same(parts, what):
        for k, (a, dim) in enumerate(zip(whole, (0, 0, 1))):
            b = torch.cat([p[k] for p in parts], dim=dim)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (what, k)

    same([part(index, slice(0, 3)), part(index, slice(3, 8))], "3 + 5")
    other = transfer.PointIndex(points.clone(), 0.1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        singles = [part(other, slice(i, i + 1)) for i in range(8)]
    torch.cuda.current_stream().wait_stream(side)
    same(singles, "one by one, a second stream, a second index")
    q = points[::7, :3].contiguous() + 0.01
    a, b = index.nearest(q, return_d2=True), other.nearest(q, return_d2=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_no_views_on_the_device():
    from segdino3d_amd import lift2d, transfer
    d = dev()
    none = lift2d.Views(torch.zeros(0, 4, 6, dtype=torch.uint16).to(d), np.zeros((0, 4), F32), np.zeros((0, 4, 4)), FK.DEPTH_SCALE)
    index = transfer.PointIndex(torch.zeros(5, 3, device=d), 0.1)
    idx, out = index.nearest_pixels(none, labels=torch.zeros(2, 5, dtype=torch.int32, device=d))
    assert tuple(idx.shape) == (0, 4, 6) and tuple(out.shape) == (2, 0, 4, 6) and idx.is_cuda and out.dtype == torch.int32


# ---------------------------------------------------------------------------------------------- instance map
@pytest.mark.parametrize("I,N", [(0, 10), (1, 1), (1, 1000), (70, 1000), (70, 1003), (5, 3)])
def test_instance_map(I, N):
    from segdino3d_amd import transfer
    d = dev()
    rng = np.random.default_rng(I * 10000 + N)
    masks = rng.random((I, N)) < 0.15
    scores = np.round(rng.random(I), 1).astype(F32)                                   # one decimal: equal scores among 70
    if I >= 5:
        scores[3] = np.nan
        masks[3] = True                                                               # the NaN covers every point and never wins
        scores[4] = scores[1] = 2.0                                                   # the two best, equal
        masks[4] |= masks[1]                                                          # an exact tie on shared points: the lower i
        masks[1, 0] = masks[4, 0] = True
        masks[4, -1], masks[1, -1] = True, False
    for thr in ((0.0, F32(0.5), 0.55, 2.0, 2.5) if I else (0.0,)):                    # 0.5 and 2.0 are exactly scores
        want = T.instance_map(masks, scores, thr)
        for m in (masks, masks.astype(np.uint8) * 3):                                 # bool, and uint8 where non-zero = set
            got = transfer.instance_map(_t(m, d), _t(scores, d), float(thr))
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (I, N, thr)
    if I >= 5:
        want = T.instance_map(masks, scores, 0.0)
        assert not (want == 3).any() and np.all(want[masks[1]] == 1) and masks[1].any() and want[-1] == 4
        assert np.array_equal(T.instance_map(masks, scores, 2.0), np.where(masks[1], 1, np.where(masks[4], 4, -1)))
        got = transfer.instance_map(_t(masks, d)[:, 1:], _t(scores, d))               # a view that is not contiguous, not 4-byte aligned
        assert np.array_equal(got.cpu().numpy(), T.instance_map(masks[:, 1:], scores))


# ---------------------------------------------------------------------------------------------- a forward's result, and a consumer
@pytest.mark.parametrize("container", ["dict", "object", "output"])
def test_render_prediction(container):
    from segdino3d_amd import transfer
    d = dev()
    c, pts = K.broken_pose_case("u16"), _noisy_cloud()
    host = K.prediction_case(len(pts))
    pred = {k: ([_t(x, d) for x in v] if isinstance(v, list) else _t(v, d)) for k, v in host.items()}
    if container != "dict":
        pred = SimpleNamespace(**pred)
    if container == "output":
        pred = SimpleNamespace(pred_pts_seg=pred)
    views = _views(c["depth"], c["scale"], c["intr"], c["poses"], d)
    kd, ki = c["depth"][c["kept"]], c["intr"][c["kept"]]
    for thr, fill in ((0.0, -1), (0.5, -3)):
        got = transfer.render_prediction(views, _t(np.concatenate([pts, np.zeros_like(pts)], axis=1), d), pred, 0.1, score_thr=thr, fill=fill)
        want = T.render_prediction(pts, host, kd, c["scale"], ki, c["c2w"], 0.1, score_thr=thr, fill=fill)
        assert tuple(got) == transfer.PREDICTION_IMAGES == tuple(want)
        for name in want:
            assert got[name].dtype == torch.int32 and np.array_equal(got[name].cpu().numpy(), want[name]), (name, thr)
    assert (want["instance"] >= 0).any() and (want["instance"] == -3).any()


def test_transferred_masks_feed_the_submission_text():
    """Instance masks carried from the points of a forward onto a scan's vertices go into submission's mask text as they come."""
    import io
    from segdino3d_amd import submission, transfer
    d = dev()
    rng = np.random.default_rng(21)
    src = rng.uniform(-1, 1, (400, 3)).astype(F32)
    dst = (src[rng.integers(0, 400, 90)] + rng.uniform(-0.05, 0.05, (90, 3))).astype(F32)
    dst[:5] += 5.0                                                                    # vertices the forward never saw: no point in reach
    masks = rng.random((6, 400)) < 0.3
    got = transfer.transfer_labels(_t(src, d), _t(masks, d), _t(dst, d), 0.1, fill=0)
    want = T.take_labels(masks, T.nearest(src, dst, 0.1)[0], fill=0)
    assert np.array_equal(got.cpu().numpy(), want) and not want[:, :5].any() and want.any()
    fmt = submission.DeviceFormatter()
    text = fmt.mask_text(fmt.masks(got), 0, 6).cpu().numpy()
    for i in range(6):
        f = io.BytesIO()
        np.savetxt(f, want[i], fmt="%d")
        assert text[i, :2 * 90].tobytes() == f.getvalue(), i
