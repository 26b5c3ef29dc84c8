"""tests/raster_ref.py - the numpy restatement of the rasteriser's rule, which csrc/raster.hip must EQUAL - against facts that need
no restatement: pixel sets counted by hand, an exact depth, the tie order, the counters' sum, and an independent float64 ray-caster."""
import numpy as np

import raster_case as K
import raster_ref as R

F32 = np.float32


def _render(corners_px, H, W, **kw):
    pm = {k: kw.pop(k) for k in ("z", "f", "cx", "cy") if k in kw}
    v, f, intr = K.pixel_mesh(corners_px, **pm)
    return R.render_mesh(v, f, intr, K.IDENTITY, H, W, **kw)


def _pixels(mask):
    return {(int(x), int(y)) for y, x in zip(*np.nonzero(mask))}


def test_right_triangle_on_pixel_centres_covers_the_inclusive_triangle():
    """Corners on pixel centres, legs of 4 px: edges are inclusive, so the 15 lattice points of the closed triangle, no more."""
    out = _render([[[2, 3], [6, 3], [2, 7]]], 12, 12)
    want = {(x, y) for x in range(2, 7) for y in range(3, 8) if (x - 2) + (y - 3) <= 4}
    assert len(want) == 15 and _pixels(out["face"][0] == 0) == want
    assert out["info"] == dict(drawn=1, near=0, guard=0, empty=0, bad=0, pixels=15) and out["samples"] == 15
    # the other winding draws the same pixels
    assert _pixels(_render([[[2, 3], [2, 7], [6, 3]]], 12, 12)["face"][0] == 0) == want


def test_two_triangles_sharing_a_diagonal_cover_the_square_without_a_hole():
    """The diagonal pixels are drawn by both faces at the same depth and go to the lower face index, whichever triangle that is."""
    lower, upper = [[2, 2], [6, 2], [6, 6]], [[2, 2], [6, 6], [2, 6]]
    for tris in ([lower, upper], [upper, lower]):
        out = _render(tris, 9, 9)
        face = out["face"][0]
        assert _pixels(face >= 0) == {(x, y) for x in range(2, 7) for y in range(2, 7)}
        assert all(face[i, i] == 0 for i in range(2, 7))
        assert (face == 0).sum() == 15 and (face == 1).sum() == 10 and out["samples"] == 30 and out["info"]["pixels"] == 25


def test_camera_facing_rectangle_renders_its_exact_depth_on_the_analytic_pixel_set():
    """A rectangle u in [3.5, 20.25], v in [2.75, 10.5] at z_c = 2 with the principal point at (16, 8): wider than high and off
    centre, so a swapped axis, a flipped sign or a half-pixel shift of the pixel centres moves the set.  The pixel centres inside
    are ui = 4 .. 20, vi = 3 .. 10.  All q_i are 0.5 exactly, w0 q0 + w1 q1 + w2 q2 is |A| / 2 up to a few float64 roundings, and a
    value within 1e-15 relative of an fp32 number rounds to that number: depth == 2.0 exactly."""
    a, b, c, d = [3.5, 2.75], [20.25, 2.75], [20.25, 10.5], [3.5, 10.5]
    out = _render([[a, b, c], [a, c, d]], 16, 32, cx=16.0, cy=8.0)
    want = {(x, y) for x in range(4, 21) for y in range(3, 11)}
    assert _pixels(out["depth"][0] > 0) == want == _pixels(out["face"][0] >= 0)
    assert set(np.unique(out["depth"][0]).tolist()) == {0.0, 2.0}
    # vertices: corner a of face 0 is vertex 0 and lies top left; the pixel next to it reads it
    assert out["vertex"][0, 3, 4] in (0, 3) and out["vertex"][0, 3, 20] == 1 and out["vertex"][0, 10, 20] in (2, 4)


def test_the_nearer_face_wins_and_coincident_faces_go_to_the_lower_index():
    tri = [[1, 1], [9, 1], [1, 9]]
    near_v, near_f, intr = K.pixel_mesh([tri], z=1.0)
    far_v, _, _ = K.pixel_mesh([[[0, 0], [11, 0], [0, 11]]], z=2.0)                    # behind it and larger, listed FIRST
    v, f = np.concatenate([far_v, near_v]), np.arange(6, dtype=np.int32).reshape(2, 3)
    out = R.render_mesh(v, f, intr, K.IDENTITY, 12, 12)
    hit_near = R.render_mesh(near_v, near_f, intr, K.IDENTITY, 12, 12)["face"][0] >= 0
    hit_far = R.render_mesh(far_v, near_f, intr, K.IDENTITY, 12, 12)["face"][0] >= 0
    assert hit_near.sum() == 45 and (hit_far & ~hit_near).sum() == 78 - 45 and not (hit_near & ~hit_far).any()
    assert (out["face"][0][hit_near] == 1).all() and (out["depth"][0][hit_near] == 1.0).all()
    assert (out["face"][0][hit_far & ~hit_near] == 0).all() and (out["depth"][0][hit_far & ~hit_near] == 2.0).all()
    # coincident duplicates
    v2 = np.concatenate([near_v, near_v, near_v])
    f2 = np.arange(9, dtype=np.int32).reshape(3, 3)
    fwd = R.render_mesh(v2, f2, intr, K.IDENTITY, 12, 12)
    rev = R.render_mesh(v2, f2, intr, K.IDENTITY, 12, 12, reverse_ties=True)
    assert (fwd["face"][0][hit_near] == 0).all() and (rev["face"][0][hit_near] == 2).all()
    assert np.array_equal(fwd["depth"], rev["depth"]) and fwd["samples"] == 3 * hit_near.sum()


def test_vertex_is_the_corner_of_the_largest_weight_with_ties_to_the_lowest_corner():
    """Corners (0, 0), (8, 0), (0, 8): pixel (4, 4) lies on the middle of the edge v1 v2, w1 == w2 > w0 = 0 -> corner 1; pixel (2, 2)
    has w0 > w1 == w2; with corners (0, 0), (6, 0), (0, 6) pixel (2, 2) is the centroid: all three equal -> corner 0."""
    out = _render([[[0, 0], [8, 0], [0, 8]]], 10, 10)
    assert out["vertex"][0, 4, 4] == 1 and out["vertex"][0, 2, 2] == 0 and out["vertex"][0, 1, 6] == 1 and out["vertex"][0, 6, 1] == 2
    out = _render([[[0, 0], [6, 0], [0, 6]]], 10, 10)
    assert out["vertex"][0, 2, 2] == 0
    out = _render([[[6, 0], [0, 6], [0, 0]]], 10, 10)                                  # the same triangle, corner 0 elsewhere
    assert out["vertex"][0, 2, 2] == 0 and out["vertex"][0, 0, 5] == 0 and out["vertex"][0, 3, 3] == 0   # (3, 3): w0 == w1 > w2


def test_the_five_classes_sum_to_the_pairs_on_every_case():
    for c, out in ((K.soup(), K.soup_ref()), (K.room(), K.room_ref())):
        k, F = len(out["kept"]), len(c["faces"])
        assert sum(out["info"][n] for n in R.INFO[:5]) == k * F and out["classes"].shape == (k, F)
        assert out["info"]["pixels"] == (out["depth"] > 0).sum() <= out["samples"]
    s, r = K.soup_ref(), K.room_ref()
    assert list(s["kept"]) == [0, 2] and min(s["info"][n] for n in ("drawn", "near", "empty")) > 0
    assert r["info"]["drawn"] > 1000 and r["info"]["pixels"] > 10000
    # classes the random cases do not reach: a bad index, a NaN vertex, a vertex at the limit, a guard hit
    v = np.array([[0, 0, 1], [0.1, 0, 1], [0, 0.1, 1], [np.nan, 0, 1], [16384.0, 0, 1], [1000.0, 0, 1]], dtype=F32)
    f = np.array([[0, 1, 2], [0, 1, -1], [0, 1, 6], [0, 1, 3], [0, 1, 4], [0, 1, 5]], dtype=np.int32)
    out = R.render_mesh(v, f, np.array([[64, 64, 8, 8]], dtype=F32), K.IDENTITY, 16, 16)
    assert list(out["classes"][0]) == [R.DRAWN, R.BAD, R.BAD, R.BAD, R.BAD, R.GUARD]


def _ray_cast(c):
    """Moeller-Trumbore through the pixel centres in float64, in the camera frame of the fp32 world_to_cam -> (depth [H, W] with inf
    where nothing is hit, face [H, W], the projected corners [F, 3, 2] in pixels, the camera-space z of the corners [F, 3])."""
    w2c, _ = R.world_to_cam(c["poses"])
    m, k = w2c[0].astype(np.float64), c["intr"][0].astype(np.float64)
    p = c["vertices"].astype(np.float64)[c["faces"]] @ m[:, :3].T + m[:, 3]               # [F, 3, 3]
    vi, ui = np.mgrid[0:c["H"], 0:c["W"]]
    dirs = np.stack([(ui - k[2]) / k[0], (vi - k[3]) / k[1], np.ones(ui.shape)], axis=-1).reshape(-1, 1, 3)      # z = 1: t IS the z-depth
    e1, e2 = (p[:, 1] - p[:, 0])[None], (p[:, 2] - p[:, 0])[None]
    h = np.cross(dirs, e2)
    det = (e1 * h).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = -p[:, 0][None]
        u = (s * h).sum(-1) / det
        q = np.cross(s, e1)
        v = (dirs * q).sum(-1) / det
        t = (e2 * q).sum(-1) / det
    ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
    t = np.where(ok, t, np.inf)
    face = t.argmin(axis=1)
    depth = t[np.arange(len(t)), face]
    uv = np.stack([k[0] * p[..., 0] / p[..., 2] + k[2], k[1] * p[..., 1] / p[..., 2] + k[3]], axis=-1)
    return depth.reshape(ui.shape), np.where(np.isfinite(depth), face, -1).reshape(ui.shape), uv, p[..., 2]


def _segment_distance(px, a, b):
    """Distance of points px [n, 2] from segments a -> b [m, 2] -> [n, m]."""
    ab = (b - a)[None]
    ap = px[:, None, :] - a[None]
    s = np.clip((ap * ab).sum(-1) / (ab * ab).sum(-1), 0.0, 1.0)
    return np.linalg.norm(ap - s[..., None] * ab, axis=-1)


def test_agrees_with_an_independent_ray_caster_away_from_the_edges():
    """On pixels whose centre lies more than one pixel from every projected edge of the mesh the face must be the ray-caster's, and
    the depth must lie within a bound that holds no fitted constant:

    The rasteriser differs from the exact projection by moving every corner on the screen: the snap by at most half a step,
    1/512 px per axis, and the fp32 rounding of u and v (three operations on values below 2^8 px) by less than 2^-14 px; together
    delta = 1/512 + 2^-14 per axis, delta sqrt(2) in length.  1/z is affine on the screen, g(P).  The rasteriser's interpolant g' is
    the affine function that takes the corners' 1/z at the MOVED corners, so h = g' - g is affine with |h| <= |grad g| delta sqrt(2) at
    the moved corners and hence everywhere inside the moved triangle.  With q the corners' 1/z, grad g = (1 / 2A) sum (q_i - q_min) n_i
    with n_i the opposite edge turned by 90 degrees (|n_i| = the edge's length; the n_i sum to zero, so q_min may be subtracted); one
    term vanishes, the other two are at most (q_max - q_min) l_max each, and 2A / l_max is the smallest altitude h_min:
    |grad g| <= 2 (q_max - q_min) / h_min.  A pixel more than a pixel inside lies in both triangles, where d and z are within
    [z_min, z_max]: |d - z| = d z |1/d - 1/z| <= z_max^2 * 2 sqrt(2) delta (q_max - q_min) / h_min.
    To that comes the fp32 rounding of the camera-space corners (four operations on terms that sum below 16 m: 2^-18 m per corner,
    which moves d by at most (z_max / z_min)^2 times as much) and of d itself (2^-24 z_max)."""
    c = K.random_mesh()
    out = R.render_mesh(c["vertices"], c["faces"], c["intr"], c["poses"], c["H"], c["W"])
    depth, face, uv, zc = _ray_cast(c)
    vi, ui = np.mgrid[0:c["H"], 0:c["W"]]
    px = np.stack([ui, vi], axis=-1).reshape(-1, 2).astype(np.float64)
    a, b = uv.reshape(-1, 2), np.roll(uv, -1, axis=1).reshape(-1, 2)
    far_from_edges = (_segment_distance(px, a, b).min(axis=1) > 1.0).reshape(ui.shape)
    hit = out["face"][0] >= 0
    compared = hit & far_from_edges
    assert compared.sum() >= 0.5 * hit.sum() and compared.sum() > 1500, (compared.sum(), hit.sum())
    assert np.array_equal(out["face"][0][compared], face[compared])
    edges = np.linalg.norm(uv - np.roll(uv, -1, axis=1), axis=-1)                      # [F, 3]
    e1, e2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
    area2 = np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])
    h_min = area2 / edges.max(axis=1)
    assert edges.min() >= 6.0
    zmin, zmax = zc.min(axis=1), zc.max(axis=1)
    delta = 1.0 / 512 + 2.0 ** -14
    bound = zmax ** 2 * 2 * np.sqrt(2) * delta * (1 / zmin - 1 / zmax) / h_min + 2.0 ** -18 * (zmax / zmin) ** 2 + 2.0 ** -24 * zmax
    err = np.abs(out["depth"][0].astype(np.float64) - depth)[compared]
    assert (err <= bound[face[compared]]).all(), (err / bound[face[compared]]).max()
    assert err.max() > 0 and bound[face[compared]].max() < 0.02                        # the bound means something
