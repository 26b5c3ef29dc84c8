"""The numpy restatement of the point-cloud superpoint rules (tests/point_superpoints_ref.py) on cases whose answer is known without it,
and the argument checks of the public functions, which need no device."""
import numpy as np
import pytest

import point_superpoints_case as C
import point_superpoints_ref as P
import superpoints_case as K
import superpoints_ref as R

F32 = np.float32


def _full_matrix_knn(p, k, radius):
    """Rule a by a Python sort of every row of the full distance matrix, with float() arithmetic rounded through float32 by hand."""
    p = np.asarray(p, dtype=F32)
    r2 = F32(F32(radius) * F32(radius))
    valid = [bool(np.all(np.isfinite(x)) and np.all(np.abs(x) < 16384)) for x in p]
    nbr = np.full((len(p), k), -1, dtype=np.int32)
    d2s = np.full((len(p), k), np.inf, dtype=F32)
    for i in range(len(p)):
        row = []
        for j in range(len(p)):
            if i == j or not (valid[i] and valid[j]):
                continue
            dx, dy, dz = F32(p[j, 0] - p[i, 0]), F32(p[j, 1] - p[i, 1]), F32(p[j, 2] - p[i, 2])
            d2 = F32(F32(F32(dx * dx) + F32(dy * dy)) + F32(dz * dz))
            if d2 <= r2:
                row.append((int(np.asarray(d2, dtype=F32).view(np.uint32)), j, d2))
        for s, (_, j, d2) in enumerate(sorted(row)[:k]):
            nbr[i, s], d2s[i, s] = j, d2
    return nbr, d2s


@pytest.mark.parametrize("name,k,radius", [("dup", 5, 0.1), ("lattice", 5, 0.125), ("lattice", 16, 0.125), ("bad", 7, 0.2), ("line", 3, 0.05),
                                           ("two", 4, 1.0), ("far", 3, 0.01)])
def test_brute_force_knn_equals_a_sort_of_the_full_matrix(name, k, radius):
    p = {"dup": C.duplicates(20), "lattice": C.lattice(4, 4, 3, 0.125), "bad": C.with_bad_rows(6, 120), "line": C.collinear(8, 20),
         "two": np.array([[0, 0, 0], [0.5, 0, 0]], dtype=F32), "far": C.uniform_cube(30, 1)}[name]
    nbr, d2 = P.knn_graph(p, k, radius, chunk=7)
    want_nbr, want_d2 = _full_matrix_knn(p, k, radius)
    assert np.array_equal(nbr, want_nbr)
    assert np.array_equal(d2.view(np.uint32), want_d2.view(np.uint32))
    if name == "dup":
        assert (d2[:20, :5] == 0).all() and nbr[0].tolist() == [1, 2, 3, 4, 5]        # duplicates are neighbours at d2 = 0, lowest index first
    if name == "far":
        assert (nbr == -1).all() and np.isinf(d2).all()
    if name == "bad":
        assert (nbr[[7, 40, 77, 100, 101]] == -1).all() and not np.isin(nbr, [7, 40, 77, 100, 101]).any()
    if name == "lattice":
        assert (d2[nbr >= 0] == F32(0.125) * F32(0.125)).all()                        # d2 == r2 exactly: on the boundary, and inside


def test_empty_and_tiny_clouds():
    for n in (0, 1, 2):
        nbr, d2 = P.knn_graph(np.zeros((n, 3), dtype=F32) + np.arange(n, dtype=F32)[:, None] * F32(0.01), 4, 0.1)
        assert nbr.shape == (n, 4) and ((nbr >= 0).sum(axis=1) == max(n - 1, 0)).all()
        r = P.point_superpoints(np.zeros((n, 3), dtype=F32), k=4)
        assert r.count == min(n, 1) and r.bad_edges == 4 * n - (2 if n == 2 else 0) and not r.labels.any()      # pass 2 joins the pair


def test_flat_grid_is_one_superpoint():
    r = P.point_superpoints(K.flat_grid(20)[0])
    assert r.count == 1 and not r.labels.any()


def test_right_angle_crease_splits_two_sheets():
    r = P.point_superpoints(K.crease(8, 8)[0])
    lab = r.labels.reshape(15, 8)
    assert r.count == 2
    assert (lab[:7] == 0).all() and (lab[9:] == 1).all()
    assert np.isin(lab[7:9], [0, 1]).all()


def test_knn_tie_order_matters_on_a_regular_lattice():
    """Rule a: among equal distances the lower index goes first.  With 6 neighbours at d2 == r2 and k = 5, which one is left out is
    decided by the tie order alone."""
    p = C.lattice(16, 16, 4, 0.125)
    nbr, d2 = P.knn_graph(p, 5, 0.125)
    rev, d2r = P.knn_graph(p, 5, 0.125, reverse_ties=True)
    assert np.array_equal(d2.view(np.uint32), d2r.view(np.uint32))
    inner = (nbr >= 0).all(axis=1) & (rev >= 0).all(axis=1)
    assert inner.sum() > 300
    assert any(set(a) != set(b) for a, b in zip(nbr[inner].tolist(), rev[inner].tolist()))


def test_edge_tie_order_matters_on_the_noise_free_cloud():
    p = C.mesh_vertices("boxes_on_plane", 40, 1)
    nbr, _ = P.knn_graph(p, 16, 0.1)
    normals = P.estimate_normals(p, nbr)
    r = P.graph_superpoints(p, normals, P.knn_edges(nbr), oriented=False, debug=True)
    assert len(np.unique(r.weights)) < len(r.weights) // 100                          # nearly every edge ties with another
    rev = P.graph_superpoints(p, normals, P.knn_edges(nbr), oriented=False, reverse_ties=True)
    assert not np.array_equal(r.labels, rev.labels)


def test_jacobi_normals_on_exact_planes_and_against_eigh():
    """Dyadic points on three planes: the moments are exact, the covariance has an exact null vector, and the normal must be the
    plane's up to sign - exactly for the axis planes, to float32 rounding for the diagonal one.  Then, on planes in general position
    as well, the float64 eigenvector against numpy.linalg.eigh.

    The bound.  Both cyclic Jacobi (24 rotations) and LAPACK return the eigenvectors of A + E with |E| <= c eps |A|, c a small multiple
    of the number of rotations; an eigenvector moves by at most |E| / gap, gap = the distance from the smallest eigenvalue to the next.
    So the sine of the angle between the two is asserted <= 256 eps lambda_max / gap per point.  Measured maximum of sine / bound:
    0.0045 on the exact planes, 0.0077 on the planes in general position (sines 3.4e-16 and 6.9e-16)."""
    eps = np.finfo(np.float64).eps
    for name, (p, plane_normal) in (("exact", C.exact_planes()), ("general", C.planes())):
        nbr, _ = P.knn_graph(p, 16, 0.1)
        cov, c = P.moments(p, nbr)
        assert (c >= 3).all()
        diag, vec = P.jacobi(cov)
        got = P.smallest_column(diag, vec)
        a = np.zeros((len(p), 3, 3))
        for t, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            a[:, i, j] = a[:, j, i] = cov[:, t]
        lam, v = np.linalg.eigh(a)
        sine = np.linalg.norm(np.cross(got, v[:, :, 0]), axis=1)
        bound = 256 * eps * lam[:, 2] / (lam[:, 1] - lam[:, 0])
        print(f"{name}: max sine {sine.max():.3e}, max sine / bound {(sine / bound).max():.4f}")
        assert (sine <= bound).all()
        est = P.estimate_normals(p, nbr)
        assert np.allclose(np.linalg.norm(est.astype(np.float64), axis=1), 1.0, atol=1e-6)
        assert ((est[:, 0] > 0) | ((est[:, 0] == 0) & ((est[:, 1] > 0) | ((est[:, 1] == 0) & (est[:, 2] > 0))))).all()     # the canonical sign
        dot = np.abs((est.astype(np.float64) * plane_normal).sum(axis=1))
        if name == "exact":
            assert np.array_equal(est[:81], np.tile(F32([0, 0, 1]), (81, 1))) and np.array_equal(est[81:162], np.tile(F32([1, 0, 0]), (81, 1)))
            assert (dot >= 1 - 2.0 ** -22).all()
        else:
            assert (np.abs(dot - 1) <= 1e-6).all()             # float32 roundings of the planes' points, and a float32 normal (2^-24 per component)


def test_normals_of_thin_rows_and_collinear_points():
    p = C.collinear()
    nbr, _ = P.knn_graph(p, 6, 0.1)
    est = P.estimate_normals(p, nbr)
    assert not est[-3:].any()                                                         # 1, 1 and 0 neighbours
    assert not est[0].any() and not est[59].any()                                     # the ends of the line have 2
    line = np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0)
    assert (np.abs(est[1:59].astype(np.float64) @ line) < 1e-6).all()                 # rank 1: some unit vector across the line
    assert np.allclose(np.linalg.norm(est[1:59].astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_viewpoint_orients_the_normals():
    p, _ = C.exact_planes()
    nbr, _ = P.knn_graph(p, 16, 0.1)
    free = P.estimate_normals(p, nbr)
    for view in (np.array([0.0, 0.0, -5.0], dtype=F32), np.array([30.0, 30.0, 5.0], dtype=F32)):
        est = P.estimate_normals(p, nbr, view)
        assert np.array_equal(np.abs(est), np.abs(free))
        assert (((view[None, :] - p).astype(np.float64) * est).sum(axis=1) >= 0).all()
        per_point = P.estimate_normals(p, nbr, np.tile(view, (len(p), 1)))
        assert np.array_equal(per_point, est)


@pytest.mark.parametrize("mesh", [("crease", 8, 8), ("boxes_on_plane", 24, 5), ("height_field", 12, 6), ("boxes_on_plane", 40, 2)])
def test_graph_superpoints_on_a_mesh_equals_mesh_superpoints(mesh):
    """A mesh's own edges, in the mesh rule's order, and its vertex normals: the general edge list must give the mesh's result."""
    v, edges, f = C.mesh_graph(*mesh)
    want = R.mesh_superpoints(v, f, debug=True)
    got = P.graph_superpoints(v, want.normals, edges, oriented=True, debug=True)
    assert np.array_equal(got.weights, want.weights)
    assert np.array_equal(got.labels, want.labels) and got.count == want.count and got.bad_edges == 0


def test_bad_edges_are_counted_not_followed():
    v, edges, f = C.mesh_graph("flat_grid", 8)
    normals = R.vertex_normals(v, f)
    want = P.graph_superpoints(v, normals, edges)
    bad = np.array([[0, 64], [-1, 2], [5, 1 << 40], [64, 64]])
    got = P.graph_superpoints(v, normals, np.concatenate([bad[:1], edges, bad[1:]]), debug=True)
    assert got.bad_edges == 4 and want.bad_edges == 0
    assert np.array_equal(got.labels, want.labels)
    assert got.weights[0] == 0 and (got.weights[-3:] == 0).all()


def test_unoriented_weights_ignore_the_sign_of_a_normal():
    p = C.mesh_vertices("height_field", 20, 3)
    nbr, _ = P.knn_graph(p, 12, 0.12)
    normals = P.estimate_normals(p, nbr)
    flipped = normals * np.where(np.random.default_rng(0).random(len(p)) < 0.5, F32(-1), F32(1))[:, None]
    a = P.graph_superpoints(p, normals, P.knn_edges(nbr), oriented=False, debug=True)
    b = P.graph_superpoints(p, flipped, P.knn_edges(nbr), oriented=False, debug=True)
    assert np.array_equal(a.weights, b.weights) and np.array_equal(a.labels, b.labels)
    c = P.graph_superpoints(p, flipped, P.knn_edges(nbr), oriented=True, debug=True)
    assert not np.array_equal(a.weights, c.weights)


def test_missing_slots_are_the_bad_edges_of_the_composition():
    p = C.mesh_vertices("height_field", 20, 3)
    r = P.point_superpoints(p, k=16, radius=0.1, debug=True)
    assert r.bad_edges == int((r.nbr < 0).sum()) > 0
    assert np.array_equal(np.unique(r.labels), np.arange(r.count))


def test_argument_validation_of_the_public_functions():
    """The checks that need no device: wrong types, CPU tensors ("no CPU fallback") and parameters out of range."""
    import torch
    from segdino3d_amd import superpoints as S
    p = torch.zeros(10, 3)
    nbr = torch.zeros(10, 4, dtype=torch.int32)
    edges = torch.zeros(5, 2, dtype=torch.int64)
    for call in (lambda: S.knn_graph(p), lambda: S.estimate_normals(p, nbr), lambda: S.graph_superpoints(p, p, edges),
                 lambda: S.point_superpoints(p), lambda: S.point_superpoints_batch([p, p])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for call in (lambda: S.knn_graph(p.numpy()), lambda: S.estimate_normals(p.numpy(), nbr), lambda: S.graph_superpoints(p.numpy(), p, edges),
                 lambda: S.point_superpoints([[0.0, 0.0, 0.0]]), lambda: S.point_superpoints_batch([]), lambda: S.point_superpoints_batch([None])):
        with pytest.raises(ValueError):
            call()
    for k in (0, 65, -1, 2.5, True):
        with pytest.raises(ValueError, match="k must be"):
            S.knn_graph(p, k=k)
        with pytest.raises(ValueError, match="k must be"):
            S.point_superpoints(p, k=k)
    for radius in (0, -0.1, 4.5, float("nan"), float("inf"), "0.1"):
        with pytest.raises(ValueError, match="radius must be"):
            S.knn_graph(p, radius=radius)
        with pytest.raises(ValueError, match="radius must be"):
            S.point_superpoints_batch([p], radius=radius)
    for kw in (dict(k_thresh=-1.0), dict(k_thresh=float("nan")), dict(min_verts=0), dict(min_verts=2.5)):
        with pytest.raises(ValueError):
            S.graph_superpoints(p, p, edges, **kw)
        with pytest.raises(ValueError):
            S.point_superpoints(p, **kw)
    with pytest.raises(ValueError, match="one entry per cloud"):
        S.point_superpoints_batch([p, p], normals=[p])
