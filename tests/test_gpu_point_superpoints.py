"""The point-cloud kernels of csrc/superpoints.hip + `segdino3d_amd.superpoints` against the restatement tests/point_superpoints_ref.py.

No tolerance anywhere: neighbours, the bits of their squared distances, the bits of the normals and of the edge weights, labels,
`count` and `bad_edges` must EQUAL the restatement.  Brute force stays at N <= 8192."""
import functools

import numpy as np
import pytest
import torch

import point_superpoints_case as C
import point_superpoints_ref as P
import superpoints_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _tiny(n):
    return (np.arange(3 * n, dtype=F32).reshape(n, 3) * F32(0.01)).astype(F32)


CLOUDS = {
    "n0": lambda: _tiny(0), "n1": lambda: _tiny(1), "n2": lambda: _tiny(2), "n5": lambda: _tiny(5), "n16": lambda: C.uniform_cube(16, 2, 0.0, 0.05),
    "lattice": lambda: C.lattice(16, 16, 4, 0.125), "dup": lambda: C.duplicates(300), "crowded": C.crowded_cell, "straddle": C.straddling,
    "limit": C.near_limit, "bad": C.with_bad_rows, "cube": lambda: C.uniform_cube(4096, 11), "cube_b": lambda: C.uniform_cube(1500, 12, 0.2, 0.9),
    "planes": lambda: C.planes()[0], "exact_planes": lambda: C.exact_planes()[0], "line": C.collinear,
    "boxes": lambda: C.mesh_vertices("boxes_on_plane", 40, 1), "field": lambda: C.mesh_vertices("height_field", 40, 1),
    "field_s": lambda: C.mesh_vertices("height_field", 20, 3),
}


@functools.lru_cache(maxsize=None)
def cloud(name):
    """The shared clouds, built once and never written to."""
    p = np.ascontiguousarray(CLOUDS[name](), dtype=F32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def ref_knn(name, k, radius):
    nbr, d2 = P.knn_graph(cloud(name), k, radius)
    nbr.setflags(write=False)
    d2.setflags(write=False)
    return nbr, d2


@functools.lru_cache(maxsize=None)
def ref_points(name, mode, k=16, radius=0.1):
    p = cloud(name)
    kw = {}
    if mode == "given":
        kw["normals"] = given_normals(name)
    elif mode == "view":
        kw["viewpoint"] = VIEW
    return P.point_superpoints(p, k=k, radius=radius, debug=True, **kw)


VIEW = np.array([0.7, 0.9, 4.0], dtype=F32)


@functools.lru_cache(maxsize=None)
def given_normals(name):
    rng = np.random.default_rng(5)
    n = rng.normal(size=(len(cloud(name)), 3)) * 0.05 + np.array([0.0, 0.0, 1.0])
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)
    n.setflags(write=False)
    return n


def _t(a, d):
    return torch.from_numpy(np.array(a)).to(d)


def _check_knn(name, k, radius, d):
    from segdino3d_amd import superpoints
    want_nbr, want_d2 = ref_knn(name, k, radius)
    nbr, d2 = superpoints.knn_graph(_t(cloud(name), d), k=k, radius=radius, return_d2=True)
    assert nbr.dtype == torch.int32 and d2.dtype == torch.float32 and nbr.is_cuda and tuple(nbr.shape) == tuple(d2.shape) == (len(cloud(name)), k)
    got_nbr, got_d2 = nbr.cpu().numpy(), d2.cpu().numpy()
    nd, dd = int((got_nbr != want_nbr).sum()), int((got_d2.view(np.uint32) != want_d2.view(np.uint32)).sum())
    print(f"{name} k {k} r {radius}: N {len(want_nbr)}, slots filled {int((want_nbr >= 0).sum())}, neighbours differing {nd}, d2 bits differing {dd}")
    assert nd == 0 and dd == 0
    assert torch.equal(superpoints.knn_graph(_t(cloud(name), d), k=k, radius=radius), nbr)
    return want_nbr, want_d2


@pytest.mark.parametrize("name,k,radius", [
    ("n0", 4, 0.1), ("n1", 4, 0.1), ("n2", 4, 0.1), ("n5", 5, 0.5), ("n16", 16, 0.2), ("n16", 33, 0.2),
    ("lattice", 5, 0.125), ("lattice", 16, 0.125), ("dup", 16, 0.1), ("dup", 64, 0.001), ("crowded", 16, 0.1), ("crowded", 64, 0.1),
    ("straddle", 16, 0.1), ("straddle", 5, 0.1025), ("limit", 16, 0.1), ("limit", 33, 4.0), ("cube", 16, 1e-4), ("bad", 16, 0.1),
    ("cube", 1, 0.1), ("cube", 5, 0.1), ("cube", 16, 0.1), ("cube", 33, 0.1), ("cube", 64, 0.1), ("cube", 64, 0.3)])
def test_knn_equals_brute_force(name, k, radius):
    d = dev()
    nbr, d2 = _check_knn(name, k, radius, d)
    if name == "lattice":
        assert (d2[nbr >= 0] == F32(0.125) * F32(0.125)).all() and (nbr[:, :3] >= 0).all()          # every neighbour sits at d2 == r2
    if name == "dup":
        assert (nbr[:300] >= 0).all() and (d2[:300, :min(k, 16)] == 0).all()
    if (name, radius) == ("cube", 1e-4):
        assert (nbr == -1).all() and np.isinf(d2).all()
    if name == "bad":
        assert (nbr[[7, 40, 77, 100, 101, 499]] == -1).all() and not np.isin(nbr, [7, 40, 77, 100, 101, 499]).any()
    if name == "limit":
        assert (nbr[:2] == -1).all() and (nbr[2:] >= 0).any()
    if name == "crowded" and k == 64:
        assert ((nbr >= 0).sum(axis=1) == 64).sum() >= 700


def test_knn_batch_of_interpenetrating_scenes():
    """Two clouds that fill the same space, an empty one and a tiny one in one launch chain: no neighbour crosses a scene (indices
    are local and each scene EQUALS its single run, which a foreign neighbour would break), wherever the scene stands."""
    from segdino3d_amd import ops
    d = dev()
    names = ["cube", "n0", "cube_b", "n2", "straddle"]
    for order in ((0, 1, 2, 3, 4), (2, 4, 0, 3, 1)):
        clouds = [cloud(names[i]) for i in order]
        off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
        nbr, d2 = ops.knn_graph(_t(np.concatenate(clouds), d), _t(off, d), 16, 0.1, return_d2=True)
        for slot, i in enumerate(order):
            want_nbr, want_d2 = ref_knn(names[i], 16, 0.1)
            assert np.array_equal(nbr[off[slot]:off[slot + 1]].cpu().numpy(), want_nbr), names[i]
            assert np.array_equal(d2[off[slot]:off[slot + 1]].cpu().numpy().view(np.uint32), want_d2.view(np.uint32)), names[i]


def test_knn_other_stream_and_reused_workspace_give_the_same_bits():
    from segdino3d_amd import superpoints
    d = dev()
    p, big = _t(cloud("straddle"), d), _t(cloud("cube"), d)
    first = superpoints.knn_graph(p, return_d2=True)
    other = superpoints.knn_graph(big, k=5)                                           # a larger cloud through the same workspace
    again = superpoints.knn_graph(p, return_d2=True)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1].view(torch.int32), again[1].view(torch.int32))
    assert np.array_equal(other.cpu().numpy(), ref_knn("cube", 5, 0.1)[0])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        streamed = superpoints.knn_graph(p, return_d2=True)
    s.synchronize()
    assert torch.equal(first[0], streamed[0]) and torch.equal(first[1].view(torch.int32), streamed[1].view(torch.int32))
    assert np.array_equal(first[0].cpu().numpy(), ref_knn("straddle", 16, 0.1)[0])


# ---------------------------------------------------------------------------------------------- normals
def _check_normals(name, k, radius, d, viewpoint=None):
    from segdino3d_amd import superpoints
    p = cloud(name)
    nbr, _ = ref_knn(name, k, radius)
    want = P.estimate_normals(p, nbr, viewpoint)
    got = superpoints.estimate_normals(_t(p, d), _t(nbr, d), None if viewpoint is None else _t(viewpoint, d))
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(p), 3)
    diff = int((got.cpu().numpy().view(np.uint32) != want.view(np.uint32)).sum())
    print(f"{name} k {k}: N {len(p)}, zero normals {int((~want.any(axis=1)).sum())}, components differing in their bits {diff}")
    assert diff == 0
    return want


@pytest.mark.parametrize("name,k,radius", [("planes", 16, 0.1), ("exact_planes", 16, 0.1), ("line", 6, 0.1), ("field", 16, 0.1), ("boxes", 16, 0.1),
                                           ("cube", 64, 0.3), ("bad", 16, 0.1), ("n2", 4, 0.1), ("n5", 5, 0.5), ("dup", 16, 0.1), ("limit", 33, 4.0)])
def test_normals_equal_the_restatement(name, k, radius):
    d = dev()
    want = _check_normals(name, k, radius, d)
    first = np.where(want[:, 0] != 0, want[:, 0], np.where(want[:, 1] != 0, want[:, 1], want[:, 2]))
    assert (first >= 0).all()                                                         # the canonical sign
    if name == "line":
        assert not want[-3:].any() and not want[0].any() and want[1:59].any(axis=1).all()          # rows with c < 3; collinear rows
    if name == "exact_planes":
        assert np.array_equal(want[:81], np.tile(F32([0, 0, 1]), (81, 1)))
    if name == "n2":
        assert not want.any()                                                         # c < 3
    if name == "dup":
        assert np.array_equal(want[:300], np.tile(F32([1, 0, 0]), (300, 1)))          # a zero covariance: no rotation, column 0 of the identity


@pytest.mark.parametrize("name", ["planes", "field", "line"])
def test_normals_with_a_viewpoint(name):
    d = dev()
    k = 6 if name == "line" else 16
    free = _check_normals(name, k, 0.1, d)
    one = _check_normals(name, k, 0.1, d, VIEW)
    rng = np.random.default_rng(9)
    per_point = (rng.uniform(-3.0, 3.0, size=(len(free), 3))).astype(F32)
    many = _check_normals(name, k, 0.1, d, per_point)
    assert np.array_equal(np.abs(one), np.abs(free)) and np.array_equal(np.abs(many), np.abs(free))
    assert not np.array_equal(one, free) or not np.array_equal(many, free)


def test_normals_tolerate_foreign_rows():
    """A row the k-NN kernel would never write: indices out of range, the point itself, a neighbour with a NaN - skipped, counted out."""
    from segdino3d_amd import superpoints
    d = dev()
    p = cloud("bad")
    rng = np.random.default_rng(2)
    nbr = rng.integers(-3, len(p) + 3, size=(len(p), 9)).astype(np.int32)
    nbr[:, 0] = np.arange(len(p))
    want = P.estimate_normals(p, nbr)
    got = superpoints.estimate_normals(_t(p, d), _t(nbr, d))
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)) and want.any()


# ---------------------------------------------------------------------------------------------- a general edge list
@functools.lru_cache(maxsize=None)
def mesh_case(mesh):
    v, edges, f = C.mesh_graph(*mesh)
    return v, edges, f, R.mesh_superpoints(v, f, debug=True)


@pytest.mark.parametrize("mesh", [("crease", 8, 8), ("boxes_on_plane", 24, 5), ("height_field", 12, 6), ("height_field", 40, 1)])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_graph_superpoints_on_a_mesh_equals_mesh_superpoints(mesh, dtype):
    from segdino3d_amd import superpoints
    d = dev()
    v, edges, f, want = mesh_case(mesh)
    labels, info = superpoints.graph_superpoints(_t(v, d), _t(want.normals, d), _t(edges, d).to(dtype), debug=True)
    assert np.array_equal(info.weights.cpu().numpy().view(np.uint32), want.weights)
    assert labels.dtype == torch.int64 and np.array_equal(labels.cpu().numpy(), want.labels)
    assert (info.count, info.bad_edges) == (want.count, 0)
    mesh_labels = superpoints.mesh_superpoints(_t(v, d), _t(f, d))
    assert torch.equal(labels, mesh_labels)
    assert torch.equal(superpoints.graph_superpoints(_t(v, d), _t(want.normals, d), _t(edges, d).to(dtype)), labels)
    if mesh == ("height_field", 40, 1):
        assert int(info.settled[0]) > 512                                             # more than one batch's worth went through the table


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_bad_edges_are_counted_not_followed(dtype):
    from segdino3d_amd import superpoints
    d = dev()
    v, edges, f, mesh_want = mesh_case(("height_field", 12, 6))
    bad = np.array([[0, len(v)], [-1, 2], [5, 1 << 40], [len(v), len(v)], [3, -(1 << 40)], [1 << 31, 0]])
    all_edges = np.concatenate([bad[:2], edges, bad[2:]])
    want = P.graph_superpoints(v, mesh_want.normals, all_edges, debug=True)
    assert want.bad_edges == 6 and np.array_equal(want.labels, mesh_want.labels)
    et = torch.from_numpy(all_edges)
    if dtype == torch.int32:
        et = et.clamp(-(1 << 31), (1 << 31) - 1).to(torch.int32)                      # an index out of range stays out of range
    labels, info = superpoints.graph_superpoints(_t(v, d), _t(mesh_want.normals, d), et.to(d), debug=True)
    assert np.array_equal(info.weights.cpu().numpy().view(np.uint32), want.weights)
    assert np.array_equal(labels.cpu().numpy(), want.labels) and (info.count, info.bad_edges) == (want.count, 6)


@pytest.mark.parametrize("kw", [dict(), dict(min_verts=1), dict(k_thresh=0.0), dict(k_thresh=0.5, min_verts=100)], ids=["default", "min_verts1", "k0", "k0.5"])
def test_unoriented_graph_ignores_sign_flips(kw):
    from segdino3d_amd import superpoints
    d = dev()
    p = cloud("field_s")
    nbr, _ = ref_knn("field_s", 12, 0.12)
    normals = P.estimate_normals(p, nbr)
    flipped = (normals * np.where(np.random.default_rng(0).random(len(p)) < 0.5, F32(-1), F32(1))[:, None]).astype(F32)
    edges = P.knn_edges(nbr)
    want = P.graph_superpoints(p, normals, edges, oriented=False, debug=True, **kw)
    for n in (normals, flipped):
        labels, info = superpoints.graph_superpoints(_t(p, d), _t(n, d), _t(edges, d), oriented=False, debug=True, **kw)
        assert np.array_equal(info.weights.cpu().numpy().view(np.uint32), want.weights)
        assert np.array_equal(labels.cpu().numpy(), want.labels) and (info.count, info.bad_edges) == (want.count, want.bad_edges)
    want_o = P.graph_superpoints(p, flipped, edges, oriented=True, debug=True, **kw)
    labels, info = superpoints.graph_superpoints(_t(p, d), _t(flipped, d), _t(edges, d), oriented=True, debug=True, **kw)
    assert np.array_equal(info.weights.cpu().numpy().view(np.uint32), want_o.weights) and np.array_equal(labels.cpu().numpy(), want_o.labels)
    assert not np.array_equal(want_o.weights, want.weights)


def test_graph_without_points_or_edges():
    from segdino3d_amd import superpoints
    d = dev()
    none, no_edges = torch.zeros(0, 3, device=d), torch.zeros(0, 2, dtype=torch.int64, device=d)
    labels, info = superpoints.graph_superpoints(none, none, no_edges, return_info=True)
    assert labels.numel() == 0 and (info.count, info.bad_edges) == (0, 0)
    labels, info = superpoints.graph_superpoints(none, none, _t(np.array([[0, 0], [0, 1]]), d), return_info=True)
    assert labels.numel() == 0 and (info.count, info.bad_edges) == (0, 2)
    p = _t(cloud("n5"), d)
    labels, info = superpoints.graph_superpoints(p, p, no_edges, return_info=True)
    assert labels.tolist() == [0, 1, 2, 3, 4] and (info.count, info.bad_edges) == (5, 0)


# ---------------------------------------------------------------------------------------------- the whole path
def _check_points(name, mode, d):
    from segdino3d_amd import superpoints
    want = ref_points(name, mode)
    p = _t(cloud(name), d)
    kw = {}
    if mode == "given":
        kw["normals"] = _t(given_normals(name), d)
    elif mode == "view":
        kw["viewpoint"] = _t(VIEW, d)
    labels, info = superpoints.point_superpoints(p, debug=True, **kw)
    nd = int((info.nbr.cpu().numpy() != want.nbr).sum())
    md = int((info.normals.cpu().numpy().view(np.uint32) != want.normals.view(np.uint32)).sum())
    wd = int((info.weights.cpu().numpy().view(np.uint32) != want.weights).sum())
    ld = int((labels.cpu().numpy() != want.labels).sum())
    print(f"{name} {mode}: N {len(want.labels)} S {want.count} bad {want.bad_edges}: neighbours differing {nd}, normal components {md}, weights {wd}, "
          f"labels {ld}, settled {info.settled.tolist()}")
    assert nd == 0 and md == 0 and wd == 0 and ld == 0
    assert (info.count, info.bad_edges) == (want.count, want.bad_edges) and want.bad_edges == int((want.nbr < 0).sum())
    assert torch.equal(superpoints.point_superpoints(p, **kw), labels)
    return labels, info


@pytest.mark.parametrize("mode", ["estimated", "given", "view"])
@pytest.mark.parametrize("name", ["boxes", "field", "n0", "n2"])
def test_point_superpoints_equal_the_restatement(name, mode):
    d = dev()
    _, info = _check_points(name, mode, d)
    if name in ("boxes", "field"):
        assert info.count > 1 and int(info.settled[0]) > 512


@pytest.mark.parametrize("mode", ["estimated", "view"])
def test_batch_of_clouds_equals_the_single_runs(mode):
    from segdino3d_amd import superpoints
    d = dev()
    names = ["field", "n0", "boxes", "line", "field_s"]
    clouds = [_t(cloud(n), d) for n in names]
    views = [_t(VIEW, d) for _ in names] if mode == "view" else None
    single = [superpoints.point_superpoints(c, viewpoint=None if views is None else views[0], debug=True) for c in clouds]
    for order in ((0, 1, 2, 3, 4), (3, 2, 4, 1, 0)):
        labels, infos = superpoints.point_superpoints_batch([clouds[i] for i in order], viewpoint=views, debug=True)
        assert len(labels) == 5
        for slot, i in enumerate(order):
            s_labels, s_info = single[i]
            assert torch.equal(labels[slot], s_labels), names[i]
            assert torch.equal(infos[slot].nbr, s_info.nbr) and torch.equal(infos[slot].weights, s_info.weights), names[i]
            assert torch.equal(infos[slot].normals.view(torch.int32), s_info.normals.view(torch.int32)), names[i]
            assert (infos[slot].count, infos[slot].bad_edges) == (s_info.count, s_info.bad_edges), names[i]
        plain = superpoints.point_superpoints_batch([clouds[i] for i in order], viewpoint=views)
        assert all(torch.equal(a, b) for a, b in zip(plain, labels))
    for i in (0, 2):
        assert np.array_equal(single[i][0].cpu().numpy(), ref_points(names[i], "estimated" if mode == "estimated" else "view").labels)


def test_device_argument_errors():
    from segdino3d_amd import superpoints
    d = dev()
    p = _t(cloud("n16"), d)
    nbr = superpoints.knn_graph(p, k=4)
    edges = torch.zeros(3, 2, dtype=torch.int64, device=d)
    for bad in (p.double(), p[:, :2], p.reshape(-1)):
        with pytest.raises(ValueError):
            superpoints.knn_graph(bad)
        with pytest.raises(ValueError):
            superpoints.point_superpoints(bad)
        with pytest.raises(ValueError):
            superpoints.graph_superpoints(p, bad, edges)
    for bad in (nbr.long(), nbr[:5], nbr.reshape(-1), torch.zeros(16, 65, dtype=torch.int32, device=d)):
        with pytest.raises(ValueError):
            superpoints.estimate_normals(p, bad)
    for bad in (edges.float(), edges[:, :1], edges.reshape(-1), edges.to(torch.int16)):
        with pytest.raises(ValueError):
            superpoints.graph_superpoints(p, p, bad)
    for bad in (torch.zeros(2, device=d), torch.zeros(3, dtype=torch.float64, device=d), torch.zeros(7, 3, device=d)):
        with pytest.raises(ValueError):
            superpoints.estimate_normals(p, nbr, bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        superpoints.estimate_normals(p, nbr, torch.zeros(3))
    with pytest.raises(ValueError, match="2\\^24"):
        superpoints.knn_graph(torch.empty(1 << 24, 3, device=d))
    with pytest.raises(ValueError):
        superpoints.graph_superpoints(p, p, edges, oriented=1)
