"""csrc/components.hip against tests/components_ref.py: labels, per-component tables, the keep table, the cleaned nodes, links and maps
and the eight counters are compared for EQUALITY (floats through a uint32 view), and `unsettled` is 0 everywhere.  The shapes are the
smallest at which each mechanism can go wrong: empty inputs, deep trees, one root taking every compare-and-swap, runs that end on wave
borders, both sides of the library sort's single-launch path, bad input, and components that sit exactly on the thresholds."""
import numpy as np
import pytest
import torch

import components_ref as R
import simplify_case as K
import tsdf_case as C

pytestmark = pytest.mark.gpu

F32 = np.float32
I32_MIN = np.iinfo(np.int32).min
NO_FACES = np.zeros((0, 3), np.int32)


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _t(a, d):
    return torch.from_numpy(np.array(a)).to(d)                   # a copy: shared cases are read-only


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert np.array_equal(got, want), what


def _check(source, links, n, coords, d, what="", **kw):
    """The device against the restatement through the operator layer - every output of the C call - and through the public function
    of the source -> the restatement."""
    from segdino3d_amd import components, ops
    links = np.ascontiguousarray(links, np.int32)
    want = R.components_ref(n, links, source, coords, **kw)
    tl, tc = _t(links, d), None if coords is None else _t(coords, d)
    out = ops.components(source, tl, n, tc, clean=True, **kw)
    info = dict(zip(ops.COMPONENTS_INFO, out["info"].tolist()))
    assert info == want.info and info["unsettled"] == 0, (what, info, want.info)
    k, nn, nl = info["components"], info["nodes"], info["links"]
    _same(out["labels"], want.labels, (what, "labels"))
    _same(out["n_nodes"][:k], want.n_nodes, (what, "n_nodes"))
    _same(out["n_links"][:k], want.n_links, (what, "n_links"))
    _same(out["box"][:k], want.box, (what, "box"))
    _same(out["keep"][:k], want.keep, (what, "keep"))
    _same(out["node_map"], want.node_map, (what, "node_map"))
    _same(out["labels_out"][:nn], want.labels_out, (what, "labels_out"))
    if coords is not None:
        _same(out["nodes"][:nn], want.nodes, (what, "nodes"))
    if source == "table":
        _same(out["links"][:nn], want.links, (what, "table"))
    else:
        _same(out["links"][:nl], want.links, (what, "links"))
        _same(out["link_source"][:nl], want.link_source, (what, "link_source"))
    # the public functions: trimmed clones
    plain = R.components_ref(n, links, source, coords) if kw else want
    if source == "faces":
        comp, cinfo = components.mesh_components(tc, tl, return_info=True)
        mesh, minfo = components.clean_mesh(tc, tl, min_faces=kw.get("min_links", 0), min_vertices=kw.get("min_nodes", 0),
                                            min_extent=kw.get("min_extent", 0.0), keep_largest=kw.get("keep_largest", 0), return_info=True)
        assert minfo._asdict() == want.info, (what, minfo)
        assert all(x.is_cuda and x.is_contiguous() for x in mesh), what
        for got, ref, name in zip(mesh, (want.nodes, want.links, want.node_map, want.link_source, want.labels_out), mesh._fields):
            _same(got, ref, (what, "clean_mesh", name))
    elif source == "edges":
        comp, cinfo = components.graph_components(n, tl, return_info=True)
    else:
        comp, cinfo = components.neighbour_components(tc, tl, return_info=True)
    assert cinfo._asdict() == plain.info, (what, cinfo)
    for got, ref, name in zip(comp, (plain.labels, plain.n_nodes, plain.n_links, plain.box), comp._fields):
        _same(got, ref, (what, "components", name))
    return want


def _coords(n, channels=3, seed=0):
    """Distinct finite coordinates with both signs, and colour channels."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-4, 4, (n, channels)).astype(F32)
    if channels > 3:
        v[:, 3:] = rng.uniform(0, 255, (n, channels - 3)).astype(F32)
    return v


# ---------------------------------------------------------------------------------------------- empty and tiny
@pytest.mark.parametrize("channels", [3, 6, 11])
def test_empty_and_tiny(channels):
    d = dev()
    none = np.zeros((0, channels), F32)
    for what, v, f in [("nothing", none, NO_FACES), ("links without nodes", none, [[0, 1, 2], [0, 0, 0], [-1, 5, I32_MIN]]),
                       ("37 vertices, no face", _coords(37, channels), NO_FACES), ("one vertex", _coords(1, channels), NO_FACES),
                       ("one face", _coords(3, channels), [[2, 0, 1]]), ("one degenerate face", _coords(1, channels), [[0, 0, 0]]),
                       ("one degenerate face of two", _coords(3, channels), [[1, 1, 2]])]:
        want = _check("faces", np.array(f, np.int32).reshape(-1, 3), len(v), v, d, what)
        if what == "37 vertices, no face":
            assert want.info["components"] == want.info["isolated"] == 37
    for what, n, e in [("graph: nothing", 0, np.zeros((0, 2), np.int32)), ("graph: links without nodes", 0, [[0, 1], [3, 3]]),
                       ("graph: no edge", 5, np.zeros((0, 2), np.int32)), ("graph: a loop and an edge", 4, [[2, 2], [3, 0]])]:
        _check("edges", np.array(e, np.int32).reshape(-1, 2), n, None, d, what)
    _check("table", np.zeros((0, 4), np.int32), 0, none, d, "table: nothing")
    _check("table", np.array([[-1, -1]], np.int32), 1, _coords(1, channels), d, "table: one point")
    _check("table", np.array([[1], [0], [2]], np.int32), 3, _coords(3, channels), d, "table: a pair and a self-loop")


# ---------------------------------------------------------------------------------------------- deep trees, contention
@pytest.mark.parametrize("order", ["in order", "reversed", "shuffled"])
def test_path_of_5000(order):
    """One component whose union-find tree is as deep as the schedule lets it be; reversed, every hook lands on the current root."""
    d = dev()
    n = 5000
    number = {"in order": np.arange(n), "reversed": np.arange(n)[::-1], "shuffled": np.random.default_rng(5).permutation(n)}[order]
    v = np.zeros((n, 3), F32)
    v[number, 0] = np.arange(n, dtype=F32) * F32(0.125)
    a, b = number[:-1], number[1:]
    want = _check("faces", np.stack([a, b, b], axis=1), n, v, d, order)
    assert want.info["components"] == 1 and want.n_links.tolist() == [n - 1] and want.box[0].tolist() == [0, (n - 1) * 0.125, 0, 0, 0, 0]
    assert _check("edges", np.stack([a, b], axis=1), n, None, d, order).info["components"] == 1


@pytest.mark.parametrize("hub", [4999, 0])
def test_star_of_5000(hub):
    """One root takes every compare-and-swap and one component takes every statistic."""
    d = dev()
    n = 5000
    i = np.arange(n)
    h = np.full(n, hub)
    want = _check("faces", np.stack([i, h, h], axis=1), n, _coords(n, 6, seed=hub), d, hub)
    assert want.info["components"] == 1 and want.n_nodes.tolist() == [n] and want.n_links.tolist() == [n]
    _check("edges", np.stack([h, i], axis=1), n, None, d, hub)


# ---------------------------------------------------------------------------------------------- run borders, sort paths
RUNS = (1, 63, 1, 64, 65, 1, 1, 257, 64, 64, 1, 63, 65, 200, 3)


def _faces_inside(members, count, rng):
    """A chain of faces that connects each member list, then random faces inside random lists, `count` in all, shuffled."""
    faces = []
    for m in members:
        faces += [[m[j], m[min(j + 1, len(m) - 1)], m[min(j + 2, len(m) - 1)]] for j in range(0, max(len(m) - 1, 1), 2)]
    assert len(faces) <= count
    while len(faces) < count:
        m = members[rng.integers(len(members))]
        faces.append([m[j] for j in rng.integers(0, len(m), 3)])
    return np.array(faces, np.int32)[rng.permutation(count)]


@pytest.mark.parametrize("interleaved", [False, True])
def test_runs_of_1_63_64_65_257_side_by_side(interleaved):
    """Sorted by label the components are runs that begin and end on, before and after the borders of a wave and of a workgroup."""
    d = dev()
    rng = np.random.default_rng(11)
    n = sum(RUNS)
    assert n == 913
    owner = np.repeat(np.arange(len(RUNS)), RUNS)
    if interleaved:
        owner = owner[rng.permutation(n)]
    members = [np.flatnonzero(owner == c).tolist() for c in range(len(RUNS))]
    f = _faces_inside(members, 1501, rng)
    want = _check("faces", f, n, _coords(n, 6, seed=12), d, interleaved)
    assert sorted(want.n_nodes.tolist()) == sorted(RUNS) and want.n_links.min() >= 1 and want.n_links.sum() == 1501
    if not interleaved:
        assert want.n_nodes.tolist() == list(RUNS)
    _check("faces", f, n, _coords(n, 6, seed=12), d, (interleaved, "kept by size"), min_nodes=64, min_links=40)


@pytest.mark.parametrize("n, F", [(4096, 4097), (4097, 4096), (9001, 17003)])
def test_sizes_across_the_sort_paths(n, F):
    """Both sides of the library sort's 4096-key single-launch path, for the node sort and for the link sort, about n / 7 components."""
    d = dev()
    rng = np.random.default_rng(n)
    owner = rng.permutation(n) % (n // 7)
    members = [m.tolist() for m in np.split(np.argsort(owner, kind="stable"), np.cumsum(np.bincount(owner))[:-1])]
    f = _faces_inside(members, F, rng)
    v = _coords(n, 3, seed=F)
    want = _check("faces", f, n, v, d, (n, F))
    assert want.info["components"] == n // 7
    _check("faces", f, n, v, d, (n, F, "largest"), keep_largest=n // 14, min_nodes=7)
    _check("edges", f[:, :2], n, None, d, (n, F, "edges"), keep_largest=5)


def test_all_singletons():
    d = dev()
    n = 5000
    f = np.stack([np.arange(100), np.full(100, n), np.arange(100)], axis=1)           # every link is bad
    want = _check("faces", f, n, _coords(n, 3, seed=3), d, "singletons")
    assert want.info["components"] == want.info["isolated"] == n and want.info["bad_links"] == 100 and want.info["links"] == 0
    assert _check("faces", f, n, _coords(n, 3, seed=3), d, "singletons, none kept", min_links=1).info["nodes"] == 0


# ---------------------------------------------------------------------------------------------- bad input
def test_bad_vertices_and_bad_faces():
    d = dev()
    v, f = K.plane(12, 0.25, channels=6, seed=4)                                       # 144 vertices, 242 faces
    v[5, 0] = np.nan
    v[17, 0] = np.inf
    v[29, 0] = 16384.0
    v[30, 0] = -16383.999
    v[40, 4] = np.nan                                                                  # a colour channel
    v[41, 5] = -np.inf
    v[42, 3] = -16384.0
    v[100, 1], v[101, 2] = np.nan, 20000.0                                             # two corners of one face
    f = np.concatenate([f, [[-1, 0, 1], [0, 144, 1], [0, 1, I32_MIN], [143, 143, 144], [2, 3, 2 ** 31 - 1]]]).astype(np.int32)
    want = _check("faces", f, len(v), v, d, "plane")
    assert want.info["bad_nodes"] == 8 and want.info["bad_links"] > 5 and want.labels[30] >= 0 and (want.labels[[5, 17, 29, 40, 41, 42, 100, 101]] == -1).all()
    _check("faces", f, len(v), v, d, "plane, largest", keep_largest=1)
    # a path that only a bad vertex cuts comes out as two components
    p = np.zeros((5, 3), F32)
    p[:, 0] = np.arange(5)
    p[2, 1] = np.nan
    path = np.array([[0, 1, 1], [1, 2, 2], [2, 3, 3], [3, 4, 4]], np.int32)
    want = _check("faces", path, 5, p, d, "cut")
    assert want.labels.tolist() == [0, 0, -1, 1, 1] and want.info["bad_links"] == 2 and want.links.tolist() == [[0, 1, 1], [2, 3, 3]]
    _check("edges", np.array([[0, 1], [1, -1], [5, 2], [I32_MIN, 0], [3, 4]], np.int32), 5, None, d, "graph indices")


# ---------------------------------------------------------------------------------------------- thresholds
def _threshold_mesh():
    """Four components: a triangle of extent 0.25; two triangles sharing an edge, extent 0.5; a 3 x 3 plane of extent 0.5 less one ulp;
    a 3 x 3 plane of extent 0.5 - the last two with 8 faces each."""
    below = float(np.nextafter(F32(0.5), F32(0)))
    tri = np.array([[0, 0, 0], [0.25, 0, 0], [0, 0.125, 0]], F32)
    quad = np.array([[2, 0, 0], [2.5, 0, 0], [2, 0.25, 0], [2.5, 0.25, -0.0]], F32)
    g = np.stack(np.meshgrid(np.arange(3), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 2).astype(F32) * F32(0.5)
    near = np.concatenate([g * F32(below), np.full((9, 1), -1.0, F32)], axis=1).astype(F32)
    full = np.concatenate([np.full((9, 1), 7.0, F32), g * F32(0.5)], axis=1).astype(F32)
    v = np.concatenate([tri, quad, near, full])
    f = np.concatenate([[[0, 1, 2]], [[3, 4, 5], [4, 6, 5]], K.grid_faces(3, 3, base=7), K.grid_faces(3, 3, base=16)]).astype(np.int32)
    return v, f, below


def test_components_exactly_on_the_thresholds():
    d = dev()
    v, f, below = _threshold_mesh()
    base = _check("faces", f, len(v), v, d, "all")
    assert base.n_nodes.tolist() == [3, 4, 9, 9] and base.n_links.tolist() == [1, 2, 8, 8]
    assert base.extent.tolist() == [0.25, 0.5, below, 0.5]
    above = float(np.nextafter(F32(0.5), F32(1)))
    for kw, keep in [(dict(min_links=2), [0, 1, 1, 1]), (dict(min_links=3), [0, 0, 1, 1]), (dict(min_nodes=4), [0, 1, 1, 1]),
                     (dict(min_nodes=5), [0, 0, 1, 1]), (dict(min_nodes=9, min_links=8), [0, 0, 1, 1]), (dict(min_nodes=10), [0, 0, 0, 0]),
                     (dict(min_extent=0.25), [1, 1, 1, 1]), (dict(min_extent=below), [0, 1, 1, 1]), (dict(min_extent=0.5), [0, 1, 0, 1]),
                     (dict(min_extent=above), [0, 0, 0, 0]),
                     (dict(keep_largest=1), [0, 0, 1, 0]), (dict(keep_largest=2), [0, 0, 1, 1]), (dict(keep_largest=3), [0, 1, 1, 1]),
                     (dict(keep_largest=4), [1, 1, 1, 1]), (dict(keep_largest=9), [1, 1, 1, 1]),
                     (dict(keep_largest=1, min_extent=0.5), [0, 0, 0, 1]), (dict(keep_largest=1, min_links=9), [0, 0, 0, 0]),
                     (dict(min_links=2, min_nodes=4, min_extent=0.5, keep_largest=2), [0, 1, 0, 1]),
                     (dict(min_links=2, min_nodes=4, min_extent=0.5, keep_largest=1), [0, 0, 0, 1])]:
        assert _check("faces", f, len(v), v, d, kw, **kw).keep.tolist() == keep, kw


# ---------------------------------------------------------------------------------------------- the table form
def _clusters():
    """Two clusters 2 m apart and a speck far from both, shuffled: 70 + 50 + 1 points with colours."""
    rng = np.random.default_rng(21)
    a = rng.uniform(0, 0.3, (70, 3))
    b = rng.uniform(0, 0.3, (50, 3)) + [2.0, 0, 0]
    xyz = np.concatenate([a, b, [[0, 5, 0]]])[rng.permutation(121)]
    return np.concatenate([xyz, rng.uniform(0, 255, (121, 3))], axis=1).astype(F32)


@pytest.mark.parametrize("k", [1, 16, 64])
def test_neighbour_table_of_two_clusters_and_a_speck(k):
    from segdino3d_amd import superpoints
    d = dev()
    pts = _clusters()
    nbr = superpoints.knn_graph(_t(pts[:, :3], d), k=k, radius=0.5).cpu().numpy()
    assert (nbr == -1).any() and (nbr >= 0).any()
    want = _check("table", nbr, len(pts), pts, d, k)
    if k > 1:
        assert sorted(want.n_nodes.tolist()) == [1, 50, 70] and want.info["isolated"] == 1 and want.info["links"] == int((nbr >= 0).sum())
    _check("table", nbr, len(pts), pts, d, (k, "speck dropped"), min_nodes=2, keep_largest=1)
    # a bad point inside a cluster: every entry that names it dangles and becomes -1, in place
    bad = pts.copy()
    hit = int(nbr[nbr >= 0][0])
    bad[hit, 4] = 16384.0
    want = _check("table", nbr, len(pts), bad, d, (k, "dangling"))
    assert want.info["bad_nodes"] == 1 and want.info["bad_links"] >= 1 and want.links.shape == (120, k)
    rows = np.delete(nbr, hit, axis=0)
    assert np.array_equal(want.links == -1, (rows == -1) | (rows == hit))
    # indices no table should hold
    odd = nbr.copy()
    odd[0, 0], odd[1, -1], odd[2, 0] = len(pts), -2, I32_MIN
    _check("table", odd, len(pts), pts, d, (k, "odd entries"))


def test_clean_points_feeds_the_normals():
    """`clean_points` = knn_graph + the table form; its cleaned table EQUALS the k-NN graph of the cleaned cloud, so `estimate_normals`
    runs on it without a second search."""
    from segdino3d_amd import components, superpoints
    d = dev()
    pts = _clusters()
    tp = _t(pts, d)
    nbr = superpoints.knn_graph(tp[:, :3].contiguous(), k=16, radius=0.5)
    want = R.components_ref(len(pts), nbr.cpu().numpy(), "table", pts, min_nodes=60)
    cloud, info = components.clean_points(tp, k=16, radius=0.5, min_points=60, return_info=True)
    assert info._asdict() == want.info and info.kept == 1 and info.nodes == 70 and info.unsettled == 0
    for got, ref, name in zip(cloud, (want.nodes, want.node_map, want.labels_out, want.links), cloud._fields):
        _same(got, ref, name)
    xyz = cloud.points[:, :3].contiguous()
    again = superpoints.knn_graph(xyz, k=16, radius=0.5)
    assert torch.equal(cloud.neighbours, again)
    assert torch.equal(superpoints.estimate_normals(xyz, cloud.neighbours), superpoints.estimate_normals(xyz, again))
    everything = components.clean_points(tp)                                             # the defaults drop nothing
    assert torch.equal(everything.points, tp) and torch.equal(everything.point_map, torch.arange(121, dtype=torch.int32, device=d))


# ---------------------------------------------------------------------------------------------- a function of the set
def _debris_mesh():
    bv, bf = K.box(24, 0.011, origin=(-0.2, -0.2, -0.2))                                 # 3176 vertices, 6348 faces
    pv, pf = K.plane(9, 0.03, origin=(1.0, 0.0, 0.0))
    sv, sf = K.sheets(4, 0.02, 0.005, origin=(0.0, 1.0, 0.0))                            # two more components
    v = np.concatenate([bv, pv, sv, [[3, 3, 3]]]).astype(F32)
    v = np.concatenate([v, np.random.default_rng(7).uniform(0, 255, (len(v), 3)).astype(F32)], axis=1)
    f = np.concatenate([bf, pf + len(bv), sf + len(bv) + len(pv)]).astype(np.int32)
    return v, f


def test_permuted_faces_and_streams_do_not_change_a_bit():
    from segdino3d_amd import components, ops
    d = dev()
    v, f = _debris_mesh()
    kw = dict(min_faces=20, keep_largest=2)
    want = _check("faces", f, len(v), v, d, "debris", min_links=20, keep_largest=2)
    assert want.info["components"] == 5 and want.info["kept"] == 2
    base = components.clean_mesh(_t(v, d), _t(f, d), **kw)
    comp = components.mesh_components(_t(v, d), _t(f, d))
    for seed in (8, 9):
        perm = np.random.default_rng(seed).permutation(len(f))
        got = components.clean_mesh(_t(v, d), _t(f[perm], d), **kw)
        assert torch.equal(got.vertices, base.vertices) and torch.equal(got.vertex_map, base.vertex_map) and torch.equal(got.labels, base.labels)
        assert all(torch.equal(a, b) for a, b in zip(components.mesh_components(_t(v, d), _t(f[perm], d)), comp))
        # only the order of the faces follows the permutation: kept face j of the permuted mesh is original face perm[face_source[j]]
        origin = _t(perm, d)[got.face_source.long()]
        assert torch.equal(origin.sort().values, base.face_source.long())
        assert torch.equal(got.faces, base.faces[torch.searchsorted(base.face_source.long(), origin)])
    # relabelled vertices: the same components, numbered by their smallest new vertex
    v2, f2, vperm = K.relabel(v, f, 10)
    _check("faces", f2, len(v2), v2, d, "relabelled", min_links=20, keep_largest=2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with ops.use_stream(side):
        again = components.clean_mesh(_t(v, d), _t(f, d), **kw)
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(a, b) for a, b in zip(again, base))
    assert all(torch.equal(a, b) for a, b in zip(components.clean_mesh(_t(v, d), _t(f, d), **kw), base))              # and twice


# ---------------------------------------------------------------------------------------------- the chain
def test_room_mesh_with_debris_to_simplify_and_back():
    """Views -> TsdfVolume -> clean_mesh -> simplify_mesh -> carry_back -> carry_back: the room with three planted floating pieces
    EQUALS the restatement, `min_faces=30` drops the two small pieces (and the room's own specks) and keeps the third, the decimation
    finds nothing bad left, and per-vertex results come back onto the original vertices through both maps."""
    import fuse_views_case as FK
    from segdino3d_amd import components, lift2d, simplify, tsdf
    d = dev()
    c = FK.room_case()
    views = lift2d.Views(_t(c["depth_u16"], d), _t(c["intr"], d), c["poses"], C.DEPTH_SCALE)
    vertices, faces = tsdf.tsdf_mesh(views, _t(c["colors"], d), capacity=1 << 12, **C.ROOM_RULE)
    _, room = C.room_ref()
    assert tuple(vertices.shape) == room.vertices.shape and tuple(faces.shape) == room.faces.shape
    nv = len(room.vertices)
    hi = room.vertices[:, :3].max(axis=0)
    tri = np.array([[0, 0, 0], [0.05, 0, 0], [0, 0.05, 0]], F32) + (hi + 1.0)
    fan = np.concatenate([[[0, 0, 0]], 0.1 * np.stack([np.cos(np.arange(18) / 3.0), np.sin(np.arange(18) / 3.0), np.zeros(18)], axis=1)]) + (hi + 2.0)
    fan_f = np.stack([np.zeros(17, np.int64), np.arange(1, 18), np.arange(2, 19)], axis=1)
    grid, grid_f = K.plane(7, 0.05, origin=tuple((hi + 3.0).tolist()))
    grid, grid_f = grid[:40], grid_f[(grid_f < 40).all(axis=1)]                          # 40 vertices, more than 30 faces
    assert len(fan) == 19 and len(fan_f) < 30 <= len(grid_f)
    pieces = np.concatenate([tri, fan, grid]).astype(F32)
    debris = np.concatenate([pieces, np.full((len(pieces), room.vertices.shape[1] - 3), 128.0, F32)], axis=1)
    v = np.concatenate([room.vertices, debris]).astype(F32)
    f = np.concatenate([room.faces, [[nv, nv + 1, nv + 2]], fan_f + nv + 3, grid_f + nv + 22]).astype(np.int32)
    tv, tf = torch.cat([vertices, _t(debris, d)]), torch.cat([faces, _t(f[len(room.faces):], d)])
    want = R.components_ref(len(v), f, "faces", v, min_links=30, min_nodes=1)
    mesh, info = components.clean_mesh(tv, tf, min_faces=30, return_info=True)
    assert info._asdict() == want.info and info.unsettled == 0
    for got, ref, name in zip(mesh, (want.nodes, want.links, want.node_map, want.link_source, want.labels_out), mesh._fields):
        _same(got, ref, name)
    vmap = mesh.vertex_map.cpu().numpy()
    assert (vmap[nv:nv + 22] == -1).all() and (vmap[nv + 22:] >= 0).all()               # the triangle and the fan go, the grid stays
    assert info.kept == int((want.n_links >= 30).sum()) >= 2 and info.components - info.kept >= 2 and info.bad_nodes == info.bad_links == 0
    small, sinfo = simplify.simplify_mesh(mesh.vertices, mesh.faces, cell=0.1, return_info=True)
    assert sinfo.bad_vertices == sinfo.bad_faces == 0 and sinfo.vertices > 0
    x = torch.arange(sinfo.vertices, dtype=torch.int64, device=d)
    back = simplify.carry_back(simplify.carry_back(x, small.vertex_map, -1), mesh.vertex_map, -1)
    assert back.shape == (len(v),) and torch.equal(back == -1, mesh.vertex_map == -1)
    live = mesh.vertex_map >= 0
    assert torch.equal(back[live], small.vertex_map[mesh.vertex_map[live].long()].long())
