"""csrc/simplify.hip + segdino3d_amd/simplify.py against the numpy restatement tests/simplify_ref.py (the reference has no counterpart) on
the hand-built meshes of tests/simplify_case.py, planted edge cases and the synthetic room of tests/tsdf_case.py.

Bounds.  None: the BITS of the vertices (compared through a uint32 view), the faces, vertex_map, face_source and all seven counters
must EQUAL the restatement.  Every decision of the rule is an integer one or a single rounded fp32 operation, the per-cell state is
int64 sums of exact fixed-point products, and every emitted float is one float64 division rounded once to fp32, or a copied row."""
import numpy as np
import pytest
import torch

import simplify_case as K
import simplify_ref as R
import tsdf_case as C

pytestmark = pytest.mark.gpu

S = 2.0 ** -5
NO_FACES = np.zeros((0, 3), np.int32)


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _t(a, d):
    return torch.from_numpy(np.array(a)).to(d)                   # a copy: shared cases are read-only


def _equal(got, info, want, what):
    assert got.vertices.dtype == torch.float32 and got.faces.dtype == got.vertex_map.dtype == got.face_source.dtype == torch.int32, what
    assert all(x.is_cuda and x.is_contiguous() for x in got), what
    assert tuple(got.vertices.shape) == want.vertices.shape and tuple(got.faces.shape) == want.faces.shape, (what, got.vertices.shape, got.faces.shape)
    assert info._asdict() == want.info, (what, info, want.info)
    assert np.array_equal(got.vertex_map.cpu().numpy(), want.vertex_map), what
    assert np.array_equal(got.face_source.cpu().numpy(), want.face_source), what
    assert np.array_equal(got.faces.cpu().numpy(), want.faces), what
    assert np.array_equal(got.vertices.cpu().numpy().view(np.uint32), want.vertices.view(np.uint32)), what


def _check(v, f, d, what="", modes=(("mean", True), ("nearest", False)), **kw):
    """The device against the restatement for each (placement, keep_unreferenced) of `modes` -> the last restatement."""
    from segdino3d_amd import simplify
    tv, tf = _t(v, d), _t(f, d)
    want = None
    for placement, keep in modes:
        want = R.simplify_ref(v, f, placement=placement, keep_unreferenced=keep, **kw)
        got, info = simplify.simplify_mesh(tv, tf, placement=placement, keep_unreferenced=keep, return_info=True, **kw)
        _equal(got, info, want, (what, placement, keep, kw))
    return want


ALL_MODES = (("mean", True), ("mean", False), ("nearest", True), ("nearest", False))


# ---------------------------------------------------------------------------------------------- empty and tiny inputs
@pytest.mark.parametrize("channels", [3, 6, 11])
def test_empty_and_tiny(channels):
    d = dev()
    rng = np.random.default_rng(channels)
    none = np.zeros((0, channels), np.float32)
    want = _check(none, NO_FACES, d, "V = 0", ALL_MODES)
    assert want.vertices.shape == (0, channels) and not any(want.info.values())
    want = _check(none, np.array([[0, 1, 2], [0, 0, 0]], np.int32), d, "V = 0 with faces", ALL_MODES)
    assert want.info["bad_faces"] == 2
    some = rng.uniform(-1, 1, (37, channels)).astype(np.float32)
    want = _check(some, NO_FACES, d, "F = 0", ALL_MODES, cell=0.5)
    assert want.info["unreferenced"] > 1 and want.faces.shape == (0, 3)
    want = _check(some[:1], NO_FACES, d, "one vertex", ALL_MODES)
    assert want.info["vertices"] == 0 and want.info["unreferenced"] == 1 and want.vertex_map.tolist() == [-1]
    want = _check(some[:1], np.array([[0, 0, 0]], np.int32), d, "one vertex, one face", ALL_MODES)
    assert want.info["collapsed"] == 1
    tri = np.zeros((3, channels), np.float32)
    tri[:, :3] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    want = _check(tri, np.array([[2, 0, 1]], np.int32), d, "one face", ALL_MODES, cell=0.25)
    assert want.info["faces"] == 1 and want.faces.tolist() == [[0, 2, 1]] and want.vertex_map.tolist() == [0, 2, 1]


# ---------------------------------------------------------------------------------------------- run lengths
def test_all_vertices_in_one_cell():
    """V = 5000 in one cell: 79 waves add into one cell; every face collapses."""
    d = dev()
    rng = np.random.default_rng(0)
    v = rng.uniform(0.01, 0.99, (5000, 6)).astype(np.float32)
    v[:, 3:] *= 255
    f = rng.integers(0, 5000, (7001, 3)).astype(np.int32)
    want = _check(v, f, d, "one cell", ALL_MODES, cell=1.0)
    assert want.info["vertices"] == 0 and want.info["unreferenced"] == 1 and want.info["faces"] == 0 and want.info["collapsed"] == 7001
    want = _check(v, f, d, "one cell", (("mean", True), ("nearest", True)), cell=1.0)
    assert want.info["vertices"] == 1 and want.info["faces"] == 0


@pytest.mark.parametrize("shuffle", [False, True])
def test_runs_of_1_63_64_65_257_side_by_side(shuffle):
    """Runs that end before, on and after a wave's border, one that spans a workgroup, and single vertices between them; sorted by key
    they sit side by side.  V = 913 and F = 1501 are no multiples of the block size."""
    d = dev()
    rng = np.random.default_rng(1)
    runs = [1, 63, 1, 64, 65, 1, 1, 257, 64, 64, 1, 63, 65, 200, 3]
    cells = np.arange(len(runs)) - 7                                                     # along x, negative cells included
    v = np.concatenate([np.concatenate([rng.uniform(c + 0.01, c + 0.99, (n, 1)), rng.uniform(0.01, 0.99, (n, 4))], axis=1)
                        for c, n in zip(cells, runs)]).astype(np.float32)
    assert len(v) == 913
    if shuffle:
        v = v[rng.permutation(len(v))]
    f = rng.integers(0, len(v), (1501, 3)).astype(np.int32)
    want = _check(v, f, d, "runs", ALL_MODES, cell=1.0)
    assert want.info["vertices"] <= len(runs) and np.bincount(want.vertex_map[want.vertex_map >= 0]).max() == 257
    assert want.info["duplicates"] > 0 and want.info["collapsed"] > 0 and want.info["faces"] > 0
    _check(v, f, d, "runs", (("mean", True),), cell=1.0)


def test_sizes_across_the_sort_paths():
    """The library's sort ranks up to 4096 keys in one launch and runs digit passes above: both sides of it for vertices and faces,
    several workgroups, ragged ends."""
    d = dev()
    rng = np.random.default_rng(2)
    for V, F in ((4096, 4097), (4097, 4096), (9001, 17003)):
        v = rng.uniform(-0.6, 0.6, (V, 4)).astype(np.float32)
        f = rng.integers(0, V, (F, 3)).astype(np.int32)
        want = _check(v, f, d, (V, F), cell=0.1)
        assert want.info["faces"] > 0 and want.info["vertices"] > 100


# ---------------------------------------------------------------------------------------------- cell arithmetic
@pytest.mark.parametrize("cell", [0.03, 0.04, 2.0 ** -6, 0.25])
def test_cell_borders_signs_and_key_bits(cell):
    """Coordinates exactly on cell borders (as the fp32 and the float64 multiple), negative ones, -0.0, and coordinates next to +-2^14,
    where the key uses its top bits when cell = 2^-6."""
    d = dev()
    k = np.arange(-40, 41)
    edge = np.float32(16384.0) - np.float32(2.0 ** -10)
    xs = np.concatenate([(k * cell).astype(np.float32), (k * np.float64(np.float32(cell))).astype(np.float32),
                         np.nextafter((k * cell).astype(np.float32), np.float32(-np.inf)), np.nextafter((k * cell).astype(np.float32), np.float32(np.inf)),
                         np.array([0.0, -0.0, edge, -edge, edge - 1, -edge + 1, 16383.0, -16383.0, 8192.0, -8192.0], np.float32)])
    rng = np.random.default_rng(3)
    v = np.stack([xs, rng.permutation(xs), rng.permutation(xs)], axis=1)
    v = np.concatenate([v, v[:, [2, 0, 1]], np.array([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [edge, edge, edge], [-edge, -edge, -edge]], np.float32)])
    f = rng.integers(0, len(v), (700, 3)).astype(np.int32)
    want = _check(v, f, d, ("borders", cell), ALL_MODES, cell=cell)
    assert want.info["bad_vertices"] == 0 and want.vertex_map[-4] == want.vertex_map[-3]
    keys = R.cell_keys(v[:, :3], cell)
    if cell == 2.0 ** -6:
        assert keys.max() >> 42 == (1 << 21) - 1 and keys.min() >> 42 == 0              # the 21 bits of an axis, end to end


# ---------------------------------------------------------------------------------------------- bad vertices and bad faces
def test_bad_vertices_and_bad_faces():
    d = dev()
    rng = np.random.default_rng(4)
    v = rng.uniform(-1, 1, (300, 6)).astype(np.float32)
    v[7, 1] = np.nan
    v[70, 5] = np.inf                                                                   # an attribute
    v[130, 4] = -np.inf
    v[131, 0] = 16384.0
    v[200, 2] = -16384.0
    v[201, 3] = 16384.0
    v[202, 0] = np.float32(16384.0) - np.float32(2.0 ** -10)                            # passes
    v[299, 3] = np.nan
    f = rng.integers(0, 300, (900, 3)).astype(np.int32)
    f[:8] = [[7, 1, 2], [1, 70, 2], [1, 2, 131], [200, 201, 202], [202, 1, 2], [299, 299, 299], [130, 130, 5], [7, 7, 7]]
    f[100] = [-1, 1, 2]
    f[101] = [1, 300, 2]
    f[102] = [1, 2, np.iinfo(np.int32).min]
    f[103] = [np.iinfo(np.int32).max, 1, 2]
    f[899] = [1, 2, 301]
    want = _check(v, f, d, "bad", ALL_MODES, cell=0.25)
    assert want.info["bad_vertices"] == 7 and want.info["bad_faces"] >= 12 and want.info["faces"] > 100
    assert (want.vertex_map[[7, 70, 130, 131, 200, 201, 299]] == -1).all() and want.vertex_map[202] >= 0
    assert 4 in want.face_source


# ---------------------------------------------------------------------------------------------- duplicates
def test_duplicates_windings_and_the_thin_sheet():
    d = dev()
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.01, 0.01, 0], [5, 5, 5], [1, 1, 0]], np.float32)
    two = [[1, 2, 3], [2, 0, 1]]                                                        # one oriented triple from 2 source faces
    seventy = [[[5, 1, 2], [1, 2, 5], [2, 5, 1]][i % 3] for i in range(70)]             # and one from 70
    opposite = [[1, 0, 2], [0, 2, 1], [2, 1, 5]]
    f = np.array([[4, 4, 4]] + two + seventy[:35] + opposite + seventy[35:] + [[1, 2, 7]], np.int32)
    want = _check(v, f, d, "duplicates", ALL_MODES, cell=0.5)
    assert want.info["duplicates"] == 1 + 69 + 1 and want.info["faces"] == 4 and want.face_source.tolist() == [1, 3, 38, 40]
    sv, sf = K.sheets(9, S, gap=S / 4)
    want = _check(sv, sf, d, "thin sheet", ALL_MODES, cell=2 * S)
    assert want.info["faces"] == 64 and want.info["duplicates"] == 0
    rng = np.random.default_rng(5)
    many = rng.integers(0, 6, (5000, 3)).astype(np.int32)                               # a few triples, thousands of times each
    want = _check(v, many, d, "many duplicates", cell=0.5)
    assert want.info["duplicates"] > 1000 and want.info["faces"] <= 40


# ---------------------------------------------------------------------------------------------- hand-built meshes and channels
@pytest.mark.parametrize("channels", [3, 6, 11])
def test_plane_and_box(channels):
    d = dev()
    pv, pf = K.plane(10, S, origin=(-3 * S, 0.0, 0.5), channels=channels, seed=channels)
    want = _check(pv, pf, d, "plane", ALL_MODES, cell=2 * S)
    assert want.info["faces"] == 2 * 5 * 4                                             # x: the quads i = 0, 2, 4, 6, 8 span two cells; y: j = 1, 3, 5, 7
    bv, bf = K.box(13, S, origin=(-8 * S, 4 * S, 0.0))
    attrs = np.random.default_rng(channels).uniform(-255, 255, (len(bv), channels - 3)).astype(np.float32)
    want = _check(np.concatenate([bv, attrs], axis=1), bf, d, "box", ALL_MODES, cell=4 * S)
    directed, undirected = C.edge_use(want.faces)
    assert (np.unique(undirected, return_counts=True)[1] == 2).all() and len(np.unique(directed)) == len(directed)
    _check(np.concatenate([bv, attrs], axis=1), bf, d, "box, inexact cell", ALL_MODES, cell=0.04)


# ---------------------------------------------------------------------------------------------- nearest: ties
def test_nearest_ties():
    d = dev()
    v = np.array([[0.10, 0.1, 0.1, 7], [0.30, 0.1, 0.1, 8], [0.30, 0.1, 0.1, 9], [0.20, 0.1, 0.1, 1], [0.20, 0.1, 0.1, 2],
                  [0.6, 0.1, 0.1, 3], [0.6, 0.1, 0.1, 4], [1.125, 0.25, 0.25, 5], [1.375, 0.25, 0.25, 6]], np.float32)
    want = _check(v, NO_FACES, d, "ties", (("nearest", True),), cell=0.5)
    assert want.vertices.view(np.uint32).tolist() == v[[3, 5, 7]].view(np.uint32).tolist()
    want = _check(v[::-1].copy(), NO_FACES, d, "ties reversed", (("nearest", True),), cell=0.5)
    assert want.vertices[:, 3].tolist() == [2.0, 4.0, 6.0]                               # the lower index of the reversed order
    rng = np.random.default_rng(6)
    twins = np.repeat(rng.uniform(-2, 2, (150, 5)).astype(np.float32), 3, axis=0)        # every vertex three times, in a random order
    twins = twins[rng.permutation(len(twins))]
    _check(twins, rng.integers(0, len(twins), (400, 3)).astype(np.int32), d, "twins", (("nearest", True), ("nearest", False)), cell=0.5)


# ---------------------------------------------------------------------------------------------- unreferenced vertices
def test_keep_unreferenced_and_the_renumbering():
    """A plane and, far from it, a speck: a small closed fan whose vertices all fall into one cell, so all its faces collapse and the
    cell stays without a face.  The speck's key lies between the plane's, so dropping it renumbers the cells after it."""
    from segdino3d_amd import simplify
    d = dev()
    pv, pf = K.plane(9, S, origin=(0.0, 0.0, 0.0))
    speck = (np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]) * (S / 8) + np.array([2.5 * S, 0.25 * S, 10 * S])).astype(np.float32)
    sf = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32) + len(pv)
    v, f = np.concatenate([pv, speck]), np.concatenate([pf[:40], sf, pf[40:]])
    keep = _check(v, f, d, "speck", (("nearest", True), ("mean", True)), cell=2 * S)
    drop = _check(v, f, d, "speck", (("nearest", False), ("mean", False)), cell=2 * S)
    assert keep.info["unreferenced"] == drop.info["unreferenced"] == 1 and keep.info["vertices"] == drop.info["vertices"] + 1 == 26
    s = keep.vertex_map[len(pv)]
    assert 0 < s < 25 and (keep.vertex_map[len(pv):] == s).all() and (drop.vertex_map[len(pv):] == -1).all()
    assert np.array_equal(drop.vertices, np.delete(keep.vertices, s, axis=0))
    assert np.array_equal(drop.faces, keep.faces - (keep.faces > s)) and (keep.faces != s).all()
    assert np.array_equal(drop.face_source, keep.face_source)
    # carry_back: per-vertex values of the small mesh on the full one
    got = simplify.simplify_mesh(_t(v, d), _t(f, d), cell=2 * S, keep_unreferenced=False)
    ids = torch.arange(got.vertices.shape[0], device=d, dtype=torch.int64) * 10
    back = simplify.carry_back(ids, got.vertex_map, -1).cpu().numpy()
    assert np.array_equal(back, np.where(drop.vertex_map >= 0, drop.vertex_map.astype(np.int64) * 10, -1))
    rows = simplify.carry_back(got.vertices, got.vertex_map, float("nan")).cpu().numpy()
    assert np.isnan(rows[len(pv):]).all() and np.array_equal(rows[:len(pv)], drop.vertices[drop.vertex_map[:len(pv)]])


# ---------------------------------------------------------------------------------------------- a function of the set
def test_permutations_and_streams_do_not_change_a_bit():
    from segdino3d_amd import ops, simplify
    d = dev()
    bv, bf = K.box(40, 0.011, origin=(-0.2, -0.2, -0.2))                                 # 9128 vertices, 18252 faces
    v = np.concatenate([bv, np.random.default_rng(7).uniform(0, 255, (len(bv), 3)).astype(np.float32)], axis=1)
    want = _check(v, bf, d, "box", cell=0.04)
    base = simplify.simplify_mesh(_t(v, d), _t(bf, d), cell=0.04)
    for seed in (8, 9):
        v2, f2, perm = K.relabel(v, bf, seed)
        _check(v2, f2, d, ("relabelled", seed), (("mean", True),), cell=0.04)
        got = simplify.simplify_mesh(_t(v2, d), _t(f2, d), cell=0.04)
        assert torch.equal(got.vertices, base.vertices)
        assert torch.equal(got.vertex_map, base.vertex_map[_t(perm, d)])
        assert np.array_equal(np.unique(got.faces.cpu().numpy(), axis=0), np.unique(base.faces.cpu().numpy(), axis=0))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with ops.use_stream(side):
        again = simplify.simplify_mesh(_t(v, d), _t(bf, d), cell=0.04)
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(a, b) for a, b in zip(again, base))
    assert all(torch.equal(a, b) for a, b in zip(simplify.simplify_mesh(_t(v, d), _t(bf, d), cell=0.04), base))     # and twice


# ---------------------------------------------------------------------------------------------- the chain
def test_room_mesh_to_superpoints_and_back():
    """Views -> TsdfVolume -> simplify_mesh -> mesh_superpoints -> carry_back: the decimated room EQUALS the restatement applied to the
    TSDF restatement's mesh, its superpoints EQUAL tests/superpoints_ref.py on it, and the labels carried back are -1 exactly where the
    map is."""
    import fuse_views_case as FK
    import superpoints_ref as SP
    from segdino3d_amd import lift2d, simplify, superpoints, tsdf
    d = dev()
    c = FK.room_case()
    views = lift2d.Views(_t(c["depth_u16"], d), _t(c["intr"], d), c["poses"], C.DEPTH_SCALE)
    vertices, faces = tsdf.tsdf_mesh(views, _t(c["colors"], d), capacity=1 << 12, **C.ROOM_RULE)
    _, room = C.room_ref()
    # the room of the TSDF tests is fused at 5 cm, so at cell = 0.04 no two of its vertices share a cell: the mesh comes through whole
    # but for the vertices of its open border that no face uses (keep_unreferenced=False drops them); at 0.1 it is decimated
    for cell in (0.1, 0.04):
        for keep in (True, False):
            want = R.simplify_ref(room.vertices, room.faces, cell=cell, keep_unreferenced=keep)
            got, info = simplify.simplify_mesh(vertices, faces, cell=cell, keep_unreferenced=keep, return_info=True)
            _equal(got, info, want, ("room", cell, keep))
            assert len(room.faces) == info.bad_faces + info.collapsed + info.duplicates + info.faces
            if cell == 0.1:
                assert 0 < info.vertices < len(room.vertices) // 2 and 0 < info.faces < len(room.faces) // 2 and info.collapsed > 0
    assert info.unreferenced > 0 and bool((got.vertex_map == -1).any())
    labels, sp = superpoints.mesh_superpoints(got.vertices[:, :3].contiguous(), got.faces, return_info=True)
    ref = SP.mesh_superpoints(np.ascontiguousarray(want.vertices[:, :3]), want.faces)
    assert np.array_equal(labels.cpu().numpy(), ref.labels) and sp.count == ref.count and ref.count > 1 and sp.bad_faces == 0
    back = simplify.carry_back(labels, got.vertex_map, -1)
    assert back.shape == (len(room.vertices),) and torch.equal(back == -1, got.vertex_map == -1)
    live = got.vertex_map >= 0
    assert torch.equal(back[live], labels[got.vertex_map[live].long()])
