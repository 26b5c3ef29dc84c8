"""The numpy restatement of the decimation rule (tests/simplify_ref.py) against counts worked out by hand: the kernels are pinned to
the restatement bit for bit (tests/test_gpu_simplify.py), so the restatement itself is held against something that is not code."""
import time

import numpy as np
import pytest

import simplify_case as K
import simplify_ref as R
import tsdf_case as T

S = 2.0 ** -5                       # the grid spacing of the hand-built meshes: exact in fp32, and so is 1 / (2 S)


def _consistent(vertices, faces, cell, placement, keep, res):
    """What must hold between the outputs of any call."""
    V, F = len(vertices), len(faces)
    i = res.info
    assert F == i["bad_faces"] + i["collapsed"] + i["duplicates"] + i["faces"]
    assert i["vertices"] == len(res.vertices) and i["faces"] == len(res.faces) == len(res.face_source)
    assert res.vertex_map.shape == (V,) and res.vertex_map.max(initial=-1) < i["vertices"]
    assert (res.vertex_map == -1).sum() >= i["bad_vertices"]
    if keep:
        assert (res.vertex_map == -1).sum() == i["bad_vertices"]
        assert np.array_equal(np.unique(res.vertex_map[res.vertex_map >= 0]), np.arange(i["vertices"]))    # every output vertex has a member
    else:
        assert np.array_equal(np.unique(res.faces), np.arange(i["vertices"]))                              # and a face
    # a kept face IS its source through the map, rotated; sources ascend
    assert (np.diff(res.face_source) > 0).all()
    through = res.vertex_map[np.asarray(faces)[res.face_source]]
    assert (res.faces[:, 0] < res.faces[:, 1]).all() and (res.faces[:, 0] < res.faces[:, 2]).all()
    for r in range(3):
        hit = (np.roll(through, -r, axis=1) == res.faces).all(axis=1)
        through[hit] = np.roll(through, -r, axis=1)[hit]
    assert np.array_equal(through, res.faces)
    assert len(np.unique(res.faces, axis=0)) == len(res.faces)
    # a member lies in its vertex's cell, and a mean vertex inside the cell's closed box
    live = res.vertex_map >= 0
    if live.any():
        inv = np.float32(1.0 / cell)
        k_in = np.floor(np.asarray(vertices, np.float32)[live, :3] * inv)
        k_out = np.floor(res.vertices[res.vertex_map[live], :3] * inv)
        if placement == "nearest":
            assert np.array_equal(k_in, k_out)
        else:
            assert (np.abs(k_in - k_out) <= 1).all()


@pytest.mark.parametrize("m", [3, 9, 10])
def test_plane_counts_by_hand(m):
    """Vertices i = 0 .. m - 1 at spacing S, cell 2 S: cell i // 2 per axis, ceil(m / 2)^2 cells.  A quad (i, j) survives iff i and j are
    both odd: an even index shares its cell with the next one, and then both triangles of the quad have two corners in one cell.
    `odd` counts the odd i among the quads' 0 .. m - 2; the surviving quads reference odd + 1 cells per axis."""
    v, f = K.plane(m, S, channels=6)
    res = R.simplify_ref(v, f, cell=2 * S)
    cells, odd = (m + 1) // 2, len([i for i in range(m - 1) if i % 2 == 1])
    want = dict(vertices=cells * cells, faces=2 * odd * odd, bad_vertices=0, bad_faces=0, collapsed=2 * (m - 1) ** 2 - 2 * odd * odd,
                duplicates=0, unreferenced=(cells * cells - (odd + 1) ** 2) if odd else cells * cells)
    assert res.info == want
    _consistent(v, f, 2 * S, "mean", True, res)
    # the mean of the cell's members: cell (a, b) holds i in {2a, 2a + 1} cut at m - 1
    mean_1d = np.array([np.mean([i for i in (2 * a, 2 * a + 1) if i < m]) for a in range(cells)]) * S
    assert np.array_equal(res.vertices[:, 0].reshape(cells, cells), np.broadcast_to(mean_1d[:, None], (cells, cells)).astype(np.float32))
    assert np.array_equal(res.vertices[:, 1].reshape(cells, cells), np.broadcast_to(mean_1d[None, :], (cells, cells)).astype(np.float32))
    assert (res.vertices[:, 2] == 0).all()
    # every kept face keeps its normal
    n = T.face_normals(res.vertices, res.faces)
    assert (n[:, 2] > 0).all() and (n[:, :2] == 0).all()
    # colours: the integer mean in fixed point, within half a unit of 2^-16 of the float64 mean
    members = [np.nonzero(res.vertex_map == k)[0] for k in range(cells * cells)]
    want_rgb = np.stack([v[idx, 3:].astype(np.float64).mean(axis=0) for idx in members])
    assert np.abs(res.vertices[:, 3:] - want_rgb).max() <= 2.0 ** -17 + 2.0 ** -17          # the quantisation + the fp32 rounding at 255


@pytest.mark.parametrize("placement", ["mean", "nearest"])
@pytest.mark.parametrize("m, cell", [(9, 2 * S), (9, 4 * S), (13, 4 * S)])
def test_closed_box_stays_closed(m, cell, placement):
    """The box sits on cell borders, so the cells of its surface form a coarser box: a closed surface again."""
    v, f = K.box(m, S, origin=(-8 * S, 4 * S, 0.0))
    directed, undirected = T.edge_use(f)
    assert (np.unique(undirected, return_counts=True)[1] == 2).all() and len(np.unique(directed)) == len(directed)      # the input is closed
    for keep in (True, False):
        res = R.simplify_ref(v, f, cell=cell, placement=placement, keep_unreferenced=keep)
        _consistent(v, f, cell, placement, keep, res)
        assert res.info["faces"] > 0 and res.info["collapsed"] > 0 and res.info["bad_faces"] == 0
        directed, undirected = T.edge_use(res.faces)
        assert (np.unique(undirected, return_counts=True)[1] == 2).all()                   # each edge is used by exactly two faces,
        assert len(np.unique(directed)) == len(directed)                                    # once in each direction
        assert res.info["unreferenced"] == 0 and res.info["duplicates"] == 0


def test_thin_sheet_keeps_both_sides():
    """Two sheets closer than the cell, in one layer of cells: the same output vertices, every triple in both windings, none a duplicate."""
    m = 9
    v, f = K.sheets(m, S, gap=S / 4)
    one = R.simplify_ref(*K.plane(m, S), cell=2 * S)
    res = R.simplify_ref(v, f, cell=2 * S)
    _consistent(v, f, 2 * S, "mean", True, res)
    assert res.info["vertices"] == one.info["vertices"] and res.info["faces"] == 2 * one.info["faces"] and res.info["duplicates"] == 0
    n = T.face_normals(res.vertices, res.faces)
    assert (n[:, 2] > 0).sum() == (n[:, 2] < 0).sum() == one.info["faces"]
    up = {tuple(t) for t in res.faces[n[:, 2] > 0]}
    down = {(a, c, b) for a, b, c in res.faces[n[:, 2] < 0]}
    assert up == down


def test_duplicates_lowest_index_wins_and_windings_differ():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.01, 0.01, 0], [5, 5, 5]], np.float32)
    f = np.array([[4, 4, 4], [1, 2, 3], [2, 0, 1], [0, 1, 2], [1, 0, 2], [3, 1, 2], [0, 2, 1], [1, 2, 7], [-1, 0, 1]], np.int32)
    res = R.simplify_ref(v, f, cell=0.5)
    # cells in key order: (0,0,0) <- vertices 0 and 3, (0,2,0) <- 2, (2,0,0) <- 1, (10,10,10) <- 4
    assert res.vertex_map.tolist() == [0, 2, 1, 0, 3]
    # face 1 = (2, 1, 0) -> rotated (0, 2, 1); faces 2, 3, 5 are the same oriented triple; faces 4 and 6 the opposite winding
    assert res.faces.tolist() == [[0, 2, 1], [0, 1, 2]] and res.face_source.tolist() == [1, 4]
    assert res.info == dict(vertices=4, faces=2, bad_vertices=0, bad_faces=2, collapsed=1, duplicates=4, unreferenced=1)
    drop = R.simplify_ref(v, f, cell=0.5, keep_unreferenced=False)
    assert drop.vertex_map.tolist() == [0, 2, 1, 0, -1] and drop.info["vertices"] == 3 and drop.info["unreferenced"] == 1
    assert np.array_equal(drop.vertices, res.vertices[:3]) and np.array_equal(drop.faces, res.faces)


def test_bad_vertices_and_their_faces():
    v = np.zeros((7, 4), np.float32)
    v[:, 0] = np.arange(7)
    v[1, 1] = np.nan
    v[2, 3] = np.inf
    v[3, 0] = 16384.0
    v[4, 0] = -np.float32(16384.0) + np.float32(2.0 ** -10)                             # the largest magnitude that passes
    f = np.array([[0, 5, 6], [0, 1, 5], [2, 5, 6], [3, 0, 6], [4, 5, 6]], np.int32)
    res = R.simplify_ref(v, f, cell=0.5)
    assert res.vertex_map.tolist() == [1, -1, -1, -1, 0, 2, 3]
    assert res.info == dict(vertices=4, faces=2, bad_vertices=3, bad_faces=3, collapsed=0, duplicates=0, unreferenced=0)
    assert res.face_source.tolist() == [0, 4] and res.faces.tolist() == [[1, 2, 3], [0, 2, 3]]
    _consistent(v, f, 0.5, "mean", True, res)


def test_nearest_picks_a_member_and_breaks_ties_by_index():
    v = np.array([[0.10, 0.1, 0.1, 7], [0.30, 0.1, 0.1, 8], [0.30, 0.1, 0.1, 9], [0.20, 0.1, 0.1, 1], [0.20, 0.1, 0.1, 2],
                  [0.6, 0.1, 0.1, 3], [0.6, 0.1, 0.1, 4], [1.125, 0.25, 0.25, 5], [1.375, 0.25, 0.25, 6]], np.float32)
    res = R.simplify_ref(v, np.zeros((0, 3), np.int32), cell=0.5, placement="nearest")
    # cell 0: the mean x is 0.22, the two vertices at 0.20 tie: the lower index.  cell 1: identical twins.  cell 2: 1.125 and 1.375 are
    # equidistant from their exact mean 1.25
    assert res.vertex_map.tolist() == [0, 0, 0, 0, 0, 1, 1, 2, 2]
    assert res.vertices.view(np.uint32).tolist() == v[[3, 5, 7]].view(np.uint32).tolist()
    assert res.info["vertices"] == 3 and res.info["unreferenced"] == 3 and res.faces.shape == (0, 3)


def test_cell_borders_signs_and_inexact_cells():
    for cell in (0.03, 0.04, 2.0 ** -6):
        inv = np.float32(1.0 / cell)
        x = np.array([0.0, -0.0, cell, -cell, np.float32(cell), -np.float32(cell), 3 * cell, -3 * cell, 16383.5, -16383.5], np.float32)
        v = np.stack([x, np.zeros_like(x), np.zeros_like(x)], axis=1)
        res = R.simplify_ref(v, np.zeros((0, 3), np.int32), cell=cell)
        k = np.floor(x * inv).astype(np.int64)
        assert k[0] == k[1] == 0 and res.vertex_map[0] == res.vertex_map[1]
        assert np.array_equal(res.vertex_map, np.unique(k, return_inverse=True)[1].reshape(-1))
        assert np.abs(k).max() < 1 << 20 or k.min() == -(1 << 20)
    # the mean of +0 and -0 is +0
    res = R.simplify_ref(np.array([[0.0, -0.0, 0.0], [-0.0, -0.0, 0.0]], np.float32), np.zeros((0, 3), np.int32))
    assert res.vertices.view(np.uint32).tolist() == [[0, 0, 0]]


def test_empty_inputs():
    e = R.simplify_ref(np.zeros((0, 6), np.float32), np.zeros((0, 3), np.int32))
    assert e.vertices.shape == (0, 6) and e.faces.shape == (0, 3) and e.vertex_map.shape == (0,) and not any(e.info.values())
    e = R.simplify_ref(np.zeros((0, 3), np.float32), np.array([[0, 1, 2]], np.int32))
    assert e.info["bad_faces"] == 1 and e.info["faces"] == 0


def test_set_property_and_speed():
    """A permutation of vertices and faces changes no vertex bit and no face as a set; 50 k vertices take well under a second."""
    v, f = K.box(92, 0.011, origin=(-0.5, -0.5, -0.5))                                  # 49 688 vertices, 99 372 faces
    assert len(v) > 49000
    rgb = np.random.default_rng(1).uniform(0, 255, (len(v), 3)).astype(np.float32)
    v = np.concatenate([v, rgb], axis=1)
    t0 = time.perf_counter()
    res = R.simplify_ref(v, f, cell=0.04)
    took = time.perf_counter() - t0
    assert took < 1.0, took
    _consistent(v, f, 0.04, "mean", True, res)
    v2, f2, _ = K.relabel(v, f, seed=3)
    res2 = R.simplify_ref(v2, f2, cell=0.04)
    assert np.array_equal(res.vertices.view(np.uint32), res2.vertices.view(np.uint32))
    assert {tuple(t) for t in res.faces} == {tuple(t) for t in res2.faces} and res.info == res2.info
