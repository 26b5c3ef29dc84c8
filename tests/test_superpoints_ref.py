"""The numpy restatement of the superpoint rule (tests/superpoints_ref.py) against expectations worked out by hand, and the batched
formulation the sweep kernel uses against the sequential one.  No device."""
import numpy as np
import pytest

import superpoints_case as case
import superpoints_ref as ref


def test_one_triangle_and_an_isolated_vertex():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], dtype=np.float32)
    r = ref.mesh_superpoints(v, np.array([[0, 1, 2]]), min_verts=1, debug=True)
    assert r.labels.tolist() == [0, 0, 0, 1] and r.count == 2 and r.bad_faces == 0
    assert np.array_equal(r.normals, np.array([[0, 0, 1]] * 3 + [[0, 0, 0]], dtype=np.float32))
    assert r.weights.tolist() == [0, 0, 0]
    # the default min_verts absorbs nothing more: the fourth vertex is attached by no edge
    assert ref.mesh_superpoints(v, np.array([[0, 1, 2]])).labels.tolist() == [0, 0, 0, 1]


def test_flat_grid_is_one_superpoint():
    v, f = case.flat_grid(60)
    r = ref.mesh_superpoints(v, f)
    assert r.count == 1 and not r.labels.any()


def test_right_angle_crease_splits_two_sheets():
    v, f = case.crease(8, 8)                                       # rows 0 .. 7 lie flat (the crease is row 7), rows 8 .. 14 go up
    r = ref.mesh_superpoints(v, f)
    lab = r.labels.reshape(15, 8)
    assert r.count == 2
    assert (lab[:7] == 0).all() and (lab[8:] == 1).all()           # each sheet has 56 vertices off the crease
    assert (lab[7] == lab[7, 0]).all()                             # the crease row goes to one side as a whole


def test_small_component_attached_by_an_edge_is_absorbed():
    v, f = case.grid_with_tail(True)
    assert ref.mesh_superpoints(v, f, min_verts=1).count > 1       # pass 1 alone keeps the fan apart
    r = ref.mesh_superpoints(v, f, min_verts=20)
    assert r.count == 1 and not r.labels.any()


def test_small_detached_component_stays():
    v, f = case.grid_with_tail(False)
    r = ref.mesh_superpoints(v, f, min_verts=20)
    assert (r.labels[:36] == 0).all() and (r.labels[36:] > 0).all()
    assert r.count == 1 + len(np.unique(r.labels[36:]))
    assert np.bincount(r.labels)[1:].max() < 20


def test_out_of_range_face_is_ignored_and_counted():
    v, f = case.flat_grid(8)
    want = ref.mesh_superpoints(v, f)
    bad = np.array([[0, 1, 64], [-1, 2, 3], [5, 6, 1 << 40]])
    got = ref.mesh_superpoints(v, np.concatenate([bad[:1], f, bad[1:]]), debug=True)
    assert got.bad_faces == 3 and want.bad_faces == 0
    assert np.array_equal(got.labels, want.labels) and got.count == want.count
    assert got.weights[:3].tolist() == [0, 0, 0]


def test_degenerate_faces_change_nothing():
    v, f = case.boxes_on_plane(24, 5)                              # row 0 is ground: vertices 0 .. 23 lie on one line
    want = ref.mesh_superpoints(v, f, debug=True)
    assert want.count > 1
    extra = np.array([[0, 1, 2], [5, 9, 20], [3, 3, 7], [9, 4, 4], [2, 2, 2]])      # two faces without area, three with a repeated index
    got = ref.mesh_superpoints(v, np.concatenate([extra, f]), debug=True)
    assert np.array_equal(got.normals, want.normals)               # they add nothing to a normal,
    assert np.array_equal(got.weights[15:], want.weights)
    assert np.array_equal(got.labels, want.labels) and got.count == want.count      # and their edges join what is joined anyway


def test_nan_and_inf_vertices_give_finite_weights_and_a_result():
    v, f = case.height_field(12, 6)
    v = v.copy()
    v[5] = np.nan
    v[40, 2] = np.inf
    v[77] = (-np.inf, np.inf, 3.0e38)
    v[100] = 3.0e38
    r = ref.mesh_superpoints(v, f, debug=True)
    w = r.weights.view(np.float32)
    assert np.isfinite(w).all() and (w >= 0).all() and (w <= 4).all()
    assert np.isfinite(r.normals).all()
    assert len(r.labels) == 144 and r.labels.max() == r.count - 1


def test_labels_are_dense_and_numbered_by_smallest_vertex():
    v, f = case.height_field(40, 1)
    r = ref.mesh_superpoints(v, f)
    assert r.count > 2
    assert np.array_equal(np.unique(r.labels), np.arange(r.count))
    first = [int(np.flatnonzero(r.labels == s)[0]) for s in range(r.count)]
    assert first == sorted(first) and first[0] == 0
    assert np.bincount(r.labels).min() >= 20
    labels, count = ref.labels_from_roots([3, 3, 2, 3, 2, 5])
    assert labels.tolist() == [0, 0, 1, 0, 1, 2] and count == 3


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_tie_order_matters_on_the_noise_free_case(seed):
    """Rule 4: among equal weights the lower edge index goes first.  Taking the higher index first changes the labels."""
    v, f = case.boxes_on_plane(80, seed)
    r = ref.mesh_superpoints(v, f, debug=True)
    assert len(np.unique(r.weights)) < 300 and len(r.weights) > 37000          # nearly every edge ties with another
    rev = ref.mesh_superpoints(v, f, reverse_ties=True)
    assert not np.array_equal(r.labels, rev.labels)


@pytest.mark.parametrize("batch", [64, 512])
def test_batched_sweep_equals_the_sequential_rule(batch):
    """The sweep kernel's formulation, written out in Python (superpoints_ref.sweep_batched), both passes."""
    for v, f in (case.height_field(40, 1), case.boxes_on_plane(40, 2), case.grid_with_tail(True)):
        for kw in (dict(), dict(min_verts=200), dict(k_thresh=0.0), dict(k_thresh=0.5, min_verts=1)):
            want = ref.mesh_superpoints(v, f, **kw)
            got = ref.mesh_superpoints(v, f, batch=batch, **kw)
            assert np.array_equal(want.labels, got.labels) and want.count == got.count


def test_batched_sweep_settles_a_minority_of_edges_in_the_table():
    v, f = case.height_field(40, 1)
    r = ref.mesh_superpoints(v, f, debug=True)
    a, b = ref.edge_ends(f)
    w, live = ref.edge_weights(v, f, r.normals)
    stats = []
    roots = ref.sweep_batched(len(v), a, b, w, live, r.order, float(np.float32(0.01)), 20, 512, stats)
    assert np.array_equal(ref.labels_from_roots(roots)[0], r.labels)
    assert len(v) - r.count <= stats[0] + stats[1] < len(a)        # every join is settled there, most edges are not
