"""tests/components_ref.py - the numpy restatement csrc/components.hip is pinned against - pinned itself: against brute-force
reachability (the boolean closure of the adjacency matrix) on small random graphs in all three link sources, and on hand-computed cases."""
import numpy as np
import pytest

import components_ref as R
import simplify_case as K

F32 = np.float32


def closure_labels(n, good, pairs):
    """Labels by brute force: reach = (I | A)^n over the good nodes, a component = a row of reach, numbered by smallest member."""
    reach = np.eye(n, dtype=bool)
    for a, b in pairs:
        reach[a, b] = reach[b, a] = True
    for _ in range(max(1, int(np.ceil(np.log2(max(n, 2)))))):
        reach = (reach.astype(np.int32) @ reach.astype(np.int32)) > 0
    labels = np.full(n, -1, np.int32)
    k = 0
    for i in range(n):
        if good[i] and labels[i] < 0:
            labels[reach[i] & good] = k
            k += 1
    return labels, k


def random_case(rng, source):
    n = int(rng.integers(1, 41))
    coords = rng.uniform(-2, 2, (n, int(rng.choice([3, 6, 11])))).astype(F32)
    for i in rng.choice(n, size=min(n, int(rng.integers(0, 4))), replace=False):
        coords[i, rng.integers(0, coords.shape[1])] = rng.choice([np.nan, np.inf, -np.inf, 16384.0, -16384.0])
    m = int(rng.integers(0, n + 3))
    if source == "table":
        links = rng.integers(-1, n, (n, int(rng.integers(1, 5)))).astype(np.int32)
        links[rng.random(links.shape) < 0.6] = -1
    else:
        links = rng.integers(0, n, (m, 3 if source == "faces" else 2)).astype(np.int32)
    if links.size and rng.random() < 0.5:
        links.reshape(-1)[rng.integers(0, links.size)] = rng.choice([n, -2, np.iinfo(np.int32).min])
    return n, coords, links


@pytest.mark.parametrize("source", ["faces", "edges", "table"])
@pytest.mark.parametrize("with_coords", [True, False])
def test_against_boolean_closure(source, with_coords):
    rng = np.random.default_rng({"faces": 1, "edges": 2, "table": 3}[source] + 10 * with_coords)
    for _ in range(60):
        n, coords, links = random_case(rng, source)
        coords = coords if with_coords else None
        got = R.components_ref(n, links, source, coords)
        good = np.ones(n, bool) if coords is None else (np.abs(np.nan_to_num(coords, nan=np.inf)) < 16384.0).all(axis=1)
        ends, skipped = R.link_ends(links, source, n)
        pairs, n_bad, link_label = [], 0, []
        for row, skip in zip(ends.tolist(), skipped.tolist()):
            if skip:
                continue
            if all(0 <= e < n and good[e] for e in row):
                pairs += [(row[j], row[j + 1]) for j in range(len(row) - 1)]
                link_label.append(row[0])
            else:
                n_bad += 1
        labels, k = closure_labels(n, good, pairs)
        assert np.array_equal(got.labels, labels) and got.info["components"] == k == len(got.n_nodes) == len(got.box)
        assert got.info["bad_links"] == n_bad and got.info["bad_nodes"] == int((~good).sum()) and got.info["unsettled"] == 0
        assert np.array_equal(got.n_nodes, np.bincount(labels[good], minlength=k))
        assert np.array_equal(got.n_links, np.bincount(labels[link_label], minlength=k) if link_label else np.zeros(k))
        in_link = np.zeros(n, bool)
        in_link[[e for p in pairs for e in p]] = True
        assert got.info["isolated"] == int((good & ~in_link).sum())
        # the defaults keep everything good
        assert got.keep.all() and got.info["kept"] == k and np.array_equal(got.node_map >= 0, good)
        assert np.array_equal(got.labels_out, labels[good])
        if coords is not None:
            assert np.array_equal(got.nodes.view(np.uint32), coords[good].view(np.uint32))
            for c in range(k):
                xyz = coords[labels == c][:, :3]
                assert np.array_equal(got.box[c, 0::2], xyz.min(axis=0)) and np.array_equal(got.box[c, 1::2], xyz.max(axis=0))
                assert got.extent[c] == (xyz.max(axis=0) - xyz.min(axis=0)).max()
        else:
            assert not got.box.any() and not got.extent.any() and got.nodes is None


TRI = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32)


def two_triangles(shared):
    """Two triangles sharing `shared` vertices (0, 1 or 2) -> (vertices, faces)."""
    second = np.array([[2, 2, 0], [3, 2, 0], [2, 3, 0]], F32)
    v = np.concatenate([TRI, second[shared:]])
    f = np.array([[0, 1, 2], list(range(shared)) + list(range(3, 6 - shared))], np.int32)
    return v, f


@pytest.mark.parametrize("shared, want", [(0, [0, 0, 0, 1, 1, 1]), (1, [0, 0, 0, 0, 0]), (2, [0, 0, 0, 0])])
def test_two_triangles(shared, want):
    v, f = two_triangles(shared)
    got = R.components_ref(len(v), f, "faces", v)
    assert got.labels.tolist() == want
    k = max(want) + 1
    assert got.info == dict(components=k, kept=k, nodes=len(v), links=2, bad_nodes=0, bad_links=0, isolated=0, unsettled=0)
    assert got.n_links.tolist() == ([1, 1] if k == 2 else [2]) and got.n_nodes.tolist() == ([3, 3] if k == 2 else [len(v)])
    assert np.array_equal(got.links, f) and got.link_source.tolist() == [0, 1] and got.node_map.tolist() == list(range(len(v)))
    if k == 2:
        assert got.box.tolist() == [[0, 1, 0, 1, 0, 0], [2, 3, 2, 3, 0, 0]] and got.extent.tolist() == [1, 1]
        only = R.components_ref(len(v), f, "faces", v, keep_largest=1)                  # equal n_links: the lower label stays
        assert only.keep.tolist() == [1, 0] and only.links.tolist() == [[0, 1, 2]] and only.node_map.tolist() == [0, 1, 2, -1, -1, -1]


def test_degenerate_faces_and_self_loops():
    v = np.zeros((5, 3), F32)
    v[:, 0] = np.arange(5)
    got = R.components_ref(5, np.array([[0, 1, 1], [3, 3, 3]], np.int32), "faces", v, min_links=1)
    assert got.labels.tolist() == [0, 0, 1, 2, 3] and got.n_links.tolist() == [1, 0, 1, 0] and got.n_nodes.tolist() == [2, 1, 1, 1]
    assert got.info["isolated"] == 2 and got.info["bad_links"] == 0                     # vertex 3 is in a good link: not isolated
    assert got.keep.tolist() == [1, 0, 1, 0] and got.links.tolist() == [[0, 1, 1], [2, 2, 2]] and got.node_map.tolist() == [0, 1, -1, 2, -1]
    assert got.labels_out.tolist() == [0, 0, 1]
    loop = R.components_ref(3, np.array([[1, 1], [2, 0]], np.int32), "edges")
    assert loop.labels.tolist() == [0, 1, 0] and loop.n_links.tolist() == [1, 1] and loop.info["isolated"] == 0


def test_signed_zero_box_and_exact_thresholds():
    v = np.array([[-0.0, 0.0, 0.0], [0.0, -0.0, 0.0], [0.0, 0.0, -0.0], [5, 5, 5], [5.25, 5, 5], [5, 5.125, 5]], F32)
    f = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    got = R.components_ref(6, f, "faces", v)
    bits = got.box.view(np.uint32)
    neg, pos = np.uint32(0x80000000), np.uint32(0)
    assert bits[0].tolist() == [neg, pos] * 3 and got.extent.tolist() == [0.0, 0.25]
    assert R.float_key(F32(-0.0)) < R.float_key(F32(0.0)) < R.float_key(F32(1e-45)) and R.float_key(F32(-1e-45)) < R.float_key(F32(-0.0))
    assert R.components_ref(6, f, "faces", v, min_extent=0.25).keep.tolist() == [0, 1]                 # equality passes
    assert R.components_ref(6, f, "faces", v, min_extent=float(np.nextafter(F32(0.25), F32(1)))).keep.tolist() == [0, 0]
    assert R.components_ref(6, f, "faces", v, min_extent=0.0).keep.tolist() == [1, 1]
    assert R.components_ref(6, f, "faces", v, min_nodes=3, min_links=1).keep.tolist() == [1, 1]
    assert R.components_ref(6, f, "faces", v, min_nodes=4).keep.tolist() == [0, 0]
    assert R.components_ref(6, f, "faces", v, min_links=2).keep.tolist() == [0, 0]


def test_keep_largest_order_and_ties():
    # components of 2, 3, 1, 3 links over nodes 0-2, 3-6, 7-8, 9-12 (paths)
    edges = np.array([[0, 1], [1, 2], [3, 4], [4, 5], [5, 6], [7, 8], [9, 10], [10, 11], [11, 12]], np.int32)
    assert R.components_ref(13, edges, "edges").n_links.tolist() == [2, 3, 1, 3]
    for m, want in [(1, [0, 1, 0, 0]), (2, [0, 1, 0, 1]), (3, [1, 1, 0, 1]), (4, [1, 1, 1, 1]), (9, [1, 1, 1, 1])]:
        assert R.components_ref(13, edges, "edges", keep_largest=m).keep.tolist() == want, m
    got = R.components_ref(13, edges, "edges", keep_largest=2, min_links=2)
    assert got.labels_out.tolist() == [0] * 4 + [1] * 4 and got.links.tolist() == [[0, 1], [1, 2], [2, 3], [4, 5], [5, 6], [6, 7]]
    assert got.link_source.tolist() == [2, 3, 4, 6, 7, 8] and got.info["links"] == 6 and got.info["kept"] == 2
    assert R.components_ref(13, edges, "edges", keep_largest=2, min_links=4).info["kept"] == 0         # the threshold comes first


def test_table_form_by_hand():
    pts = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [3, 0, 0], [4, 0, 0]], F32)
    nbr = np.array([[1, -1], [0, 2], [1, 3], [4, 7], [-1, -1]], np.int32)
    got = R.components_ref(5, nbr, "table", pts, min_nodes=2)
    # entries: (0,1) good, (1,0) good, (1,2) bad end, (2,1) and (2,3) bad row, (3,4) good, (3,7) out of range; three empty slots
    assert got.labels.tolist() == [0, 0, -1, 1, 1] and got.n_links.tolist() == [2, 1] and got.info["bad_links"] == 4
    assert got.links.tolist() == [[1, -1], [0, -1], [3, -1], [-1, -1]] and got.node_map.tolist() == [0, 1, -1, 2, 3] and got.link_source is None
    assert got.info == dict(components=2, kept=2, nodes=4, links=3, bad_nodes=1, bad_links=4, isolated=0, unsettled=0)


def test_numbering_follows_the_smallest_node_under_relabel():
    bv, bf = K.box(6, 0.25)
    pv, pf = K.plane(5, 0.25, origin=(5.0, 0.0, 0.0))
    v = np.concatenate([bv, pv, [[9, 9, 9], [8, 8, 8]]]).astype(F32)
    f = np.concatenate([bf, pf + len(bv)]).astype(np.int32)
    base = R.components_ref(len(v), f, "faces", v)
    assert base.info["components"] == 4 and base.info["isolated"] == 2
    for seed in (1, 2, 3):
        v2, f2, perm = K.relabel(v, f, seed)
        got = R.components_ref(len(v2), f2, "faces", v2)
        old = base.labels[perm]                                                          # the old component of each new vertex
        firsts = [int(np.flatnonzero(old == c)[0]) for c in range(4)]
        rank = np.argsort(np.argsort(firsts))                                            # old component -> its new number
        assert np.array_equal(got.labels, rank[old])
        assert np.array_equal(got.n_nodes[rank], base.n_nodes) and np.array_equal(got.n_links[rank], base.n_links)
        assert np.array_equal(got.box[rank].view(np.uint32), base.box.view(np.uint32))
