"""tests/transfer_ref.py, the numpy restatement the nearest-point kernels are pinned against, held against independent statements of
the same thing.  No GPU.

Bounds.  None: every comparison is equality, or a count that must be zero.  Where a figure was measured it is noted as a comment; the
assertion is the condition, not the figure."""
import numpy as np
import pytest

import fuse_views_case as FK
import fuse_views_ref as FR
import transfer_case as K
import transfer_ref as T


def test_float32_rule_names_the_float64_nearest():
    """The fixed fp32 operation order is not a different answer: on 8 000 queries against 4 000 points the rule names the index a
    float64 evaluation names, for every query.  (Measured: 0 of 8 000 differ; 71 % of the queries have a hit.)"""
    p, q, r = K.agreement_case()
    idx, d2 = T.nearest(p, q, r)
    want = T.nearest_f64(p, q, r)
    assert idx.shape == (8000,) and np.array_equal(idx.astype(np.int64), want)
    assert 0.6 < (idx >= 0).mean() < 0.8
    hit = idx >= 0
    assert np.all(np.isinf(d2[~hit])) and np.all(d2[hit] <= np.float32(np.float32(r) * np.float32(r)))


def test_prefilter_is_the_brute_force():
    """The box prefilter of `nearest` only skips pairs that cannot be candidates: same idx and the same d2 bits as all pairs."""
    for p, q, r in (K.agreement_case(), K.lattice_case()):
        a, b = T.nearest(p, q, r, prefilter=True), T.nearest(p, q, r, prefilter=False)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    p, q, r = K.lattice_case()
    a, b = T.nearest(p, q, r, reverse_ties=True), T.nearest(p, q, r, reverse_ties=True, prefilter=False)
    assert np.array_equal(a[0], b[0])


def test_ties_go_to_the_lower_index_and_the_order_matters():
    p, q, r = K.lattice_case()
    idx, d2 = T.nearest(p, q, r)
    hit = np.flatnonzero(idx >= 0)
    assert len(hit) > 2000
    # every point at the winning distance has an index >= the winner's: checked directly, in float64 (lattice distances are exact)
    d = ((p[None, :, :].astype(np.float64) - q[hit, None, :].astype(np.float64)) ** 2).sum(axis=2)
    first = np.array([np.flatnonzero(row == row.min())[0] for row in d])
    assert np.array_equal(first, idx[hit])
    assert np.array_equal(d.min(axis=1).astype(np.float32), d2[hit])
    other, d2_other = T.nearest(p, q, r, reverse_ties=True)
    assert np.array_equal(d2_other.view(np.uint32), d2.view(np.uint32))              # the same distance ...
    assert (other != idx).sum() > 0                                                   # ... from another point: the order is part of the rule
    assert np.all(other[hit] >= idx[hit])


def test_validity_and_empty_inputs():
    p = np.array([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [16384.0, 0, 0], [0, 0, 0]], dtype=np.float32)
    q = np.array([[0, 0, 0], [np.nan, 0, 0], [0, -np.inf, 0], [0, 0, -16384.0], [16383.5, 0, 0]], dtype=np.float32)
    for pre in (True, False):
        idx, d2 = T.nearest(p, q, 4.0, prefilter=pre)
        assert idx.tolist() == [0, -1, -1, -1, -1] and d2[0] == 0 and np.all(np.isinf(d2[1:]))
        idx, _ = T.nearest(np.zeros((0, 3), np.float32), q, 1.0, prefilter=pre)
        assert idx.tolist() == [-1] * 5
        assert T.nearest(p, np.zeros((0, 3), np.float32), 1.0, prefilter=pre)[0].shape == (0,)
    near_limit = np.array([[16383.0, 0, 0]], dtype=np.float32)
    assert T.nearest(near_limit, q, 1.0)[0].tolist() == [-1, -1, -1, -1, 0]


def test_take_labels_and_instance_map():
    lab = np.array([[5, -1, 7], [1, 2, 3]])
    idx = np.array([[2, -1], [0, 1]])
    assert T.take_labels(lab, idx, fill=-7).tolist() == [[[7, -7], [5, -1]], [[3, -7], [1, 2]]]
    assert T.take_labels(lab[0], idx).tolist() == [[7, -1], [5, -1]]
    masks = np.array([[1, 1, 0, 0], [1, 0, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0]], dtype=bool)
    scores = np.array([0.5, 0.7, 0.7, np.nan], dtype=np.float32)
    assert T.instance_map(masks, scores, 0.0).tolist() == [1, 2, 1, -1]               # equal scores: the lower i; the NaN never wins
    assert T.instance_map(masks, scores, np.float32(0.7)).tolist() == [1, 2, 1, -1]   # a threshold exactly at a score keeps it
    assert T.instance_map(masks, scores, 0.71).tolist() == [-1, -1, -1, -1]
    assert T.instance_map(masks[:0], scores[:0]).tolist() == [-1] * 4


def test_pixel_queries_are_the_fusion_observations():
    """`pixel_queries` with the fusion's own depth rule and no edge test is `fuse_views_ref.observations` pixel for pixel."""
    c = FK.noisy(24, 32, V=3)
    c2w, kept = FR.cam_to_world(c["poses"])
    obs = FR.observations(c["depth_u16"], FK.DEPTH_SCALE, c["intr"], c2w, c["colors"], edge_rel=None)
    w, ok = T.pixel_queries(c["depth_u16"], FK.DEPTH_SCALE, c["intr"], c2w)
    assert obs["out_of_range"] == 0 and int(ok.sum()) == len(obs["w"])
    assert np.array_equal(w[obs["view"], obs["vi"], obs["ui"]].view(np.uint32), obs["w"].view(np.uint32))
    assert not ok[c["depth_u16"] == 0].any() and np.isnan(w[~ok]).all()
    assert not T.pixel_queries(c["depth_u16"], FK.DEPTH_SCALE, c["intr"], c2w, far=1.0)[1][c["depth_u16"] > 1000].any()


@pytest.mark.parametrize("voxel", [0.02, 0.05])
def test_every_observation_of_the_room_finds_a_point(voxel):
    """Coverage: fuse the room with min_obs = 1 and no edge test; at radius = 2 voxels every observation the fusion made finds a point
    (a pixel lies in its cell, and so does the cell's mean: at most a cell's diagonal, 1.74 voxels, apart).  (Measured on a
    6 000-pixel sample: no miss at 1.75 and at 2 voxels, largest distance 0.68 voxels.)  The condition: zero misses over ALL
    observations."""
    c = FK.room_case()
    points, fused = K.room_cloud(voxel)
    c2w, kept = FR.cam_to_world(c["poses"])
    obs = FR.observations(c["depth_u16"], FK.DEPTH_SCALE, c["intr"], c2w, c["colors"], voxel=voxel, min_obs=1, edge_rel=None)
    assert len(obs["w"]) == fused["pixels_used"] > 100000
    idx, d2 = T.nearest(points, obs["w"], 2.0 * voxel)
    assert int((idx < 0).sum()) == 0
    assert float(np.sqrt(d2.max())) < 1.75 * voxel
