"""bench.py --dump-outputs: what the last timed step returned, as float32 / float64 .npy files under 64 MB (host tensors stand in
for the device outputs of the benchmark's forward: 150 k points, topk_insts = 600 instance rows)."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _point_data(seed, n_points=150_000, n_inst=600):
    from segdino3d_amd import PointData
    g = torch.Generator().manual_seed(seed)
    masks = torch.rand(n_inst, n_points, generator=g) < 0.05
    sem = torch.randint(0, 200, (n_points,), generator=g)
    return PointData(pts_semantic_mask=[sem, sem.clone()], pts_instance_mask=[masks, torch.randint(0, 50, (n_points,), generator=g)],
                     instance_labels=torch.randint(0, 200, (n_inst,), generator=g), instance_scores=torch.rand(n_inst, generator=g),
                     sort_and_mask=(torch.randperm(n_inst, generator=g), torch.rand(n_inst, generator=g) > 0.5,
                                    torch.rand(n_inst, generator=g) > 0.5),
                     instance_boxes=torch.rand(n_inst, 6, generator=g))


def test_dump_outputs_are_float_arrays_under_64mb(tmp_path):
    bench = _bench()
    pd = _point_data(0)
    shapes = bench.dump_outputs(pd, str(tmp_path / "a"))
    total = 0
    for name, shape in shapes.items():
        a = np.load(tmp_path / "a" / (name + ".npy"))
        assert a.dtype in (np.float32, np.float64) and a.shape == shape and a.size, (name, a.dtype, a.shape)
        total += a.nbytes
    assert total <= 64 << 20, total
    masks = pd.pts_instance_mask[0].numpy()
    cols = np.load(tmp_path / "a" / "instance_masks_sample_points.npy").astype(np.int64)
    assert len(cols) == bench.DUMP_MASK_POINTS and np.all(np.diff(cols) > 0)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "instance_masks_sample.npy"), masks[:, cols])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "instance_mask_points.npy"), masks.sum(axis=1))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "semantic_mask.npy"), pd.pts_semantic_mask[0].numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "instance_scores.npy"), pd.instance_scores.numpy())
    # the sampled points are fixed: a second dump of the same outputs is byte-identical
    bench.dump_outputs(pd, str(tmp_path / "b"))
    for name in shapes:
        assert (tmp_path / "a" / (name + ".npy")).read_bytes() == (tmp_path / "b" / (name + ".npy")).read_bytes(), name


def test_dump_outputs_of_an_empty_selection(tmp_path):
    """The benchmark's random weights keep no instance in its scenes: the per-instance fields have no rows.  No written file is
    empty, `instance_count` says 0, and the per-instance files of an earlier dump into the same directory are gone."""
    bench = _bench()
    bench.dump_outputs(_point_data(1, n_points=1000, n_inst=7), str(tmp_path))
    pd = _point_data(2, n_points=1000, n_inst=0)
    pd.sort_and_mask = (torch.arange(600) // 3, torch.zeros(600, dtype=torch.bool), torch.zeros(0, dtype=torch.bool))
    shapes = bench.dump_outputs(pd, str(tmp_path))
    assert sorted(shapes) == ["instance_count", "panoptic_instance_mask", "panoptic_semantic_mask", "score_mask", "semantic_mask",
                              "sort_idx"], shapes
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(name + ".npy" for name in shapes)
    assert all(np.load(p).size for p in tmp_path.iterdir())
    assert np.load(tmp_path / "instance_count.npy").tolist() == [0.0]


def test_dump_outputs_without_boxes(tmp_path):
    pd = _point_data(1, n_points=1000, n_inst=7)
    pd.instance_boxes = None
    shapes = _bench().dump_outputs(pd, str(tmp_path))
    assert "instance_boxes" not in shapes and shapes["instance_masks_sample"] == (7, 1000)
    assert np.load(tmp_path / "instance_count.npy").tolist() == [7.0]
