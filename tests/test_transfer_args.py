"""segdino3d_amd/transfer.py refuses bad arguments before anything touches a device, and refuses CPU tensors.  No GPU."""
import numpy as np
import pytest
import torch


def _index_shell(n_points=5, radius=0.1):
    """A PointIndex without its build: what the argument checks of its methods see.  (Its constructor needs a device.)"""
    from segdino3d_amd import transfer
    index = object.__new__(transfer.PointIndex)
    index.radius, index.n_points, index.device, index._ws = radius, n_points, torch.device("cpu"), torch.zeros(0, dtype=torch.uint8)
    return index


def _views_shell(K=0, H=4, W=6):
    """A lift2d.Views without its constructor (which needs a device), with K kept views."""
    from segdino3d_amd import lift2d
    views = object.__new__(lift2d.Views)
    views.kept, views.n_given, views.height, views.width, views.depth_scale = np.arange(K), K, H, W, 0.001
    views.depth = torch.zeros(K, H, W, dtype=torch.uint16)
    views.intrinsics, views.cam_to_world = torch.zeros(K, 4), torch.zeros(K, 3, 4)
    return views


def test_radius_outside_its_range():
    from segdino3d_amd import ops, transfer
    assert ops.KNN_MAX_RADIUS == 4.0 and ops.NEAREST_MAX_LABELS == 8
    pts = torch.zeros(3, 3)
    for radius in (0.0, -1.0, 4.0001, float("nan"), float("inf"), None, "1"):
        with pytest.raises(ValueError, match="radius"):
            transfer.PointIndex(pts, radius)
    for radius in (4.0, 2.0 ** -9):                      # the limits are inside: the next refusal is the device's
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            transfer.PointIndex(pts, radius)


def test_wrong_dtype_and_shape_before_the_device_is_asked():
    from segdino3d_amd import transfer
    with pytest.raises(TypeError, match="fp32"):
        transfer.PointIndex(torch.zeros(3, 3, dtype=torch.float64), 0.1)
    with pytest.raises(TypeError, match="tensor"):
        transfer.PointIndex(np.zeros((3, 3), np.float32), 0.1)
    for shape in ((3,), (3, 2), (2, 3, 3)):
        with pytest.raises(ValueError, match=r">= 3"):
            transfer.PointIndex(torch.zeros(shape), 0.1)
    index = _index_shell()
    with pytest.raises(TypeError, match="fp32"):
        index.nearest(torch.zeros(4, 3, dtype=torch.float16))
    with pytest.raises(ValueError, match=r">= 3"):
        index.nearest(torch.zeros(4, 2))
    with pytest.raises(TypeError, match="lift2d.Views"):
        index.nearest_pixels(torch.zeros(1, 4, 6))
    with pytest.raises(ValueError, match="near"):
        index.nearest_pixels(_views_shell(), near=2.0, far=1.0)
    with pytest.raises(ValueError, match="nothing to return"):
        index.nearest_pixels(_views_shell(), return_index=False)
    with pytest.raises(TypeError, match=r"unknown pixel-query parameter\(s\) \['stride'\]"):
        transfer.render_labels(_views_shell(), torch.zeros(3, 3), torch.zeros(3, dtype=torch.int32), 0.1, stride=2)


def test_label_channels_outside_1_to_8():
    index = _index_shell(n_points=5)
    q = torch.zeros(2, 3)
    for L in (0, 9):
        with pytest.raises(ValueError, match="1 <= L <= 8"):
            index.nearest(q, labels=torch.zeros(L, 5, dtype=torch.int32))
        with pytest.raises(ValueError, match="1 <= L <= 8"):
            index.nearest_pixels(_views_shell(), labels=torch.zeros(L, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\[N = 5\]"):
        index.nearest(q, labels=torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\[N = 5\]"):
        index.nearest(q, labels=torch.zeros(1, 2, 5, dtype=torch.int32))
    with pytest.raises(TypeError, match="int32, int64, uint8 or bool"):
        index.nearest(q, labels=torch.zeros(5))
    for fill in (1.5, 1 << 31, True):
        with pytest.raises(ValueError, match="fill"):
            index.nearest_pixels(_views_shell(), labels=torch.zeros(5, dtype=torch.int32), fill=fill)


def test_cpu_tensors_are_refused():
    from segdino3d_amd import ops, transfer
    index = _index_shell()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transfer.PointIndex(torch.zeros(3, 6), 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.nearest(torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.nearest(torch.zeros(2, 3), labels=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.nearest_pixels(_views_shell(K=1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transfer.transfer_labels(torch.zeros(3, 3), torch.zeros(3, dtype=torch.int32), torch.zeros(2, 3), 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        transfer.instance_map(torch.zeros(2, 5, dtype=torch.bool), torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.instance_map(torch.zeros(2, 5, dtype=torch.uint8), torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.point_index_build(torch.zeros(3, 3), 0.1)
    pred = dict(pts_semantic_mask=[torch.zeros(5), torch.zeros(5)], pts_instance_mask=[torch.zeros(2, 5, dtype=torch.bool), torch.zeros(5)],
                instance_labels=torch.zeros(2), instance_scores=torch.zeros(2))
    with pytest.raises(RuntimeError, match="to_host = False"):
        transfer.render_prediction(_views_shell(), torch.zeros(5, 3), pred, 0.1)


def test_instance_map_argument_checks():
    from segdino3d_amd import transfer
    with pytest.raises(TypeError, match="bool or uint8"):
        transfer.instance_map(torch.zeros(2, 5), torch.zeros(2))
    with pytest.raises(TypeError, match="fp32"):
        transfer.instance_map(torch.zeros(2, 5, dtype=torch.bool), torch.zeros(2, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"\[I, N\]"):
        transfer.instance_map(torch.zeros(2, 5, dtype=torch.bool), torch.zeros(3))
    with pytest.raises(ValueError, match=r"\[I, N\]"):
        transfer.instance_map(torch.zeros(5, dtype=torch.bool), torch.zeros(5))
    with pytest.raises(ValueError, match="NaN"):
        transfer.instance_map(torch.zeros(2, 5, dtype=torch.bool), torch.zeros(2), float("nan"))


def test_no_views_means_no_launch():
    """`len(views) == 0` returns empty tensors of the right shapes and dtypes without a launch: on this host a launch would raise."""
    index = _index_shell(n_points=5)
    views = _views_shell(K=0, H=4, W=6)
    idx = index.nearest_pixels(views)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (0, 4, 6)
    idx, d2, out = index.nearest_pixels(views, labels=torch.zeros(3, 5, dtype=torch.int64), return_d2=True)
    assert (idx.dtype, d2.dtype, out.dtype) == (torch.int32, torch.float32, torch.int32)
    assert tuple(idx.shape) == tuple(d2.shape) == (0, 4, 6) and tuple(out.shape) == (3, 0, 4, 6)
    out = index.nearest_pixels(views, labels=torch.zeros(5, dtype=torch.uint8), return_index=False)
    assert tuple(out.shape) == (0, 4, 6)
