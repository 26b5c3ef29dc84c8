"""segdino3d_amd/fuse_views.py refuses bad parameters before anything touches a device.  No GPU."""
import pytest


def test_fuser_parameter_checks():
    from segdino3d_amd import fuse_views as fuse
    assert fuse.RULE_DEFAULTS == dict(near=0.1, far=6.0, stride=1, edge_abs=0.02, edge_rel=0.02, min_obs=2)
    f = fuse.PointCloudFuser()
    assert (f.voxel, f.capacity) == (0.02, 1 << 21)
    fuse.PointCloudFuser(voxel=2.0 ** -6, capacity=16, edge_rel=None, stride=4, min_obs=1)
    with pytest.raises(ValueError, match="voxel"):
        fuse.PointCloudFuser(voxel=2.0 ** -7)
    with pytest.raises(ValueError, match="voxel"):
        fuse.PointCloudFuser(voxel=float("nan"))
    for capacity in (0, 8, 1000, (1 << 21) + 1, 1 << 25):
        with pytest.raises(ValueError, match="capacity"):
            fuse.PointCloudFuser(capacity=capacity)
    with pytest.raises(TypeError, match=r"unknown fusion parameter\(s\) \['edge'\]"):
        fuse.PointCloudFuser(edge=0.1)
    for bad in (dict(stride=0), dict(stride=1.5), dict(min_obs=0), dict(near=-1.0), dict(near=2.0, far=1.0), dict(edge_abs=-0.1),
                dict(far=float("nan"))):
        with pytest.raises(ValueError):
            fuse.PointCloudFuser(**bad)


def test_the_module_does_not_shadow_the_optimizer_wrapper():
    """`segdino3d_amd.fuse(optimizer)` is the package's AdamW wrapper; a submodule named `fuse` would replace it on import."""
    import segdino3d_amd
    from segdino3d_amd import fuse_views, optim  # noqa: F401
    assert segdino3d_amd.fuse is optim.fuse and callable(segdino3d_amd.fuse)


def test_cpu_tensors_are_refused():
    import numpy as np
    import torch
    from segdino3d_amd import fuse_views as fuse, lift2d
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lift2d.Views(torch.zeros(1, 4, 6), np.ones((1, 4), np.float32), np.eye(4)[None])
    with pytest.raises(TypeError, match="lift2d.Views"):
        fuse.PointCloudFuser().add(None, torch.zeros(1, 4, 6, 3, dtype=torch.uint8))
