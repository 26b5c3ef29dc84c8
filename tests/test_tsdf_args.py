"""Argument checks of segdino3d_amd/tsdf.py and of the tsdf operators that run before anything reaches the device.  No GPU."""
import numpy as np
import pytest
import torch


def test_volume_arguments():
    from segdino3d_amd import tsdf
    for voxel in (2.0 ** -7, 0.0, -0.02, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel"):
            tsdf.TsdfVolume(voxel=voxel, trunc=4 * voxel if voxel == voxel else 0.08)
    for trunc in (0.019, 0.17, float("nan")):                                          # below a voxel, beyond a block
        with pytest.raises(ValueError, match=r"voxel <= trunc <= 8 \* voxel"):
            tsdf.TsdfVolume(voxel=0.02, trunc=trunc)
    tsdf.TsdfVolume(voxel=0.02, trunc=0.02)
    tsdf.TsdfVolume(voxel=0.02, trunc=0.16)
    for capacity in (0, 8, 1000, 1 << 21, 64.5):
        with pytest.raises(ValueError, match="capacity"):
            tsdf.TsdfVolume(capacity=capacity)
    with pytest.raises(TypeError, match=r"unknown TSDF parameter\(s\) \['min_obs', 'stride'\]"):
        tsdf.TsdfVolume(stride=2, min_obs=2)
    for bad in (dict(min_weight=0), dict(min_weight=1.5), dict(near=-1.0), dict(near=2.0, far=1.0), dict(edge_abs=-0.01)):
        with pytest.raises(ValueError):
            tsdf.TsdfVolume(**bad)
    v = tsdf.TsdfVolume(edge_rel=None, min_weight=3)
    assert v.rule["edge_rel"] is None and v.rule["min_weight"] == 3 and v.capacity == 1 << 16 and v.voxel == 0.02 and v.trunc == 0.08


def test_view_cap_follows_from_the_widths():
    """|q| <= 4097 and a colour byte <= 255 per view: MAX_VIEWS views keep every 32-bit sum of a voxel."""
    from segdino3d_amd import tsdf
    assert tsdf.MAX_VIEWS * 4097 < 2 ** 30 and tsdf.MAX_VIEWS * 255 < 2 ** 31
    for trunc in (0.02, 0.08, 0.125, 0.16, 1.0 / 3.0):
        assert abs(float(np.float32(trunc)) * float(np.float32(4096.0 / trunc))) < 4097


def test_cpu_tensors_are_refused():
    from segdino3d_amd import lift2d, ops, tsdf
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tsdf_workspace(64, "cpu")
    with pytest.raises(ValueError, match="capacity"):
        ops.tsdf_workspace(100, "cpu")
    views = object.__new__(lift2d.Views)                                               # a Views needs the device; `add` looks at the colours first
    views.n_given, views.kept = 1, np.arange(1)
    vol = tsdf.TsdfVolume()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vol.add(views, torch.zeros(1, 4, 6, 3, dtype=torch.uint8))
    with pytest.raises(TypeError, match="lift2d.Views"):
        vol.add(np.zeros((1, 4, 6)), torch.zeros(1, 4, 6, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tsdf_mesh(torch.zeros(1 << 20, dtype=torch.uint8), 16, 1, 0.02, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tsdf_touch(torch.zeros(1, 4, 6), None, torch.zeros(1, 4), torch.zeros(1, 3, 4), torch.zeros(64, dtype=torch.uint8), 16, 50.0, 0.04)
    assert vol.n_views == 0
