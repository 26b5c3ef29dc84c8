"""The argument checks of segdino3d_amd/simplify.py that need no device: every one of them strikes before anything touches the HIP
runtime, so they run on CPU tensors here; a CPU tensor that passes them all is refused with "no CPU fallback"."""
import os
import re

import numpy as np
import pytest
import torch

from segdino3d_amd import ops, simplify

V = torch.zeros(5, 6)
F = torch.zeros(4, 3, dtype=torch.int32)


def run(vertices=V, faces=F, **kw):
    return simplify.simplify_mesh(vertices, faces, **kw)


def test_constants_and_surface():
    assert ops.SIMPLIFY_INFO == ("vertices", "faces", "bad_vertices", "bad_faces", "collapsed", "duplicates", "unreferenced")
    assert simplify.SimplifyInfo._fields == ops.SIMPLIFY_INFO
    assert simplify.SimplifiedMesh._fields == ("vertices", "faces", "vertex_map", "face_source")
    assert ops.SIMPLIFY_MAX_CHANNELS == 11 and simplify.MIN_CELL == 2.0 ** -6 and ops.SIMPLIFY_MAX_INV_CELL == 1.0 / simplify.MIN_CELL
    assert ops.SIMPLIFY_MAX_CELLS == 1 << 21
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "segdino3d_hip.h")).read()
    assert int(re.search(r"#define SD3D_SIMPLIFY_INFO_WORDS (\d+)", header).group(1)) == len(ops.SIMPLIFY_INFO) == 7
    assert int(re.search(r"#define SD3D_SIMPLIFY_MAX_CHANNELS (\d+)", header).group(1)) == ops.SIMPLIFY_MAX_CHANNELS
    assert int(re.search(r"#define SD3D_ABI_VERSION (\d+)", header).group(1)) == 25


@pytest.mark.parametrize("kw, exc, match", [
    (dict(vertices=np.zeros((5, 3), np.float32)), TypeError, "simplify_mesh: vertices: expected a tensor"),
    (dict(vertices=V.double()), TypeError, "simplify_mesh: vertices must be fp32"),
    (dict(vertices=V.half()), TypeError, "simplify_mesh: vertices must be fp32"),
    (dict(vertices=torch.zeros(5)), ValueError, r"simplify_mesh: vertices must be \[V, C\]"),
    (dict(vertices=torch.zeros(5, 3, 1)), ValueError, r"simplify_mesh: vertices must be \[V, C\]"),
    (dict(faces=[[0, 1, 2]]), TypeError, "simplify_mesh: faces: expected a tensor"),
    (dict(faces=F.long()), TypeError, "simplify_mesh: faces must be int32"),
    (dict(faces=torch.zeros(4, 4, dtype=torch.int32)), ValueError, r"simplify_mesh: faces must be \[F, 3\]"),
    (dict(faces=torch.zeros(12, dtype=torch.int32)), ValueError, r"simplify_mesh: faces must be \[F, 3\]"),
])
def test_mesh_dtypes_and_shapes(kw, exc, match):
    with pytest.raises(exc, match=match):
        run(**kw)


@pytest.mark.parametrize("C", [0, 1, 2, 12, 64])
def test_channels_out_of_range(C):
    with pytest.raises(ValueError, match=r"simplify_mesh: vertices must be \[V, C\] with 3 <= C <= 11"):
        run(vertices=torch.zeros(5, C))
    with pytest.raises(ValueError, match="simplify_mesh: vertices must be fp32 \\[V, C\\] with 3 <= C <= 11"):
        ops.simplify_mesh(torch.zeros(5, C), F, 25.0)


@pytest.mark.parametrize("cell", [float("nan"), 0.0, -0.04, 2.0 ** -7, 0.0156, float("inf"), -float("inf")])
def test_cell_out_of_range(cell):
    with pytest.raises(ValueError, match=r"simplify_mesh: cell must be finite and >= 2\^-6"):
        run(cell=cell)


def test_cell_type_and_ops_inv_cell():
    for bad in ("0.04", True, None, torch.tensor(0.04)):
        with pytest.raises(TypeError, match="simplify_mesh: cell must be a number"):
            run(cell=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="simplify_mesh: inv_cell must be positive and finite"):
            ops.simplify_mesh(V, F, bad)
    with pytest.raises(ValueError, match="simplify_mesh: inv_cell must be at most 64"):
        ops.simplify_mesh(V, F, 64.5)


def test_placement_and_flags():
    for bad in ("median", "Mean", "", None, 0):
        with pytest.raises(ValueError, match=r"simplify_mesh: placement must be one of \('mean', 'nearest'\)"):
            run(placement=bad)
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match="simplify_mesh: keep_unreferenced must be a bool"):
            run(keep_unreferenced=bad)
    with pytest.raises(TypeError, match="unexpected keyword argument 'target_vertices'"):
        run(target_vertices=1000)


def test_carry_back_on_the_host():
    """Plain torch indexing: it runs wherever its tensors are."""
    small = torch.tensor([[1.0, 2.0], [3.0, 4.0]])
    vmap = torch.tensor([1, -1, 0, 1], dtype=torch.int32)
    assert simplify.carry_back(small, vmap, -7.0).tolist() == [[3.0, 4.0], [-7.0, -7.0], [1.0, 2.0], [3.0, 4.0]]
    labels = torch.tensor([5, 9], dtype=torch.int64)
    assert simplify.carry_back(labels, vmap, -1).tolist() == [9, -1, 5, 9]
    assert simplify.carry_back(labels[:0], torch.full((3,), -1, dtype=torch.int32), -1).tolist() == [-1, -1, -1]
    assert simplify.carry_back(labels, vmap[:0], -1).shape == (0,)
    with pytest.raises(ValueError, match="carry_back: vertex_map must be int32 or int64"):
        simplify.carry_back(labels, vmap.float(), -1)
    with pytest.raises(TypeError, match="carry_back: values_small and vertex_map must be tensors"):
        simplify.carry_back([1, 2], vmap, -1)


def test_cpu_tensors_are_refused():
    """Everything else in order: the device is what is missing."""
    with pytest.raises(RuntimeError, match="simplify_mesh: vertices: expected a tensor on the HIP device, got cpu \\(no CPU fallback\\)"):
        run()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        run(vertices=torch.zeros(0, 11), faces=torch.zeros(0, 3, dtype=torch.int32), cell=2.0 ** -6, placement="nearest",
            keep_unreferenced=False, return_info=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.simplify_mesh(torch.zeros(5, 3), F, 25.0, nearest=True, keep_unreferenced=False)
