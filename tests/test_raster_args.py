"""The argument checks of segdino3d_amd/raster.py that need no device: every one of them strikes before anything touches the HIP
runtime, so they run on CPU tensors here; a CPU tensor that passes them all is refused with "no CPU fallback"."""
import numpy as np
import pytest
import torch

from segdino3d_amd import ops, raster

V = torch.zeros(5, 3)
F = torch.zeros(4, 3, dtype=torch.int32)
INTR = np.array([[64, 64, 8, 8]] * 2, dtype=np.float32)
POSES = np.stack([np.eye(4)] * 2)


def render(vertices=V, faces=F, intrinsics=INTR, cam_to_world=POSES, height=16, width=16, **kw):
    return raster.render_mesh(vertices, faces, intrinsics, cam_to_world, height, width, **kw)


def test_constants_and_surface():
    assert ops.RASTER_INFO == ("drawn", "near", "guard", "empty", "bad", "pixels") and ops.RASTER_MAX_LABELS == 8
    assert isinstance(ops.RASTER_SMALL_MAX_PIXELS, int) and ops.RASTER_SMALL_MAX_PIXELS >= 1
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "segdino3d_hip.h")).read()
    assert int(re.search(r"#define SD3D_RASTER_SMALL_MAX_PIXELS (\d+)", header).group(1)) == ops.RASTER_SMALL_MAX_PIXELS
    assert int(re.search(r"#define SD3D_RASTER_MAX_LABELS (\d+)", header).group(1)) == ops.RASTER_MAX_LABELS
    assert int(re.search(r"#define SD3D_RASTER_INFO_WORDS (\d+)", header).group(1)) == len(ops.RASTER_INFO)


@pytest.mark.parametrize("kw, exc, match", [
    (dict(vertices=np.zeros((5, 3), np.float32)), TypeError, "render_mesh: vertices: expected a tensor"),
    (dict(vertices=V.double()), TypeError, "render_mesh: vertices must be fp32"),
    (dict(vertices=torch.zeros(5, 2)), ValueError, "render_mesh: vertices must be"),
    (dict(vertices=torch.zeros(5)), ValueError, "render_mesh: vertices must be"),
    (dict(faces=[[0, 1, 2]]), TypeError, "render_mesh: faces: expected a tensor"),
    (dict(faces=F.long()), TypeError, "render_mesh: faces must be int32"),
    (dict(faces=torch.zeros(4, 4, dtype=torch.int32)), ValueError, r"render_mesh: faces must be \[F, 3\]"),
    (dict(faces=torch.zeros(12, dtype=torch.int32)), ValueError, r"render_mesh: faces must be \[F, 3\]"),
])
def test_mesh_dtypes_and_shapes(kw, exc, match):
    with pytest.raises(exc, match=match):
        render(**kw)


@pytest.mark.parametrize("kw, exc", [
    (dict(near=0.0), ValueError), (dict(near=-0.1), ValueError), (dict(near=float("nan")), ValueError),
    (dict(near=1.0, far=0.5), ValueError), (dict(far=float("nan")), ValueError), (dict(near="0.1"), TypeError),
    (dict(near=True), TypeError),
])
def test_depth_range(kw, exc):
    with pytest.raises(exc, match="render_mesh: "):
        render(**kw)


@pytest.mark.parametrize("kw", [dict(height=0), dict(width=0), dict(height=16385), dict(width=16385), dict(height=-3)])
def test_image_size_out_of_range(kw):
    with pytest.raises(ValueError, match="render_mesh: (height|width) must lie in 1 .. 16384"):
        render(**kw)
    with pytest.raises(TypeError, match="render_mesh: height must be an integer"):
        render(height=16.0)


def test_views():
    with pytest.raises(ValueError, match=r"cam_to_world must be \[V, 4, 4\]"):
        render(cam_to_world=np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match=r"render_mesh: intrinsics must be fp32 \[V = 2, 4\]"):
        render(intrinsics=INTR[:1])
    with pytest.raises(ValueError, match="render_mesh: intrinsics must be fp32"):
        render(intrinsics=torch.zeros(2, 4, dtype=torch.float64))
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="render_mesh: views_per_pass must be an integer >= 1"):
            render(views_per_pass=bad)


def test_labels():
    with pytest.raises(ValueError, match=r"render_mesh: face_labels must be \[F = 4\] or \[L, F\]"):
        render(face_labels=torch.zeros(2, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"render_mesh: vertex_labels must be \[Nv = 5\] or \[L, Nv\]"):
        render(vertex_labels=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"render_mesh: vertex_labels must be"):
        render(vertex_labels=torch.zeros(1, 2, 5, dtype=torch.int32))
    with pytest.raises(TypeError, match="render_mesh: face_labels must be int32, int64, uint8 or bool"):
        render(face_labels=torch.zeros(4))
    with pytest.raises(TypeError, match="render_mesh: vertex_labels: expected a tensor"):
        render(vertex_labels=np.zeros(5, np.int32))
    with pytest.raises(ValueError, match="render_mesh: 1 <= L <= 8 channels of face_labels"):
        render(face_labels=torch.zeros(9, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="render_mesh: 1 <= L <= 8 channels of vertex_labels"):
        render(vertex_labels=torch.zeros(0, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match="render_mesh: at most 8 label channels in one call, got 9"):
        render(face_labels=torch.zeros(4, 4, dtype=torch.int32), vertex_labels=torch.zeros(5, 5, dtype=torch.int64))
    for fill in (1 << 31, -(1 << 31) - 1, 0.5, True):
        with pytest.raises(ValueError, match="render_mesh: fill must be an integer that fits int32"):
            render(fill=fill)
    with pytest.raises(ValueError, match="render_mesh: nothing to return"):
        render(return_depth=False, return_face=False)


def test_unknown_rule_parameters():
    with pytest.raises(TypeError, match="unexpected keyword argument 'nearr'"):
        render(nearr=0.2)
    with pytest.raises(TypeError, match=r"rendered_views: unknown rule parameter\(s\) \['tol_abs'\]; known: \['far', 'near', 'views_per_pass'\]"):
        raster.rendered_views(V, F, INTR, POSES, 16, 16, tol_abs=0.1)
    with pytest.raises(TypeError, match=r"render_prediction_mesh: unknown rule parameter\(s\) \['radius'\]"):
        raster.render_prediction_mesh(V, F, INTR, POSES, 16, 16, {}, radius=0.1)
    with pytest.raises(ValueError, match="render_mesh: need 0 < near <= far"):
        raster.rendered_views(V, F, INTR, POSES, 16, 16, near=0.0)


def test_cpu_tensors_are_refused():
    """Everything else in order: the device is what is missing."""
    with pytest.raises(RuntimeError, match="render_mesh: vertices: expected a tensor on the HIP device, got cpu \\(no CPU fallback\\)"):
        render()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render(face_labels=torch.zeros(4, dtype=torch.int64), vertex_labels=torch.zeros(2, 5, dtype=torch.bool), fill=-7, return_vertex=True,
               views_per_pass=1, near=0.5, far=0.5, cam_to_world=torch.from_numpy(POSES), intrinsics=torch.from_numpy(INTR))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        raster.rendered_views(V, F, INTR, POSES, 16, 16)
    pred = dict(pts_semantic_mask=[torch.zeros(5, dtype=torch.int64)] * 2, pts_instance_mask=[torch.zeros(2, 5, dtype=torch.bool)] * 2,
                instance_labels=torch.zeros(2, dtype=torch.int64), instance_scores=torch.zeros(2))
    with pytest.raises(RuntimeError, match="render_prediction_mesh: pts_semantic_mask: expected tensors on the HIP device"):
        raster.render_prediction_mesh(V, F, INTR, POSES, 16, 16, pred)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.raster_views(V, F, torch.zeros(2, 3, 4), torch.zeros(2, 4), 16, 16)
