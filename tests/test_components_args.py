"""The argument checks of segdino3d_amd/components.py that need no device: every one of them strikes before anything touches the HIP
runtime, so they run on CPU tensors here; a CPU tensor that passes them all is refused with "no CPU fallback"."""
import os
import re

import numpy as np
import pytest
import torch

from segdino3d_amd import _lib, components, ops

V = torch.zeros(5, 6)
F = torch.zeros(4, 3, dtype=torch.int32)
E = torch.zeros(4, 2, dtype=torch.int32)
NBR = torch.zeros(5, 8, dtype=torch.int32)
HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "segdino3d_hip.h")).read()


def test_constants_and_surface():
    assert ops.COMPONENTS_INFO == ("components", "kept", "nodes", "links", "bad_nodes", "bad_links", "isolated", "unsettled")
    assert components.ComponentsInfo._fields == ops.COMPONENTS_INFO
    assert components.Components._fields == ("labels", "n_nodes", "n_links", "box")
    assert components.CleanedMesh._fields == ("vertices", "faces", "vertex_map", "face_source", "labels")
    assert components.CleanedPoints._fields == ("points", "point_map", "labels", "neighbours")
    assert int(re.search(r"#define SD3D_COMPONENTS_INFO_WORDS (\d+)", HEADER).group(1)) == len(ops.COMPONENTS_INFO) == 8
    assert int(re.search(r"#define SD3D_COMPONENTS_MAX_CHANNELS (\d+)", HEADER).group(1)) == ops.COMPONENTS_MAX_CHANNELS == ops.SIMPLIFY_MAX_CHANNELS
    for i, name in enumerate(ops.COMPONENTS_SOURCES):
        assert int(re.search(rf"#define SD3D_COMPONENTS_{name.upper()} (\d+)", HEADER).group(1)) == i
    assert int(re.search(r"#define SD3D_ABI_VERSION (\d+)", HEADER).group(1)) == 25 == _lib.ABI_VERSION
    for name in ("sd3d_components_ws_bytes", "sd3d_components"):
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\s*\(", HEADER)


CALLS = {
    "mesh_components": lambda **kw: components.mesh_components(**{**dict(vertices=V, faces=F), **kw}),
    "clean_mesh": lambda **kw: components.clean_mesh(**{**dict(vertices=V, faces=F), **kw}),
    "graph_components": lambda **kw: components.graph_components(**{**dict(n=5, edges=E), **kw}),
    "neighbour_components": lambda **kw: components.neighbour_components(**{**dict(points=V, nbr=NBR), **kw}),
    "clean_points": lambda **kw: components.clean_points(**{**dict(points=V), **kw}),
}


@pytest.mark.parametrize("who, name", [("mesh_components", "vertices"), ("clean_mesh", "vertices"), ("neighbour_components", "points"),
                                       ("clean_points", "points")])
def test_node_tensors(who, name):
    call = CALLS[who]
    with pytest.raises(TypeError, match=f"{who}: {name}: expected a tensor"):
        call(**{name: np.zeros((5, 3), np.float32)})
    for bad in (V.double(), V.half(), V.int()):
        with pytest.raises(TypeError, match=f"{who}: {name} must be fp32"):
            call(**{name: bad})
    for bad in (torch.zeros(5), torch.zeros(5, 3, 1), torch.zeros(5, 2), torch.zeros(5, 12), torch.zeros(5, 0)):
        with pytest.raises(ValueError, match=rf"{who}: {name} must be \[N, C\] with 3 <= C <= 11"):
            call(**{name: bad})


@pytest.mark.parametrize("who", ["mesh_components", "clean_mesh"])
def test_faces(who):
    call = CALLS[who]
    with pytest.raises(TypeError, match=f"{who}: faces: expected a tensor"):
        call(faces=[[0, 1, 2]])
    with pytest.raises(TypeError, match=f"{who}: faces must be int32"):
        call(faces=F.long())
    for bad in (torch.zeros(4, 4, dtype=torch.int32), torch.zeros(12, dtype=torch.int32)):
        with pytest.raises(ValueError, match=rf"{who}: faces must be \[F, 3\]"):
            call(faces=bad)


def test_edges_and_n():
    call = CALLS["graph_components"]
    with pytest.raises(TypeError, match="graph_components: edges: expected a tensor"):
        call(edges=np.zeros((4, 2), np.int32))
    with pytest.raises(TypeError, match="graph_components: edges must be int32"):
        call(edges=E.long())
    for bad in (F, torch.zeros(8, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"graph_components: edges must be \[E, 2\]"):
            call(edges=bad)
    for bad in (True, 5.0, "5", None, torch.tensor(5)):
        with pytest.raises(TypeError, match="graph_components: n must be an integer"):
            call(n=bad)
    for bad in (-1, 1 << 31):
        with pytest.raises(ValueError, match="graph_components: n must be an integer >= 0"):
            call(n=bad)


def test_neighbour_table():
    call = CALLS["neighbour_components"]
    with pytest.raises(TypeError, match="neighbour_components: nbr: expected a tensor"):
        call(nbr=None)
    with pytest.raises(TypeError, match="neighbour_components: nbr must be int32"):
        call(nbr=NBR.long())
    for bad in (torch.zeros(4, 8, dtype=torch.int32), torch.zeros(5, 0, dtype=torch.int32), torch.zeros(5, 65, dtype=torch.int32),
                torch.zeros(5, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"neighbour_components: nbr must be \[N"):
            call(nbr=bad)


@pytest.mark.parametrize("who, names", [("clean_mesh", ("min_faces", "min_vertices", "keep_largest")), ("clean_points", ("min_points", "keep_largest"))])
def test_counts(who, names):
    for name in names:
        for bad in (True, False, 1.0, "1", None, torch.tensor(1)):
            with pytest.raises(TypeError, match=f"{who}: {name} must be an integer"):
                CALLS[who](**{name: bad})
        for bad in (-1, -100, 1 << 31):
            with pytest.raises(ValueError, match=f"{who}: {name} must be an integer >= 0"):
                CALLS[who](**{name: bad})


@pytest.mark.parametrize("who", ["clean_mesh", "clean_points"])
def test_min_extent_and_flags(who):
    for bad in (True, "0.1", None, torch.tensor(0.1)):
        with pytest.raises(TypeError, match=f"{who}: min_extent must be a number"):
            CALLS[who](min_extent=bad)
    for bad in (float("nan"), float("inf"), -float("inf"), -0.01):
        with pytest.raises(ValueError, match=f"{who}: min_extent must be finite and >= 0"):
            CALLS[who](min_extent=bad)
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match=f"{who}: return_info must be a bool"):
            CALLS[who](return_info=bad)
    with pytest.raises(TypeError, match="unexpected keyword argument 'min_area'"):
        CALLS[who](min_area=1.0)


def test_clean_points_search_arguments():
    for bad in (0, 65, 1.5, True):
        with pytest.raises(ValueError, match=r"clean_points: k must be an integer in \[1, 64\]"):
            CALLS["clean_points"](k=bad)
    for bad in (0.0, -1.0, float("nan"), 4.5):
        with pytest.raises(ValueError, match="clean_points: radius must be a number in"):
            CALLS["clean_points"](radius=bad)


def test_ops_layer_checks():
    with pytest.raises(ValueError, match="components: source must be one of"):
        ops.components("mesh", F, 5)
    with pytest.raises(ValueError, match="components: links must be int32"):
        ops.components("edges", F, 5)
    with pytest.raises(ValueError, match="components: links must be int32"):
        ops.components("table", NBR, 4)
    with pytest.raises(ValueError, match="components: coords must be fp32"):
        ops.components("faces", F, 5, torch.zeros(4, 3))
    with pytest.raises(ValueError, match="components: min_nodes, min_links, keep_largest must be >= 0"):
        ops.components("faces", F, 5, V, min_extent=float("inf"))


@pytest.mark.parametrize("who", sorted(CALLS))
def test_cpu_tensors_are_refused(who):
    """Everything else in order: the device is what is missing."""
    with pytest.raises(RuntimeError, match=rf"{who}: \w+: expected a tensor on the HIP device, got cpu \(no CPU fallback\)"):
        CALLS[who]()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CALLS[who](return_info=True)


def test_cpu_tensors_are_refused_with_every_option():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        components.clean_mesh(torch.zeros(0, 11), torch.zeros(0, 3, dtype=torch.int32), min_faces=0, min_vertices=0, min_extent=2.5, keep_largest=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        components.clean_points(torch.zeros(0, 3), k=64, radius=4.0, min_points=7, min_extent=0, keep_largest=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.components("edges", E, 5)
