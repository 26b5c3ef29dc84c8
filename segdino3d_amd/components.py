"""Connected components of a mesh, an edge list or a neighbour table on the device, and the clean that throws away what is not the
scene (csrc/components.hip).  A TSDF fused from real depth leaves floating shells and specks - flying pixels the edge test let through,
noise seen in a handful of frames, the far side of a window - and a voxel-grid cloud has the same; `tsdf.py` carves no free space, so
nothing removes them later.  Every floating piece of `min_verts` or more vertices becomes a superpoint of its own, and with
`query_num = -1` a decoder query.  ScanNet's meshes had their isolated pieces removed offline; `clean_mesh` and `clean_points` do it
here: `Views -> TsdfVolume.mesh() -> clean_mesh -> simplify_mesh -> mesh_superpoints -> lift -> forward -> carry_back -> carry_back`,
and `fuse_views -> clean_points -> estimate_normals / graph_superpoints`.  The reference has no counterpart, so there is nothing to pin
against: the rule below is restated in numpy in tests/components_ref.py, and the kernels are tested to EQUAL that, bit for bit.

`n` nodes and a list of links.  A link source is one of three forms: `faces` int32 `[F, 3]` (a link joins its three corners), `edges`
int32 `[E, 2]`, or a neighbour table int32 `[N, k]`, what `knn_graph` returns: entry `j` of row `i` joins `i` and `j`, and an entry of
`-1` is an empty slot, skipped and not counted.

  1. Good node.  With coordinates (fp32 `[n, C]`, `3 <= C <= 11`, x y z first) a node is good iff all `C` channels satisfy
     `|c| < 2^14`, compared as floats: a NaN fails.  This is step 1 of `simplify.py`, so a cleaned mesh has no bad vertex left for it.
     Without coordinates (the pure graph form) every node is good.  A bad node has label `-1`, is never written out and counts in
     `bad_nodes`.
  2. Good link.  Every index lies inside `[0, n)` and every end is good; otherwise the link counts in `bad_links` and joins nothing.  A
     link with repeated ends (a degenerate face, a self-loop) is good: it joins its distinct ends and is kept or dropped with its
     component.  Removing it is `simplify_mesh`'s job.
  3. Components.  The classes of the good nodes under "joined by a good link", closed transitively.  A good node that is in no good link
     is a component of one node and counts in `isolated`.  Components are numbered densely, `0 .. K-1`, in ascending order of their
     smallest node index: the numbering of `mesh_superpoints`.  `labels[i]` is that number, or `-1` for a bad node.
  4. Per component, as functions of the member set only: `n_nodes` (int32); `n_links` (int32): good links, table entries counted one
     each; `box` fp32 `[K, 6]` = x lo, x hi, y lo, y hi, z lo, z hi: per axis the member coordinate that is smallest, then largest,
     under the order of the integer key of its bits (`b ^ 0x80000000` for `b >= 0`, `~b` otherwise), so `-0` sorts below `+0` and the
     emitted float is a member's coordinate bit for bit; `extent = max over axes of (hi - lo)`, one fp32 subtraction per axis, rounded
     on its own.  In the graph form the box and the extent are 0.
  5. Keep.  A component passes iff `n_nodes >= min_nodes`, `n_links >= min_links` and `extent >= float32(min_extent)`: equality passes.
     If `keep_largest = m > 0`, only the first `m` of the passing components stay, in the order `(n_links descending, label ascending)`;
     `m >= K` keeps all passing components.
  6. Output of a clean.  Kept nodes come out in ascending original index, each row copied bit for bit.  `node_map` int32 `[n]` maps old
     to new, or `-1`.  Kept links come out in ascending original index with their ends renumbered, corner order untouched;
     `link_source` int32 gives their original rows.  `labels` of the output is the component of each output node, renumbered densely
     over the kept components in the same order.  The table form writes the cleaned table of the same `k`: entries that were no good
     link (their target was dropped as a bad point, or out of range) become `-1`, in place, with no compaction inside a row.
  7. Counters, `ops.COMPONENTS_INFO`: `components`, `kept`, `nodes` and `links` written, `bad_nodes`, `bad_links`, `isolated`,
     `unsettled`.  Over the faces form `F = bad_links + links + the links of dropped components`.  Sizes up to `2^31 - 1`; a table has
     fewer than `2^31` entries.  `n = 0` and `F = 0` are ordinary inputs and return empty tensors on the device.

`unsettled` counts good links whose two ends ended in different components.  The union runs lock-free across the chip's eight L2s on
relaxed atomics, and this one pass over the links turns a coherence mistake into a `RuntimeError` instead of a wrong mesh; it is 0.

Each call enqueues, then makes ONE host read, of the counters, to trim the outputs; the trimmed outputs are clones, not views of the
capacity buffers, as in `simplify_mesh`.  Nothing else synchronises.  The result is a pure function of nodes, links and rule: the
components are a function of the SET of links, every count is an integer and every choice a minimum over a set, so the bits do not
depend on the schedule or the stream.

Not built: free-space carving in the TSDF (this removes what carving would have prevented, after the fact); surface area per component
(it needs a square root the restatement cannot pin without care); welding of coincident vertices before the components (two shells
that touch without sharing a vertex stay two); DBSCAN-style core / border rules for clouds (the k-NN table's links are taken as they
are); batches of meshes in one launch; a `clean=` argument on `TsdfVolume.mesh()`; reading or writing mesh files."""
from __future__ import annotations

import math
import numbers
from collections import namedtuple

import torch

from . import ops
from .raster import _faces, _on_device

Components = namedtuple("Components", ("labels", "n_nodes", "n_links", "box"))
CleanedMesh = namedtuple("CleanedMesh", ("vertices", "faces", "vertex_map", "face_source", "labels"))
CleanedPoints = namedtuple("CleanedPoints", ("points", "point_map", "labels", "neighbours"))
ComponentsInfo = namedtuple("ComponentsInfo", ops.COMPONENTS_INFO)
ComponentsInfo.__doc__ = """Host integers read by every call of this module: components found and kept, nodes and links written, bad_nodes
(step 1), bad_links (step 2), isolated (good nodes in no good link), unsettled (always 0: see the module)."""


def _count(x, name, who) -> int:
    if isinstance(x, bool) or not isinstance(x, numbers.Integral):
        raise TypeError(f"{who}: {name} must be an integer, got {type(x).__name__}")
    if not 0 <= int(x) < 1 << 31:
        raise ValueError(f"{who}: {name} must be an integer >= 0 (and below 2^31), got {x}")
    return int(x)


def _extent(x, who) -> float:
    if isinstance(x, bool) or not isinstance(x, numbers.Real):
        raise TypeError(f"{who}: min_extent must be a number, got {type(x).__name__}")
    if not (math.isfinite(x) and float(x) >= 0.0):
        raise ValueError(f"{who}: min_extent must be finite and >= 0, got {x}")
    return float(x)


def _flag(x, name, who) -> bool:
    if not isinstance(x, bool):
        raise TypeError(f"{who}: {name} must be a bool, got {type(x).__name__}")
    return x


def _nodes(t, name, who):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name}: expected a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: {name} must be fp32, got {t.dtype}")
    if t.dim() != 2 or not 3 <= t.shape[1] <= ops.COMPONENTS_MAX_CHANNELS:
        raise ValueError(f"{who}: {name} must be [N, C] with 3 <= C <= {ops.COMPONENTS_MAX_CHANNELS} (x, y, z first), got {list(t.shape)}")
    return t


def _links(t, name, width, who):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name}: expected a tensor, got {type(t).__name__}")
    if t.dtype != torch.int32:
        raise TypeError(f"{who}: {name} must be int32, got {t.dtype}")
    if width is not None and (t.dim() != 2 or t.shape[1] != width):
        raise ValueError(f"{who}: {name} must be [E, {width}], got {list(t.shape)}")
    return t


def _table(nbr, n, who):
    _links(nbr, "nbr", None, who)
    if nbr.dim() != 2 or nbr.shape[0] != n or not 1 <= nbr.shape[1] <= ops.KNN_MAX_K:
        raise ValueError(f"{who}: nbr must be [N = {n}, k] with 1 <= k <= {ops.KNN_MAX_K}, got {list(nbr.shape)}")
    if n * nbr.shape[1] >= 1 << 31:
        raise ValueError(f"{who}: nbr must have fewer than 2^31 entries, got {n} x {nbr.shape[1]}")
    return nbr


def _read(out, who) -> ComponentsInfo:
    info = ComponentsInfo(*(int(x) for x in out["info"].tolist()))                      # the one host read
    if info.unsettled:
        raise RuntimeError(f"{who}: {info.unsettled} good links ended with their ends in different components: the union did not settle "
                           f"(a memory-coherence fault in csrc/components.hip); the result is refused")
    return info


def _components(out, return_info, who):
    info = _read(out, who)
    K = info.components
    # a view of a far larger buffer would pin it: copy
    res = Components(out["labels"], out["n_nodes"][:K].clone(), out["n_links"][:K].clone(), out["box"][:K].clone())
    return (res, info) if return_info else res


def mesh_components(vertices, faces, return_info: bool = False):
    """The components of a mesh by the rule of this module: `vertices` fp32 [V, C], `faces` int32 [F, 3] -> `Components(labels int32
    [V], n_nodes int32 [K], n_links int32 [K], box fp32 [K, 6])`, then a `ComponentsInfo` with `return_info`.  One host read."""
    who = "mesh_components"
    _nodes(vertices, "vertices", who)
    _faces(faces, who)
    _flag(return_info, "return_info", who)
    _on_device(vertices, "vertices", who)
    _on_device(faces, "faces", who)
    return _components(ops.components("faces", faces.contiguous(), vertices.shape[0], vertices.contiguous()), return_info, who)


def graph_components(n, edges, return_info: bool = False):
    """The components of `n` nodes under `edges` int32 [E, 2], the pure graph form: every node is good, box and extent are 0."""
    who = "graph_components"
    n = _count(n, "n", who)
    _links(edges, "edges", 2, who)
    _flag(return_info, "return_info", who)
    _on_device(edges, "edges", who)
    return _components(ops.components("edges", edges.contiguous(), n), return_info, who)


def neighbour_components(points, nbr, return_info: bool = False):
    """The components of a cloud under a neighbour table: `points` fp32 [N, C], `nbr` int32 [N, k] as `knn_graph` returns it."""
    who = "neighbour_components"
    _nodes(points, "points", who)
    _table(nbr, points.shape[0], who)
    _flag(return_info, "return_info", who)
    _on_device(points, "points", who)
    _on_device(nbr, "nbr", who)
    return _components(ops.components("table", nbr.contiguous(), points.shape[0], points.contiguous()), return_info, who)


def clean_mesh(vertices, faces, min_faces: int = 1, min_vertices: int = 1, min_extent: float = 0.0, keep_largest: int = 0,
               return_info: bool = False):
    """The mesh without the components that fail step 5 (`min_faces` is `min_links`, `min_vertices` is `min_nodes`) ->
    `CleanedMesh(vertices [Vn, C], faces [Fn, 3], vertex_map int32 [V], face_source int32 [Fn], labels int32 [Vn])`, then a
    `ComponentsInfo` with `return_info`.  `simplify.carry_back(pred, vertex_map, fill)` carries per-vertex results of the cleaned mesh
    back.  Enqueues, then reads the eight counters once to trim the outputs."""
    who = "clean_mesh"
    _nodes(vertices, "vertices", who)
    _faces(faces, who)
    min_faces, min_vertices = _count(min_faces, "min_faces", who), _count(min_vertices, "min_vertices", who)
    min_extent, keep_largest = _extent(min_extent, who), _count(keep_largest, "keep_largest", who)
    _flag(return_info, "return_info", who)
    _on_device(vertices, "vertices", who)
    _on_device(faces, "faces", who)
    out = ops.components("faces", faces.contiguous(), vertices.shape[0], vertices.contiguous(), min_nodes=min_vertices, min_links=min_faces,
                         min_extent=min_extent, keep_largest=keep_largest, clean=True)
    info = _read(out, who)
    mesh = CleanedMesh(out["nodes"][:info.nodes].clone(), out["links"][:info.links].clone(), out["node_map"],
                       out["link_source"][:info.links].clone(), out["labels_out"][:info.nodes].clone())
    return (mesh, info) if return_info else mesh


def clean_points(points, k: int = 16, radius: float = 0.1, min_points: int = 1, min_extent: float = 0.0, keep_largest: int = 0,
                 return_info: bool = False):
    """The cloud without the components of its k-NN graph (`superpoints.knn_graph(points[:, :3], k, radius)`) that fail step 5 ->
    `CleanedPoints(points [Nn, C], point_map int32 [N], labels int32 [Nn], neighbours int32 [Nn, k])`.  `neighbours` is the table of
    the cleaned cloud in its new numbering: it feeds `estimate_normals` / `graph_superpoints` without a second search."""
    from . import superpoints
    who = "clean_points"
    _nodes(points, "points", who)
    superpoints._check_knn(k, radius, who)
    min_points = _count(min_points, "min_points", who)
    min_extent, keep_largest = _extent(min_extent, who), _count(keep_largest, "keep_largest", who)
    _flag(return_info, "return_info", who)
    _on_device(points, "points", who)
    points = points.contiguous()
    nbr = superpoints.knn_graph(points[:, :3].contiguous(), k, radius)
    out = ops.components("table", nbr, points.shape[0], points, min_nodes=min_points, min_extent=min_extent, keep_largest=keep_largest, clean=True)
    info = _read(out, who)
    cloud = CleanedPoints(out["nodes"][:info.nodes].clone(), out["node_map"], out["labels_out"][:info.nodes].clone(),
                          out["links"][:info.nodes].clone())
    return (cloud, info) if return_info else cloud
