"""Decimate a triangle mesh on the device by vertex clustering (csrc/simplify.hip): the stage between `TsdfVolume.mesh()` and
`superpoints.mesh_superpoints`.  `tsdf.py` at 2 cm makes a mesh about three times denser than the decimated ScanNet scans the model was
trained on, and every stage after the mesher - the superpoint sweep, `raster.py`, voxelisation, pooling and the 2D lift - scales with
that density, while `min_verts` and `k_thresh` of the superpoint rule mean something else at it.  `simplify_mesh` brings the mesh down
to one vertex per grid cell, and its `vertex_map` carries the forward's per-vertex results back onto the full-resolution mesh:
`Views -> TsdfVolume.mesh() -> simplify_mesh -> mesh_superpoints -> lift -> forward -> carry_back`.  The reference has no counterpart
(it loads meshes that MeshLab decimated offline), so there is nothing to pin against: the rule below is restated in numpy in
tests/simplify_ref.py, and the kernels are tested to EQUAL that, bit for bit.

Inputs: `vertices` fp32 `[V, C]` on the device with `3 <= C <= 11` - x, y, z and up to 8 attribute channels; the `[V, 6]` of `points`
and of `TsdfVolume.mesh()` goes in unchanged and the output has the same `C` - and `faces` int32 `[F, 3]` on the device.  `cell`
(default 0.04) must be finite and `>= 2^-6`, so that cell indices fit 21 bits, as `tsdf.MIN_VOXEL` does.  Host constant:
`inv_cell = float32(1 / cell)`, made in float64 and rounded once.  Every fp32 operation is rounded on its own, no fused multiply-add.

  1. Valid vertex.  All `C` channels must satisfy `|c| < 2^14`, compared as floats: a NaN or an infinity fails.  Otherwise the vertex
     is bad: `bad_vertices += 1`, `vertex_map = -1`.
  2. Cell.  `k_i = floorf(x_i * inv_cell)` per axis; key `((k_x + 2^20) << 42) | ((k_y + 2^20) << 21) | (k_z + 2^20)`, the key layout
     of `fuse_views` and `tsdf`.
  3. Per cell, integers only.  `n` = the number of members; per channel `S_j = sum of (int64) rintf(c_j * 65536.0f)` (the product is
     exact and `|.| < 2^30`).  Integer sums make the cell a function of the SET of its vertices.
  4. Output vertices, one per occupied cell, in ascending key.  `placement="mean"`: channel `j` is
     `float32((double) S_j / ((double) n * 65536.0))`.  `placement="nearest"`: the whole row of one member, copied bit for bit - the
     member with the smallest `(bits of d2, vertex index)`, `d2 = (dx dx + dy dy) + dz dz` against the fp32 mean of the xyz channels,
     `dx = x - mean_x`, one rounding per operation: the distance form of `transfer`.  The vertex stays on the surface and colours stay
     crisp.
  5. Faces.  A face with an index outside `[0, V)` or a bad corner is bad and counted.  Otherwise its corners go through `vertex_map`.
     If two mapped corners are equal the face is collapsed and counted.  Otherwise it is rotated so that its smallest index comes
     first; rotation keeps the winding, so the oriented triple is the face's identity.  Among faces with the same oriented triple the
     lowest original face index survives, the others count as `duplicates`.  Opposite windings of the same three vertices are
     different faces and both stay: the two sides of a thin sheet are like that.  Survivors come out in ascending original face index,
     written as the rotated triple.
  6. `keep_unreferenced=False`.  Output vertices that no surviving face references are dropped; they count as `unreferenced` and their
     members' `vertex_map` becomes -1.  The rest are renumbered in the same key order and faces are written with the new numbers.
     With `True` the counter is still filled and nothing is dropped.
  7. Limits.  More than `2^21` occupied cells raise (the oriented triple packs into one 63-bit sort key), and so do sizes the workspace
     cannot hold.  `V = 0` and `F = 0` are ordinary inputs and return empty tensors on the device.

Outputs: `SimplifiedMesh(vertices [Vn, C], faces [Fn, 3], vertex_map int32 [V], face_source int32 [Fn])`.  `vertex_map` is old vertex ->
new vertex or -1: `pred_small[vertex_map]` (`carry_back`) carries per-vertex results of a forward on the small mesh back to the scan.
`face_source` is the original face of each kept face: `face_labels[face_source]` carries face labels forward.  `SimplifyInfo` holds
the seven counters of `ops.SIMPLIFY_INFO`; `F = bad_faces + collapsed + duplicates + faces`.

The call enqueues, then makes ONE host read, of the counters, to trim the outputs; the trimmed outputs are clones, not views of the
capacity buffers, as in `TsdfVolume.mesh()`.  Nothing else synchronises.  The result is a pure function of mesh and rule: every sum is
an integer and every choice a minimum over a set, so the bits do not depend on the schedule or the stream.

Not built: quadric-error placement and edge-collapse decimation (clustering moves vertices by up to a cell and does not weigh
curvature), a `target_vertices` search over `cell`, batches of meshes in one launch, welding without a grid (two vertices closer than
`cell` on either side of a cell border stay apart), reading or writing mesh files, a `simplify=` argument on `TsdfVolume.mesh()`."""
from __future__ import annotations

import math
import numbers
from collections import namedtuple

import torch

from . import ops
from .raster import _faces, _on_device

MIN_CELL = 2.0 ** -6                # |x| < 2^14 then keeps every cell index inside [-2^20, 2^20)
PLACEMENTS = ("mean", "nearest")

SimplifiedMesh = namedtuple("SimplifiedMesh", ("vertices", "faces", "vertex_map", "face_source"))
SimplifyInfo = namedtuple("SimplifyInfo", ops.SIMPLIFY_INFO)
SimplifyInfo.__doc__ = """Host integers read by `simplify_mesh`: vertices and faces written, bad_vertices (step 1), bad_faces, collapsed and
duplicates (step 5; with `faces` they sum to F), unreferenced (output vertices no surviving face uses, dropped or not)."""


def _vertices(vertices, who):
    if not isinstance(vertices, torch.Tensor):
        raise TypeError(f"{who}: vertices: expected a tensor, got {type(vertices).__name__}")
    if vertices.dtype != torch.float32:
        raise TypeError(f"{who}: vertices must be fp32, got {vertices.dtype}")
    if vertices.dim() != 2 or not 3 <= vertices.shape[1] <= ops.SIMPLIFY_MAX_CHANNELS:
        raise ValueError(f"{who}: vertices must be [V, C] with 3 <= C <= {ops.SIMPLIFY_MAX_CHANNELS} (x, y, z first), got {list(vertices.shape)}")
    return vertices


def _cell(cell, who) -> float:
    if isinstance(cell, bool) or not isinstance(cell, numbers.Real):
        raise TypeError(f"{who}: cell must be a number, got {type(cell).__name__}")
    if not (math.isfinite(cell) and float(cell) >= MIN_CELL):
        raise ValueError(f"{who}: cell must be finite and >= 2^-6 m (cell indices must fit 21 bits), got {cell}")
    return float(cell)


def simplify_mesh(vertices, faces, cell: float = 0.04, placement: str = "mean", keep_unreferenced: bool = True, return_info: bool = False):
    """The mesh clustered on a grid of `cell` metres by the rule of this module -> `SimplifiedMesh(vertices, faces, vertex_map,
    face_source)`, then a `SimplifyInfo` with `return_info`.  Enqueues, then reads the seven counters once to trim the outputs."""
    who = "simplify_mesh"
    _vertices(vertices, who)
    _faces(faces, who)
    cell = _cell(cell, who)
    if placement not in PLACEMENTS:
        raise ValueError(f"{who}: placement must be one of {PLACEMENTS}, got {placement!r}")
    if not isinstance(keep_unreferenced, bool):
        raise TypeError(f"{who}: keep_unreferenced must be a bool, got {type(keep_unreferenced).__name__}")
    _on_device(vertices, "vertices", who)
    _on_device(faces, "faces", who)
    vout, fout, vmap, fsrc, info = ops.simplify_mesh(vertices.contiguous(), faces.contiguous(), 1.0 / cell, nearest=placement == "nearest",
                                                     keep_unreferenced=keep_unreferenced)
    info = SimplifyInfo(*(int(x) for x in info.tolist()))                              # the one host read
    if info.vertices + (0 if keep_unreferenced else info.unreferenced) > ops.SIMPLIFY_MAX_CELLS:
        raise RuntimeError(f"{who}: {info.vertices + (0 if keep_unreferenced else info.unreferenced)} occupied cells, more than 2^21: the "
                           f"oriented triple of a face must pack into one 63-bit sort key; use a larger cell than {cell} or cut the mesh")
    # a view of a far larger buffer would pin it: copy
    mesh = SimplifiedMesh(vout[:info.vertices].clone(), fout[:info.faces].clone(), vmap, fsrc[:info.faces].clone())
    return (mesh, info) if return_info else mesh


def carry_back(values_small, vertex_map, fill):
    """Per-vertex results of the small mesh on the vertices of the full one: `values_small` [Vn, ...] and `vertex_map` [V] ->
    [V, ...], `fill` where the map is -1.  Plain torch indexing, no kernel."""
    if not isinstance(values_small, torch.Tensor) or not isinstance(vertex_map, torch.Tensor):
        raise TypeError("carry_back: values_small and vertex_map must be tensors")
    if vertex_map.dim() != 1 or vertex_map.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"carry_back: vertex_map must be int32 or int64 [V], got {vertex_map.dtype} {list(vertex_map.shape)}")
    idx = vertex_map.long()
    shape = (idx.shape[0],) + tuple(values_small.shape[1:])
    if values_small.shape[0] == 0:
        return values_small.new_full(shape, fill)
    live = (idx >= 0).reshape((-1,) + (1,) * (values_small.dim() - 1))
    return torch.where(live, values_small[idx.clamp_min(0)], values_small.new_full((), fill))           # no mask indexing: nothing synchronises
