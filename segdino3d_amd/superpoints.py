"""Superpoints from a triangle mesh on the device (csrc/superpoints.hip): the producer of the model's `super_points` input, the graph
segmentation ScanNet's segmentator applies to a scan.  The reference takes it from an external package
(`data/scannet/batch_load_scannet_data.py:84-87`) and ships no code that makes it, so there is no reference implementation to pin
against: the rule below is restated in float32 numpy and integers in tests/superpoints_ref.py, and the kernels EQUAL that restatement
label for label.  A segmentation is discontinuous in its weights, so every arithmetic step is one correctly rounded float32 operation
(no fused multiply-add) or an exact integer one.

Inputs: `vertices` fp32 [N, 3], `faces` int32 or int64 [F, 3], `k_thresh` (0.01), `min_verts` (20); N < 2^24 and 3 F < 2^31.  A face
with an index outside [0, N) is ignored and counted in `bad_faces`; a face with a repeated index is kept: its self-edges join
nothing and its normal is zero.

  1. Face normal.  `a = p1 - p0`, `b = p2 - p0`, `n = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x)`, every product and
     difference rounded on its own; `l = sqrt((n.x n.x + n.y n.y) + n.z n.z)`; valid iff `l` is finite and > 0, then `n /= l`.
  2. Vertex normal.  Each valid face adds `rint(n 2^24)` to its three vertices, int64 sums (order-free, so integer atomics);
     `m = float32(float64(sum))`, normalised as above; a zero or invalid `m` is (0, 0, 0).  Area-free: every face counts alike.
  3. Edges.  Face `f = (i, j, k)` gives edges `3 f = (i, j)`, `3 f + 1 = (i, k)`, `3 f + 2 = (k, j)`; shared sides appear once per
     face.  For edge `(a, b)`: `dot = (m_a.x m_b.x + m_a.y m_b.y) + m_a.z m_b.z`, `w = max(1 - dot, 0)`,
     `s = (m_b.x (p_b.x - p_a.x) + m_b.y (p_b.y - p_a.y)) + m_b.z (p_b.z - p_a.z)`; if `s > 0` (convex; a NaN is not) `w = w w`.
  4. Order.  Ascending `(bits of w as uint32, edge index)`.
  5. Pass 1 (Felzenszwalb-Huttenlocher).  Every vertex is a component with `size = 1`, `thr = k_thresh`.  In order: the components
     `A != B` of an edge's ends join iff `w <= thr[A]` and `w <= thr[B]`; then `size = size_A + size_B` and
     `thr = w + k_thresh / float32(size)`.  A refused edge is not looked at again in this pass.
  6. Pass 2.  In the same order: `A != B` join iff `size[A] < min_verts` or `size[B] < min_verts`.
  7. Output.  `labels` int64 [N] on the device, dense `0 .. S - 1`, components numbered by their smallest vertex; `count = S` and
     `bad_faces` come in one host read.  A vertex in no face is a component of its own.

The labels are what `io_scene.pack_scene(scene["super_points"])` and the architecture's `extra_features["super_point_masks"]` take,
unchanged; the point features of `lift2d` are pooled over them like every other point feature.

Out of scope: reading mesh files, and the segmentator's other front ends (point clouds with k-nearest-neighbour graphs)."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from . import ops

MAX_VERTICES = ops.SUPERPOINTS_MAX_VERTICES


def _check_mesh(vertices, faces, who):
    for t, name in ((vertices, "vertices"), (faces, "faces")):
        if not torch.is_tensor(t):
            raise ValueError(f"{who}: {name} must be a tensor on the HIP device, got {type(t).__name__}")
        if not t.is_cuda:
            raise RuntimeError(f"{who}: {name}: expected a tensor on the HIP device, got {t.device} (no CPU fallback)")
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"{who}: vertices must be fp32 [N, 3], got {vertices.dtype} {list(vertices.shape)}")
    if faces.dtype not in (torch.int32, torch.int64) or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{who}: faces must be int32 or int64 [F, 3], got {faces.dtype} {list(faces.shape)}")
    if vertices.shape[0] >= MAX_VERTICES:
        raise ValueError(f"{who}: a mesh must have fewer than 2^24 vertices, got {vertices.shape[0]}")
    if 3 * faces.shape[0] >= 1 << 31:
        raise ValueError(f"{who}: a mesh must have fewer than 2^31 / 3 faces, got {faces.shape[0]}")


def _check_rule(k_thresh, min_verts, who):
    if not isinstance(k_thresh, (int, float, np.floating, np.integer)) or not np.isfinite(k_thresh) or k_thresh < 0 \
            or k_thresh > float(np.finfo(np.float32).max):
        raise ValueError(f"{who}: k_thresh must be a finite number >= 0, got {k_thresh}")
    if not isinstance(min_verts, (int, np.integer)) or isinstance(min_verts, bool) or min_verts < 1 or min_verts >= 1 << 31:
        raise ValueError(f"{who}: min_verts must be an integer >= 1, got {min_verts}")


def _run(meshes, k_thresh, min_verts, debug, who):
    _check_rule(k_thresh, min_verts, who)
    if len(meshes) < 1:
        raise ValueError(f"{who}: at least one mesh")
    for v, f in meshes:
        _check_mesh(v, f, who)
    dev = meshes[0][0].device
    dtypes = {f.dtype for _, f in meshes}
    if len(dtypes) > 1 or any(v.device != dev or f.device != dev for v, f in meshes):
        raise ValueError(f"{who}: the meshes of a batch must share one device and one face dtype")
    voff = np.concatenate([[0], np.cumsum([v.shape[0] for v, _ in meshes])]).astype(np.int64)
    foff = np.concatenate([[0], np.cumsum([f.shape[0] for _, f in meshes])]).astype(np.int64)
    if len(meshes) == 1:
        vertices, faces = meshes[0][0].contiguous(), meshes[0][1].contiguous()
    else:
        vertices, faces = torch.cat([v for v, _ in meshes]), torch.cat([f for _, f in meshes])
    off = torch.from_numpy(np.stack([voff, foff])).to(dev, non_blocking=True)
    out = ops.mesh_superpoints(vertices, faces, off[0], off[1], float(k_thresh), int(min_verts), debug=debug)
    return out, voff, foff


def _split(t, off, scale=1):
    return [t[int(off[i]) * scale:int(off[i + 1]) * scale] for i in range(len(off) - 1)]


def mesh_superpoints_batch(meshes, k_thresh: float = 0.01, min_verts: int = 20, return_info: bool = False, debug: bool = False):
    """Superpoints of a list of `(vertices, faces)` in one launch chain, one sweep workgroup per scene -> a list of int64 label
    tensors, each with the same bits as when its mesh runs alone, wherever it stands in the list.  `return_info`: also a list of
    `info` (one host read for the whole batch).  `debug`: each info also carries `normals` fp32 [N, 3], `weights` int32 [3 F] (the
    bits of every edge weight) and `settled` = the edges of pass 1 / pass 2 the sweep settled in LDS."""
    who = "mesh_superpoints_batch"
    meshes = list(meshes)
    out, voff, foff = _run(meshes, k_thresh, min_verts, debug, who)
    labels = _split(out[0], voff)
    if not (return_info or debug):
        return labels
    host = out[1].cpu().numpy()                                                       # the one host read
    infos = [SimpleNamespace(count=int(host[i, 0]), bad_faces=int(host[i, 1])) for i in range(len(meshes))]
    if debug:
        normals, weights = _split(out[2], voff), _split(out[3], foff, 3)
        for i, info in enumerate(infos):
            info.normals, info.weights, info.settled = normals[i], weights[i], out[4][i]
    return labels, infos


def mesh_superpoints(vertices, faces, k_thresh: float = 0.01, min_verts: int = 20, return_info: bool = False, debug: bool = False):
    """`vertices` fp32 [N, 3], `faces` int32 or int64 [F, 3] on the device -> `labels` int64 [N] on the device (enqueues only), or
    `(labels, info)` with `info.count` (the number of superpoints) and `info.bad_faces` from one host read.  N == 0 and F == 0 are
    legal: zero faces give every vertex its own label."""
    who = "mesh_superpoints"
    out, voff, foff = _run([(vertices, faces)], k_thresh, min_verts, debug, who)
    if not (return_info or debug):
        return out[0]
    host = out[1].cpu().numpy()                                                       # the one host read
    info = SimpleNamespace(count=int(host[0, 0]), bad_faces=int(host[0, 1]))
    if debug:
        info.normals, info.weights, info.settled = out[2], out[3], out[4][0]
    return out[0], info
