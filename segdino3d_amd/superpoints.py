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

A scan without faces (a fused point cloud, a ScanNet++ cloud, an S3DIS room) takes the segmentator's second entry,
`segment_point(vertices, normals, edges)`, here `graph_superpoints`, with the two steps in front of it when the caller has neither
edges nor normals; `point_superpoints` is the composition.  The rules are stated in include/segdino3d_hip.h, restated in
tests/point_superpoints_ref.py, and the kernels EQUAL the restatement bit for bit:

  a. `knn_graph`: row i holds the `k` smallest `(bits of d2, j)` among the valid `j != i` with `d2 = (dx dx + dy dy) + dz dz <= r2`,
     `r2 = float32(radius radius)`; a point is valid iff its coordinates are finite and below 2^14 in magnitude; missing slots are -1.
     A hashed grid of fixed-point cells chooses which pairs are evaluated; it cannot change the answer.
  b. `estimate_normals`: exact int64 moments of the row's offsets `rint((p_j - p_i) 2^20)`, the covariance in fp64, 8 sweeps of cyclic
     Jacobi in fp64, the eigenvector of the smallest eigenvalue, normalised in fp32; fewer than 3 neighbours give (0, 0, 0).  With a
     `viewpoint` the normal faces it; without, its first non-zero component is positive and the graph is segmented unoriented.
  c. `graph_superpoints`: step 3 on the given normals for every edge of the list (an edge with an end outside [0, N) is ignored and
     counted in `bad_edges`), then steps 4 to 7.  `oriented=False`: `dot = |dot|` and no convexity squaring.  `point_superpoints`
     feeds it edge `i k + s = (i, nbr[i, s])`: both copies of a mutual edge are kept and a missing slot is a bad edge.

Out of scope: reading mesh and point-cloud files, and dropping the mirrored copy of a mutual edge."""
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


# --------------------------------------------------------------------------------------------
# point clouds: k-NN graph, normals, segmentation of a general edge list
# --------------------------------------------------------------------------------------------
MAX_K = ops.KNN_MAX_K
MAX_RADIUS = ops.KNN_MAX_RADIUS


def _check_cloud(t, who, name="points"):
    if not torch.is_tensor(t):
        raise ValueError(f"{who}: {name} must be a tensor on the HIP device, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{who}: {name}: expected a tensor on the HIP device, got {t.device} (no CPU fallback)")
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{who}: {name} must be fp32 [N, 3], got {t.dtype} {list(t.shape)}")
    if t.shape[0] >= MAX_VERTICES:
        raise ValueError(f"{who}: a cloud must have fewer than 2^24 points, got {t.shape[0]}")


def _check_knn(k, radius, who):
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or k < 1 or k > MAX_K:
        raise ValueError(f"{who}: k must be an integer in [1, {MAX_K}], got {k}")
    if not isinstance(radius, (int, float, np.floating, np.integer)) or isinstance(radius, bool) or not np.isfinite(radius) \
            or radius <= 0 or radius > MAX_RADIUS:
        raise ValueError(f"{who}: radius must be a number in (0, {MAX_RADIUS}] metres, got {radius}")


def _check_nbr(nbr, n, who):
    if not torch.is_tensor(nbr):
        raise ValueError(f"{who}: nbr must be a tensor on the HIP device, got {type(nbr).__name__}")
    if not nbr.is_cuda:
        raise RuntimeError(f"{who}: nbr: expected a tensor on the HIP device, got {nbr.device} (no CPU fallback)")
    if nbr.dtype != torch.int32 or nbr.dim() != 2 or nbr.shape[0] != n or not 1 <= nbr.shape[1] <= MAX_K:
        raise ValueError(f"{who}: nbr must be int32 [N, k] with 1 <= k <= {MAX_K}, got {nbr.dtype} {list(nbr.shape)}")


def _check_viewpoint(viewpoint, n, dev, who):
    if viewpoint is None:
        return
    if not torch.is_tensor(viewpoint):
        raise ValueError(f"{who}: viewpoint must be a tensor on the HIP device, got {type(viewpoint).__name__}")
    if not viewpoint.is_cuda:
        raise RuntimeError(f"{who}: viewpoint: expected a tensor on the HIP device, got {viewpoint.device} (no CPU fallback)")
    if viewpoint.dtype != torch.float32 or tuple(viewpoint.shape) not in ((3,), (n, 3)) or viewpoint.device != dev:
        raise ValueError(f"{who}: viewpoint must be fp32 [3] or [N, 3] on the points' device, got {viewpoint.dtype} {list(viewpoint.shape)}")


def _offsets(counts, dev, scale=None):
    """Scene offsets on the host and (rows stacked, one asynchronous copy) on the device."""
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rows = [off] if scale is None else [off, off * scale]
    return off, torch.from_numpy(np.stack(rows)).to(dev, non_blocking=True)


def knn_graph(points, k: int = 16, radius: float = 0.1, return_d2: bool = False):
    """`points` fp32 [N, 3] on the device -> `nbr` int32 [N, k]: row i holds the up to `k` nearest points within `radius` of point i,
    nearest first, ties to the lower index, -1 in the missing slots (rule a); with `return_d2` also their squared distances fp32
    [N, k], +inf in the missing slots.  Exact: equal to brute force.  N == 0 and k > N - 1 are legal.  Enqueues only."""
    who = "knn_graph"
    _check_knn(k, radius, who)
    _check_cloud(points, who)
    _, off = _offsets([points.shape[0]], points.device)
    return ops.knn_graph(points.contiguous(), off[0], int(k), float(radius), return_d2=return_d2)


def estimate_normals(points, nbr, viewpoint=None):
    """`points` fp32 [N, 3], `nbr` int32 [N, k] (of `knn_graph`) -> unit normals fp32 [N, 3] (rule b); (0, 0, 0) where a row has
    fewer than 3 neighbours.  `viewpoint` fp32 [3] or [N, 3]: every normal faces it; None: the first non-zero component of every
    normal is positive (segment those with `oriented=False`).  Enqueues only."""
    who = "estimate_normals"
    _check_cloud(points, who)
    _check_nbr(nbr, points.shape[0], who)
    _check_viewpoint(viewpoint, points.shape[0], points.device, who)
    _, off = _offsets([points.shape[0]], points.device)
    view = None if viewpoint is None else (viewpoint.reshape(1, 3) if viewpoint.dim() == 1 else viewpoint).contiguous()
    return ops.point_normals(points.contiguous(), nbr.contiguous(), off[0], view)


def _edge_ends(edges):
    """[E, 2] int32 or int64 -> two contiguous int32 [E]; an index beyond int32 stays out of every scene's range."""
    if edges.dtype == torch.int64:
        edges = edges.clamp(-1, (1 << 31) - 1).to(torch.int32)
    return edges[:, 0].contiguous(), edges[:, 1].contiguous()


def _graph_infos(out, n_scenes, debug, eoff):
    host = out[1].cpu().numpy()                                                       # the one host read
    infos = [SimpleNamespace(count=int(host[i, 0]), bad_edges=int(host[i, 1])) for i in range(n_scenes)]
    if debug:
        weights = _split(out[2], eoff)
        for i, info in enumerate(infos):
            info.weights, info.settled = weights[i], out[3][i]
    return infos


def graph_superpoints(points, normals, edges, oriented: bool = True, k_thresh: float = 0.01, min_verts: int = 20,
                      return_info: bool = False, debug: bool = False):
    """The segmentator's `segment_point`: `points`, `normals` fp32 [N, 3], `edges` int32 or int64 [E, 2] on the device -> `labels`
    int64 [N] on the device (enqueues only), or `(labels, info)` with `info.count` and `info.bad_edges` (edges with an end outside
    [0, N): ignored) from one host read (rule c).  `oriented=False`: the normals carry no sign.  `debug`: info also carries `weights`
    int32 [E] (the bits of every edge weight) and `settled`.  N == 0 and E == 0 are legal."""
    who = "graph_superpoints"
    _check_rule(k_thresh, min_verts, who)
    _check_cloud(points, who)
    _check_cloud(normals, who, "normals")
    if normals.shape[0] != points.shape[0] or normals.device != points.device:
        raise ValueError(f"{who}: normals must have one row per point on the points' device, got {list(normals.shape)}")
    if not torch.is_tensor(edges):
        raise ValueError(f"{who}: edges must be a tensor on the HIP device, got {type(edges).__name__}")
    if not edges.is_cuda:
        raise RuntimeError(f"{who}: edges: expected a tensor on the HIP device, got {edges.device} (no CPU fallback)")
    if edges.dtype not in (torch.int32, torch.int64) or edges.dim() != 2 or edges.shape[1] != 2:
        raise ValueError(f"{who}: edges must be int32 or int64 [E, 2], got {edges.dtype} {list(edges.shape)}")
    if edges.shape[0] >= 1 << 31:
        raise ValueError(f"{who}: a graph must have fewer than 2^31 edges, got {edges.shape[0]}")
    if not isinstance(oriented, (bool, np.bool_)):
        raise ValueError(f"{who}: oriented must be a bool, got {oriented}")
    N, E = points.shape[0], edges.shape[0]
    off = torch.from_numpy(np.array([[0, N], [0, E]], dtype=np.int64)).to(points.device, non_blocking=True)
    ea, eb = _edge_ends(edges)
    out = ops.graph_superpoints(points.contiguous(), normals.contiguous(), ea, eb, off[0], off[1], bool(oriented), float(k_thresh),
                                int(min_verts), debug=debug)
    if not (return_info or debug):
        return out[0]
    return out[0], _graph_infos(out, 1, debug, [0, E])[0]


def _run_clouds(clouds, k, radius, normals, viewpoint, k_thresh, min_verts, debug, who):
    _check_rule(k_thresh, min_verts, who)
    _check_knn(k, radius, who)
    if len(clouds) < 1:
        raise ValueError(f"{who}: at least one cloud")
    S = len(clouds)
    for given, name in ((normals, "normals"), (viewpoint, "viewpoint")):
        if given is not None and len(given) != S:
            raise ValueError(f"{who}: {name} must be None or one entry per cloud, got {len(given)} for {S}")
    dev = clouds[0].device if torch.is_tensor(clouds[0]) else None
    for i, p in enumerate(clouds):
        _check_cloud(p, who)
        if p.device != dev:
            raise ValueError(f"{who}: the clouds of a batch must share one device")
        if normals is not None:
            _check_cloud(normals[i], who, "normals")
            if normals[i].shape[0] != p.shape[0] or normals[i].device != dev:
                raise ValueError(f"{who}: normals must have one row per point on the points' device, got {list(normals[i].shape)}")
        if viewpoint is not None:
            if viewpoint[i] is None:
                raise ValueError(f"{who}: a viewpoint for every cloud of the batch, or for none")
            _check_viewpoint(viewpoint[i], p.shape[0], dev, who)
    counts = [p.shape[0] for p in clouds]
    voff, off = _offsets(counts, dev, scale=int(k))
    N = int(voff[-1])
    points = clouds[0].contiguous() if S == 1 else torch.cat(list(clouds))
    nbr = ops.knn_graph(points, off[0], int(k), float(radius))
    if normals is not None:
        nrm = normals[0].contiguous() if S == 1 else torch.cat(list(normals))
    else:
        view = None
        if viewpoint is not None:
            if all(v.dim() == 1 for v in viewpoint):
                view = torch.stack(list(viewpoint))
            else:
                view = torch.cat([v.reshape(1, 3).expand(n, 3) if v.dim() == 1 else v for v, n in zip(viewpoint, counts)]).contiguous()
        nrm = ops.point_normals(points, nbr, off[0], view)
    index = torch.arange(N, dtype=torch.int64, device=dev)
    if S > 1:                                                                         # the index inside its scene
        index = index - torch.repeat_interleave(off[0, :-1], off[0, 1:] - off[0, :-1], output_size=N)
    ea = index.to(torch.int32).repeat_interleave(int(k))                              # edge i k + s = (i, nbr[i, s])
    oriented = normals is not None or viewpoint is not None
    out = ops.graph_superpoints(points, nrm, ea, nbr.reshape(-1), off[0], off[1], oriented, float(k_thresh), int(min_verts), debug=debug)
    return out, voff, nbr, nrm


def point_superpoints_batch(clouds, k: int = 16, radius: float = 0.1, normals=None, viewpoint=None, k_thresh: float = 0.01,
                            min_verts: int = 20, return_info: bool = False, debug: bool = False):
    """Superpoints of a list of point clouds (fp32 [N_i, 3] each) in one launch chain, one sweep workgroup per scene -> a list of
    int64 label tensors, each with the bits of its single run wherever it stands in the list; no neighbour crosses a scene.
    `normals` / `viewpoint`: None, or a list with one entry per cloud.  `return_info`: also a list of `info` (one host read for the
    whole batch).  `debug`: each info also carries `nbr`, `normals`, `weights` and `settled`."""
    who = "point_superpoints_batch"
    clouds = list(clouds)
    normals = None if normals is None else list(normals)
    viewpoint = None if viewpoint is None else list(viewpoint)
    out, voff, nbr, nrm = _run_clouds(clouds, k, radius, normals, viewpoint, k_thresh, min_verts, debug, who)
    labels = _split(out[0], voff)
    if not (return_info or debug):
        return labels
    infos = _graph_infos(out, len(clouds), debug, voff * int(k))
    if debug:
        for i, info in enumerate(infos):
            info.nbr, info.normals = _split(nbr, voff)[i], _split(nrm, voff)[i]
    return labels, infos


def point_superpoints(points, k: int = 16, radius: float = 0.1, normals=None, viewpoint=None, k_thresh: float = 0.01,
                      min_verts: int = 20, return_info: bool = False, debug: bool = False):
    """`points` fp32 [N, 3] on the device -> `labels` int64 [N] on the device (enqueues only), or `(labels, info)` with `info.count`
    and `info.bad_edges` (= the missing slots of the k-NN graph) from one host read: `knn_graph`, then `estimate_normals` unless
    `normals` fp32 [N, 3] are given, then `graph_superpoints` over the edges `(i, nbr[i, s])`, oriented iff `normals` or a
    `viewpoint` (fp32 [3] or [N, 3]) is given."""
    who = "point_superpoints"
    out, voff, nbr, nrm = _run_clouds([points], k, radius, None if normals is None else [normals],
                                      None if viewpoint is None else [viewpoint], k_thresh, min_verts, debug, who)
    if not (return_info or debug):
        return out[0]
    info = _graph_infos(out, 1, debug, voff * int(k))[0]
    if debug:
        info.nbr, info.normals = nbr, nrm
    return out[0], info
