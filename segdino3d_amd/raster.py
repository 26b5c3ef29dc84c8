"""Rasterise a triangle mesh into posed views on the device (csrc/raster.hip, csrc/raster_rule.h): depth, face and vertex maps and
label images for frames that have NO depth of their own - DSLR frames registered against a scan, a phone walk-through against a lidar
mesh, any SfM camera - and the model's depth of a fused `TsdfVolume` at a pose nobody recorded.  Every stage between a sensor and a
forward takes a `lift2d.Views`, and a `Views` needs a depth image: the depth rendered here is exactly what `Views` takes as fp32
metres, so `lift_point_features`, `lift_queries`, `PointCloudFuser`, `PointIndex.nearest_pixels` and `render_prediction` work
unchanged on RGB-only frames, and the face and vertex maps carry a forward's per-vertex result onto such frames.  The reference has
no counterpart, so there is no reference implementation to pin against: the rule below is a pure function of its inputs, it is
restated in numpy in tests/raster_ref.py, and the kernels are tested to EQUAL that, bit for bit.

Inputs: `vertices` fp32 `[Nv, >= 3]` on the device (x, y, z are read), `faces` int32 `[F, 3]` on the device; per view `intrinsics`
fp32 `[V, 4] = (fx, fy, cx, cy)` on the device or the host and `cam_to_world` `[V, 4, 4]` on the host; one image size `(H, W)`,
`1 <= H, W <= 16384`; `near > 0` (default 0.1), `far >= near` (default 6.0).  Views with a non-finite pose are dropped by
`lift2d.world_to_cam`, which also supplies the fp32 `world_to_cam [K, 3, 4]` (inverted in float64, each entry rounded once); `kept`
tells which views stayed.  Pixel centres lie at integer coordinates, as in `lift2d` and `backproject.h`.

Per (kept view, face), every fp32 operation rounded on its own, no fused multiply-add:

  1. Bad face.  An index outside `[0, Nv)`, or a corner with a coordinate that fails `|c| < 2^14` compared as floats (NaN and infinity
     fail): the face is ignored and counted under `bad`.
  2. Camera space.  `x_c = ((r00 x + r01 y) + r02 z) + t0`, `y_c` and `z_c` alike.  If any corner has `z_c < near` the face is dropped
     and counted under `near`.  There is NO near-plane clipping: a triangle that crosses the near plane is lost whole.  That is the
     limit of this rule; with scan-sized triangles the lost strip lies at depths the depth rule of every consumer rejects anyway.
  3. Projection and snap.  `u = (fx * x_c) / z_c + cx`, `v` alike.  If any corner fails `|u| < 2^14 && |v| < 2^14` (floats, before
     anything becomes an integer) the face is dropped and counted under `guard`.  Otherwise `X = (int) rint(u * 256)`, `Y` alike:
     eight sub-pixel bits.
  4. Edge functions in int64.  For pixel `(vi, ui)`, `P = (256 ui, 256 vi)`; `E(a, b, P) = (bx - ax)(Py - ay) - (by - ay)(Px - ax)`;
     `A = E(v0, v1, v2)`.  If `A == 0`, or the bounding box clamped to the image holds no pixel centre, the face is dropped and counted
     under `empty`.  With `s = sign(A)`: `w0 = s E(v1, v2, P)`, `w1 = s E(v2, v0, P)`, `w2 = s E(v0, v1, P)`.  The pixel is covered iff
     all three are `>= 0`: edges are inclusive, both windings draw, nothing is culled.  `w0 + w1 + w2 == |A|` exactly.
  5. Depth in float64, one rounding per operation.  `q_i = 1.0 / (double) z_c,i`, `num = (w0 q0 + w1 q1) + w2 q2`,
     `d = (float) ((double) |A| / num)`: perspective-correct z-depth (`1 / z` is linear on the screen).  The sample is kept iff
     `near <= d <= far`.
  6. Key.  `(bits of d << 32) | face index`; the pixel keeps the minimum over all samples: the nearest face, ties to the lower face
     index.  A minimum over a set: the images are a pure function of mesh, cameras and rule, and do not depend on the order of the
     faces in flight, on the cut of the views into calls or passes, or on the stream.
  7. Outputs per pixel.  `depth` fp32, `0` where nothing was hit (the "invalid" of `Views`); `face` int32, `-1` where nothing was hit;
     `vertex` int32: `faces[face][i]` for the `i` with the largest `w_i`, ties to the lowest `i` (the weights recomputed for the
     winning face by the same device function).  Up to 8 label channels by the same resolve kernel: `face_labels` int32 `[L, F]` read
     at `face`, `vertex_labels` int32 `[L, Nv]` read at `vertex`, `fill` (default `-1`) where nothing was hit.
  8. Counters.  `info` int64 on the device, `ops.RASTER_INFO = ("drawn", "near", "guard", "empty", "bad", "pixels")`: the first five
     classify every (kept view, face) pair exactly once (precedence `bad`, `near`, `guard`, `empty`, `drawn`) and sum to `K * F`;
     `pixels` is the number of pixels hit.  Reading it (`read_info()`) is the one optional host read.

The views are drawn in passes of at most `views_per_pass` (default 32) that share one key buffer `uint64 [views, H, W]`: 79 MB at
480 x 640 against 629 MB for 256 views at once.  Nothing in this module reads the device.

Not built: near-plane clipping, back-face culling, a top-left fill rule (a pixel centre exactly on a shared edge is drawn by both
faces and goes to the nearer, then the lower index), anti-aliasing and interpolated attributes (colour, normals, features), a tiled
on-chip z-buffer (bins per screen tile and LDS atomics in place of the global key buffer), reading mesh or image files, batches of
meshes in one launch."""
from __future__ import annotations

import numbers

import numpy as np
import torch

from . import ops
from .lift2d import Views, world_to_cam
from .transfer import PREDICTION_IMAGES, _fill, _xyz, prediction_channels

RULE_DEFAULTS = dict(near=0.1, far=6.0, views_per_pass=None)
DEFAULT_VIEWS_PER_PASS = 32


def _rule(rule: dict, who: str) -> dict:
    bad = set(rule) - set(RULE_DEFAULTS)
    if bad:
        raise TypeError(f"{who}: unknown rule parameter(s) {sorted(bad)}; known: {sorted(RULE_DEFAULTS)}")
    return {**RULE_DEFAULTS, **rule}


def _range(near, far, who):
    for x, name in ((near, "near"), (far, "far")):
        if isinstance(x, bool) or not isinstance(x, numbers.Real):
            raise TypeError(f"{who}: {name} must be a number, got {type(x).__name__}")
    if not (float(near) > 0.0 and float(far) >= float(near)):
        raise ValueError(f"{who}: need 0 < near <= far, got near = {near}, far = {far}")
    return float(near), float(far)


def _size(height, width, who):
    for x, name in ((height, "height"), (width, "width")):
        if isinstance(x, bool) or not isinstance(x, numbers.Integral):
            raise TypeError(f"{who}: {name} must be an integer, got {type(x).__name__}")
        if not 1 <= x <= ops.RASTER_MAX_DIM:
            raise ValueError(f"{who}: {name} must lie in 1 .. {ops.RASTER_MAX_DIM}, got {x}")
    return int(height), int(width)


def _faces(faces, who):
    if not isinstance(faces, torch.Tensor):
        raise TypeError(f"{who}: faces: expected a tensor, got {type(faces).__name__}")
    if faces.dtype != torch.int32:
        raise TypeError(f"{who}: faces must be int32, got {faces.dtype}")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{who}: faces must be [F, 3], got {list(faces.shape)}")
    return faces


def _labels(labels, n, name, rows, who):
    """None, [n] or [L, n] of int32 / int64 / uint8 / bool -> (the labels as [L, n] or None, whether a row was given alone)."""
    if labels is None:
        return None, False
    if not isinstance(labels, torch.Tensor):
        raise TypeError(f"{who}: {name}: expected a tensor, got {type(labels).__name__}")
    if labels.dtype not in (torch.int32, torch.int64, torch.uint8, torch.bool):
        raise TypeError(f"{who}: {name} must be int32, int64, uint8 or bool, got {labels.dtype}")
    single = labels.dim() == 1
    if single:
        labels = labels[None]
    if labels.dim() != 2 or labels.shape[1] != n:
        raise ValueError(f"{who}: {name} must be [{rows} = {n}] or [L, {rows}], got {list(labels.shape)}")
    if not 1 <= labels.shape[0] <= ops.RASTER_MAX_LABELS:
        raise ValueError(f"{who}: 1 <= L <= {ops.RASTER_MAX_LABELS} channels of {name} in one call, got L = {labels.shape[0]}")
    return labels, single


def _on_device(t, name, who):
    if not t.is_cuda:
        raise RuntimeError(f"{who}: {name}: expected a tensor on the HIP device, got {t.device} (no CPU fallback)")
    return t


def _intrinsics(intrinsics, V, who):
    if not isinstance(intrinsics, torch.Tensor):
        intrinsics = torch.from_numpy(np.array(intrinsics, dtype=np.float32))       # a copy: the caller's array may be read-only
    if intrinsics.dtype != torch.float32 or tuple(intrinsics.shape) != (V, 4):
        raise ValueError(f"{who}: intrinsics must be fp32 [V = {V}, 4] = (fx, fy, cx, cy), got {intrinsics.dtype} {list(intrinsics.shape)}")
    return intrinsics


class RenderResult:
    """What `render_mesh` returns, one image per KEPT view: `depth` fp32 [K, H, W] (0 = nothing hit), `face` and `vertex` int32
    [K, H, W] (-1), `face_label_images` / `vertex_label_images` int32 [L, K, H, W] ([K, H, W] for labels given as one row); each is
    None when it was not asked for.  `kept` (host int64 [K]) holds the indices of the views that stayed, `n_given` the number handed
    in, `info` the counters int64 [6] on the device."""

    __slots__ = ("depth", "face", "vertex", "face_label_images", "vertex_label_images", "kept", "n_given", "info")

    def __init__(self, depth, face, vertex, face_label_images, vertex_label_images, kept, n_given, info):
        self.depth, self.face, self.vertex = depth, face, vertex
        self.face_label_images, self.vertex_label_images = face_label_images, vertex_label_images
        self.kept, self.n_given, self.info = kept, n_given, info

    def read_info(self) -> dict:
        """The counters as a dict of ints keyed by `ops.RASTER_INFO`: the one host read (it waits for the stream)."""
        return dict(zip(ops.RASTER_INFO, (int(x) for x in self.info.cpu().tolist())))


def render_mesh(vertices, faces, intrinsics, cam_to_world, height, width, *, face_labels=None, vertex_labels=None, fill=-1,
                return_depth=True, return_face=True, return_vertex=False, views_per_pass=None, near=0.1, far=6.0) -> RenderResult:
    """The mesh drawn into the kept views by the rule of this module -> `RenderResult`.  `face_labels` ([F] or [L, F]) are read at the
    pixel's face and `vertex_labels` ([Nv] or [L, Nv]) at its vertex, int32 / int64 / uint8 / bool, at most 8 channels together.
    `K == 0`, `F == 0` or `Nv == 0` launch nothing and return the fills.  Enqueues only."""
    who = "render_mesh"
    _xyz(vertices, "vertices", who, on_device=False)
    _faces(faces, who)
    H, W = _size(height, width, who)
    near, far = _range(near, far, who)
    fill = _fill(fill, who)
    if views_per_pass is not None and (isinstance(views_per_pass, bool) or not isinstance(views_per_pass, numbers.Integral) or views_per_pass < 1):
        raise ValueError(f"{who}: views_per_pass must be an integer >= 1 (None = the default, {DEFAULT_VIEWS_PER_PASS}), got {views_per_pass}")
    Nv, F = vertices.shape[0], faces.shape[0]
    flab, fsingle = _labels(face_labels, F, "face_labels", "F", who)
    vlab, vsingle = _labels(vertex_labels, Nv, "vertex_labels", "Nv", who)
    n_channels = (0 if flab is None else flab.shape[0]) + (0 if vlab is None else vlab.shape[0])
    if n_channels > ops.RASTER_MAX_LABELS:
        raise ValueError(f"{who}: at most {ops.RASTER_MAX_LABELS} label channels in one call, got {n_channels} (face and vertex labels together)")
    if not (return_depth or return_face or return_vertex or n_channels):
        raise ValueError(f"{who}: nothing to return: give labels, or ask for the depth, the face or the vertex")
    w2c, kept = world_to_cam(cam_to_world)
    V = int(np.shape(cam_to_world)[0])
    intrinsics = _intrinsics(intrinsics, V, who)
    # everything above needs no device
    xyz = _xyz(vertices, "vertices", who)
    faces = _on_device(faces, "faces", who).contiguous()
    flab = None if flab is None else _on_device(flab, "face_labels", who).to(torch.int32).contiguous()
    vlab = None if vlab is None else _on_device(vlab, "vertex_labels", who).to(torch.int32).contiguous()
    dev, K = xyz.device, len(kept)
    if K == 0 or F == 0 or Nv == 0:                     # no launch: the fills, and every pair a bad face when there is no vertex
        shape = (K, H, W)
        full = lambda value, lead=(): torch.full(tuple(lead) + shape, value, dtype=torch.int32, device=dev)  # noqa: E731
        depth = torch.zeros(shape, dtype=torch.float32, device=dev) if return_depth else None
        face = full(-1) if return_face else None
        vertex = full(-1) if return_vertex else None
        fout = None if flab is None else full(fill, (flab.shape[0],))
        vout = None if vlab is None else full(fill, (vlab.shape[0],))
        info = torch.tensor([0, 0, 0, 0, K * F, 0], dtype=torch.int64).to(dev)
    else:
        intr = intrinsics.to(dev)
        if K != V:
            intr = intr.index_select(0, torch.from_numpy(kept).to(dev))
        depth, face, vertex, fout, vout, info = ops.raster_views(
            xyz, faces, torch.from_numpy(w2c).to(dev), intr.contiguous(), H, W, near=near, far=far,
            views_per_pass=views_per_pass or DEFAULT_VIEWS_PER_PASS, face_labels=flab, vertex_labels=vlab, fill=fill,
            return_depth=return_depth, return_face=return_face, return_vertex=return_vertex)
    if fout is not None and fsingle:
        fout = fout[0]
    if vout is not None and vsingle:
        vout = vout[0]
    return RenderResult(depth, face, vertex, fout, vout, kept, V, info)


def rendered_views(vertices, faces, intrinsics, cam_to_world, height, width, **rule) -> Views:
    """The kept views as a `lift2d.Views` that holds the rendered fp32 depth (metres, 0 = nothing hit): ready for
    `lift_point_features`, `lift_queries`, `PointCloudFuser`, `PointIndex.nearest_pixels` and `render_prediction`.  `kept` and
    `n_given` are those of the poses handed in, so per-view maps and colours may be given per given or per kept view."""
    who = "rendered_views"
    r = _rule(rule, who)
    res = render_mesh(vertices, faces, intrinsics, cam_to_world, height, width, return_face=False, **r)
    V, kept = res.n_given, res.kept
    pose = np.asarray(cam_to_world.detach().numpy() if isinstance(cam_to_world, torch.Tensor) else cam_to_world, dtype=np.float64)
    intrinsics = _intrinsics(intrinsics, V, who)
    if len(kept) != V:
        intrinsics = intrinsics.index_select(0, torch.from_numpy(kept).to(intrinsics.device))
    views = Views(res.depth, intrinsics, pose[kept])
    if len(kept) != V:                                  # the views dropped here, not by `Views`
        views.n_given, views.kept = V, kept
        views._kept_dev = torch.from_numpy(kept).to(res.depth.device)
    return views


def render_prediction_mesh(vertices, faces, intrinsics, cam_to_world, height, width, pred, score_thr: float = 0.0, fill: int = -1, **rule):
    """A forward's result painted onto frames WITHOUT depth, for a forward that ran on the mesh vertices: the five images of
    `transfer.PREDICTION_IMAGES` as a dict of int32 [K, H, W], each pixel reading the channels `transfer.render_prediction` builds at
    the vertex of rule 7; `fill` where nothing was hit.  One render call with the five channels as vertex labels."""
    who = "render_prediction_mesh"
    r = _rule(rule, who)
    fill = _fill(fill, who)
    _xyz(vertices, "vertices", who, on_device=False)
    chans = prediction_channels(pred, score_thr, fill, who)
    if chans.shape[1] != vertices.shape[0]:
        raise ValueError(f"{who}: the prediction covers {chans.shape[1]} points but the mesh has {vertices.shape[0]} vertices")
    res = render_mesh(vertices, faces, intrinsics, cam_to_world, height, width, vertex_labels=chans, fill=fill, return_depth=False,
                      return_face=False, **r)
    return {name: res.vertex_label_images[i] for i, name in enumerate(PREDICTION_IMAGES)}
