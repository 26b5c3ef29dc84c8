"""Carry what a forward computed per point onto the frames and onto other clouds (csrc/transfer.hip): the output-side counterpart of
`fuse_views.py`.  `pts_semantic_mask`, `pts_instance_mask`, `instance_labels` and `instance_scores` are indexed by the points the
forward ran on; a labelling tool, a robot or an overlay needs them on the pixels of the frames, `submission.py` and `eval_ap` /
`eval_seg` need them on a scan's mesh vertices or on ground-truth points.  The reference has no code for this (it evaluates on the
points it loaded), so there is no reference implementation to pin against: the rule below is restated in numpy in
tests/transfer_ref.py, and the kernels are tested to EQUAL that, bit for bit.

A depth pixel back-projected through its own pose IS the visible surface, so painting a frame needs no z-buffer and no splat radius:
it is a nearest-point query per pixel, and one kernel family serves both uses.

Source cloud `P` fp32 `[N, >= 3]`, radius `0 < r <= 4` (`ops.KNN_MAX_RADIUS`), `r2 = fl32(r * r)`.

  1. Valid points.  A source point or a query is valid iff all three coordinates satisfy `|c| < 2^14`, compared as floats; a NaN or an
     infinity fails.  An invalid query gets `-1`; an invalid source point is never a candidate.
  2. Distance.  For query `q` and valid source `j`: `dx = P[j].x - q.x` (`dy`, `dz` alike), `d2 = (dx * dx + dy * dy) + dz * dz`, every
     operation rounded on its own in fp32, no fused multiply-add; `j` is a candidate iff `d2 <= r2`.  This is `knn_graph`'s distance
     without the self-exclusion.
  3. Answer.  The candidate with the smallest key `(bits of d2 << 32) | j`: the nearest, ties to the lower index.  `idx` int32 (`-1`
     when there is no candidate) and, on request, `d2` fp32 (`+inf` when there is none).
  4. Pixel queries.  Pixel `(vi, ui)` of kept view `v` of a `lift2d.Views`: `d` by step 2 of `fuse_views` (`(float) raw * depth_scale`,
     valid iff `d > 0`, `d >= near`, `d <= far`; defaults `near=0.1`, `far=6.0`; no edge test, no stride); `w` = step 4 of
     `fuse_views`, the same device function, every operation rounded on its own; `w` is then a query as in steps 1 to 3.  A pixel
     whose depth is invalid gets `-1`.
  5. Labels.  `labels` int32 `[L, N]`, `1 <= L <= 8`: `out[l, query] = labels[l, idx]`, or `fill` (default `-1`) where `idx < 0`,
     written by the kernel that found `idx`: a frame's label image costs no second pass over an index image.
  6. Instance map.  The instance result is overlapping masks `[I, N]` with scores, not a map: `map[n]` is the `i` with `masks[i, n]`
     set and `scores[i] >= score_thr` that has the largest score, compared in fp32; ties go to the lower `i`; a NaN score never wins;
     `-1` if there is none.

The answer is a minimum over a set, so it is a pure function of the source cloud and the set of queries: the same bits however the
views are cut into calls and on whatever stream.  The grid behind the search (the one `knn_graph` builds) only chooses which pairs are
evaluated and cannot change the answer.  Nothing in this module reads the device.

Frames without depth are served by `raster.py`: it z-buffers a mesh into posed views, and `raster.render_prediction_mesh` paints the
same five images onto them.

Out of scope: `k > 1` and interpolated (soft) transfer, batches of scenes in one launch, writing image files, the edge test of
`fuse_views` step 3."""
from __future__ import annotations

import numbers

import torch

from . import ops
from .lift2d import Views, check_depth_range

RULE_DEFAULTS = dict(near=0.1, far=6.0)


def _rule(rule: dict) -> dict:
    bad = set(rule) - set(RULE_DEFAULTS)
    if bad:
        raise TypeError(f"unknown pixel-query parameter(s) {sorted(bad)}; known: {sorted(RULE_DEFAULTS)}")
    r = {**RULE_DEFAULTS, **rule}
    check_depth_range(r)
    return r


def _xyz(t, name, who, on_device=True):
    """fp32 [n, >= 3] on the device -> contiguous fp32 [n, 3]; `on_device=False`: the type, dtype and shape checks alone."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name}: expected a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: {name} must be fp32, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] < 3:
        raise ValueError(f"{who}: {name} must be [n, >= 3] (x, y, z first), got {list(t.shape)}")
    if not on_device:
        return t
    if not t.is_cuda:
        raise RuntimeError(f"{who}: {name}: expected a tensor on the HIP device, got {t.device} (no CPU fallback)")
    return t[:, :3].contiguous()


def _labels(labels, N, who):
    """None, [N] or [L, N] of int32 / int64 / uint8 / bool -> (the labels as [L, N] or None, whether a row was given alone)."""
    if labels is None:
        return None, False
    if not isinstance(labels, torch.Tensor):
        raise TypeError(f"{who}: labels: expected a tensor, got {type(labels).__name__}")
    if labels.dtype not in (torch.int32, torch.int64, torch.uint8, torch.bool):
        raise TypeError(f"{who}: labels must be int32, int64, uint8 or bool, got {labels.dtype}")
    single = labels.dim() == 1
    if single:
        labels = labels[None]
    if labels.dim() != 2 or labels.shape[1] != N:
        raise ValueError(f"{who}: labels must be [N = {N}] or [L, N], got {list(labels.shape)}")
    if not 1 <= labels.shape[0] <= ops.NEAREST_MAX_LABELS:
        raise ValueError(f"{who}: 1 <= L <= {ops.NEAREST_MAX_LABELS} label channels in one call, got L = {labels.shape[0]}")
    return labels, single


def _labels_i32(labels, who):
    """The checked labels as contiguous int32 on the device (the conversion is a device copy)."""
    if labels is None:
        return None
    if not labels.is_cuda:
        raise RuntimeError(f"{who}: labels: expected a tensor on the HIP device, got {labels.device} (no CPU fallback)")
    return labels.to(torch.int32).contiguous()


def _fill(fill, who):
    if isinstance(fill, bool) or int(fill) != fill or not -(1 << 31) <= fill < 1 << 31:
        raise ValueError(f"{who}: fill must be an integer that fits int32, got {fill}")
    return int(fill)


def _pack(idx, d2, out, single):
    if out is not None and single:
        out = out[0]
    res = tuple(x for x in (idx, d2, out) if x is not None)
    return res[0] if len(res) == 1 else res


class PointIndex:
    """The search index of one source cloud at one radius: built once (three kernels and a sort, enqueued by the constructor), kept in
    a workspace this object owns, and queried any number of times.  `points` fp32 [N, >= 3] on the device; only x, y, z are read, and
    the index holds its own copy: the cloud may be freed.  Queries must be enqueued on a stream that is ordered after the build."""

    def __init__(self, points, radius: float):
        who = "PointIndex"
        if isinstance(radius, bool) or not isinstance(radius, numbers.Real) or not (0.0 < float(radius) <= ops.KNN_MAX_RADIUS):
            raise ValueError(f"{who}: radius must lie in (0, {ops.KNN_MAX_RADIUS}], got {radius}")
        xyz = _xyz(points, "points", who)
        self.radius, self.n_points, self.device = float(radius), int(xyz.shape[0]), xyz.device
        self._ws = ops.point_index_build(xyz, self.radius)

    def nearest(self, queries, labels=None, fill: int = -1, return_d2: bool = False):
        """queries fp32 [M, >= 3] -> idx int32 [M], then d2 fp32 [M] with `return_d2`, then out int32 [L, M] ([M] for labels [N]) with
        `labels`.  Enqueues only."""
        who = "PointIndex.nearest"
        _xyz(queries, "queries", who, on_device=False)
        lab, single = _labels(labels, self.n_points, who)
        fill = _fill(fill, who)
        idx, d2, out = ops.nearest_points(_xyz(queries, "queries", who), self._ws, self.n_points, self.radius, labels=_labels_i32(lab, who),
                                          fill=fill, return_d2=return_d2)
        return _pack(idx, d2, out, single)

    def nearest_pixels(self, views: Views, labels=None, fill: int = -1, return_index: bool = True, return_d2: bool = False, near=0.1,
                       far=6.0):
        """-> idx int32 [K, Hd, Wd] with `return_index`, then d2 fp32 [K, Hd, Wd] with `return_d2`, then out int32 [L, K, Hd, Wd]
        ([K, Hd, Wd] for labels [N]) with `labels`, over the K kept views (`views.kept` tells which).  One launch; enqueues only."""
        who = "PointIndex.nearest_pixels"
        if not isinstance(views, Views):
            raise TypeError(f"{who}: views must be a lift2d.Views, got {type(views).__name__}")
        r = _rule(dict(near=near, far=far))
        lab, single = _labels(labels, self.n_points, who)
        fill = _fill(fill, who)
        if not (return_index or return_d2 or lab is not None):
            raise ValueError(f"{who}: nothing to return: give labels, or ask for the index or d2")
        K, shape = len(views), (len(views), views.height, views.width)
        if K == 0:                                      # no launch
            dev = views.depth.device
            idx = torch.empty(shape, dtype=torch.int32, device=dev) if return_index else None
            d2 = torch.empty(shape, dtype=torch.float32, device=dev) if return_d2 else None
            out = torch.empty((lab.shape[0],) + shape, dtype=torch.int32, device=dev) if lab is not None else None
        else:
            idx, d2, out = ops.nearest_pixels(views.depth, views.depth_scale, views.intrinsics, views.cam_to_world, self._ws, self.n_points,
                                              self.radius, labels=_labels_i32(lab, who), fill=fill, return_index=return_index,
                                              return_d2=return_d2, **r)
        return _pack(idx, d2, out, single)


def instance_map(masks, scores, score_thr: float = 0.0):
    """Rule 6: masks bool / uint8 [I, N], scores fp32 [I] on the device -> int32 [N].  Enqueues only."""
    who = "instance_map"
    for t, name in ((masks, "masks"), (scores, "scores")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: {name}: expected a tensor, got {type(t).__name__}")
    if masks.dtype not in (torch.bool, torch.uint8) or scores.dtype != torch.float32:
        raise TypeError(f"{who}: masks must be bool or uint8 and scores fp32, got {masks.dtype} and {scores.dtype}")
    if masks.dim() != 2 or tuple(scores.shape) != (masks.shape[0],):
        raise ValueError(f"{who}: masks must be [I, N] and scores [I], got {list(masks.shape)} and {list(scores.shape)}")
    if score_thr != score_thr:
        raise ValueError(f"{who}: score_thr must not be a NaN")
    for t, name in ((masks, "masks"), (scores, "scores")):
        if not t.is_cuda:
            raise RuntimeError(f"{who}: {name}: expected a tensor on the HIP device, got {t.device} (no CPU fallback)")
    return ops.instance_map(masks.contiguous(), scores.contiguous(), score_thr)


def transfer_labels(src_points, labels, dst_points, radius: float, fill: int = -1):
    """The one-shot point form: the labels ([N] or [L, N]) of `src_points` at the nearest source point of every row of `dst_points`
    -> int32 [M] or [L, M]; `fill` where no source point lies within `radius`."""
    if labels is None:
        raise TypeError("transfer_labels: labels are required")
    res = PointIndex(src_points, radius).nearest(dst_points, labels=labels, fill=fill)
    return res[-1]


def render_labels(views: Views, src_points, labels, radius: float, fill: int = -1, **rule):
    """The one-shot pixel form: label images int32 [K, Hd, Wd] or [L, K, Hd, Wd] of the kept views."""
    if labels is None:
        raise TypeError("render_labels: labels are required")
    rule = _rule(rule)
    return PointIndex(src_points, radius).nearest_pixels(views, labels=labels, fill=fill, return_index=False, **rule)


def _field(pred, key):
    return pred[key] if isinstance(pred, dict) else getattr(pred, key)


def _device_field(pred, key, who="render_prediction"):
    t = _field(pred, key)
    if isinstance(t, (list, tuple)):
        return [_device_tensor(x, key, who) for x in t]
    return _device_tensor(t, key, who)


def _device_tensor(t, key, who="render_prediction"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who}: {key}: expected tensors on the HIP device (run the model with `model.to_host = False`; "
                           "no CPU fallback)")
    return t


PREDICTION_IMAGES = ("semantic", "panoptic_semantic", "panoptic_instance", "instance", "instance_label")


def prediction_channels(pred, score_thr, fill, who):
    """The five per-point channels of `PREDICTION_IMAGES`, int32 [5, N] on the device, of a model output or its `pred_pts_seg`: what
    `render_prediction` paints through the nearest point and `raster.render_prediction_mesh` through the nearest vertex of a face."""
    pred = getattr(pred, "pred_pts_seg", pred)
    sem, inst = _device_field(pred, "pts_semantic_mask", who), _device_field(pred, "pts_instance_mask", who)
    labels, scores = _device_field(pred, "instance_labels", who), _device_field(pred, "instance_scores", who)
    if len(sem) < 2 or len(inst) < 2:
        raise ValueError(f"{who}: pts_semantic_mask and pts_instance_mask must hold the plain and the panoptic result")
    imap = instance_map(inst[0], scores.to(torch.float32), score_thr)
    ilab = labels.reshape(-1).to(torch.int32)
    ilabel = torch.cat([ilab, ilab.new_full((1,), fill)])[imap.long()]                # -1 reads the appended `fill`
    return torch.stack([sem[0].to(torch.int32), sem[1].to(torch.int32), inst[1].to(torch.int32), imap, ilabel])


def render_prediction(views: Views, points, pred, radius: float, score_thr: float = 0.0, fill: int = -1, **rule):
    """A forward's result painted onto the kept views: `pred` is a model output or its `pred_pts_seg` (`PointData` / dict) with device
    tensors (`model.to_host = False`), `points` the cloud the forward ran on.  -> dict of int32 images [K, Hd, Wd]:

        semantic            pts_semantic_mask[0]
        panoptic_semantic   pts_semantic_mask[1]
        panoptic_instance   pts_instance_mask[1]
        instance            instance_map(pts_instance_mask[0], instance_scores, score_thr)
        instance_label      instance_labels gathered through `instance` (`fill` where it is -1)

    `fill` where a pixel has no depth or no point within `radius`.  One index build, one pixel launch with the five channels."""
    rule, fill = _rule(rule), _fill(fill, "render_prediction")
    chans = prediction_channels(pred, score_thr, fill, "render_prediction")
    out = PointIndex(points, radius).nearest_pixels(views, labels=chans, fill=fill, return_index=False, **rule)
    return {name: out[i] for i, name in enumerate(PREDICTION_IMAGES)}
