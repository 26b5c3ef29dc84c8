"""Lift posed 2D feature maps onto scene points on the device (csrc/lift2d.hip): the producer of `points_2dfeats`, the [N, C]
per-point 2D features the backbone's early fusion concatenates to rgb.  The reference only loads them from a per-scene dump and ships
no code that makes them, so there is no reference implementation to pin against: the rule below is restated in float64 numpy in
tests/lift2d_ref.py, and the kernels are tested against that.

The rule is the standard multi-view lifting.  For point `n` and view `v`, with `world_to_cam = inverse(cam_to_world)` (inverted on
the host in float64, rounded to fp32):

  1. `p_c = R p + t`, `z = p_c.z`; require `z > near`;
  2. `u = fx x / z + cx`, `v = fy y / z + cy` in pixels of the depth image (pixel centres at integer coordinates);
     `ui = floor(u + 0.5)`, `vi` likewise; require `border <= ui < Wd - border` and the same for `vi`;
  3. `d = depth[v, vi, ui] * depth_scale`; require `d > 0` and `|d - z| <= tol_abs + tol_rel * d`.

Every comparison is made on floats before anything becomes an index, so NaN, infinite and huge coordinates are simply not visible.
A visible pair is sampled at `xf = (u + 0.5) * Wf / Wd - 0.5`, `yf` likewise (`align_corners=False`), bilinearly with the tap indices
clamped to the map (`grid_sample(padding_mode="border")`).  Per scale, `sum[n]` adds the samples of the visible views in ascending view
order in fp32, `mean = sum / count` (zero where `count == 0`), and the output is `(mean_0 + mean_1 + ...) / n_scales` in list order.
Visibility is computed once per view and shared by the scales.  The result is a pure function of the inputs: it does not depend on
`views_per_pass`, on how the views are split over `add` calls (as long as they arrive in the same order), or on the stream.

Out of scope: the 2D network that makes the maps and reading image files.  The DINO-X query side (`query2d_feats` / `query2d_pos`)
is made by `lift_queries.py` from the same `Views`."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops

RULE_DEFAULTS = dict(near=0.05, border=0, tol_abs=0.05, tol_rel=0.0)


def _host_f64(x, name):
    if isinstance(x, torch.Tensor):
        if x.is_cuda:
            raise TypeError(f"Views: {name} are host data (numpy or a CPU tensor): they are inverted on the host in float64")
        x = x.detach().numpy()
    return np.asarray(x, dtype=np.float64)


def world_to_cam(cam_to_world):
    """cam_to_world [V, 4, 4] (host) -> (world_to_cam fp32 [K, 3, 4], kept int64 [K]): the views whose pose has a non-finite entry
    are dropped (ScanNet has such poses), the rest are inverted in float64 and rounded to fp32."""
    pose = _host_f64(cam_to_world, "poses")
    if pose.ndim != 3 or pose.shape[1:] != (4, 4):
        raise ValueError(f"Views: cam_to_world must be [V, 4, 4], got {list(pose.shape)}")
    kept = np.flatnonzero(np.isfinite(pose).all(axis=(1, 2)))
    inv = np.linalg.inv(pose[kept]) if len(kept) else np.zeros((0, 4, 4))
    return np.ascontiguousarray(inv[:, :3, :].astype(np.float32)), kept


class Views:
    """A batch of posed depth frames: `depth` [V, Hd, Wd] on the device, uint16 with `depth_scale` (ScanNet: 0.001) or fp32 metres
    (0 = invalid); `intrinsics` [V, 4] = (fx, fy, cx, cy) in pixels of the depth image, on the device or the host; `cam_to_world`
    [V, 4, 4] on the host.  Views with a non-finite pose are dropped here, before anything is launched: `kept` holds the indices of
    the others (host int64), `n_given` the number handed in, and `depth` / `intrinsics` / `world_to_cam` / `cam_to_world` (both fp32
    [K, 3, 4] on the device) have one row per kept view."""

    def __init__(self, depth, intrinsics, cam_to_world, depth_scale: Optional[float] = None):
        if not isinstance(depth, torch.Tensor) or depth.dim() != 3:
            raise ValueError("Views: depth must be a tensor [V, Hd, Wd]")
        if depth.dtype == torch.uint16:
            if depth_scale is None or not float(depth_scale) > 0.0:
                raise ValueError("Views: uint16 depth needs a depth_scale > 0 (ScanNet: 0.001)")
            depth_scale = float(depth_scale)
        elif depth.dtype == torch.float32:
            if depth_scale is not None:
                raise ValueError("Views: fp32 depth is in metres and takes no depth_scale")
        else:
            raise TypeError(f"Views: depth must be uint16 or fp32, got {depth.dtype}")
        V = depth.shape[0]
        w2c, kept = world_to_cam(cam_to_world)
        if _host_f64(cam_to_world, "poses").shape[0] != V:
            raise ValueError(f"Views: {V} depth images but {np.shape(cam_to_world)[0]} poses")
        if not isinstance(intrinsics, torch.Tensor):
            intrinsics = torch.from_numpy(np.ascontiguousarray(intrinsics, dtype=np.float32))
        if intrinsics.dtype != torch.float32 or tuple(intrinsics.shape) != (V, 4):
            raise ValueError(f"Views: intrinsics must be fp32 [V = {V}, 4] = (fx, fy, cx, cy), got {intrinsics.dtype} {list(intrinsics.shape)}")
        if not depth.is_cuda:
            raise RuntimeError(f"Views: depth: expected a tensor on the HIP device, got {depth.device} (no CPU fallback)")
        dev = depth.device
        self.n_given, self.kept, self.depth_scale = V, kept, depth_scale
        self.height, self.width = depth.shape[1], depth.shape[2]
        intrinsics = intrinsics.to(dev)
        if len(kept) != V:
            self._kept_dev = torch.from_numpy(kept).to(dev)
            intrinsics = intrinsics.index_select(0, self._kept_dev)
            # uint16 has no index kernels: select through the int16 view of the same bytes
            depth = depth.view(torch.int16).index_select(0, self._kept_dev).view(torch.uint16) if depth.dtype == torch.uint16 \
                else depth.index_select(0, self._kept_dev)
        else:
            self._kept_dev = None
        self.depth, self.intrinsics = depth.contiguous(), intrinsics.contiguous()
        self.world_to_cam = torch.from_numpy(w2c).to(dev)
        # the poses themselves, rounded to fp32 [K, 3, 4]: what lift_queries back-projects with
        c2w = _host_f64(cam_to_world, "poses")[kept][:, :3, :]
        self.cam_to_world = torch.from_numpy(np.ascontiguousarray(c2w.astype(np.float32))).to(dev)

    def __len__(self) -> int:
        return len(self.kept)

    def select_maps(self, maps: torch.Tensor) -> torch.Tensor:
        """One map per GIVEN view -> one per kept view (a copy only when views were dropped); maps that already have one row per
        kept view pass through."""
        if self._kept_dev is not None and maps.shape[0] == self.n_given:
            return maps.index_select(0, self._kept_dev)
        if maps.shape[0] != len(self.kept):
            raise ValueError(f"feature maps: expected one per view ({self.n_given} given, {len(self.kept)} kept), got {maps.shape[0]}")
        return maps

    def check_colors(self, colors, who) -> None:
        """`colors` as the fusion stages take them: uint8 [V, Hc, Wc, 3] on the device, one per given or per kept view."""
        check_colors(colors, who)
        if colors.shape[0] not in (self.n_given, len(self)):
            raise ValueError(f"{who}: expected one colour image per view ({self.n_given} given, {len(self)} kept), got {list(colors.shape)}")


def check_colors(colors, who, V=None) -> None:
    """Colour images uint8 [V, Hc, Wc, 3] on the device; with `V` their number is checked too."""
    if not isinstance(colors, torch.Tensor):
        raise TypeError(f"{who}: colors: expected a tensor, got {type(colors).__name__}")
    if not colors.is_cuda:
        raise RuntimeError(f"{who}: colors: expected a tensor on the HIP device, got {colors.device} (no CPU fallback)")
    if colors.dtype != torch.uint8:
        raise TypeError(f"{who}: colors must be uint8, got {colors.dtype}")
    if colors.dim() != 4 or (V is not None and colors.shape[0] != V) or colors.shape[3] != 3 or colors.shape[1] < 1 or colors.shape[2] < 1:
        raise ValueError(f"{who}: colors must be [{'V' if V is None else f'V = {V}'}, Hc, Wc, 3], got {list(colors.shape)}")


def check_depth_range(r: dict) -> None:
    """The depth-pixel parameters of a stage's rule (csrc/depth_pixel.h): `near`, `far` and, where the stage has the edge test,
    `edge_abs`, `edge_rel` (`None` turns it off)."""
    if not (float(r["near"]) >= 0.0 and float(r["far"]) >= float(r["near"])):
        raise ValueError(f"need 0 <= near <= far, got near = {r['near']}, far = {r['far']}")
    if r.get("edge_rel") is not None and not (float(r["edge_abs"]) >= 0.0 and float(r["edge_rel"]) >= 0.0):
        raise ValueError(f"edge_abs and edge_rel must be >= 0 (edge_rel=None: no edge test), got {r['edge_abs']}, {r['edge_rel']}")


def _rule(rule: dict) -> dict:
    bad = set(rule) - set(RULE_DEFAULTS)
    if bad:
        raise TypeError(f"unknown visibility parameter(s) {sorted(bad)}; known: {sorted(RULE_DEFAULTS)}")
    return {**RULE_DEFAULTS, **rule}


def _points(points):
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise RuntimeError(f"points: expected a tensor on the HIP device, got {getattr(points, 'device', type(points))} (no CPU fallback)")
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] < 3:
        raise TypeError("points must be fp32 [N, >= 3] (world x, y, z first)")
    return points if points.stride(1) == 1 else points.contiguous()


def visibility(points, views: Views, count=None, **rule):
    """(bits int32 [N, ceil(V / 32)], count int32 [N]) of `points` in the kept views of `views`; enqueues only."""
    r = _rule(rule)
    points = _points(points)
    if len(views) == 0:
        N = points.shape[0]
        return (torch.zeros(N, 0, dtype=torch.int32, device=points.device),
                count if count is not None else torch.zeros(N, dtype=torch.int32, device=points.device))
    return ops.lift_visibility(points, views.world_to_cam, views.intrinsics, views.depth, views.depth_scale, count=count, **r)


def default_views_per_pass(n_views: int) -> int:
    """A pass = the views one accumulate launch walks.  The default is ONE pass over all views of an `add`: every further pass reads
    and writes the running sums again, and at 150 k points / 256 views / 60 x 80 x 256 fp16 maps (630 MB, beyond the Infinity Cache)
    every cut measured slower - neighbouring points share rows, so the L2 already serves most taps (profiles/lift_2d.md has the
    sweep).  `views_per_pass` stays as an argument: the bits do not depend on it."""
    return max(int(n_views), 1)


class PointFeatureAccumulator:
    """Per-point features of one scene, accumulated over any number of batches of frames, as a 2D network delivers them.

    `add(views, maps)` only enqueues kernels (visibility once, one accumulate launch per scale and pass; one pass by default); `maps` is one channels-last
    tensor [V, Hf, Wf, C] or a list of `n_scales` of them (fp16 or fp32, any Hf, Wf per scale, the same C).  `result()` enqueues the
    finish kernels and returns a device tensor; nothing here reads the device.  The views must arrive in the same order for the same
    bits; how they are cut into `add` calls and passes does not matter.  One accumulator per stream."""

    def __init__(self, points, channels: int, n_scales: int = 1, views_per_pass: Optional[int] = None, **rule):
        self.rule = _rule(rule)
        self.points = _points(points)
        if channels < 64 or channels > ops.LIFT_MAX_CHANNELS or channels % 64:
            raise ValueError(f"PointFeatureAccumulator: channels must be a multiple of 64 up to {ops.LIFT_MAX_CHANNELS}, got {channels}")
        if n_scales < 1:
            raise ValueError("PointFeatureAccumulator: n_scales >= 1")
        if views_per_pass is not None and views_per_pass < 1:
            raise ValueError("PointFeatureAccumulator: views_per_pass >= 1 (None = the default)")
        self.channels, self.n_scales, self.views_per_pass = int(channels), int(n_scales), views_per_pass
        N, dev = self.points.shape[0], self.points.device
        self.sums = [torch.zeros(N, self.channels, dtype=torch.float32, device=dev) for _ in range(self.n_scales)]
        self.count = torch.zeros(N, dtype=torch.int32, device=dev)
        self.n_views = 0

    def add(self, views: Views, maps) -> None:
        maps = [maps] if isinstance(maps, torch.Tensor) else list(maps)
        if len(maps) != self.n_scales:
            raise ValueError(f"PointFeatureAccumulator.add: expected {self.n_scales} scale(s) of maps, got {len(maps)}")
        for m in maps:
            if not isinstance(m, torch.Tensor) or m.dim() != 4 or m.shape[3] != self.channels:
                raise ValueError(f"PointFeatureAccumulator.add: maps must be channels-last [V, Hf, Wf, {self.channels}]")
            if m.dtype not in (torch.float16, torch.float32):
                raise TypeError(f"PointFeatureAccumulator.add: maps must be fp16 or fp32, got {m.dtype}")
            if not m.is_cuda:
                raise RuntimeError(f"maps: expected a tensor on the HIP device, got {m.device} (no CPU fallback)")
        maps = [views.select_maps(m).contiguous() for m in maps]
        V = len(views)
        if V == 0:
            return
        bits, _ = visibility(self.points, views, count=self.count, **self.rule)
        step = self.views_per_pass or default_views_per_pass(V)
        hw = (views.height, views.width)
        for v0 in range(0, V, step):
            for s, m in enumerate(maps):
                ops.lift_accumulate(self.points, views.world_to_cam, views.intrinsics, hw, bits, m, self.sums[s], v0, min(V, v0 + step))
        self.n_views += V

    def counts(self) -> torch.Tensor:
        """int32 [N]: the number of views that see each point so far (the live device tensor)."""
        return self.count

    def result(self, out_dtype=torch.float32, return_scales: bool = False):
        """[N, C] = the mean over the scales of the per-scale means; with `return_scales` the list of per-scale means instead (what
        the reference's per-scene dump holds).  May be called at any time; the accumulator goes on."""
        if return_scales:
            return [ops.lift_finish(s, self.count, out_dtype=out_dtype) for s in self.sums]
        acc = torch.empty_like(self.sums[0]) if self.n_scales > 1 else None
        out = None
        for i, s in enumerate(self.sums):
            out = ops.lift_finish(s, self.count, i, self.n_scales, acc=acc, out_dtype=out_dtype)
        return out


def lift_point_features(points, views: Views, maps, views_per_pass: Optional[int] = None, out_dtype=torch.float32, return_counts: bool = False,
                        **rule):
    """The one-shot form: points fp32 [N, >= 3], `views`, `maps` one tensor or a list (one per scale) -> [N, C], ready for
    `io_scene.pack_scene(..., "points_2dfeats": ...)` or `extra_features["points_2dfeats"]`."""
    m0 = maps if isinstance(maps, torch.Tensor) else maps[0]
    acc = PointFeatureAccumulator(points, m0.shape[-1], 1 if isinstance(maps, torch.Tensor) else len(maps), views_per_pass=views_per_pass, **rule)
    acc.add(views, maps)
    out = acc.result(out_dtype=out_dtype)
    return (out, acc.counts()) if return_counts else out
