"""Fuse posed RGB-D frames into the scene's point cloud on the device (csrc/fuse_views.hip): the producer of `points` [N, 6] (xyz,
rgb), the input `superpoints.py`, `lift2d.py` and `lift_queries.py` start from.  The reference reads it from a file made offline from
ScanNet's meshes and ships no code that makes it, so there is no reference implementation to pin against: the rule below is restated
in numpy in tests/fuse_views_ref.py, and the kernels are tested to EQUAL that, bit for bit.

Inputs per batch of frames: a `lift2d.Views` (depth uint16 with `depth_scale` or fp32 metres, intrinsics, the fp32 `cam_to_world`
[K, 3, 4] it keeps; views with a non-finite pose are dropped) and `colors` uint8 [V, Hc, Wc, 3] on the device, one per given or per
kept view (`views.select_maps`), at any resolution.

Parameters: `voxel` 0.02, `near` 0.1, `far` 6.0, `stride` 1, `edge_abs` 0.02, `edge_rel` 0.02 (`None` turns step 3 off), `min_obs` 2,
`capacity` 2^21 slots (a power of two).

  1. Pixels.  Depth pixel `(vi, ui)` of view `v` takes part iff `vi % stride == 0 and ui % stride == 0`.  It reads the colour pixel
     `(((2 vi + 1) Hc) // (2 Hd), ((2 ui + 1) Wc) // (2 Wd))`: the sampling rule `lift_queries` uses for masks.
  2. Depth.  `d = (float)raw * depth_scale`, one rounded fp32 multiply (fp32 depth is used as it is).  The pixel is valid iff `d > 0`,
     `d >= near` and `d <= far`, compared in fp32; a NaN fails.
  3. Edges (flying pixels at depth discontinuities).  For each of the 4 neighbours `(vi +- 1, ui)`, `(vi, ui +- 1)` that lies inside
     the image, whatever the stride: `dn` is the neighbour's depth by step 2; it is a jump iff `!(dn > 0)` or
     `|dn - d| > edge_abs + edge_rel * d`, the right-hand side one rounded multiply then one rounded add, the difference one rounded
     subtract.  A pixel with any jump is dropped.
  4. Back-projection.  Exactly step 5 of `lift_queries`, the same device function: `x = (ui - cx) * d / fx`, `y` likewise,
     `w_i = ((R_i0 x + R_i1 y) + R_i2 d) + R_i3`, every operation rounded on its own, left to right, no fused multiply-add.  Unless all
     three `w_i` are finite with `|w_i| < 2^14` the pixel is dropped and counted in `out_of_range`.
  5. Cell.  `c_i = floorf(w_i * inv_voxel)` with `inv_voxel = float32(1.0 / voxel)` (the division on the host in float64, the multiply
     one rounded fp32 operation).  Unless `-2^20 <= c_i < 2^20` on all axes, compared as floats before anything becomes an integer,
     the pixel is dropped and counted in `out_of_range`.  Key: `((c_x + 2^20) << 42) | ((c_y + 2^20) << 21) | (c_z + 2^20)`.  `floor`,
     not truncation: negative coordinates are ordinary.
  6. Per cell, integers only: `n += 1`, `S_i += (int64) rint((double) w_i * 2^20)`, `C_j += colour byte j`; all sums are 64-bit, wide
     enough for 2^28 observations of one cell.
  7. Output.  The cells with `n >= min_obs` in ascending key order: `xyz_i = float32((double) S_i / (double) n / 2^20)`,
     `rgb_j = float32((double) C_j / (double) n)` on the 0-255 scale `io_scene.normalize_points_color` expects, `obs = n` as int32.

Step 6 is integer addition, so the result is a pure function of the SET of (view, pixel) observations: the bits are the same however
the views are cut into `add` calls, in whatever order they arrive, and on whatever stream.

The table has `capacity` slots and does not grow.  A cell that finds no slot within the probe limit is dropped and its pixels are
counted in `overflow`; `result()` then raises: a scene that does not fit is an error, not a thinner cloud.  Use a larger `capacity`
(64 bytes a slot) or a larger `voxel`.

Out of scope: reading image files, growing the table, per-point normals (`superpoints.point_superpoints` computes its own); a mesh
from the same frames is `tsdf.py`."""
from __future__ import annotations

from collections import namedtuple

import torch

from . import ops
from .lift2d import Views, check_depth_range

RULE_DEFAULTS = dict(near=0.1, far=6.0, stride=1, edge_abs=0.02, edge_rel=0.02, min_obs=2)
MIN_VOXEL = 2.0 ** -6               # |w| < 2^14 then keeps every cell index inside [-2^20, 2^20)
MAX_OBSERVATIONS = 1 << 28          # per fuser: what the 64-bit sums of ONE cell are sized for

FuseInfo = namedtuple("FuseInfo", ops.FUSE_INFO)
FuseInfo.__doc__ = """Host integers read by `result()`: n (points emitted), cells (occupied slots), pixels_used (observations added to a
cell), out_of_range (dropped at steps 4 and 5), overflow (dropped for want of a slot; `result()` raises when it is not 0)."""


def _rule(rule: dict) -> dict:
    bad = set(rule) - set(RULE_DEFAULTS)
    if bad:
        raise TypeError(f"unknown fusion parameter(s) {sorted(bad)}; known: {sorted(RULE_DEFAULTS)}")
    r = {**RULE_DEFAULTS, **rule}
    if int(r["stride"]) != r["stride"] or r["stride"] < 1:
        raise ValueError(f"stride must be an integer >= 1, got {r['stride']}")
    if int(r["min_obs"]) != r["min_obs"] or r["min_obs"] < 1:
        raise ValueError(f"min_obs must be an integer >= 1, got {r['min_obs']}")
    check_depth_range(r)
    return r


class PointCloudFuser:
    """The point cloud of one scene, accumulated over any number of batches of posed RGB-D frames.

    `add(views, colors)` only enqueues: one accumulate launch over the kept views.  `result()` enqueues the emit and makes the one
    host read, of the five counters.  The bits do not depend on how the views are cut into `add` calls, on their order, or on the
    stream.  The table is allocated on the first `add` (64 bytes a slot) and does not grow.  One fuser per stream."""

    def __init__(self, voxel: float = 0.02, capacity: int = 1 << 21, **rule):
        self.rule = _rule(rule)
        if not float(voxel) >= MIN_VOXEL or float(voxel) == float("inf"):
            raise ValueError(f"PointCloudFuser: voxel must be finite and >= 2^-6 m (cell indices must fit 21 bits), got {voxel}")
        self.voxel = float(voxel)
        self.capacity = ops._pow2_capacity(capacity, ops.FUSE_MIN_CAPACITY, ops.FUSE_MAX_CAPACITY, "PointCloudFuser")
        self.inv_voxel = 1.0 / self.voxel               # float64 here; ops.fuse_accumulate rounds it to fp32
        self.n_views, self.n_pixels = 0, 0
        self._ws = None
        self.info = None

    def add(self, views: Views, colors) -> None:
        if not isinstance(views, Views):
            raise TypeError(f"PointCloudFuser.add: views must be a lift2d.Views, got {type(views).__name__}")
        views.check_colors(colors, "PointCloudFuser.add")
        K = len(views)
        if K == 0:
            return
        r = self.rule
        pixels = K * -(-views.height // r["stride"]) * -(-views.width // r["stride"])
        if self.n_pixels + pixels > MAX_OBSERVATIONS:
            raise ValueError(f"PointCloudFuser.add: more than 2^28 observations in one fuser ({self.n_pixels} + {pixels}): the sums of one "
                             "cell are sized for that many; raise the stride or fuse the scene in parts")
        colors = views.select_maps(colors).contiguous()
        if self._ws is None:
            self._ws = ops.fuse_workspace(self.capacity, colors.device)
        ops.fuse_accumulate(views.depth, views.depth_scale, views.intrinsics, views.cam_to_world, colors, self._ws, self.capacity,
                            self.inv_voxel, r["stride"], r["near"], r["far"], r["edge_abs"], r["edge_rel"])
        self.n_views += K
        self.n_pixels += pixels

    def result(self, return_obs: bool = False, return_info: bool = False, return_keys: bool = False):
        """-> points fp32 [N, 6] on the device (xyz, rgb 0-255), then `obs` int32 [N] with `return_obs`, then a `FuseInfo` with
        `return_info`, then the cell keys int64 [N] (ascending) with `return_keys`.  Raises RuntimeError when cells were dropped for
        want of a slot (`self.info` then holds the counters).  May be called at any time; the fuser goes on."""
        keys = None
        if self._ws is None:
            dev = torch.device("cuda", torch.cuda.current_device())
            points, obs = torch.empty(0, 6, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
            keys = torch.empty(0, dtype=torch.int64, device=dev)
            self.info = FuseInfo(0, 0, 0, 0, 0)
        else:
            # a cell holds at least one observation: no more rows than pixels, and no more than slots
            cap = min(self.capacity, self.n_pixels)
            points, obs, keys, info = ops.fuse_emit(self._ws, self.capacity, self.rule["min_obs"], cap, want_keys=return_keys)
            self.info = FuseInfo(*(int(x) for x in info.tolist()))                     # the one host read
            if self.info.overflow > 0:
                raise RuntimeError(f"PointCloudFuser: overflow = {self.info.overflow} pixels found no slot in a table of capacity = "
                                   f"{self.capacity} ({self.info.cells} cells held); the table does not grow: use a larger capacity or voxel")
            n = self.info.n
            # a view of a far larger buffer would pin it: copy when the cloud is much smaller
            tight = (lambda t: t[:n].clone()) if 2 * n < cap else (lambda t: t[:n])
            points, obs, keys = tight(points), tight(obs), tight(keys) if keys is not None else None
        out = (points,) + ((obs,) if return_obs else ()) + ((self.info,) if return_info else ()) + ((keys,) if return_keys else ())
        return out[0] if len(out) == 1 else out


def fuse_views(views: Views, colors, voxel: float = 0.02, capacity: int = 1 << 21, return_obs: bool = False, return_info: bool = False,
               return_keys: bool = False, **rule):
    """The one-shot form: -> points fp32 [N, 6], ready for `superpoints.point_superpoints`, `lift2d.lift_point_features` and, after
    `io_scene.normalize_points_color`, the model."""
    fuser = PointCloudFuser(voxel=voxel, capacity=capacity, **rule)
    fuser.add(views, colors)
    return fuser.result(return_obs=return_obs, return_info=return_info, return_keys=return_keys)
