"""TSDF fusion of posed RGB-D frames and a surface-net mesh of the fused volume on the device (csrc/tsdf.hip): the producer of a MESH -
`vertices` [V, 6] in the layout of `points` (xyz, rgb 0-255) and `faces` [F, 3] - so that a user who starts from frames can feed
`superpoints.mesh_superpoints`, the superpoint rule the network saw in training, without an offline tool:
`lift2d.Views -> tsdf_mesh -> mesh_superpoints -> lift2d / lift_queries -> forward`.  The reference reads meshes made offline and ships
no code that makes one, so there is nothing to pin against: the rule below is restated in numpy in tests/tsdf_ref.py, and the kernels
are tested to EQUAL that, bit for bit.

Inputs per batch of frames: a `lift2d.Views` (depth uint16 with `depth_scale` or fp32 metres, intrinsics, the fp32 `cam_to_world` and
`world_to_cam` [K, 3, 4] it keeps; views with a non-finite pose are dropped) and `colors` uint8 [V, Hc, Wc, 3] on the device, one per
given or per kept view, at any resolution.

Parameters: `voxel` 0.02, `trunc` 0.08 (`voxel <= trunc <= 8 voxel`: the band is at most one block), `near` 0.1, `far` 6.0, `edge_abs`
0.02, `edge_rel` 0.02 (`None` turns the edge test off), `min_weight` 2, `capacity` 2^16 BLOCKS of 8 x 8 x 8 voxels (a power of two).
Host constants, each made in float64 and rounded once: `voxel_f = float32(voxel)`, `inv_voxel = float32(1 / voxel)`,
`trunc_f = float32(trunc)`, `h = float32(trunc / 2)`, `qscale = float32(4096 / trunc)`.

  1. Valid pixel and colour pixel.  Steps 1 to 3 of `fuse_views` with stride 1, the same rule: `d = (float)raw * depth_scale`, one
     rounded fp32 multiply (fp32 depth as it is); valid iff `d > 0`, `d >= near`, `d <= far` (a NaN fails) and none of the 4 neighbours
     inside the image is a jump, `!(dn > 0)` or `|dn - d| > edge_abs + edge_rel * d` (one rounded multiply, add, subtract).  Depth pixel
     `(vi, ui)` reads colour pixel `(((2 vi + 1) Hc) // (2 Hd), ((2 ui + 1) Wc) // (2 Wd))`.
  2. Touched blocks of a view.  For each valid pixel and `j = -2 .. 2`: `d_j = d + (float)j * h` (the product is exact, the sum one
     rounded add) is back-projected by the device function `fuse_views` and `lift_queries` use (`x = (ui - cx) * d_j / fx`, `y`
     likewise, `w_i = ((R_i0 x + R_i1 y) + R_i2 d_j) + R_i3`, left to right, no fused multiply-add).  Unless all `|w_i| < 2^14` and
     `c_i = floorf(w_i * inv_voxel)` lies in `[-2^20, 2^20)` on all axes, compared as floats, the sample is counted in `out_of_range`.
     Otherwise the view TOUCHES the block `b_i = c_i >> 3` (an arithmetic shift: negative coordinates are ordinary), key
     `((b_x + 2^17) << 36) | ((b_y + 2^17) << 18) | (b_z + 2^17)`.
  3. Integration, per (view, touched block) pair and per each of the block's 512 voxels `c`.  Centre `p_i = ((float)c_i + 0.5f) *
     voxel_f`.  Camera point through the fp32 `world_to_cam`: `((r0 p_x + r1 p_y) + r2 p_z) + t` per row, left to right.  `z > 0`.
     `uf = floorf(((fx * x) / z + cx) + 0.5f)`, `vf` likewise; `0 <= uf < Wd` and `0 <= vf < Hd` compared as floats before anything
     becomes an index.  The pixel `(vf, uf)` must be valid by step 1, with depth `d`.  `sdf = d - z`; skipped if `sdf < -trunc_f`;
     `q = (int) rintf(fminf(sdf, trunc_f) * qscale)`.  Per voxel, integers only: `W += 1`, `T += q`, `C_j += colour byte j`.
     A view contributes to a voxel only through a block it touched: that is part of the rule, and it is what makes the volume a
     function of the SET of views, whatever the order and the cut of the `add` calls.
  4. Voxel state.  Observed iff `W >= min_weight`; inside iff `T < 0` (`T == 0` is outside).
  5. Vertices (naive surface nets: one per cell, no case table).  Cell `c` has the corner voxels `c + {0,1}^3`, across block borders.
     It is active iff all eight are observed and their signs are not all equal.  Its 12 edges are walked in a fixed order: the four
     x-edges at `(y, z) = (0,0), (0,1), (1,0), (1,1)`, then the four y-edges at `(x, z)` and the four z-edges at `(x, y)` in the same
     order (the earlier axis is the major one), each from its lower end `a` to its upper end `b`.  An edge whose ends differ in sign
     crosses at `s = f_a / (f_a - f_b)` along its axis, with `f = float32((double) T / (double) W)`; the divisor is never 0 since
     exactly one end has `f < 0`.  `m` = the fp32 sums of the crossings' coordinates in the cell (`s` on the edge's axis, 0 or 1 on the
     others) in that order, divided once by their number; `vertex_i = ((float)c_i + (0.5f + m_i)) * voxel_f`.  Colour: the integer sums
     over the eight corners, `rgb_j = float32((double) sum C_j / (double) sum W)`.  Vertices come out in ascending cell key
     `((c_x + 2^20) << 42) | ((c_y + 2^20) << 21) | (c_z + 2^20)`, the key layout of `fuse_views`.
  6. Faces.  A grid edge `a -> a + e_k` with both ends observed and of different sign emits one quad iff the four cells around it are
     active: with `(u, w) = (k + 1, k + 2) mod 3`, `q0 = a - e_u - e_w`, `q1 = a - e_w`, `q2 = a`, `q3 = a - e_u`, which turn about
     `+e_k`.  Two triangles split on the diagonal `q0 q2`: `(q0 q1 q2), (q0 q2 q3)` if `a` is inside, `(q0 q2 q1), (q0 q3 q2)`
     otherwise, so that the right-hand normal points from the inside end to the outside end, towards observed free space.  Faces come
     out in ascending `(key of a, k)`, the two triangles of a quad adjacent, as int32 indices into the vertex order.

Widths.  `W`, `T` and `C_j` are 32-bit.  `|q| <= 4097` (`trunc_f * qscale` is 4096 within two roundings), so `MAX_VIEWS = 2^17` kept
views per volume keep `|T| <= 2^17 * 4097 < 2^30`, `C_j <= 2^17 * 255 < 2^25` and `W <= 2^17`; `add` refuses more.

The block table has `capacity` slots and does not grow; a block costs 12 KiB + 20 bytes (20 bytes a voxel and a 4-byte cell-to-vertex
entry per cell, a key, a touched word and a list entry).  A block that finds no slot within the probe limit counts into `overflow`,
and `mesh()` then raises: a scene that does not fit is an error, not a thinner mesh.  `mesh()` writes at most `max_vertices` vertices
(default 16 per block of capacity) and raises when the volume holds more.

Not built: reading image files, marching cubes proper (it needs a case table; the surface nets here put one vertex in a cell and so
round sharp edges), growing the table, free-space carving outside the touched blocks (a voxel in front of a surface
is only updated within the band, so an object that was removed between frames leaves its surface behind)."""
from __future__ import annotations

from collections import namedtuple

import torch

from . import ops
from .lift2d import Views, check_colors, check_depth_range

RULE_DEFAULTS = dict(near=0.1, far=6.0, edge_abs=0.02, edge_rel=0.02, min_weight=2)
MIN_VOXEL = 2.0 ** -6               # |w| < 2^14 then keeps every voxel index inside [-2^20, 2^20)
MAX_VIEWS = 1 << 17                 # kept views per volume: 2^17 * 4097 < 2^30 keeps the 32-bit sums of one voxel
VERTICES_PER_BLOCK = 16             # the default `max_vertices` per block of capacity

TsdfInfo = namedtuple("TsdfInfo", ops.TSDF_INFO)
TsdfInfo.__doc__ = """Host integers read by `mesh()`: vertices, faces, blocks (occupied slots), voxels_observed (W >= min_weight), updates
(voxel updates of step 3), out_of_range (samples dropped at step 2), overflow (blocks that found no slot; `mesh()` raises when it is
not 0)."""


def _rule(rule: dict) -> dict:
    bad = set(rule) - set(RULE_DEFAULTS)
    if bad:
        raise TypeError(f"unknown TSDF parameter(s) {sorted(bad)}; known: {sorted(RULE_DEFAULTS)}")
    r = {**RULE_DEFAULTS, **rule}
    if int(r["min_weight"]) != r["min_weight"] or r["min_weight"] < 1:
        raise ValueError(f"min_weight must be an integer >= 1, got {r['min_weight']}")
    check_depth_range(r)
    return r


class TsdfVolume:
    """The TSDF volume of one scene, accumulated over any number of batches of posed RGB-D frames, and its mesh.

    `add(views, colors)` only enqueues: a touch and an integrate launch per 64 kept views.  `mesh()` enqueues the extraction and makes
    the one host read, of the seven counters.  The bits do not depend on how the views are cut into `add` calls, on their order, or
    on the stream.  The table is allocated on the first `add` and does not grow.  One volume per stream."""

    def __init__(self, voxel: float = 0.02, trunc: float = 0.08, capacity: int = 1 << 16, **rule):
        self.rule = _rule(rule)
        if not float(voxel) >= MIN_VOXEL or float(voxel) == float("inf"):
            raise ValueError(f"TsdfVolume: voxel must be finite and >= 2^-6 m (voxel indices must fit 21 bits), got {voxel}")
        if not float(voxel) <= float(trunc) <= 8.0 * float(voxel):
            raise ValueError(f"TsdfVolume: need voxel <= trunc <= 8 * voxel (the band is at most one block), got voxel = {voxel}, trunc = {trunc}")
        self.voxel, self.trunc = float(voxel), float(trunc)
        self.capacity = ops._pow2_capacity(capacity, ops.TSDF_MIN_CAPACITY, ops.TSDF_MAX_CAPACITY, "TsdfVolume", " blocks")
        # float64 here; ops rounds each to fp32 once
        self.inv_voxel, self.half_step, self.qscale = 1.0 / self.voxel, self.trunc / 2.0, 4096.0 / self.trunc
        self.n_views = 0
        self._ws = None
        self.info = None

    def add(self, views: Views, colors) -> None:
        if not isinstance(views, Views):
            raise TypeError(f"TsdfVolume.add: views must be a lift2d.Views, got {type(views).__name__}")
        views.check_colors(colors, "TsdfVolume.add")
        K = len(views)
        if K == 0:
            return
        if self.n_views + K > MAX_VIEWS:
            raise ValueError(f"TsdfVolume.add: more than 2^17 views in one volume ({self.n_views} + {K}): the 32-bit sums of one voxel "
                             "are sized for that many; fuse the scene in parts")
        colors = views.select_maps(colors).contiguous()
        if self._ws is None:
            self._ws = ops.tsdf_workspace(self.capacity, colors.device)
        r, step = self.rule, ops.TSDF_MAX_CALL_VIEWS
        for i in range(0, K, step):
            s = slice(i, i + step)
            intr = views.intrinsics[s]
            vdepth = ops.tsdf_touch(views.depth[s], views.depth_scale, intr, views.cam_to_world[s], self._ws, self.capacity, self.inv_voxel,
                                    self.half_step, r["near"], r["far"], r["edge_abs"], r["edge_rel"])
            ops.tsdf_integrate(vdepth, intr, views.world_to_cam[s], colors[s], self._ws, self.capacity, self.voxel, self.trunc, self.qscale)
        self.n_views += K

    def add_posed(self, depth, depth_scale, intrinsics, cam_to_world, world_to_cam, colors) -> None:
        """`add` for frames whose poses are already ON THE DEVICE (`track.Tracker` makes them there): depth [V, Hd, Wd] uint16 with
        `depth_scale` or fp32 metres, intrinsics fp32 [V, 4], the fp32 `cam_to_world` and `world_to_cam` [V, 3, 4], colors uint8
        [V, Hc, Wc, 3].  Nothing is read back, so no view can be dropped here: a view with a non-finite pose goes through the same two
        launches, every one of its samples fails `|w| < 2^14` at step 2 and is counted in `out_of_range`, and it writes no voxel.
        Every view counts towards the 2^17 of a volume.  Enqueues only."""
        who = "TsdfVolume.add_posed"
        for t, name in ((depth, "depth"), (intrinsics, "intrinsics"), (cam_to_world, "cam_to_world"), (world_to_cam, "world_to_cam")):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{who}: {name}: expected a tensor, got {type(t).__name__}")
            if not t.is_cuda:
                raise RuntimeError(f"{who}: {name}: expected a tensor on the HIP device, got {t.device} (no CPU fallback)")
        if depth.dim() != 3:
            raise ValueError(f"{who}: depth must be [V, Hd, Wd], got {list(depth.shape)}")
        K = depth.shape[0]
        check_colors(colors, who, K)
        if K == 0:
            return
        if self.n_views + K > MAX_VIEWS:
            raise ValueError(f"{who}: more than 2^17 views in one volume ({self.n_views} + {K}): the 32-bit sums of one voxel "
                             "are sized for that many; fuse the scene in parts")
        if self._ws is None:
            self._ws = ops.tsdf_workspace(self.capacity, colors.device)
        r, step = self.rule, ops.TSDF_MAX_CALL_VIEWS
        for i in range(0, K, step):
            s = slice(i, i + step)
            vdepth = ops.tsdf_touch(depth[s], depth_scale, intrinsics[s], cam_to_world[s], self._ws, self.capacity, self.inv_voxel,
                                    self.half_step, r["near"], r["far"], r["edge_abs"], r["edge_rel"])
            ops.tsdf_integrate(vdepth, intrinsics[s], world_to_cam[s], colors[s], self._ws, self.capacity, self.voxel, self.trunc, self.qscale)
        self.n_views += K

    def mesh(self, return_info: bool = False, return_keys: bool = False, max_vertices: int | None = None):
        """-> vertices fp32 [V, 6] on the device (xyz, rgb 0-255) and faces int32 [F, 3], then a `TsdfInfo` with `return_info`, then the
        cell keys int64 [V] (ascending) with `return_keys`.  Raises RuntimeError when blocks were dropped for want of a slot or the
        volume holds more than `max_vertices` vertices (`self.info` then holds the counters).  May be called at any time; the volume
        goes on."""
        keys = None
        if self._ws is None:
            dev = torch.device("cuda", torch.cuda.current_device())
            vertices, faces = torch.empty(0, 6, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev)
            keys = torch.empty(0, dtype=torch.int64, device=dev)
            self.info = TsdfInfo(0, 0, 0, 0, 0, 0, 0)
        else:
            cap = int(max_vertices) if max_vertices is not None else VERTICES_PER_BLOCK * self.capacity
            vertices, keys, faces, info = ops.tsdf_mesh(self._ws, self.capacity, self.rule["min_weight"], self.voxel, cap, want_keys=return_keys)
            self.info = TsdfInfo(*(int(x) for x in info.tolist()))                     # the one host read
            if self.info.overflow > 0:
                raise RuntimeError(f"TsdfVolume: overflow = {self.info.overflow} blocks found no slot in a table of capacity = "
                                   f"{self.capacity} ({self.info.blocks} blocks held, {self.info.updates} updates, {self.info.out_of_range} "
                                   "out of range); the table does not grow: use a larger capacity or voxel")
            if self.info.vertices > cap:
                raise RuntimeError(f"TsdfVolume: the volume holds vertices = {self.info.vertices}, more than max_vertices = {cap}")
            n, f = self.info.vertices, self.info.faces
            # a view of a far larger buffer would pin it: copy
            vertices, faces, keys = vertices[:n].clone(), faces[:f].clone(), keys[:n].clone() if keys is not None else None
        out = (vertices, faces) + ((self.info,) if return_info else ()) + ((keys,) if return_keys else ())
        return out

    def state(self):
        """The voxel state sorted by block key, for tests: (block keys int64 [B], W int32 [B, 512], T int32 [B, 512], C int32 [B, 512,
        3]) on the device, voxel (lx, ly, lz) of a block at lx * 64 + ly * 8 + lz.  Synchronises."""
        if self._ws is None:
            dev = torch.device("cuda", torch.cuda.current_device())
            z = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)             # noqa: E731
            return torch.empty(0, dtype=torch.int64, device=dev), z(0, 512), z(0, 512), z(0, 512, 3)
        _, keys, vox = ops.tsdf_state_views(self._ws, self.capacity)
        slots = torch.nonzero(keys != -1).flatten()                                   # SD3D_EMPTY_KEY is all ones
        order = torch.argsort(keys[slots])
        slots = slots[order]
        v = vox[slots]
        return keys[slots], v[:, 0].contiguous(), v[:, 1].contiguous(), v[:, 2:5].permute(0, 2, 1).contiguous()


def tsdf_mesh(views: Views, colors, voxel: float = 0.02, trunc: float = 0.08, capacity: int = 1 << 16, return_info: bool = False,
              return_keys: bool = False, max_vertices: int | None = None, **rule):
    """The one-shot form: -> (vertices fp32 [V, 6], faces int32 [F, 3]), ready for `superpoints.mesh_superpoints(vertices[:, :3], faces)`,
    `lift2d.lift_point_features` and, after `io_scene.normalize_points_color`, the model."""
    volume = TsdfVolume(voxel=voxel, trunc=trunc, capacity=capacity, **rule)
    volume.add(views, colors)
    return volume.mesh(return_info=return_info, return_keys=return_keys, max_vertices=max_vertices)
