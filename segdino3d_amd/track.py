"""Camera tracking against the TSDF volume on the device (csrc/track.hip): what turns an ordered stream of UNPOSED RGB-D frames into
poses and a fused volume, so that `lift2d.Views -> tsdf_mesh / fuse_views -> mesh_superpoints -> lift2d / lift_queries -> forward ->
transfer` has an input for someone who holds a sensor and no offline pose tool.  The volume `tsdf.TsdfVolume` keeps is a signed
distance field; aligning a new depth frame to it is a small non-linear least-squares problem: back-project the pixels, read the field
where they land, move the camera until they land on the zero level (frame-to-model tracking on the SDF itself, as Bylow et al.,
"Real-time camera tracking and 3D reconstruction using signed distance functions", and the SDF-Tracker do; no ray-caster, no vertex
or normal maps).  The reference reads poses made offline and ships no tracker, so there is nothing to pin against: the rule below is
restated in numpy in tests/track_ref.py, and the kernels are tested to EQUAL that, bit for bit.

THE LIMIT: the field is known within `trunc` of the surface, so the basin of convergence is about `trunc`.  The motion between two
frames must stay WELL UNDER `trunc` (at the defaults `voxel=0.02, trunc=0.08`, on the room of the tests: 2 cm + 0.7 degrees and 6 cm +
2.1 degrees a frame converge, 12 cm + 4.2 degrees does not; it is not lost either, the solve stays well-posed, but its `e` stays
at an rms of 0.2 `trunc` where a tracked frame ends near 0.03: read `info.e / info.count`).  Numbers: profiles/track.md.

State per tracker: the current `cam_to_world` `[R | t]` as float64 [3, 4] on the device.  Steps 1 to 4 read its fp32 rounding.
Host constants, each made in float64 and rounded once to fp32: `inv_voxel = float32(1 / voxel)`, `voxel_f = float32(voxel)`,
`ymax = float32(far * sqrt(3))`, `damping_f`, `max_rot_f`, `max_trans_f`; step 5 widens them to float64 again.

One ITERATION at stride `s`:

  1. Samples.  A sample is a depth pixel `(vi, ui)` with `vi % s == 0` and `ui % s == 0` that is valid by step 1 of the TSDF rule
     (`tsdf.py`): `d = (float)raw * depth_scale`, `d > 0`, `near <= d <= far`, and no 4-neighbour AT FULL RESOLUTION is a jump.
  2. Position.  `p = ((ui - cx) d / fx, (vi - cy) d / fy, d)` with the arithmetic of csrc/backproject.h; `y_i = (R_i0 p_x + R_i1 p_y)
     + R_i2 p_z`, the point relative to the camera centre; `w_i = y_i + t_i`.  All `|w_i| < 2^14` and all `|y_i| <= ymax`, compared as
     floats, or the sample is dropped (a camera whose field of view is under 90 degrees an axis never meets the second test; it is
     what bounds the integer sums below whatever the intrinsics are).
  3. Field.  `g_i = w_i * inv_voxel - 0.5f`, `c_i = floorf(g_i)`, `f_i = g_i - c_i`.  The eight voxels `c + {0,1}^3` must lie in
     `[-2^20, 2^20)` (as floats: `c_i >= -2^20` and `c_i + 1 < 2^20`) and have `W >= track_min_weight` - the tracker's own
     parameter, default 1: after the first frame nothing has `W >= 2`.  Each voxel's value is `float32((double) T / (double) W) *
     float32(1 / 4096)`: step 5 of the TSDF rule in units of `trunc`, in [-1, 1].  `phi` is the trilinear interpolant, lerped along
     x, then y, then z, each lerp `a + (b - a) * f`.  `n` is its analytic gradient in `trunc` per voxel: for each axis the four
     corner differences along it (`upper - lower`), lerped along the two other axes in the same order (x before y before z).  No
     ninth voxel is read.  The lookups go through the block table of the volume's workspace.
  4. Row.  `q = y * inv_voxel` (voxels); `J = (q x n, n)`, the cross product term by term (`q_1 n_2 - q_2 n_1`, ...), six fp32
     numbers; `Jq_k = (int) rintf(J_k * 1024)`, `rq = (int) rintf(phi * 16384)`.  From here integers only: `A += Jq Jq^T` (21 sums,
     the upper triangle row-major), `b += Jq rq` (6), `count += 1`, `e += rq rq`, all int64: a function of the SET of samples.
  5. Solve.  One lane, float64, one rounding per operation, only `+ - * /`.  `A_kk *= 1 + damping`; an `A_kk` whose integer
     sum is exactly 0 (no sample moves with that variable: its row, its column and `b_k` are 0 too, as for the sliding directions of
     a wall that lies along the voxel grid) becomes 1, which leaves `x_k = 0`.  `L D L^T` without pivoting:
     for `j = 0 .. 5`: `d_j = A_jj - sum_{m<j} L_jm (L_jm D_m)` (subtracted one at a time, m ascending), then for `i > j`:
     `L_ij = (A_ij - sum_{m<j} L_jm (L_im D_m)) / d_j`.  Forward: `z_i = b_i - sum_{m<i} L_im z_m`; back, `i = 5 .. 0`: `x_i = z_i /
     D_i - sum_{m>i} L_mi x_m` (m ascending).  `x = -(x / 16)`: the two fixed-point scales leave exactly that power of two.  The
     iteration is LOST iff `count < min_samples`, a pivot fails `d_j > 0`, a component of `x` is not finite, `(x_0^2 + x_1^2) + x_2^2
     > max_rot^2` or the same sum over `x_{3+i} * voxel` exceeds `max_trans^2`.  The defaults (0.5 rad, `4 trunc`) only catch
     divergence.
  6. Update.  `a = x[0:3] / 2`, `dR = ((1 - a.a) I + 2 a a^T + 2 [a]_x) / (1 + a.a)`, the Cayley map (rational; exactly orthogonal
     in real arithmetic), entries as `((1 - a.a) + 2 (a_i a_i)) / (1 + a.a)` and `(2 (a_i a_j) -+ 2 a_k) / (1 + a.a)`; `R <- dR R`,
     each entry `(dR_i0 R_0j + dR_i1 R_1j) + dR_i2 R_2j`; `t <- t + x[3:6] * voxel`.  All in float64.  This is a rotation about
     the camera centre, which is why the row uses `q` and not the world position.

The damping makes a degenerate scene harmless: with a single wall `A` has rank 3 and `b` lies in its range, so the sliding directions
come out as (numerically) zero motion instead of a failed pivot.

Widths.  `|n_k| <= 2` (differences of values in [-1, 1]) and `|q_i| <= Q = ymax * inv_voxel`, so `|(q x n)_k| <= 4 Q` and `|Jq_k| <=
4096 Q + 2` with the roundings; `|rq| <= 16384`.  The largest sum is an `A_kk` over at most `ceil(H / s) * ceil(W / s)` samples: `add`
and the C entry point refuse parameters with `(4096 Q + 2)^2 * samples >= 2^63` (at `far = 6, voxel = 0.02`, 480 x 640: 1.4e18).

A FRAME starts from the state (the previous frame's pose is the initial guess) and runs a fixed `schedule` of `(stride, iterations)`,
default `((4, 3), (2, 3), (1, 3))`: nothing on the host depends on the data.  Once an iteration is lost, the rest of the frame's
iterations do nothing, the state goes back to its value before the frame, the frame's pose is emitted as NaN and `lost` is set;
`count` and `e` are those of the last iteration that ran.  Otherwise the pose is emitted as float64 [3, 4] together with the fp32
`cam_to_world` and the fp32 `world_to_cam = [R^T | -(R^T t)]`, the translation as `-((R_0i t_0 + R_1i t_1) + R_2i t_2)` in float64,
every entry rounded once.  The frame is then integrated into the volume with exactly those two fp32 matrices
(`TsdfVolume.add_posed`).  A lost frame goes through the same two launches: by the TSDF rule every sample of a non-finite pose fails
`|w| < 2^14`, is counted in `out_of_range` and writes nothing, so `TsdfInfo.out_of_range` INCLUDES the samples of lost frames.  The
next frame tries again from the last good pose.  Frame 0 takes `first_pose` and is integrated without tracking.

Not built: loop closure and global optimisation (the drift of a long trajectory stays), a constant-velocity or IMU prior (the guess
is the previous pose), colour / photometric terms, robust weights (a moving object pulls the pose), relocalisation after long loss
(a tracker that stays lost needs a pose from outside: `align` from a guess)."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .lift2d import check_colors
from .tsdf import TsdfVolume

DEFAULT_SCHEDULE = ((4, 3), (2, 3), (1, 3))
MAX_ITERATIONS = 256                # of one frame's schedule: a frame is that many launches

TrackInfo = namedtuple("TrackInfo", "count e")
TrackInfo.__doc__ = """Host integers read by `poses()`: per frame, the samples `count` and the squared residual `e` (units of trunc / 16384,
squared and summed) of the last iteration that ran; 0 for frame 0."""


def _schedule(schedule):
    try:
        sched = tuple((int(s), int(n)) for s, n in schedule)
        same = all(int(s) == s and int(n) == n for s, n in schedule)
    except (TypeError, ValueError):
        raise TypeError(f"schedule must be a sequence of (stride, iterations) pairs, got {schedule!r}") from None
    if not same or not sched or any(not 1 <= s <= ops.TRACK_MAX_STRIDE or n < 1 for s, n in sched):
        raise ValueError(f"schedule needs at least one (stride, iterations) pair of integers with 1 <= stride <= {ops.TRACK_MAX_STRIDE} and "
                         f"iterations >= 1, got {schedule!r}")
    if sum(n for _, n in sched) > MAX_ITERATIONS:
        raise ValueError(f"schedule: at most {MAX_ITERATIONS} iterations a frame, got {sum(n for _, n in sched)}")
    return sched


def _pose(pose, who, name="first_pose"):
    p = np.asarray(pose.detach().cpu().numpy() if isinstance(pose, torch.Tensor) else pose, dtype=np.float64)
    if p.shape != (4, 4) or not np.isfinite(p).all():
        raise ValueError(f"{who}: {name} must be a finite float64 [4, 4] cam_to_world, got shape {list(p.shape)}")
    return np.array(p[:3])                                                             # a copy: the caller's array may be read-only


class _Params:
    """The tracker's own parameters, checked once."""

    def __init__(self, who, voxel, trunc, far, schedule, track_min_weight, min_samples, damping, max_rot, max_trans):
        self.schedule = _schedule(schedule)
        if int(track_min_weight) != track_min_weight or track_min_weight < 1:
            raise ValueError(f"{who}: track_min_weight must be an integer >= 1, got {track_min_weight}")
        if int(min_samples) != min_samples or min_samples < 1:
            raise ValueError(f"{who}: min_samples must be an integer >= 1, got {min_samples}")
        if not 0.0 <= float(damping) <= 1.0:
            raise ValueError(f"{who}: damping must lie in [0, 1], got {damping}")
        max_trans = 4.0 * float(trunc) if max_trans is None else max_trans
        if not (0.0 < float(max_rot) < float("inf") and 0.0 < float(max_trans) < float("inf")):
            raise ValueError(f"{who}: max_rot and max_trans must be positive and finite, got {max_rot}, {max_trans}")
        if not 0.0 < float(far) < float("inf"):
            raise ValueError(f"{who}: tracking needs a finite far > 0 (it bounds the integer sums), got {far}")
        self.track_min_weight, self.min_samples, self.damping = int(track_min_weight), int(min_samples), float(damping)
        self.max_rot, self.max_trans = float(max_rot), float(max_trans)
        self.ymax = float(far) * math.sqrt(3.0)
        self.q = float(np.float32(self.ymax)) * float(np.float32(1.0 / float(voxel)))

    def check_width(self, who, H, W):
        s = min(s for s, _ in self.schedule)
        samples = -(-H // s) * -(-W // s)
        jq = 4096.0 * self.q * 1.001 + 2.0
        if not (jq < 2.0 ** 31 and jq * jq * samples < 9.0e18):
            raise ValueError(f"{who}: the int64 sums need (4096 far sqrt(3) / voxel + 2)^2 * samples < 2^63; {H} x {W} at stride {s} with "
                             f"far sqrt(3) / voxel = {self.q:.0f} breaks it: use a smaller far, a larger voxel or a larger stride")


def _frame_args(who, depth, intrinsics, depth_scale):
    for t, name in ((depth, "depth"), (intrinsics, "intrinsics")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: {name}: expected a tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise RuntimeError(f"{who}: {name}: expected a tensor on the HIP device, got {t.device} (no CPU fallback)")
    if depth.dtype not in (torch.uint16, torch.float32):
        raise TypeError(f"{who}: depth must be uint16 or fp32, got {depth.dtype}")
    if depth.dtype == torch.uint16 and (depth_scale is None or not float(depth_scale) > 0.0):
        raise ValueError(f"{who}: uint16 depth needs a depth_scale > 0 (ScanNet: 0.001)")
    if depth.dtype == torch.float32 and depth_scale is not None:
        raise ValueError(f"{who}: fp32 depth is in metres and takes no depth_scale")
    if intrinsics.dtype != torch.float32:
        raise TypeError(f"{who}: intrinsics must be fp32, got {intrinsics.dtype}")


def _run_frame(p: _Params, volume: TsdfVolume, state, depth, depth_scale, intrinsics):
    """begin + the schedule for one frame [Hd, Wd]: enqueues only."""
    r = volume.rule
    ops.track_begin(state)
    for stride, iters in p.schedule:
        for _ in range(iters):
            ops.track_iterate(depth, depth_scale, intrinsics, state, volume._ws, volume.capacity, stride, volume.inv_voxel, volume.voxel, p.ymax,
                              p.track_min_weight, p.min_samples, p.damping, p.max_rot, p.max_trans, r["near"], r["far"], r["edge_abs"],
                              r["edge_rel"])


class Tracker:
    """Tracks an ordered stream of RGB-D frames against the volume it fuses them into.

    `add(depth, intrinsics, colors, depth_scale)` takes frames IN ORDER and only enqueues: per frame a begin, the schedule's iterations
    (an accumulate and a one-lane solve launch each), an end, and the touch and integrate launches of the fusion.  `poses()` makes
    the one host read.  `volume` is the `tsdf.TsdfVolume` (`mesh()`, `state()`); `info` holds the per-frame final `count` and `e`
    after `poses()`.  The bits do not depend on how the frames are cut into `add` calls or on the stream.  One tracker per stream."""

    def __init__(self, voxel: float = 0.02, trunc: float = 0.08, capacity: int = 1 << 16, schedule=DEFAULT_SCHEDULE, track_min_weight: int = 1,
                 min_samples: int = 64, damping: float = 1e-6, max_rot: float = 0.5, max_trans: float | None = None, first_pose=None,
                 **tsdf_rule):
        self.volume = TsdfVolume(voxel=voxel, trunc=trunc, capacity=capacity, **tsdf_rule)
        self._p = _Params("Tracker", voxel, trunc, self.volume.rule["far"], schedule, track_min_weight, min_samples, damping, max_rot,
                          max_trans)
        self.first_pose = _pose(np.eye(4) if first_pose is None else first_pose, "Tracker")
        self.n_frames = 0
        self.info = None
        self._state = None
        self._out = []                                  # per add: (pose float64 [V, 3, 4], info int64 [V, 3])

    def add(self, depth, intrinsics, colors, depth_scale=None) -> None:
        who = "Tracker.add"
        _frame_args(who, depth, intrinsics, depth_scale)
        if depth.dim() != 3:
            raise ValueError(f"{who}: depth must be [V, Hd, Wd], got {list(depth.shape)}")
        V, H, W = depth.shape
        if tuple(intrinsics.shape) != (V, 4):
            raise ValueError(f"{who}: intrinsics must be [V = {V}, 4], got {list(intrinsics.shape)}")
        check_colors(colors, who, V)
        if V == 0:
            return
        self._p.check_width(who, H, W)
        depth, intrinsics, colors = depth.contiguous(), intrinsics.contiguous(), colors.contiguous()
        dev = depth.device
        if self._state is None:
            self._state = ops.track_state(dev)
            ops.track_pose_view(self._state).copy_(torch.from_numpy(self.first_pose))
        pose = torch.empty(V, 3, 4, dtype=torch.float64, device=dev)
        c2w, w2c = torch.empty(V, 3, 4, dtype=torch.float32, device=dev), torch.empty(V, 3, 4, dtype=torch.float32, device=dev)
        info = torch.empty(V, len(ops.TRACK_INFO), dtype=torch.int64, device=dev)
        for v in range(V):
            if self.n_frames == 0:
                ops.track_begin(self._state)                                          # frame 0: its pose is the first pose, nothing is tracked
            else:
                _run_frame(self._p, self.volume, self._state, depth[v], depth_scale, intrinsics[v])
            ops.track_end(self._state, pose[v], c2w[v], w2c[v], info[v])
            self.volume.add_posed(depth[v:v + 1], depth_scale, intrinsics[v:v + 1], c2w[v:v + 1], w2c[v:v + 1], colors[v:v + 1])
            self.n_frames += 1
        self._out.append((pose, info))

    def poses(self):
        """-> (cam_to_world float64 [N, 4, 4] on the host, NaN for lost frames; lost bool [N]): the one host read.  The poses go straight
        into `lift2d.Views(depth, intrinsics, poses, depth_scale)`, which drops the NaN ones."""
        if not self._out:
            self.info = TrackInfo(np.zeros(0, np.int64), np.zeros(0, np.int64))
            return np.zeros((0, 4, 4)), np.zeros(0, dtype=bool)
        n = self.n_frames
        both = torch.cat([torch.cat([p.reshape(-1, 12).view(torch.int64), i], dim=1) for p, i in self._out]).cpu()     # the one host read
        pose34 = both[:, :12].contiguous().view(torch.float64).numpy().reshape(n, 3, 4)
        info = both[:, 12:].numpy()
        poses = np.zeros((n, 4, 4))
        poses[:, :3], poses[:, 3, 3] = pose34, 1.0
        lost = info[:, 0] != 0
        poses[lost] = np.nan
        self.info = TrackInfo(info[:, 1].copy(), info[:, 2].copy())
        return poses, lost


def align(volume: TsdfVolume, depth, intrinsics, pose, depth_scale=None, schedule=DEFAULT_SCHEDULE, track_min_weight: int = 1,
          min_samples: int = 64, damping: float = 1e-6, max_rot: float = 0.5, max_trans: float | None = None, return_info: bool = False):
    """One frame - depth [H, W], intrinsics fp32 [4] - against an existing volume from the guess `pose` (float64 [4, 4]); nothing is
    integrated and the volume is only read.  -> cam_to_world float64 [4, 4] ON THE DEVICE (NaN when the frame was lost), then info
    int64 [3] = (lost, count, e) on the device with `return_info`.  Enqueues only.  Use it to relocalise a frame in a scene that is
    already fused."""
    who = "align"
    if not isinstance(volume, TsdfVolume):
        raise TypeError(f"{who}: volume must be a tsdf.TsdfVolume, got {type(volume).__name__}")
    _frame_args(who, depth, intrinsics, depth_scale)
    if depth.dim() != 2 or tuple(intrinsics.shape) != (4,):
        raise ValueError(f"{who}: one frame: depth [H, W] and intrinsics [4], got {list(depth.shape)} and {list(intrinsics.shape)}")
    if volume._ws is None:
        raise RuntimeError(f"{who}: the volume is empty: there is nothing to align to")
    p = _Params(who, volume.voxel, volume.trunc, volume.rule["far"], schedule, track_min_weight, min_samples, damping, max_rot, max_trans)
    p.check_width(who, depth.shape[0], depth.shape[1])
    first = _pose(pose, who, "pose")
    state = ops.track_state(depth.device)
    ops.track_pose_view(state).copy_(torch.from_numpy(first))
    _run_frame(p, volume, state, depth.contiguous(), depth_scale, intrinsics.contiguous())
    out = torch.zeros(4, 4, dtype=torch.float64, device=depth.device)
    out[3, 3] = 1.0
    pose34, _, _, info = ops.track_end(state)
    out[:3] = pose34
    out = torch.where(info[0] != 0, torch.full_like(out, float("nan")), out)
    return (out, info) if return_info else out


def track_and_fuse(depth, intrinsics, colors, depth_scale=None, **kw):
    """The one-shot form: an ordered stream of frames -> (poses float64 [V, 4, 4] on the host, lost bool [V], the `TsdfVolume`)."""
    tracker = Tracker(**kw)
    tracker.add(depth, intrinsics, colors, depth_scale)
    poses, lost = tracker.poses()
    return poses, lost, tracker.volume
