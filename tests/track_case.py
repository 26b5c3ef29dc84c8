"""Inputs shared by the tracking tests (tests/test_track_ref.py, tests/test_gpu_track.py) and tools/track_bench.py: a trajectory through
the room of tests/fuse_views_case.py, and the restatement's result on it, computed once and read-only.  No file is read."""
import functools

import numpy as np

import fuse_views_case as K
import track_ref as R

DEPTH_SCALE = K.DEPTH_SCALE
ROOM_RULE = dict(voxel=0.02, trunc=0.08)            # the defaults of the tracker, where the issue's prototype converged
STEP = 0.02                                         # metres a frame; the turn that goes with it is 0.7 degrees


def trajectory_poses(V, step=STEP, turn_deg=0.7, scale=1.0):
    """V poses float64 [V, 4, 4]: the camera walks `step` metres a frame along a line through the room and turns `turn_deg` degrees a
    frame about the vertical while its pitch drifts, so that both parts of the motion are about the issue's 2 cm + 0.7 degrees."""
    poses = []
    for i in range(V):
        eye = np.array([-0.3, -0.2, 1.2]) * scale + step * i * np.array([0.8, 0.5, 0.33])
        a = np.deg2rad(20.0 + turn_deg * i)
        poses.append(K.look_at(eye, eye + np.array([np.cos(a), np.sin(a), -0.45 + 0.003 * i])))
    return np.stack(poses)


def trajectory(V, H, W, color_hw, step=STEP, turn_deg=0.7, scale=1.0):
    """The room rendered along `trajectory_poses` -> the dict of fuse_views_case.room."""
    Hc, Wc = color_hw
    poses, intr = trajectory_poses(V, step, turn_deg, scale), K.intrinsics(H, W, V)
    depth, colors = np.zeros((V, H, W), np.uint16), np.zeros((V, Hc, Wc, 3), np.uint8)
    for i in range(V):
        fx, fy, cx, cy = (float(x) for x in intr[i])
        z, _, _ = K.render(poses[i], H, W, fx, fy, cx, cy, scale)
        depth[i] = np.clip(np.rint(z / DEPTH_SCALE), 0, 65535).astype(np.uint16)
        sx, sy = Wc / W, Hc / H
        _, surf, hit = K.render(poses[i], Hc, Wc, fx * sx, fy * sy, (cx + 0.5) * sx - 0.5, (cy + 0.5) * sy - 0.5, scale)
        colors[i] = K.shade(surf, hit / scale)
    return dict(depth_u16=depth, depth_f32=depth.astype(np.float32) * np.float32(DEPTH_SCALE), intr=intr, poses=poses, colors=colors)


def _freeze(c):
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def room_trajectory():
    """The tests' trajectory: 5 frames of 120 x 160, colours 30 x 40.  Shared by the tests: read-only."""
    return _freeze(trajectory(5, 120, 160, (30, 40)))


@functools.lru_cache(maxsize=None)
def room_trajectory_ref():
    """The restatement on `room_trajectory`, frame 0 at its true pose.  Shared by the tests: read-only."""
    c = room_trajectory()
    out = R.track(c["depth_u16"], DEPTH_SCALE, c["intr"], c["colors"], first_pose=c["poses"][0], **ROOM_RULE)
    _freeze(out)
    for a in out["volume"]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def pose_error(a, b):
    """Two poses float64 [>= 3, 4] -> (translation distance in metres, rotation angle in degrees)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    dR = a[:3, :3] @ b[:3, :3].T
    return float(np.linalg.norm(a[:3, 3] - b[:3, 3])), float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))))


def one_view_volume(c, kind="u16", views=1, **tsdf_rule):
    """The tsdf_ref.Volume of the first `views` views of a fuse_views_case scene at their true poses."""
    import tsdf_ref as TR
    depth, scale = (c["depth_u16"], c.get("scale", DEPTH_SCALE)) if kind == "u16" else (c["depth_f32"], None)
    return TR.integrate(depth[:views], scale, c["intr"][:views], c["poses"][:views], c["colors"][:views], **tsdf_rule)


if __name__ == "__main__":
    c, out = room_trajectory(), room_trajectory_ref()
    for v in range(1, len(c["poses"])):
        t0, r0 = pose_error(c["poses"][v], c["poses"][v - 1] if v == 1 else out["poses"][v - 1])
        t1, r1 = pose_error(c["poses"][v], out["poses"][v])
        print(f"frame {v}: lost {bool(out['lost'][v])}, start {t0 * 1e3:.2f} mm {r0:.3f} deg -> {t1 * 1e3:.3f} mm {r1:.4f} deg "
              f"({t1 / t0:.4f}, {r1 / r0:.4f} of the start); count {out['count'][v]}, e {out['e'][v]}")
