"""Inputs for the fusion tests (tests/fuse_views_ref.py, tests/test_gpu_fuse_views.py): a synthetic room rendered in closed form and
small hand-built scenes.  No file is read.

The room: a pinhole camera inside an axis-aligned box `ROOM_LO .. ROOM_HI` (metres, z up, the box crosses the origin so that negative
coordinates occur), with two axis-aligned boxes standing on the floor.  The depth of a pixel is the camera-z of the first surface its
ray meets (ray / plane intersections, float64), quantised to uint16 millimetres; the colour is a function of the surface hit and of
where it is hit.  Poses look around from a few positions.  Run as a script it prints the figures profiles/fuse_views.md records."""
import functools

import numpy as np

import fuse_views_ref as R

DEPTH_SCALE = 0.001
ROOM_LO, ROOM_HI = np.array([-2.1, -1.6, -0.3]), np.array([2.3, 1.9, 2.4])
BOXES = ((np.array([0.4, -0.5, -0.3]), np.array([1.1, 0.3, 0.5])), (np.array([-1.4, 0.6, -0.3]), np.array([-0.8, 1.2, 0.9])))
SURFACE_RGB = np.array([[200, 190, 170], [120, 140, 200], [90, 160, 110], [210, 120, 90], [160, 160, 160], [230, 220, 120],      # room faces
                        [200, 60, 60], [60, 60, 200]], dtype=np.float64)                                                          # the boxes


def look_at(eye, target):
    """cam_to_world float64 [4, 4]: camera x right, y down, z forward; the world's z is up."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, down, fwd, eye
    return pose


def room_poses(V):
    """V poses: a few standpoints, each looking around."""
    eyes = np.array([[0.1, 0.0, 1.2], [-0.9, -0.7, 1.4], [1.3, 0.9, 1.0], [0.3, 1.1, 1.6]])
    poses = []
    for i in range(V):
        e = eyes[i % len(eyes)]
        a = 2.0 * np.pi * (i * 0.381966 + 0.05)
        poses.append(look_at(e, e + np.array([np.cos(a), np.sin(a), -0.35 - 0.1 * (i % 3)])))
    return np.stack(poses)


def intrinsics(H, W, V):
    f = 0.9 * W
    return np.tile(np.array([f, f * 1.01, (W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2], dtype=np.float32), (V, 1))


def render(pose, H, W, fx, fy, cx, cy, scale=1.0):
    """Closed-form render at the pixel centres of an H x W image -> (camera-z float64 [H, W], surface index int64 [H, W], hit points
    float64 [H, W, 3]).  `scale`: the room and the boxes are scaled about the origin (the benchmark's ScanNet-sized room)."""
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1) @ pose[:3, :3].T     # camera-z grows by 1 per unit of t
    eye = pose[:3, 3]
    best, surf = np.full((H, W), np.inf), np.zeros((H, W), dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for axis in range(3):                                                          # the room, from inside: the far plane along each axis
            for side, bound in enumerate((ROOM_LO[axis] * scale, ROOM_HI[axis] * scale)):
                t = (bound - eye[axis]) / ray[..., axis]
                hit = (t > 0) & ((ray[..., axis] > 0) == bool(side)) & (t < best)
                best, surf = np.where(hit, t, best), np.where(hit, 2 * axis + side, surf)
        for b, (lo, hi) in enumerate(BOXES):                                           # the boxes, from outside: slabs
            t0 = (lo * scale - eye) / ray
            t1 = (hi * scale - eye) / ray
            tn, tf = np.minimum(t0, t1).max(axis=-1), np.maximum(t0, t1).min(axis=-1)
            hit = (tn < tf) & (tn > 0) & (tn < best)
            best, surf = np.where(hit, tn, best), np.where(hit, 6 + b, surf)
    return best, surf, eye + ray * best[..., None]


def shade(surf, hit):
    """The colour of a surface point: the surface's base colour, darker on the odd squares of a 0.25 m checker -> uint8 [H, W, 3]."""
    odd = (np.floor(hit / 0.25).sum(axis=-1).astype(np.int64) & 1).astype(np.float64)
    return np.clip(np.rint(SURFACE_RGB[surf] * (1.0 - 0.3 * odd[..., None])), 0, 255).astype(np.uint8)


def room(V, H, W, color_hw, scale=1.0):
    """dict(depth_u16 [V, H, W], depth_f32, intr fp32 [V, 4], poses float64 [V, 4, 4], colors uint8 [V, Hc, Wc, 3]); the colour camera
    is the depth camera at another resolution (pixel centres at (x + 0.5) W / Wc - 0.5)."""
    Hc, Wc = color_hw
    poses, intr = room_poses(V), intrinsics(H, W, V)
    poses[:, :3, 3] *= scale
    depth, colors = np.zeros((V, H, W), np.uint16), np.zeros((V, Hc, Wc, 3), np.uint8)
    for i in range(V):
        fx, fy, cx, cy = (float(x) for x in intr[i])
        z, _, _ = render(poses[i], H, W, fx, fy, cx, cy, scale)
        depth[i] = np.clip(np.rint(z / DEPTH_SCALE), 0, 65535).astype(np.uint16)
        sx, sy = Wc / W, Hc / H
        _, surf, hit = render(poses[i], Hc, Wc, fx * sx, fy * sy, (cx + 0.5) * sx - 0.5, (cy + 0.5) * sy - 0.5, scale)
        colors[i] = shade(surf, hit / scale)
    return dict(depth_u16=depth, depth_f32=depth.astype(np.float32) * np.float32(DEPTH_SCALE), intr=intr, poses=poses, colors=colors)


def _freeze(c):
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def room_case(color_hw=(60, 80)):
    """The tests' room: 8 views of 120 x 160.  Shared by the tests: read-only."""
    return _freeze(room(8, 120, 160, color_hw))


def wall(H, W, distance, plane_x=None, V=1, color_hw=None, seed=0):
    """A fronto-parallel wall: every pixel at camera-z `distance`, the camera looking along world +x (cam z -> world x, cam x -> world
    -y, cam y -> world -z) from the point that puts the wall at world x = `plane_x` (default: `distance`).  Views 1.. are shifted
    sideways by whole pixels' worth so that they see the same cells.  Random colours."""
    rng = np.random.default_rng(seed)
    Hc, Wc = color_hw or (H, W)
    poses = np.tile(np.eye(4), (V, 1, 1))
    for i in range(V):
        poses[i, :3, :3] = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
        poses[i, :3, 3] = [(distance if plane_x is None else plane_x) - distance, 0.004 * i, 0.003 * i]
    intr = np.tile(np.array([W * 1.0, W * 1.0, (W - 1) / 2, (H - 1) / 2], dtype=np.float32), (V, 1))
    depth = np.full((V, H, W), int(round(distance / DEPTH_SCALE)), dtype=np.uint16)
    return _freeze(dict(depth_u16=depth, depth_f32=depth.astype(np.float32) * np.float32(DEPTH_SCALE), intr=intr, poses=poses,
                        colors=rng.integers(0, 256, (V, Hc, Wc, 3), dtype=np.uint8)))


def noisy(H, W, V=1, seed=0, color_hw=None):
    """Random smooth-ish depth with holes (0) and steps: exercises every branch of steps 2 and 3 at any size."""
    rng = np.random.default_rng(seed)
    Hc, Wc = color_hw or (H, W)
    base = 900 + 40 * np.add.outer(np.arange(H) // 3, np.arange(W) // 4)
    depth = (base[None] + rng.integers(0, 12, (V, H, W))).astype(np.int64)
    depth[rng.random((V, H, W)) < 0.05] = 0
    depth[rng.random((V, H, W)) < 0.03] += 700
    poses = np.stack([look_at([0.2 * i, -0.1 * i, 0.0], [1.0 + 0.2 * i, 0.3, -0.2]) for i in range(V)])
    intr = np.tile(np.array([W * 0.8, W * 0.8, (W - 1) / 2 + 0.25, (H - 1) / 2], dtype=np.float32), (V, 1))
    depth = depth.astype(np.uint16)
    return _freeze(dict(depth_u16=depth, depth_f32=depth.astype(np.float32) * np.float32(DEPTH_SCALE), intr=intr, poses=poses,
                        colors=rng.integers(0, 256, (V, Hc, Wc, 3), dtype=np.uint8)))


def cell_shift_share(c=None, **kw):
    """The share of the room's observations whose cell differs between the float32 and the float64 back-projection."""
    c = c or room_case()
    c2w, kept = R.cam_to_world(c["poses"])
    a = R.observations(c["depth_u16"][kept], DEPTH_SCALE, c["intr"][kept], c2w, c["colors"][kept], np.float32, **kw)
    b = R.observations(c["depth_u16"][kept], DEPTH_SCALE, c["intr"][kept], c2w, c["colors"][kept], np.float64, **kw)
    assert len(a["key"]) == len(b["key"])                                             # nothing of the room is near a range limit
    return float((a["key"] != b["key"]).mean()), len(a["key"])


if __name__ == "__main__":
    share, P = cell_shift_share()
    c = room_case()
    c2w, kept = R.cam_to_world(c["poses"])
    obs = R.observations(c["depth_u16"], DEPTH_SCALE, c["intr"], c2w, c["colors"])
    cells, per_cell, per_pair = R.tile_stats(obs)
    print(f"room 8 x 120 x 160: {P} observations, {cells} cells, {per_cell:.2f} observations per cell, {per_pair:.2f} per (tile, cell); "
          f"cells moved by the float32 back-projection: {share:.3%}")
