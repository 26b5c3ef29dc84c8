"""Inputs shared by the nearest-point tests (tests/test_transfer_ref.py, tests/test_gpu_transfer.py).  No file is read; everything is
cached and read-only."""
import functools

import numpy as np

import fuse_views_case as FK
import fuse_views_ref as FR

F32 = np.float32


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def agreement_case():
    """(points [4000, 3] uniform in [-1, 1]^3, queries [8000, 3] uniform in [-1.1, 1.1]^3, radius 0.1), seed 0."""
    rng = np.random.default_rng(0)
    p = rng.uniform(-1.0, 1.0, (4000, 3)).astype(F32)
    q = rng.uniform(-1.1, 1.1, (8000, 3)).astype(F32)
    return _ro(p, q) + (0.1,)


@functools.lru_cache(maxsize=None)
def lattice_case():
    """(points [2000, 3], queries [4000, 3], radius 2^-4): every coordinate a multiple of 2^-6 in [-2, 2].  500 sites, four points
    within one lattice step of each (so points coincide and distances tie exactly); a query is a point moved by up to four steps
    per axis, so queries sit on, next to and just out of reach of their points, on both sides of the cell faces, edges and corners
    of any grid, with both signs of every coordinate."""
    rng = np.random.default_rng(1)
    sites = rng.integers(-126, 127, (500, 3))
    p = np.clip(np.repeat(sites, 4, axis=0) + rng.integers(-1, 2, (2000, 3)), -128, 128)
    p = p[rng.permutation(2000)]
    q = np.clip(p[rng.integers(0, 2000, 4000)] + rng.integers(-4, 5, (4000, 3)), -128, 128)
    return _ro((p / 64.0).astype(F32), (q / 64.0).astype(F32)) + (0.0625,)


@functools.lru_cache(maxsize=None)
def room_cloud(voxel=0.05):
    """The room of fuse_views_case.room_case() fused with min_obs = 1 and no edge test -> (points float32 [N, 3], the fusion's dict)."""
    c = FK.room_case()
    fused = FR.fuse(c["depth_u16"], FK.DEPTH_SCALE, c["intr"], c["poses"], c["colors"], voxel=voxel, min_obs=1, edge_rel=None)
    return _ro(np.ascontiguousarray(fused["points"][:, :3])), fused


def room_views():
    """(depth uint16 [8, 120, 160], intr fp32 [8, 4], c2w fp32 [8, 3, 4]) of the room's kept views (all eight)."""
    c = FK.room_case()
    c2w, kept = FR.cam_to_world(c["poses"])
    assert len(kept) == 8
    return c["depth_u16"], c["intr"], c2w


@functools.lru_cache(maxsize=None)
def broken_pose_case(kind="u16"):
    """fuse_views_case.noisy(24, 32, V=3) with the pose of view 1 made non-finite -> dict(depth, scale, intr, poses, kept, c2w)."""
    c = FK.noisy(24, 32, V=3)
    poses = np.array(c["poses"])
    poses[1, 0, 3] = np.nan
    c2w, kept = FR.cam_to_world(poses)
    depth, scale = (c["depth_u16"], FK.DEPTH_SCALE) if kind == "u16" else (c["depth_f32"], None)
    return dict(depth=depth, scale=scale, intr=c["intr"], poses=poses, kept=kept, c2w=c2w)


def labels_for(n, L, seed=0):
    """int32 [L, n] with -1 among the values."""
    return np.random.default_rng(seed).integers(-1, 40, (L, n)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def prediction_case(n, n_inst=12, seed=3):
    """A hand-made prediction over n points: the five fields `transfer.render_prediction` reads, as host arrays (overlapping bool
    masks, equal scores among them)."""
    rng = np.random.default_rng(seed)
    masks = rng.random((n_inst, n)) < 0.2
    scores = np.round(rng.random(n_inst), 1).astype(F32)                              # one decimal: ties
    return dict(pts_semantic_mask=[rng.integers(0, 20, n).astype(np.int64), rng.integers(0, 20, n).astype(np.int64)],
                pts_instance_mask=[masks, rng.integers(0, 9, n).astype(np.int64)],
                instance_labels=rng.integers(0, 200, n_inst).astype(np.int64), instance_scores=scores)
