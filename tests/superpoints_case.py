"""Seeded triangle meshes shared by the CPU and GPU superpoint tests (numpy only).

`height_field`: an n x n grid with spacing 0.05, jittered in all three coordinates, with raised boxes; two triangles per cell, the face
order shuffled.  `boxes_on_plane`: the same layout without noise on a dyadic grid (x, y multiples of 1/32, box heights multiples of
1/16): flat ground, flat tops and a few wall directions, so only a hundred or so distinct edge weights occur and most edges tie."""
import numpy as np


def grid_faces(n, m=None):
    """Two triangles per cell of an n x m vertex grid (vertex r m + c) -> int64 [2 (n - 1) (m - 1), 3]."""
    m = n if m is None else m
    r, c = np.meshgrid(np.arange(n - 1), np.arange(m - 1), indexing="ij")
    v00 = (r * m + c).reshape(-1)
    v01, v10, v11 = v00 + 1, v00 + m, v00 + m + 1
    return np.concatenate([np.stack([v00, v01, v11], axis=1), np.stack([v00, v11, v10], axis=1)], axis=0).astype(np.int64)


def _boxes(n, rng, n_boxes, heights):
    z = np.zeros((n, n), dtype=np.float64)
    for _ in range(n_boxes):
        w, h = rng.integers(max(6, n // 8), max(8, n // 3), size=2)
        r0, c0 = rng.integers(1, max(2, n - w - 1)), rng.integers(1, max(2, n - h - 1))
        z[r0:r0 + w, c0:c0 + h] = heights[rng.integers(len(heights))]
    return z


def height_field(n, seed, n_boxes=None, jitter=0.004, shuffle=True):
    """-> (vertices float32 [n n, 3], faces int64 [2 (n - 1)^2, 3])."""
    rng = np.random.default_rng(seed)
    n_boxes = max(2, n // 12) if n_boxes is None else n_boxes
    z = _boxes(n, rng, n_boxes, np.array([0.2, 0.3, 0.45, 0.6]))
    r, c = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([c * 0.05, r * 0.05, z], axis=-1).reshape(-1, 3)
    v = v + rng.normal(0.0, jitter, size=v.shape)
    f = grid_faces(n)
    if shuffle:
        f = f[rng.permutation(len(f))]
    return v.astype(np.float32), f


def boxes_on_plane(n, seed, n_boxes=None, shuffle=True):
    """The noise-free case: every coordinate is dyadic, so normals repeat exactly and weights tie -> (vertices, faces)."""
    rng = np.random.default_rng(seed)
    n_boxes = max(2, n // 10) if n_boxes is None else n_boxes
    z = _boxes(n, rng, n_boxes, np.array([1, 2, 3, 5, 8]) / 16.0)
    r, c = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([c / 32.0, r / 32.0, z], axis=-1).reshape(-1, 3)
    f = grid_faces(n)
    if shuffle:
        f = f[rng.permutation(len(f))]
    return v.astype(np.float32), f


def crease(n=8, m=8):
    """Two flat n x m sheets meeting at a right angle along the row of vertices r = n - 1 (which belongs to both): the first in the
    plane z = 0, the second going up -> (vertices float32 [(2 n - 1) m, 3], faces)."""
    rows = 2 * n - 1
    v = np.zeros((rows, m, 3), dtype=np.float64)
    for r in range(rows):
        for c in range(m):
            v[r, c] = (c * 0.05, min(r, n - 1) * 0.05, max(r - (n - 1), 0) * 0.05)
    return v.reshape(-1, 3).astype(np.float32), grid_faces(rows, m)


def flat_grid(n):
    """A flat n x n grid with spacing 0.05 in the plane z = 0."""
    r, c = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([c * 0.05, r * 0.05, np.zeros_like(c, dtype=np.float64)], axis=-1).reshape(-1, 3).astype(np.float32)
    return v, grid_faces(n)


def grid_with_tail(tail_attached):
    """A flat 6 x 6 grid (36 vertices) and a small tilted triangle fan of 4 vertices, attached through one face or not at all."""
    v, f = flat_grid(6)
    fan = np.array([[1.0, 1.0, 0.0], [1.0, 1.1, 0.1], [1.0, 1.2, 0.0], [1.1, 1.1, 0.3]], dtype=np.float32)
    v = np.concatenate([v, fan])
    faces = [f, np.array([[36, 37, 39], [37, 38, 39]])]
    if tail_attached:
        faces.append(np.array([[35, 36, 37]]))
    return v, np.concatenate(faces)
