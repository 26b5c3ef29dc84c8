"""Seeded point clouds shared by the CPU and GPU point-cloud superpoint tests (numpy only): the vertices of the meshes of
superpoints_case.py, and hand-made clouds that put the k-NN search on its edges."""
import numpy as np

import superpoints_case as K

F32 = np.float32


def mesh_vertices(kind, *args):
    """The vertices alone of `superpoints_case.<kind>(*args)`."""
    return np.ascontiguousarray(getattr(K, kind)(*args)[0], dtype=F32)


def mesh_graph(kind, *args):
    """A mesh as a graph: (vertices, edges int64 [3 F, 2]) with edge 3 f + k of face (i, j, k) = (i, j), (i, k), (k, j)."""
    v, f = getattr(K, kind)(*args)
    f = np.asarray(f, dtype=np.int64)
    a = np.stack([f[:, 0], f[:, 0], f[:, 2]], axis=1).reshape(-1)
    b = np.stack([f[:, 1], f[:, 2], f[:, 1]], axis=1).reshape(-1)
    return np.ascontiguousarray(v, dtype=F32), np.stack([a, b], axis=1), f


def lattice(nx, ny, nz, spacing):
    """A regular lattice whose spacing is a float32 value: axis neighbours lie at d2 == float32(spacing)^2 exactly when the
    coordinates are small multiples of a dyadic spacing."""
    x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    return (np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(F32) * F32(spacing)).astype(F32)


def uniform_cube(n, seed, lo=0.0, hi=1.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, size=(n, 3)).astype(F32)


def duplicates(n=300):
    """n exact copies of one point, and two points apart from them."""
    return np.concatenate([np.tile(np.array([[0.3, -0.2, 1.7]], dtype=F32), (n, 1)), np.array([[0.31, -0.2, 1.7], [5, 5, 5]], dtype=F32)])


def crowded_cell(seed=3, n_dense=700, n_sparse=200):
    """One grid cell's worth of space (a cube of edge 0.02 with radius 0.1) holding 700 points, beside sparse points around it."""
    rng = np.random.default_rng(seed)
    dense = rng.uniform(0.0, 0.02, size=(n_dense, 3)) + np.array([0.41, 0.41, 0.41])
    sparse = rng.uniform(0.0, 1.0, size=(n_sparse, 3))
    p = np.concatenate([dense, sparse]).astype(F32)
    return p[rng.permutation(len(p))]


def straddling(seed=4, n=600):
    """Points around the origin and around multiples of the cell edge (radius 0.1: 105 fixed-point units of 2^-10), on both sides."""
    rng = np.random.default_rng(seed)
    centres = np.array([[0, 0, 0], [105 / 1024.0, 0, 0], [0, -105 / 1024.0, 210 / 1024.0], [-0.05, 0.05, -0.05]])
    p = centres[rng.integers(len(centres), size=n)] + rng.uniform(-0.06, 0.06, size=(n, 3))
    return p.astype(F32)


def near_limit(seed=5, n=400):
    """Clusters next to +2^14 and -2^14, where the float32 spacing is 2^-10 (one fixed-point unit), with points on and beyond the limit."""
    rng = np.random.default_rng(seed)
    steps = rng.integers(1, 200, size=(n, 3)).astype(np.float64) / 1024.0
    sign = np.where(rng.random((n, 1)) < 0.5, -1.0, 1.0)
    p = (sign * (16384.0 - steps)).astype(F32)
    p[0] = (16384.0, 0.0, 0.0)                                                        # not valid: |c| < 2^14 is strict
    p[1] = (-16384.0, 1.0, 1.0)
    p[2] = (16383.999, 16383.999, 16383.999)
    p[3] = (-16383.999, -16383.999, -16383.999)
    return p


def with_bad_rows(seed=6, n=500):
    """A cube of points some of whose rows hold a NaN, an infinity or 3e38."""
    p = uniform_cube(n, seed, 0.0, 0.5)
    p[7] = np.nan
    p[40, 2] = np.inf
    p[77] = (-np.inf, np.inf, 3.0e38)
    p[100] = 3.0e38
    p[101, 0] = -3.0e38
    p[n - 1, 1] = np.nan
    return p


def planes(seed=7, n_planes=6, per_plane=80):
    """Points exactly representable on planes in general position are rare; these are float32 roundings of points of random planes,
    each plane a patch of 0.3 x 0.3 -> (points, the unit normal float64 of every point's plane)."""
    rng = np.random.default_rng(seed)
    pts, nrm = [], []
    for i in range(n_planes):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        u = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
        u /= np.linalg.norm(u)
        w = np.cross(n, u)
        c = rng.uniform(-1.0, 1.0, size=3) + 3.0 * i
        st = rng.uniform(-0.15, 0.15, size=(per_plane, 2))
        pts.append(c + st[:, :1] * u + st[:, 1:] * w)
        nrm.append(np.tile(n, (per_plane, 1)))
    return np.concatenate(pts).astype(F32), np.concatenate(nrm)


def exact_planes():
    """Dyadic points on the planes z = 0, x = 1/4 and x + y = 1 (every coordinate a multiple of 1/64: float32 holds them exactly)
    -> (points, the unit normal of every point's plane, up to sign)."""
    g = np.arange(9) / 64.0
    a, b = np.meshgrid(g, g, indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    z0 = np.stack([a, b, np.zeros_like(a)], axis=1)
    x0 = np.stack([np.full_like(a, 0.25) + 4.0, a, b], axis=1)
    diag = np.stack([a + 8.0, 1.0 - a, b], axis=1)
    normals = np.concatenate([np.tile([0.0, 0.0, 1.0], (81, 1)), np.tile([1.0, 0.0, 0.0], (81, 1)),
                              np.tile([np.sqrt(0.5), np.sqrt(0.5), 0.0], (81, 1))])
    return np.concatenate([z0, x0, diag]).astype(F32), normals


def collinear(seed=8, n=60):
    """Points on one line (dyadic steps along (1, 2, -1) / 64), and a far tail of three points: neighbourhoods of rank 1, and rows with
    fewer than 3 neighbours."""
    t = np.arange(n)[:, None] / 64.0
    line = t * np.array([[1.0, 2.0, -1.0]])
    tail = np.array([[9.0, 9.0, 9.0], [9.05, 9.0, 9.0], [20.0, 0.0, 0.0]])
    return np.concatenate([line, tail]).astype(F32)
