"""Small meshes built by hand for the decimation tests (tests/test_simplify_ref.py, tests/test_gpu_simplify.py).  No file is read."""
import numpy as np

F32 = np.float32


def grid_faces(rows, cols, base=0, flip=False):
    """The 2 (rows - 1)(cols - 1) triangles of a rows x cols vertex grid numbered row-major from `base`; each quad is cut on the diagonal
    from its corner (i, j) to (i + 1, j + 1).  With the grid's rows along +u and columns along +v the right-hand normal is u x v; `flip`
    turns it round."""
    i, j = np.meshgrid(np.arange(rows - 1), np.arange(cols - 1), indexing="ij")
    p00 = (base + i * cols + j).reshape(-1)
    p01, p10, p11 = p00 + 1, p00 + cols, p00 + cols + 1
    f = np.concatenate([np.stack([p00, p10, p11], axis=1), np.stack([p00, p11, p01], axis=1)])
    if flip:
        f = f[:, [0, 2, 1]]
    return f.astype(np.int32)


def plane(m, spacing, origin=(0.0, 0.0, 0.0), channels=3, seed=0):
    """An m x m grid plane in z = origin_z: vertex (i, j) at origin + (i, j, 0) spacing (exact when `spacing` is a power of two), normal
    +z.  Channels past xyz are random 0 .. 255.  -> (vertices fp32 [m m, channels], faces int32 [2 (m - 1)^2, 3])."""
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    xyz = np.stack([origin[0] + i.reshape(-1) * spacing, origin[1] + j.reshape(-1) * spacing, np.full(m * m, origin[2])], axis=1)
    v = np.zeros((m * m, channels), F32)
    v[:, :3] = xyz.astype(F32)
    if channels > 3:
        v[:, 3:] = np.random.default_rng(seed).uniform(0, 255, (m * m, channels - 3)).astype(F32)
    return v, grid_faces(m, m)


def box(m, spacing, origin=(0.0, 0.0, 0.0)):
    """The closed surface of a cube of (m - 1) spacing a side: six m x m grids with their shared border vertices welded, every normal
    outwards.  -> (vertices fp32 [n, 3], faces int32 [12 (m - 1)^2, 3])."""
    L = m - 1
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    i, j = i.reshape(-1), j.reshape(-1)
    z, full = np.zeros_like(i), np.full_like(i, L)
    sides = [  # (lattice coordinates of grid vertex (i, j), whether u x v points inwards)
        (np.stack([i, j, z], 1), True), (np.stack([i, j, full], 1), False),             # z = 0 (normal -z), z = L (+z)
        (np.stack([z, i, j], 1), True), (np.stack([full, i, j], 1), False),             # x = 0, x = L: u = y, v = z, u x v = +x
        (np.stack([j, z, i], 1), True), (np.stack([j, full, i], 1), False),             # y = 0, y = L: u = z, v = x, u x v = +y
    ]
    lattice = np.concatenate([s for s, _ in sides])
    code = (lattice[:, 0] * m + lattice[:, 1]) * m + lattice[:, 2]
    ucode, weld = np.unique(code, return_inverse=True)
    weld = weld.reshape(-1)
    faces = np.concatenate([weld[grid_faces(m, m, base=k * m * m, flip=inwards)] for k, (_, inwards) in enumerate(sides)])
    lat = np.stack([ucode // (m * m), (ucode // m) % m, ucode % m], axis=1)
    vertices = (np.asarray(origin)[None] + lat * spacing).astype(F32)
    return vertices, faces.astype(np.int32)


def sheets(m, spacing, gap, origin=(0.0, 0.0, 0.0)):
    """Two parallel m x m sheets `gap` apart, the lower with normal -z and the upper with normal +z: the two sides of a thin wall.  With
    `gap` < cell and both in one layer of cells they cluster onto the same output vertices, and every surviving triple appears in both
    windings.  -> (vertices fp32 [2 m m, 3], faces int32 [4 (m - 1)^2, 3])."""
    lo, f = plane(m, spacing, origin)
    hi = lo.copy()
    hi[:, 2] += F32(gap)
    return np.concatenate([lo, hi]), np.concatenate([f[:, [0, 2, 1]], f + m * m]).astype(np.int32)


def relabel(vertices, faces, seed):
    """A random permutation of the vertices with the faces relabelled, and a permutation of the faces: the same mesh as a set.
    -> (vertices, faces, perm) with vertices_new[k] = vertices[perm[k]]."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(vertices))
    inverse = np.empty_like(perm)
    inverse[perm] = np.arange(len(perm))
    return np.ascontiguousarray(vertices[perm]), inverse[faces][rng.permutation(len(faces))].astype(np.int32), perm
