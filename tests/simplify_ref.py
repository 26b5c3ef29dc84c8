"""The rule of segdino3d_amd/simplify.py restated in numpy: what csrc/simplify.hip is tested to EQUAL, bit for bit.  Every fp32 operation
is an explicit `np.float32` operation (numpy rounds each on its own, there is no fused multiply-add), every sum is an int64 sum, every
choice a minimum found by a stable sort.  Vectorised with `np.unique` / `np.lexsort`: 50 k vertices take well under a second."""
from collections import namedtuple

import numpy as np

INFO = ("vertices", "faces", "bad_vertices", "bad_faces", "collapsed", "duplicates", "unreferenced")
SimplifyRef = namedtuple("SimplifyRef", ("vertices", "faces", "vertex_map", "face_source", "info"))

F32 = np.float32
LIMIT = F32(16384.0)
OFFSET = np.int64(1 << 20)


def cell_keys(xyz, cell):
    """Step 2 for valid xyz fp32 [n, 3] -> int64 [n]."""
    inv_cell = F32(1.0 / float(cell))                                                   # float64, rounded once
    k = np.floor(xyz.astype(F32) * inv_cell).astype(np.int64) + OFFSET                  # one rounded fp32 multiply per axis
    return (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]


def simplify_ref(vertices, faces, cell=0.04, placement="mean", keep_unreferenced=True) -> SimplifyRef:
    vertices = np.ascontiguousarray(vertices, dtype=F32)
    faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
    V, C = vertices.shape
    F = faces.shape[0]
    assert 3 <= C <= 11 and placement in ("mean", "nearest")
    # 1. valid vertices
    with np.errstate(invalid="ignore"):
        ok = (np.abs(vertices) < LIMIT).all(axis=1) if V else np.zeros(0, bool)
    valid = np.nonzero(ok)[0]
    # 2. cells, numbered in ascending key
    keys = cell_keys(vertices[valid, :3], cell)
    ukeys, cell_of = np.unique(keys, return_inverse=True)
    cell_of = cell_of.reshape(-1)
    n_cells = ukeys.shape[0]
    vertex_map = np.full(V, -1, np.int64)
    vertex_map[valid] = cell_of
    # 3. integer sums
    q = np.rint(vertices[valid] * F32(65536.0)).astype(np.int64)                        # the product is exact
    S = np.zeros((n_cells, C), np.int64)
    np.add.at(S, cell_of, q)
    n = np.bincount(cell_of, minlength=n_cells).astype(np.int64)
    # 4. output vertices
    mean = (S.astype(np.float64) / (n.astype(np.float64) * 65536.0)[:, None]).astype(F32)
    if placement == "mean":
        cells = mean
    else:
        x = vertices[valid, :3]
        m = mean[cell_of, :3]
        dx, dy, dz = x[:, 0] - m[:, 0], x[:, 1] - m[:, 1], x[:, 2] - m[:, 2]
        d2 = ((dx * dx + dy * dy) + dz * dz).astype(F32)
        order = np.lexsort((valid, d2.view(np.uint32), cell_of))                        # cell, then bits of d2, then vertex index
        first = np.ones(order.shape[0], bool)
        first[1:] = cell_of[order[1:]] != cell_of[order[:-1]]
        cells = vertices[valid[order[first]]]                                           # the member's row, bit for bit
    # 5. faces
    f64 = faces.astype(np.int64)
    inside = ((f64 >= 0) & (f64 < V)).all(axis=1) if F else np.zeros(0, bool)
    mapped = np.full((F, 3), -1, np.int64)
    mapped[inside] = vertex_map[f64[inside]]
    bad = ~inside | (mapped < 0).any(axis=1)
    a, b, c = mapped[:, 0], mapped[:, 1], mapped[:, 2]
    collapsed = ~bad & ((a == b) | (b == c) | (a == c))
    live = np.nonzero(~bad & ~collapsed)[0]
    t = mapped[live]
    shift = np.argmin(t, axis=1)                                                        # the corners are distinct: one smallest
    rows = np.arange(t.shape[0])
    rot = np.stack([t[rows, shift], t[rows, (shift + 1) % 3], t[rows, (shift + 2) % 3]], axis=1) if t.shape[0] else t
    assert n_cells <= 1 << 21, "the oriented triple must pack into 63 bits"
    tkey = (rot[:, 0] << 42) | (rot[:, 1] << 21) | rot[:, 2]
    _, first_idx = np.unique(tkey, return_index=True)                                   # the first occurrence: the lowest original face
    kept = np.sort(first_idx)
    face_source = live[kept]
    out_faces = rot[kept]
    duplicates = live.shape[0] - kept.shape[0]
    # 6. unreferenced output vertices
    referenced = np.zeros(n_cells, bool)
    referenced[out_faces.reshape(-1)] = True
    unreferenced = int(n_cells - referenced.sum())
    if not keep_unreferenced:
        renumber = np.where(referenced, np.cumsum(referenced) - 1, -1)
        cells = cells[referenced]
        out_faces = renumber[out_faces]
        vertex_map[valid] = renumber[cell_of]
    info = dict(vertices=int(cells.shape[0]), faces=int(out_faces.shape[0]), bad_vertices=int(V - valid.shape[0]), bad_faces=int(bad.sum()),
                collapsed=int(collapsed.sum()), duplicates=int(duplicates), unreferenced=unreferenced)
    return SimplifyRef(np.ascontiguousarray(cells, dtype=F32).reshape(-1, C), out_faces.astype(np.int32).reshape(-1, 3),
                       vertex_map.astype(np.int32), face_source.astype(np.int32), info)
