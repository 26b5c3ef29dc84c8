"""The rule of segdino3d_amd/tsdf.py (include/segdino3d_hip.h, "TSDF fusion ...") restated in numpy: what csrc/tsdf.hip is tested
against, bit for bit, since the reference ships no code that makes a mesh.  The steps carry the numbers of the module's docstring.
Every float operation is a single float32 numpy operation in the stated order; the per-voxel state is integer sums.

A volume is a `Volume`: block keys uint64 [B] ascending and unique, W, T int64 [B, 512], C int64 [B, 512, 3] (voxel (lx, ly, lz) of a
block at lx * 64 + ly * 8 + lz) and the counters `updates` and `out_of_range`.  `merge` adds two of them."""
from collections import namedtuple

import numpy as np

import fuse_views_ref as FR

F32 = np.float32
WORLD_BITS, CELL_BITS, BLOCK_BITS = 14, 20, 17
RULE_DEFAULTS = dict(voxel=0.02, trunc=0.08, near=0.1, far=6.0, edge_abs=0.02, edge_rel=0.02, min_weight=2)

Volume = namedtuple("Volume", "keys W T C updates out_of_range")
Mesh = namedtuple("Mesh", "vertices faces keys blocks voxels_observed updates out_of_range")

_L = np.arange(512)
LOCAL = np.stack([_L >> 6, (_L >> 3) & 7, _L & 7], axis=1)                            # [512, 3]


def rule(**kw):
    bad = set(kw) - set(RULE_DEFAULTS)
    assert not bad, bad
    return {**RULE_DEFAULTS, **kw}


def constants(r):
    """The host constants: each made in float64 and rounded once."""
    return dict(voxel=F32(r["voxel"]), inv_voxel=F32(1.0 / float(r["voxel"])), trunc=F32(r["trunc"]), h=F32(float(r["trunc"]) / 2.0),
                qscale=F32(4096.0 / float(r["trunc"])))


def world_to_cam(poses):
    """float64 [V, 4, 4] -> (fp32 [K, 3, 4], kept): as lift2d.Views makes it."""
    poses = np.asarray(poses, dtype=np.float64)
    kept = np.flatnonzero(np.isfinite(poses).all(axis=(1, 2)))
    inv = np.linalg.inv(poses[kept]) if len(kept) else np.zeros((0, 4, 4))
    return np.ascontiguousarray(inv[:, :3, :].astype(np.float32)), kept


def block_keys(b):
    b = (b.astype(np.int64) + (1 << BLOCK_BITS)).astype(np.uint64)
    return (b[:, 0] << np.uint64(36)) | (b[:, 1] << np.uint64(18)) | b[:, 2]


def block_coords(keys):
    k = np.asarray(keys, dtype=np.uint64)
    m = np.uint64(0x3FFFF)
    return np.stack([(k >> np.uint64(36)) & m, (k >> np.uint64(18)) & m, k & m], axis=1).astype(np.int64) - (1 << BLOCK_BITS)


def cell_keys(c):
    c = (c.astype(np.int64) + (1 << CELL_BITS)).astype(np.uint64)
    return (c[:, 0] << np.uint64(42)) | (c[:, 1] << np.uint64(21)) | c[:, 2]


def touched_blocks(d, ok, intr, c2w, k):
    """Step 2 for one view: d fp32 [Hd, Wd], ok bool -> (block keys uint64, unique and ascending; out_of_range)."""
    vi, ui = np.nonzero(ok)
    fx, fy, cx, cy = (F32(x) for x in intr)
    R = c2w.astype(F32)
    keys, out = [], 0
    with np.errstate(all="ignore"):
        for j in range(-2, 3):
            dj = d[vi, ui] + F32(j) * k["h"]
            x = (ui.astype(F32) - cx) * dj / fx
            y = (vi.astype(F32) - cy) * dj / fy
            w = np.stack([((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * dj) + R[i, 3] for i in range(3)], axis=1)
            fine = (np.abs(w) < F32(2 ** WORLD_BITS)).all(axis=1)                       # a NaN fails
            c = np.floor(w * k["inv_voxel"])
            fine &= ((c >= F32(-2 ** CELL_BITS)) & (c < F32(2 ** CELL_BITS))).all(axis=1)
            out += int((~fine).sum())
            keys.append(block_keys(c[fine].astype(np.int64) >> 3))
    return np.unique(np.concatenate(keys)), out


def integrate_view(keys, d, ok, intr, w2c, colors, k):
    """Step 3 for one view and the blocks it touched -> (W, T int64 [B, 512], C int64 [B, 512, 3])."""
    Hd, Wd = d.shape
    Hc, Wc = colors.shape[:2]
    B = len(keys)
    c = (block_coords(keys)[:, None, :] * 8 + LOCAL[None]).reshape(-1, 3)
    p = (c.astype(F32) + F32(0.5)) * k["voxel"]
    fx, fy, cx, cy = (F32(x) for x in intr)
    m = w2c.astype(F32)
    W, T, C = np.zeros(B * 512, np.int64), np.zeros(B * 512, np.int64), np.zeros((B * 512, 3), np.int64)
    with np.errstate(all="ignore"):
        x, y, z = (((m[i, 0] * p[:, 0] + m[i, 1] * p[:, 1]) + m[i, 2] * p[:, 2]) + m[i, 3] for i in range(3))
        uf = np.floor(((fx * x) / z + cx) + F32(0.5))
        vf = np.floor(((fy * y) / z + cy) + F32(0.5))
        take = (z > 0) & (uf >= 0) & (uf < F32(Wd)) & (vf >= 0) & (vf < F32(Hd))
    idx = np.flatnonzero(take)
    ui, vi = uf[idx].astype(np.int64), vf[idx].astype(np.int64)
    valid = ok[vi, ui]
    idx, ui, vi = idx[valid], ui[valid], vi[valid]
    sdf = d[vi, ui] - z[idx]
    keep = ~(sdf < -k["trunc"])
    idx, ui, vi, sdf = idx[keep], ui[keep], vi[keep], sdf[keep]
    q = np.rint(np.minimum(sdf, k["trunc"]) * k["qscale"]).astype(np.int64)
    W[idx] = 1
    T[idx] = q
    C[idx] = colors[((2 * vi + 1) * Hc) // (2 * Hd), ((2 * ui + 1) * Wc) // (2 * Wd)]
    return W.reshape(B, 512), T.reshape(B, 512), C.reshape(B, 512, 3)


def _reduce(keys, W, T, C):
    uk, inv = np.unique(keys, return_inverse=True)
    W2, T2, C2 = np.zeros((len(uk), 512), np.int64), np.zeros((len(uk), 512), np.int64), np.zeros((len(uk), 512, 3), np.int64)
    np.add.at(W2, inv, W)
    np.add.at(T2, inv, T)
    np.add.at(C2, inv, C)
    return uk, W2, T2, C2


def empty():
    return Volume(np.zeros(0, np.uint64), np.zeros((0, 512), np.int64), np.zeros((0, 512), np.int64), np.zeros((0, 512, 3), np.int64), 0, 0)


def integrate_kept(depth, depth_scale, intr, c2w, w2c, colors, **kw):
    """Steps 1 to 3 for kept views -> Volume."""
    r = rule(**kw)
    k = constants(r)
    parts, updates, out = [empty()], 0, 0
    for v in range(depth.shape[0]):
        d = FR.depth_metres(depth[v], depth_scale)
        ok = FR.valid_pixels(d, r["near"], r["far"], r["edge_abs"], r["edge_rel"])
        keys, o = touched_blocks(d, ok, intr[v], c2w[v], k)
        out += o
        W, T, C = integrate_view(keys, d, ok, intr[v], w2c[v], colors[v], k)
        updates += int(W.sum())
        parts.append(Volume(keys, W, T, C, 0, 0))
    cat = lambda f: np.concatenate([getattr(p, f) for p in parts])                    # noqa: E731
    return Volume(*_reduce(cat("keys"), cat("W"), cat("T"), cat("C")), updates, out)


def integrate(depth, depth_scale, intr, poses, colors, **kw):
    """Steps 1 to 3 for GIVEN views (float64 poses [V, 4, 4]; colours per given view)."""
    c2w, kept = FR.cam_to_world(poses)
    w2c, _ = world_to_cam(poses)
    return integrate_kept(depth[kept], depth_scale, intr[kept], c2w, w2c, colors[kept], **kw)


def merge(a, b):
    """The volume after both `a` and `b`: integer sums, so the order and the cut cannot matter."""
    cat = lambda f: np.concatenate([getattr(a, f), getattr(b, f)])                    # noqa: E731
    return Volume(*_reduce(cat("keys"), cat("W"), cat("T"), cat("C")), a.updates + b.updates, a.out_of_range + b.out_of_range)


# the 12 edges of a cell as (axis, corner a, corner b), corners as (dx, dy, dz): x-edges, y-edges, z-edges; within an axis the two
# remaining coordinates ascending, the earlier axis the major one
EDGES = []
for _axis in range(3):
    _u, _w = [i for i in range(3) if i != _axis]
    for _cu in (0, 1):
        for _cw in (0, 1):
            _a = [0, 0, 0]
            _a[_u], _a[_w] = _cu, _cw
            _b = list(_a)
            _b[_axis] = 1
            EDGES.append((_axis, tuple(_a), tuple(_b)))


def extract(vol, **kw):
    """Steps 4 to 6 -> Mesh."""
    r = rule(**kw)
    k = constants(r)
    B = len(vol.keys)
    coords = (block_coords(vol.keys)[:, None, :] * 8 + LOCAL[None]).reshape(-1, 3)   # ascending voxel key: blocks ascending, local ascending
    vkeys = cell_keys(coords)
    order = np.argsort(vkeys, kind="stable")
    skeys = vkeys[order]
    W, T, C = vol.W.reshape(-1), vol.T.reshape(-1), vol.C.reshape(-1, 3)
    observed = W >= r["min_weight"]

    def find(c):
        """voxel coordinates int64 [N, 3] -> the row of each in `coords`, -1 for a voxel of no block."""
        if len(skeys) == 0:
            return np.full(len(c), -1, np.int64)
        inr = ((c >= -(1 << CELL_BITS)) & (c < (1 << CELL_BITS))).all(axis=1)
        kq = cell_keys(np.where(inr[:, None], c, 0))
        pos = np.minimum(np.searchsorted(skeys, kq), len(skeys) - 1)
        return np.where(inr & (skeys[pos] == kq), order[pos], -1)

    # ---- step 5: cells
    cand = np.flatnonzero(observed)                                                   # a cell's low corner is observed
    cc = coords[cand]
    corner = {}
    alive = np.ones(len(cand), dtype=bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                row = find(cc + np.array([dx, dy, dz]))
                corner[(dx, dy, dz)] = row
                alive &= (row >= 0) & observed[np.maximum(row, 0)]
    cand, cc = cand[alive], cc[alive]
    corner = {key: row[alive] for key, row in corner.items()}
    inside = np.stack([T[row] < 0 for row in corner.values()], axis=1)
    active = inside.any(axis=1) & ~inside.all(axis=1)
    cand, cc = cand[active], cc[active]
    corner = {key: row[active] for key, row in corner.items()}
    n = len(cand)
    f = {key: (T[row].astype(np.float64) / W[row].astype(np.float64)).astype(F32) for key, row in corner.items()}
    s = np.zeros((n, 3), F32)
    cnt = np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for axis, a, b in EDGES:
            cross = (T[corner[a]] < 0) != (T[corner[b]] < 0)
            pos = np.zeros((n, 3), F32)
            pos[:, :] = np.array(a, F32)
            pos[:, axis] = f[a] / (f[a] - f[b])
            s[cross] = s[cross] + pos[cross]
            cnt += cross
        m = s / cnt.astype(F32)[:, None]
        xyz = (cc.astype(F32) + (F32(0.5) + m)) * k["voxel"]
    sw = sum(W[row] for row in corner.values())
    sc = sum(C[row] for row in corner.values())
    rgb = (sc.astype(np.float64) / sw.astype(np.float64)[:, None]).astype(F32)
    ckeys = cell_keys(cc)
    o = np.argsort(ckeys, kind="stable")
    cand, cc, ckeys = cand[o], cc[o], ckeys[o]
    vertices = np.concatenate([xyz[o], rgb[o]], axis=1).astype(F32).reshape(-1, 6)
    vindex = np.full(len(coords), -1, np.int64)                                       # voxel row -> the vertex of the cell that begins there
    vindex[cand] = np.arange(n)

    def cell_vertex(c):
        row = find(c)
        return np.where(row >= 0, vindex[np.maximum(row, 0)], -1)

    # ---- step 6: faces, in ascending (vertex of a, axis)
    quads = []
    a_in = T[cand] < 0
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        e, eu, ew = (np.eye(3, dtype=np.int64)[i] for i in (axis, u, w))
        rb = find(cc + e)
        ok = (rb >= 0) & observed[np.maximum(rb, 0)] & ((T[np.maximum(rb, 0)] < 0) != a_in)
        q0, q1, q3 = cell_vertex(cc - eu - ew), cell_vertex(cc - ew), cell_vertex(cc - eu)
        ok &= (q0 >= 0) & (q1 >= 0) & (q3 >= 0)
        j = np.flatnonzero(ok)
        q0, q1, q2, q3 = q0[j], q1[j], j, q3[j]
        fwd = np.stack([q0, q1, q2, q0, q2, q3], axis=1)
        rev = np.stack([q0, q2, q1, q0, q3, q2], axis=1)
        quads.append((j * 3 + axis, np.where(a_in[j][:, None], fwd, rev)))
    rank = np.concatenate([q[0] for q in quads])
    tri = np.concatenate([q[1] for q in quads]).reshape(-1, 6)
    faces = tri[np.argsort(rank, kind="stable")].reshape(-1, 3).astype(np.int32)
    return Mesh(vertices, faces, ckeys, B, int(observed.sum()), vol.updates, vol.out_of_range)


def tsdf_mesh(depth, depth_scale, intr, poses, colors, **kw):
    """The whole rule for one batch of GIVEN views -> (Volume, Mesh)."""
    vol = integrate(depth, depth_scale, intr, poses, colors, **kw)
    return vol, extract(vol, **kw)
