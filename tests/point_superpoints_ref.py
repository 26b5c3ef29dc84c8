"""The point-cloud rules of include/segdino3d_hip.h restated in numpy: the exact k-NN graph by brute force, normals from int64 moments
and a float64 Jacobi iteration written one operation per line, and the segmentation of a general edge list, which reuses the sweep
and the labelling of tests/superpoints_ref.py.  No torch, no device code.  float32 arrays keep one rounding per operation, and so do
float64 ones.  The kernels of csrc/superpoints.hip must EQUAL these functions bit for bit."""
from types import SimpleNamespace

import numpy as np

import superpoints_ref as R

F32 = np.float32
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
Q_SCALE = F32(2.0 ** 20)
MAX_OFFSET = F32(8.0)
JACOBI_SWEEPS = 8


def valid_points(points):
    """A point is valid iff its three coordinates are finite and below 2^14 in magnitude."""
    p = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.all(np.abs(p) < F32(16384.0), axis=1)                # a NaN or an infinity compares false


# ---------------------------------------------------------------------------------------------- rule a: the k-NN graph
def knn_keys(points, rows, radius, valid=None):
    """The keys (bits of d2 << 32) | j of the candidates of the points `rows` against every point -> uint64 [len(rows), N], NO_KEY
    where j is no candidate."""
    p = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    valid = valid_points(p) if valid is None else valid
    r = F32(radius)
    r2 = F32(r * r)
    rows = np.asarray(rows, dtype=np.int64)
    with np.errstate(all="ignore"):
        dx = p[None, :, 0] - p[rows, None, 0]
        dy = p[None, :, 1] - p[rows, None, 1]
        dz = p[None, :, 2] - p[rows, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        cand = (d2 <= r2) & valid[None, :] & valid[rows, None] & (np.arange(len(p))[None, :] != rows[:, None])
    keys = (np.ascontiguousarray(d2, dtype=F32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(p), dtype=np.uint64)[None, :]
    return np.where(cand, keys, NO_KEY)


def knn_graph(points, k=16, radius=0.1, chunk=256, reverse_ties=False):
    """-> (nbr int32 [N, k], d2 float32 [N, k]): per row the k smallest keys, ascending; -1 and +inf in the missing slots.
    `reverse_ties` prefers the HIGHER index among equal distances (not the rule: it exists so that a test can show that the tie order
    matters)."""
    p = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    n = len(p)
    nbr = np.full((n, k), -1, dtype=np.int32)
    d2 = np.full((n, k), np.inf, dtype=F32)
    valid = valid_points(p)
    for start in range(0, n, chunk):
        rows = np.arange(start, min(n, start + chunk))
        keys = knn_keys(p, rows, radius, valid)
        if reverse_ties:
            low = keys & np.uint64(0xFFFFFFFF)
            keys = np.where(keys == NO_KEY, NO_KEY, (keys - low) | (np.uint64(0xFFFFFFFE) - low))
        keys = np.sort(keys, axis=1)[:, :k]
        have = keys != NO_KEY
        low = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        if reverse_ties:
            low = 0xFFFFFFFE - low
        m = keys.shape[1]
        nbr[rows, :m] = np.where(have, low, -1).astype(np.int32)
        d2[rows, :m] = np.where(have, (keys >> np.uint64(32)).astype(np.uint32).view(F32), F32(np.inf))
    return nbr, d2


# ---------------------------------------------------------------------------------------------- rule b: normals
def moments(points, nbr):
    """-> (C float64 [N, 6] = the entries 00, 01, 02, 11, 12, 22 of n Sqq - Sq Sq^T, each one rounding of an exact int64; c int64 [N]
    = the slots of each row that count)."""
    p = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    nb = np.asarray(nbr).astype(np.int64).reshape(len(p), -1)
    ok = (nb >= 0) & (nb < len(p))
    j = np.where(ok, nb, 0)
    with np.errstate(all="ignore"):
        d = p[j] - p[:, None, :]                                                      # float32 [N, k, 3]
        ok = ok & np.all(np.abs(d) <= MAX_OFFSET, axis=2)                             # a NaN compares false
        d = np.where(ok[:, :, None], d, F32(0))
        q = np.rint(d * Q_SCALE).astype(np.int64)
    c = ok.sum(axis=1).astype(np.int64)
    n = c + 1                                                                         # the point itself: q = 0
    sq = q.sum(axis=1)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    cov = np.stack([n * (q[:, :, a] * q[:, :, b]).sum(axis=1) - sq[:, a] * sq[:, b] for a, b in pairs], axis=1)
    return cov.astype(np.float64), c


def _rotate(a, v, p, q):
    """One Jacobi rotation in the plane (p, q) of the symmetric a (dict (i, j) -> float64 [N], i <= j) and of the columns p, q of v
    (dict (i, j) -> float64 [N]), skipped where a_pq == 0.  THE definition of the update: one operation per line."""
    r = 3 - p - q
    sym = lambda i, j: (i, j) if i <= j else (j, i)
    apq = a[(p, q)]
    go = apq != 0.0
    with np.errstate(all="ignore"):
        diff = a[(q, q)] - a[(p, p)]
        two = 2.0 * apq
        theta = diff / two
        th2 = theta * theta
        rad = np.sqrt(th2 + 1.0)
        den = np.abs(theta) + rad
        t = 1.0 / den
        t = np.where(theta < 0.0, -t, t)
        t2 = t * t
        c = 1.0 / np.sqrt(t2 + 1.0)
        s = t * c
        tap = t * apq
        app = a[(p, p)] - tap
        aqq = a[(q, q)] + tap
        arp, arq = a[sym(r, p)], a[sym(r, q)]
        c_arp = c * arp
        s_arq = s * arq
        s_arp = s * arp
        c_arq = c * arq
        new_rp = c_arp - s_arq
        new_rq = s_arp + c_arq
        a[(p, p)] = np.where(go, app, a[(p, p)])
        a[(q, q)] = np.where(go, aqq, a[(q, q)])
        a[(p, q)] = np.where(go, 0.0, apq)
        a[sym(r, p)] = np.where(go, new_rp, arp)
        a[sym(r, q)] = np.where(go, new_rq, arq)
        for i in range(3):
            vip, viq = v[(i, p)], v[(i, q)]
            c_vip = c * vip
            s_viq = s * viq
            s_vip = s * vip
            c_viq = c * viq
            v[(i, p)] = np.where(go, c_vip - s_viq, vip)
            v[(i, q)] = np.where(go, s_vip + c_viq, viq)


def jacobi(cov, sweeps=JACOBI_SWEEPS):
    """cov float64 [N, 6] -> (diag float64 [N, 3], V float64 [N, 3, 3] whose column i belongs to diag[:, i])."""
    cov = np.asarray(cov, dtype=np.float64).reshape(-1, 6)
    n = len(cov)
    a = {(0, 0): cov[:, 0].copy(), (0, 1): cov[:, 1].copy(), (0, 2): cov[:, 2].copy(), (1, 1): cov[:, 3].copy(), (1, 2): cov[:, 4].copy(),
         (2, 2): cov[:, 5].copy()}
    v = {(i, j): np.full(n, 1.0 if i == j else 0.0) for i in range(3) for j in range(3)}
    for _ in range(sweeps):
        _rotate(a, v, 0, 1)
        _rotate(a, v, 0, 2)
        _rotate(a, v, 1, 2)
    diag = np.stack([a[(0, 0)], a[(1, 1)], a[(2, 2)]], axis=1)
    vec = np.stack([np.stack([v[(i, j)] for j in range(3)], axis=1) for i in range(3)], axis=1)
    return diag, vec


def smallest_column(diag, vec):
    """The column of V at the smallest diagonal entry, ties to the lowest index -> float64 [N, 3]."""
    c1 = diag[:, 1] < diag[:, 0]
    d01 = np.where(c1, diag[:, 1], diag[:, 0])
    c2 = diag[:, 2] < d01
    col = np.where(c2, 2, np.where(c1, 1, 0))
    return vec[np.arange(len(diag)), :, col]


def estimate_normals(points, nbr, viewpoint=None):
    """-> float32 [N, 3].  `viewpoint` float32 [3] or [N, 3]: the normal faces it; None: its first non-zero component is positive."""
    p = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    if len(p) == 0:
        return np.zeros((0, 3), dtype=F32)
    cov, c = moments(p, nbr)
    m = smallest_column(*jacobi(cov)).astype(F32)
    x, y, z, good = R._normalise(m[:, 0], m[:, 1], m[:, 2])
    out = np.stack([x, y, z], axis=1).astype(F32)
    out[~good] = 0
    with np.errstate(all="ignore"):
        if viewpoint is not None:
            v = np.broadcast_to(np.asarray(viewpoint, dtype=F32).reshape(-1, 3), p.shape)
            side = (out[:, 0] * (v[:, 0] - p[:, 0]) + out[:, 1] * (v[:, 1] - p[:, 1])) + out[:, 2] * (v[:, 2] - p[:, 2])
            flip = side < 0
        else:
            flip = (out[:, 0] < 0) | ((out[:, 0] == 0) & ((out[:, 1] < 0) | ((out[:, 1] == 0) & (out[:, 2] < 0))))
    out = np.where(flip[:, None], -out, out)
    out[c < 3] = 0
    return out


# ---------------------------------------------------------------------------------------------- rule c: a general edge list
def graph_edge_weights(points, normals, a, b, oriented=True):
    """Step 3 on the given normals -> (w float32 [E], live bool [E]); an edge with an end outside [0, N) has w = 0, live = False."""
    p = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    m = np.ascontiguousarray(normals, dtype=F32).reshape(-1, 3)
    live = (a >= 0) & (a < len(p)) & (b >= 0) & (b < len(p))
    w = np.zeros(len(a), dtype=F32)
    if live.any():
        a_, b_ = a[live], b[live]
        with np.errstate(all="ignore"):
            ma, mb = m[a_], m[b_]
            dot = (ma[:, 0] * mb[:, 0] + ma[:, 1] * mb[:, 1]) + ma[:, 2] * mb[:, 2]
            if not oriented:
                dot = np.abs(dot)
            t = F32(1) - dot
            wl = np.where(t > 0, t, F32(0)).astype(F32)
            if oriented:
                d = p[b_] - p[a_]
                s = (mb[:, 0] * d[:, 0] + mb[:, 1] * d[:, 1]) + mb[:, 2] * d[:, 2]
                wl = np.where(s > 0, wl * wl, wl).astype(F32)
        w[live] = wl
    return w, live


def graph_superpoints(points, normals, edges, oriented=True, k_thresh=0.01, min_verts=20, reverse_ties=False, debug=False):
    """points, normals float32 [N, 3], edges int [E, 2] -> SimpleNamespace(labels int64 [N], count, bad_edges[, weights, order])."""
    p = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    e = np.asarray(edges).astype(np.int64).reshape(-1, 2)
    a, b = e[:, 0].copy(), e[:, 1].copy()
    w, live = graph_edge_weights(p, normals, a, b, oriented)
    order = R.edge_order(w, reverse_ties)
    roots = R.sweep(len(p), a, b, w, live, order, float(F32(k_thresh)), int(min_verts))
    labels, count = R.labels_from_roots(roots)
    out = SimpleNamespace(labels=labels, count=count, bad_edges=int((~live).sum()))
    if debug:
        out.weights, out.order = w.view(np.uint32).copy(), order
    return out


def knn_edges(nbr):
    """Edge i k + s = (i, nbr[i, s]) -> int64 [N k, 2]."""
    n, k = nbr.shape
    return np.stack([np.repeat(np.arange(n, dtype=np.int64), k), nbr.reshape(-1).astype(np.int64)], axis=1)


def point_superpoints(points, k=16, radius=0.1, normals=None, viewpoint=None, k_thresh=0.01, min_verts=20, debug=False):
    """The composition; oriented iff `normals` or `viewpoint` is given -> as graph_superpoints, with nbr, d2 and normals under `debug`."""
    p = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    nbr, d2 = knn_graph(p, k, radius)
    oriented = normals is not None or viewpoint is not None
    if normals is None:
        normals = estimate_normals(p, nbr, viewpoint)
    out = graph_superpoints(p, normals, knn_edges(nbr), oriented, k_thresh, min_verts, debug=debug)
    if debug:
        out.nbr, out.d2, out.normals = nbr, d2, np.ascontiguousarray(normals, dtype=F32)
    return out
