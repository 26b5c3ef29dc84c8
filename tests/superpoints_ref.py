"""The superpoint rule of include/segdino3d_hip.h restated in numpy: float32 with one rounding per operation, int64 sums, a plain
sequential union-find.  No torch, no device code.  The kernels of csrc/superpoints.hip must EQUAL `mesh_superpoints` label for label.

`sweep_batched` writes out the formulation the sweep kernel uses (batches of B edges, roots looked up as they stood when the batch
began, the surviving edges settled in order on a small table of start-roots); tests/test_superpoints_ref.py holds it equal to the
sequential `sweep`."""
from types import SimpleNamespace

import numpy as np

F32 = np.float32
SCALE = F32(2.0 ** 24)


def _normalise(x, y, z):
    """(x, y, z) / l with l = sqrt((x x + y y) + z z), each operation rounded to float32 -> (x, y, z, valid)."""
    with np.errstate(all="ignore"):
        l = np.sqrt((x * x + y * y) + z * z)
        ok = np.isfinite(l) & (l > 0)
        ls = np.where(ok, l, F32(1))
        return x / ls, y / ls, z / ls, ok


def valid_faces(n_vertices, faces):
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    return f, np.all((f >= 0) & (f < n_vertices), axis=1)


def vertex_normals(vertices, faces):
    """Steps 1 and 2 -> float32 [N, 3]."""
    v = np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    f, ok = valid_faces(len(v), faces)
    f = f[ok]
    sums = np.zeros((len(v), 3), dtype=np.int64)
    if len(f):
        with np.errstate(all="ignore"):
            p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
            a, b = p1 - p0, p2 - p0
            nx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
            ny = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
            nz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
            nx, ny, nz, good = _normalise(nx, ny, nz)
            q = np.stack([np.rint(nx[good] * SCALE), np.rint(ny[good] * SCALE), np.rint(nz[good] * SCALE)], axis=1).astype(np.int64)
        for k in range(3):
            np.add.at(sums, f[good, k], q)
    m = sums.astype(np.float64).astype(F32)
    x, y, z, good = _normalise(m[:, 0], m[:, 1], m[:, 2])
    out = np.stack([x, y, z], axis=1).astype(F32)
    out[~good] = 0
    return out


def edge_ends(faces):
    """Edge 3 f + k of face (i, j, k): (i, j), (i, k), (k, j) -> a, b int64 [3 F]."""
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    a = np.stack([f[:, 0], f[:, 0], f[:, 2]], axis=1).reshape(-1)
    b = np.stack([f[:, 1], f[:, 2], f[:, 1]], axis=1).reshape(-1)
    return a, b


def edge_weights(vertices, faces, normals):
    """Step 3 -> (w float32 [3 F], live bool [3 F]); the edges of an ignored face have w = 0 and live = False."""
    v = np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    f, ok = valid_faces(len(v), faces)
    a, b = edge_ends(f)
    live = np.repeat(ok, 3)
    w = np.zeros(len(a), dtype=F32)
    if live.any():
        a_, b_ = a[live], b[live]
        with np.errstate(all="ignore"):
            ma, mb = normals[a_], normals[b_]
            dot = (ma[:, 0] * mb[:, 0] + ma[:, 1] * mb[:, 1]) + ma[:, 2] * mb[:, 2]
            t = F32(1) - dot
            wl = np.where(t > 0, t, F32(0)).astype(F32)
            d = v[b_] - v[a_]
            s = (mb[:, 0] * d[:, 0] + mb[:, 1] * d[:, 1]) + mb[:, 2] * d[:, 2]
            wl = np.where(s > 0, wl * wl, wl).astype(F32)
        w[live] = wl
    return w, live


def edge_order(w, reverse_ties=False):
    """Step 4: ascending (bits of w, edge index); `reverse_ties` puts the HIGHER edge index first among equal weights (not the rule:
    it exists so that a test can show that the tie order matters)."""
    bits = np.ascontiguousarray(w, dtype=F32).view(np.uint32)
    if not reverse_ties:
        return np.argsort(bits, kind="stable")
    idx = np.arange(len(bits))
    return np.lexsort((-idx, bits))


def _thr_after(w, k_thresh, size):
    return float(F32(F32(w) + F32(F32(k_thresh) / F32(size))))


class _Forest:
    def __init__(self, n, k_thresh):
        self.parent = list(range(n))
        self.size = [1] * n
        self.thr = [float(F32(k_thresh))] * n

    def find(self, x):
        p = self.parent
        r = x
        while p[r] != r:
            r = p[r]
        while p[x] != r:
            p[x], x = r, p[x]
        return r


def _settle(forest_like, find, x, y, w, pass_, k_thresh, min_verts):
    """One edge between the components with representatives x != y -> the surviving representative, or -1 (refused)."""
    size, thr, parent = forest_like.size, forest_like.thr, forest_like.parent
    if pass_ == 0:
        if not (w <= thr[x] and w <= thr[y]):
            return -1
    elif not (size[x] < min_verts or size[y] < min_verts):
        return -1
    if size[x] < size[y]:
        x, y = y, x
    parent[y] = x
    size[x] += size[y]
    thr[x] = _thr_after(w, k_thresh, size[x])
    return x


def sweep(n, a, b, w, live, order, k_thresh, min_verts):
    """Steps 5 and 6, one edge at a time -> the root of every vertex (list)."""
    fr = _Forest(n, k_thresh)
    a, b, live = a.tolist(), b.tolist(), live.tolist()
    wf = [float(x) for x in w]
    order = order.tolist()
    for pass_ in (0, 1):
        for e in order:
            if not live[e]:
                continue
            x, y = fr.find(a[e]), fr.find(b[e])
            if x != y:
                _settle(fr, fr.find, x, y, wf[e], pass_, k_thresh, min_verts)
    return [fr.find(v) for v in range(n)]


def sweep_batched(n, a, b, w, live, order, k_thresh, min_verts, batch, stats=None):
    """The same two passes as the sweep kernel takes them: per batch of `batch` edges all roots are looked up in the forest as it stood
    when the batch began; edges inside one component are dropped (in pass 2 also those between two components that are large already:
    sizes only grow); the start-roots of the rest get slots in a table holding their size and thr; the rest is settled in order on a
    union-find over the slots; the table is written back.  Pass 2 walks only the edges that are candidates when it begins (ends in
    different components, one of them small): components only merge and only grow, so no other edge can join anything in it.
    `stats` (a list) receives the number of table-settled edges per pass."""
    fr = _Forest(n, k_thresh)
    a, b, live = a.tolist(), b.tolist(), live.tolist()
    wf = [float(x) for x in w]
    order = order.tolist()

    def small_and_apart(x, y):
        return x != y and (fr.size[x] < min_verts or fr.size[y] < min_verts)

    for pass_ in (0, 1):
        settled = 0
        if pass_ == 1:                                     # the candidates, found once when the pass begins, in order
            order = [e for e in order if live[e] and small_and_apart(fr.find(a[e]), fr.find(b[e]))]
        for start in range(0, len(order), batch):
            surv = []
            for e in order[start:start + batch]:
                if not live[e]:
                    continue
                x, y = fr.find(a[e]), fr.find(b[e])
                if x == y or (pass_ == 1 and not (fr.size[x] < min_verts or fr.size[y] < min_verts)):
                    continue
                surv.append((x, y, wf[e]))
            settled += len(surv)
            slot = {}
            for x, y, _ in surv:
                for r in (x, y):
                    if r not in slot:
                        slot[r] = len(slot)
            assert len(slot) <= 2 * batch
            keys = list(slot)
            tab = SimpleNamespace(parent=list(range(len(keys))), size=[fr.size[r] for r in keys], thr=[fr.thr[r] for r in keys])

            def tfind(i):
                while tab.parent[i] != i:
                    i = tab.parent[i]
                return i
            for x, y, we in surv:
                i, j = tfind(slot[x]), tfind(slot[y])
                if i != j:
                    _settle(tab, tfind, i, j, we, pass_, k_thresh, min_verts)
            for i, r in enumerate(keys):
                t = tfind(i)
                if t != i:
                    fr.parent[r] = keys[t]
                else:
                    fr.size[r], fr.thr[r] = tab.size[i], tab.thr[i]
        if stats is not None:
            stats.append(settled)
    return [fr.find(v) for v in range(n)]


def labels_from_roots(roots):
    """Step 7: dense labels, components numbered by ascending smallest vertex -> (labels int64 [N], S)."""
    roots = np.asarray(roots, dtype=np.int64)
    n = len(roots)
    if n == 0:
        return np.zeros(0, dtype=np.int64), 0
    minv = np.full(n, n, dtype=np.int64)
    np.minimum.at(minv, roots, np.arange(n))
    first = minv[roots]                                    # the smallest vertex of each vertex's component
    flag = first == np.arange(n)
    number = np.cumsum(flag) - flag
    return number[first].astype(np.int64), int(flag.sum())


def mesh_superpoints(vertices, faces, k_thresh=0.01, min_verts=20, reverse_ties=False, batch=None, debug=False):
    """vertices float32 [N, 3], faces int [F, 3] -> SimpleNamespace(labels int64 [N], count, bad_faces[, normals, weights, order])."""
    v = np.ascontiguousarray(vertices, dtype=F32).reshape(-1, 3)
    f, ok = valid_faces(len(v), faces)
    normals = vertex_normals(v, f)
    w, live = edge_weights(v, f, normals)
    order = edge_order(w, reverse_ties)
    a, b = edge_ends(f)
    if batch is None:
        roots = sweep(len(v), a, b, w, live, order, float(F32(k_thresh)), int(min_verts))
    else:
        roots = sweep_batched(len(v), a, b, w, live, order, float(F32(k_thresh)), int(min_verts), int(batch))
    labels, count = labels_from_roots(roots)
    out = SimpleNamespace(labels=labels, count=count, bad_faces=int((~ok).sum()))
    if debug:
        out.normals, out.weights, out.order = normals, w.view(np.uint32).copy(), order
    return out
