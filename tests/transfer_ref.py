"""The rule of segdino3d_amd/transfer.py (include/segdino3d_hip.h, "Nearest point") restated in numpy: what csrc/transfer.hip is
tested against, bit for bit, since the reference ships no code that carries a result from the points of a forward onto frames or
other clouds.  No torch, no device code, no grid: every query is compared with every source point.

  1-3. `nearest`: the smallest key (bits of d2 << 32) | j over the valid source points with d2 <= r2, built on the arithmetic of
       `point_superpoints_ref.knn_keys` (the same differences, products and sums, one fp32 rounding each) without the self-exclusion.
  4.   `pixel_queries`: the depth of `fuse_views_ref.depth_metres`, the range test of step 2 and the fp32 back-projection of step 4
       of tests/fuse_views_ref.py, for EVERY pixel (no stride, no edge test).
  5.   `take_labels`.
  6.   `instance_map`."""
import numpy as np

import fuse_views_ref as FR
import point_superpoints_ref as PR

F32 = np.float32
NO_KEY = PR.NO_KEY


def keys(ref, queries, radius):
    """uint64 [M, N]: the key of source point j for query m, NO_KEY where j is no candidate (steps 1 and 2)."""
    p = np.ascontiguousarray(ref, dtype=F32).reshape(-1, 3)
    q = np.ascontiguousarray(queries, dtype=F32).reshape(-1, 3)
    n, m = len(p), len(q)
    if n == 0 or m == 0:
        return np.full((m, n), NO_KEY, dtype=np.uint64)
    # knn_keys evaluates rows of ONE array against all of it: stack the queries behind the cloud and keep the columns of the cloud.
    # Its validity test is the rule's; its self-exclusion (column == row) cannot strike, because the rows lie behind the columns kept.
    both = np.concatenate([p, q])
    return PR.knn_keys(both, np.arange(n, n + m), radius, PR.valid_points(both))[:, :n]


def _best(k, reverse_ties):
    """uint64 [m, n] keys with ascending column = ascending index -> (column int64 [m] or -1, d2 float32 [m])."""
    low_mask = np.uint64(0xFFFFFFFF)
    if k.shape[1] == 0:
        return np.full(len(k), -1, dtype=np.int64), np.full(len(k), np.inf, dtype=F32)
    if reverse_ties:
        low = k & low_mask
        k = np.where(k == NO_KEY, NO_KEY, (k - low) | (np.uint64(0xFFFFFFFE) - low))
    best = k.min(axis=1)
    have = best != NO_KEY
    low = (best & low_mask).astype(np.int64)
    if reverse_ties:
        low = 0xFFFFFFFE - low
    return np.where(have, low, -1), np.where(have, (best >> np.uint64(32)).astype(np.uint32).view(F32), F32(np.inf))


def nearest(ref, queries, radius, chunk=512, reverse_ties=False, prefilter=True):
    """-> (idx int32 [M], d2 float32 [M]); -1 and +inf where a query is invalid or has no candidate.  `reverse_ties` prefers the HIGHER
    index among equal distances (not the rule: it exists so that a test can show that the tie order matters).

    `prefilter=False` compares every query with every source point.  `prefilter=True` gives the same answer in a fraction of the time,
    so that whole frames can be restated: the valid queries are grouped by the cube of side 8 r they lie in, and a group is compared
    with the valid source points inside the group's bounding box widened by 1.001 r on every side, in ascending index order.  A
    candidate has d2 <= r2, hence |dx| <= r (1 + 2^-22) on every axis (the argument above the kernels), so the box holds every
    candidate of every query of the group; the float64 comparisons that draw the box are exact.  The distances and the keys are
    `knn_keys`'s either way, and tests/test_transfer_ref.py holds the two forms against each other."""
    p = np.ascontiguousarray(ref, dtype=F32).reshape(-1, 3)
    q = np.ascontiguousarray(queries, dtype=F32).reshape(-1, 3)
    m = len(q)
    idx, d2 = np.full(m, -1, dtype=np.int32), np.full(m, np.inf, dtype=F32)
    if not prefilter:
        for start in range(0, m, chunk):
            idx[start:start + chunk], d2[start:start + chunk] = _best(keys(p, q[start:start + chunk], radius), reverse_ties)
        return idx, d2
    qv, pv = np.flatnonzero(PR.valid_points(q)), np.flatnonzero(PR.valid_points(p))
    if len(qv) == 0 or len(pv) == 0:
        return idx, d2
    r = float(F32(radius))
    p64, q64 = p[pv].astype(np.float64), q[qv].astype(np.float64)
    by_x = np.argsort(p64[:, 0], kind="stable")
    px = p64[by_x, 0]
    cube = np.floor(q64 / (8.0 * r)).astype(np.int64)
    order = np.lexsort((cube[:, 2], cube[:, 1], cube[:, 0]))
    cuts = np.flatnonzero(np.any(np.diff(cube[order], axis=0) != 0, axis=1)) + 1
    for grp in np.split(order, cuts):
        lo, hi = q64[grp].min(axis=0) - 1.001 * r, q64[grp].max(axis=0) + 1.001 * r
        slab = by_x[np.searchsorted(px, lo[0], "left"):np.searchsorted(px, hi[0], "right")]
        inside = np.all((p64[slab, 1:] >= lo[1:]) & (p64[slab, 1:] <= hi[1:]), axis=1)
        sel = pv[np.sort(slab[inside])]                                               # ascending index: ties resolve as in the whole cloud
        if len(sel) == 0:
            continue
        for start in range(0, len(grp), chunk):
            rows = qv[grp[start:start + chunk]]
            col, dist = _best(keys(p[sel], q[rows], radius), reverse_ties)
            idx[rows] = np.where(col >= 0, sel[np.maximum(col, 0)], -1).astype(np.int32)
            d2[rows] = dist
    return idx, d2


def nearest_f64(ref, queries, radius, chunk=512):
    """The same question asked in float64 (exact products of the fp32 inputs' differences, to far below the gaps between distances):
    the nearest valid source point with d2 <= r2, ties to the lower index -> idx int64 [M]."""
    p = np.asarray(ref, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    r2 = float(F32(F32(radius) * F32(radius)))
    out = np.full(len(q), -1, dtype=np.int64)
    for start in range(0, len(q), chunk):
        d = p[None, :, :] - q[start:start + chunk, None, :]
        d2 = (d * d).sum(axis=2)
        d2 = np.where(d2 <= r2, d2, np.inf)
        j = d2.argmin(axis=1)                                                         # the first of equal minima
        out[start:start + chunk] = np.where(np.isfinite(d2[np.arange(len(j)), j]), j, -1)
    return out


def pixel_queries(depth, depth_scale, intr, c2w, near=0.1, far=6.0):
    """Step 4 for kept views: depth uint16 / fp32 [V, Hd, Wd], intr fp32 [V, 4], c2w fp32 [V, 3, 4] -> (w float32 [V, Hd, Wd, 3], ok bool
    [V, Hd, Wd]): the query of every pixel and whether its depth is valid (w is NaN where it is not)."""
    V, Hd, Wd = depth.shape
    w = np.full((V, Hd, Wd, 3), np.nan, dtype=F32)
    ok = np.zeros((V, Hd, Wd), dtype=bool)
    vi, ui = np.meshgrid(np.arange(Hd), np.arange(Wd), indexing="ij")
    for v in range(V):
        d = FR.depth_metres(depth[v], depth_scale)
        ok[v] = FR.valid_pixels(d, near, far, None, None)                             # step 2 alone: no edge test
        fx, fy, cx, cy = (F32(x) for x in intr[v])
        R = c2w[v].astype(F32)
        with np.errstate(all="ignore"):                                               # step 4 of fuse_views_ref, float32, left to right
            x = (ui.astype(F32) - cx) * d / fx
            y = (vi.astype(F32) - cy) * d / fy
            wv = np.stack([((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * d) + R[i, 3] for i in range(3)], axis=-1).astype(F32)
        w[v][ok[v]] = wv[ok[v]]
    return w, ok


def nearest_pixels(ref, depth, depth_scale, intr, c2w, radius, near=0.1, far=6.0):
    """-> (idx int32 [V, Hd, Wd], d2 float32 [V, Hd, Wd])."""
    w, ok = pixel_queries(depth, depth_scale, intr, c2w, near, far)
    idx, d2 = np.full(ok.shape, -1, dtype=np.int32), np.full(ok.shape, np.inf, dtype=F32)
    idx[ok], d2[ok] = nearest(ref, w[ok], radius)
    return idx, d2


def take_labels(labels, idx, fill=-1):
    """Step 5: labels int [L, N] or [N], idx of any shape -> int32 [L, ...] or [...]."""
    lab = np.asarray(labels).astype(np.int64)
    idx = np.asarray(idx)
    safe = np.where(idx >= 0, idx, 0)
    if lab.shape[-1] == 0:
        return np.full(lab.shape[:-1] + idx.shape, fill, dtype=np.int32)
    return np.where(idx >= 0, lab[..., safe], fill).astype(np.int32)


def instance_map(masks, scores, score_thr=0.0):
    """Step 6: masks [I, N], scores float32 [I] -> int32 [N]; written as the loop it is."""
    m = np.asarray(masks) != 0
    s = np.asarray(scores, dtype=F32)
    out = np.full(m.shape[1], -1, dtype=np.int32)
    top = np.zeros(m.shape[1], dtype=F32)
    for i in range(m.shape[0]):
        if not s[i] >= F32(score_thr):                                                # a NaN fails
            continue
        win = m[i] & ((out < 0) | (s[i] > top))                                       # strictly larger: ties stay with the lower i
        out[win], top[win] = i, s[i]
    return out


def render_prediction(ref, pred, depth, depth_scale, intr, c2w, radius, score_thr=0.0, fill=-1, near=0.1, far=6.0):
    """The five images of `transfer.render_prediction` from host arrays of the same fields -> dict of int32 [V, Hd, Wd]."""
    idx, _ = nearest_pixels(ref, depth, depth_scale, intr, c2w, radius, near, far)
    imap = instance_map(pred["pts_instance_mask"][0], pred["instance_scores"], score_thr)
    chans = dict(semantic=pred["pts_semantic_mask"][0], panoptic_semantic=pred["pts_semantic_mask"][1],
                 panoptic_instance=pred["pts_instance_mask"][1], instance=imap,
                 instance_label=take_labels(pred["instance_labels"], imap, fill))
    return {k: take_labels(v, idx, fill) for k, v in chans.items()}
