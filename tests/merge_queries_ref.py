"""The rule of the query merging (segdino3d_amd/lift_queries.py, steps 1 to 8 of `merge_queries`; include/segdino3d_hip.h) restated on
the CPU: numpy float32 for the fixed-point centre and the quantised feature (single rounded operations, the same bits anywhere), exact
integers from there on (numpy int64 inside the bounds the rule states, Python ints for the cluster sums), float64 for the feature mean
(`feat_dtype=np.float32` evaluates that mean sequentially in float32 instead, the arithmetic the kernel is asked to perform).

The adjacency of a rank is computed when the walk makes it a seed, so a case of many rows and few clusters stays cheap."""
import numpy as np

MAX_ROWS = 16384
WORLD = float(2 ** 14)
W_MAX = 2 ** 20
DEFAULTS = dict(radius=0.3, sim=0.75, min_views=1, max_queries=None, reduce="mean", score_thr=0.3, min_pixels=16)


def rule(**kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    r = {**DEFAULTS, **kw}
    r["radius_q"] = round(float(r["radius"]) * 1024)
    r["sim_q"] = 0 if r["sim"] is None else round(float(r["sim"]) * 128)
    assert 1 <= r["radius_q"] <= 2 ** 20 and 0 <= r["sim_q"] <= 128 and (r["sim"] is None or r["sim_q"] >= 1)
    return r


def score_keys(scores):
    """The keys of `sd3d_keys_from_f32(descending)`: ascending key = descending score; equal floats are equal keys, +0 before -0."""
    u = np.ascontiguousarray(scores, np.float32).view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return (~k).astype(np.uint32)


def ranked_rows(centre, scores, count, score_thr, min_pixels):
    """Steps 1 and 2 -> the entering rows in rank order (score descending, ties to the lower row), at most MAX_ROWS of them."""
    centre, scores, count = np.asarray(centre, np.float32).reshape(-1, 3), np.asarray(scores, np.float32), np.asarray(count)
    with np.errstate(invalid="ignore"):
        valid = (scores >= np.float32(score_thr)) & (count >= min_pixels) & (np.abs(centre) < np.float32(WORLD)).all(axis=1)
    rows = np.nonzero(valid)[0]
    order = np.lexsort((rows, score_keys(scores[rows])))                              # the last key is the primary one
    return rows[order][:MAX_ROWS].astype(np.int64)


def fixed_point(centre):
    """Step 3: rint(centre * 1024) as int32, the product rounded to float32 (it is exact)."""
    return np.rint(np.asarray(centre, np.float32) * np.float32(1024.0)).astype(np.int32)


def quantise(feats):
    """Step 4 -> (codes int8 [m, C], nrm int64 [m])."""
    f = np.asarray(feats).astype(np.float32)                                          # float16 -> float32 is exact
    m, C = f.shape
    q = np.zeros((m, C), np.int8)
    for i in range(m):
        with np.errstate(invalid="ignore"):
            s = np.float32(np.abs(f[i]).max()) if C else np.float32(0)
        if not np.isfinite(f[i]).all() or not s >= np.float32(2.0 ** -100):
            continue
        e = int(np.frexp(s)[1])                                                       # s = m 2^e with 1/2 <= m < 1
        x = np.rint(f[i] * np.float32(2.0 ** (7 - e)))                                # float32 times a power of two: one rounding
        q[i] = np.clip(x, -127, 127).astype(np.int8)
    return q, (q.astype(np.int64) ** 2).sum(axis=1)


def adjacent_row(a, p, q64, nrm, radius_q, sim_q):
    """Step 5 for rank `a` against every rank -> bool [m], False at ranks <= a.  p int64 [m, 3], q64 float64 codes (sums of products of
    int8 values stay far below 2^53: exact), nrm int64."""
    m = len(nrm)
    d2 = ((p - p[a]) ** 2).sum(axis=1)                                                # int64, <= 3 * 2^50
    ok = (d2 <= radius_q * radius_q) & (nrm > 0) & bool(nrm[a] > 0)
    if sim_q:
        d = (q64 @ q64[a]).astype(np.int64)
        ok &= (d > 0) & (d * d * 16384 >= sim_q * sim_q * int(nrm[a]) * nrm)         # both sides below 2^63 for C <= 1024
    ok[:a + 1] = False
    return ok


def adjacency_bits(ranks_p, codes, nrm, radius_q, sim_q):
    """The whole matrix, for the tests of the Gram kernel: bool [m, m], entry [a, b] set iff a < b and the ranks are adjacent."""
    p, q64 = ranks_p.astype(np.int64), codes.astype(np.float64)
    return np.stack([adjacent_row(a, p, q64, nrm, radius_q, sim_q) for a in range(len(nrm))]) if len(nrm) else np.zeros((0, 0), bool)


def leader_labels(p, codes, nrm, radius_q, sim_q):
    """Step 6 -> label int64 [m]: the seed rank of every rank."""
    m = len(nrm)
    p, q64 = p.astype(np.int64), codes.astype(np.float64)
    label = np.full(m, -1, np.int64)
    for a in range(m):
        if label[a] >= 0:
            continue
        label[a] = a
        take = adjacent_row(a, p, q64, nrm, radius_q, sim_q) & (label < 0)
        label[take] = a
    return label


def merge(feats, centre, scores, count, queries_per_view, feat_dtype=np.float64, **kw):
    """-> dict(feats [K, C] in `feat_dtype`, pos float32 [K, 3], scores float32 [K], views int32 [K], labels int32 [n], seeds: the seed
    row of each emitted cluster, members: their rows ascending)."""
    r = rule(**kw)
    feats, centre = np.asarray(feats), np.asarray(centre, np.float32).reshape(-1, 3)
    scores, count = np.asarray(scores, np.float32), np.asarray(count, np.int32)
    n, C = feats.shape
    assert C <= 1024
    rows = ranked_rows(centre, scores, count, r["score_thr"], r["min_pixels"])
    p = fixed_point(centre[rows])
    codes, nrm = quantise(feats[rows])
    label = leader_labels(p, codes, nrm, r["radius_q"], r["sim_q"])
    clusters = []
    for a in np.nonzero(label == np.arange(len(rows)))[0]:
        ranks = np.nonzero(label == a)[0]
        ranks = ranks[np.argsort(rows[ranks])]                                        # members in ascending row order
        w = [min(int(count[i]), W_MAX) for i in rows[ranks]]
        sw = sum(w)
        pos = [np.float32(float(sum(wi * int(p[k, c]) for wi, k in zip(w, ranks))) / float(sw) / 1024.0) for c in range(3)]
        views = len({int(i) // queries_per_view for i in rows[ranks]})
        clusters.append(dict(seed=int(rows[a]), rows=rows[ranks], w=w, sw=sw, pos=pos, views=views, score=scores[rows[a]]))
    clusters = [c for c in clusters if c["views"] >= r["min_views"]]
    if r["max_queries"] is not None and len(clusters) > r["max_queries"]:
        keys = score_keys(np.array([c["score"] for c in clusters], np.float32))
        order = sorted(range(len(clusters)), key=lambda i: (int(keys[i]), clusters[i]["seed"]))
        clusters = [clusters[i] for i in order[:r["max_queries"]]]
    clusters.sort(key=lambda c: c["seed"])
    K = len(clusters)
    out = np.zeros((K, C), feat_dtype)
    labels = np.full(n, -1, np.int32)
    for k, c in enumerate(clusters):
        labels[c["rows"]] = k
        if r["reduce"] == "best":
            out[k] = feats[c["seed"]].astype(feat_dtype)
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            if feat_dtype == np.float32:                                              # acc = acc + (float) w * f, each operation rounded
                acc = np.zeros(C, np.float32)
                for wi, i in zip(c["w"], c["rows"]):
                    acc = acc + np.float32(wi) * feats[i].astype(np.float32)
                out[k] = acc / np.float32(c["sw"])
            else:
                acc = np.zeros(C, np.float64)
                for wi, i in zip(c["w"], c["rows"]):
                    acc += float(wi) * feats[i].astype(np.float64)
                out[k] = acc / float(c["sw"])
    return dict(feats=out, pos=np.array([c["pos"] for c in clusters], np.float32).reshape(K, 3),
                scores=np.array([c["score"] for c in clusters], np.float32), views=np.array([c["views"] for c in clusters], np.int32),
                labels=labels, seeds=np.array([c["seed"] for c in clusters], np.int64), members=[c["rows"] for c in clusters])
