"""numpy float64 restatement of the 3D box AP / AR protocol of segdino3d_amd/eval_box.py (csrc/boxeval.hip): the VOC-style indoor
detection protocol for axis-aligned boxes as include/segdino3d_hip.h states it.  Test infrastructure, no device.

The matching is written as the protocol reads: one sequential walk over a scene's predictions in (score descending, row ascending) order
with `taken` flags per (ground truth, threshold) - NOT as the decomposition the kernels use (best ground truth first, then a minimum
per (ground truth, threshold)); the device route is held to this un-decomposed form."""
import numpy as np

INSTANCE_COLS = 1000
BAD_INSTANCE, MIXED_SEMANTIC, BAD_LABEL, BAD_SCORE, STORE_FULL, BAD_COORD, BAD_BOX = 1, 2, 4, 8, 16, 32, 64
EPS = np.finfo(np.float64).eps


def map_ids(gt_sem, gt_inst, valid_class_ids, num_stuff):
    """`map_inst_markup` as the kernels apply it: ids shifted by the stuff classes, semantic ids through valid_class_ids + [-1]."""
    sem, inst = np.asarray(gt_sem, dtype=np.int64).copy(), np.asarray(gt_inst, dtype=np.int64).copy()
    inst -= num_stuff
    inst[inst < 0] = -1
    sem -= num_stuff
    sem[inst == -1] = -1
    id_map = np.array(list(valid_class_ids) + [-1], dtype=np.int64)
    idx = np.where(sem < 0, sem + len(id_map), sem)
    ok = (idx >= 0) & (idx < len(id_map))
    return np.where(ok, id_map[np.clip(idx, 0, len(id_map) - 1)], -1), inst


def gt_boxes(points, gt_sem, gt_inst, valid_class_ids, num_stuff=None):
    """(corners float32 [1000, 6], cls int32 [1000], status): one box per instance column, the id rule of `sd3d_ap_scene`.
    num_stuff None: ids as given."""
    pts = np.asarray(points, dtype=np.float32)[:, :3]
    valid = list(valid_class_ids)
    C = len(valid)
    if num_stuff is None:
        sem, inst = np.asarray(gt_sem, dtype=np.int64), np.asarray(gt_inst, dtype=np.int64)
    else:
        sem, inst = map_ids(gt_sem, gt_inst, valid, num_stuff)
    lut = np.full(max(valid) + 1, -1, dtype=np.int64)
    lut[valid] = np.arange(C)
    cls_pt = np.where((sem >= 0) & (sem < len(lut)), lut[np.clip(sem, 0, len(lut) - 1)], -1)
    status = 0
    corners = np.zeros((INSTANCE_COLS, 6), dtype=np.float32)
    cls = np.full(INSTANCE_COLS, -1, dtype=np.int32)
    bad = (inst < -1) | (inst >= INSTANCE_COLS)
    if bad.any():
        status |= BAD_INSTANCE
    member = ~bad & (cls_pt >= 0) & (inst != -1) & ~((sem == 0) & (inst == 0))
    for i in np.unique(inst[member]):
        sel = member & (inst == i)
        cs = np.unique(cls_pt[sel])
        if len(cs) > 1:
            status |= MIXED_SEMANTIC
        p = pts[sel]
        if not np.isfinite(p).all():
            status |= BAD_COORD
            continue
        cls[i] = cs.max()
        corners[i, :3] = p.min(axis=0) + np.float32(0.0)          # -0 reads as +0
        corners[i, 3:] = p.max(axis=0) + np.float32(0.0)
    assert C >= 1
    return corners, cls, status


def iou_to_all(box, gt_corners):
    """float64 IoU of one (centre, size) fp32 box against corner boxes [G, 6]; every operation rounded on its own."""
    b = np.asarray(box, dtype=np.float32).astype(np.float64)
    g = np.asarray(gt_corners, dtype=np.float32).astype(np.float64).reshape(-1, 6)
    half = b[3:] / 2.0
    alo, ahi = b[:3] - half, b[:3] + half
    blo, bhi = g[:, :3], g[:, 3:]
    da, db = ahi - alo, bhi - blo
    va = (da[0] * da[1]) * da[2]
    vb = (db[:, 0] * db[:, 1]) * db[:, 2]
    o = np.maximum(0.0, np.minimum(ahi[None], bhi) - np.maximum(alo[None], blo))
    inter = (o[:, 0] * o[:, 1]) * o[:, 2]
    den = (va + vb) - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den == 0.0, 0.0, inter / np.where(den == 0.0, 1.0, den))


def scene(gt_corners, gt_cls, boxes, labels, scores, n_classes, thresholds):
    """One scene -> dict(entries = [(group, score float32, true)], npos [C], has_pred [C], status, ious = every IoU that was computed)."""
    C, thr = int(n_classes), [float(t) for t in thresholds]
    T = len(thr)
    gt_corners = np.asarray(gt_corners, dtype=np.float32).reshape(-1, 6)
    gt_cls = np.asarray(gt_cls, dtype=np.int64).reshape(-1).copy()
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 6)
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    status = 0
    npos, has_pred = np.zeros(C, dtype=np.int64), np.zeros(C, dtype=bool)
    for g in range(len(gt_cls)):
        if gt_cls[g] < -1 or gt_cls[g] >= C:
            status |= BAD_LABEL
            gt_cls[g] = -1
        if gt_cls[g] >= 0 and not (np.isfinite(gt_corners[g]).all() and (gt_corners[g, 3:] >= gt_corners[g, :3]).all()):
            status |= BAD_COORD
            gt_cls[g] = -1
        if gt_cls[g] >= 0:
            npos[gt_cls[g]] += 1
    keep = np.ones(len(labels), dtype=bool)
    for r in range(len(labels)):
        if labels[r] < 0 or labels[r] >= C:
            status |= BAD_LABEL
            keep[r] = False
        if not np.isfinite(scores[r]):
            status |= BAD_SCORE
            keep[r] = False
        if not (np.isfinite(boxes[r]).all() and (boxes[r, 3:] >= 0).all()):
            status |= BAD_BOX
            keep[r] = False
    entries, ious = [], []
    neg = -scores.astype(np.float64)
    order = np.lexsort((np.arange(len(scores)), neg))                 # score descending, row ascending (-0 == +0)
    taken = np.zeros((len(gt_cls), T), dtype=bool)
    for r in order:
        if not keep[r]:
            continue
        c = int(labels[r])
        has_pred[c] = True
        cols = np.flatnonzero(gt_cls == c)
        if len(cols) == 0:
            entries += [(c * T + o, scores[r], 0) for o in range(T)]
            continue
        v = iou_to_all(boxes[r], gt_corners[cols])
        ious.append(v)
        k = int(np.argmax(v))                                         # the first maximum: the lowest column
        j = cols[k]
        for o in range(T):
            if v[k] > thr[o] and not taken[j, o]:
                taken[j, o] = True
                entries.append((c * T + o, scores[r], 1))
            else:
                entries.append((c * T + o, scores[r], 0))
    return dict(entries=entries, npos=npos, has_pred=has_pred, status=status, ious=np.concatenate(ious) if ious else np.zeros(0))


def accumulate(scenes, n_classes):
    """Scenes of `scene()` -> (group, score, true) sorted by (group, score, true), npos [C], has_pred [C], status."""
    C = int(n_classes)
    npos, has_pred, status = np.zeros(C, dtype=np.int64), np.zeros(C, dtype=bool), 0
    ent = []
    for s in scenes:
        npos += s["npos"]
        has_pred |= s["has_pred"]
        status |= s["status"]
        ent += s["entries"]
    group = np.array([e[0] for e in ent], dtype=np.int64)
    score = np.array([e[1] for e in ent], dtype=np.float32)
    true = np.array([e[2] for e in ent], dtype=np.int64)
    order = np.lexsort((true, score, group))
    return group[order], score[order], true[order], npos, has_pred, status


def finish(group, score, true, npos, n_thresholds):
    """(ap [C, T], ar [C, T]) float64."""
    C, T = len(npos), int(n_thresholds)
    ap, ar = np.full((C, T), np.nan), np.full((C, T), np.nan)
    for c in range(C):
        if npos[c] == 0:
            continue
        for o in range(T):
            sel = group == c * T + o
            if not sel.any():
                ap[c, o] = ar[c, o] = 0.0
                continue
            s, t = score[sel].astype(np.float64), true[sel]
            order = np.lexsort((-t, -s))                              # score descending, true before false
            t = t[order]
            tp, fp = np.cumsum(t).astype(np.float64), np.cumsum(1 - t).astype(np.float64)
            rec = tp / float(npos[c])
            prec = tp / np.maximum(tp + fp, EPS)
            mrec = np.concatenate([[0.0], rec, [1.0]])
            mpre = np.concatenate([[0.0], prec, [0.0]])
            for i in range(len(mpre) - 1, 0, -1):
                mpre[i - 1] = max(mpre[i - 1], mpre[i])
            idx = np.flatnonzero(mrec[1:] != mrec[:-1])
            ap[c, o] = np.sum((mrec[idx + 1] - mrec[idx]) * mpre[idx + 1])
            ar[c, o] = rec[-1]
    return ap, ar


def tables(scenes, n_classes, n_thresholds):
    group, score, true, npos, _, _ = accumulate(scenes, n_classes)
    return finish(group, score, true, npos, n_thresholds)


def result(ap, ar, class_labels, thresholds):
    """The dictionary with mmdet3d's key shapes; the means run over the classes with ground truth."""
    out = {}
    for o, t in enumerate(thresholds):
        for c, name in enumerate(class_labels):
            out[f"{name}_AP_{t:.2f}"] = float(ap[c, o])
            out[f"{name}_rec_{t:.2f}"] = float(ar[c, o])
        have = ~np.isnan(ap[:, o])
        out[f"mAP_{t:.2f}"] = float(ap[have, o].mean()) if have.any() else float("nan")
        out[f"mAR_{t:.2f}"] = float(ar[have, o].mean()) if have.any() else float("nan")
    return out


def make_scene(seed, n, n_classes, present, gt_per_class, distinct_scores=False):
    """A generated scene: `gt_per_class` ground-truth boxes for each class of `present`, `n` predictions scattered around them (some
    with another label, some far from everything).  Returns dict(gt_corners, gt_cls, boxes, labels, scores); the ground truth sits
    in scattered instance columns, columns without an instance have class -1."""
    rng = np.random.RandomState(seed)
    present = list(present)
    G = len(present) * gt_per_class
    cols = np.sort(rng.choice(INSTANCE_COLS, size=G, replace=False)) if G else np.zeros(0, dtype=np.int64)
    n_cols = int(cols.max()) + 1 if G else 0
    gt_corners = np.zeros((n_cols, 6), dtype=np.float32)
    gt_cls = np.full(n_cols, -1, dtype=np.int32)
    centre = rng.uniform(0.0, 6.0, size=(G, 3))
    size = rng.uniform(0.3, 1.5, size=(G, 3))
    if G:
        gt_corners[cols, :3] = (centre - size / 2).astype(np.float32)
        gt_corners[cols, 3:] = (centre + size / 2).astype(np.float32)
        gt_cls[cols] = np.repeat(np.asarray(present, dtype=np.int32), gt_per_class)[rng.permutation(G)]
    boxes = np.zeros((n, 6), dtype=np.float32)
    labels = np.zeros(n, dtype=np.int64)
    for r in range(n):
        if G and rng.rand() < 0.85:
            g = rng.randint(G)
            boxes[r, :3] = centre[g] + rng.normal(0.0, 0.12, 3) * size[g]
            boxes[r, 3:] = size[g] * rng.uniform(0.75, 1.3, 3)
            labels[r] = gt_cls[cols[g]] if rng.rand() < 0.85 else rng.randint(n_classes)
        else:
            boxes[r, :3] = rng.uniform(0.0, 6.0, 3)
            boxes[r, 3:] = rng.uniform(0.3, 1.5, 3)
            labels[r] = rng.randint(n_classes)
    if distinct_scores:
        scores = (rng.permutation(n).astype(np.float32) + 1.0) / np.float32(n + 1)
    else:
        scores = rng.randint(1, 33, size=n).astype(np.float32) / np.float32(32.0)      # many ties
    return dict(gt_corners=gt_corners, gt_cls=gt_cls, boxes=boxes, labels=labels, scores=scores)


def scene_of(s, n_classes, thresholds):
    return scene(s["gt_corners"], s["gt_cls"], s["boxes"], s["labels"], s["scores"], n_classes, thresholds)
