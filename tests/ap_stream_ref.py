"""Plain numpy restatement of the streamed AP protocol (segdino3d_amd.eval_ap.ApAccumulator, csrc/apeval.hip) - test infrastructure.

`evaluate_records` (the reference's `evaluate_matches`) loops overlaps x classes x scenes; its `visited` flags never cross a
(scene, label, overlap) triple, so the protocol decomposes:

  * per scene and per (class, overlap) the greedy matching emits ENTRIES `(group = class * O + overlap, score, true)`, a count of hard
    false negatives and the flags has_gt / has_pred (`scene_entries`);
  * the entries of all scenes, in any order, sorted by (group, score) give every group's precision / recall curve (`finish`).

`scene_record` builds the compact record of one scene from raw arrays by the device path's column rule (the instance index is the
ground-truth instance when the semantic id is a valid class; void otherwise), so device integers can be compared against it.
"""
import numpy as np

from segdino3d_amd.eval_ap import SceneRecord

INSTANCE_COLS = 1000


def entry_bound(th) -> int:
    """Entries one prediction can emit at overlap th: IoU > th needs inter > th * |pred|, ground truths are disjoint."""
    return max(1, int(np.ceil(1.0 / float(th))) - 1)


def scene_record(gt_sem, gt_inst, masks, labels, scores, valid_class_ids, min_region) -> SceneRecord:
    """What `rename_gt` + `assign_scene` give for ids that went through `map_inst_markup` (instance index in [-1, 1000), one semantic
    id per instance, semantic id -1 wherever the index is -1), by the column rule of the device path."""
    gt_sem, gt_inst = np.asarray(gt_sem, dtype=np.int64), np.asarray(gt_inst, dtype=np.int64)
    masks = np.asarray(masks).astype(bool).reshape(len(labels), len(gt_sem))
    valid = [int(v) for v in valid_class_ids]
    assert gt_inst.min(initial=0) >= -1 and gt_inst.max(initial=0) < INSTANCE_COLS
    is_valid = np.isin(gt_sem, valid)
    inst_pt = is_valid & (gt_inst >= 0) & ~((gt_sem == 0) & (gt_inst == 0))
    void_pt = ~is_valid | (gt_inst == -1)
    col = np.where(inst_pt, gt_inst, np.where(void_pt, INSTANCE_COLS, INSTANCE_COLS + 1))   # instance index, void, counted nowhere
    ids = np.unique(gt_inst[inst_pt])                                          # ascending instance index
    gt_vert = np.bincount(col, minlength=INSTANCE_COLS + 2)[ids].astype(np.int64)
    gt_label = np.zeros(len(ids), dtype=np.int64)
    for g, i in enumerate(ids):
        sems = np.unique(gt_sem[col == i])
        assert len(sems) == 1, "an instance spans several semantic classes"
        gt_label[g] = sems[0]
    # the reference lists ground truth in ascending id = 1000 * label + index: within a label that is ascending index
    vert = masks.sum(axis=1).astype(np.int64)
    label_id = np.asarray(valid, dtype=np.int64)[np.asarray(labels, dtype=np.int64)] if len(labels) else np.zeros(0, dtype=np.int64)
    idx = np.flatnonzero(vert >= min_region)
    counts = np.stack([np.bincount(col[masks[p]], minlength=INSTANCE_COLS + 2) for p in idx]) if len(idx) else \
        np.zeros((0, INSTANCE_COLS + 2), dtype=np.int64)
    inter = counts[:, ids]
    same = (label_id[idx][:, None] == gt_label[None, :]) & (inter > 0)
    pp, gg = np.nonzero(same)                                                  # row-major: predictions in order, their ground truths in order
    a = lambda x: np.asarray(x, dtype=np.int64)                                # noqa: E731
    return SceneRecord(pred_label=label_id[idx], pred_index=a(idx), pred_vert=vert[idx], pred_void=a(counts[:, INSTANCE_COLS]),
                       pred_conf=np.asarray(scores, dtype=np.float64)[idx], gt_label=gt_label, gt_id=gt_label * 1000 + ids,
                       gt_vert=gt_vert, pair_pred=a(pp), pair_gt=a(gg), pair_inter=a(inter[pp, gg]))


def scene_entries(rec: SceneRecord, valid_class_ids, overlaps, min_region):
    """One scene of `evaluate_records:214-269`: (entries [(group, score, true)], hard_fn [C, O], has_gt [C], has_pred [C], stats).
    `stats`: counts of matched / extra / false-positive entries, predictions dropped by the ignore test, and the largest number of
    entries one prediction emitted per overlap."""
    label_ids = [int(v) for v in valid_class_ids]
    C, O = len(label_ids), len(overlaps)
    entries = []
    hard_fn = np.zeros((C, O), dtype=np.int64)
    has_gt, has_pred = np.zeros(C, dtype=bool), np.zeros(C, dtype=bool)
    stats = dict(matched=0, extra=0, fp=0, ignored=0, per_pred_max=np.zeros(O, dtype=np.int64))
    by_gt = np.lexsort((rec.pair_pred, rec.pair_gt))                           # a ground truth's pairs in prediction order
    gt_start = np.searchsorted(rec.pair_gt[by_gt], np.arange(len(rec.gt_id) + 1))
    pred_start = np.searchsorted(rec.pair_pred, np.arange(len(rec.pred_label) + 1))   # pairs are stored prediction by prediction
    for oi, th in enumerate(overlaps):
        visited = np.zeros(len(rec.pred_label), dtype=bool)
        emitted = np.zeros(len(rec.pred_label), dtype=np.int64)
        for li, lid in enumerate(label_ids):
            gts = [g for g in np.flatnonzero(rec.gt_label == lid) if rec.gt_vert[g] >= min_region]
            preds = np.flatnonzero(rec.pred_label == lid)
            has_gt[li] |= len(gts) > 0
            has_pred[li] |= len(preds) > 0
            group = li * O + oi
            for g in gts:
                cur_match, cur_score, first = False, -np.inf, -1
                for q in by_gt[gt_start[g]:gt_start[g + 1]]:
                    p = rec.pair_pred[q]
                    if visited[p]:
                        continue
                    inter = rec.pair_inter[q]
                    if float(inter) / (rec.gt_vert[g] + rec.pred_vert[p] - inter) > th:
                        conf = rec.pred_conf[p]
                        if cur_match:
                            entries.append((group, min(cur_score, conf), 0))
                            cur_score = max(cur_score, conf)
                            emitted[p] += 1
                            stats["extra"] += 1
                        else:
                            cur_match, cur_score, first = True, conf, p
                            visited[p] = True
                if not cur_match:
                    hard_fn[li, oi] += 1
                else:
                    entries.append((group, cur_score, 1))
                    emitted[first] += 1
                    stats["matched"] += 1
            for p in preds:
                qs = range(pred_start[p], pred_start[p + 1])
                if any(float(rec.pair_inter[q]) / (rec.gt_vert[rec.pair_gt[q]] + rec.pred_vert[p] - rec.pair_inter[q]) > th for q in qs):
                    continue
                ignore = int(rec.pred_void[p])
                for q in qs:
                    g = rec.pair_gt[q]
                    if rec.gt_id[g] < 1000:
                        ignore += int(rec.pair_inter[q])
                    if rec.gt_vert[g] < min_region:
                        ignore += int(rec.pair_inter[q])
                if float(ignore) / rec.pred_vert[p] <= th:
                    entries.append((group, rec.pred_conf[p], 0))
                    emitted[p] += 1
                    stats["fp"] += 1
                else:
                    stats["ignored"] += 1
        stats["per_pred_max"][oi] = emitted.max(initial=0)
    return entries, hard_fn, has_gt, has_pred, stats


def accumulate(records, valid_class_ids, overlaps, min_region):
    """All scenes: (entries sorted by (group, score, true) as three arrays, hard_fn, has_gt, has_pred, summed stats)."""
    C, O = len(valid_class_ids), len(overlaps)
    ent, hard_fn = [], np.zeros((C, O), dtype=np.int64)
    has_gt, has_pred = np.zeros(C, dtype=bool), np.zeros(C, dtype=bool)
    total = dict(matched=0, extra=0, fp=0, ignored=0, per_pred_max=np.zeros(O, dtype=np.int64))
    for rec in records:
        e, h, g, p, st = scene_entries(rec, valid_class_ids, overlaps, min_region)
        ent += e
        hard_fn += h
        has_gt |= g
        has_pred |= p
        for k in ("matched", "extra", "fp", "ignored"):
            total[k] += st[k]
        total["per_pred_max"] = np.maximum(total["per_pred_max"], st["per_pred_max"])
    group = np.array([e[0] for e in ent], dtype=np.int64)
    score = np.array([e[1] for e in ent], dtype=np.float64)
    true = np.array([e[2] for e in ent], dtype=np.int64)
    order = np.lexsort((true, score, group))
    return (group[order], score[order], true[order]), hard_fn, has_gt, has_pred, total


def finish(entries, hard_fn, has_gt, has_pred):
    """`evaluate_records:270-298` per group on the sorted entries: (ap [1, C, O], pr_rc [2, C, O])."""
    group, score, true = entries
    C, O = hard_fn.shape
    ap = np.zeros((1, C, O), float)
    pr_rc = np.zeros((2, C, O), float)
    for li in range(C):
        for oi in range(O):
            if has_gt[li] and has_pred[li]:
                sel = group == li * O + oi
                ys, yt = score[sel], true[sel].astype(float)                   # already ascending in the score
                n_ex, n_true = len(ys), yt.sum()
                first = np.flatnonzero(np.r_[True, ys[1:] != ys[:-1]]) if n_ex else np.zeros(0, dtype=np.int64)
                exc = np.cumsum(yt) - yt                                       # true entries of strictly smaller index
                prec, rec_ = np.zeros(len(first) + 1), np.zeros(len(first) + 1)
                for ir, isc in enumerate(first):
                    c = exc[isc]                                               # at the first index of a score: strictly smaller scores only
                    tp = n_true - c
                    fp = n_ex - isc - tp
                    fn = c + hard_fn[li, oi]
                    prec[ir] = float(tp) / (tp + fp)
                    rec_[ir] = float(tp) / (tp + fn)
                prec[-1], rec_[-1] = 1.0, 0.0
                f1 = 2 * prec * rec_ / (prec + rec_ + 0.0001)
                best = f1.argmax()
                best_pr, best_rc = prec[best], rec_[best]
                r_prev, r_next = np.r_[rec_[0], rec_[:-1]], np.r_[rec_[1:], 0.0]
                ap_cur = np.dot(prec, 0.5 * r_prev - 0.5 * r_next)
            elif has_gt[li]:
                ap_cur, best_pr, best_rc = 0.0, 0, 0
            else:
                ap_cur = best_pr = best_rc = float("nan")
            ap[0, li, oi] = ap_cur
            pr_rc[0, li, oi], pr_rc[1, li, oi] = best_pr, best_rc
    return ap, pr_rc
