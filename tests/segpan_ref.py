"""Plain numpy restatement of the two protocols `segdino3d_amd/eval_seg.py` scores on the device - test infrastructure, written the
slow way the protocols are written and sharing no code with the package:

  * semantic: mmdet3d's `seg_eval` - ignored ground truth set to -1, `fast_hist` (`np.bincount(C * gt[k] + pred[k])` over
    `k = (gt >= 0) & (gt < C)`), `per_class_iou`, `get_acc`, `get_acc_cls`;
  * panoptic: mmdet3d's `EvalPanoptic.add_batch_panoptic` (the SemanticKITTI protocol): the class loop with full-length masks and
    `np.unique(..., return_counts=True)` on `pred + offset * gt`, then `evaluate` (sq / rq / pq per class and their means).

Ratios are taken in float64."""
import numpy as np


# ------------------------------------------------------------------------------------------------ semantic
def fast_hist(preds, labels, num_classes):
    k = (labels >= 0) & (labels < num_classes)
    bin_count = np.bincount(num_classes * labels[k].astype(np.int64) + preds[k], minlength=num_classes ** 2)
    return bin_count[:num_classes ** 2].reshape(num_classes, num_classes)


def confusion(gt_labels, seg_preds, num_classes, ignore_index):
    hist = np.zeros((num_classes, num_classes), dtype=np.int64)
    for gt, pred in zip(gt_labels, seg_preds):
        gt = np.asarray(gt).astype(np.int64).copy()
        pred = np.asarray(pred).astype(np.int64).copy()
        pred[gt == ignore_index] = -1
        gt[gt == ignore_index] = -1
        hist += fast_hist(pred, gt, num_classes)
    return hist


def seg_eval(gt_labels, seg_preds, label2cat, ignore_index):
    num_classes = len(label2cat)
    hist = confusion(gt_labels, seg_preds, num_classes, ignore_index).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.diag(hist) / (hist.sum(1) + hist.sum(0) - np.diag(hist))
        if 0 <= ignore_index < num_classes:
            iou[ignore_index] = np.nan
        ret = {label2cat[i]: float(iou[i]) for i in range(num_classes)}
        ret["miou"] = float(np.nanmean(iou)) if np.isfinite(iou).any() else float("nan")
        ret["acc"] = float(np.diag(hist).sum() / hist.sum())
        acc_cls = np.diag(hist) / hist.sum(axis=1)
        ret["acc_cls"] = float(np.nanmean(acc_cls)) if np.isfinite(acc_cls).any() else float("nan")
    return ret


# ------------------------------------------------------------------------------------------------ panoptic
class EvalPanoptic:
    def __init__(self, n_classes, ignore, min_points, offset=2 ** 16):
        self.n_classes = n_classes
        self.ignore = np.array(sorted(ignore), dtype=np.int64)
        self.include = np.array([n for n in range(n_classes) if n not in ignore], dtype=np.int64)
        self.min_points = min_points
        self.offset = offset
        self.pan_tp = np.zeros(n_classes, dtype=np.int64)
        self.pan_iou = np.zeros(n_classes, dtype=np.float64)
        self.pan_fp = np.zeros(n_classes, dtype=np.int64)
        self.pan_fn = np.zeros(n_classes, dtype=np.int64)
        self.n_matches = 0

    def add_scene(self, x_sem_row, x_inst_row, y_sem_row, y_inst_row):
        """x: prediction, y: ground truth."""
        x_sem_row = np.asarray(x_sem_row).astype(np.int64)
        y_sem_row = np.asarray(y_sem_row).astype(np.int64)
        x_inst_row = np.asarray(x_inst_row).astype(np.int64) + 1
        y_inst_row = np.asarray(y_inst_row).astype(np.int64) + 1
        for cl in self.ignore:
            keep = y_sem_row != cl
            x_sem_row, y_sem_row = x_sem_row[keep], y_sem_row[keep]
            x_inst_row, y_inst_row = x_inst_row[keep], y_inst_row[keep]
        for cl in self.include:
            x_inst_in_cl = x_inst_row * (x_sem_row == cl).astype(np.int64)
            y_inst_in_cl = y_inst_row * (y_sem_row == cl).astype(np.int64)
            unique_pred, counts_pred = np.unique(x_inst_in_cl[x_inst_in_cl > 0], return_counts=True)
            id2idx_pred = {i: idx for idx, i in enumerate(unique_pred)}
            matched_pred = np.zeros(unique_pred.shape[0], dtype=bool)
            unique_gt, counts_gt = np.unique(y_inst_in_cl[y_inst_in_cl > 0], return_counts=True)
            id2idx_gt = {i: idx for idx, i in enumerate(unique_gt)}
            matched_gt = np.zeros(unique_gt.shape[0], dtype=bool)
            valid_combos = np.logical_and(x_inst_in_cl > 0, y_inst_in_cl > 0)
            offset_combo = x_inst_in_cl[valid_combos] + self.offset * y_inst_in_cl[valid_combos]
            unique_combo, counts_combo = np.unique(offset_combo, return_counts=True)
            gt_labels = unique_combo // self.offset
            pred_labels = unique_combo % self.offset
            gt_areas = np.array([counts_gt[id2idx_gt[i]] for i in gt_labels], dtype=np.int64)
            pred_areas = np.array([counts_pred[id2idx_pred[i]] for i in pred_labels], dtype=np.int64)
            intersections = counts_combo.astype(np.int64)
            unions = gt_areas + pred_areas - intersections
            ious = intersections.astype(np.float64) / unions.astype(np.float64)
            tp_indexes = 2 * intersections > unions                     # iou > 0.5, strictly, decided on integers
            self.pan_tp[cl] += int(np.sum(tp_indexes))
            self.pan_iou[cl] += np.sum(ious[tp_indexes])
            self.n_matches += int(np.sum(tp_indexes))
            matched_gt[[id2idx_gt[i] for i in gt_labels[tp_indexes]]] = True
            matched_pred[[id2idx_pred[i] for i in pred_labels[tp_indexes]]] = True
            self.pan_fn[cl] += int(np.sum(np.logical_and(counts_gt >= self.min_points, ~matched_gt)))
            self.pan_fp[cl] += int(np.sum(np.logical_and(counts_pred >= self.min_points, ~matched_pred)))

    def evaluate(self, classes, thing_classes, stuff_classes, label2cat):
        eps = 1e-15
        tp, fp, fn = (a.astype(np.float64) for a in (self.pan_tp, self.pan_fp, self.pan_fn))
        sq_all = self.pan_iou / np.maximum(tp, eps)
        rq_all = tp / np.maximum(tp + 0.5 * fp + 0.5 * fn, eps)
        pq_all = sq_all * rq_all
        inc = self.include
        ret = {"pq": float(pq_all[inc].mean()) if len(inc) else 0.0, "sq": float(sq_all[inc].mean()) if len(inc) else 0.0,
               "rq": float(rq_all[inc].mean()) if len(inc) else 0.0}
        per = {}
        for i in inc:
            per[label2cat[int(i)]] = {"pq": float(pq_all[i]), "sq": float(sq_all[i]), "rq": float(rq_all[i])}
        for name, subset in (("thing", thing_classes), ("stuff", stuff_classes)):
            for m in ("pq", "sq", "rq"):
                vals = [per[c][m] for c in subset if c in per]
                ret[f"{m}_{name}"] = float(np.mean(vals)) if vals else 0.0
        ret["classes"] = per
        return ret


def panoptic_counts(gt_sem, gt_inst, pred_sem, pred_inst, n_classes, ignore, min_num_points, id_offset=2 ** 16):
    """Scene lists -> (tp, fp, fn, iou_sum, n_matches) summed over the scenes."""
    ev = EvalPanoptic(n_classes, list(ignore), min_num_points, id_offset)
    for gs, gi, ps, pi in zip(gt_sem, gt_inst, pred_sem, pred_inst):
        ev.add_scene(ps, pi, gs, gi)
    return ev.pan_tp, ev.pan_fp, ev.pan_fn, ev.pan_iou, ev.n_matches


def panoptic_seg_eval(gt_labels, seg_preds, classes, thing_classes, stuff_classes, min_num_points, id_offset, label2cat, ignore_index):
    """gt_labels / seg_preds: per scene dict(pts_semantic_mask, pts_instance_mask); ignore_index: a list of class indices."""
    ev = EvalPanoptic(len(classes), list(ignore_index), min_num_points, id_offset)
    for gt, pred in zip(gt_labels, seg_preds):
        ev.add_scene(pred["pts_semantic_mask"], pred["pts_instance_mask"], gt["pts_semantic_mask"], gt["pts_instance_mask"])
    return ev.evaluate(classes, thing_classes, stuff_classes, label2cat)


# ------------------------------------------------------------------------------------------------ seeded scenes
def make_gt(seed, n, n_classes, n_stuff=2, n_runs=14):
    """Contiguous ground-truth runs as tests/golden/make_golden_evaluator.py draws them: `n_stuff` stuff classes whose instance id
    equals the class, things numbered from `n_stuff`; the last class index (`n_classes - 1`) is the ignored one and is not drawn."""
    g = np.random.default_rng(seed)
    n_runs = max(1, min(n_runs, n // 2))
    if n_runs > 1:
        bounds = np.sort(g.choice(np.arange(1, n), size=n_runs - 1, replace=False))
        edges = [0] + bounds.tolist() + [n]
    else:
        edges = [0, n]
    sem = np.zeros(n, dtype=np.int64)
    inst = np.zeros(n, dtype=np.int64)
    next_inst = n_stuff
    for lo, hi in zip(edges[:-1], edges[1:]):
        c = int(g.integers(0, n_classes - 1))
        sem[lo:hi] = c
        if c < n_stuff:
            inst[lo:hi] = c
        else:
            inst[lo:hi] = next_inst
            next_inst += 1
    return sem, inst, edges


def make_pred(seed, sem, inst, edges, n_classes, n_stuff=2):
    """Predictions: the ground truth rolled by 5..60 points; a quarter of the runs relabelled, a fifth split in two."""
    g = np.random.default_rng(seed + 7919)
    n = sem.shape[0]
    ps, pi = sem.copy(), inst.copy()
    next_inst = int(inst.max()) + 1
    for lo, hi in zip(edges[:-1], edges[1:]):
        if g.random() < 0.25:
            c = int(g.integers(0, n_classes - 1))
            ps[lo:hi] = c
            if c < n_stuff:
                pi[lo:hi] = c
            elif sem[lo] < n_stuff:
                pi[lo:hi] = next_inst
                next_inst += 1
        if g.random() < 0.2 and hi - lo >= 2:
            mid = (lo + hi) // 2
            if ps[lo] >= n_stuff:
                pi[mid:hi] = next_inst
                next_inst += 1
    shift = int(g.integers(5, 61)) % max(n, 1)
    return np.roll(ps, shift), np.roll(pi, shift)


def make_scene(seed, n, n_classes, n_stuff=2, n_runs=14):
    sem, inst, edges = make_gt(seed, n, n_classes, n_stuff, n_runs)
    ps, pi = make_pred(seed, sem, inst, edges, n_classes, n_stuff)
    return sem, inst, ps, pi
