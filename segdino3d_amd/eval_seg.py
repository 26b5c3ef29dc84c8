"""Semantic mIoU and panoptic PQ with the per-scene counting on the device.

The reference's evaluator collects, scene by scene, the semantic pair (`eval_ann['pts_semantic_mask']`, `pts_semantic_mask[0]`) and
the panoptic pair (`eval_ann`, `pts_semantic_mask[1]` / `pts_instance_mask[1]`) (`evaluation/evaluator_3d.py:128-163`) and would hand
them to mmdet3d's `seg_eval` / `panoptic_seg_eval` in a block that is commented out (`:184-196`).  This module restates the two
protocols:

  * `seg_eval`: `fast_hist` after ignored ground truth became -1 - a confusion matrix [C, C] (rows = ground truth) over the points
    whose ground truth lies in [0, C) and is not `ignore_index`; `miou` = nanmean of diag / (row + col - diag) with the ignored class
    NaN, `acc` = trace / total, `acc_cls` = nanmean of diag / row;
  * `panoptic_seg_eval`: `EvalPanoptic.add_batch_panoptic` (SemanticKITTI): ids + 1, ignored ground truth dropped, per class the
    segments of both sides, a pair with `2 * inter > union` is a true positive, unmatched segments of at least `min_num_points`
    points are fn / fp; `sq = iou_sum / max(tp, 1e-15)`, `rq = tp / max(tp + fp / 2 + fn / 2, 1e-15)`, `pq = sq * rq`, means over
    the classes that are not ignored.

`SegPanAccumulator.add` only enqueues the kernels of `csrc/segeval.hip` on the scene's tensors (no read-back, no synchronisation);
the counts live in one device buffer until `result()` reads it - the only read-back.  `state()` is a flat float64 tensor of fixed
width, so `dist_eval.all_gather_records(state()[None])` carries it between ranks and `merge` sums what arrives.  There is no CPU
path: `add` raises on CPU tensors.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .eval_ap import evaluator_instance_metrics


def _as_list(ignore_index) -> List[int]:
    if ignore_index is None:
        return []
    if isinstance(ignore_index, (int, np.integer)):
        return [int(ignore_index)]
    return [int(v) for v in ignore_index]


class SegPanAccumulator:
    """Device-resident counts of the semantic and the panoptic protocol over any number of scenes.

    State layout (`state()`, float64 [C * C + 4 C + 1]): confusion (row-major, rows = ground truth), tp, fp, fn, iou_sum, status.
    Counts are integers below 2^53, exact in float64.  `ignore_index`: a class index or a list of them (the reference's
    `metric_meta['ignore_index']`); the semantic protocol ignores the first, the panoptic one all of them.
    One accumulator belongs to one stream: the per-class adds of a scene are ordered by the stream, not by atomics.  A run that
    keeps several scenes in flight on several streams gives each stream its own accumulator and merges their states."""

    def __init__(self, n_classes: int, ignore_index, stuff_class_inds: Sequence[int], thing_class_inds: Sequence[int],
                 min_num_points: int, id_offset: int = 2 ** 16, device=None):
        self.n_classes = int(n_classes)
        if not 1 <= self.n_classes <= 1024:
            raise ValueError("n_classes: 1..1024")
        self.ignore = _as_list(ignore_index)
        if len(self.ignore) > 8:
            raise ValueError("ignore_index: at most 8 classes")
        self.stuff_class_inds = [int(i) for i in stuff_class_inds]
        self.thing_class_inds = [int(i) for i in thing_class_inds]
        self.min_num_points = int(min_num_points)
        if int(id_offset) != 2 ** 16:
            raise ValueError("id_offset: the device path ranks shifted instance ids in [0, 2^16); id_offset must be 2^16")
        self.id_offset = int(id_offset)
        self.device = torch.device(device) if device is not None else None
        self._buf = None

    # ---- layout
    @property
    def width(self) -> int:
        C = self.n_classes
        return C * C + 4 * C + 1

    def _views(self, buf):
        C = self.n_classes
        o = C * C
        return dict(confusion=buf[:o], tp=buf[o:o + C], fp=buf[o + C:o + 2 * C], fn=buf[o + 2 * C:o + 3 * C],
                    iou_sum=buf[o + 3 * C:o + 4 * C].view(torch.float64), status=buf[o + 4 * C:o + 4 * C + 1])

    def _buffers(self, device):
        if self._buf is None:
            if self.device is None:
                self.device = device
            self._buf = torch.zeros(self.width, dtype=torch.int64, device=self.device)
        if device != self._buf.device:
            raise RuntimeError(f"SegPanAccumulator: the accumulators live on {self._buf.device}, the scene on {device}")
        return self._views(self._buf)

    # ---- accumulation
    @staticmethod
    def _labels(t, name):
        if not torch.is_tensor(t) or not t.is_cuda:
            where = t.device if torch.is_tensor(t) else type(t).__name__
            raise RuntimeError(f"SegPanAccumulator.add: {name}: expected a tensor on the HIP device, got {where} (no CPU fallback)")
        return t if t.dim() == 1 else t.reshape(-1)

    def add(self, eval_ann, pred) -> None:
        """One scene: `eval_ann` as `eval_ap.eval_ann_info` returns it, `pred` the model's `PointData` (or its dict)."""
        if not isinstance(pred, dict):
            pred = dict(pred.items())
        gt_sem = self._labels(eval_ann["pts_semantic_mask"], "eval_ann.pts_semantic_mask")
        gt_inst = self._labels(eval_ann["pts_instance_mask"], "eval_ann.pts_instance_mask")
        sem = self._labels(pred["pts_semantic_mask"][0], "pts_semantic_mask[0]")
        pan_sem = self._labels(pred["pts_semantic_mask"][1], "pts_semantic_mask[1]")
        pan_inst = self._labels(pred["pts_instance_mask"][1], "pts_instance_mask[1]")
        v = self._buffers(gt_sem.device)
        self.add_semantic(sem, gt_sem, v)
        self.add_panoptic(pan_sem, pan_inst, gt_sem, gt_inst, v)

    def add_semantic(self, pred_sem, gt_sem, views=None) -> None:
        v = views if views is not None else self._buffers(gt_sem.device)
        ops.semantic_confusion(pred_sem, gt_sem, self.n_classes, self.ignore[0] if self.ignore else -1, v["confusion"], v["status"])

    def add_panoptic(self, pred_sem, pred_inst, gt_sem, gt_inst, views=None) -> None:
        v = views if views is not None else self._buffers(gt_sem.device)
        ops.panoptic_accumulate(pred_sem, pred_inst, gt_sem, gt_inst, self.n_classes, self.ignore, self.min_num_points,
                                v["tp"], v["fp"], v["fn"], v["iou_sum"], v["status"])

    # ---- state
    def state(self) -> torch.Tensor:
        if self._buf is None:
            return torch.zeros(self.width, dtype=torch.float64, device=self.device if self.device is not None else "cpu")
        v = self._views(self._buf)
        return torch.cat([v["confusion"].double(), v["tp"].double(), v["fp"].double(), v["fn"].double(), v["iou_sum"],
                          v["status"].double()])

    @staticmethod
    def merge(states) -> torch.Tensor:
        """Sum of state tensors ([width] each, or the [n, width] rows `all_gather_records` returns); status words are OR-ed."""
        rows = torch.cat([s.reshape(-1, s.shape[-1]) for s in states if s.numel() > 0])
        out = rows.sum(dim=0)
        status = 0
        for s in rows[:, -1].tolist():
            status |= int(s)
        out[-1] = float(status)
        return out

    def counts(self, state: Optional[torch.Tensor] = None) -> Dict[str, np.ndarray]:
        """The read-back: the state as host arrays (int64 but iou_sum); raises when the status word is set and names the bits."""
        s = (self.state() if state is None else state).detach().cpu().numpy()
        if s.shape != (self.width,):
            raise ValueError(f"state: expected {self.width} values, got {s.shape}")
        C = self.n_classes
        o = C * C
        status = int(s[-1])
        if status:
            raise RuntimeError(f"SegPanAccumulator: status {status}: " + "; ".join(msg for bit, msg in ops.SEG_EVAL_STATUS if status & bit))
        as_int = lambda a: np.rint(a).astype(np.int64)                                  # noqa: E731
        return dict(confusion=as_int(s[:o]).reshape(C, C), tp=as_int(s[o:o + C]), fp=as_int(s[o + C:o + 2 * C]),
                    fn=as_int(s[o + 2 * C:o + 3 * C]), iou_sum=s[o + 3 * C:o + 4 * C].copy())

    def result(self, classes=None, label2cat=None, state: Optional[torch.Tensor] = None) -> dict:
        """Both metric dictionaries from the accumulated (or a merged) state: `{"seg": ..., "pan": ...}`."""
        c = self.counts(state)
        if label2cat is None:
            names = list(classes) if classes is not None else [str(i) for i in range(self.n_classes)]
            label2cat = {i: n for i, n in enumerate(names)}
        names = [label2cat[i] for i in range(self.n_classes)]
        seg = seg_metrics(c["confusion"], label2cat, self.ignore[0] if self.ignore else -1)
        pan = panoptic_metrics(c["tp"], c["fp"], c["fn"], c["iou_sum"], names, [names[i] for i in self.thing_class_inds],
                               [names[i] for i in self.stuff_class_inds], label2cat, self.ignore)
        return {"seg": seg, "pan": pan}


# ---------------------------------------------------------------------------------------------------- dictionary arithmetic (host, float64)
def seg_metrics(confusion, label2cat, ignore_index) -> dict:
    hist = np.asarray(confusion, dtype=np.float64)
    C = hist.shape[0]
    diag, row, col = np.diag(hist), hist.sum(axis=1), hist.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = diag / (row + col - diag)
        acc_cls = diag / row
        acc = diag.sum() / hist.sum()
    if 0 <= int(ignore_index) < C:
        iou[int(ignore_index)] = np.nan
    nanmean = lambda a: float(np.nanmean(a)) if np.isfinite(a).any() else float("nan")   # noqa: E731
    ret = {label2cat[i]: float(iou[i]) for i in range(C)}
    ret["miou"], ret["acc"], ret["acc_cls"] = nanmean(iou), float(acc), nanmean(acc_cls)
    return ret


def panoptic_metrics(tp, fp, fn, iou_sum, classes, thing_classes, stuff_classes, label2cat, ignore_index) -> dict:
    tp, fp, fn = (np.asarray(a, dtype=np.float64) for a in (tp, fp, fn))
    iou_sum = np.asarray(iou_sum, dtype=np.float64)
    ignored = set(_as_list(ignore_index))
    include = [i for i in range(len(classes)) if i not in ignored]
    sq = iou_sum / np.maximum(tp, 1e-15)
    rq = tp / np.maximum(tp + 0.5 * fp + 0.5 * fn, 1e-15)
    pq = sq * rq
    per = {label2cat[i]: {"pq": float(pq[i]), "sq": float(sq[i]), "rq": float(rq[i])} for i in include}
    mean = lambda vals: float(np.mean(vals)) if len(vals) else 0.0                      # noqa: E731
    ret = {m: mean([per[label2cat[i]][m] for i in include]) for m in ("pq", "sq", "rq")}
    for name, subset in (("thing", thing_classes), ("stuff", stuff_classes)):
        for m in ("pq", "sq", "rq"):
            ret[f"{m}_{name}"] = mean([per[c][m] for c in subset if c in per])
    ret["classes"] = per
    return ret


# ---------------------------------------------------------------------------------------------------- the reference's call shapes
def seg_eval(gt_labels, seg_preds, label2cat, ignore_index, logger=None) -> dict:
    """mmdet3d's `seg_eval(gt_labels, seg_preds, label2cat, ignore_index)` on per-scene device tensors (int64 [N])."""
    acc = SegPanAccumulator(len(label2cat), ignore_index, (), (), 1)
    for gt, pred in zip(gt_labels, seg_preds):
        acc.add_semantic(acc._labels(pred, "seg_preds"), acc._labels(gt, "gt_labels"))
    return seg_metrics(acc.counts()["confusion"], label2cat, acc.ignore[0] if acc.ignore else -1)


def panoptic_seg_eval(gt_labels, seg_preds, classes, thing_classes, stuff_classes, min_num_points, id_offset, label2cat, ignore_index,
                      logger=None) -> dict:
    """mmdet3d's `panoptic_seg_eval`: `gt_labels` / `seg_preds` are per-scene dicts with `pts_semantic_mask` / `pts_instance_mask`
    (device tensors, int64 [N]); `ignore_index` is the list of ignored class indices."""
    acc = SegPanAccumulator(len(classes), ignore_index, (), (), min_num_points, id_offset)
    for gt, pred in zip(gt_labels, seg_preds):
        acc.add_panoptic(acc._labels(pred["pts_semantic_mask"], "seg_preds.pts_semantic_mask"),
                         acc._labels(pred["pts_instance_mask"], "seg_preds.pts_instance_mask"),
                         acc._labels(gt["pts_semantic_mask"], "gt_labels.pts_semantic_mask"),
                         acc._labels(gt["pts_instance_mask"], "gt_labels.pts_instance_mask"))
    c = acc.counts()
    return panoptic_metrics(c["tp"], c["fp"], c["fn"], c["iou_sum"], list(classes), list(thing_classes), list(stuff_classes), label2cat,
                            acc.ignore)


def evaluator_metrics(results, classes, valid_class_ids, thing_class_inds, stuff_class_inds, min_num_points, ignore_index,
                      id_offset: int = 2 ** 16, label2cat=None, options=None, groups=None, return_all: bool = False) -> dict:
    """What the reference's `InstanceSeg3DEvaluator.compute_metrics` (ScanNet branch) would return with its last lines restored:
    `miou`, `all_ap`, `all_ap_50%`, `all_ap_25%`, `pq` (its `logger_keys`).  `results`: per scene `(eval_ann, pred)` with device
    tensors.  The AP part is `eval_ap.evaluator_instance_metrics`, unchanged.  `return_all` adds the three full dictionaries
    under `ret_sem` / `ret_inst` / `ret_pan`."""
    classes = list(classes)
    if label2cat is None:
        label2cat = {i: c for i, c in enumerate(classes)}
    acc = SegPanAccumulator(len(classes), ignore_index, stuff_class_inds, thing_class_inds, min_num_points, id_offset)
    for ann, pred in results:
        acc.add(ann, pred)
    ret_inst = evaluator_instance_metrics(results, classes, valid_class_ids, len(list(stuff_class_inds)), options=options, groups=groups)
    r = acc.result(label2cat=label2cat)
    metrics = {"miou": r["seg"]["miou"]}
    for k in ("all_ap", "all_ap_50%", "all_ap_25%"):
        metrics[k] = ret_inst[k]
    metrics["pq"] = r["pan"]["pq"]
    if return_all:
        metrics.update(ret_sem=r["seg"], ret_inst=ret_inst, ret_pan=r["pan"])
    return metrics
