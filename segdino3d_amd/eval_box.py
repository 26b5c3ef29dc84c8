"""3D box AP / AR of `instance_boxes`, the one output of a forward that nothing scored, accumulated and scored on the device
(csrc/boxeval.hip).

The protocol is the VOC-style indoor detection protocol that mmdet3d's `indoor_eval` implements, for axis-aligned boxes, per class
`c` and IoU threshold `t` (include/segdino3d_hip.h states it in full; tests/box_ap_ref.py restates it in numpy):

  * ground truth = the min / max corner box of every thing instance of a scene (instances and classes read exactly as
    `ApAccumulator` reads them; one point is enough, there is no `min_region`), `npos[c]` = their number over all scenes;
  * IoU in float64 from the fp32 values, prediction corners `centre -+ size / 2`;
  * within a scene, the predictions of a class in (score descending, row ascending) order each take the ground truth of their class
    with the largest IoU (lowest instance column on equal IoU): a true positive when that IoU is > t and the ground truth is still
    free at t, a false positive otherwise - no second choice;
  * the curve of (c, t) over the entries of all scenes in descending score; AP is the "area" form (precision envelope), AR the last
    recall.

Two differences from mmdet3d, both where it leaves the result undefined:

  * among EQUAL scores true positives come before false positives (mmdet3d leaves the order to an unstable `argsort`), which makes the
    tables independent of scene and rank order;
  * a class without ground truth anywhere is NaN and is left out of `mAP_t` / `mAR_t` (mmdet3d divides by `npos = 0` and poisons its
    mean); a class with ground truth but no prediction is 0 and counts.

The sequential walk is not sequential on the device: a prediction's best ground truth depends on neither the threshold nor the taken
flags, so `(jmax, iou_max)` is computed for all predictions in parallel, and the true positive of (ground truth j, t) is the first
prediction in walk order among those with `jmax == j` and `iou_max > t` - a minimum over a 64-bit key, then a compare."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops
from .eval_ap import ApAccumulator


class BoxApAccumulator(ApAccumulator):
    """Box AP / AR over any number of scenes; the surface and rules of `ApAccumulator`: device tensors only, fp32 scores (fp16 / bf16
    are widened), one accumulator per stream, a store that grows in chunks (`max_slots` caps it), `state()` / `merge` in the
    [R, 1024] float64 row format of `dist_eval.all_gather_records`, one read-back in `tables()`.

    `add(eval_ann, pred, points)` only enqueues: `ops.gt_boxes` (ground-truth boxes from the points, `map_inst_markup` applied inside
    the kernel) and `ops.box_ap_scene` (one entry per prediction and threshold into the device-resident store, `npos` / `has_pred`
    into device counters).  `pred_boxes="head"` scores `pred["instance_boxes"]` [n, 6] (centre, size), the output of the box heads;
    `pred_boxes="masks"` scores the boxes of the predicted masks, `ops.instance_boxes(points, pred["pts_instance_mask"][0],
    "median")` - for models without a box head (the `Baseline_ScanNet200` prototype returns zeros there).
    `add_boxes(gt_corners, gt_classes, boxes, labels, scores)` takes ground-truth corner boxes [G, 6] (min xyz, max xyz) with class
    indices [G] (-1 = none), G <= 1000, from the caller.  At most `ops.AP_MAX_PREDS` predictions per scene.
    Counter rows of the state: npos [C], has_pred [C]."""

    def __init__(self, valid_class_ids, class_labels, iou_thr=(0.25, 0.5), num_stuff_cls: int = 0, pred_boxes: str = "head", device=None):
        if pred_boxes not in ("head", "masks"):
            raise ValueError("pred_boxes: 'head' (pred['instance_boxes']) or 'masks' (boxes of pred['pts_instance_mask'][0])")
        thr = np.ascontiguousarray(iou_thr, dtype=np.float64).reshape(-1)
        if not 1 <= len(thr) <= 16 or not np.all((thr > 0.0) & (thr < 1.0)):
            raise ValueError("iou_thr: 1..16 thresholds, each in (0, 1)")
        super().__init__(valid_class_ids, class_labels, options=dict(overlaps=thr), num_stuff_cls=num_stuff_cls, groups={}, device=device)
        self.iou_thr = tuple(float(t) for t in thr)
        self.pred_boxes = pred_boxes
        self.slots = [1] * self.n_overlaps                       # one entry per prediction and threshold
        self.slots_per_pred = self.n_overlaps

    # ---- layout
    @property
    def n_counters(self) -> int:
        return 2 * self.n_classes

    def _views(self, buf):
        C = self.n_classes
        return dict(npos=buf[:C], has_pred=buf[C:2 * C], status=buf[2 * C:])

    # ---- accumulation
    def add(self, eval_ann, pred, points) -> None:
        """One scene as the evaluator collects it: `eval_ann` = dict(pts_semantic_mask, pts_instance_mask) before `map_inst_markup`,
        `pred` the model's `PointData` (or its dict) with `model.to_host = False`, `points` fp32 [N, >= 3] (x, y, z first)."""
        if not isinstance(pred, dict):
            pred = dict(pred.items())
        points = self._on_device(points, "points")
        gt_sem, gt_inst = self._on_device(eval_ann["pts_semantic_mask"], "gt_sem"), self._on_device(eval_ann["pts_instance_mask"], "gt_inst")
        as_ids = lambda t: (t if t.dim() == 1 else t.reshape(-1)).long()              # noqa: E731
        gt_sem, gt_inst = as_ids(gt_sem), as_ids(gt_inst)
        if points.dtype != torch.float32 or points.dim() != 2:
            raise TypeError("BoxApAccumulator: points must be fp32 [N, >= 3]")
        v = self._buffers(points.device)
        corners, cls = ops.gt_boxes(points, gt_sem, gt_inst, self._const["lut"], self.n_classes, v["status"], id_map=self._const["id_map"],
                                    num_stuff=self.num_stuff_cls)
        if self.pred_boxes == "head":
            boxes = self._on_device(pred["instance_boxes"], "instance_boxes")
        else:
            masks = self._on_device(pred["pts_instance_mask"][0], "masks")
            if masks.dtype != torch.bool or masks.dim() != 2 or masks.shape[1] != points.shape[0]:
                raise TypeError("BoxApAccumulator: pred_boxes='masks' needs bool masks [n, N]")
            boxes = torch.cat(ops.instance_boxes(points, masks, "median"), dim=1)
        self._add_boxes(corners, cls, boxes, pred["instance_labels"], pred["instance_scores"])

    def add_boxes(self, gt_corners, gt_classes, boxes, labels, scores) -> None:
        """One scene from boxes the caller has: gt_corners fp32 [G, 6] (min xyz, max xyz), gt_classes integer class indices [G]
        (-1 = no ground truth), boxes fp32 [n, 6] (centre, size), labels [n] class indices, scores [n]."""
        gt_corners, gt_classes = self._on_device(gt_corners, "gt_corners"), self._on_device(gt_classes, "gt_classes")
        if gt_classes.is_floating_point() or gt_classes.dtype == torch.bool:
            raise TypeError(f"BoxApAccumulator: gt_classes must be integer class indices, got {gt_classes.dtype}")
        self._buffers(gt_corners.device)
        self._add_boxes(gt_corners, gt_classes.reshape(-1).int(), boxes, labels, scores)

    def _add_boxes(self, gt_corners, gt_cls, boxes, labels, scores) -> None:
        boxes, labels, scores = self._on_device(boxes, "boxes"), self._on_device(labels, "labels"), self._on_device(scores, "scores")
        if scores.dtype == torch.float64:
            raise TypeError("BoxApAccumulator: float64 scores: the sort key holds the 32 bits of an fp32 score")
        if scores.dtype in (torch.float16, torch.bfloat16):
            scores = scores.float()                                                  # exact
        if scores.dtype != torch.float32:
            raise TypeError(f"BoxApAccumulator: scores must be fp32 (fp16 / bf16 are widened), got {scores.dtype}")
        if labels.is_floating_point() or labels.dtype == torch.bool:
            raise TypeError(f"BoxApAccumulator: labels must be integer class indices, got {labels.dtype}")
        if boxes.dtype != torch.float32 or gt_corners.dtype != torch.float32:
            raise TypeError("BoxApAccumulator: boxes and ground-truth corners must be fp32")
        labels, scores = labels.detach().reshape(-1).long().contiguous(), scores.detach().reshape(-1).contiguous()
        boxes, gt_corners = boxes.detach().reshape(-1, 6).contiguous(), gt_corners.detach().reshape(-1, 6).contiguous()
        v = self._views(self._counters)
        n = labels.numel()
        need = n * self.slots_per_pred
        room = self._reserve(need)
        ops.box_ap_scene(boxes, labels, scores, gt_corners, gt_cls.contiguous(), self.n_classes, self._const["overlaps"], self._store, self.used,
                         room, v["npos"], v["has_pred"], v["status"])
        self.used += room

    def add_scene(self, *a, **kw):
        raise NotImplementedError("BoxApAccumulator: use add(eval_ann, pred, points) or add_boxes(...)")

    # ---- read-back
    def _raise_on(self, status: int):
        if status:
            raise RuntimeError(f"BoxApAccumulator: status {status}: " + "; ".join(msg for bit, msg in ops.BOX_AP_STATUS if status & bit))

    def tables(self, state: Optional[torch.Tensor] = None):
        """The read-back: `(ap [C, T], ar [C, T])` float64 from this accumulator or a merged state; NaN for a class without ground
        truth; raises when the status word is set and names the bits."""
        C, T = self.n_classes, self.n_overlaps
        codes, counters, status = self._parse(state)
        self._raise_on(status)
        dev = self.device if self.device is not None and self.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
        codes, counters = codes.to(dev).contiguous(), counters.to(dev)
        ap, ar = ops.box_ap_finish(codes, C, T, counters[:C].contiguous())
        out = torch.stack([ap, ar]).cpu().numpy()
        return out[0].reshape(C, T).copy(), out[1].reshape(C, T).copy()

    def result(self, state: Optional[torch.Tensor] = None) -> dict:
        """The metrics dictionary with mmdet3d's key shapes: `{class}_AP_{t:.2f}`, `{class}_rec_{t:.2f}`, `mAP_{t:.2f}`,
        `mAR_{t:.2f}`; the means run over the classes with ground truth (NaN when there is none)."""
        return metrics_dict(*self.tables(state), self.class_labels, self.iou_thr)

    def entries(self, state: Optional[torch.Tensor] = None) -> dict:
        """Read-back for tests and debugging: the entries sorted by (group, score, true) - `group` = class * T + threshold - with
        npos [C], has_pred [C] and the status word (no raise)."""
        C, T = self.n_classes, self.n_overlaps
        codes, counters, status = self._parse(state)
        counters = counters.cpu().numpy()
        group, score, true = self._decode(codes.cpu().numpy(), C * T)
        return dict(group=group, score=score, true=true, npos=counters[:C].copy(), has_pred=counters[C:2 * C] > 0, status=status)


def metrics_dict(ap, ar, class_labels, iou_thr) -> dict:
    out = {}
    for o, t in enumerate(iou_thr):
        for c, name in enumerate(class_labels):
            out[f"{name}_AP_{t:.2f}"] = float(ap[c, o])
            out[f"{name}_rec_{t:.2f}"] = float(ar[c, o])
        have = ~np.isnan(ap[:, o])
        out[f"mAP_{t:.2f}"] = float(ap[have, o].mean()) if have.any() else float("nan")
        out[f"mAR_{t:.2f}"] = float(ar[have, o].mean()) if have.any() else float("nan")
    return out


def evaluator_box_metrics(results, points, classes, valid_class_ids, num_stuff_cls: int, iou_thr=(0.25, 0.5), pred_boxes: str = "head"):
    """The list-of-results form, next to `eval_ap.evaluator_instance_metrics` and `eval_seg.evaluator_metrics`: `results` = per scene
    `(eval_ann, pred)` as the evaluator collects them, `points` = the scenes' point tensors in the same order, `classes` /
    `valid_class_ids` the dataset's (stuff first, `classes` with the trailing "unlabeled").  Returns `BoxApAccumulator.result()`."""
    results, points = list(results), list(points)
    if len(results) != len(points):
        raise ValueError("evaluator_box_metrics: one point tensor per result")
    acc = BoxApAccumulator(tuple(int(v) for v in valid_class_ids[num_stuff_cls:]), tuple(classes[num_stuff_cls:-1]), iou_thr=iou_thr,
                           num_stuff_cls=num_stuff_cls, pred_boxes=pred_boxes)
    for (ann, pred), pts in zip(results, points):
        acc.add(ann, pred, pts)
    return acc.result()
