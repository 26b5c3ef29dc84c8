"""Dataset targets on the device: raw per-point labels -> the fields the model, the criterion and the evaluator read.

The label side of the reference's `Dataset.__getitem__` (`segdino3d/datasets/dataset/scannet200.py:155-193, 198-289, 291-326`,
`scannet.py` likewise, and `datasets/preparer/instance_seg_3d_preparer.py`), in the reference's order:
  1. semantic ids: `sem = LUT[swap(sem_raw)]` (`adjust_class_ids_`; the 2 <-> 3 swap is ScanNet200's);
  2. `exclude_stuffs_`: points whose class is a stuff id or the background class get instance -1, then every point gets
     `new id = rank of its id among the scene's distinct ids - 1` - one rule that reproduces the reference including its quirk:
     with no background point in the scene the smallest instance id becomes -1;
  3. superpoint votes (`:243-253`): an instance / a class owns a superpoint iff MORE THAN HALF of its points carry it, decided in
     integers (`2 k > n`, equal to the reference's fp32 `scatter_mean(...) > 0.5` for superpoints below 2^22 points); a superpoint
     without an owning class gets the background class;
  4. instances (`split_instance_gt` + the preparer): one mask row per id >= 0 in ascending order, `area` = its point count,
     category = the class at its lowest point index; train view: `labels = category - len(stuff_ids)`; val view
     (`merge_stuffs_`): the votes are taken first, then every present stuff class becomes one instance in front of the others
     and categories are not shifted.  (`instance_sp_mask` of the reference is dead code and is not built.)
  5. 2D-query dropout (`:227-232`): `drop_2d_queries`.
All arithmetic runs in `csrc/targets.hip`; there is no host label arithmetic and no CPU path.

Synchronisation: the number of instances G, of superpoints S and the range status decide the sizes of the outputs, so
`build_targets` reads 16 bytes back from the device - ONE read-back per scene, the only synchronisation in the feature.  Inside
`io_scene.ScenePrefetcher` it happens on the copy stream in a reader thread, `depth` scenes ahead of the consumer, which never
waits for it.
"""
from __future__ import annotations

import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from .gtypes import GD3DTarget


class LabelSpec:
    """What turns a dataset's raw labels into classes: `n_classes` C (`bg_class_id` = C), the stuff class ids, the int64
    lookup table `seg_label_mapping` (raw semantic id -> class in 0..C) and whether raw ids 2 and 3 are swapped first.
    `dataset_type` / `loss_branch` are the strings the reference's dataset classes put on every target."""

    def __init__(self, n_classes: int, seg_label_mapping, stuff_ids: Sequence[int] = (0, 1), swap_2_3: bool = False,
                 dataset_type: str = "", loss_branch: Optional[str] = None):
        lut = torch.as_tensor(np.asarray(seg_label_mapping.cpu() if torch.is_tensor(seg_label_mapping) else seg_label_mapping)).reshape(-1)
        if lut.dtype not in (torch.int64, torch.int32, torch.int16, torch.uint8, torch.int8) or lut.numel() == 0:
            raise TypeError("seg_label_mapping: expected a non-empty integer table")
        lut = lut.to(torch.int64).contiguous().clone()
        self.n_classes = int(n_classes)
        if int(lut.min()) < 0 or int(lut.max()) > self.n_classes:
            raise ValueError(f"seg_label_mapping: classes must lie in [0, {self.n_classes}]")
        self.stuff_ids = tuple(int(s) for s in stuff_ids)
        if list(self.stuff_ids) != sorted(set(self.stuff_ids)) or any(s < 0 or s >= self.n_classes for s in self.stuff_ids) or len(self.stuff_ids) > 8:
            raise ValueError("stuff_ids: at most 8 ascending class ids below n_classes")
        self.seg_label_mapping = lut
        self.swap_2_3 = bool(swap_2_3)
        self.dataset_type = dataset_type
        self.loss_branch = loss_branch
        self._dev = {}

    @property
    def bg_class_id(self) -> int:
        return self.n_classes

    @classmethod
    def scannet200(cls, seg_label_mapping) -> "LabelSpec":
        """ScanNet200 (`scannet200.py:60-63`): 200 classes, stuff = (0, 1), raw ids 2 and 3 swapped before the lookup.
        `seg_label_mapping`: the table as a tensor or an array, or the path of its `.npy` (the reference loads
        `scannet200_seg_label_mapping.npy` from the working directory)."""
        if isinstance(seg_label_mapping, (str, os.PathLike)):
            seg_label_mapping = np.load(seg_label_mapping, allow_pickle=False)
        return cls(200, seg_label_mapping, (0, 1), True, "scannet200_InstanceSeg3D", "cdn")

    @classmethod
    def scannet(cls, valid_cat_ids: Sequence[int]) -> "LabelSpec":
        """ScanNetv2 (`scannet.py:73-82`): 20 classes; the 42-entry table maps the 20 valid raw category ids, in the order
        given, to 0..19 and everything else to the background class."""
        valid = [int(v) for v in valid_cat_ids]
        if len(valid) != 20 or any(v < 0 or v > 41 for v in valid):
            raise ValueError("scannet: expected the 20 valid raw category ids (each in 0..41)")
        lut = np.full(42, 20, dtype=np.int64)
        lut[valid] = np.arange(20)
        return cls(20, lut, (0, 1), False, "scannet_train_mask3d", None)

    def table(self, device) -> torch.Tensor:
        device = torch.device(device)
        t = self._dev.get(device)
        if t is None:
            t = self._dev[device] = self.seg_label_mapping.to(device)
        return t


def build_targets(instance_mask: torch.Tensor, semantic_mask: torch.Tensor, super_points: torch.Tensor, spec: LabelSpec,
                  scene_set: str, target: Optional[GD3DTarget] = None, scene_id=None, index: int = 0) -> GD3DTarget:
    """Raw label arrays (int64 [N], on the device) -> the reference's target fields on `target` (a new `GD3DTarget` when None):
    `masks` bool [G, N, 1], `labels` / `area` / `iscrowd` int64 [G], `sp_inst_sem_masks` bool [G' + C + 1, S] (instance rows of
    the train numbering first, then the classes), `orig_size` / `size` ([N], host tensors as the preparer makes them),
    `scene_id`, `data_source`, `loss_branch` (only when the spec has one) and `prompt_type`.  `scene_set` "train" gives the
    train view, anything else ("val", "test") the val view with merged stuff instances.  G = 0 gives empty tensors.
    Costs one 16-byte read-back (see the module docstring); an out-of-range raw id raises and names the status."""
    if scene_set not in ("train", "val", "test"):
        raise ValueError(f"Invalid scene set: {scene_set}")
    N = instance_mask.numel()
    for name, t in (("instance_mask", instance_mask), ("semantic_mask", semantic_mask), ("super_points", super_points)):
        if not t.is_cuda:
            raise RuntimeError(f"build_targets: {name}: expected a tensor on the HIP device, got {t.device} (no CPU fallback)")
    ws, header = ops.targets_scan(instance_mask.reshape(-1), semantic_mask.reshape(-1), super_points.reshape(-1),
                                  spec.table(instance_mask.device), spec.n_classes, spec.stuff_ids, spec.swap_2_3)
    r = ops.targets_build(ws, header.wait(), N, spec.n_classes, spec.stuff_ids, val_view=scene_set != "train")
    tgt = GD3DTarget() if target is None else target
    tgt["masks"] = r["masks"].view(torch.bool).unsqueeze(-1)
    tgt["labels"], tgt["area"] = r["labels"], r["area"]
    tgt["iscrowd"] = torch.zeros_like(r["labels"])
    tgt["sp_inst_sem_masks"] = r["sp_masks"].view(torch.bool)
    tgt["orig_size"], tgt["size"] = torch.as_tensor([int(N)]), torch.as_tensor([int(N)])
    tgt["scene_id"] = scene_id if scene_id is not None else tgt.get("scene_id")
    tgt["data_source"] = f"{spec.dataset_type}:{index}"
    if spec.loss_branch is not None:
        tgt["loss_branch"] = spec.loss_branch
    tgt["prompt_type"] = "text"
    return tgt


def drop_2d_queries(target, rate: float, seed_module=np.random):
    """2D-query dropout of the training datasets (`scannet200.py:227-232`, `dropout_rate_2dfeats`): keeps
    `int(M * (1 - rate))` of the M 2D queries, drawn by `seed_module.choice(M, n, replace=False)` on the host - the
    reference's call on the caller's generator, hence its stream - and indexes `query2d_feats` / `query2d_pos` on the device.
    The index tensor is staged in pinned memory and copied asynchronously (a pageable copy would block the host until the
    stream has drained).  Returns the kept indices (host array)."""
    if not rate > 0.0:
        return None
    ef = target["extra_features"]
    pos, feats = ef["query2d_pos"], ef["query2d_feats"]
    if not pos.is_cuda:
        raise RuntimeError(f"drop_2d_queries: expected tensors on the HIP device, got {pos.device} (no CPU fallback)")
    num_query = pos.shape[0]
    num_sample = int(num_query * (1 - rate))
    sample_idx = seed_module.choice(num_query, num_sample, replace=False)
    idx = torch.from_numpy(np.ascontiguousarray(sample_idx, dtype=np.int64)).pin_memory().to(pos.device, non_blocking=True)
    ef["query2d_pos"] = pos[idx]
    ef["query2d_feats"] = feats[idx]
    return sample_idx
