"""ScanNet instance AP per scene on the device: `InstanceSeg3DEvaluator.compute_each_sample_metrics`
(evaluation/evaluator_3d.py:227-321), which runs `instance_seg_eval` on one scene at a time and returns {lidar_idx: metrics}.

`SceneApAccumulator` is an `eval_ap.ApAccumulator` whose counters are kept per scene: scene s writes row s of a
[S_cap, C * O + 2 * C] int64 buffer through the unchanged `ops.ap_scene`, and owns the slots [off[s], off[s + 1]) of the entry store,
offsets the host knows.  `scene_tables()` scores every (scene, class, overlap) group in one pass (`ops.ap_finish_scenes`,
csrc/apeval_scene.hip) and is the one read-back; `tables()` / `result()` are the global metrics from the same accumulator
(`ops.ap_reduce_counters` + the existing `ops.ap_finish`), bit for bit those of an `ApAccumulator` fed the same scenes."""
from typing import Dict, Optional

import numpy as np
import torch

from . import ops
from .eval_ap import ApAccumulator, compute_averages

MAX_SCENE_KEY = 1 << 31


def _overlap_mask(overlaps, value: float) -> int:
    """Bit o set where overlap o is `value`, by `np.isclose` as `compute_averages` selects its columns."""
    return int(sum(1 << int(o) for o in np.flatnonzero(np.isclose(overlaps, value))))


def _to(a: np.ndarray, dev) -> torch.Tensor:
    """A host array on `dev` without a blocking copy."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if torch.device(dev).type != "cuda" or t.numel() == 0:
        return t.to(dev)
    return t.pin_memory().to(dev, non_blocking=True)


class SceneApAccumulator(ApAccumulator):
    """`ApAccumulator` with per-scene tables.  Same constructor; `add(eval_ann, pred, scene_key)` and
    `add_scene(gt_sem, gt_inst, masks, labels, scores, scene_key)` take an integer key 0 <= key < 2^31 the caller chooses (the index
    in the split list, say); a repeated key raises `ValueError`.  Both only enqueue - no read-back, no synchronisation - so `add`
    can be the `on_result` consumer of a `dist_eval.PipelinedRunner`.  The counter rows are zero-filled and grown on the host by
    doubling (a device copy); the status word stays one word for all scenes.

    `scene_tables()` -> `(keys [S], ap [S, C, O], pr_rc [2, S, C, O], summary [S, 5])`, scenes in ascending key order, the
    columns of `summary` being all_ap, all_ap_50%, all_ap_25%, all_prec_50%, all_rec_50%.  `scene_results(names)` is the
    dictionary `compute_each_sample_metrics` returns.  S * (C * O + 1) must stay below 2^30 (`ops.AP_SCENE_KEY_LIMIT`): the scene
    shares the 63-bit sort key with the group and the score, inside the finish call only - the store and the state keep the codes
    of `ApAccumulator`, below 2^53.

    State (`state()`, float64 [R, STATE_WIDTH], rows in any order and number, the payload of `dist_eval.all_gather_records`):
    column 0 names the kind - 3: the status word; 4: counters of one scene (column 1 = scene key, 2 = chunk index, 3 = the scene's
    slot count, then the chunk of hard_fn [C, O], has_gt [C], has_pred [C]); 5: entry codes of one scene (column 1 = scene key,
    then codes, -1 = no entry).  `merge` raises on a key that two states hold."""

    COUNTER_ROWS = 16                     # scene rows the counter buffer starts with; it doubles

    def __init__(self, valid_class_ids, class_labels, options: Optional[dict] = None, num_stuff_cls: int = 0, groups=None, device=None):
        self._keys = []                   # scene keys in the order of the adds; scene s owns row s and the slots [offsets[s], offsets[s + 1])
        self._seen = set()
        self._offsets = [0]
        self._scene_rows = None
        self._status = None
        super().__init__(valid_class_ids, class_labels, options=options, num_stuff_cls=num_stuff_cls, groups=groups, device=device)
        overlaps = np.asarray(self.options["overlaps"], dtype=np.float64).reshape(-1)
        self.mask50, self.mask25 = _overlap_mask(overlaps, 0.5), _overlap_mask(overlaps, 0.25)

    # ---- layout
    def _buffers(self, device):
        """The counter views of the NEXT scene (row len(keys)) for `ops.ap_scene`."""
        C, G = self.n_classes, self.n_classes * self.n_overlaps
        if self._scene_rows is None:
            if self.device is None:
                self.device = device
            self._const = {k: (v.pin_memory() if torch.cuda.is_available() else v).to(self.device, non_blocking=True)
                           for k, v in self._host.items()}
            self._scene_rows = torch.zeros(self.COUNTER_ROWS, self.n_counters, dtype=torch.int64, device=self.device)
            self._status = torch.zeros(1, dtype=torch.int64, device=self.device)
            self._store = torch.empty(0, dtype=torch.int64, device=self.device)
        if device != self._scene_rows.device:
            raise RuntimeError(f"SceneApAccumulator: the accumulators live on {self._scene_rows.device}, the scene on {device}")
        s, cap = len(self._keys), self._scene_rows.shape[0]
        if s >= cap:
            grown = torch.zeros(2 * cap, self.n_counters, dtype=torch.int64, device=self.device)
            grown[:cap].copy_(self._scene_rows)
            self._scene_rows = grown
        row = self._scene_rows[s]
        return dict(hard_fn=row[:G], has_gt=row[G:G + C], has_pred=row[G + C:], status=self._status)

    # ---- accumulation
    def _check_key(self, scene_key) -> int:
        if isinstance(scene_key, bool) or not isinstance(scene_key, (int, np.integer)):
            raise ValueError(f"scene_key: an integer 0 <= key < 2^31, got {scene_key!r}")
        key = int(scene_key)
        if not 0 <= key < MAX_SCENE_KEY:
            raise ValueError(f"scene_key: an integer 0 <= key < 2^31, got {key}")
        if key in self._seen:
            raise ValueError(f"scene_key {key} was added before")
        return key

    def _record(self, key: int) -> None:
        self._keys.append(key)
        self._seen.add(key)
        self._offsets.append(self.used)

    def add(self, eval_ann, pred, scene_key: int) -> None:
        key = self._check_key(scene_key)
        super().add(eval_ann, pred)
        self._record(key)

    def add_scene(self, gt_sem, gt_inst, masks, labels, scores, scene_key: int) -> None:
        key = self._check_key(scene_key)
        super().add_scene(gt_sem, gt_inst, masks, labels, scores)
        self._record(key)

    # ---- state
    @classmethod
    def _pack(cls, keys, offsets, counters, codes, status) -> torch.Tensor:
        """The state rows of scenes `keys` (host) with slots `offsets` (host, [S + 1]) of `codes` int64, `counters` int64 [S, n]
        and `status` int64 [1], on the tensors' device, without a read-back."""
        W, dev = cls.STATE_WIDTH, counters.device
        S, n = len(keys), counters.shape[1]
        keys, offsets = np.asarray(keys, dtype=np.int64).reshape(-1), np.asarray(offsets, dtype=np.int64).reshape(-1)
        counts = np.diff(offsets)
        srow = torch.cat([torch.full((1, 1), 3.0, dtype=torch.float64, device=dev), status.double().reshape(1, 1),
                          torch.zeros(1, W - 2, dtype=torch.float64, device=dev)], dim=1)
        pc = W - 4
        nch = -(-n // pc)
        body = torch.cat([counters[:S].double(), torch.zeros(S, nch * pc - n, dtype=torch.float64, device=dev)], dim=1).reshape(S * nch, pc)
        head = np.stack([np.full(S * nch, 4.0), np.repeat(keys, nch).astype(np.float64), np.tile(np.arange(nch, dtype=np.float64), S),
                         np.repeat(counts, nch).astype(np.float64)], axis=1)
        crow = torch.cat([_to(head, dev), body], dim=1)
        pe = W - 2
        rows_per = -(-counts // pe)
        first_row = np.concatenate([[0], np.cumsum(rows_per)])
        idx = np.full(int(first_row[-1]) * pe, -1, dtype=np.int64)
        for s in range(S):
            idx[first_row[s] * pe:first_row[s] * pe + counts[s]] = np.arange(offsets[s], offsets[s + 1])
        if len(idx):
            idx_t = _to(idx, dev)
            picked = codes[idx_t.clamp(min=0)].double()
            body = torch.where(idx_t >= 0, picked, torch.full_like(picked, -1.0)).reshape(-1, pe)
        else:
            body = torch.zeros(0, pe, dtype=torch.float64, device=dev)
        head = np.stack([np.full(len(idx) // pe, 5.0), np.repeat(keys, rows_per).astype(np.float64)], axis=1)
        erow = torch.cat([_to(head, dev), body], dim=1)
        return torch.cat([srow, crow, erow], dim=0)

    def state(self) -> torch.Tensor:
        S = len(self._keys)
        if self._scene_rows is None:                                                  # no scene yet: nothing lives on a device
            dev = self.device if self.device is not None else torch.device("cpu")
            return self._pack([], [0], torch.zeros(0, self.n_counters, dtype=torch.int64, device=dev),
                              torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
        return self._pack(self._keys, self._offsets, self._scene_rows[:S], self._store[:self.used], self._status)

    @staticmethod
    def _gather_rows(states):
        states = [s for s in states if s.numel() > 0]
        dev = next((s.device for s in states if s.is_cuda), states[0].device)
        rows = torch.cat([s.reshape(-1, s.shape[-1]).to(dev) for s in states])
        return rows, rows[:, :4].cpu().numpy()                                        # the small read of the row headers

    @staticmethod
    def _scene_index(head, n_chunks: Optional[int] = None):
        """(ascending keys [S], rows of kind 4, their (scene, chunk)) from the row headers; raises on a (key, chunk) present twice."""
        h4 = np.flatnonzero(head[:, 0] == 4)
        keys4, chunk = head[h4, 1].astype(np.int64), head[h4, 2].astype(np.int64)
        keys = np.unique(keys4)
        scene = np.searchsorted(keys, keys4)
        if len(chunk) and chunk.min() < 0:
            raise ValueError("state: a counter row with a negative chunk index")
        width = int(chunk.max()) + 1 if len(chunk) else 1
        pairs = scene * width + chunk
        twice = np.flatnonzero(np.bincount(pairs) > 1) if len(pairs) else pairs
        if len(twice):
            raise ValueError(f"SceneApAccumulator: scene key {int(keys[twice[0] // width])} is present in two states")
        if n_chunks is not None and (len(pairs) != len(keys) * n_chunks or (len(chunk) and chunk.max() >= n_chunks)):
            raise ValueError("state: the counter rows do not belong to an accumulator of this shape")
        return keys, h4, scene, chunk

    @classmethod
    def merge(cls, states) -> torch.Tensor:
        """One state from several ([R, W] each, or the per-rank tensors `all_gather_records` returns): the rows of all scenes, the
        status words OR-ed; raises `ValueError` on a scene key that two states hold."""
        rows, head = cls._gather_rows(states)
        cls._scene_index(head)
        status = 0
        for s in head[head[:, 0] == 3][:, 1].tolist():
            status |= int(s)
        srow = torch.zeros(1, rows.shape[1], dtype=rows.dtype, device=rows.device)
        srow[0, 0], srow[0, 1] = 3.0, float(status)
        keep = np.flatnonzero(head[:, 0] != 3)
        return torch.cat([srow, rows[_to(keep, rows.device)]], dim=0)

    def _parse_scenes(self, state):
        """(keys [S] ascending, slot offsets [S + 1], codes int64 with the sentinel where there is no entry, counters int64 [S, n],
        status) from a state: keys and offsets on the host, codes and counters on the state's device."""
        W, n = self.STATE_WIDTH, self.n_counters
        if state.dim() != 2 or state.shape[1] != W:
            raise ValueError(f"state: expected [R, {W}], got {tuple(state.shape)}")
        rows, head = self._gather_rows([state])
        dev = rows.device
        pc, pe = W - 4, W - 2
        nch = -(-n // pc)
        keys, h4, scene, chunk = self._scene_index(head, nch)
        S = len(keys)
        status = 0
        for s in head[head[:, 0] == 3][:, 1].tolist():
            status |= int(s)
        counters = torch.zeros(S * nch, pc, dtype=torch.float64, device=dev)
        if len(h4):
            counters[_to(scene * nch + chunk, dev)] = rows[_to(h4, dev)][:, 4:]
        counters = counters.reshape(S, nch * pc)[:, :n].round().long().contiguous()
        h5 = np.flatnonzero(head[:, 0] == 5)
        keys5 = head[h5, 1].astype(np.int64)
        scene5 = np.minimum(np.searchsorted(keys, keys5), max(S - 1, 0))
        if len(h5) and (S == 0 or np.any(keys[scene5] != keys5)):
            raise ValueError("state: entry rows of a scene without counter rows")
        order = np.argsort(scene5, kind="stable")
        offsets = np.concatenate([[0], np.cumsum(np.bincount(scene5, minlength=S) * pe)]).astype(np.int64)
        if len(h5):
            codes = rows[_to(h5[order], dev)][:, 2:].reshape(-1)
            codes = torch.where(codes < 0, torch.full_like(codes, float(self.sentinel)), codes).long()
        else:
            codes = torch.zeros(0, dtype=torch.int64, device=dev)
        return keys, offsets, codes, counters, status

    def _cuda(self):
        return self.device if self.device is not None and self.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())

    def _parse(self, state):
        """What `ApAccumulator` parses from its state - (codes, counters [C O + 2 C], status) - from the per-scene rows: the
        global `tables()`, `result()` and `entries()` are the parent's on these."""
        dev = self._cuda()
        if state is None:
            S = len(self._keys)
            if self._scene_rows is None:
                counters, codes, status = torch.zeros(0, self.n_counters, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), 0
            else:
                counters, codes, status = self._scene_rows[:S], self._store[:self.used].clone(), int(self._status[0])
        else:
            _, _, codes, counters, status = self._parse_scenes(state)
        return codes.to(dev), ops.ap_reduce_counters(counters.to(dev).contiguous(), self.n_classes, self.n_overlaps), status

    # ---- per-scene tables
    def scene_tables(self, state: Optional[torch.Tensor] = None):
        """`(keys [S] int64, ap [S, C, O], pr_rc [2, S, C, O], summary [S, 5])`, numpy float64, scenes in ascending key order, from
        this accumulator (one read-back) or a merged state (one more small read, of the row headers); raises when the status
        word is set."""
        C, O = self.n_classes, self.n_overlaps
        if state is None:
            keys = np.asarray(self._keys, dtype=np.int64)
            offsets, status = np.asarray(self._offsets, dtype=np.int64), None
            if len(keys):
                codes, counters = self._store[:self.used], self._scene_rows[:len(keys)]
        else:
            keys, offsets, codes, counters, status = self._parse_scenes(state)
            self._raise_on(status)
        S = len(keys)
        if S == 0:
            if state is None and self._status is not None:
                self._raise_on(int(self._status[0]))
            return keys, np.zeros((0, C, O)), np.zeros((2, 0, C, O)), np.zeros((0, 5))
        dev = self._cuda()
        ap, pr_rc, summary = ops.ap_finish_scenes(codes.to(dev).contiguous(), offsets, C, O, counters.to(dev).contiguous(), self.mask50, self.mask25)
        parts = [ap.reshape(-1), pr_rc.reshape(-1), summary.reshape(-1)]
        if status is None:
            parts.append(self._status.double())
        out = torch.cat(parts).cpu().numpy()
        if status is None:
            self._raise_on(int(out[-1]))
        G = S * C * O
        ap, pr_rc, summary = out[:G].reshape(S, C, O), out[G:3 * G].reshape(2, S, C, O), out[3 * G:3 * G + 5 * S].reshape(S, 5)
        order = np.argsort(keys, kind="stable")
        return keys[order], ap[order].copy(), pr_rc[:, order].copy(), summary[order].copy()

    def results_from_tables(self, keys, ap, pr_rc, names: Optional[Dict] = None) -> dict:
        """{names.get(key, key): the metrics dictionary of `instance_seg_eval` on that scene alone} from per-scene tables."""
        names = names or {}
        return {names.get(int(k), int(k)): compute_averages(ap[s:s + 1], pr_rc[:, s], self.options, self.class_labels, self.groups)
                for s, k in enumerate(keys)}

    def scene_results(self, names: Optional[Dict] = None, state: Optional[torch.Tensor] = None) -> dict:
        """The dictionary `compute_each_sample_metrics` returns: one metrics dictionary per scene, under `names[key]` (the key itself
        where `names` has none)."""
        keys, ap, pr_rc, _ = self.scene_tables(state)
        return self.results_from_tables(keys, ap, pr_rc, names)


def evaluator_each_sample_metrics(results, classes, valid_class_ids, num_stuff_cls: int, options=None, groups=None) -> dict:
    """`InstanceSeg3DEvaluator.compute_each_sample_metrics` (evaluator_3d.py:227-321, the ScanNet branch) for `(eval_ann, pred)`
    pairs on the device, as `eval_ap.evaluator_instance_metrics` takes them: {eval_ann["lidar_idx"]: the metrics dictionary of
    `instance_seg_eval` on that scene alone}.  The scene key is the position in `results`."""
    things = tuple(int(v) for v in valid_class_ids[num_stuff_cls:])
    acc = SceneApAccumulator(things, tuple(classes[num_stuff_cls:-1]), options=options, num_stuff_cls=num_stuff_cls, groups=groups)
    names = {}
    for i, (ann, pred) in enumerate(results):
        acc.add(ann, pred, i)
        names[i] = ann["lidar_idx"]
    return acc.scene_results(names)
