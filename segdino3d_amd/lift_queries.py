"""Lift a 2D detector's queries to 3D centres on the device (csrc/lift_queries.hip): the producer of `query2d_feats` [M, C] and
`query2d_pos` [M, 3], the two inputs of the decoder's DINO-X query cross-attention and its 0.2 m distance mask.  The reference only
loads them from a per-scene dump (`scannet200.py:218-232`) and ships no code that makes them, so there is no reference
implementation to pin against: the rule below is restated in float64 numpy in tests/lift_queries_ref.py, and the kernels are tested
against that.

Inputs per batch of frames: a `lift2d.Views` (depth, intrinsics, poses; views with a non-finite pose are dropped), `masks`
[V, Q, Hm, Wm] bool or uint8 (non-zero = set) at any resolution, `scores` fp32 [V, Q] and `feats` [V, Q, C] fp16 or fp32.

  1. Mask sample.  Depth pixel `(vi, ui)` reads mask pixel `ym = ((2 vi + 1) Hm) / (2 Hd)`, `xm = ((2 ui + 1) Wm) / (2 Wd)`, integer
     divisions: the mask pixel nearest to the depth pixel's centre, exactly.
  2. Depth key.  `d` = depth in fp32 metres (`raw * depth_scale` in fp32 for uint16); require `d > 0`; `t = d * 1000 + 0.5` in fp32;
     require `t < 65536`; `k = (int) floor(t)`, millimetres; require `1 <= k <= far_mm`.  Every comparison is made on floats before
     anything becomes an integer: NaN, infinite, negative and huge depths are simply invalid.
  3. Median.  Over the `n` valid masked pixels of `(v, q)`, `k_med` is the key of rank `(n - 1) / 2` in ascending order, the lower
     median, exact.  `n == 0` gives `count = 0`.
  4. Gate.  Keep a pixel iff `1000 |k - k_med| <= 1000 gate_mm + gate_permille * k_med` (integers): it removes the background a mask
     leaks onto at depth edges.  `gate_abs` (metres) and `gate_rel` become `gate_mm` and `gate_permille` by `round(x * 1000)`.
  5. Back-projection.  `p_c = ((ui - cx) d / fx, (vi - cy) d / fy, d)` in fp32, `w = R p_c + t` with the fp32 `cam_to_world`, each
     component as `((r0 x + r1 y) + r2 z) + t` with every operation rounded on its own (no fused multiply-add); require every
     component finite and `|w| < 2^14`, otherwise the pixel is dropped and not counted.
  6. Centre.  Each kept component becomes `rint(w * 2^20)` as int64; the three sums are int64, so the result has the same bits under
     any schedule, cut of the views into `add` calls, or stream; `count` = the kept pixels;
     `centre = (float)((double) sum / (double) count / 2^20)`, zero where `count == 0`.
  7. Validity and selection.  `(v, q)` is valid iff `score >= score_thr` (a NaN fails) and `count >= min_pixels`.  The flat index is
     `(running kept-view index) * Q + q` over all `add` calls.  With `max_queries = None`, or no more valid entries than the cap, all
     valid entries are emitted in ascending flat index; otherwise the `max_queries` best by score descending, ties to the lower flat
     index, again in ascending flat index.  Equal floats are ties; the order is the one of `sd3d_keys_from_f32`, under which +0
     sorts before -0.
  8. Output.  `query2d_feats` fp32 [M, C] = the selected rows of `feats` (fp16 to fp32 is exact), `query2d_pos` fp32 [M, 3]; both
     contiguous device tensors, ready for `extra_features`, `targets.drop_2d_queries` and `io_scene.pack_scene`.

`result()` keeps duplicates: the object in front of the camera is in dozens of its rows.  `merged()` / `merge_queries` /
`lift_queries(..., merge=dict(...))` group the rows that are the same object (csrc/merge_queries.hip) and emit one query per group.
The rule is restated with exact integers in tests/merge_queries_ref.py; inputs are rows `feats [n, C]`, `centre [n, 3]`, `scores [n]`,
`count [n]` with `view = row // queries_per_view`:

  1. Valid rows.  `score >= score_thr` (a NaN fails), `count >= min_pixels`, every centre component finite with `|c| < 2^14`.  If
     more than 16384 rows are valid the best by score enter, ties to the lower row.
  2. Order.  Entering rows are ranked by score descending, ties to the lower row (the order of `sd3d_keys_from_f32`).
  3. Fixed-point centre.  `p = rint(centre * 1024)` per component as int32.
  4. Quantised feature.  `s = max_j |f_j|` in fp32; a row whose `s` is not finite or below `2^-100` has an all-zero code; otherwise,
     with `2^(e-1) <= s < 2^e`, `q_j = clamp(rint(f_j * 2^(7-e)), -127, 127)` as int8 and `nrm = sum q_j^2`.
  5. Adjacency of ranks `a < b`.  `r_q = round(radius * 1024)` in `1 .. 2^20`: `dx^2 + dy^2 + dz^2 <= r_q^2`; and, unless `sim` is
     None, with `s7 = round(sim * 128)` in `1 .. 128` and `d = sum q_a q_b`: `d > 0` and `d d 16384 >= s7 s7 nrm_a nrm_b` in int64.  A
     zero code is adjacent to nothing, with or without `sim`.
  6. Leader clustering, the greedy order of NMS.  Walk the ranks upward; an unlabelled rank becomes a seed and labels every later
     unlabelled rank adjacent to it.  Not a transitive closure: a chair next to a table does not chain into one cluster.
  7. Per cluster, members in ascending row order: `w_i = min(count_i, 2^20)`, `pos = (float)((double) sum w_i p_i / (double) sum w_i /
     1024)` with int64 sums, `views` = the distinct `row // queries_per_view`, `score` = the seed's, `feat` = per channel in fp32
     `acc = acc + (float) w_i * f_i` (two rounded operations per member) then `acc / (float) sum w_i` (`reduce="mean"`), or the seed's
     row (`reduce="best"`).
  8. Emit.  Clusters with `views < min_views` are dropped; of the rest at most the `max_queries` best by seed score, ties to the lower
     seed row; in ascending seed row.  `labels` int32 [n] = the output index of each input row's cluster, or -1.

Two detections of one object in the same frame merge too, and count as one view.

Out of scope: the 2D detector and reading image files; the dataset's `dropout_rate_2dfeats` and the decoder's distance mask are what
the reference applies to the queries."""
from __future__ import annotations

from collections import namedtuple

import torch

from . import ops
from .lift2d import Views

RULE_DEFAULTS = dict(far=20.0, gate_abs=0.10, gate_rel=0.05, min_pixels=16, score_thr=0.3, max_queries=None)
MERGE_DEFAULTS = dict(radius=0.3, sim=0.75, min_views=1, max_queries=None, reduce="mean")

Merged = namedtuple("Merged", "feats pos scores views labels")
Merged.__doc__ = """One query per object: feats fp32 [K, C], pos fp32 [K, 3], scores fp32 [K] (the seed's), views int32 [K] (the distinct
frames behind it), labels int32 [n] (the output index of each input row's cluster, or -1); contiguous device tensors."""


def _merge_rule(rule: dict, score_thr, min_pixels) -> dict:
    """MERGE_DEFAULTS plus the lifter's own `score_thr` and `min_pixels` -> the checked rule with its integer forms."""
    known = set(MERGE_DEFAULTS) | {"score_thr", "min_pixels"}
    bad = set(rule) - known
    if bad:
        raise TypeError(f"unknown query-merging parameter(s) {sorted(bad)}; known: {sorted(known)}")
    r = {**MERGE_DEFAULTS, "score_thr": score_thr, "min_pixels": min_pixels, **rule}
    r["radius_q"] = round(float(r["radius"]) * 1024)
    if not 1 <= r["radius_q"] <= 1 << 20:
        raise ValueError(f"radius must lie in [1/1024, 1024] m, got {r['radius']}")
    if r["sim"] is None:
        r["sim_q"] = 0
    else:
        r["sim_q"] = round(float(r["sim"]) * 128)
        if not 0.0 <= float(r["sim"]) <= 1.0 or not 1 <= r["sim_q"] <= 128:
            raise ValueError(f"sim must be None (distance only) or a cosine in [1/256, 1], got {r['sim']}")
    if int(r["min_views"]) != r["min_views"] or r["min_views"] < 1:
        raise ValueError(f"min_views must be an integer >= 1, got {r['min_views']}")
    if int(r["min_pixels"]) != r["min_pixels"] or r["min_pixels"] < 1:
        raise ValueError(f"min_pixels must be an integer >= 1, got {r['min_pixels']}")
    if r["max_queries"] is not None and (int(r["max_queries"]) != r["max_queries"] or r["max_queries"] < 0):
        raise ValueError(f"max_queries must be None or an integer >= 0, got {r['max_queries']}")
    if r["reduce"] not in ("mean", "best"):
        raise ValueError(f"reduce must be 'mean' or 'best', got {r['reduce']!r}")
    return r


def merge_queries(feats, centre, scores, count, queries_per_view: int, **rule) -> Merged:
    """One query per object from rows `feats` fp16 or fp32 [n, C <= 1024], `centre` fp32 [n, 3], `scores` fp32 [n], `count` int32 [n]
    (the pixels behind each centre), `view = row // queries_per_view`: the rule of the module docstring, steps 1 to 8.  `rule`:
    MERGE_DEFAULTS, plus `score_thr` and `min_pixels` (the lifter's defaults).  Two detections of one object in the same frame merge
    too, and count as one view.  One host read, of the cluster count."""
    r = _merge_rule(rule, RULE_DEFAULTS["score_thr"], RULE_DEFAULTS["min_pixels"])
    for t, name in ((feats, "feats"), (centre, "centre"), (scores, "scores"), (count, "count")):
        _on_device(t, f"merge_queries: {name}")
    if int(queries_per_view) != queries_per_view or queries_per_view < 1:
        raise ValueError(f"merge_queries: queries_per_view must be an integer >= 1, got {queries_per_view}")
    ws = ops.merge_queries_adjacency(feats, centre, scores, count, r["score_thr"], r["min_pixels"], r["radius_q"], r["sim_q"])
    n, C = feats.shape
    ops.merge_queries_sweep(n, C, ws)
    k = ops.merge_queries_reduce(scores, count, C, queries_per_view, r["score_thr"], r["min_views"], r["max_queries"], ws)
    K = int(k.item()) if n else 0                                                       # the one host read
    return Merged(*ops.merge_queries_emit(feats, scores, count, K, r["reduce"] == "best", ws))


def _rule(rule: dict) -> dict:
    bad = set(rule) - set(RULE_DEFAULTS)
    if bad:
        raise TypeError(f"unknown query-lifting parameter(s) {sorted(bad)}; known: {sorted(RULE_DEFAULTS)}")
    r = {**RULE_DEFAULTS, **rule}
    r["far_mm"], r["gate_mm"], r["gate_permille"] = round(r["far"] * 1000), round(r["gate_abs"] * 1000), round(r["gate_rel"] * 1000)
    if not 1 <= r["far_mm"] <= 65535:
        raise ValueError(f"far must lie in [0.001, 65.535] m (16-bit millimetre keys), got {r['far']}")
    if not 0 <= r["gate_mm"] <= 65535 or not 0 <= r["gate_permille"] <= 65535:
        raise ValueError(f"gate_abs and gate_rel must lie in [0, 65.535], got {r['gate_abs']}, {r['gate_rel']}")
    if int(r["min_pixels"]) != r["min_pixels"] or r["min_pixels"] < 1:
        raise ValueError(f"min_pixels must be an integer >= 1, got {r['min_pixels']}")
    if r["max_queries"] is not None and (int(r["max_queries"]) != r["max_queries"] or r["max_queries"] < 0):
        raise ValueError(f"max_queries must be None or an integer >= 0, got {r['max_queries']}")
    return r


def _on_device(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor on the HIP device, got {t.device} (no CPU fallback)")


class QueryLifter:
    """The 2D queries of one scene, accumulated over any number of batches of frames, as a 2D detector delivers them.

    `add(views, masks, scores, feats)` only enqueues: one centre kernel over the batch, whose rows are appended to device-resident
    stores that grow geometrically.  `result()` enqueues the selection, reads `M` (the one host read) and gathers
    `(query2d_feats, query2d_pos)`.  `centres()`, `counts()` and `medians_mm()` are the live per-(view, query) tensors.  One lifter
    per stream."""

    def __init__(self, channels: int, **rule):
        self.rule = _rule(rule)
        if int(channels) != channels or channels < 8 or channels % 8:
            raise ValueError(f"QueryLifter: channels must be a multiple of 8, got {channels}")
        self.channels, self.n_queries, self.n_views = int(channels), None, 0
        self._cap = 0
        self._centre = self._count = self._median = self._scores = self._feats = None

    def _grow(self, need: int, Q: int, feat_dtype, dev) -> None:
        if need <= self._cap:
            return
        cap = max(need, 2 * self._cap, 16)
        shapes = (("_centre", (cap, Q, 3), torch.float32), ("_count", (cap, Q), torch.int32), ("_median", (cap, Q), torch.int32),
                  ("_scores", (cap, Q), torch.float32), ("_feats", (cap, Q, self.channels), feat_dtype))
        for name, shape, dtype in shapes:
            new, old = torch.empty(shape, dtype=dtype, device=dev), getattr(self, name)
            if old is not None and self.n_views:
                new[:self.n_views].copy_(old[:self.n_views])
            setattr(self, name, new)
        self._cap = cap

    def add(self, views: Views, masks, scores, feats) -> None:
        if not isinstance(views, Views):
            raise TypeError(f"QueryLifter.add: views must be a lift2d.Views, got {type(views).__name__}")
        for t, name in ((masks, "masks"), (scores, "scores"), (feats, "feats")):
            _on_device(t, f"QueryLifter.add: {name}")
        if masks.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"QueryLifter.add: masks must be bool or uint8, got {masks.dtype}")
        if scores.dtype != torch.float32:
            raise TypeError(f"QueryLifter.add: scores must be fp32, got {scores.dtype}")
        if feats.dtype not in (torch.float16, torch.float32):
            raise TypeError(f"QueryLifter.add: feats must be fp16 or fp32, got {feats.dtype}")
        if masks.dim() != 4 or masks.shape[2] < 1 or masks.shape[3] < 1:
            raise ValueError(f"QueryLifter.add: masks must be [V, Q, Hm, Wm], got {list(masks.shape)}")
        V, Q = masks.shape[:2]
        if V not in (views.n_given, len(views)):
            raise ValueError(f"QueryLifter.add: expected one row of masks per view ({views.n_given} given, {len(views)} kept), got {list(masks.shape)}")
        if tuple(scores.shape) != (V, Q):
            raise ValueError(f"QueryLifter.add: scores must be [V = {V}, Q = {Q}] as the masks {list(masks.shape)}, got {list(scores.shape)}")
        if tuple(feats.shape) != (V, Q, self.channels):
            raise ValueError(f"QueryLifter.add: feats must be [V = {V}, Q = {Q}, C = {self.channels}], got {list(feats.shape)}")
        if self.n_queries is not None and Q != self.n_queries:
            raise ValueError(f"QueryLifter.add: {Q} queries per view, earlier calls had {self.n_queries}: masks {list(masks.shape)}")
        if self._feats is not None and feats.dtype != self._feats.dtype:
            raise TypeError(f"QueryLifter.add: feats are {feats.dtype}, earlier calls had {self._feats.dtype}")
        if views.height * views.width > ops.LIFTQ_MAX_PIXELS:
            raise ValueError(f"QueryLifter.add: depth images of {views.height} x {views.width} exceed 2^28 pixels (the int64 sums could overflow)")
        self.n_queries = Q
        K = len(views)
        if K == 0 or Q == 0:
            return
        # bool has the bytes of uint8; rows of dropped views are skipped the way select_maps does it
        masks = views.select_maps(masks.view(torch.uint8) if masks.dtype == torch.bool else masks).contiguous()
        scores, feats = views.select_maps(scores), views.select_maps(feats)
        self._grow(self.n_views + K, Q, feats.dtype, masks.device)
        lo, hi, r = self.n_views, self.n_views + K, self.rule
        self._scores[lo:hi].copy_(scores)
        self._feats[lo:hi].copy_(feats)
        ops.lift_query_centres(views.depth, views.depth_scale, views.intrinsics, views.cam_to_world, masks, r["far_mm"], r["gate_mm"],
                               r["gate_permille"], self._centre[lo:hi], self._count[lo:hi], self._median[lo:hi])
        self.n_views = hi

    def _live(self, store):
        if store is None:
            raise RuntimeError("QueryLifter: nothing was added yet")
        return store[:self.n_views]

    def centres(self) -> torch.Tensor:
        """fp32 [views so far, Q, 3] (the live device tensor; a later `add` may move the store)."""
        return self._live(self._centre)

    def counts(self) -> torch.Tensor:
        """int32 [views so far, Q]: the pixels that passed the gate."""
        return self._live(self._count)

    def medians_mm(self) -> torch.Tensor:
        """int32 [views so far, Q]: the median depth key in millimetres (0 where nothing valid lay under the mask)."""
        return self._live(self._median)

    def result(self):
        """-> (query2d_feats fp32 [M, C], query2d_pos fp32 [M, 3]).  May be called at any time; the lifter goes on."""
        r = self.rule
        if self._centre is None or self.n_views == 0:
            dev = self._centre.device if self._centre is not None else torch.device("cuda", torch.cuda.current_device())
            return torch.empty(0, self.channels, device=dev), torch.empty(0, 3, device=dev)
        n = self.n_views * self.n_queries
        rows, m = ops.lift_query_select(self._scores[:self.n_views].view(n), self._count[:self.n_views].view(n), r["score_thr"],
                                        r["min_pixels"], r["max_queries"])
        M = int(m.item())                                                              # the one host read
        return ops.lift_query_gather(self._feats[:self.n_views].view(n, self.channels), self._centre[:self.n_views].view(n, 3), rows, M)


    def merged(self, **merge_rule) -> Merged:
        """One query per object over the live stores (`merge_queries` with the lifter's `score_thr` and `min_pixels`; `merge_rule`:
        MERGE_DEFAULTS).  One host read, of the cluster count.  May be called at any time; the lifter goes on, and `result()` is
        what it was."""
        r = self.rule
        _merge_rule(merge_rule, r["score_thr"], r["min_pixels"])                        # refuse a bad rule before anything else
        if self._centre is None or self.n_views == 0:
            dev = self._centre.device if self._centre is not None else torch.device("cuda", torch.cuda.current_device())
            return Merged(torch.empty(0, self.channels, device=dev), torch.empty(0, 3, device=dev), torch.empty(0, device=dev),
                          torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev))
        n = self.n_views * self.n_queries
        rule = {"score_thr": r["score_thr"], "min_pixels": r["min_pixels"], **merge_rule}
        return merge_queries(self._feats[:self.n_views].view(n, self.channels), self._centre[:self.n_views].view(n, 3),
                             self._scores[:self.n_views].view(n), self._count[:self.n_views].view(n), self.n_queries, **rule)


def lift_queries(views: Views, masks, scores, feats, merge=None, **rule):
    """The one-shot form: -> (query2d_feats fp32 [M, C], query2d_pos fp32 [M, 3]), ready for `extra_features["query2d_feats"]` /
    `["query2d_pos"]` or `io_scene.pack_scene`.  With `merge=dict(...)` (MERGE_DEFAULTS; `{}` takes them as they are) the rows of one
    object are merged first and the pair is `Merged.feats`, `Merged.pos`: one query per object."""
    if not isinstance(feats, torch.Tensor) or feats.dim() != 3:
        raise ValueError(f"lift_queries: feats must be a tensor [V, Q, C], got {list(getattr(feats, 'shape', []))}")
    if merge is not None and not isinstance(merge, dict):
        raise TypeError(f"lift_queries: merge must be None or a dict of merging parameters, got {type(merge).__name__}")
    lifter = QueryLifter(feats.shape[2], **rule)
    lifter.add(views, masks, scores, feats)
    if merge is None:
        return lifter.result()
    m = lifter.merged(**merge)
    return m.feats, m.pos
