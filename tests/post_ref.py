"""Plain restatements of the post-processing steps, one per kernel of `segdino3d_amd/csrc/post.hip`, written from
`oracle/postprocess_ref.py` (line numbers below are that file's).  Test infrastructure: tests/test_post_ref_oracle.py pins the pieces,
reassembled, to the oracle on the CPU; tests/test_gpu_post_kernels.py compares every kernel with its piece.

The float pieces take `dtype`: float64 is the reference, float32 is the same expression as the oracle evaluates it (the tests measure
the distance between the two and derive their tolerance from it).  The discrete pieces are numpy."""
import numpy as np
import torch

ULP32 = 2.0 ** -23


# ---- float pieces ---------------------------------------------------------------------------------------------------------------------
def class_scores_ref(cls, C, dtype=torch.float64):
    """softmax over the C + 1 columns without the last one (:89) -> (prob [Q, C], row maximum over those C)."""
    p = torch.softmax(cls[:, :C + 1].to(dtype), dim=-1)[:, :C]
    return p, p.max(dim=1)[0]


def mask_scores_ref(masks, flat_idx, score_in, C, normalize, dtype=torch.float64):
    """(:93-99) labels = f % C, queries = f // C, score * sum(sigmoid * [x > 0]) / (sum([x > 0]) + 1e-6)."""
    f = flat_idx.long()
    labels = f % C
    qidx = torch.div(f, C, rounding_mode="floor")
    score = score_in.to(dtype)
    if normalize:
        x = masks[qidx].to(dtype)
        pos = x > 0
        score = score * ((torch.sigmoid(x) * pos).sum(1) / (pos.sum(1).to(dtype) + 1e-6))
    return labels, qidx, score


def gather_sigmoid_ref(masks, S, qidx, order, ld_out, dtype=torch.float64):
    """(:96, :39, :41) sigmoid rows masks[qidx[order]] over the first S columns, zero padded to ld_out, and their sums."""
    x = masks[qidx.long()[order.long()]][:, :S].to(dtype)
    sig = torch.zeros(x.shape[0], ld_out, dtype=dtype)
    sig[:, :S] = torch.sigmoid(x)
    return sig, sig.sum(1)


def nms_decay_ref(inter, area, labels, scores, kernel="linear", sigma=2.0, dtype=torch.float64):
    """(:44-54) the decay of `matrix_nms` between its two sorts, on a given intersection matrix and given areas: rows are already in
    descending score order.  max / min propagate NaN, as torch's do."""
    n = scores.shape[0]
    inter, area = inter[:, :n].to(dtype), area.to(dtype)
    iou = (inter / (area[None, :] + area[:, None] - inter)).triu(diagonal=1)
    same = (labels[None, :] == labels[:, None]).triu(diagonal=1)
    decay_iou = iou * same
    comp = decay_iou.max(0)[0][:, None].expand(n, n)
    if kernel == "gaussian":
        coef = (torch.exp(-sigma * decay_iou ** 2) / torch.exp(-sigma * comp ** 2)).min(0)[0]
    elif kernel == "linear":
        coef = ((1 - decay_iou) / (1 - comp)).min(0)[0]
    else:
        raise NotImplementedError(kernel)
    return scores.to(dtype) * coef


def max_rel_err(a, ref):
    """Largest |a - ref| / |ref| over the finite, non-zero entries of ref (float64)."""
    a, ref = a.double().reshape(-1), ref.double().reshape(-1)
    ok = torch.isfinite(ref) & (ref != 0)
    if not bool(ok.any()):
        return 0.0
    return float(((a[ok] - ref[ok]).abs() / ref[ok].abs()).max())


# ---- discrete pieces ------------------------------------------------------------------------------------------------------------------
def row_argmax_ref(x, ncols=None, cols=None):
    """(:121) x[:, cols].argmax(1) on the CPU: the first maximum, and the first NaN if there is one."""
    x = x.detach().cpu()
    sel = x[:, [int(c) for c in cols]] if cols is not None else x[:, :(x.shape[1] if ncols is None else ncols)]
    return sel.argmax(dim=1)


def expand_masks_ref(sig, src, superpoints, points, thr, boxes=None, loose=1.5):
    """(:104, :77-81) sig[src][:, sp] > thr, the row sums, and the box filter; float32 numpy in the oracle's expression order.
    A superpoint id outside [0, sig.shape[1]) gives 0.  -> (masks uint8 [n, N], count int64 [n] taken before the box filter)."""
    sig = np.asarray(sig, dtype=np.float32)
    sp = np.asarray(superpoints, dtype=np.int64)
    valid = (sp >= 0) & (sp < sig.shape[1])
    rows = sig[np.asarray(src, dtype=np.int64)]
    mask = (rows[:, np.where(valid, sp, 0)] > np.float32(thr)) & valid[None, :]
    count = mask.sum(1).astype(np.int64)
    if boxes is not None:
        b = np.asarray(boxes, dtype=np.float32)
        p = np.asarray(points, dtype=np.float32)[:, :3]
        c, sizes = b[:, :3], b[:, 3:6]
        s = sizes * np.float32(1 + loose)
        lo, hi = c - s / np.float32(2), c + s / np.float32(2)
        inside = ((p[None, :, :] >= lo[:, None, :]) & (p[None, :, :] <= hi[:, None, :])).all(axis=2)
        mask = mask & inside
    return mask.astype(np.uint8), count


def panoptic_ref(masks, rows_desc, labels_desc, n_stuff, npoint_thr, sem_stuff):
    """(:135-150) on given masks: rows_desc / labels_desc list the candidates by descending score.  -> (sem_map, inst_map) int64."""
    m = np.asarray(masks)[np.asarray(rows_desc, dtype=np.int64)][::-1].astype(np.int64)       # ascending, as after `scores.sort()`
    labels = np.asarray(labels_desc, dtype=np.int64)[::-1]
    n = m.shape[0]
    prod = np.arange(n_stuff, n + n_stuff, dtype=np.int64)[:, None] * m
    things_inst, arg = prod.max(0), prod.argmax(0)
    things_sem = labels[arg] + n_stuff
    ids, cnt = np.unique(things_inst, return_counts=True)
    for i, c in zip(ids.tolist(), cnt.tolist()):
        if c <= npoint_thr and i != 0:
            things_inst[things_inst == i] = 0
    things_sem[things_inst == 0] = 0
    sem_map = np.asarray(sem_stuff, dtype=np.int64).copy()
    sem_map[things_inst != 0] = 0
    return sem_map + things_sem, sem_map + things_inst


# ---- the pieces reassembled (what tests/test_post_ref_oracle.py compares with the oracle) ------------------------------------------------
def _desc(v):
    return torch.sort(v, descending=True, stable=True)[1]


def predict_instance_ref(cls, mask_logits, superpoints, points, centers, sizes, C, cfg, score_thr, box_filter, dtype=torch.float64):
    """`predict_instance` (:84-115) from the pieces above.  -> dict(masks uint8 [n, N], labels, scores (dtype), record,
    all_scores [k] after NMS in final order, pre_nms [k] scores before it in top-k order)."""
    S = mask_logits.shape[1]
    k = cfg.topk_insts
    prob, _ = class_scores_ref(cls, C, dtype)
    top, flat_idx = prob.flatten().topk(k, sorted=True)
    labels, qidx, scores = mask_scores_ref(mask_logits, flat_idx, top, C, cfg.obj_normalization, dtype)
    if cfg.nms:
        order1 = _desc(scores)
        sig, area = gather_sigmoid_ref(mask_logits, S, qidx, order1, S, dtype)
        scores2 = nms_decay_ref(sig @ sig.t(), area, labels[order1], scores[order1], cfg.matrix_nms_kernel, 2.0, dtype)
        order2 = _desc(scores2)
        final_scores, final_labels, record = scores2[order2], labels[order1][order2], order1[order2]
    else:
        sig, _ = gather_sigmoid_ref(mask_logits, S, qidx, torch.arange(k), S, dtype)
        order2 = torch.arange(k)
        final_scores, final_labels, record = scores, labels, torch.arange(k)
    boxes = torch.cat([centers[qidx][record], sizes[qidx][record]], dim=-1).float().numpy()
    masks, count = expand_masks_ref(sig.float().numpy(), order2.numpy(), superpoints.numpy(), points.numpy(), cfg.sp_score_thr,
                                    boxes if box_filter else None)
    keep = ((final_scores > score_thr) & torch.from_numpy(count > cfg.npoint_thr)).nonzero().flatten()
    return dict(masks=masks[keep.numpy()], labels=final_labels[keep], scores=final_scores[keep], record=record[keep],
                all_scores=final_scores, pre_nms=scores)


def predict_panoptic_ref(cls, sem_preds, mask_logits, superpoints, points, centers, sizes, C, cfg, box_filter, query_num=-1,
                         dtype=torch.float64):
    """`predict_panoptic` (:127-150) from the pieces above."""
    am = row_argmax_ref(sem_preds, cols=cfg.stuff_classes)
    sem_stuff = (am[superpoints] if query_num == -1 else am[torch.zeros_like(superpoints)]).numpy()
    r = predict_instance_ref(cls, mask_logits, superpoints, points, centers, sizes, C, cfg, cfg.pan_score_thr, box_filter, dtype)
    n = r["masks"].shape[0]
    if n == 0:
        return sem_stuff, sem_stuff
    return panoptic_ref(r["masks"], np.arange(n), r["labels"].numpy(), len(cfg.stuff_classes), cfg.npoint_thr, sem_stuff)


# ---- constructed decoder outputs --------------------------------------------------------------------------------------------------------
# the scene of the GPU chain test; tests/test_post_ref_oracle.py checks its conditions on the CPU
CHAIN = dict(seed=5, Q=64, C=198, grid=(9, 10), N=10_003, n_peaked=40)


def chain_scene(seed, Q, C, grid, N, n_peaked, scale=0.37):
    """Decoder outputs made by hand so that the whole post-processing chain has content: superpoints are the cells of a grid[0] x
    grid[1] grid over the points; a query's mask is a rectangle of cells (logits 2 .. 6 inside, -8 .. -4 outside, a few outside cells
    between -0.35 and -0.05: negative logit, sigmoid above sp_score_thr = 0.4); the first n_peaked queries have one class logit peaked
    at a height of their own, every fourth of them repeats its predecessor's class and rectangle less one cell (matrix-NMS demotes
    the weaker twin); the boxes are 0.75 .. 1.5 of the rectangle, so the out-of-box filter cuts some of them.
    -> dict(cls_preds [Q, C + 1], masks [Q, S], centers, sizes [Q, 3], sem_preds [S, C + 3], superpoints [N], points [N, 6])."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=g)  # noqa: E731
    gx, gy = grid
    S = gx * gy
    xy = u(N, 2) * torch.tensor([gx, gy], dtype=torch.float32)
    cell = xy.floor().long()
    superpoints = cell[:, 0].clamp(max=gx - 1) * gy + cell[:, 1].clamp(max=gy - 1)
    points = torch.cat([xy * scale, u(N, 1) * scale, u(N, 3)], dim=1)
    cls = -10.0 + 0.01 * torch.randn(Q, C + 1, generator=g)
    cls[:, C] = 0.0
    heights = torch.linspace(-3.0, 4.0, n_peaked)[torch.randperm(n_peaked, generator=g)]
    masks = torch.empty(Q, S)
    centers, sizes = torch.empty(Q, 3), torch.empty(Q, 3)
    rect, klass = None, 0
    for q in range(Q):
        twin = q < n_peaked and q % 4 == 3
        if twin:
            x0, y0, w, h = rect
        else:
            w, h = int(torch.randint(1, min(3, gx - 1) + 1, (1,), generator=g)), int(torch.randint(2, min(3, gy) + 1, (1,), generator=g))
            x0, y0 = int(torch.randint(0, gx - w + 1, (1,), generator=g)), int(torch.randint(0, gy - h + 1, (1,), generator=g))
            klass = int(torch.randint(0, C, (1,), generator=g))
        rect = (x0, y0, w, h)
        inside = torch.zeros(gx, gy, dtype=torch.bool)
        inside[x0:x0 + w, y0:y0 + h] = True
        inside = inside.flatten()
        if twin:                                                   # the twin lacks one cell of the rectangle
            cells = inside.nonzero().flatten()
            inside[cells[int(torch.randint(0, cells.numel(), (1,), generator=g))]] = False
        row = -(4.0 + 4.0 * u(S))
        weak = (u(S) < 0.1) & ~inside
        row[weak] = -(0.05 + 0.3 * u(int(weak.sum())))
        row[inside] = 2.0 + 4.0 * u(int(inside.sum()))
        masks[q] = row
        if q < n_peaked:
            cls[q, klass] = heights[q]
        shrink = 0.3 + 0.3 * u(3)
        centers[q] = torch.tensor([x0 + w / 2, y0 + h / 2, 0.5]) * scale
        sizes[q] = torch.tensor([float(w), float(h), 1.0]) * scale * shrink
    sem = 2.0 * torch.randn(S, C + 3, generator=g)
    return dict(cls_preds=cls, masks=masks, centers=centers, sizes=sizes, sem_preds=sem, superpoints=superpoints, points=points)


def chain_conditions(P, scene, C, cfg, box_filter, query_num):
    """The conditions of the chain test, taken from the oracle's own output: -> (oracle result, dict of the measured quantities).
    Asserts them."""
    import dataclasses
    out = {k: scene[k] for k in ("cls_preds", "masks", "centers", "sizes", "sem_preds")}
    sp, xyz = scene["superpoints"], scene["points"][:, :3]
    res = P.predict_by_feat(out, sp, xyz, C, cfg, box_filter, query_num)
    args = (out["cls_preds"], out["masks"], sp, xyz, out["centers"], out["sizes"], C)
    pan = P.predict_instance(*args, cfg, cfg.pan_score_thr, box_filter)
    n_pan = int(pan["scores"].shape[0])
    # demoted by NMS: the same top-k entry (`record`) with and without the decay
    free_cfg = dataclasses.replace(cfg, npoint_thr=-1)
    with_nms = P.predict_instance(*args, free_cfg, -1.0, False)
    without = P.predict_instance(*args, dataclasses.replace(free_cfg, nms=False), -1.0, False)
    before = torch.empty(cfg.topk_insts)
    before[without["record"]] = without["scores"]
    before = before[with_nms["record"]]
    demoted = int(((before > 1e-3) & (with_nms["scores"] < 0.9 * before)).sum())
    s = with_nms["scores"]
    s = torch.sort(s[s > 1e-3])[0]
    gap = float(((s[1:] - s[:-1]) / s[1:]).min())
    for t in (cfg.pan_score_thr, cfg.inst_score_thr, 1e-3):
        if t > 0:
            gap = min(gap, float(((with_nms["scores"] - t).abs() / t).min()))
    logit_margin = float(out["masks"].abs().min())
    sig_margin = float((torch.sigmoid(out["masks"].double()) - cfg.sp_score_thr).abs().min())
    assert n_pan >= 10, n_pan
    assert demoted >= 3, demoted
    assert gap > 1e-3, gap
    assert logit_margin > 1e-4 and sig_margin > 1e-4, (logit_margin, sig_margin)
    return res, dict(n_pan=n_pan, demoted=demoted, n_scored=int(s.numel()), gap=gap, logit_margin=logit_margin, sig_margin=sig_margin)
