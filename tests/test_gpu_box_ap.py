"""`eval_box.BoxApAccumulator` + csrc/boxeval.hip against the numpy restatement of the protocol (tests/box_ap_ref.py), which walks
the predictions sequentially with taken flags; the kernels decompose the walk.

Bounds: entries (group, score bits, true), npos, has_pred, the status word, `ar` and the ground-truth corners must equal the restatement
exactly.  `ap` within 1e-12 absolute, the bound of every AP comparison in this project: at most 4096 terms of magnitude at most 1
summed in float64 in another order differ by less than 4096 * 2^-52 ~ 9e-13 (every group here holds at most 4096 entries; asserted).
Inputs: every IoU the restatement computes lies at least 1e-9 from every threshold - asserted on the CPU before anything is compared -
so a last-bit difference cannot move a decision; the deliberate equality cases are built on a 1/8 grid, where the arithmetic is exact."""
import numpy as np
import pytest
import torch

import box_ap_ref as R

pytestmark = pytest.mark.gpu

THR = (0.25, 0.5)


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _names(C):
    return tuple(f"c{i}" for i in range(C))


def _lut(valid, d):
    lut = np.full(max(valid) + 1, -1, dtype=np.int32)
    lut[list(valid)] = np.arange(len(valid), dtype=np.int32)
    return torch.from_numpy(lut).to(d)


def _dev_scene(s, d):
    return (torch.from_numpy(s["gt_corners"]).to(d), torch.from_numpy(s["gt_cls"]).to(d), torch.from_numpy(s["boxes"]).to(d),
            torch.from_numpy(s["labels"]).to(d), torch.from_numpy(np.asarray(s["scores"], dtype=np.float32)).to(d))


def _assert_margin(refs, thr):
    for ref in refs:
        if len(ref["ious"]):
            gap = np.abs(ref["ious"][:, None] - np.asarray(thr)[None, :]).min()
            assert gap >= 1e-9, f"an IoU lies {gap} from a threshold: choose another seed"


def _same(a, b):
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _assert_entries(e, want):
    group, score, true, npos, has_pred, status = want
    assert e["status"] == status
    assert np.array_equal(e["group"], group) and np.array_equal(e["true"], true)
    assert e["score"].tobytes() == score.astype(np.float32).tobytes()
    assert np.array_equal(e["npos"], npos) and np.array_equal(e["has_pred"], has_pred)


def _check(scenes, C, d, thr=THR, margin=True):
    """Device route over `scenes` == restatement: entries and counters exactly, ar exactly, ap within 1e-12.  Returns
    (accumulator, restatement entries, tables)."""
    from segdino3d_amd import eval_box
    refs = [R.scene_of(s, C, thr) for s in scenes]
    if margin:
        _assert_margin(refs, thr)
    want = R.accumulate(refs, C)
    if len(want[0]):
        assert np.bincount(want[0]).max() <= 4096
    acc = eval_box.BoxApAccumulator(tuple(range(C)), _names(C), iou_thr=thr)
    for s in scenes:
        acc.add_boxes(*_dev_scene(s, d))
    _assert_entries(acc.entries(), want)
    ap, ar = acc.tables()
    ap_w, ar_w = R.finish(want[0], want[1], want[2], want[3], len(thr))
    print("max |ap - restatement|:", np.nanmax(np.abs(ap - ap_w)) if np.isfinite(ap_w).any() else 0.0)
    assert _same(ar, ar_w), "ar is not equal to the restatement"
    assert ap.shape == ap_w.shape and np.array_equal(np.isnan(ap), np.isnan(ap_w))
    assert np.allclose(ap, ap_w, rtol=0, atol=1e-12, equal_nan=True)
    return acc, want, (ap, ar)


# ------------------------------------------------------------------------------------------------------------------ 1. ground-truth boxes
VALID = (5, 6, 9)
SEM_OF = {0: 5, 1: 6, 7: 5, 999: 9}


def _gt_case(N, seed):
    rng = np.random.RandomState(seed)
    pts = rng.normal(0.0, 3.0, size=(N, 3)).astype(np.float32)
    options = np.array([-1, 0, 0, 0, 1, 7, 999, 3])
    inst = rng.choice(options, size=N).astype(np.int64)                                  # instance 0 spans every workgroup
    inst[:len(options)] = options[:N]                                                    # every case occurs
    if N == 1:
        inst[:] = 999                                                                    # a one-point instance: a zero-size box
    sem = np.array([SEM_OF.get(int(i), 4) for i in inst], dtype=np.int64)                # id 4 has no class: instance 3 is void
    pts[inst == 7] = -np.abs(pts[inst == 7]) - 1.0                                       # all-negative coordinates
    one = np.flatnonzero(inst == 1)
    if len(one):
        pts[one, 0] = -np.abs(pts[one, 0])
        pts[one[0], 0] = -0.0                                                            # the maximum of x is -0: reads as +0
        pts[one, 1] = np.abs(pts[one, 1])
        pts[one[-1], 1] = -0.0                                                           # the minimum of y is -0 (or +0 beside it)
    return pts, sem, inst


def _gt_on_device(pts, sem, inst, d, padded, valid=VALID, **kw):
    from segdino3d_amd import ops
    N = len(sem)
    status = torch.zeros(1, dtype=torch.int64, device=d)
    if padded:
        big = torch.full((N, 6), 123.0, dtype=torch.float32, device=d)                   # leading dimension 6
        big[:, :3] = torch.from_numpy(pts).to(d)
        ids = torch.full((N, 3), 5, dtype=torch.int64, device=d)                         # element stride 3
        ids[:, 0] = torch.from_numpy(sem).to(d)
        ids[:, 2] = torch.from_numpy(inst).to(d)
        args = (big, ids[:, 0], ids[:, 2])
    else:
        args = (torch.from_numpy(pts).to(d), torch.from_numpy(sem).to(d), torch.from_numpy(inst).to(d))
    corners, cls = ops.gt_boxes(*args, _lut(valid, d), len(valid), status, **kw)
    return corners.cpu().numpy(), cls.cpu().numpy(), int(status.item())


@pytest.mark.parametrize("N", [1, 63, 64, 65, 4097])
def test_ground_truth_boxes_are_exact(N):
    d = dev()
    pts, sem, inst = _gt_case(N, 100 + N)
    corners_w, cls_w, status_w = R.gt_boxes(pts, sem, inst, VALID)
    assert status_w == 0 and (cls_w >= 0).sum() == len(set(inst.tolist()) & set(SEM_OF))
    for padded in (False, True):
        corners, cls, status = _gt_on_device(pts, sem, inst, d, padded)
        assert status == 0 and np.array_equal(cls, cls_w)
        assert corners.tobytes() == corners_w.tobytes()                                  # bit for bit, the sign of zero included
    if N == 1:
        assert cls_w[999] == 2 and corners_w[999, :3].tolist() == corners_w[999, 3:].tolist() == pts[0].tolist()
    if N >= 63:
        assert cls_w[0] == 0 and cls_w[7] == 0 and (corners_w[7] < 0).all() and cls_w[3] == -1
        assert corners_w[1, 3] == 0.0 and not np.signbit(corners_w[1, 3]) and corners_w[1, 1] == 0.0 and not np.signbit(corners_w[1, 1])


def test_ground_truth_status_bits_come_alone():
    d = dev()
    pts, sem, inst = _gt_case(65, 7)
    for what, bit in (("mixed", R.MIXED_SEMANTIC), ("instance", R.BAD_INSTANCE), ("nan", R.BAD_COORD)):
        p, s, i = pts.copy(), sem.copy(), inst.copy()
        k = int(np.flatnonzero(inst == 0)[1])
        if what == "mixed":
            s[k] = 9                                                                     # instance 0 over classes 0 and 2
        elif what == "instance":
            i[k] = 1000
        else:
            p[k, 1] = np.nan
        corners_w, cls_w, status_w = R.gt_boxes(p, s, i, VALID)
        assert status_w == bit
        corners, cls, status = _gt_on_device(p, s, i, d, padded=False)
        assert status == bit and np.array_equal(cls, cls_w) and corners.tobytes() == corners_w.tobytes()
    assert R.gt_boxes(p, s, i, VALID)[1][0] == -1                                        # the NaN instance is left out


# ------------------------------------------------------------------------------------------------------------------ 2. one scene
@pytest.mark.parametrize("n,per_class,C,present", [(0, 1, 1, (0,)), (1, 1, 1, (0,)), (64, 64, 3, (0, 2)), (65, 65, 3, (0, 1, 2)),
                                                   (600, 65, 200, (3, 77, 199)), (600, 0, 200, ()), (64, 1, 3, (1,))])
def test_one_scene_equals_the_sequential_walk(n, per_class, C, present):
    d = dev()
    s = R.make_scene(1000 + n + per_class, n, C, present, per_class)
    acc, want, (ap, ar) = _check([s], C, d)
    assert len(want[0]) == 2 * n and want[3].sum() == per_class * len(present)
    if n >= 64 and per_class:
        assert want[2].sum() > 0 and (want[2] == 0).sum() > 0 and np.nanmax(ap) > 0.0
    if not present:
        assert np.isnan(ap).all() and np.isnan(ar).all()


def test_one_group_longer_than_a_tile():
    """Four scenes of 600 predictions with almost every entry in the groups of one class: the curve walks several tiles of 256 with
    its running counts and running maximum carried over; the group stays under the 4096 entries of the AP bound."""
    d = dev()
    scenes = [R.make_scene(2000 + k, 600, 2, (0,), 65) for k in range(4)]
    acc, want, (ap, ar) = _check(scenes, 2, d)
    assert 8 * 256 < np.bincount(want[0]).max() <= 4096 and 0.0 < ap[0, 1] < ap[0, 0] < 1.0 and np.isnan(ap[1]).all()


def _corner(lo, hi):
    return list(lo) + list(hi)


def _cs(lo, hi):
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    return list((lo + hi) / 2) + list(hi - lo)


def test_deliberate_equalities_on_a_grid():
    """Coordinates on a 1/8 grid: every IoU below is the same exact arithmetic on both sides, so equalities are real."""
    d = dev()
    gt_corners = np.zeros((30, 6), dtype=np.float32)
    gt_cls = np.full(30, -1, dtype=np.int32)
    gts = {2: (0, _corner((0, 0, 0), (1, 1, 1))), 5: (1, _corner((2, 0, 0), (3, 1, 1))),
           10: (2, _corner((4, 0, 0), (5, 1, 1))), 20: (2, _corner((4, 0, 1), (5, 1, 2))),
           7: (3, _corner((6, 0, 0), (7, 1, 1))), 8: (3, _corner((6, 0, 0.5), (7, 1, 1.5)))}
    for col, (c, box) in gts.items():
        gt_cls[col], gt_corners[col] = c, box
    preds = [  # class, box, score
        (0, _cs((0, 0, 0), (1, 1, 1)), 0.875),          # three predictions on one ground truth: tp
        (0, _cs((0, 0, 0), (1, 1, 0.75)), 0.75),        # IoU 0.75, taken: fp
        (0, _cs((0, 0, 0), (1, 1, 0.5)), 0.625),        # IoU 0.5 exactly: fp
        (1, _cs((2, 0, 0), (3, 1, 0.5)), 0.5),          # equal scores: the lower row takes the ground truth - at 0.25 only (IoU 0.5 exactly)
        (1, _cs((2, 0, 0), (3, 1, 0.5)), 0.5),
        (2, _cs((4, 0, 0.5), (5, 1, 1.5)), 0.875),      # IoU 1/3 to columns 10 and 20: column 10
        (2, _cs((4, 0, 0.5), (5, 1, 1.5)), 0.75),       # column 10 again (taken): fp, column 20 stays free
        (3, _cs((6, 0, 0), (7, 1, 1)), 0.875),          # takes column 7
        (3, _cs((6, 0, 0.125), (7, 1, 1.125)), 0.75),   # best is column 7 (taken); column 8 is above 0.25 but no second choice: fp
        (4, _cs((0, 0, 0), (1, 1, 1)), 0.5),            # no ground truth of its class
    ]
    s = dict(gt_corners=gt_corners, gt_cls=gt_cls, boxes=np.array([p[1] for p in preds], dtype=np.float32),
             labels=np.array([p[0] for p in preds], dtype=np.int64), scores=np.array([p[2] for p in preds], dtype=np.float32))
    for a in (s["gt_corners"], s["boxes"]):
        assert np.array_equal(a * 8, np.round(a * 8))
    ref = R.scene_of(s, 5, THR)
    by_row = {}
    for (g, sc, t), r in zip(ref["entries"], np.repeat(np.lexsort((np.arange(10), -s["scores"].astype(np.float64))), 2)):
        by_row[(int(r), g % 2)] = t
    assert [by_row[(r, 0)] for r in range(10)] == [1, 0, 0, 1, 0, 1, 0, 1, 0, 0]         # at 0.25
    assert [by_row[(r, 1)] for r in range(10)] == [1, 0, 0, 0, 0, 0, 0, 1, 0, 0]         # at 0.5
    acc, want, (ap, ar) = _check([s], 5, d, margin=False)
    assert want[3].tolist() == [1, 1, 2, 2, 0] and np.isnan(ap[4]).all()
    assert ar.tolist()[:4] == [[1.0, 1.0], [1.0, 0.0], [0.5, 0.0], [0.5, 0.5]]


def test_left_out_predictions_set_their_bit_alone():
    from segdino3d_amd import eval_box
    d = dev()
    base = R.make_scene(77, 65, 3, (0, 1, 2), 3)
    for what, bit in (("size", R.BAD_BOX), ("label", R.BAD_LABEL), ("score", R.BAD_SCORE), ("centre", R.BAD_BOX), ("gt", R.BAD_COORD)):
        s = {k: v.copy() for k, v in base.items()}
        if what == "size":
            s["boxes"][64, 4] = -0.5
        elif what == "label":
            s["labels"][64] = 3
        elif what == "score":
            s["scores"][64] = np.inf
        elif what == "centre":
            s["boxes"][0, 0] = np.nan
        else:
            s["gt_corners"][np.flatnonzero(s["gt_cls"] >= 0)[0], 5] = -np.inf
        ref = R.scene_of(s, 3, THR)
        _assert_margin([ref], THR)
        assert ref["status"] == bit and len(ref["entries"]) == 2 * (65 if what == "gt" else 64)
        acc = eval_box.BoxApAccumulator((0, 1, 2), _names(3))
        acc.add_boxes(*_dev_scene(s, d))
        _assert_entries(acc.entries(), R.accumulate([ref], 3))
        with pytest.raises(RuntimeError, match=f"status {bit}"):
            acc.tables()


# ------------------------------------------------------------------------------------------------------------------ 3. the accumulator
def _three_scenes():
    return [R.make_scene(500 + k, 70 + 30 * k, 6, (0, 2, 5), 5) for k in range(3)]


def test_scene_order_merge_and_state_round_trip():
    from segdino3d_amd import dist_eval, eval_box
    d = dev()
    scenes = _three_scenes()
    acc, want, (ap, ar) = _check(scenes, 6, d)
    assert np.isfinite(ap[[0, 2, 5]]).all() and np.isnan(ap[[1, 3, 4]]).all() and 0.0 < np.nanmean(ap) < 1.0
    new = lambda: eval_box.BoxApAccumulator(tuple(range(6)), _names(6))                  # noqa: E731
    other, first, second = new(), new(), new()
    for k in (2, 0, 1):
        other.add_boxes(*_dev_scene(scenes[k], d))
    ap2, ar2 = other.tables()
    assert ap2.tobytes() == ap.tobytes() and ar2.tobytes() == ar.tobytes()               # bit-identical in another order
    first.add_boxes(*_dev_scene(scenes[0], d))
    for k in (1, 2):
        second.add_boxes(*_dev_scene(scenes[k], d))
    gathered = dist_eval.all_gather_records(second.state())
    merged = eval_box.BoxApAccumulator.merge(gathered + [first.state(), new().state()])
    _assert_entries(new().entries(merged), want)
    ap3, ar3 = new().tables(merged.cpu())                                                # a gathered state may arrive on the host
    assert ap3.tobytes() == ap.tobytes() and ar3.tobytes() == ar.tobytes()
    ap4, ar4 = acc.tables(acc.state())                                                   # round trip, and tables() twice
    assert ap4.tobytes() == ap.tobytes() and ar4.tobytes() == ar.tobytes()
    res = acc.result()
    wres = R.result(ap, ar, _names(6), THR)
    assert res.keys() == wres.keys() and "mAP_0.25" in res and "c2_rec_0.50" in res
    assert all(res[k] == wres[k] or (np.isnan(res[k]) and np.isnan(wres[k])) for k in res)
    e_ap, e_ar = new().tables()
    assert np.isnan(e_ap).all() and np.isnan(e_ar).all() and e_ap.shape == (6, 2)


def test_a_full_store_sets_the_status():
    from segdino3d_amd import eval_box
    d = dev()
    s = R.make_scene(9, 40, 3, (0, 1), 3)
    acc = eval_box.BoxApAccumulator((0, 1, 2), _names(3))
    acc.max_slots = 2 * 40 + 50
    acc.add_boxes(*_dev_scene(s, d))
    assert acc.entries()["status"] == 0
    acc.add_boxes(*_dev_scene(s, d))                                                     # 80 more slots, 50 fit
    e = acc.entries()
    assert e["status"] == R.STORE_FULL and acc.used == 130 and acc._store.numel() == 130 and len(e["group"]) == 130
    with pytest.raises(RuntimeError, match="entry store"):
        acc.tables()


def _ann_scene(seed, N, n, d):
    """Points, evaluator-style annotations (two stuff classes in front, ids before map_inst_markup) and mask predictions."""
    rng = np.random.RandomState(seed)
    pts = rng.uniform(0.0, 4.0, size=(N, 6)).astype(np.float32)
    cell = (pts[:, 0] // 1.0).astype(np.int64) + 4 * (pts[:, 1] // 2.0).astype(np.int64)   # 8 instances, spatially compact
    inst = cell + 2
    sem = 2 + cell % 3
    inst[cell == 7], sem[cell == 7] = 1, 1                                               # a stuff region
    masks = np.zeros((n, N), dtype=bool)
    for r in range(n):
        masks[r] = (cell == rng.randint(8)) & (rng.rand(N) < 0.9)
    ann = dict(pts_semantic_mask=torch.from_numpy(sem).to(d), pts_instance_mask=torch.from_numpy(inst).to(d))
    pred = dict(pts_instance_mask=[torch.from_numpy(masks).to(d)], instance_labels=torch.from_numpy(rng.randint(0, 3, n)).to(d),
                instance_scores=torch.from_numpy(rng.rand(n).astype(np.float32)).to(d),
                instance_boxes=torch.from_numpy(np.concatenate([rng.uniform(0, 4, (n, 3)), rng.uniform(0.5, 2, (n, 3))], 1).astype(np.float32)).to(d))
    return torch.from_numpy(pts).to(d), ann, pred, (pts, sem, inst)


THINGS, THING_NAMES = (10, 11, 12), ("a", "b", "c")


def test_boxes_from_masks_equal_add_boxes_on_the_same_boxes():
    from segdino3d_amd import eval_box, ops
    d = dev()
    pts, ann, pred, (pts_h, sem_h, inst_h) = _ann_scene(3, 3000, 24, d)
    acc = eval_box.BoxApAccumulator(THINGS, THING_NAMES, num_stuff_cls=2, pred_boxes="masks")
    acc.add(ann, pred, pts)
    corners_w, cls_w, status_w = R.gt_boxes(pts_h, sem_h, inst_h, THINGS, num_stuff=2)
    assert status_w == 0 and (cls_w >= 0).sum() == 7
    status = torch.zeros(1, dtype=torch.int64, device=d)
    id_map = torch.tensor(list(THINGS) + [-1], dtype=torch.int64, device=d)
    corners, cls = ops.gt_boxes(pts, ann["pts_semantic_mask"], ann["pts_instance_mask"], _lut(THINGS, d), 3, status, id_map=id_map, num_stuff=2)
    assert int(status.item()) == 0 and np.array_equal(cls.cpu().numpy(), cls_w) and corners.cpu().numpy().tobytes() == corners_w.tobytes()
    boxes = torch.cat(ops.instance_boxes(pts, pred["pts_instance_mask"][0], "median"), dim=1)
    other = eval_box.BoxApAccumulator(THINGS, THING_NAMES, num_stuff_cls=2)
    other.add_boxes(corners, cls, boxes, pred["instance_labels"], pred["instance_scores"])
    e, eo = acc.entries(), other.entries()
    for k in ("group", "score", "true", "npos", "has_pred"):
        assert e[k].tobytes() == eo[k].tobytes(), k
    assert e["status"] == 0 and len(e["group"]) == 48 and e["true"].sum() > 0 and e["npos"].sum() == 7
    # and the head's boxes through add(): the restatement on the same numbers
    head = eval_box.BoxApAccumulator(THINGS, THING_NAMES, num_stuff_cls=2)
    head.add(ann, pred, pts)
    ref = R.scene(corners_w, cls_w, pred["instance_boxes"].cpu().numpy(), pred["instance_labels"].cpu().numpy(),
                  pred["instance_scores"].cpu().numpy(), 3, THR)
    _assert_margin([ref], THR)
    _assert_entries(head.entries(), R.accumulate([ref], 3))


def test_add_on_a_forward_result_equals_add_boxes():
    import segdino3d_amd as seg
    from segdino3d_amd import eval_ap, eval_box, ops
    from segdino3d_amd.configs import scannet200_model_cfg
    from segdino3d_amd.synth import make_scene, sharpen_random_model, structure_scene
    d = dev()
    pts, tgt = make_scene(21, n_points=8000, n_superpoints=64, n_query2d=8)
    structure_scene(pts, tgt)
    cfg = scannet200_model_cfg(query_num=-1)
    cfg["test_cfg"]["npoint_thr"] = 20
    torch.manual_seed(0)
    model = sharpen_random_model(seg.build_architecture(cfg).eval()).to(d)
    model.to_host = False
    N = pts.shape[0]
    block = torch.arange(N) * 6 // N                                                     # six ground-truth masks: two stuff, four things
    tgt.masks = torch.stack([block == k for k in range(6)])[:, :, None]
    tgt.labels = torch.tensor([0, 1, 5, 9, 9, 150])
    with torch.no_grad():
        out = model([pts.to(d)], [tgt.to(d)])[0]
    pred = out.pred_pts_seg
    n = pred.instance_scores.shape[0]
    assert n > 0 and tuple(pred.instance_boxes.shape) == (n, 6) and pred.instance_boxes.is_cuda
    classes = tuple(f"c{i}" for i in range(200)) + ("unlabeled",)
    valid = tuple(range(1, 201))
    ann = eval_ap.eval_ann_info(out, 200)
    points = pts.to(d)
    acc = eval_box.BoxApAccumulator(valid[2:], classes[2:-1], num_stuff_cls=2)
    acc.add(ann, pred, points)
    status = torch.zeros(1, dtype=torch.int64, device=d)
    id_map = torch.tensor(list(valid[2:]) + [-1], dtype=torch.int64, device=d)
    corners, cls = ops.gt_boxes(points, ann["pts_semantic_mask"], ann["pts_instance_mask"], _lut(valid[2:], d), 198, status, id_map=id_map,
                                num_stuff=2)
    other = eval_box.BoxApAccumulator(valid[2:], classes[2:-1], num_stuff_cls=2)
    other.add_boxes(corners, cls, pred.instance_boxes, pred.instance_labels, pred.instance_scores)
    e, eo = acc.entries(), other.entries()
    for k in ("group", "score", "true", "npos", "has_pred"):
        assert e[k].tobytes() == eo[k].tobytes(), k
    assert e["status"] == 0 and int(status.item()) == 0 and len(e["group"]) == 2 * n
    assert e["npos"].sum() == 4 and e["npos"][[3, 7, 148]].tolist() == [1, 2, 1]
    res = eval_box.evaluator_box_metrics([(ann, pred)], [points], classes, valid, 2)
    ap, ar = acc.tables()
    assert res["mAP_0.25"] == float(np.nanmean(ap[:, 0])) and f"{classes[5]}_AP_0.50" in res


def test_add_does_not_synchronise():
    from segdino3d_amd import eval_box
    d = dev()
    pts, ann, pred, _ = _ann_scene(5, 3000, 24, d)
    head = eval_box.BoxApAccumulator(THINGS, THING_NAMES, num_stuff_cls=2, device=d)
    masks = eval_box.BoxApAccumulator(THINGS, THING_NAMES, num_stuff_cls=2, pred_boxes="masks", device=d)
    head.STORE_CHUNK = masks.STORE_CHUNK = 64                                            # the stores grow under the sync check
    head.add(ann, pred, pts)                                                             # first calls: allocations, library load
    masks.add(ann, pred, pts)
    one = head.entries()
    half = dict(pred, instance_scores=pred["instance_scores"].half())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(20):
            head.add(ann, pred, pts)
            masks.add(ann, half, pts)
        state = head.state()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert head._store.numel() >= 21 * 48 > 4 * 64
    assert state.is_cuda and state.dtype == torch.float64 and state.dim() == 2 and state.shape[1] == head.STATE_WIDTH
    e = head.entries()
    assert e["status"] == 0 and masks.entries()["status"] == 0 and len(one["group"]) == 48
    assert np.array_equal(np.bincount(e["group"]), 21 * np.bincount(one["group"])) and e["true"].sum() == 21 * one["true"].sum()
    assert np.array_equal(e["npos"], 21 * one["npos"])
