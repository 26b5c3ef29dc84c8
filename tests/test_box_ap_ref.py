"""The numpy restatement of the 3D box AP / AR protocol (tests/box_ap_ref.py) on hand-computed cases, its invariances, and the host
side of segdino3d_amd/eval_box.py that needs no device (the metrics dictionary, argument checks).  No GPU."""
import numpy as np
import pytest

import box_ap_ref as R

THR = (0.25, 0.5)


def _cube(lo, hi):
    return np.array([list(lo) + list(hi)], dtype=np.float32)


def _centre_size(lo, hi):
    lo, hi = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    return np.concatenate([(lo + hi) / 2, hi - lo]).astype(np.float32)


def test_one_ground_truth_two_duplicate_predictions():
    gt = _cube((0, 0, 0), (1, 1, 1))
    box = _centre_size((0, 0, 0), (1, 1, 1))
    s = R.scene(gt, [0], np.stack([box, box]), [0, 0], [0.8, 0.9], 1, THR)
    group, score, true, npos, has_pred, status = R.accumulate([s], 1)
    assert status == 0 and npos.tolist() == [1] and has_pred.tolist() == [True]
    assert group.tolist() == [0, 0, 1, 1] and true.tolist() == [0, 1, 0, 1]              # the higher score took it, the duplicate is a fp
    assert score.tolist() == [np.float32(0.8), np.float32(0.9)] * 2
    ap, ar = R.finish(group, score, true, npos, 2)
    assert ap.tolist() == [[1.0, 1.0]] and ar.tolist() == [[1.0, 1.0]]
    # equal scores: the lower row takes it
    s = R.scene(gt, [0], np.stack([box, box]), [0, 0], [0.5, 0.5], 1, THR)
    assert [e[2] for e in s["entries"]] == [1, 1, 0, 0]


def test_iou_exactly_at_the_threshold_is_a_false_positive():
    gt = _cube((0, 0, 0), (1, 1, 0.5))
    box = _centre_size((0, 0, 0), (1, 1, 1))
    assert R.iou_to_all(box, gt).tolist() == [0.5]                                       # exact in binary
    s = R.scene(gt, [0], box[None], [0], [0.7], 1, THR)
    assert sorted(s["entries"]) == [(0, np.float32(0.7), 1), (1, np.float32(0.7), 0)]    # tp at 0.25, fp at 0.5
    ap, ar = R.tables([s], 1, 2)
    assert ap.tolist() == [[1.0, 0.0]] and ar.tolist() == [[1.0, 0.0]]


def test_no_second_choice_and_lowest_column_on_equal_iou():
    # ground truths 0 and 1 overlap; both predictions fit 0 best, the second one still passes 0.25 on ground truth 1: it stays a fp
    gt = np.concatenate([_cube((0, 0, 0), (1, 1, 1)), _cube((0, 0, 0.5), (1, 1, 1.5))])
    a = _centre_size((0, 0, 0), (1, 1, 1))
    b = _centre_size((0, 0, 0.125), (1, 1, 1.125))
    v = R.iou_to_all(b, gt)
    assert v[0] > v[1] > 0.25
    s = R.scene(gt, [0, 0], np.stack([a, b]), [0, 0], [0.9, 0.8], 1, (0.25,))
    assert s["entries"] == [(0, np.float32(0.9), 1), (0, np.float32(0.8), 0)] and s["npos"].tolist() == [2]
    # a prediction midway between two equal ground truths: the lower column is taken, the higher one stays free for the next
    gt = np.concatenate([_cube((0, 0, 0), (1, 1, 1)), _cube((0, 0, 1), (1, 1, 2))])
    mid = _centre_size((0, 0, 0.5), (1, 1, 1.5))
    v = R.iou_to_all(mid, gt)
    assert v[0] == v[1] == 1.0 / 3.0
    s = R.scene(gt, [0, 0], np.stack([mid, mid]), [0, 0], [0.9, 0.8], 1, (0.25,))
    assert [e[2] for e in s["entries"]] == [1, 0]


def test_class_cases():
    gt = np.concatenate([_cube((0, 0, 0), (1, 1, 1)), _cube((3, 3, 3), (4, 4, 4))])
    box = _centre_size((0, 0, 0), (1, 1, 1))
    # class 0: ground truth and a hit; class 1: ground truth, no prediction; class 2: a prediction, no ground truth; class 3: nothing
    s = R.scene(gt, [0, 1], np.stack([box, box]), [0, 2], [0.9, 0.8], 4, THR)
    ap, ar = R.tables([s], 4, 2)
    assert ap[0].tolist() == [1.0, 1.0] and ap[1].tolist() == [0.0, 0.0] and ar[1].tolist() == [0.0, 0.0]
    assert np.isnan(ap[2:]).all() and np.isnan(ar[2:]).all()
    res = R.result(ap, ar, ("a", "b", "c", "d"), THR)
    assert res["mAP_0.25"] == 0.5 and res["mAR_0.50"] == 0.5 and res["b_AP_0.50"] == 0.0 and np.isnan(res["c_rec_0.25"])
    from segdino3d_amd import eval_box
    mine = eval_box.metrics_dict(ap, ar, ("a", "b", "c", "d"), THR)
    assert mine.keys() == res.keys() and all(mine[k] == res[k] or (np.isnan(mine[k]) and np.isnan(res[k])) for k in res)
    empty = eval_box.metrics_dict(np.full((2, 2), np.nan), np.full((2, 2), np.nan), ("a", "b"), THR)
    assert np.isnan(empty["mAP_0.25"]) and np.isnan(empty["mAR_0.50"])


def test_left_out_inputs_set_their_bit():
    gt = _cube((0, 0, 0), (1, 1, 1))
    box = _centre_size((0, 0, 0), (1, 1, 1))
    neg = box.copy(); neg[4] = -1.0
    for boxes, label, score, bit in ((neg, 0, 0.5, R.BAD_BOX), (box, 3, 0.5, R.BAD_LABEL), (box, 0, np.inf, R.BAD_SCORE)):
        s = R.scene(gt, [0], np.stack([box, boxes]), [0, label], [0.9, score], 3, THR)
        assert s["status"] == bit and len(s["entries"]) == 2 and s["has_pred"].tolist() == [True, False, False]
    s = R.scene(_cube((0, 0, 0), (1, 1, -1)), [0], box[None], [0], [0.9], 1, THR)
    assert s["status"] == R.BAD_COORD and s["npos"].tolist() == [0]


def test_tables_do_not_depend_on_scene_or_row_order():
    C = 5
    scenes = [R.make_scene(10 + k, 60, C, (0, 2, 3), 4, distinct_scores=True) for k in range(4)]
    base = R.tables([R.scene_of(s, C, THR) for s in scenes], C, 2)
    assert np.nanmin(base[0]) < 1.0 and np.nanmax(base[0]) > 0.0 and np.isnan(base[0][1]).all()
    for perm in ((3, 1, 0, 2), (1, 2, 3, 0)):
        got = R.tables([R.scene_of(scenes[k], C, THR) for k in perm], C, 2)
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes()
    rng = np.random.RandomState(0)
    shuffled = []
    for s in scenes:
        p = rng.permutation(len(s["labels"]))
        shuffled.append(dict(s, boxes=s["boxes"][p], labels=s["labels"][p], scores=s["scores"][p]))
    got = R.tables([R.scene_of(s, C, THR) for s in shuffled], C, 2)
    assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes()
    # tied scores: scene order still moves nothing (true before false is part of the sort key)
    tied = [R.make_scene(30 + k, 60, C, (0, 2, 3), 4) for k in range(3)]
    a = R.tables([R.scene_of(s, C, THR) for s in tied], C, 2)
    b = R.tables([R.scene_of(s, C, THR) for s in tied[::-1]], C, 2)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_ground_truth_boxes_of_the_restatement():
    pts = np.array([[-1.0, -2.0, -3.0], [-0.5, -0.0, -4.0], [2.0, 0.0, 1.0], [7.0, 7.0, 7.0], [9.0, 9.0, 9.0]], dtype=np.float32)
    sem = np.array([5, 5, 5, 6, 4])
    inst = np.array([3, 3, 3, 0, -1])
    corners, cls, status = R.gt_boxes(pts, sem, inst, (5, 6))
    assert status == 0 and cls[3] == 0 and cls[0] == 1 and (cls >= 0).sum() == 2
    assert corners[3].tolist() == [-1.0, -2.0, -4.0, 2.0, 0.0, 1.0]
    assert not np.signbit(corners[3, 4])                                               # max(-2, -0, 0) is +0
    assert corners[0].tolist() == [7.0] * 6                                            # one point: a zero-size box
    _, cls, status = R.gt_boxes(pts, np.array([5, 6, 5, 6, 4]), inst, (5, 6))
    assert status == R.MIXED_SEMANTIC and cls[3] == 1
    bad = pts.copy(); bad[1, 2] = np.nan
    _, cls, status = R.gt_boxes(bad, sem, inst, (5, 6))
    assert status == R.BAD_COORD and cls[3] == -1 and cls[0] == 1
    # through map_inst_markup: two stuff classes, thing ids 2.. -> valid_class_ids
    _, cls, status = R.gt_boxes(pts, np.array([2, 2, 2, 3, 0]), np.array([5, 5, 5, 2, 1]), (5, 6), num_stuff=2)
    assert status == 0 and cls[3] == 0 and cls[0] == 1 and (cls >= 0).sum() == 2


def test_accumulator_argument_checks():
    from segdino3d_amd import eval_box
    with pytest.raises(ValueError, match="iou_thr"):
        eval_box.BoxApAccumulator((1, 2), ("a", "b"), iou_thr=(0.5, 1.0))
    with pytest.raises(ValueError, match="pred_boxes"):
        eval_box.BoxApAccumulator((1, 2), ("a", "b"), pred_boxes="both")
    acc = eval_box.BoxApAccumulator((1, 2), ("a", "b"))
    assert acc.iou_thr == (0.25, 0.5) and acc.n_counters == 4 and acc.slots_per_pred == 2
    state = acc.state()                                                                # no scene yet: lives on the host
    assert tuple(state.shape) == (2, acc.STATE_WIDTH) and state.dtype.is_floating_point
    e = acc.entries(eval_box.BoxApAccumulator.merge([state, state]))
    assert len(e["group"]) == 0 and e["npos"].tolist() == [0, 0] and e["status"] == 0
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        acc.add_boxes(torch.zeros(1, 6), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 6), torch.zeros(1, dtype=torch.long), torch.zeros(1))
