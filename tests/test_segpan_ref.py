"""The numpy restatement of the semantic / panoptic protocols (tests/segpan_ref.py) against numbers worked by hand, and the host
side of segdino3d_amd/eval_seg.py (state merge, status, dictionary arithmetic).  No GPU."""
import math

import numpy as np
import pytest
import torch

import segpan_ref as R
from segdino3d_amd import eval_seg

# the worked example: C = 4 (0 stuff; 1, 2 things; 3 ignored), N = 12
GT_SEM = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3])
GT_INST = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, -1, -1])
PRED_SEM = np.array([0, 0, 0, 1, 1, 1, 1, 2, 2, 1, 0, 0])
PRED_INST = np.array([0, 0, 0, 2, 2, 2, 2, 3, 3, 4, 0, 0])
NAMES = ["floor", "chair", "table", "unlabeled"]
L2C = {i: n for i, n in enumerate(NAMES)}


def test_worked_example_semantic():
    hist = R.confusion([GT_SEM], [PRED_SEM], 4, 3)
    assert hist.tolist() == [[3, 1, 0, 0], [0, 3, 1, 0], [0, 1, 1, 0], [0, 0, 0, 0]]
    ret = R.seg_eval([GT_SEM], [PRED_SEM], L2C, 3)
    assert ret["floor"] == pytest.approx(0.75, abs=1e-15) and ret["chair"] == pytest.approx(0.5, abs=1e-15)
    assert ret["table"] == pytest.approx(1 / 3, abs=1e-15) and math.isnan(ret["unlabeled"])
    assert ret["miou"] == pytest.approx(19 / 36, abs=1e-15)
    assert ret["acc"] == pytest.approx(0.7, abs=1e-15)
    assert ret["acc_cls"] == pytest.approx(2 / 3, abs=1e-15)


def test_worked_example_panoptic():
    tp, fp, fn, iou, n_matches = R.panoptic_counts([GT_SEM], [GT_INST], [PRED_SEM], [PRED_INST], 4, [3], 1)
    assert tp[:3].tolist() == [1, 1, 0] and fp[:3].tolist() == [0, 1, 1] and fn[:3].tolist() == [0, 0, 1]
    assert iou[:3].tolist() == [0.75, 0.6, 0.0] and n_matches == 2
    assert tp[3] == fp[3] == fn[3] == 0 and iou[3] == 0.0
    gt = [dict(pts_semantic_mask=GT_SEM, pts_instance_mask=GT_INST)]
    pred = [dict(pts_semantic_mask=PRED_SEM, pts_instance_mask=PRED_INST)]
    ret = R.panoptic_seg_eval(gt, pred, NAMES, NAMES[1:3], NAMES[:1], 1, 2 ** 16, L2C, [3])
    assert [ret["classes"][n]["pq"] for n in NAMES[:3]] == pytest.approx([0.75, 0.4, 0.0], abs=1e-15)
    assert ret["pq"] == pytest.approx(23 / 60, abs=1e-15)
    assert ret["pq_stuff"] == pytest.approx(0.75, abs=1e-15) and ret["pq_thing"] == pytest.approx(0.2, abs=1e-15)
    # min_num_points = 2: the one-point prediction of class 1 is no longer a false positive
    tp2, fp2, fn2, _, _ = R.panoptic_counts([GT_SEM], [GT_INST], [PRED_SEM], [PRED_INST], 4, [3], 2)
    assert tp2[:3].tolist() == [1, 1, 0] and fp2[:3].tolist() == [0, 0, 1] and fn2[:3].tolist() == [0, 0, 1]
    ret2 = R.panoptic_seg_eval(gt, pred, NAMES, NAMES[1:3], NAMES[:1], 2, 2 ** 16, L2C, [3])
    assert ret2["pq"] == pytest.approx(0.45, abs=1e-15)


def test_iou_of_exactly_one_half_is_no_match():
    # gt area 3, prediction area 3, intersection 2: iou = 2 / 4
    gs = np.array([1, 1, 1, 1, 0])
    gi = np.array([5, 5, 5, -1, -1])
    ps = np.array([0, 1, 1, 1, 0])
    pi = np.array([-1, 9, 9, 9, -1])
    tp, fp, fn, iou, n = R.panoptic_counts([gs], [gi], [ps], [pi], 2, [], 1)
    assert tp.tolist() == [0, 0] and fp.tolist() == [0, 1] and fn.tolist() == [0, 1] and iou.tolist() == [0.0, 0.0] and n == 0


def test_generator_gives_work_on_all_three_counts():
    """The seeded scenes the GPU tests use are not empty work: tp, fp and fn are all positive and min_num_points changes fp / fn."""
    scenes = [R.make_scene(100 + s, 3000, 11) for s in range(4)]
    gs, gi, ps, pi = (list(x) for x in zip(*scenes))
    tp1, fp1, fn1, _, _ = R.panoptic_counts(gs, gi, ps, pi, 11, [10], 1)
    tp50, fp50, fn50, _, _ = R.panoptic_counts(gs, gi, ps, pi, 11, [10], 50)
    assert tp1.sum() > 0 and fp1.sum() > 0 and fn1.sum() > 0
    assert tp1.tolist() == tp50.tolist()
    assert (fp1.sum(), fn1.sum()) != (fp50.sum(), fn50.sum())


def _state(C, seed, status=0):
    g = np.random.default_rng(seed)
    conf = g.integers(0, 1000, size=C * C)
    tp, fp, fn = (g.integers(0, 50, size=C) for _ in range(3))
    iou = g.random(C) * tp
    return torch.from_numpy(np.concatenate([conf, tp, fp, fn, iou, [status]]).astype(np.float64))


def test_merge_sums_states_and_status_raises():
    C = 5
    acc = eval_seg.SegPanAccumulator(C, [4], [0], [1, 2, 3], 1, device="cpu")
    assert acc.width == C * C + 4 * C + 1 and acc.state().shape == (acc.width,) and float(acc.state().abs().sum()) == 0.0
    a, b = _state(C, 1), _state(C, 2)
    m = eval_seg.SegPanAccumulator.merge([a, b])
    assert torch.equal(m, a + b)
    # rows as all_gather_records returns them ([n_local, width] per rank), an empty rank included
    m2 = eval_seg.SegPanAccumulator.merge([a[None], torch.zeros(0, acc.width, dtype=torch.float64), b[None]])
    assert torch.equal(m2, a + b)
    c = acc.counts(m)
    assert c["confusion"].shape == (C, C) and c["confusion"].dtype == np.int64
    assert c["confusion"].ravel().tolist() == (a + b)[:C * C].long().tolist()
    assert c["tp"].tolist() == (a + b)[C * C:C * C + C].long().tolist()
    assert np.array_equal(c["iou_sum"], (a + b)[C * C + 3 * C:C * C + 4 * C].numpy())
    r = acc.result(classes=["a", "b", "c", "d", "e"], state=m)
    assert set(r) == {"seg", "pan"} and 0.0 <= r["pan"]["pq"] <= 1.0
    # status words are OR-ed, not added, and a set status raises with the name of the bit
    bad = eval_seg.SegPanAccumulator.merge([_state(C, 3, status=1), _state(C, 4, status=1), _state(C, 5, status=2)])
    assert float(bad[-1]) == 3.0
    with pytest.raises(RuntimeError, match="semantic prediction lies outside"):
        acc.result(state=bad)
    with pytest.raises(RuntimeError, match="instance id"):
        acc.result(state=_state(C, 6, status=2))
    with pytest.raises(RuntimeError, match="segments"):
        acc.counts(_state(C, 7, status=4))


def test_add_refuses_cpu_tensors():
    acc = eval_seg.SegPanAccumulator(4, [3], [0], [1, 2], 1)
    ann = dict(pts_semantic_mask=torch.from_numpy(GT_SEM), pts_instance_mask=torch.from_numpy(GT_INST))
    pred = dict(pts_semantic_mask=[torch.from_numpy(PRED_SEM)] * 2, pts_instance_mask=[None, torch.from_numpy(PRED_INST)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        acc.add(ann, pred)
    with pytest.raises(ValueError, match="id_offset"):
        eval_seg.SegPanAccumulator(4, [3], [0], [1, 2], 1, id_offset=1000)


def test_dictionary_arithmetic_from_counts():
    # the worked example's counts through the package's arithmetic
    conf = [[3, 1, 0, 0], [0, 3, 1, 0], [0, 1, 1, 0], [0, 0, 0, 0]]
    seg = eval_seg.seg_metrics(conf, L2C, 3)
    assert seg["miou"] == pytest.approx(19 / 36, abs=1e-15) and seg["acc"] == pytest.approx(0.7, abs=1e-15)
    assert seg["acc_cls"] == pytest.approx(2 / 3, abs=1e-15) and seg["table"] == pytest.approx(1 / 3, abs=1e-15)
    assert math.isnan(seg["unlabeled"])
    pan = eval_seg.panoptic_metrics([1, 1, 0, 0], [0, 1, 1, 0], [0, 0, 1, 0], [0.75, 0.6, 0.0, 0.0], NAMES, NAMES[1:3], NAMES[:1], L2C, [3])
    assert pan["pq"] == pytest.approx(23 / 60, abs=1e-15)
    assert pan["classes"]["chair"] == pytest.approx({"pq": 0.4, "sq": 0.6, "rq": 2 / 3}, abs=1e-15)
    assert pan["sq"] == pytest.approx((0.75 + 0.6 + 0.0) / 3, abs=1e-15) and pan["rq"] == pytest.approx((1 + 2 / 3 + 0) / 3, abs=1e-15)
    assert pan["pq_thing"] == pytest.approx(0.2, abs=1e-15) and pan["pq_stuff"] == pytest.approx(0.75, abs=1e-15)
    assert "unlabeled" not in pan["classes"]
    # a class seen nowhere: NaN in the semantic mean (left out), 0 in the panoptic mean (counted)
    conf5 = np.zeros((5, 5), dtype=np.int64)
    conf5[:4, :4] = conf
    conf5[3, 3] = 0
    names5 = ["floor", "chair", "table", "lamp", "unlabeled"]
    l2c5 = {i: n for i, n in enumerate(names5)}
    seg5 = eval_seg.seg_metrics(conf5, l2c5, 4)
    assert math.isnan(seg5["lamp"]) and seg5["miou"] == pytest.approx(19 / 36, abs=1e-15)
    pan5 = eval_seg.panoptic_metrics([1, 1, 0, 0, 0], [0, 1, 1, 0, 0], [0, 0, 1, 0, 0], [0.75, 0.6, 0, 0, 0], names5, names5[1:4], names5[:1],
                                     l2c5, [4])
    assert pan5["classes"]["lamp"] == {"pq": 0.0, "sq": 0.0, "rq": 0.0}
    assert pan5["pq"] == pytest.approx((0.75 + 0.4) / 4, abs=1e-15)
    # an all-ignored scene: nothing counted anywhere
    seg0 = eval_seg.seg_metrics(np.zeros((4, 4)), L2C, 3)
    assert math.isnan(seg0["miou"]) and math.isnan(seg0["acc"]) and math.isnan(seg0["acc_cls"])
    pan0 = eval_seg.panoptic_metrics([0] * 4, [0] * 4, [0] * 4, [0.0] * 4, NAMES, NAMES[1:3], NAMES[:1], L2C, [3])
    assert pan0["pq"] == 0.0 and pan0["sq"] == 0.0 and pan0["rq"] == 0.0 and pan0["pq_thing"] == 0.0


def test_package_arithmetic_equals_the_restatement_on_seeded_scenes():
    scenes = [R.make_scene(200 + s, 2000, 11) for s in range(3)]
    gs, gi, ps, pi = (list(x) for x in zip(*scenes))
    names = [f"c{i}" for i in range(11)]
    l2c = {i: n for i, n in enumerate(names)}
    want_seg = R.seg_eval(gs, ps, l2c, 10)
    got_seg = eval_seg.seg_metrics(R.confusion(gs, ps, 11, 10), l2c, 10)
    for k, v in want_seg.items():
        assert (math.isnan(v) and math.isnan(got_seg[k])) or got_seg[k] == pytest.approx(v, abs=1e-15), k
    tp, fp, fn, iou, _ = R.panoptic_counts(gs, gi, ps, pi, 11, [10], 1)
    got = eval_seg.panoptic_metrics(tp, fp, fn, iou, names, names[2:10], names[:2], l2c, [10])
    want = R.panoptic_seg_eval([dict(pts_semantic_mask=a, pts_instance_mask=b) for a, b in zip(gs, gi)],
                               [dict(pts_semantic_mask=a, pts_instance_mask=b) for a, b in zip(ps, pi)],
                               names, names[2:10], names[:2], 1, 2 ** 16, l2c, [10])
    for k in ("pq", "sq", "rq", "pq_thing", "sq_thing", "rq_thing", "pq_stuff", "sq_stuff", "rq_stuff"):
        assert got[k] == pytest.approx(want[k], abs=1e-15), k
    assert got["classes"] == want["classes"]
