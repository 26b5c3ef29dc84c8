"""segdino3d_amd/eval_seg.py + csrc/segeval.hip against the numpy restatement of the two protocols (tests/segpan_ref.py).

Integer outputs (confusion, tp, fp, fn) must equal the restatement's bit for bit; iou_sum within n_matches * 2^-52 relative (a float64
sum of that many terms in another order - every term is the same correctly rounded quotient of two integers); two runs of the device
path on one input must give identical bits."""
import numpy as np
import pytest
import torch

import segpan_ref as R

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _t(a, d, strided=False):
    a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))
    if not strided:
        return a.to(d)
    wide = torch.full((a.numel(), 3), -7, dtype=torch.int64)
    wide[:, 1] = a
    v = wide.to(d)[:, 1]
    assert v.numel() < 2 or v.stride(0) == 3
    return v


def _device_counts(scenes, C, ignore, min_pts, d, strided=False, sem_preds=None):
    """scenes: (gt_sem, gt_inst, pred_sem, pred_inst) numpy arrays; the semantic task scores `sem_preds` (default: pred_sem)."""
    from segdino3d_amd import eval_seg
    acc = eval_seg.SegPanAccumulator(C, ignore, [0, 1], list(range(2, C - 1)), min_pts)
    for k, (gs, gi, ps, pi) in enumerate(scenes):
        sp = ps if sem_preds is None else sem_preds[k]
        ann = dict(pts_semantic_mask=_t(gs, d, strided), pts_instance_mask=_t(gi, d, strided))
        pred = dict(pts_semantic_mask=[_t(sp, d, strided), _t(ps, d, strided)], pts_instance_mask=[None, _t(pi, d, strided)])
        acc.add(ann, pred)
    return acc, acc.counts()


def _check(scenes, C, ignore, min_pts, d, strided=False):
    gs, gi, ps, pi = (list(x) for x in zip(*scenes))
    conf = R.confusion(gs, ps, C, ignore[0] if ignore else -1)
    tp, fp, fn, iou, n_matches = R.panoptic_counts(gs, gi, ps, pi, C, ignore, min_pts)
    acc, got = _device_counts(scenes, C, ignore, min_pts, d, strided)
    assert np.array_equal(got["confusion"], conf)
    assert np.array_equal(got["tp"], tp), (got["tp"], tp)
    assert np.array_equal(got["fp"], fp), (got["fp"], fp)
    assert np.array_equal(got["fn"], fn), (got["fn"], fn)
    bound = max(n_matches, 1) * 2.0 ** -52
    assert np.all(np.abs(got["iou_sum"] - iou) <= bound * np.abs(iou)), (got["iou_sum"], iou)
    _, again = _device_counts(scenes, C, ignore, min_pts, d, strided)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    return dict(tp=tp, fp=fp, fn=fn, iou=iou, conf=conf, n_matches=n_matches)


@pytest.mark.parametrize("C", [11, 201])
@pytest.mark.parametrize("N", [1, 63, 65, 1007, 20011])
def test_generated_scene_equals_the_restatement(N, C):
    d = dev()
    scene = R.make_scene(1000 + N + C, N, C, n_runs=max(14, N // 200))
    for strided in (False, True):
        _check([scene], C, [C - 1], 1, d, strided)


@pytest.mark.parametrize("C", [11, 201])
def test_one_bin_and_uniformly_random_labels(C):
    d = dev()
    N = 20011
    one = (np.full(N, 3), np.full(N, 7), np.full(N, 3), np.full(N, 4))
    r = _check([one], C, [C - 1], 1, d)
    assert r["conf"][3, 3] == N and r["tp"][3] == 1
    g = np.random.default_rng(5)
    rnd = (g.integers(0, C, N), g.integers(-1, 40, N), g.integers(0, C, N), g.integers(-1, 40, N))
    r = _check([rnd], C, [C - 1], 1, d)
    assert r["fp"].sum() > 0 and r["fn"].sum() > 0


@pytest.mark.parametrize("C", [128, 129])
def test_either_side_of_the_lds_table_threshold(C):
    """C = 128 is the largest table a workgroup keeps in LDS (16 384 bins), C = 129 the first that goes to global memory; labels over
    the whole range so that the last bin is hit, more than one workgroup."""
    d = dev()
    N = 2500
    g = np.random.default_rng(C)
    gs, ps = np.repeat(g.integers(0, C, N // 4 + 1), 4)[:N], np.repeat(g.integers(0, C, N // 5 + 1), 5)[:N]
    gs[-1] = ps[-1] = C - 2
    gs[0], ps[0] = C - 2, 0
    r = _check([(gs, g.integers(-1, 30, N), ps, g.integers(-1, 30, N))], C, [C - 1], 1, d)
    assert r["conf"][C - 2, C - 2] >= 1 and r["conf"][C - 2, 0] >= 1 and r["conf"].sum() == (gs != C - 1).sum()


def test_four_scenes_accumulate_without_a_result_in_between():
    d = dev()
    C = 11
    scenes = [R.make_scene(100 + s, n, C) for s, n in enumerate((3000, 1007, 2500, 3001))]
    r1 = _check(scenes, C, [C - 1], 1, d)
    r50 = _check(scenes, C, [C - 1], 50, d)
    assert r1["tp"].sum() > 0 and r1["fp"].sum() > 0 and r1["fn"].sum() > 0
    assert (r1["fp"].sum(), r1["fn"].sum()) != (r50["fp"].sum(), r50["fn"].sum())


def test_edge_scenes():
    d = dev()
    C = 11
    gs, gi, ps, pi = R.make_scene(77, 1007, C)
    # every point ignored: nothing is counted anywhere, miou is NaN and pq 0
    acc, got = _device_counts([(np.full(1007, C - 1), gi, ps, pi)], C, [C - 1], 1, d)
    assert not got["confusion"].any() and not got["tp"].any() and not got["fp"].any() and not got["fn"].any()
    res = acc.result()
    assert np.isnan(res["seg"]["miou"]) and res["pan"]["pq"] == 0.0
    # no ground-truth instance at all: only false positives
    r = _check([(gs, np.full(1007, -1), ps, pi)], C, [C - 1], 1, d)
    assert r["tp"].sum() == 0 and r["fn"].sum() == 0 and r["fp"].sum() > 0
    # instance id 0 is a real segment (stuff class 0 on both sides), and one id under two classes is two segments
    gs2 = np.array([0] * 40 + [3] * 30 + [4] * 30)
    gi2 = np.array([0] * 40 + [5] * 30 + [5] * 30)
    ps2 = np.array([0] * 38 + [3] * 32 + [4] * 30)
    pi2 = np.array([0] * 38 + [9] * 62)
    r = _check([(gs2, gi2, ps2, pi2)], C, [C - 1], 1, d)
    assert r["tp"][0] == 1 and r["tp"][3] == 1 and r["tp"][4] == 1 and r["fp"].sum() == 0 and r["fn"].sum() == 0


def test_worked_examples_through_the_device():
    d = dev()
    gt_sem = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3])
    gt_inst = np.array([0, 0, 0, 0, 1, 1, 1, 1, 2, 2, -1, -1])
    pred_sem = np.array([0, 0, 0, 1, 1, 1, 1, 2, 2, 1, 0, 0])
    pred_inst = np.array([0, 0, 0, 2, 2, 2, 2, 3, 3, 4, 0, 0])
    from segdino3d_amd import eval_seg
    for min_pts, fp_want, pq_want in ((1, [0, 1, 1, 0], 23 / 60), (2, [0, 0, 1, 0], 0.45)):
        acc = eval_seg.SegPanAccumulator(4, [3], [0], [1, 2], min_pts)
        acc.add(dict(pts_semantic_mask=_t(gt_sem, d), pts_instance_mask=_t(gt_inst, d)),
                dict(pts_semantic_mask=[_t(pred_sem, d)] * 2, pts_instance_mask=[None, _t(pred_inst, d)]))
        c = acc.counts()
        assert c["confusion"].tolist() == [[3, 1, 0, 0], [0, 3, 1, 0], [0, 1, 1, 0], [0, 0, 0, 0]]
        assert c["tp"].tolist() == [1, 1, 0, 0] and c["fp"].tolist() == fp_want and c["fn"].tolist() == [0, 0, 1, 0]
        assert c["iou_sum"].tolist() == [0.75, 0.6, 0.0, 0.0]
        res = acc.result(classes=["floor", "chair", "table", "unlabeled"])
        assert res["seg"]["miou"] == pytest.approx(19 / 36, abs=1e-15) and res["seg"]["acc"] == pytest.approx(0.7, abs=1e-15)
        assert res["pan"]["pq"] == pytest.approx(pq_want, abs=1e-15)
    # iou of exactly 0.5 (areas 3 and 3, intersection 2) is no match: one fn and one fp
    gs, gi = np.array([1, 1, 1, 1, 0]), np.array([5, 5, 5, -1, -1])
    ps, pi = np.array([0, 1, 1, 1, 0]), np.array([-1, 9, 9, 9, -1])
    r = _check([(gs, gi, ps, pi)], 2, [], 1, d)
    assert r["tp"].tolist() == [0, 0] and r["fp"].tolist() == [0, 1] and r["fn"].tolist() == [0, 1]
    # the call shapes of the reference's commented lines
    l2c = {0: "floor", 1: "chair", 2: "table", 3: "unlabeled"}
    sem = eval_seg.seg_eval([_t(gt_sem, d)], [_t(pred_sem, d)], l2c, 3)
    want = R.seg_eval([gt_sem], [pred_sem], l2c, 3)
    assert all((np.isnan(v) and np.isnan(sem[k])) or sem[k] == pytest.approx(v, abs=1e-15) for k, v in want.items())
    pan = eval_seg.panoptic_seg_eval([dict(pts_semantic_mask=_t(gt_sem, d), pts_instance_mask=_t(gt_inst, d))],
                                     [dict(pts_semantic_mask=_t(pred_sem, d), pts_instance_mask=_t(pred_inst, d))],
                                     list(l2c.values()), ["chair", "table"], ["floor"], 1, 2 ** 16, l2c, [3])
    assert pan["pq"] == pytest.approx(23 / 60, abs=1e-15) and pan["pq_stuff"] == pytest.approx(0.75, abs=1e-15)


def _runs(n, n_runs, g, step=4):
    """Run edges at multiples of `step`: every run has at least `step` points."""
    bounds = np.sort(g.choice(np.arange(1, n // step), size=n_runs - 1, replace=False)) * step
    return [0] + bounds.tolist() + [n]


def test_300_ground_truth_and_602_predicted_segments():
    """More segments than any single-pass table of 256 entries holds, ids up to 601."""
    d = dev()
    N, C = 20011, 201
    g = np.random.default_rng(11)
    gs, gi, ps, pi = (np.zeros(N, dtype=np.int64) for _ in range(4))
    ge = _runs(N, 300, g)
    for k, (lo, hi) in enumerate(zip(ge[:-1], ge[1:])):
        gs[lo:hi], gi[lo:hi] = 2 + k % 190, k
    # every ground-truth run is predicted as two runs (the first two as three): the larger part usually matches, the rest are false positives
    k = 0
    for r, (lo, hi) in enumerate(zip(ge[:-1], ge[1:])):
        cut = [lo, lo + max(1, (hi - lo) // 3), hi] if r >= 2 else [lo, lo + 1, hi - 1, hi]
        for a, b in zip(cut[:-1], cut[1:]):
            ps[a:b], pi[a:b] = gs[lo] if g.random() > 0.1 else 2 + int(g.integers(190)), k
            k += 1
    assert len(np.unique(gi)) == 300 and len(np.unique(pi)) == 602
    r = _check([(gs, gi, ps, pi)], C, [C - 1], 1, d)
    assert r["tp"].sum() > 100 and r["fp"].sum() > 100 and r["fn"].sum() > 0


def test_status_bits_and_guarded_accumulators():
    """Out-of-range predictions set the status word, are skipped without a write outside the tables, and result() raises."""
    from segdino3d_amd import eval_seg, ops
    d = dev()
    C, G = 11, 512                                             # a page of int64 sentinels on either side of the accumulators
    width = C * C + 4 * C + 1
    SENT = -0x0123456789ABCDEF
    buf = torch.full((G + width + G,), SENT, dtype=torch.int64, device=d)
    buf[G:G + width] = 0
    o = G + C * C
    v = dict(confusion=buf[G:o], tp=buf[o:o + C], fp=buf[o + C:o + 2 * C], fn=buf[o + 2 * C:o + 3 * C],
             iou_sum=buf[o + 3 * C:o + 4 * C].view(torch.float64), status=buf[o + 4 * C:o + 4 * C + 1])
    gs, gi, ps, pi = R.make_scene(31, 1007, C)
    counted = np.flatnonzero(gs != C - 1)
    bad_sem = ps.copy()
    bad_sem[counted[3]] = C                                    # one past the table
    bad_sem[counted[500]] = -1
    bad_sem[counted[900]] = 2 ** 40
    bad_inst = pi.copy()
    bad_inst[counted[10]] = 2 ** 16                            # shifted: 2^16 + 1
    bad_inst[counted[11]] = -5                                 # shifted: -4

    def run():
        ops.semantic_confusion(_t(bad_sem, d), _t(gs, d), C, C - 1, v["confusion"], v["status"])
        ops.panoptic_accumulate(_t(ps, d), _t(bad_inst, d), _t(gs, d), _t(gi, d), C, [C - 1], 1, v["tp"], v["fp"], v["fn"], v["iou_sum"], v["status"])
    run()
    host = buf.cpu().numpy()
    assert (host[:G] == SENT).all() and (host[-G:] == SENT).all()
    assert int(host[G + width - 1]) == 1 | 2
    # what was legitimately counted: the three bad predictions skipped, the two bad ids "no instance"
    keep = np.ones(1007, dtype=bool)
    keep[counted[[3, 500, 900]]] = False
    conf = R.confusion([gs[keep]], [ps[keep]], C, C - 1)
    ok_inst = bad_inst.copy()
    ok_inst[counted[[10, 11]]] = -1
    tp, fp, fn, iou, n_m = R.panoptic_counts([gs], [gi], [ps], [ok_inst], C, [C - 1], 1)
    assert np.array_equal(host[G:o].reshape(C, C), conf)
    assert np.array_equal(host[o:o + C], tp) and np.array_equal(host[o + C:o + 2 * C], fp) and np.array_equal(host[o + 2 * C:o + 3 * C], fn)
    got_iou = host[o + 3 * C:o + 4 * C].view(np.float64)
    assert np.all(np.abs(got_iou - iou) <= max(n_m, 1) * 2.0 ** -52 * np.abs(iou))
    # through the accumulator: result() raises and names the bits
    acc = eval_seg.SegPanAccumulator(C, [C - 1], [0, 1], list(range(2, C - 1)), 1)
    acc.add(dict(pts_semantic_mask=_t(gs, d), pts_instance_mask=_t(gi, d)),
            dict(pts_semantic_mask=[_t(bad_sem, d), _t(ps, d)], pts_instance_mask=[None, _t(pi, d)]))
    with pytest.raises(RuntimeError, match="semantic prediction lies outside"):
        acc.result()
    acc = eval_seg.SegPanAccumulator(C, [C - 1], [0, 1], list(range(2, C - 1)), 1)
    acc.add(dict(pts_semantic_mask=_t(gs, d), pts_instance_mask=_t(gi, d)),
            dict(pts_semantic_mask=[_t(ps, d), _t(ps, d)], pts_instance_mask=[None, _t(bad_inst, d)]))
    with pytest.raises(RuntimeError, match="instance id"):
        acc.result()
    # wrong dtypes / shapes are refused, not converted
    with pytest.raises(TypeError):
        ops.semantic_confusion(_t(ps, d).int(), _t(gs, d), C, C - 1, v["confusion"], v["status"])
    with pytest.raises(ValueError):
        ops.semantic_confusion(_t(ps, d)[:-1], _t(gs, d), C, C - 1, v["confusion"], v["status"])


def test_add_does_not_synchronise():
    from segdino3d_amd import eval_seg
    d = dev()
    C = 11
    gs, gi, ps, pi = R.make_scene(41, 3000, C)
    ann = dict(pts_semantic_mask=_t(gs, d), pts_instance_mask=_t(gi, d))
    pred = dict(pts_semantic_mask=[_t(ps, d), _t(ps, d)], pts_instance_mask=[None, _t(pi, d)])
    acc = eval_seg.SegPanAccumulator(C, [C - 1], [0, 1], list(range(2, C - 1)), 1)
    acc.add(ann, pred)                                          # first call: allocations, library load
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        acc.add(ann, pred)
        state = acc.state()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert state.is_cuda and state.dtype == torch.float64 and state.shape == (acc.width,)
    c = acc.counts()
    tp, fp, fn, iou, _ = R.panoptic_counts([gs, gs], [gi, gi], [ps, ps], [pi, pi], C, [C - 1], 1)
    assert np.array_equal(c["tp"], tp) and np.array_equal(c["fp"], fp) and np.array_equal(c["fn"], fn)
    # a state that went through merge gives the same metrics as the accumulator itself
    merged = eval_seg.SegPanAccumulator.merge([state[None]])
    assert acc.result(state=merged)["pan"]["pq"] == acc.result()["pan"]["pq"]


def test_evaluator_metrics_end_to_end():
    """miou / all_ap* / pq over the four scenes of the evaluator fixture: AP equal to evaluator_instance_metrics, miou and pq to the
    restatement; the panoptic predictions are the generator's (ground truth rolled, relabelled and split)."""
    from segdino3d_amd import eval_ap, eval_seg
    from test_oracle_golden import _evaluator_fixture
    d = dev()
    z, classes, valid, n_stuff, results = _evaluator_fixture()
    C = len(classes)
    on_dev, gts, preds = [], [], []
    for si, (a, p) in enumerate(results):
        gs, gi = np.asarray(a["pts_semantic_mask"]), np.asarray(a["pts_instance_mask"])
        edges = [0] + (np.flatnonzero((np.diff(gs) != 0) | (np.diff(gi) != 0)) + 1).tolist() + [len(gs)]
        ps, pi = R.make_pred(500 + si, gs, gi, edges, C, n_stuff)
        gts.append(dict(pts_semantic_mask=gs, pts_instance_mask=gi))
        preds.append(dict(pts_semantic_mask=ps, pts_instance_mask=pi))
        on_dev.append((dict(pts_semantic_mask=_t(gs, d), pts_instance_mask=_t(gi, d)),
                       dict(pts_semantic_mask=[_t(ps, d), _t(ps, d)], pts_instance_mask=[torch.from_numpy(p["pts_instance_mask"][0]).to(d), _t(pi, d)],
                            instance_labels=torch.from_numpy(p["instance_labels"]).to(d), instance_scores=torch.from_numpy(p["instance_scores"]).to(d))))
    thing, stuff = list(range(n_stuff, C - 1)), list(range(n_stuff))
    m = eval_seg.evaluator_metrics(on_dev, classes, valid, thing, stuff, 1, [C - 1])
    assert set(m) == {"miou", "all_ap", "all_ap_50%", "all_ap_25%", "pq"}
    ap = eval_ap.evaluator_instance_metrics(on_dev, classes, valid, n_stuff)
    for k in ("all_ap", "all_ap_50%", "all_ap_25%"):
        assert m[k] == ap[k], k
    l2c = {i: c for i, c in enumerate(classes)}
    want_sem = R.seg_eval([g["pts_semantic_mask"] for g in gts], [p["pts_semantic_mask"] for p in preds], l2c, C - 1)
    want_pan = R.panoptic_seg_eval(gts, preds, list(classes), [classes[i] for i in thing], [classes[i] for i in stuff], 1, 2 ** 16, l2c, [C - 1])
    assert 0.0 < want_sem["miou"] < 1.0 and 0.0 < want_pan["pq"] < 1.0
    assert m["miou"] == pytest.approx(want_sem["miou"], abs=1e-15)
    # iou_sum within n_matches * 2^-52 relative; sq * rq, the sum over C classes and the division add at most C + 4 roundings
    n_m = R.panoptic_counts([g["pts_semantic_mask"] for g in gts], [g["pts_instance_mask"] for g in gts], [p["pts_semantic_mask"] for p in preds],
                            [p["pts_instance_mask"] for p in preds], C, [C - 1], 1)[4]
    assert n_m > 0
    assert m["pq"] == pytest.approx(want_pan["pq"], rel=(n_m + C + 4) * 2.0 ** -52, abs=0)
