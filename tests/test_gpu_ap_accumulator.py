"""`eval_ap.ApAccumulator` + csrc/apeval.hip against the numpy restatement of the streamed protocol (tests/ap_stream_ref.py), against
the host route on the same device tensors (`rename_gt` + `assign_scene` + `evaluate_records`, the body of `instance_seg_eval`) and
against the reference's golden output.

Bounds: entries, hard_fn and the flags are integers / fp32 bit patterns and must equal the restatement exactly; `ap` and `pr_rc`
within 1e-12 absolute, the bound of every AP comparison in this project.  `pr_rc` is the same IEEE operations in the same order as
`evaluate_records` and is additionally required to be bit-equal."""
import numpy as np
import pytest
import torch

import ap_stream_ref as A
from test_oracle_golden import _ap_fixture, _evaluator_fixture

pytestmark = pytest.mark.gpu

SCORES = np.array([0.125, 0.3, 0.45, 0.5, 0.62, 0.75, 0.9, 0.97], dtype=np.float32)


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _to_dev(scene, d, pitch_pad=0):
    """(sem, inst, masks, labels, scores) numpy -> device tensors; pitch_pad > 0: mask rows with a pitch of N + pitch_pad whose padding
    is all ones (it must not be read)."""
    sem, inst, masks, labels, scores = scene
    n, N = masks.shape
    if pitch_pad:
        big = torch.ones(max(n, 1), N + pitch_pad, dtype=torch.bool, device=d)
        mt = big[:n, :N]
        mt.copy_(torch.from_numpy(masks))
    else:
        mt = torch.from_numpy(masks).to(d)
    return (torch.from_numpy(sem).to(d), torch.from_numpy(inst).to(d), mt, torch.from_numpy(np.asarray(labels, dtype=np.int64)).to(d),
            torch.from_numpy(np.asarray(scores, dtype=np.float32)).to(d))


def _host_route(dev_scenes, class_labels, valid, opts):
    """The body of `instance_seg_eval` up to the tables."""
    from segdino3d_amd import eval_ap
    gts = eval_ap.rename_gt([s[0] for s in dev_scenes], [s[1] for s in dev_scenes], valid)
    recs = [eval_ap.assign_scene(s[2], s[3], s[4], g, opts, valid) for s, g in zip(dev_scenes, gts)]
    return eval_ap.evaluate_records(recs, class_labels, valid, opts)


def _restatement(scenes, valid, opts):
    min_region = int(opts["min_region_sizes"][0])
    recs = [A.scene_record(s[0], s[1], s[2], s[3], s[4], valid, min_region) for s in scenes]
    return A.accumulate(recs, valid, opts["overlaps"], min_region)


def _assert_entries(e, want):
    (group, score, true), hard_fn, has_gt, has_pred, _ = want
    assert e["status"] == 0
    assert np.array_equal(e["group"], group) and np.array_equal(e["true"], true)
    assert e["score"].tobytes() == score.astype(np.float32).tobytes()
    assert np.array_equal(e["hard_fn"], hard_fn) and np.array_equal(e["has_gt"], has_gt) and np.array_equal(e["has_pred"], has_pred)


def _assert_tables(got, want, exact_pr_rc=True):
    ap, pr_rc = got
    ap_w, pr_rc_w = want
    assert ap.shape == ap_w.shape and pr_rc.shape == pr_rc_w.shape
    assert np.allclose(ap, ap_w, rtol=0, atol=1e-12, equal_nan=True), np.nanmax(np.abs(ap - ap_w))
    assert np.allclose(pr_rc, pr_rc_w, rtol=0, atol=1e-12, equal_nan=True)
    if exact_pr_rc:
        cell = np.argwhere(~((pr_rc == pr_rc_w) | (np.isnan(pr_rc) & np.isnan(pr_rc_w))))
        assert len(cell) == 0, ("pr_rc is not bit-equal at", cell[:4].tolist())


def _check(scenes, valid, class_labels, options, d, pitch_pad=0, via=None):
    """Device route over `scenes` == restatement (entries, exact) == host route (tables); returns (accumulator, restatement, tables)."""
    from segdino3d_amd import eval_ap
    opts = eval_ap.get_options(options)
    dev_scenes = [_to_dev(s, d, pitch_pad) for s in scenes]
    acc = eval_ap.ApAccumulator(valid, class_labels, options=options)
    for s in dev_scenes:
        acc.add_scene(*s)
    want = _restatement(scenes, valid, opts)
    _assert_entries(acc.entries(), want)
    tables = acc.tables()
    _assert_tables(tables, A.finish(*want[:4]))
    _assert_tables(tables, _host_route(dev_scenes, class_labels, valid, opts))
    return acc, want, tables


# ------------------------------------------------------------------------------------------------------------------ 1. golden
@pytest.mark.parametrize("opt_name,options", [("default", None), ("min30", dict(min_region_sizes=np.array([30])))])
def test_golden_ap_protocol(opt_name, options):
    from segdino3d_amd import eval_ap
    d = dev()
    z, class_labels, valid, scenes, groups = _ap_fixture()
    acc = eval_ap.ApAccumulator(valid, class_labels, options=options)
    for s in scenes:
        acc.add_scene(*_to_dev(s, d))
    metrics = acc.result()
    for k, v in zip(z[f"{opt_name}_keys"], z[f"{opt_name}_vals"]):
        got = metrics[str(k)]
        assert (np.isnan(got) and np.isnan(v)) or abs(got - v) < 1e-12, (k, got, v)
    cls = np.array([[metrics["classes"][c][f] for f in ("ap", "ap50%", "ap25%", "prec50%", "rec50%")] for c in class_labels])
    assert np.allclose(cls, z[f"{opt_name}_class_ap"], rtol=0, atol=1e-12, equal_nan=True)
    _check(scenes, valid, class_labels, options, d)


def test_golden_evaluator_through_add():
    """`add(eval_ann, pred)`: map_inst_markup inside the kernel, the stuff classes drop out."""
    from segdino3d_amd import eval_ap
    d = dev()
    z, classes, valid, n_stuff, results = _evaluator_fixture()
    things, labels = tuple(valid[n_stuff:]), tuple(classes[n_stuff:-1])
    acc = eval_ap.ApAccumulator(things, labels, num_stuff_cls=n_stuff)
    on_dev = []
    for ann, pred in results:
        a = dict(pts_semantic_mask=torch.from_numpy(ann["pts_semantic_mask"]).to(d), pts_instance_mask=torch.from_numpy(ann["pts_instance_mask"]).to(d))
        p = dict(pts_instance_mask=[torch.from_numpy(pred["pts_instance_mask"][0]).to(d)], instance_labels=torch.from_numpy(pred["instance_labels"]).to(d),
                 instance_scores=torch.from_numpy(pred["instance_scores"]).to(d))
        on_dev.append((a, p))
        acc.add(a, p)
    metrics = acc.result()
    for k, v in zip(z["keys"], z["vals"]):
        got = metrics[str(k)]
        assert (np.isnan(got) and np.isnan(v)) or abs(got - v) < 1e-12, (k, got, v)
    cls = np.array([[metrics["classes"][c][f] for f in ("ap", "ap50%", "ap25%")] for c in labels])
    assert np.allclose(cls, z["class_ap"][:, :3], rtol=0, atol=1e-12, equal_nan=True)
    host = eval_ap.evaluator_instance_metrics(on_dev, classes, valid, n_stuff)
    for k in ("all_ap", "all_ap_50%", "all_ap_25%"):
        assert abs(metrics[k] - host[k]) < 1e-12


# ------------------------------------------------------------------------------------------------------------------ 2. device == host
def make_scene(seed, N, n_inst, n_pred, valid, n_sem=46):
    """Ground truth: n_inst instances over the points with distinct indices in [0, 1000) (0 and 999 among them), semantic ids in
    [0, n_sem) (some not valid -> void), 15 % of the points unannotated (-1, -1).  Predictions: most of one instance plus noise with the
    instance's label (85 %) or another one, a block of unannotated points (dropped by the ignore test), or three points (too small)."""
    g = np.random.default_rng(seed)
    C = len(valid)
    if n_inst >= 2:
        idxs = np.sort(np.r_[0, 999, g.choice(np.arange(1, 999), n_inst - 2, replace=False)])
    else:
        idxs = np.arange(n_inst)
    inst_sem = g.integers(0, n_sem, n_inst)
    owner = np.where(g.random(N) < 0.15, -1, g.integers(0, max(n_inst, 1), N)) if n_inst else np.full(N, -1)
    gt_inst = np.where(owner >= 0, idxs[np.maximum(owner, 0)] if n_inst else -1, -1).astype(np.int64)
    gt_sem = np.where(owner >= 0, inst_sem[np.maximum(owner, 0)] if n_inst else -1, -1).astype(np.int64)
    masks = np.zeros((n_pred, N), dtype=bool)
    labels = g.integers(0, C, n_pred)
    for p in range(n_pred):
        kind = g.random()
        if kind < 0.75 and n_inst:
            o = int(g.integers(0, n_inst))
            masks[p] = ((owner == o) & (g.random(N) > 0.2)) | (g.random(N) > 0.995)
            if inst_sem[o] in valid and g.random() < 0.85:
                labels[p] = valid.index(int(inst_sem[o]))
        elif kind < 0.9:
            masks[p] = (owner == -1) & (g.random(N) > 0.5)
        else:
            masks[p, g.integers(0, N, 3)] = True
    return gt_sem, gt_inst, masks, labels, SCORES[g.integers(0, len(SCORES), n_pred)]


def test_device_route_equals_host_route_over_several_scenes():
    d = dev()
    valid = tuple(range(2, 42))
    class_labels = tuple(f"c{i}" for i in valid)
    options = dict(min_region_sizes=np.array([10]))
    shapes = [(20011, 400, 150), (5003, 3, 0), (7001, 0, 20), (32773, 60, 64), (1, 1, 1)]
    scenes = [make_scene(100 + k, N, n_inst, n_pred, valid) for k, (N, n_inst, n_pred) in enumerate(shapes)]
    assert {0, 999} <= set(scenes[0][1].tolist()) and {0, 999} <= set(scenes[3][1].tolist())
    acc, want, (ap, pr_rc) = _check(scenes, valid, class_labels, options, d, pitch_pad=37)
    stats = want[4]
    assert stats["matched"] > 0 and stats["extra"] > 0 and stats["fp"] > 0 and stats["ignored"] > 0 and want[1].sum() > 0, stats
    assert ((ap > 0) & (ap < 1)).any()
    # the metrics dictionary is the host route's
    from segdino3d_amd import eval_ap
    dev_scenes = [_to_dev(s, d, 37) for s in scenes]
    host = eval_ap.instance_seg_eval([s[0] for s in dev_scenes], [s[1] for s in dev_scenes], [s[2] for s in dev_scenes], [s[3] for s in dev_scenes],
                                     [s[4] for s in dev_scenes], valid, class_labels, options=options, groups={})
    got = eval_ap.ApAccumulator(valid, class_labels, options=options, groups={})
    for s in dev_scenes:
        got.add_scene(*s)
    got = got.result()
    for k in ("all_ap", "all_ap_50%", "all_ap_25%", "all_prec_50%", "all_rec_50%"):
        assert abs(got[k] - host[k]) < 1e-12, k
    # two runs: the same bits
    again = eval_ap.ApAccumulator(valid, class_labels, options=options)
    for s in dev_scenes:
        again.add_scene(*s)
    assert torch.equal(again.state(), acc.state())
    t2 = again.tables()
    assert t2[0].tobytes() == ap.tobytes() and t2[1].tobytes() == pr_rc.tobytes()


def test_valid_class_id_zero_and_fp16_scores():
    """Dataset id 0 is a valid class: a point of instance index 0 with semantic id 0 is counted nowhere (as in `assign_scene`), and the
    ground truths of that class add to the ignore count (`gt_id < 1000`).  Every instance has a valid semantic id here.  fp16 scores
    are widened exactly.  (An instance with a semantic id that is NOT valid is where the routes differ when id 0 is valid: the host
    route reads its id below 1000 as an instance of class 0, the device route as void - see the `ApAccumulator` docstring.)"""
    from segdino3d_amd import eval_ap
    d = dev()
    valid = tuple(range(0, 6))
    class_labels = tuple(f"c{i}" for i in valid)
    options = dict(min_region_sizes=np.array([5]))
    scene = make_scene(7, 3001, 12, 40, valid, n_sem=6)
    scene[0][scene[1] == 0] = 0                                               # instance index 0 has semantic id 0
    acc, want, _ = _check([scene], valid, class_labels, options, d)
    assert want[4]["matched"] > 0
    half = eval_ap.ApAccumulator(valid, class_labels, options=options)
    s = _to_dev(scene, d)
    exact = torch.from_numpy(np.asarray(scene[4], dtype=np.float16).astype(np.float32)).to(d)
    half.add_scene(s[0], s[1], s[2], s[3].int(), exact.half())
    ref = eval_ap.ApAccumulator(valid, class_labels, options=options)
    ref.add_scene(s[0], s[1], s[2], s[3], exact)
    assert torch.equal(half.state(), ref.state())
    with pytest.raises(TypeError, match="host route"):
        half.add_scene(s[0], s[1], s[2], s[3], s[4].double())


# ------------------------------------------------------------------------------------------------------------------ 3. exact ratios
class _Builder:
    def __init__(self):
        self.sem, self.inst, self.preds = [], [], []

    def points(self, n, sem, inst):
        lo = len(self.sem)
        self.sem += [sem] * n
        self.inst += [inst] * n
        return lo

    def pred(self, label, score, *ranges):
        self.preds.append((label, score, ranges))

    def scene(self):
        N = len(self.sem)
        masks = np.zeros((len(self.preds), N), dtype=bool)
        for p, (_, _, ranges) in enumerate(self.preds):
            for lo, n in ranges:
                masks[p, lo:lo + n] = True
        return (np.array(self.sem, dtype=np.int64), np.array(self.inst, dtype=np.int64), masks, np.array([p[0] for p in self.preds], dtype=np.int64),
                np.array([p[1] for p in self.preds], dtype=np.float32))


def test_exact_ratios_decide_as_the_host_route():
    """IoU = inter / 40 with inter = 2 * (5, 10, 11, ..., 18) - the rationals 1/4, 1/2, 11/20, ..., 9/10 - and one point either side;
    the same for the ignore ratio void / 40.  min_region = 1."""
    d = dev()
    valid = tuple(range(2, 42))
    class_labels = tuple(f"c{i}" for i in valid)
    b = _Builder()
    filler = b.points(400, valid[39], 500)                                    # another label: neither void nor ground truth of the predictions
    void = b.points(60, -1, -1)
    k = 0
    for twentieths in (5, 10, 11, 12, 13, 14, 15, 16, 17, 18):
        for delta in (-1, 0, 1):
            inter = 2 * twentieths + delta                                    # union 40: gt + pred - inter == 40
            gt = inter + (40 - inter) // 2
            pred = 40 - gt + inter
            lo = b.points(gt, valid[k % 3], k)
            b.pred(k % 3, SCORES[k % len(SCORES)], (lo, inter), (filler + k, pred - inter))
            v = 2 * twentieths + delta                                        # ignore ratio v / 40
            b.pred(k % 3, SCORES[(k + 3) % len(SCORES)], (void, v), (filler + 100 + k, 40 - v))
            k += 1
    scene = b.scene()
    acc, want, (ap, pr_rc) = _check([scene], valid, class_labels, dict(min_region_sizes=np.array([1])), d)
    stats = want[4]
    assert stats["matched"] > 0 and stats["fp"] > 0 and stats["ignored"] > 0 and want[1].sum() > 0
    # the thresholds decide differently at the exact ratio and one point above it somewhere
    assert len(set(np.round(ap[0, :3].ravel(), 12))) > 3


# ------------------------------------------------------------------------------------------------------------------ 4. capacity bound
def test_the_capacity_bound_is_reached_and_nothing_is_written_outside_the_slot_range():
    from segdino3d_amd import eval_ap, ops
    d = dev()
    valid, class_labels = (2, 3), ("a", "b")
    b = _Builder()
    los = [b.points(10, 2, i) for i in range(3)]
    for lo in los:
        b.pred(0, 0.5, (lo, 10))
    b.pred(0, 0.25, (los[0], 30))                                             # the three ground truths lie inside this prediction
    scene = b.scene()
    options = dict(min_region_sizes=np.array([1]))
    acc, want, _ = _check([scene], valid, class_labels, options, d)
    assert want[4]["per_pred_max"].tolist() == [1] * 9 + [3] and want[4]["extra"] == 3
    # the same scene into a guarded store through the C entry
    n, per, G, SENT = 4, acc.slots_per_pred, 512, -0x0123456789ABCDEF
    assert per == 12 and acc.slots == [1] * 9 + [3]
    store = torch.full((G + n * per + G,), SENT, dtype=torch.int64, device=d)
    counters = torch.full((G + acc.n_counters + 1 + G,), SENT, dtype=torch.int64, device=d)
    counters[G:-G] = 0
    v = acc._views(counters[G:-G])
    s = _to_dev(scene, d)
    ops.ap_scene(s[0], s[1], s[2].view(torch.uint8), s[3], s[4], acc._const["lut"], acc.zero_class, 2, acc._const["overlaps"], acc.slots, 1,
                 store, G, n * per, v["hard_fn"], v["has_gt"], v["has_pred"], v["status"])
    host, chost = store.cpu().numpy(), counters.cpu().numpy()
    assert (host[:G] == SENT).all() and (host[-G:] == SENT).all() and (chost[:G] == SENT).all() and (chost[-G:] == SENT).all()
    body = host[G:-G]
    assert (body != SENT).all()                                                # every slot of the range was written: an entry or the sentinel
    assert np.array_equal(np.sort(body), np.sort(acc._store[:acc.used].cpu().numpy()))
    at25 = body[n * 9 + 3 * 3:n * 9 + 3 * 3 + 3]                               # the slots of prediction 3 at overlap 0.25
    assert ((at25 >> 33) == 0 * 10 + 9).all() and (at25 & 1).sum() == 0
    assert chost[G + acc.n_counters] == 0


# ------------------------------------------------------------------------------------------------------------------ 5. a long group
def test_one_group_longer_than_a_tile_among_mostly_empty_groups():
    d = dev()
    valid = tuple(range(2, 200))
    class_labels = tuple(f"c{i}" for i in valid)
    scenes = []
    for k in range(5):
        g = np.random.default_rng(50 + k)
        N, n_inst, n_pred = 3000, 30, 600
        owner = np.repeat(np.arange(n_inst), N // n_inst)
        gt_sem = np.where(owner < 22, valid[17], valid[101])[...]                 # class 17 has predictions, class 101 ground truth only
        gt_sem = np.where(owner >= 27, -1, gt_sem)
        gt_inst = np.where(owner >= 27, -1, owner * 7)
        masks = np.zeros((n_pred, N), dtype=bool)
        for p in range(n_pred):
            o = int(g.integers(0, n_inst))
            masks[p] = ((owner == o) & (g.random(N) > g.random() * 0.7)) | (g.random(N) > 0.99)
        scores = np.where(g.random(n_pred) < 0.5, g.random(n_pred).astype(np.float32), SCORES[g.integers(0, len(SCORES), n_pred)])
        scenes.append((gt_sem.astype(np.int64), gt_inst.astype(np.int64), masks, np.full(n_pred, 17), scores.astype(np.float32)))
    acc, want, (ap, pr_rc) = _check(scenes, valid, class_labels, dict(min_region_sizes=np.array([10])), d)
    assert acc.used > 4096                                                     # the radix path of the sort (even pass count)
    assert np.bincount(want[0][0]).max() > 1024                                # one group holds more entries than several tiles of 256
    assert ((0 < ap[0, 17]) & (ap[0, 17] < 1)).sum() >= 8 and (ap[0, 17] < 1).all()   # the curve
    assert (ap[0, 101] == 0).all() and (pr_rc[:, 101] == 0).all()              # ground truth without predictions
    rest = np.delete(np.arange(198), [17, 101])
    assert np.isnan(ap[0, rest]).all() and np.isnan(pr_rc[:, rest]).all()      # neither


def test_radix_sort_with_an_odd_pass_count():
    """Which sort `sd3d_ap_finish` runs depends on the slots: up to 4096 one rank-sort launch (the golden, ratio and capacity tests),
    above that radix passes of 8 bits over 33 + ceil(log2(C O + 1)) bits.  40 and 198 classes need 6 passes - an even count, the
    sorted codes land in the input buffer (tests 2, 5) - and two classes need 5, an odd count: they land in the workspace."""
    d = dev()
    valid, class_labels = (2, 3), ("a", "b")
    scene = make_scene(11, 3001, 20, 400, valid, n_sem=5)
    acc, want, _ = _check([scene], valid, class_labels, dict(min_region_sizes=np.array([10])), d)
    assert acc.used == 400 * 12 > 4096 and want[4]["matched"] > 0 and want[4]["fp"] > 0


# ------------------------------------------------------------------------------------------------------------------ 6. status bits
def test_status_bits():
    from segdino3d_amd import eval_ap
    d = dev()
    valid = tuple(range(2, 42))
    C = len(valid)
    class_labels = tuple(f"c{i}" for i in valid)
    options = dict(min_region_sizes=np.array([10]))
    clean = make_scene(3, 5003, 20, 30, valid)

    def run(scene, **kw):
        acc = eval_ap.ApAccumulator(valid, class_labels, options=options)
        for k, v in kw.items():
            setattr(acc, k, v)                                                 # max_slots: the cap on the store
        acc.add_scene(*_to_dev(scene, d))
        return acc

    sem, inst, masks, labels, scores = clean
    some = np.flatnonzero(inst >= 0)
    bad_inst = inst.copy(); bad_inst[some[5]] = 1000; bad_inst[some[9]] = -2
    pt = np.flatnonzero(np.isin(sem, valid) & (inst >= 0))[0]                 # one point of an instance moves to another valid class
    two_sem = sem.copy(); two_sem[pt] = valid[(valid.index(int(sem[pt])) + 1) % C]
    bad_label = labels.copy(); bad_label[4] = C
    bad_score = scores.copy(); bad_score[7] = np.nan
    cases = [((sem, bad_inst, masks, labels, scores), {}, 1, "instance index lies outside"),
             ((two_sem, inst, masks, labels, scores), {}, 2, "spans two semantic classes"),
             ((sem, inst, masks, bad_label, scores), {}, 4, "label lies outside"),
             ((sem, inst, masks, labels, bad_score), {}, 8, "score is not finite"),
             (clean, dict(max_slots=100), 16, "store is too small")]
    for scene, kw, bit, msg in cases:
        acc = run(scene, **kw)
        assert acc.entries()["status"] == bit, (bit, acc.entries()["status"])
        with pytest.raises(RuntimeError, match=msg):
            acc.result()
        with pytest.raises(RuntimeError, match=msg):
            acc.tables(eval_ap.ApAccumulator.merge([acc.state(), run(clean).state()]))      # a set bit survives merging
    # the bad prediction is left out, nothing else changes: label == C and the NaN score
    keep = np.ones(len(labels), dtype=bool); keep[[4, 7]] = False
    both = run((sem, inst, masks, bad_label, bad_score))
    e = both.entries()
    assert e["status"] == 4 | 8
    e["status"] = 0
    opts = eval_ap.get_options(options)
    _assert_entries(e, _restatement([(sem, inst, masks[keep], labels[keep], scores[keep])], valid, opts))
    # an instance index outside the range counts as void
    e = run((sem, bad_inst, masks, labels, scores)).entries()
    e["status"] = 0
    as_void_sem, as_void_inst = sem.copy(), inst.copy()
    as_void_sem[some[[5, 9]]], as_void_inst[some[[5, 9]]] = -1, -1
    _assert_entries(e, _restatement([(as_void_sem, as_void_inst, masks, labels, scores)], valid, opts))
    # a clean accumulator afterwards is untouched by all of that
    _check([clean], valid, class_labels, options, d)


# ------------------------------------------------------------------------------------------------------------------ 7. no synchronisation
def test_add_does_not_synchronise():
    from segdino3d_amd import eval_ap
    d = dev()
    z, classes, valid, n_stuff, results = _evaluator_fixture()
    things, labels = tuple(valid[n_stuff:]), tuple(classes[n_stuff:-1])
    ann, pred = results[0]
    a = dict(pts_semantic_mask=torch.from_numpy(ann["pts_semantic_mask"]).to(d), pts_instance_mask=torch.from_numpy(ann["pts_instance_mask"]).to(d))
    p = dict(pts_instance_mask=[torch.from_numpy(pred["pts_instance_mask"][0]).to(d)], instance_labels=torch.from_numpy(pred["instance_labels"]).to(d),
             instance_scores=torch.from_numpy(pred["instance_scores"]).to(d))
    acc = eval_ap.ApAccumulator(things, labels, num_stuff_cls=n_stuff, device=d)
    acc.STORE_CHUNK = 256                                                      # one scene's slots: the store grows under the sync check
    acc.add(a, p)                                                              # first call: allocations, library load
    sem, inst = eval_ap.map_inst_markup(a["pts_semantic_mask"], a["pts_instance_mask"], things, n_stuff)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(40):
            acc.add(a, p)
        acc.add_scene(sem, inst, p["pts_instance_mask"][0], p["instance_labels"], p["instance_scores"].half())
        state = acc.state()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert acc._store.numel() >= 42 * 19 * 12 > 4 * 256                        # it grew several times
    assert state.is_cuda and state.dtype == torch.float64 and state.dim() == 2 and state.shape[1] == acc.STATE_WIDTH
    one = eval_ap.ApAccumulator(things, labels, num_stuff_cls=n_stuff)
    one.add_scene(sem, inst, p["pts_instance_mask"][0], p["instance_labels"], p["instance_scores"])
    e1, e = one.entries(), acc.entries()                                       # 42 copies of one scene (fp16 scores move no decision)
    assert e["status"] == 0 and len(e1["group"]) > 0 and e1["true"].sum() > 0
    assert np.array_equal(np.bincount(e["group"]), 42 * np.bincount(e1["group"])) and e["true"].sum() == 42 * e1["true"].sum()
    assert np.array_equal(e["hard_fn"], 42 * e1["hard_fn"])
    assert np.array_equal(e["has_gt"], e1["has_gt"]) and np.array_equal(e["has_pred"], e1["has_pred"])


# ------------------------------------------------------------------------------------------------------------------ 8. merging
def test_merged_halves_equal_one_accumulator_and_an_empty_one_is_all_nan():
    from segdino3d_amd import dist_eval, eval_ap
    d = dev()
    valid = tuple(range(2, 42))
    class_labels = tuple(f"c{i}" for i in valid)
    options = dict(min_region_sizes=np.array([10]))
    scenes = [_to_dev(make_scene(200 + k, 4001 + 13 * k, 25, 40, valid), d) for k in range(4)]
    new = lambda: eval_ap.ApAccumulator(valid, class_labels, options=options)  # noqa: E731
    whole, first, second = new(), new(), new()
    for k, s in enumerate(scenes):
        whole.add_scene(*s)
        (first if k < 2 else second).add_scene(*s)
    gathered = dist_eval.all_gather_records(second.state())                    # outside a process group: the tensor itself
    assert len(gathered) == 1 and gathered[0].dim() == 2
    merged = eval_ap.ApAccumulator.merge(gathered + [first.state(), new().state()])
    e, ew = whole.entries(merged), whole.entries()
    for k in ("group", "score", "true", "hard_fn", "has_gt", "has_pred"):
        assert e[k].tobytes() == ew[k].tobytes(), k
    assert len(ew["group"]) > 0 and ew["true"].sum() > 0
    t, tw = new().tables(merged.cpu()), whole.tables()                         # a gathered state may arrive on the host
    assert t[0].tobytes() == tw[0].tobytes() and t[1].tobytes() == tw[1].tobytes()
    ap, pr_rc = new().tables()
    assert ap.shape == (1, 40, 10) and pr_rc.shape == (2, 40, 10) and np.isnan(ap).all() and np.isnan(pr_rc).all()
    assert np.isnan(new().result()["all_ap"])
