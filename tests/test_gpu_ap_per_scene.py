"""`eval_ap_scene.SceneApAccumulator` + csrc/apeval_scene.hip against the host route called with ONE scene at a time
(`eval_ap.instance_seg_eval`, the body of the reference's `compute_each_sample_metrics`).

Bounds: those of tests/test_gpu_ap_accumulator.py (`_assert_tables`): `ap` within 1e-12 absolute, NaNs equal; `pr_rc` the same bound
and bit-equal.  `summary` is a mean of at most C * O such cells, so it carries the same 1e-12.  Everything compared between two device
runs (merged states, the global tables next to `ApAccumulator`, two runs) must be equal bit for bit."""
import numpy as np
import pytest
import torch

from test_gpu_ap_accumulator import SCORES, _Builder, _assert_tables, _host_route, dev, make_scene
from test_gpu_ap_accumulator import _to_dev as _to_dev_rows
from test_oracle_golden import _ap_fixture, _evaluator_fixture

pytestmark = pytest.mark.gpu

SUMMARY = ("all_ap", "all_ap_50%", "all_ap_25%", "all_prec_50%", "all_rec_50%")
VALID6 = (2, 3, 4, 5, 6, 7)
LABELS6 = tuple(f"c{i}" for i in VALID6)
OPTIONS = dict(min_region_sizes=np.array([10]))


def _to_dev(scene, d):
    """`_to_dev` of the accumulator tests; a scene without predictions gets its [0, N] mask made on the device (`from_numpy` of an
    empty array has no unit stride, which the accumulator asks of mask rows)."""
    out = _to_dev_rows(scene, d)
    if scene[2].shape[0] == 0:
        out = out[:2] + (torch.zeros(scene[2].shape, dtype=torch.bool, device=d),) + out[3:]
    return out


def _close(a, b):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-12


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _new(valid=VALID6, labels=LABELS6, options=OPTIONS, **kw):
    from segdino3d_amd import eval_ap_scene
    return eval_ap_scene.SceneApAccumulator(valid, labels, options=options, groups={}, **kw)


def _fill(acc, by_key, order=None):
    for k in (order if order is not None else by_key):
        acc.add_scene(*by_key[k], k)
    return acc


def _assert_scenes(tables, by_key, valid=VALID6, labels=LABELS6, options=OPTIONS):
    """Every scene of `tables` == the host route on that scene alone; `summary` == `compute_averages` of the host tables."""
    from segdino3d_amd import eval_ap
    opts = eval_ap.get_options(options)
    keys, ap, pr_rc, summary = tables
    C, O = len(valid), len(opts["overlaps"])
    assert keys.dtype == np.int64 and keys.tolist() == sorted(by_key)
    assert ap.shape == (len(keys), C, O) and pr_rc.shape == (2, len(keys), C, O) and summary.shape == (len(keys), 5)
    assert ap.dtype == pr_rc.dtype == summary.dtype == np.float64
    host = {}
    for s, k in enumerate(keys.tolist()):
        want = _host_route([by_key[k]], labels, valid, opts)
        _assert_tables((ap[s:s + 1], pr_rc[:, s]), want)
        d = eval_ap.compute_averages(want[0], want[1], opts, labels, groups={})
        for j, name in enumerate(SUMMARY):
            assert _close(summary[s, j], d[name]), (k, name, summary[s, j], d[name])
        host[k] = want
    return host


def _mixed_scenes(d):
    """Five scenes over six classes.  Random scenes only use classes 0 .. 3 (`make_scene` over the first four ids); the hand-made one
    holds class 4 (ground truth and predictions, nowhere else), class 0 as ground truth without a prediction and class 1 as a prediction
    without ground truth; class 5 is nowhere."""
    four = VALID6[:4]
    b = _Builder()
    b.points(1500, -1, -1)
    other = b.points(300, VALID6[3], 50)
    g4 = [b.points(40, VALID6[4], 10 + i) for i in range(3)]
    b.points(60, VALID6[0], 20)                                                # class 0: ground truth only
    b.pred(4, 0.9, (g4[0], 40))
    b.pred(4, 0.62, (g4[1], 30), (other, 5))
    b.pred(4, 0.3, (other + 10, 40))                                           # a false positive of class 4
    b.pred(1, 0.75, (other + 60, 40))                                          # class 1: a prediction only
    no_gt = list(make_scene(23, 2503, 10, 25, four, n_sem=6))
    no_gt[0] = np.where(no_gt[0] >= 0, 40, no_gt[0])                           # every semantic id outside the valid ones
    scenes = {7: make_scene(21, 3001, 12, 30, four, n_sem=6), 3: make_scene(22, 2003, 8, 0, four, n_sem=6), 11: tuple(no_gt),
              0: b.scene(), 5: make_scene(24, 4000, 15, 40, four, n_sem=6)}
    return {k: _to_dev(s, d) for k, s in scenes.items()}


# ------------------------------------------------------------------------------------------------------------------ 1. per scene == host
def test_per_scene_tables_equal_the_host_route_one_scene_at_a_time():
    from segdino3d_amd import eval_ap
    d = dev()
    by_key = _mixed_scenes(d)
    acc = _fill(_new(), by_key)
    keys, ap, pr_rc, summary = tables = acc.scene_tables()
    _assert_scenes(tables, by_key)
    at = {k: s for s, k in enumerate(keys.tolist())}
    assert np.isnan(ap[at[3]][:, :]).sum() > 0 and (ap[at[3]][~np.isnan(ap[at[3]])] == 0).all()       # no predictions: 0 or NaN
    assert (ap[at[3]] == 0).any()
    assert np.isnan(ap[at[11]]).all() and np.isnan(summary[at[11]]).all()                              # no ground truth of a valid class
    assert (ap[at[0], 0] == 0).all() and (pr_rc[:, at[0], 0] == 0).all()                               # ground truth, no prediction
    assert np.isnan(ap[at[0], 1]).all()                                                                # a prediction, no ground truth
    assert (ap[at[0], 4] > 0).all() and all(np.isnan(ap[at[k], 4]).all() for k in (3, 5, 7, 11))       # a class of one scene only
    assert np.isnan(ap[:, 5]).all()
    assert ((ap > 0) & (ap < 1)).any()
    # the dictionaries, key by key
    names = {k: f"scene{k:04d}_00" for k in by_key if k != 5}                                          # key 5 keeps its key as the name
    got = acc.scene_results(names)
    assert set(got) == {names.get(k, k) for k in by_key}
    for k, s in by_key.items():
        want = eval_ap.instance_seg_eval([s[0]], [s[1]], [s[2]], [s[3]], [s[4]], VALID6, LABELS6, options=OPTIONS, groups={})
        mine = got[names.get(k, k)]
        assert set(mine) == set(want) and set(mine["classes"]) == set(want["classes"]) == set(LABELS6)
        for name in SUMMARY:
            assert _close(mine[name], want[name]), (k, name)
        for c in LABELS6:
            assert set(mine["classes"][c]) == set(want["classes"][c])
            for f, v in want["classes"][c].items():
                assert _close(mine["classes"][c][f], v), (k, c, f)


# ------------------------------------------------------------------------------------------------------------------ 2. ties
def test_ties_do_not_cross_scenes():
    """Two scenes whose predictions have the same classes and the same scores: in one they cover their ground truth, in the other
    they lie beside it.  Sorted by (group, score) alone their entries would interleave."""
    d = dev()
    scenes = {}
    for key, hit in ((0, True), (1, False)):
        b = _Builder()
        b.points(1900, -1, -1)
        filler = b.points(400, VALID6[5], 90)
        for i in range(6):
            lo = b.points(40, VALID6[i % 2], i)
            score = SCORES[[3, 3, 5, 5, 5, 6][i]]
            if hit or i == 4:
                b.pred(i % 2, score, (lo, 40))
            else:
                b.pred(i % 2, score, (filler + 50 * i, 40))
        scenes[key] = _to_dev(b.scene(), d)
    assert torch.equal(scenes[0][3], scenes[1][3]) and torch.equal(scenes[0][4], scenes[1][4])
    host = _assert_scenes(_fill(_new(), scenes).scene_tables(), scenes)
    assert (host[0][0][0, :2] > 0.999).all() and (host[1][0][0, :2] < 0.999).all()
    _assert_scenes(_fill(_new(), scenes, order=[1, 0]).scene_tables(), scenes)


# ------------------------------------------------------------------------------------------------------------------ 3. segment boundaries
def test_zero_slot_scenes_first_last_and_between_and_a_single_scene():
    d = dev()
    four = VALID6[:4]
    scenes = {k: _to_dev(make_scene(40 + k, 2001 + 7 * k, 9, n_pred, four, n_sem=6), d) for k, n_pred in enumerate((0, 25, 0, 0, 33, 0))}
    acc = _fill(_new(), scenes)
    assert acc._offsets == [0, 0, 300, 300, 300, 696, 696]
    _assert_scenes(acc.scene_tables(), scenes)
    for k in (0, 1):                                                            # S = 1: without and with slots
        _assert_scenes(_fill(_new(), {k: scenes[k]}).scene_tables(), {k: scenes[k]})


def test_one_scene_group_longer_than_a_tile_beside_empty_groups():
    """The scene of `test_one_group_longer_than_a_tile_among_mostly_empty_groups`: 198 classes, 600 predictions of class 17, so the
    (scene, class 17, overlap) segments cross the 256-entry tile while 196 classes of the scene are empty; two small scenes around it."""
    d = dev()
    valid = tuple(range(2, 200))
    labels = tuple(f"c{i}" for i in valid)
    g = np.random.default_rng(50)
    N, n_inst, n_pred = 3000, 30, 600
    owner = np.repeat(np.arange(n_inst), N // n_inst)
    gt_sem = np.where(owner < 22, valid[17], valid[101])
    gt_sem = np.where(owner >= 27, -1, gt_sem)
    gt_inst = np.where(owner >= 27, -1, owner * 7)
    masks = np.zeros((n_pred, N), dtype=bool)
    for p in range(n_pred):
        o = int(g.integers(0, n_inst))
        masks[p] = ((owner == o) & (g.random(N) > g.random() * 0.7)) | (g.random(N) > 0.99)
    scores = np.where(g.random(n_pred) < 0.5, g.random(n_pred).astype(np.float32), SCORES[g.integers(0, len(SCORES), n_pred)])
    long_scene = (gt_sem.astype(np.int64), gt_inst.astype(np.int64), masks, np.full(n_pred, 17), scores.astype(np.float32))
    scenes = {0: make_scene(60, 2001, 10, 12, valid), 1: long_scene, 2: make_scene(61, 2500, 10, 0, valid)}
    assert 17 not in scenes[0][3].tolist()
    scenes = {k: _to_dev(s, d) for k, s in scenes.items()}
    acc = _fill(_new(valid, labels), scenes)
    e = acc.entries()
    assert np.bincount(e["group"]).max() > 256 and set(e["group"][e["group"] // 10 == 17]) == set(range(170, 180))
    keys, ap, pr_rc, summary = tables = acc.scene_tables()
    _assert_scenes(tables, scenes, valid, labels)
    assert ((0 < ap[1, 17]) & (ap[1, 17] < 1)).sum() >= 8
    assert (ap[1, 101] == 0).all() and np.isnan(np.delete(ap[1], [17, 101], axis=0)).all()


# ------------------------------------------------------------------------------------------------------------------ 4. key width
@pytest.mark.parametrize("n_classes,n_scenes,n_pred,passes", [(2, 3, 150, 5), (6, 5, 80, 6)])
def test_radix_pass_counts(n_classes, n_scenes, n_pred, passes):
    """Above 4096 slots the sort runs radix passes of 8 bits over 33 + ceil(log2(S (C O + 1))) bits: 3 scenes of 2 classes sort
    33 + 6 bits in 5 passes (odd: the keys land in the second buffer), 5 scenes of 6 classes 33 + 9 bits in 6 (even: in the first)."""
    d = dev()
    valid, labels = VALID6[:n_classes], LABELS6[:n_classes]
    bits = 33 + int(np.ceil(np.log2(n_scenes * (n_classes * 10 + 1))))
    assert -(-bits // 8) == passes
    scenes = {k: _to_dev(make_scene(70 + k, 3001, 20, n_pred, valid, n_sem=n_classes + 3), d) for k in range(n_scenes)}
    acc = _fill(_new(valid, labels), scenes)
    assert acc.used == n_scenes * n_pred * 12 > 4096
    _assert_scenes(acc.scene_tables(), scenes, valid, labels)


def test_a_key_too_wide_is_refused_before_anything_is_launched():
    from segdino3d_amd import _lib, ops
    d = dev()
    lib = _lib.load()
    C, O = 1024, 1
    S = (1 << 30) // (C * O + 1) + 1                                            # S (C O + 1) >= 2^30
    assert S * (C * O + 1) >= 1 << 30 > (S - 1) * (C * O + 1)
    guard = torch.full((64,), -7.0, dtype=torch.float64, device=d)              # stands for every pointer: nothing may touch it
    p = guard.data_ptr()
    rc = lib.sd3d_ap_finish_scenes(None, 0, p, S, C, O, p, 1, 0, p, p, p, p, 1 << 20, torch.cuda.current_stream().cuda_stream)
    assert rc == -1 and b"2^30" in lib.sd3d_last_error()
    with pytest.raises(ValueError, match="2\\^30"):
        ops.ap_finish_scenes(torch.zeros(0, dtype=torch.int64, device=d), [0] * (S + 1), C, O,
                             torch.zeros(1, dtype=torch.int64, device=d).expand(S, C * O + 2 * C), 1, 0)
    torch.cuda.synchronize()
    assert (guard == -7.0).all()


# ------------------------------------------------------------------------------------------------------------------ 5. global tables
def test_global_tables_are_those_of_ap_accumulator_bit_for_bit():
    from segdino3d_amd import eval_ap
    d = dev()
    by_key = _mixed_scenes(d)
    scene_acc = _fill(_new(), by_key)
    plain = eval_ap.ApAccumulator(VALID6, LABELS6, options=OPTIONS, groups={})
    for s in by_key.values():
        plain.add_scene(*s)
    want, got = plain.tables(), scene_acc.tables()
    assert got[0].shape == (1, 6, 10) and got[1].shape == (2, 6, 10) and np.isfinite(want[0]).any()
    assert _same(got, want)
    assert _same(scene_acc.tables(scene_acc.state()), want)
    e, ew = scene_acc.entries(), plain.entries()
    for k in ("group", "score", "true", "hard_fn", "has_gt", "has_pred"):
        assert e[k].tobytes() == ew[k].tobytes(), k
    rs, rp = scene_acc.result(), plain.result()
    assert all(_close(rs[k], rp[k]) and rs[k] == rs[k] for k in SUMMARY)


@pytest.mark.parametrize("opt_name,options", [("default", None), ("min30", dict(min_region_sizes=np.array([30])))])
def test_golden_ap_protocol_through_both_accumulators(opt_name, options):
    from segdino3d_amd import eval_ap, eval_ap_scene
    d = dev()
    z, class_labels, valid, scenes, groups = _ap_fixture()
    plain = eval_ap.ApAccumulator(valid, class_labels, options=options)
    per_scene = eval_ap_scene.SceneApAccumulator(valid, class_labels, options=options)
    for k, s in enumerate(scenes):
        plain.add_scene(*_to_dev(s, d))
        per_scene.add_scene(*_to_dev(s, d), k)
    assert _same(per_scene.tables(), plain.tables())
    for metrics in (plain.result(), per_scene.result()):
        for k, v in zip(z[f"{opt_name}_keys"], z[f"{opt_name}_vals"]):
            assert _close(metrics[str(k)], v), (k, metrics[str(k)], v)


# ------------------------------------------------------------------------------------------------------------------ 6. golden evaluator
def test_golden_evaluator_each_sample_metrics():
    from segdino3d_amd import eval_ap, eval_ap_scene
    d = dev()
    z, classes, valid, n_stuff, results = _evaluator_fixture()
    on_dev = []
    for i, (ann, pred) in enumerate(results):
        a = dict(pts_semantic_mask=torch.from_numpy(ann["pts_semantic_mask"]).to(d), pts_instance_mask=torch.from_numpy(ann["pts_instance_mask"]).to(d),
                 lidar_idx=f"scene{700 + i:04d}_00")
        p = dict(pts_instance_mask=[torch.from_numpy(pred["pts_instance_mask"][0]).to(d)], instance_labels=torch.from_numpy(pred["instance_labels"]).to(d),
                 instance_scores=torch.from_numpy(pred["instance_scores"]).to(d))
        on_dev.append((a, p))
    got = eval_ap_scene.evaluator_each_sample_metrics(on_dev, classes, valid, n_stuff)
    assert list(got) == [a["lidar_idx"] for a, _ in on_dev]
    finite = 0
    for a, p in on_dev:
        want = eval_ap.evaluator_instance_metrics([(a, p)], classes, valid, n_stuff)
        mine = got[a["lidar_idx"]]
        assert set(mine) == set(want)
        for k, v in want.items():
            if k == "classes":
                continue
            assert _close(mine[k], v), (a["lidar_idx"], k, mine[k], v)
            finite += int(v == v)
        assert set(mine["classes"]) == set(want["classes"])
        for c, fields in want["classes"].items():
            for f, v in fields.items():
                assert _close(mine["classes"][c][f], v), (a["lidar_idx"], c, f)
    assert finite >= 4 * len(SUMMARY)


# ------------------------------------------------------------------------------------------------------------------ 7. state
def test_merged_shuffled_states_equal_one_accumulator():
    from segdino3d_amd import dist_eval, eval_ap_scene
    d = dev()
    by_key = _mixed_scenes(d)
    whole, even, odd = _fill(_new(), by_key), _new(), _new()
    for i, k in enumerate(sorted(by_key)):
        (even if i % 2 == 0 else odd).add_scene(*by_key[k], k)
    want = whole.scene_tables()
    states = dist_eval.all_gather_records(even.state()) + [odd.state(), _new().state()]
    assert all(s.dim() == 2 and s.shape[1] == whole.STATE_WIDTH and s.dtype == torch.float64 for s in states)
    rows = torch.cat([s.to(d) for s in states])
    assert float(rows.max()) < 2.0 ** 53
    rows = rows[torch.randperm(rows.shape[0], generator=torch.Generator().manual_seed(5)).to(d)]
    merged = eval_ap_scene.SceneApAccumulator.merge([rows])
    assert _same(_new().scene_tables(merged), want)
    assert _same(_new().scene_tables(merged.cpu()), want)                       # a gathered state may arrive on the host
    assert _same(_new().scene_tables(rows), want)                               # unmerged rows are a state too
    assert _same(whole.scene_tables(whole.state()), want)
    assert _same(_new().tables(merged), whole.tables())
    with pytest.raises(ValueError, match="present in two states"):
        eval_ap_scene.SceneApAccumulator.merge([even.state(), odd.state(), even.state()])
    with pytest.raises(ValueError, match="added before"):
        even.add_scene(*by_key[0], sorted(by_key)[0])


def test_an_accumulator_without_scenes():
    acc = _new()
    dev()
    keys, ap, pr_rc, summary = acc.scene_tables()
    assert keys.shape == (0,) and ap.shape == (0, 6, 10) and pr_rc.shape == (2, 0, 6, 10) and summary.shape == (0, 5)
    assert acc.scene_results() == {}
    assert [t.shape for t in acc.scene_tables(acc.state())] == [(0,), (0, 6, 10), (2, 0, 6, 10), (0, 5)]
    g_ap, g_pr_rc = acc.tables()
    assert g_ap.shape == (1, 6, 10) and g_pr_rc.shape == (2, 6, 10) and np.isnan(g_ap).all() and np.isnan(g_pr_rc).all()
    assert all(np.isnan(acc.result()[k]) for k in SUMMARY)


# ------------------------------------------------------------------------------------------------------------------ 8. no synchronisation
def test_add_does_not_synchronise_while_the_buffers_grow():
    d = dev()
    four = VALID6[:4]
    scene = _to_dev(make_scene(80, 2001, 9, 12, four, n_sem=6), d)
    acc = _new()
    acc.STORE_CHUNK = 256
    acc.COUNTER_ROWS = 2
    acc.add_scene(*scene, 1000)                                                # first call: allocations, library load
    assert acc._scene_rows.shape[0] == 2 and acc._store.numel() == 256
    ann = dict(pts_semantic_mask=scene[0], pts_instance_mask=scene[1])
    pred = dict(pts_instance_mask=[scene[2]], instance_labels=scene[3], instance_scores=scene[4])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for k in range(20):
            acc.add_scene(*scene, k)
        acc.add_scene(scene[0], scene[1], scene[2], scene[3].int(), scene[4].half(), 2000)
        acc.add(ann, pred, 3000)                                               # the evaluator's call: ids mapped inside the kernel
        state = acc.state()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert acc._scene_rows.shape[0] == 32 and acc._store.numel() >= 23 * 12 * 12 > 4 * 256       # both grew, several times
    assert state.is_cuda and state.dtype == torch.float64 and state.dim() == 2 and state.shape[1] == acc.STATE_WIDTH
    keys, ap, pr_rc, summary = tables = acc.scene_tables()
    assert keys.tolist() == list(range(20)) + [1000, 2000, 3000]
    for s in range(1, 21):                                                     # the same scene every time (fp16 scores aside)
        assert _same((ap[s], pr_rc[:, s], summary[s]), (ap[0], pr_rc[:, 0], summary[0]))
    _assert_scenes((keys[:2], ap[:2], pr_rc[:, :2], summary[:2]), {0: scene, 1: scene})
    assert _same(acc.scene_tables(state), tables)


# ------------------------------------------------------------------------------------------------------------------ 9. determinism
def test_two_runs_give_the_same_bits():
    d = dev()
    by_key = _mixed_scenes(d)
    a, b = _fill(_new(), by_key), _fill(_new(), by_key)
    assert torch.equal(a.state(), b.state())
    ta = a.scene_tables()
    assert _same(ta, b.scene_tables()) and _same(ta, a.scene_tables())          # the store is only read: a second call sees the same codes
    assert _same(a.tables(), b.tables())
