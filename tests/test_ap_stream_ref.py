"""The decomposition behind `eval_ap.ApAccumulator` on the CPU: per-scene entries + sorted per-group curves (tests/ap_stream_ref.py)
against `eval_ap.evaluate_records` - `pr_rc` bit for bit, `ap` within 1e-12 (another summation order of the same products) - on the
golden records and on random multi-scene records with tied scores fed in reverse order; the per-prediction entry bound; the host
surface of the accumulator (no CPU path, argument checks, state layout)."""
import numpy as np
import pytest
import torch

import ap_stream_ref as A
from test_eval_ap import _records


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _check_against_evaluate_records(recs, class_labels, valid, opts, reverse=False):
    from segdino3d_amd import eval_ap
    ap, pr_rc = eval_ap.evaluate_records(recs, class_labels, valid, opts)
    fed = list(reversed(recs)) if reverse else recs
    ent, hard_fn, has_gt, has_pred, stats = A.accumulate(fed, valid, opts["overlaps"], opts["min_region_sizes"][0])
    ap2, pr_rc2 = A.finish(ent, hard_fn, has_gt, has_pred)
    assert _same(pr_rc, pr_rc2)
    assert np.allclose(ap, ap2, rtol=0, atol=1e-12, equal_nan=True)
    for oi, th in enumerate(opts["overlaps"]):
        assert stats["per_pred_max"][oi] <= A.entry_bound(th), (th, stats["per_pred_max"][oi])
    return ap, stats


@pytest.mark.parametrize("opt_name,options", [("default", None), ("min30", dict(min_region_sizes=np.array([30])))])
def test_decomposition_equals_evaluate_records_on_the_golden_records(opt_name, options):
    z, class_labels, valid, groups, opts, id_to_label, preds, gts, recs = _records(options)
    ap, stats = _check_against_evaluate_records(recs, class_labels, valid, opts)
    assert stats["matched"] > 0 and stats["fp"] > 0 and np.nanmax(ap) > 0


def random_record(g, valid, n_gt, n_pred, scores=(0.125, 0.25, 0.5, 0.75, 0.875), min_region=10):
    """A random compact record: disjoint ground truths, predictions that intersect one to three ground truths of their label."""
    from segdino3d_amd.eval_ap import SceneRecord
    valid = np.asarray(valid)
    gt_label = valid[g.integers(0, len(valid), n_gt)]
    gt_vert = g.integers(4, 60, n_gt)
    pred_label = valid[g.integers(0, len(valid), n_pred)]
    pred_vert = g.integers(min_region, 80, n_pred)
    pred_void = np.array([g.integers(0, v // 2 + 1) for v in pred_vert], dtype=np.int64)
    pp, gg, ii = [], [], []
    for p in range(n_pred):
        room = int(pred_vert[p] - pred_void[p])
        for gi in g.permutation(np.flatnonzero(gt_label == pred_label[p]))[:3]:
            inter = int(g.integers(0, min(room, gt_vert[gi]) + 1))
            if inter > 0:
                pp.append(p); gg.append(int(gi)); ii.append(inter)
                room -= inter
    order = np.lexsort((gg, pp))
    a = lambda x: np.asarray(x, dtype=np.int64)                                # noqa: E731
    return SceneRecord(pred_label=a(pred_label), pred_index=np.arange(n_pred), pred_vert=a(pred_vert), pred_void=pred_void,
                       pred_conf=np.asarray(scores, dtype=np.float32)[g.integers(0, len(scores), n_pred)].astype(np.float64),
                       gt_label=a(gt_label), gt_id=a(gt_label) * 1000 + np.arange(n_gt), gt_vert=a(gt_vert), pair_pred=a(pp)[order],
                       pair_gt=a(gg)[order], pair_inter=a(ii)[order])


def test_random_multi_scene_records_with_tied_scores_in_reverse_order():
    from segdino3d_amd import eval_ap
    valid = (2, 3, 5, 8)
    class_labels = tuple(f"c{v}" for v in valid)
    opts = eval_ap.get_options(dict(min_region_sizes=np.array([10])))
    seen = dict(matched=0, extra=0, fp=0, ignored=0)
    for seed in range(12):
        g = np.random.default_rng(seed)
        recs = [random_record(g, valid, int(g.integers(0, 12)), int(g.integers(0, 25))) for _ in range(int(g.integers(1, 5)))]
        _, stats = _check_against_evaluate_records(recs, class_labels, valid, opts, reverse=True)
        for k in seen:
            seen[k] += stats[k]
    assert all(v > 0 for v in seen.values()), seen


def test_entry_bound():
    from segdino3d_amd import eval_ap, ops
    overlaps = eval_ap.get_options(None)["overlaps"]
    assert [A.entry_bound(t) for t in overlaps] == [1] * 9 + [3]
    assert ops.ap_slots_per_prediction(overlaps) == [A.entry_bound(t) for t in overlaps]
    assert [A.entry_bound(t) for t in (0.2, 0.3, 1.0 / 3.0, 0.34, 0.9)] == [4, 3, 2, 2, 1]
    # three ground truths of 10 points inside one 30-point prediction, each matched first by an earlier prediction: three extras at 0.25
    from segdino3d_amd.eval_ap import SceneRecord
    a = lambda x: np.asarray(x, dtype=np.int64)                                # noqa: E731
    rec = SceneRecord(pred_label=a([2] * 4), pred_index=np.arange(4), pred_vert=a([10, 10, 10, 30]), pred_void=a([0] * 4),
                      pred_conf=np.array([0.5, 0.5, 0.5, 0.25]), gt_label=a([2] * 3), gt_id=a([2000, 2001, 2002]), gt_vert=a([10] * 3),
                      pair_pred=a([0, 1, 2, 3, 3, 3]), pair_gt=a([0, 1, 2, 0, 1, 2]), pair_inter=a([10, 10, 10, 10, 10, 10]))
    ent, hard_fn, has_gt, has_pred, stats = A.scene_entries(rec, (2,), overlaps, 1)
    assert stats["per_pred_max"].tolist() == [1] * 9 + [3] and stats["extra"] == 3 and stats["fp"] == 9


def test_accumulator_has_no_cpu_path_and_checks_its_arguments():
    from segdino3d_amd import eval_ap
    acc = eval_ap.ApAccumulator((2, 3, 5), ("a", "b", "c"))
    z = torch.zeros(4, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        acc.add_scene(z, z, torch.zeros(1, 4, dtype=torch.bool), torch.zeros(1, dtype=torch.long), torch.zeros(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        acc.add(dict(pts_semantic_mask=z.numpy(), pts_instance_mask=z.numpy()),
                dict(pts_instance_mask=[torch.zeros(1, 4, dtype=torch.bool)], instance_labels=z[:1], instance_scores=torch.zeros(1)))
    for bad in ([0.5, 1.0], [0.0, 0.5], [-0.25], [1.5]):
        with pytest.raises(ValueError, match=r"\(0, 1\)"):
            eval_ap.ApAccumulator((2, 3), ("a", "b"), options=dict(overlaps=np.array(bad)))
    with pytest.raises(ValueError):
        eval_ap.ApAccumulator((2, 3), ("a",))
    # the thresholds are staged as the float64 bits of the options, not recomputed
    assert acc._host["overlaps"].numpy().tobytes() == np.asarray(eval_ap.get_options(None)["overlaps"], dtype=np.float64).tobytes()
    assert acc._host["lut"].tolist() == [-1, -1, 0, 1, -1, 2] and acc._host["id_map"].tolist() == [2, 3, 5, -1]


def test_state_layout_and_merge_on_the_host():
    """An accumulator that saw no scene: a 2-D float64 state of fixed width whose rows name their kind; merging any number of such
    states in any row order gives the same counters."""
    from segdino3d_amd import dist_eval, eval_ap
    acc = eval_ap.ApAccumulator(tuple(range(2, 200)), tuple(f"c{i}" for i in range(2, 200)))
    s = acc.state()
    assert s.dtype == torch.float64 and s.dim() == 2 and s.shape[1] == eval_ap.ApAccumulator.STATE_WIDTH
    assert sorted(set(s[:, 0].tolist())) == [1.0, 3.0]                          # counters and status, no entry rows yet
    gathered = dist_eval.all_gather_records(s)                                  # outside a process group: the tensor itself
    m = eval_ap.ApAccumulator.merge(gathered + [s.flip(0)])
    codes, counters, status = acc._parse(m)
    assert codes.numel() == 0 and status == 0 and counters.shape == (198 * 10 + 2 * 198,) and not counters.any()
    # hand-made rows: counters add, the status words are OR-ed, entry rows are kept
    a, b = s.clone(), s.clone()
    a[a[:, 0] == 3, 1], b[b[:, 0] == 3, 1] = 4.0, 16.0
    a[1, 2], b[1, 2] = 2.0, 3.0
    e = torch.full((1, s.shape[1]), -1.0, dtype=torch.float64)
    e[0, 0], e[0, 1] = 2.0, float((7 << 33) | (5 << 1) | 1)
    codes, counters, status = acc._parse(eval_ap.ApAccumulator.merge([a, e, b]))
    assert status == 20 and counters[0] == 5
    assert codes[0] == (7 << 33) | 11 and (codes[1:] == acc.sentinel).all() and codes.numel() == s.shape[1] - 1
