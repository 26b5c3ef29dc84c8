"""csrc/lift_queries.hip + segdino3d_amd/lift_queries.py against the float64 restatement tests/lift_queries_ref.py (the reference has
no counterpart) on the room and the hand-built cases of tests/lift_queries_case.py.

Bounds.  `count`, `median_mm`, the selected rows and the gathered features must EQUAL the restatement: every decision of the rule is
an integer one or a single rounded fp32 operation.  Centres: `TOL` = 4 x DEV32 = 4 x 9.537e-07 absolute, four times the largest
deviation of the restatement evaluated in float32 from the same restatement in float64 over these cases (`python
tests/lift_queries_case.py` prints it; profiles/lift_queries.md records it) - the margin of tests/test_gpu_lift2d.py.  The "same bits"
tests carry no tolerance."""
import numpy as np
import pytest
import torch

import lift_queries_case as K
import lift_queries_ref as R

pytestmark = pytest.mark.gpu

TOL = 4 * K.DEV32


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _t(a, d):
    return torch.from_numpy(np.array(a)).to(d)                   # a copy: the shared cases are read-only


def _views(c, d, kind="u16", lo=0, hi=None):
    from segdino3d_amd import lift2d
    depth = (c["depth_u16"] if kind == "u16" else c["depth_f32"])[lo:hi]
    return lift2d.Views(_t(depth, d), _t(c["intr"][lo:hi], d), c["poses"][lo:hi], K.DEPTH_SCALE if kind == "u16" else None)


def _masks(c, size, d, as_bool=False, lo=0, hi=None, q=None):
    m = c["masks"][size][lo:hi]
    m = m if q is None else m[:, :q]
    return _t(m != 0, d) if as_bool else _t(m, d)


def _check_centres(lifter, ref, what):
    centre, count, median, _ = ref
    assert np.array_equal(lifter.counts().cpu().numpy(), count), what
    assert np.array_equal(lifter.medians_mm().cpu().numpy(), median), what
    got = lifter.centres().cpu().numpy()
    err = np.abs(got.astype(np.float64) - centre).max() if got.size else 0.0
    print(f"{what}: largest centre error {err:.3e} (bound {TOL:.3e})")
    assert err <= TOL, what
    assert not got[count == 0].any(), what


@pytest.mark.parametrize("size", K.MASK_SIZES)
@pytest.mark.parametrize("kind,as_bool", [("u16", False), ("f32", True)])
def test_centres_equal_the_restatement(size, kind, as_bool):
    from segdino3d_amd import lift_queries
    d = dev()
    c = K.room_case()
    scores = c["scores"]
    for V in (1, 3, 70):
        for Q in (1, 6):
            lifter = lift_queries.QueryLifter(64, **K.ROOM_RULE)
            lifter.add(_views(c, d, kind, hi=V), _masks(c, size, d, as_bool, hi=V, q=Q), _t(scores[:V, :Q], d), torch.zeros(V, Q, 64, device=d))
            _check_centres(lifter, tuple(x[:V, :Q] for x in c["ref"][size]), (size, kind, V, Q))


@pytest.mark.parametrize("size", [(24, 32), (17, 23)])
def test_seventy_queries_per_view(size):
    from segdino3d_amd import lift_queries
    d = dev()
    c = K.room_case()
    tile = lambda a: np.tile(a, (1, 12) + (1,) * (a.ndim - 2))[:, :70]
    lifter = lift_queries.QueryLifter(64, **K.ROOM_RULE)
    lifter.add(_views(c, d), _t(tile(c["masks"][size]), d), _t(tile(c["scores"]), d), torch.zeros(70, 70, 64, device=d))
    _check_centres(lifter, tuple(tile(x) for x in c["ref"][size]), (size, "Q = 70"))


def test_hand_built_cases():
    from segdino3d_amd import lift2d, lift_queries
    d = dev()
    for case, scale, expect in ((K.hand_case_u16(), K.DEPTH_SCALE, K.HAND_EXPECT_U16), (K.hand_case_f32(), None, K.HAND_EXPECT_F32)):
        depth, intr, poses, masks = case
        for kw, table in expect:
            rule = {**K.HAND_RULE, **kw}
            lifter = lift_queries.QueryLifter(8, **rule)
            V, Q = masks.shape[:2]
            lifter.add(lift2d.Views(_t(depth, d), _t(intr, d), poses, scale), _t(masks, d), torch.ones(V, Q, device=d), torch.zeros(V, Q, 8, device=d))
            _check_centres(lifter, K.hand_ref(depth, scale, intr, poses, masks, **kw), ("hand", kw))
            got_c, got_n, got_m = lifter.centres().cpu().numpy(), lifter.counts().cpu().numpy(), lifter.medians_mm().cpu().numpy()
            for (v, q), (k_med, n, centre) in table.items():
                assert (got_m[v, q], got_n[v, q]) == (k_med, n), (kw, v, q)
                assert np.allclose(got_c[v, q], centre, rtol=1e-6, atol=2e-6), (kw, v, q, got_c[v, q])


def _reference_result(c, size, feats, rule, kind="u16"):
    depth, scale = (c["depth_u16"], K.DEPTH_SCALE) if kind == "u16" else (c["depth_f32"], None)
    return R.lift_queries(depth, scale, c["intr"], c["poses"], c["masks"][size], c["scores"], feats, **rule)


@pytest.mark.parametrize("C,dtype", [(64, np.float16), (256, np.float16), (320, np.float16), (64, np.float32), (256, np.float32), (320, np.float32)])
def test_result_equals_the_restatement(C, dtype):
    """The whole path through the public interface, with three bad poses dropped: rows of masks, scores and feats are given per GIVEN view."""
    from segdino3d_amd import lift_queries
    d = dev()
    c = K.room_case(n_bad_poses=3)
    size = K.MASK_SIZES[(C // 64) % 4]
    feats = K.make_feats(C, K.N_VIEWS, 6, C, dtype)
    views = _views(c, d)
    assert views.n_given == 70 and len(views) == 67
    qf, qp = lift_queries.lift_queries(views, _masks(c, size, d), _t(c["scores"], d), _t(feats, d), **K.ROOM_RULE)
    ref = _reference_result(c, size, feats, K.ROOM_RULE)
    assert len(ref["rows"]) > 20
    assert qf.dtype == torch.float32 and qp.dtype == torch.float32 and qf.is_contiguous() and qp.is_contiguous() and qf.is_cuda and qp.is_cuda
    assert tuple(qf.shape) == (len(ref["rows"]), C) and tuple(qp.shape) == (len(ref["rows"]), 3)
    assert np.array_equal(qf.cpu().numpy(), ref["feats"])
    assert np.abs(qp.cpu().numpy().astype(np.float64) - ref["pos"]).max() <= TOL
    # rows given per kept view give the same bits
    kept = c["kept"]
    again = lift_queries.lift_queries(views, _t(c["masks"][size][kept], d), _t(c["scores"][kept], d), _t(feats[kept], d), **K.ROOM_RULE)
    assert torch.equal(again[0], qf) and torch.equal(again[1], qp)


def _lifter_state(lifter):
    return [lifter.centres(), lifter.counts(), lifter.medians_mm()] + list(lifter.result())


@pytest.mark.parametrize("size", [(24, 32), (17, 23)])
def test_same_bits_whatever_the_cut_the_mask_dtype_and_the_stream(size):
    from segdino3d_amd import lift_queries, ops
    d = dev()
    c = K.room_case()
    feats = K.make_feats(1, K.N_VIEWS, 6, 64, np.float16)
    scores = c["scores"]

    def run(cuts, as_bool, kind="u16"):
        lifter = lift_queries.QueryLifter(64, max_queries=40, **K.ROOM_RULE)
        for lo, hi in cuts:
            lifter.add(_views(c, d, kind, lo, hi), _masks(c, size, d, as_bool, lo, hi), _t(scores[lo:hi], d), _t(feats[lo:hi], d))
        return _lifter_state(lifter)

    base = run([(0, 70)], False)
    assert base[3].shape[0] == 40
    for other in (run([(0, 1), (1, 33), (33, 70)], False), run([(0, 70)], True), run([(0, 70)], False, "f32"), run([(0, 70)], False)):
        assert all(torch.equal(a, b) for a, b in zip(base, other))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with ops.use_stream(side):
        other = run([(0, 20), (20, 70)], True)
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(a, b) for a, b in zip(base, other))


def test_selection():
    from segdino3d_amd import lift_queries
    d = dev()
    c = K.room_case()
    size = (24, 32)
    feats = K.make_feats(2, K.N_VIEWS, 6, 64, np.float32)
    views, masks, scores_d, feats_d = _views(c, d), _masks(c, size, d), _t(c["scores"], d), _t(feats, d)
    n_valid = len(_reference_result(c, size, feats, K.ROOM_RULE)["rows"])
    variants = [dict(max_queries=m) for m in (None, 0, 5, n_valid, n_valid + 1, n_valid - 1, 10 ** 6)]
    variants += [dict(min_pixels=16), dict(min_pixels=1, score_thr=0.0), dict(score_thr=0.6, max_queries=7), dict(min_pixels=600, max_queries=3)]
    for kw in variants:
        rule = {**K.ROOM_RULE, **kw}
        qf, qp = lift_queries.lift_queries(views, masks, scores_d, feats_d, **rule)
        ref = _reference_result(c, size, feats, rule)
        assert tuple(qf.shape) == (len(ref["rows"]), 64) and tuple(qp.shape) == (len(ref["rows"]), 3), kw
        assert np.array_equal(qf.cpu().numpy(), ref["feats"]), kw                  # the rows of feats are all different: the same row set
        assert np.abs(qp.cpu().numpy().astype(np.float64) - ref["pos"]).max(initial=0.0) <= TOL, kw
    # the tie at the cut of 5 goes to the lower flat index
    flat = c["scores"].reshape(-1)
    valid = R.select(flat, c["ref"][size][1], 0.3, 4, None)
    ranked = sorted(valid.tolist(), key=lambda i: (-flat[i], i))
    assert flat[ranked[4]] == flat[ranked[5]]
    qf, _ = lift_queries.lift_queries(views, masks, scores_d, feats_d, max_queries=5, **K.ROOM_RULE)
    assert np.array_equal(qf.cpu().numpy(), feats.reshape(-1, 64)[sorted(ranked[:5])])
    # no valid query at all
    for kw in (dict(score_thr=2.0), dict(min_pixels=100000), dict(max_queries=0)):
        qf, qp = lift_queries.lift_queries(views, masks, scores_d, feats_d, **kw)
        assert tuple(qf.shape) == (0, 64) and tuple(qp.shape) == (0, 3) and qf.dtype == qp.dtype == torch.float32 and qf.is_cuda
    empty = lift_queries.QueryLifter(64).result()
    assert tuple(empty[0].shape) == (0, 64) and tuple(empty[1].shape) == (0, 3) and empty[0].is_cuda


def test_selection_beyond_one_sort_tile():
    """More rows than the single-workgroup rank sort and scan take (4096 / 16384): the radix sort and the tiled scan do the selection."""
    from segdino3d_amd import ops
    d = dev()
    n = 20000
    rng = np.random.default_rng(5)
    scores = rng.integers(0, 64, n).astype(np.float32) / 64                        # many ties
    scores[rng.integers(0, n, 50)] = np.nan
    count = rng.integers(0, 40, n).astype(np.int32)
    for cap in (None, 0, 1, 777, 5000, n):
        rows, m = ops.lift_query_select(_t(scores, d), _t(count, d), 0.25, 16, cap)
        want = R.select(scores, count, 0.25, 16, cap)
        assert int(m.item()) == len(want) and np.array_equal(rows.cpu().numpy()[:len(want)], want), cap


def test_output_feeds_the_dataset_side():
    """`targets.drop_2d_queries` and the augmentation's `query2d_pos` path take the outputs as they are."""
    from segdino3d_amd import augment, lift_queries, targets
    d = dev()
    c = K.room_case()
    feats = K.make_feats(3, K.N_VIEWS, 6, 64, np.float16)
    qf, qp = lift_queries.lift_queries(_views(c, d), _masks(c, (12, 16), d), _t(c["scores"], d), _t(feats, d), **K.ROOM_RULE)
    M = qf.shape[0]
    target = {"extra_features": {"query2d_feats": qf, "query2d_pos": qp.clone()}}
    kept = targets.drop_2d_queries(target, 0.25, np.random.RandomState(0))
    ef = target["extra_features"]
    assert len(kept) == int(M * 0.75) and tuple(ef["query2d_feats"].shape) == (len(kept), 64) and tuple(ef["query2d_pos"].shape) == (len(kept), 3)
    assert torch.equal(ef["query2d_pos"], qp[torch.from_numpy(kept).to(d)])
    target = {"extra_features": {"query2d_feats": qf, "query2d_pos": qp.clone()}, "pcd_horizontal_flip": True, "pcd_vertical_flip": False}
    points = torch.zeros(4, 6, device=d)
    augment.CustomRandomFlip3D(1.0, 0.0)(points, target)
    want = qp.clone()
    want[:, 0] = -want[:, 0]
    assert torch.allclose(target["extra_features"]["query2d_pos"], want, rtol=0.0, atol=1e-6)


def test_add_does_not_synchronise():
    from segdino3d_amd import lift_queries
    d = dev()
    c = K.room_case()
    feats = _t(K.make_feats(4, K.N_VIEWS, 6, 64, np.float16), d)
    masks, scores = _masks(c, (24, 32), d), _t(c["scores"], d)
    base = lift_queries.QueryLifter(64, **K.ROOM_RULE)
    base.add(_views(c, d), masks, scores, feats)                                      # first calls: allocations, library load
    batches = [(_views(c, d, "u16", lo, hi), masks[lo:hi], scores[lo:hi], feats[lo:hi]) for lo, hi in ((0, 10), (10, 40), (40, 70))]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        lifter = lift_queries.QueryLifter(64, **K.ROOM_RULE)
        for b in batches:                                                             # the store grows twice: 16 -> 40 -> 80 views
            lifter.add(*b)
        centres, counts = lifter.centres(), lifter.counts()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(centres, base.centres()) and torch.equal(counts, base.counts())
    assert all(torch.equal(a, b) for a, b in zip(lifter.result(), base.result()))


def test_wrong_inputs_are_refused():
    from segdino3d_amd import lift2d, lift_queries, ops
    d = dev()
    V, Q, C = 3, 2, 64
    views = lift2d.Views(torch.ones(V, 8, 8, device=d), torch.ones(V, 4, device=d), np.stack([np.eye(4)] * V))
    masks, scores, feats = torch.ones(V, Q, 8, 8, dtype=torch.bool, device=d), torch.ones(V, Q, device=d), torch.zeros(V, Q, C, device=d)
    lifter = lift_queries.QueryLifter(C)
    lifter.add(views, masks, scores, feats)
    assert lifter.counts().tolist() == [[64, 64]] * 3
    for bad in ((masks.cpu(), scores, feats), (masks, scores.cpu(), feats), (masks, scores, feats.cpu())):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            lifter.add(views, *bad)
    with pytest.raises(TypeError, match="bool or uint8"):
        lifter.add(views, masks.float(), scores, feats)
    with pytest.raises(TypeError, match="scores must be fp32"):
        lifter.add(views, masks, scores.double(), feats)
    with pytest.raises(TypeError, match="fp16 or fp32"):
        lifter.add(views, masks, scores, feats.bfloat16())
    with pytest.raises(TypeError, match="earlier calls"):
        lifter.add(views, masks, scores, feats.half())
    with pytest.raises(ValueError, match=r"masks must be \[V, Q, Hm, Wm\], got \[3, 8, 8\]"):
        lifter.add(views, masks[:, 0], scores, feats)
    with pytest.raises(ValueError, match=r"one row of masks per view .* got \[2, 2, 8, 8\]"):
        lifter.add(views, masks[:2], scores, feats)
    with pytest.raises(ValueError, match=r"scores must be .* got \[2, 2\]"):
        lifter.add(views, masks, scores[:2], feats)
    with pytest.raises(ValueError, match=r"scores must be .* got \[3, 1\]"):
        lifter.add(views, masks, scores[:, :1], feats)
    with pytest.raises(ValueError, match=r"feats must be .* got \[3, 1, 64\]"):
        lifter.add(views, masks, scores, feats[:, :1])
    with pytest.raises(ValueError, match=r"feats must be .* got \[3, 2, 32\]"):
        lifter.add(views, masks, scores, feats[:, :, :32])
    with pytest.raises(ValueError, match="earlier calls had 2"):
        lifter.add(views, masks[:, :1], scores[:, :1], feats[:, :1])
    with pytest.raises(ValueError, match="multiple of 8"):
        lift_queries.lift_queries(views, masks, scores, torch.zeros(V, Q, 12, device=d))
    with pytest.raises(ValueError, match=r"feats must be a tensor \[V, Q, C\]"):
        lift_queries.lift_queries(views, masks, scores, feats[0])
    with pytest.raises(TypeError, match="unknown"):
        lift_queries.lift_queries(views, masks, scores, feats, tol_abs=0.1)
    assert lifter.n_views == 3                                                        # a refused call leaves the lifter as it was
    centre, count, median = torch.zeros(V, Q, 3, device=d), torch.zeros(V, Q, dtype=torch.int32, device=d), torch.zeros(V, Q, dtype=torch.int32, device=d)
    args = (views.depth, None, views.intrinsics, views.cam_to_world, masks)
    ops.lift_query_centres(*args, 20000, 100, 50, centre, count, median)
    with pytest.raises(ValueError, match="far_mm"):
        ops.lift_query_centres(*args, 70000, 100, 50, centre, count, median)
    with pytest.raises(ValueError, match="centre"):
        ops.lift_query_centres(*args, 20000, 100, 50, centre[:2], count, median)
    with pytest.raises(ValueError, match="cam_to_world"):
        ops.lift_query_centres(views.depth, None, views.intrinsics, views.cam_to_world[:2], masks, 20000, 100, 50, centre, count, median)
    with pytest.raises(ValueError, match="min_pixels"):
        ops.lift_query_select(scores.view(-1), count.view(-1), 0.3, 0)
    with pytest.raises(ValueError, match="count"):
        ops.lift_query_select(scores.view(-1), count.view(-1)[:3], 0.3, 1)
    with pytest.raises(TypeError):
        ops.lift_query_select(scores.view(-1), count.view(-1).long(), 0.3, 1)
