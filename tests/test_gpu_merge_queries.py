"""csrc/merge_queries.hip + `lift_queries.merge_queries` / `QueryLifter.merged` against the restatement tests/merge_queries_ref.py (the
reference has no counterpart) on the hand cases, the room and the sweeps of tests/merge_queries_case.py.

Bounds.  Labels, the order, `views`, `scores`, `pos` and `reduce="best"` features must EQUAL the restatement: every decision of the rule is
an integer one.  Merged features (`reduce="mean"`): `TOL` = 4 x DEV32 = 4 x 4.519e-06 absolute, four times the largest deviation of the
restatement's mean evaluated sequentially in float32 from the same mean in float64 over these cases (`python tests/merge_queries_case.py`
prints it; profiles/merge_queries.md records it) - the margin of tests/test_gpu_lift2d.py and tests/test_gpu_lift_queries.py.  The kernel is
asked for exactly that float32 sequence (two rounded operations per member, no fused multiply-add), which the tests hold it to as well.
The "same bits" tests carry no tolerance."""
import warnings

import numpy as np
import pytest
import torch

import merge_queries_case as K
import merge_queries_ref as R

pytestmark = pytest.mark.gpu

TOL = 4 * K.DEV32


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _t(a, d):
    return torch.from_numpy(np.array(a)).to(d)                   # a copy: the shared cases are read-only


def _merge(case, d, **kw):
    from segdino3d_amd import lift_queries
    return lift_queries.merge_queries(_t(case["feats"], d), _t(case["centre"], d), _t(case["scores"], d), _t(case["count"], d), case["Q"],
                                      **{**case["rule"], **kw})


def _same_or_close(got, want64, tol):
    """Finite entries within `tol`; NaN and infinities in the same places."""
    fin = np.isfinite(want64)
    assert np.array_equal(fin, np.isfinite(got)) and np.array_equal(np.isnan(want64), np.isnan(got))
    assert np.array_equal(got[~fin & ~np.isnan(got)], want64[~fin & ~np.isnan(want64)].astype(np.float32))
    return float(np.abs(got[fin].astype(np.float64) - want64[fin]).max(initial=0.0))


def _check(case, d, what, **kw):
    got = _merge(case, d, **kw)
    ref = K.reference(case, **kw)
    k, n, C = len(ref["seeds"]), len(case["scores"]), case["feats"].shape[1]
    assert tuple(got.feats.shape) == (k, C) and tuple(got.pos.shape) == (k, 3) and tuple(got.scores.shape) == (k,), what
    assert tuple(got.views.shape) == (k,) and tuple(got.labels.shape) == (n,), what
    assert got.feats.dtype == got.pos.dtype == got.scores.dtype == torch.float32 and got.views.dtype == got.labels.dtype == torch.int32
    assert all(t.is_cuda and t.is_contiguous() for t in got)
    assert np.array_equal(got.labels.cpu().numpy(), ref["labels"]), what
    assert np.array_equal(got.views.cpu().numpy(), ref["views"]), what
    assert np.array_equal(got.scores.cpu().numpy().view(np.int32), ref["scores"].view(np.int32)), what
    assert np.array_equal(got.pos.cpu().numpy().view(np.int32), ref["pos"].view(np.int32)), what
    feats = got.feats.cpu().numpy()
    if {**case["rule"], **kw}.get("reduce", "mean") == "best":
        assert np.array_equal(feats, ref["feats"].astype(np.float32), equal_nan=True), what
    else:
        err = _same_or_close(feats, ref["feats"], TOL)
        print(f"{what}: {n} rows -> {k} clusters, largest feature error {err:.3e} (bound {TOL:.3e})")
        assert err <= TOL, what
        assert np.array_equal(feats, K.reference(case, np.float32, **kw)["feats"], equal_nan=True), what      # the float32 sequence itself
    return got, ref


def test_hand_cases():
    d = dev()
    for case in K.hand_cases():
        got, _ = _check(case, d, case["name"])
        assert got.labels.tolist() == case["expect"]["labels"], case["name"]
        for key in ("views", "pos", "feats"):
            if key in case["expect"]:
                have = getattr(got, key).cpu().numpy()
                assert np.array_equal(have, np.array(case["expect"][key], have.dtype).reshape(have.shape)), (case["name"], key)


SWEEP = K.sweep_cases()


@pytest.mark.parametrize("name", [name for name, _ in SWEEP])
def test_sweeps_equal_the_restatement(name):
    """M in {1, 2, 63, 64, 65, 129, 1000} and 17600 valid rows (the pre-cap); C in {8, 64, 72, 256, 1024} in fp16 and fp32 (C = 8 and 72
    end in a padded 64-wide k step); one cluster of everything; no two rows adjacent; the room."""
    d = dev()
    case = dict(SWEEP)[name]
    _, ref = _check(case, d, name)
    if name == "pre-cap":
        assert len(case["scores"]) > R.MAX_ROWS and int((ref["labels"] >= 0).sum()) == R.MAX_ROWS
    if name.startswith("room"):
        assert len(ref["seeds"]) == K.ROOM_K                                          # tests/test_merge_queries_ref.py: the objects
    if name in ("room-f16", "C72-float32", "M129", "one-cluster"):
        _check(case, d, name + " best", reduce="best")
        _check(case, d, name + " distance only", sim=None)
        _check(case, d, name + " capped", max_queries=3, min_views=2)


def test_no_valid_row_and_no_row():
    d = dev()
    case = K.rows_case(65, 64)
    for kw in (dict(score_thr=2.0), dict(min_pixels=10 ** 7), dict(max_queries=0), dict(min_views=1000)):
        got, _ = _check(case, d, str(kw), **kw)
        assert got.feats.shape[0] == 0 and (got.labels == -1).all()
    from segdino3d_amd import lift_queries
    for C, dt in ((64, torch.float16), (8, torch.float32)):
        got = lift_queries.merge_queries(torch.zeros(0, C, dtype=dt, device=d), torch.zeros(0, 3, device=d), torch.zeros(0, device=d),
                                         torch.zeros(0, dtype=torch.int32, device=d), 4)
        assert tuple(got.feats.shape) == (0, C) and tuple(got.pos.shape) == (0, 3) and got.labels.numel() == 0 and got.feats.is_cuda
    empty = lift_queries.QueryLifter(64).merged()
    assert tuple(empty.feats.shape) == (0, 64) and tuple(empty.pos.shape) == (0, 3) and empty.labels.numel() == 0 and empty.feats.is_cuda


def _unpack(adj, m):
    """int64 words [Mp, Mp / 64] -> bool [m, m]."""
    words = adj.cpu().numpy().view(np.uint64)
    bits = (words[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    return bits.reshape(words.shape[0], -1)[:m, :m].astype(bool)


@pytest.mark.parametrize("C", [8, 64, 72, 256])
def test_mfma_lane_map_with_asymmetric_exact_integers(C):
    """Row i holds (i mod 5) + 1 at channel i mod C and -(i mod 3) - 1 at channel (7 i + 3) mod C (added where the two meet), as small
    integers in fp32: the quantiser scales a row by a power of two, so the codes are these integers times 16, 32 or 64, and every dot
    product differs from its neighbours'.  A swapped or permuted operand map, a transposed accumulator or a ballot bit in the wrong
    place changes bits of the adjacency matrix, which must equal the restatement's for several s7 (all centres coincide)."""
    from segdino3d_amd import ops
    d = dev()
    m = 200 if C < 256 else 600                                                       # enough rows for the channels to wrap and meet
    f = np.zeros((m, C), np.float32)
    for i in range(m):
        f[i, i % C] += (i % 5) + 1
        f[i, (7 * i + 3) % C] += -(i % 3) - 1
    scores = np.linspace(0.9, 0.4, m).astype(np.float32)
    scores[::7] += np.float32(0.3)                                                    # rank != row
    centre, count = np.zeros((m, 3), np.float32), np.full(m, 16, np.int32)
    rows = R.ranked_rows(centre, scores, count, 0.3, 16)
    codes, nrm = R.quantise(f[rows])
    assert len(rows) == m and len(np.unique(codes.astype(np.int64) @ codes.astype(np.int64).T)) > 20
    seen = set()
    for s7 in (0, 1, 64, 96, 112, 128):
        ws = ops.merge_queries_adjacency(_t(f, d), _t(centre, d), _t(scores, d), _t(count, d), 0.3, 16, 307, s7)
        rank_row, adj = ops.merge_queries_adjacency_read(m, C, ws)
        assert np.array_equal(rank_row.cpu().numpy()[:m], rows) and (rank_row[m:] == -1).all()
        want = R.adjacency_bits(np.zeros((m, 3), np.int32), codes, nrm, 307, s7)
        got = _unpack(adj, m)
        assert np.array_equal(got, want), (C, s7, int((got != want).sum()))
        assert not np.tril(got).any()                                                  # the diagonal tile is masked
        seen.add(int(want.sum()))
    assert len(seen) >= 4                                                              # the thresholds cut at different places


# ---------------------------------------------------------------------------------------------- through the lifter
def _lifter_inputs(d, C=64, dtype=np.float16):
    """The room of tests/lift_queries_case.py (70 views x 6 queries) with one feature per query slot plus noise: the views of a slot
    that see the same surface merge."""
    import lift_queries_case as LK
    from segdino3d_amd import lift2d
    c = LK.room_case()
    rng = np.random.default_rng(21)
    base = rng.standard_normal((1, 6, C))
    feats = (base + 0.1 * rng.standard_normal((LK.N_VIEWS, 6, C))).astype(dtype)

    def batch(lo, hi):
        views = lift2d.Views(_t(c["depth_u16"][lo:hi], d), _t(c["intr"][lo:hi], d), c["poses"][lo:hi], LK.DEPTH_SCALE)
        return views, _t(c["masks"][(24, 32)][lo:hi], d), _t(c["scores"][lo:hi], d), _t(feats[lo:hi], d)
    return batch, dict(LK.ROOM_RULE), LK.N_VIEWS


MERGE = dict(radius=0.5, sim=0.75, min_views=2)


def _lifted(d, cuts):
    from segdino3d_amd import lift_queries
    batch, rule, V = _lifter_inputs(d)
    lifter = lift_queries.QueryLifter(64, **rule)
    edges = np.linspace(0, V, cuts + 1).astype(int)
    for lo, hi in zip(edges[:-1], edges[1:]):
        lifter.add(*batch(int(lo), int(hi)))
    return lifter


def test_merged_equals_the_restatement_over_the_lifters_stores():
    d = dev()
    lifter = _lifted(d, 1)
    before = lifter.result()
    got = lifter.merged(**MERGE)
    n = lifter.n_views * lifter.n_queries
    ref = R.merge(lifter._feats[:lifter.n_views].view(n, 64).cpu().numpy(), lifter.centres().view(n, 3).cpu().numpy(),
                  lifter._scores[:lifter.n_views].view(n).cpu().numpy(), lifter.counts().view(n).cpu().numpy(), lifter.n_queries,
                  feat_dtype=np.float32, score_thr=lifter.rule["score_thr"], min_pixels=lifter.rule["min_pixels"], **MERGE)
    assert 2 <= len(ref["seeds"]) < before[0].shape[0] / 4                            # dozens of rows per surface became a few queries
    assert np.array_equal(got.labels.cpu().numpy(), ref["labels"]) and np.array_equal(got.views.cpu().numpy(), ref["views"])
    assert np.array_equal(got.pos.cpu().numpy(), ref["pos"]) and np.array_equal(got.feats.cpu().numpy(), ref["feats"])
    after = lifter.result()                                                           # result() is what it was
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    again = lifter.merged(**MERGE)                                                    # merged() twice: the same bits
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    batch, _, V = _lifter_inputs(d)                                                   # the lifter goes on afterwards
    lifter.add(*batch(0, 5))
    assert lifter.merged(**MERGE).labels.numel() == (V + 5) * 6


def test_same_bits_whatever_the_cut_and_the_stream():
    from segdino3d_amd import ops
    d = dev()
    base = _lifted(d, 1).merged(**MERGE)
    assert base.feats.shape[0] >= 2
    for cuts in (2, 7):
        other = _lifted(d, cuts).merged(**MERGE)
        assert all(torch.equal(a, b) for a, b in zip(base, other)), cuts
    # two lifters on two streams at once, each with its own workspace
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    out = []
    for s, cuts in zip(streams, (1, 2)):
        s.wait_stream(torch.cuda.current_stream())
        with ops.use_stream(s):
            out.append(_lifted(d, cuts).merged(**MERGE))
    for s in streams:
        torch.cuda.current_stream().wait_stream(s)
    for other in out:
        assert all(torch.equal(a, b) for a, b in zip(base, other))


def test_one_shot_form_feeds_the_dataset_side(tmp_path):
    """`lift_queries(..., merge=dict(...))` gives the pair that `extra_features`, `targets.drop_2d_queries` and `io_scene.pack_scene` take."""
    from segdino3d_amd import io_scene, lift_queries, targets
    d = dev()
    batch, rule, V = _lifter_inputs(d)
    qf, qp = lift_queries.lift_queries(*batch(0, V), merge=MERGE, **rule)
    want = _lifted(d, 1).merged(**MERGE)
    assert torch.equal(qf, want.feats) and torch.equal(qp, want.pos) and qf.dtype == qp.dtype == torch.float32
    plain = lift_queries.lift_queries(*batch(0, V), **rule)                           # without `merge`: as before
    assert all(torch.equal(a, b) for a, b in zip(plain, _lifted(d, 1).result()))
    target = {"extra_features": {"query2d_feats": qf, "query2d_pos": qp.clone()}}
    kept = targets.drop_2d_queries(target, 0.5, np.random.RandomState(0))
    assert tuple(target["extra_features"]["query2d_feats"].shape) == (len(kept), 64)
    N = 32
    scene = {"points": torch.rand(N, 6), "super_points": torch.zeros(N, dtype=torch.long), "points_2dfeats": torch.rand(N, 64),
             "query2d_feats": qf.cpu(), "query2d_pos": qp.cpu()}
    path = str(tmp_path / "scene.sd3d")
    io_scene.pack_scene(path, scene)
    back = io_scene.load_packed(path)
    assert torch.equal(back["query2d_feats"], qf.cpu()) and torch.equal(back["query2d_pos"], qp.cpu())


def test_merged_reads_the_host_once():
    d = dev()
    lifter = _lifted(d, 1)
    lifter.merged(**MERGE)                                                            # first call: allocations, library load
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            lifter.merged(**MERGE)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in caught if "synchroniz" in str(w.message).lower()]
    assert len(syncs) == 1, [str(w.message) for w in caught]


def test_wrong_inputs_are_refused():
    from segdino3d_amd import lift_queries, ops
    d = dev()
    n, C = 10, 16
    feats, centre = torch.zeros(n, C, device=d), torch.zeros(n, 3, device=d)
    scores, count = torch.ones(n, device=d), torch.full((n,), 16, dtype=torch.int32, device=d)
    assert lift_queries.merge_queries(feats, centre, scores, count, 2).labels.tolist() == list(range(n))       # zero codes: clusters of one
    for bad in ((feats.cpu(), centre, scores, count), (feats, centre.cpu(), scores, count), (feats, centre, scores.cpu(), count),
                (feats, centre, scores, count.cpu())):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            lift_queries.merge_queries(*bad, 2)
    with pytest.raises(ValueError, match="1 <= C <= 1024"):
        lift_queries.merge_queries(torch.zeros(n, 1032, device=d), centre, scores, count, 2)
    with pytest.raises(TypeError, match="fp16 or fp32"):
        lift_queries.merge_queries(feats.double(), centre, scores, count, 2)
    with pytest.raises(ValueError, match="centre"):
        lift_queries.merge_queries(feats, centre[:5], scores, count, 2)
    with pytest.raises(ValueError, match="scores"):
        lift_queries.merge_queries(feats, centre, scores[:5], count, 2)
    with pytest.raises(TypeError):
        lift_queries.merge_queries(feats, centre, scores, count.long(), 2)
    with pytest.raises(ValueError, match="queries_per_view"):
        lift_queries.merge_queries(feats, centre, scores, count, 0)
    for kw, err, match in ((dict(radius=0.0), ValueError, "radius"), (dict(radius=2000.0), ValueError, "radius"), (dict(sim=1.5), ValueError, "sim"),
                           (dict(sim=0.0), ValueError, "sim"), (dict(min_views=0), ValueError, "min_views"), (dict(max_queries=-1), ValueError, "max_queries"),
                           (dict(reduce="median"), ValueError, "reduce"), (dict(min_pixels=0), ValueError, "min_pixels"), (dict(gate=1), TypeError, "unknown")):
        with pytest.raises(err, match=match):
            lift_queries.merge_queries(feats, centre, scores, count, 2, **kw)
        with pytest.raises(err, match=match):
            lift_queries.QueryLifter(64).merged(**kw)
    with pytest.raises(TypeError, match="merge must be"):
        lift_queries.lift_queries(None, None, None, torch.zeros(1, 1, 8), merge=3)
    with pytest.raises(ValueError, match="radius_q"):
        ops.merge_queries_adjacency(feats, centre, scores, count, 0.3, 16, 0, 96)
    with pytest.raises(ValueError, match="sim_q"):
        ops.merge_queries_adjacency(feats, centre, scores, count, 0.3, 16, 307, 129)
    ws = ops.merge_queries_adjacency(feats, centre, scores, count, 0.3, 16, 307, 96)
    with pytest.raises(ValueError, match="workspace"):
        ops.merge_queries_sweep(n, C, ws[:256])
    with pytest.raises(ValueError, match="K"):
        ops.merge_queries_emit(feats, scores, count, n + 1, False, ws)
