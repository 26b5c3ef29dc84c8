"""Pins the numpy restatement of the query lifting (tests/lift_queries_ref.py) - the only thing csrc/lift_queries.hip can be compared
with, since the reference has no code that makes `query2d_feats` / `query2d_pos` - on medians, counts and centres worked out by hand,
the properties the room case must have, the selection order against a plain Python sort, and the host-side checks of the module.
No GPU."""
import math

import numpy as np
import pytest
import torch

import lift_queries_case as K
import lift_queries_ref as R


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("which", ["u16", "f32"])
def test_hand_built_medians_counts_and_centres(which, dtype):
    case, scale, expect = (K.hand_case_u16(), K.DEPTH_SCALE, K.HAND_EXPECT_U16) if which == "u16" else (K.hand_case_f32(), None, K.HAND_EXPECT_F32)
    seen = 0
    for kw, table in expect:
        centre, count, median, _ = K.hand_ref(case[0], scale, *case[1:], dtype=dtype, **kw)
        assert centre.dtype == np.float32
        for (v, q), (k_med, n, c) in table.items():
            assert (median[v, q], count[v, q]) == (k_med, n), (kw, v, q, median[v, q], count[v, q])
            assert np.allclose(centre[v, q], c, rtol=1e-6, atol=2e-6), (kw, v, q, centre[v, q])
            seen += 1
    assert seen >= 3


def test_mask_sample_is_the_nearest_mask_pixel():
    for Hd, Hm in ((24, 24), (24, 12), (24, 48), (24, 17), (480, 240), (7, 50), (50, 7), (1, 9), (9, 1)):
        ym, _ = R.mask_samples(Hd, 1, Hm, 1)
        centre = (np.arange(Hd) + 0.5) * Hm / Hd                     # the depth pixel's centre in mask pixels: pixel j covers [j, j + 1)
        assert np.array_equal(ym, np.floor(centre).astype(np.int64)) and ym.min() >= 0 and ym.max() < Hm
    assert np.array_equal(R.mask_samples(4, 4, 4, 4)[1], np.arange(4))


def test_depth_keys_decide_on_floats():
    far = 65535
    raw = np.array([0, 1, 2, 255, 256, 999, 1000, 20000, 20001, 65535], np.uint16)
    d, k = R.depth_keys(raw, K.DEPTH_SCALE, far)
    assert np.array_equal(k, raw.astype(np.int64))                    # millimetres in, millimetres out, 0 invalid
    assert np.array_equal(R.depth_keys(raw, K.DEPTH_SCALE, 20000)[1], np.where(raw <= 20000, raw, 0))
    every = np.arange(65536, dtype=np.uint16)
    assert np.array_equal(R.depth_keys(every, K.DEPTH_SCALE, far)[1], every.astype(np.int64))
    f = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 70.0, 1e30, 65.5354, 65.5356, 0.0004, 0.0006, 1.2344, 1.2346], np.float32)
    assert np.array_equal(R.depth_keys(f, None, far)[1], [0, 0, 0, 0, 0, 0, 0, 0, 65535, 0, 0, 1, 1234, 1235])


def test_room_case_has_what_it_is_meant_to_test():
    c = K.room_case()                                                  # the builder asserts the rest ("choose another seed")
    assert c["dev32"] <= K.DEV32 and K.dev32() == pytest.approx(K.DEV32, rel=1e-3)
    for size in K.MASK_SIZES:
        centre, count, median, n_valid = c["ref"][size]
        assert count.shape == (K.N_VIEWS, 6) and (count <= n_valid).all()
        assert (n_valid[:, K.Q_WHOLE] > 256).all() and count.max() >= 512    # more valid pixels than the owner has lanes
        assert (count[:, K.Q_DILATED] < n_valid[:, K.Q_DILATED]).any()
        assert ((median > 0) == (n_valid > 0)).all()
        assert not centre[count == 0].any()
        m = c["masks"][size]
        assert m.dtype == np.uint8 and m.max() > 1                     # "non-zero = set" is exercised
    bad = K.room_case(n_bad_poses=3)
    assert len(bad["kept"]) == K.N_VIEWS - 3 and bad["ref"][(24, 32)][1].shape[0] == K.N_VIEWS - 3
    # the kept views of the case with bad poses are the same views: dropping rows is all that happens
    assert np.array_equal(bad["ref"][(24, 32)][1], c["ref"][(24, 32)][1][bad["kept"]])


def _python_select(scores, count, thr, min_pixels, cap):
    valid = [i for i, (s, n) in enumerate(zip(scores, count)) if not math.isnan(s) and s >= np.float32(thr) and n >= min_pixels]
    if cap is not None and len(valid) > cap:
        valid = sorted(sorted(valid, key=lambda i: (-scores[i], i))[:cap])
    return valid


def test_selection_order_against_a_plain_sort():
    c = K.room_case()
    scores = c["scores"].reshape(-1)
    count = c["ref"][(24, 32)][1].reshape(-1)
    assert np.isnan(scores).sum() == 1 and np.abs(scores[~np.isnan(scores)] - 0.3).min() > 0.015
    n_valid = len(R.select(scores, count, 0.3, 4, None))
    assert 20 < n_valid < len(scores)
    for thr, min_pixels in ((0.3, 4), (0.3, 16), (0.6, 4), (0.0, 1)):
        for cap in (None, 0, 1, 5, n_valid - 1, n_valid, n_valid + 1, 10 ** 6):
            got = R.select(scores, count, thr, min_pixels, cap)
            assert got.tolist() == _python_select(scores.tolist(), count.tolist(), thr, min_pixels, cap), (thr, min_pixels, cap)
    # two equal scores straddle the cut at 5: the lower flat index is taken
    valid = R.select(scores, count, 0.3, 4, None)
    ranked = sorted(valid.tolist(), key=lambda i: (-scores[i], i))
    assert scores[ranked[4]] == scores[ranked[5]] and ranked[4] < ranked[5]
    five = R.select(scores, count, 0.3, 4, 5).tolist()
    assert ranked[4] in five and ranked[5] not in five


def test_rule_defaults_agree_with_the_module():
    from segdino3d_amd import lift_queries
    assert lift_queries.RULE_DEFAULTS == R.RULE_DEFAULTS
    r = lift_queries._rule(dict(gate_abs=0.25, far=65.535))
    assert (r["far_mm"], r["gate_mm"], r["gate_permille"]) == (65535, 250, 50)
    assert R.rule(gate_abs=0.25, far=65.535)["gate_mm"] == 250
    with pytest.raises(TypeError, match="unknown"):
        lift_queries._rule(dict(tol_abs=0.1))
    with pytest.raises(TypeError, match="unknown"):
        lift_queries.QueryLifter(64, near=0.1)
    for bad in (dict(far=0.0), dict(far=70.0), dict(gate_abs=-1.0), dict(min_pixels=0), dict(min_pixels=2.5), dict(max_queries=-1)):
        with pytest.raises(ValueError):
            lift_queries._rule(bad)
    for bad_c in (0, 4, 12, 100):
        with pytest.raises(ValueError, match="multiple of 8"):
            lift_queries.QueryLifter(bad_c)


def test_header_constants_and_views_cam_to_world():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "segdino3d_hip.h")).read()
    assert int(re.search(r"#define SD3D_LIFTQ_FIXED_BITS (\d+)", header).group(1)) == R.FIXED_BITS == 20
    assert int(re.search(r"#define SD3D_LIFTQ_WORLD_BITS (\d+)", header).group(1)) == R.WORLD_BITS == 14
    from segdino3d_amd import _lib
    for name in ("sd3d_lift_query_centres", "sd3d_lift_query_select_ws_bytes", "sd3d_lift_query_select", "sd3d_lift_query_gather"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.sd3d_lift_query_select_ws_bytes(1000) >= 1000 * 32 and lib.sd3d_lift_query_select_ws_bytes(0) > 0


def test_cpu_inputs_are_refused():
    from segdino3d_amd import lift2d, lift_queries, ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lift2d.Views(torch.zeros(1, 8, 8), np.ones((1, 4), np.float32), np.eye(4)[None])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lift_query_select(torch.zeros(4), torch.zeros(4, dtype=torch.int32), 0.3, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lift_query_gather(torch.zeros(4, 8), torch.zeros(4, 3), torch.zeros(2, dtype=torch.int32), 2)
    with pytest.raises(TypeError, match="Views"):
        lift_queries.QueryLifter(64).add(None, torch.zeros(1, 1, 8, 8, dtype=torch.bool), torch.zeros(1, 1), torch.zeros(1, 1, 64))
