"""csrc/lift2d.hip + segdino3d_amd/lift2d.py against the float64 restatement tests/lift2d_ref.py (the reference has no counterpart) on
the analytic room of tests/lift2d_case.py.

Bounds.  Visibility bits and counts must EQUAL the restatement: the case builder removed every point with a decision within 1e-3 px /
m of its boundary, four orders of magnitude above fp32 rounding at these coordinates.  The "same bits" tests carry no tolerance
either.  Values (accumulate + finish, given the restatement's mask): `TOL` = 4 x 8.979e-06 = 3.592e-05 absolute, four times the largest
deviation of the restatement evaluated in float32 from the same restatement in float64 on exactly these cases (`python
tests/lift2d_case.py` prints it; profiles/lift_2d.md records it; summation order and FMA contraction differ between numpy and the
device).  An fp16 output adds its own rounding, |x| * 2^-11 (+ 2^-25 below the normal range)."""
import numpy as np
import pytest
import torch

import lift2d_case as K
import lift2d_ref as R

pytestmark = pytest.mark.gpu

TOL = 4 * K.DEV32                    # 4 x 8.979e-06; profiles/lift_2d.md, "tolerance"


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _t(a, d):
    return torch.from_numpy(np.array(a)).to(d)                   # a copy: the shared cases are read-only


def _views(c, d, V=None, kind="u16", lo=0):
    from segdino3d_amd import lift2d
    V = len(c["poses"]) if V is None else V
    depth = c["depth_u16"][lo:V] if kind == "u16" else c["depth_f32"][lo:V]
    return lift2d.Views(_t(depth, d), _t(c["intr"][lo:V], d), c["poses"][lo:V], K.DEPTH_SCALE if kind == "u16" else None)


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_visibility_equals_the_restatement(kind):
    from segdino3d_amd import lift2d
    d = dev()
    c = K.build_case()
    depth, scale = (c["depth_u16"], K.DEPTH_SCALE) if kind == "u16" else (c["depth_f32"], None)
    pts_d = _t(c["points"], d)
    seen = 0
    for rule in K.RULES:
        want = R.outcomes(c["points"], c["w2c"], c["intr"], depth, scale, **rule) == R.VISIBLE
        for V in (1, 31, 32, 33, 70):
            views = _views(c, d, V, kind)
            for N in (1, 63, 64, 65, 1000):
                bits, count = lift2d.visibility(pts_d[:N], views, **rule)
                assert bits.dtype == torch.int32 and tuple(bits.shape) == (N, (V + 31) // 32) and count.dtype == torch.int32
                assert np.array_equal(bits.cpu().numpy(), R.pack_bits(want[:N, :V])), (rule, V, N)
                assert np.array_equal(count.cpu().numpy(), want[:N, :V].sum(axis=1)), (rule, V, N)
                seen += int(want[:N, :V].sum())
    assert seen > 10000


def test_dropped_poses_and_count_accumulation():
    from segdino3d_amd import lift2d
    d = dev()
    c = K.build_case(n_bad_poses=3)
    views = _views(c, d)
    assert views.n_given == 70 and len(views) == 67 and np.array_equal(views.kept, c["kept"])
    want = R.outcomes(c["points"], c["w2c"], c["intr"][c["kept"]], c["depth_u16"][c["kept"]], K.DEPTH_SCALE) == R.VISIBLE
    pts_d = _t(c["points"], d)
    bits, count = lift2d.visibility(pts_d, views)
    assert np.array_equal(bits.cpu().numpy(), R.pack_bits(want))
    bits2, count2 = lift2d.visibility(pts_d, views, count=count)
    assert count2 is count and np.array_equal(count.cpu().numpy(), 2 * want.sum(axis=1))
    # maps given per GIVEN view are selected; the result equals the one from maps per kept view
    maps = K.make_maps(3, 70, [(7, 9)], 64, np.float16)[0]
    a = lift2d.lift_point_features(pts_d, views, _t(maps, d))
    b = lift2d.lift_point_features(pts_d, views, _t(maps[c["kept"]], d))
    assert torch.equal(a, b)
    ref = R.lift_point_features(c["points"], c["poses"], c["intr"], c["depth_u16"], [maps], K.DEPTH_SCALE)
    assert np.abs(a.cpu().numpy() - ref[0]).max() <= TOL


def _run_ops(c, case, d):
    """accumulate + finish through the thin wrappers, given the restatement's mask -> (out, [mean_s])"""
    from segdino3d_amd import ops
    V, C = case["V"], case["C"]
    pts_d, w2c, intr = _t(c["points"], d), _t(c["w2c"][:V], d), _t(c["intr"][:V], d)
    bits = _t(R.pack_bits(case["vis"]), d)
    count = _t(case["vis"].sum(axis=1).astype(np.int32), d)
    N, S = len(c["points"]), len(case["maps"])
    out_dtype = getattr(torch, case["out_dtype"])
    acc = torch.empty(N, C, device=d) if S > 1 else None
    out, means = None, []
    for s, m in enumerate(case["maps"]):
        total = torch.zeros(N, C, device=d)
        ops.lift_accumulate(pts_d, w2c, intr, (c["H"], c["W"]), bits, _t(m, d), total)
        means.append(ops.lift_finish(total, count, out_dtype=out_dtype))
        out = ops.lift_finish(total, count, s, S, acc=acc, out_dtype=out_dtype)
    return out, means


@pytest.mark.parametrize("name", [case[0] for case in K.VALUE_CASES])
def test_accumulate_and_finish_given_the_mask(name):
    d = dev()
    c, case = K.build_case(), K.value_case(name)
    ref_out, ref_means, ref_count = case["ref"]
    out, means = _run_ops(c, case, d)
    assert out.dtype == getattr(torch, case["out_dtype"]) and tuple(out.shape) == ref_out.shape
    # the case has what it is meant to test: seen and unseen points, and (on maps wider than one texel) taps clamped at the border
    assert (ref_count == 0).sum() > 10 and (ref_count > 0).sum() > 500
    _, u, v = R.project(c["points"], c["w2c"][:case["V"]], c["intr"][:case["V"]])
    Hf, Wf = case["maps"][0].shape[1:3]
    xf, yf = (u + 0.5) * Wf / c["W"] - 0.5, (v + 0.5) * Hf / c["H"] - 0.5
    clamped = case["vis"] & ((xf < 0) | (xf > Wf - 1) | (yf < 0) | (yf > Hf - 1))
    assert clamped.sum() > 20, clamped.sum()
    for got, want in zip([out] + means, [ref_out] + ref_means):
        got = got.float().cpu().numpy().astype(np.float64)
        bound = TOL + (np.abs(want) * 2.0 ** -11 + 2.0 ** -25 if case["out_dtype"] == "float16" else 0.0)
        err = np.abs(got - want)
        print(f"{name}: largest error {err.max():.3e} (bound {TOL:.3e})")
        assert (err <= bound).all(), err.max()
        assert not got[ref_count == 0].any()                       # unseen and non-finite points: exact zeros


@pytest.mark.parametrize("name", ["c256_f16_3scales_f16out", "c320_f32_15x20"])
def test_public_interface_matches_and_same_bits(name):
    """`lift_point_features` / `PointFeatureAccumulator` against the restatement, then the same bits whatever the cut of the views
    into passes and `add` calls, on another stream, and twice."""
    from segdino3d_amd import lift2d, ops
    d = dev()
    c, case = K.build_case(), K.value_case(name)
    V, C, S = case["V"], case["C"], len(case["maps"])
    out_dtype = getattr(torch, case["out_dtype"])
    pts_d = _t(c["points"], d)
    views = _views(c, d, V)
    maps = [_t(m, d) for m in case["maps"]]
    base, counts = lift2d.lift_point_features(pts_d, views, maps if S > 1 else maps[0], out_dtype=out_dtype, return_counts=True)
    ref_out, ref_means, ref_count = case["ref"]
    assert np.array_equal(counts.cpu().numpy(), ref_count)
    bound = TOL + (np.abs(ref_out) * 2.0 ** -11 + 2.0 ** -25 if out_dtype == torch.float16 else 0.0)
    assert (np.abs(base.float().cpu().numpy().astype(np.float64) - ref_out) <= bound).all()
    bad = ~np.isfinite(c["points"]).all(axis=1) | (np.abs(c["points"]) >= 1e30).any(axis=1)
    assert bad.sum() >= 6 and not counts.cpu().numpy()[bad].any() and not base.float().cpu().numpy()[bad].any()
    for vpp in (1, 32, V):
        again = lift2d.lift_point_features(pts_d, views, maps, views_per_pass=vpp, out_dtype=out_dtype)
        assert torch.equal(again, base), vpp
    assert torch.equal(lift2d.lift_point_features(pts_d, views, maps, out_dtype=out_dtype), base)                # two runs
    acc = lift2d.PointFeatureAccumulator(pts_d, C, S)
    for lo, hi in ((0, 20), (20, 52), (52, V)):                                                                     # three adds
        acc.add(_views(c, d, hi, lo=lo), [m[lo:hi] for m in maps])
    assert torch.equal(acc.result(out_dtype=out_dtype), base) and torch.equal(acc.counts(), counts)
    scales = acc.result(return_scales=True)
    assert len(scales) == S
    for got, want in zip(scales, ref_means):
        assert np.abs(got.cpu().numpy() - want).max() <= TOL
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with ops.use_stream(side):
        other = lift2d.lift_point_features(pts_d, views, maps, out_dtype=out_dtype)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(other, base)


def test_accumulator_does_not_synchronise():
    from segdino3d_amd import lift2d
    d = dev()
    c, case = K.build_case(), K.value_case("c64_f32_3scales")
    pts_d = _t(c["points"], d)
    views = _views(c, d)
    maps = [_t(m, d) for m in case["maps"]]
    base = lift2d.lift_point_features(pts_d, views, maps)                               # first calls: allocations, library load
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        acc = lift2d.PointFeatureAccumulator(pts_d, 64, 3, views_per_pass=32)
        acc.add(views, maps)
        out = acc.result()
        half = acc.result(out_dtype=torch.float16)
        scales = acc.result(return_scales=True)
        counts = acc.counts()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(out, base) and half.dtype == torch.float16 and len(scales) == 3
    assert np.array_equal(counts.cpu().numpy(), case["ref"][2])


def test_wrappers_refuse_wrong_inputs():
    from segdino3d_amd import lift2d, ops
    d = dev()
    N, V, H, W, C = 10, 3, 4, 6, 64
    pts, w2c, intr = torch.zeros(N, 3, device=d), torch.zeros(V, 3, 4, device=d), torch.ones(V, 4, device=d)
    depth = torch.zeros(V, H, W, device=d)
    bits, maps, total = torch.zeros(N, 1, dtype=torch.int32, device=d), torch.zeros(V, 2, 2, C, device=d), torch.zeros(N, C, device=d)
    count = torch.zeros(N, dtype=torch.int32, device=d)
    ops.lift_visibility(pts, w2c, intr, depth)
    ops.lift_accumulate(pts, w2c, intr, (H, W), bits, maps, total)
    ops.lift_finish(total, count)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lift_visibility(pts.cpu(), w2c, intr, depth)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lift_visibility(pts, w2c, intr, depth.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lift_accumulate(pts, w2c, intr, (H, W), bits, maps.cpu(), total)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lift_finish(total.cpu(), count)
    with pytest.raises(ValueError):
        ops.lift_visibility(pts[:, :2].contiguous(), w2c, intr, depth)
    with pytest.raises(ValueError):
        ops.lift_visibility(pts.double(), w2c, intr, depth)
    with pytest.raises(ValueError, match="world_to_cam"):
        ops.lift_visibility(pts, torch.zeros(V, 4, 4, device=d), intr, depth)
    with pytest.raises(ValueError, match="intrinsics"):
        ops.lift_visibility(pts, w2c, intr[:2], depth)
    with pytest.raises(ValueError, match="depth"):
        ops.lift_visibility(pts, w2c, intr, depth[:2])
    with pytest.raises(TypeError, match="uint16 or fp32"):
        ops.lift_visibility(pts, w2c, intr, depth.half())
    with pytest.raises(ValueError, match="depth_scale"):
        ops.lift_visibility(pts, w2c, intr, torch.zeros(V, H, W, dtype=torch.uint16).to(d))
    with pytest.raises(ValueError, match="border"):
        ops.lift_visibility(pts, w2c, intr, depth, border=-1)
    with pytest.raises(TypeError):
        ops.lift_visibility(pts, w2c.double(), intr, depth)
    for bad_c in (48, 32, 1088):
        with pytest.raises(ValueError, match="multiple of 64"):
            ops.lift_accumulate(pts, w2c, intr, (H, W), bits, torch.zeros(V, 2, 2, bad_c, device=d), torch.zeros(N, bad_c, device=d))
        with pytest.raises(ValueError, match="multiple of 64"):
            ops.lift_finish(torch.zeros(N, bad_c, device=d), count)
    with pytest.raises(ValueError, match="multiple of 64"):
        lift2d.PointFeatureAccumulator(pts, 48)
    with pytest.raises(TypeError, match="fp16 or fp32"):
        ops.lift_accumulate(pts, w2c, intr, (H, W), bits, maps.bfloat16(), total)
    with pytest.raises(ValueError, match="maps"):
        ops.lift_accumulate(pts, w2c, intr, (H, W), bits, maps[:2], total)
    with pytest.raises(ValueError, match="bits"):
        ops.lift_accumulate(pts, w2c, intr, (H, W), torch.zeros(N, 2, dtype=torch.int32, device=d), maps, total)
    with pytest.raises(TypeError):
        ops.lift_accumulate(pts, w2c, intr, (H, W), bits.long(), maps, total)
    with pytest.raises(ValueError, match="sum"):
        ops.lift_accumulate(pts, w2c, intr, (H, W), bits, maps, total[:5])
    with pytest.raises(ValueError, match="v0"):
        ops.lift_accumulate(pts, w2c, intr, (H, W), bits, maps, total, 2, 5)
    with pytest.raises(ValueError, match="count"):
        ops.lift_finish(total, count[:5])
    with pytest.raises(TypeError):
        ops.lift_finish(total, count.long())
    with pytest.raises(ValueError, match="acc"):
        ops.lift_finish(total, count, 0, 2)
    with pytest.raises(TypeError, match="fp32 or fp16"):
        ops.lift_finish(total, count, out_dtype=torch.bfloat16)
    acc = lift2d.PointFeatureAccumulator(pts, C, 2)
    views = lift2d.Views(depth, intr, np.stack([np.eye(4)] * V))
    with pytest.raises(ValueError, match="2 scale"):
        acc.add(views, maps)
    with pytest.raises(ValueError, match="channels-last"):
        acc.add(views, [maps, torch.zeros(V, 2, 2, 128, device=d)])
    with pytest.raises(ValueError, match="one per view"):
        acc.add(views, [maps, maps[:2]])
