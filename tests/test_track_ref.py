"""The restatement of the tracking rule (tests/track_ref.py) does what the rule is for, on the CPU: it follows the room trajectory, a
single wall is harmless, a jump beyond the basin shows, and the sums do not depend on the order of the samples.  The kernels are
pinned against this restatement in tests/test_gpu_track.py."""
import numpy as np

import fuse_views_case as K
import fuse_views_ref as FR
import track_case as C
import track_ref as R
import tsdf_ref as TR


def test_room_trajectory_is_followed():
    """5 frames of 120 x 160, voxel 0.02, trunc 0.08, 2 cm + 0.7 degrees a frame, default schedule: no frame is lost and every frame
    ends under one tenth of the error it started from (the previous estimate against this frame's truth), in translation and in
    angle.  Measured: 0.070 - 0.081 of the translation and 0.066 - 0.087 of the angle (profiles/track.md)."""
    c, out = C.room_trajectory(), C.room_trajectory_ref()
    assert not out["lost"].any()
    assert np.array_equal(out["poses"][0], c["poses"][0])
    for v in range(1, len(c["poses"])):
        t0, r0 = C.pose_error(c["poses"][v], out["poses"][v - 1])
        t1, r1 = C.pose_error(c["poses"][v], out["poses"][v])
        print(f"frame {v}: {t0 * 1e3:.2f} mm {r0:.3f} deg -> {t1 * 1e3:.3f} mm {r1:.4f} deg")
        assert t0 > 0.015 and r0 > 0.5                                                  # the frame did start a frame's motion away
        assert t1 < 0.1 * t0 and r1 < 0.1 * r0
        assert out["count"][v] > 10000


def test_degenerate_wall_is_harmless():
    """A wall along the voxel grid, the camera moved 1 cm along its normal: the translation along the normal is recovered and the
    in-plane components stay at zero exactly (their columns of A are exactly 0: step 5 leaves those variables alone)."""
    c = K.wall(48, 64, 0.5)
    vol = TR.integrate(c["depth_u16"], C.DEPTH_SCALE, c["intr"], c["poses"], c["colors"], min_weight=1)
    nearer = np.full((48, 64), 490, np.uint16)                                          # the same wall from 1 cm closer
    start = c["poses"][0][:3]
    pose, count, e, trace = R.track_frame(vol, nearer, C.DEPTH_SCALE, c["intr"][0], start, min_samples=16)
    assert pose is not None and count > 2000
    delta = pose[:, 3] - start[:, 3]                                                    # the camera looks along world +x
    assert abs(delta[0] - 0.01) < 1e-4                                                  # a hundredth of the motion
    assert delta[1] == 0.0 and delta[2] == 0.0
    assert np.abs(pose[:, :3] - start[:, :3]).max() < 1e-6
    assert trace[0][2] > 0 and e < trace[0][2] // 1000                                  # the residual went away


def test_a_jump_beyond_the_basin_shows():
    """A frame 12 cm + 4.2 degrees from the guess (trunc is 8 cm) does not converge.  The restatement does not lose it - the solve
    stays well-posed - but its residual says so: the rms of phi stays at 0.196 of trunc where a tracked frame ends at 0.034 (the
    depth quantisation and the one-view field).  The bounds: a tracked frame under 0.05, the jump over 0.15."""
    c = C.room_trajectory()
    vol = TR.integrate(c["depth_u16"][:1], C.DEPTH_SCALE, c["intr"][:1], c["poses"][:1], c["colors"][:1], **C.ROOM_RULE)
    rms = {}
    for step in (0.02, 0.12):
        far = C.trajectory(2, 120, 160, (30, 40), step=step, turn_deg=0.7 * step / 0.02)
        pose, count, e, _ = R.track_frame(vol, far["depth_u16"][1], C.DEPTH_SCALE, far["intr"][1], c["poses"][0][:3], **C.ROOM_RULE)
        assert pose is not None
        rms[step] = (e / count) ** 0.5 / 16384.0
        err = C.pose_error(far["poses"][1], pose)[0]
        assert (err < 0.002) == (step == 0.02), (step, err)
    print(rms)
    assert rms[0.02] < 0.05 and rms[0.12] > 0.15


def test_sums_do_not_depend_on_the_order_of_the_samples():
    c = K.noisy(17, 33, V=2, seed=3)
    vol = TR.integrate(c["depth_u16"][:1], C.DEPTH_SCALE, c["intr"][:1], c["poses"][:1], c["colors"][:1], min_weight=1)
    t, r = R.split_rule(min_weight=1)
    k = R.constants(t, r)
    d = FR.depth_metres(c["depth_u16"][1], C.DEPTH_SCALE)
    ok = FR.valid_pixels(d, r["near"], r["far"], r["edge_abs"], r["edge_rel"])
    Jq, rq = R.rows(vol, d, ok, c["intr"][1], c["poses"][0][:3], 1, k)
    assert len(rq) > 50
    want = R.sums(Jq, rq)
    for seed in range(3):
        o = np.random.default_rng(seed).permutation(len(rq))
        assert np.array_equal(R.sums(Jq[o], rq[o]), want)
    half = len(rq) // 2                                                                 # and any cut adds up
    assert np.array_equal(R.sums(Jq[:half], rq[:half]) + R.sums(Jq[half:], rq[half:]), want)


def test_a_lost_iteration_ends_the_frame():
    """count < min_samples loses the frame: the trace stops at the first iteration."""
    c = K.noisy(9, 63)
    vol = TR.integrate(c["depth_u16"], C.DEPTH_SCALE, c["intr"], c["poses"], c["colors"], min_weight=1)
    pose, count, e, trace = R.track_frame(vol, c["depth_u16"][0], C.DEPTH_SCALE, c["intr"][0], c["poses"][0][:3], min_samples=10 ** 6)
    assert pose is None and len(trace) == 1 and count == trace[0][1]


def test_matrices_invert_each_other():
    c = C.room_trajectory()
    c2w, w2c = R.matrices(c["poses"][2][:3])
    assert c2w.dtype == np.float32 and w2c.dtype == np.float32
    full = np.eye(4)
    full[:3] = w2c
    assert np.abs(full @ c["poses"][2] - np.eye(4)).max() < 1e-6
    nan = R.matrices(np.full((3, 4), np.nan))
    assert np.isnan(nan[0]).all() and np.isnan(nan[1]).all()
