"""Argument checks of segdino3d_amd/track.py and of the track operators that run before anything reaches the device.  No GPU."""
import numpy as np
import pytest
import torch


def test_tracker_arguments():
    from segdino3d_amd import track
    for schedule in ((), ((0, 3),), ((4, 0),), ((2.5, 1),), ((1 << 15, 1),), ((1, 300),)):
        with pytest.raises(ValueError, match="schedule"):
            track.Tracker(schedule=schedule)
    for schedule in (3, ((1, 2, 3),), (("a", "b"),)):
        with pytest.raises(TypeError, match="schedule"):
            track.Tracker(schedule=schedule)
    for bad, name in ((dict(track_min_weight=0), "track_min_weight"), (dict(track_min_weight=1.5), "track_min_weight"),
                      (dict(min_samples=0), "min_samples"), (dict(min_samples=2.5), "min_samples"), (dict(damping=-1e-6), "damping"),
                      (dict(damping=float("nan")), "damping"), (dict(damping=2.0), "damping"), (dict(max_rot=0.0), "max_rot"),
                      (dict(max_rot=float("inf")), "max_rot"), (dict(max_trans=-1.0), "max_trans"), (dict(max_trans=float("nan")), "max_trans"),
                      (dict(far=float("inf")), "far")):
        with pytest.raises(ValueError, match=name):
            track.Tracker(**bad)
    for pose in (np.eye(3), np.full((4, 4), np.nan), np.zeros((2, 4, 4))):
        with pytest.raises(ValueError, match="first_pose"):
            track.Tracker(first_pose=pose)
    # the volume's own checks still hold
    with pytest.raises(ValueError, match="voxel"):
        track.Tracker(voxel=0.0)
    with pytest.raises(TypeError, match="unknown TSDF parameter"):
        track.Tracker(stride=2)
    t = track.Tracker(first_pose=torch.eye(4, dtype=torch.float64), min_weight=3)
    assert t.volume.rule["min_weight"] == 3 and t._p.schedule == track.DEFAULT_SCHEDULE and t._p.max_trans == 4 * 0.08
    assert t.n_frames == 0 and t.first_pose.shape == (3, 4)
    poses, lost = t.poses()
    assert poses.shape == (0, 4, 4) and lost.shape == (0,)


def test_the_width_of_the_sums_is_refused_not_overflowed():
    """(4096 far sqrt(3) / voxel + 2)^2 * samples must stay below 2^63: the defaults hold at 480 x 640 and at the largest image a
    coarser stride is needed."""
    from segdino3d_amd import track
    t = track.Tracker()
    t._p.check_width("Tracker.add", 480, 640)
    jq = 4096.0 * t._p.q * 1.001 + 2.0
    assert jq * jq * 480 * 640 < 2 ** 63 and 519 < t._p.q < 521
    with pytest.raises(ValueError, match="int64 sums"):
        t._p.check_width("Tracker.add", 16384, 16384)
    track.Tracker(schedule=((16, 2),))._p.check_width("Tracker.add", 16384, 16384)
    with pytest.raises(ValueError, match="int64 sums"):
        track.Tracker(voxel=2.0 ** -6, trunc=2.0 ** -4, far=1.0e6)._p.check_width("Tracker.add", 4, 4)


def test_cpu_tensors_and_wrong_inputs_are_refused():
    from segdino3d_amd import ops, track, tsdf
    t = track.Tracker()
    depth, intr = torch.zeros(2, 4, 6), torch.zeros(2, 4)
    colors = torch.zeros(2, 4, 6, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.add(depth, intr, colors)
    with pytest.raises(TypeError, match="expected a tensor"):
        t.add(np.zeros((2, 4, 6), np.float32), intr, colors)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        track.align(tsdf.TsdfVolume(), depth[0], intr[0], np.eye(4))
    with pytest.raises(TypeError, match="tsdf.TsdfVolume"):
        track.align(None, depth[0], intr[0], np.eye(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        track.track_and_fuse(depth, intr, colors)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.track_state("cpu")
    state = torch.zeros(1024, dtype=torch.uint8)
    assert ops.track_pose_view(state).shape == (3, 4) and ops.track_pose_view(state).dtype == torch.float64
    with pytest.raises(TypeError, match="track_state"):
        ops.track_pose_view(torch.zeros(12, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.track_begin(state)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.track_end(state)
    ws = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.track_iterate(depth[0], None, intr[0], state, ws, 16, 1, 50.0, 0.02, 10.4)
    for kw, err in ((dict(stride=0), ValueError), (dict(stride=1.5), ValueError), (dict(track_min_weight=0), ValueError),
                    (dict(min_samples=0), ValueError), (dict(damping=-1.0), ValueError), (dict(max_rot=0.0), ValueError),
                    (dict(far=0.05), ValueError), (dict(edge_abs=-1.0), ValueError), (dict(ymax=1.0e9), ValueError)):
        args = dict(stride=1, inv_voxel=50.0, voxel=0.02, ymax=10.4)
        args.update(kw)
        with pytest.raises(err):
            ops.track_iterate(depth[0], None, intr[0], state, ws, 16, **args)
    with pytest.raises(ValueError, match="one frame"):
        ops.track_iterate(depth, None, intr[0], state, ws, 16, 1, 50.0, 0.02, 10.4)
    with pytest.raises(ValueError, match="depth_scale"):
        ops.track_iterate(depth[0], 0.001, intr[0], state, ws, 16, 1, 50.0, 0.02, 10.4)
    vol = tsdf.TsdfVolume()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vol.add_posed(depth, None, intr, torch.zeros(2, 3, 4), torch.zeros(2, 3, 4), colors)
    with pytest.raises(TypeError, match="expected a tensor"):
        vol.add_posed(np.zeros((2, 4, 6), np.float32), None, intr, torch.zeros(2, 3, 4), torch.zeros(2, 3, 4), colors)
    assert vol.n_views == 0 and t.n_frames == 0
