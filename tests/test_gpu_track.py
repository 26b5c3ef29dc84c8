"""csrc/track.hip + segdino3d_amd/track.py against the numpy restatement tests/track_ref.py (the reference has no counterpart) on the
room trajectory of tests/track_case.py and the hand-built scenes of tests/fuse_views_case.py and tests/tsdf_case.py.

Bounds.  None: the 29 integer sums of an iteration, every bit of every float64 pose, `lost`, `count`, `e` and the voxel state of the
volume the frames were fused into must EQUAL the restatement.  Steps 1 to 4 are single rounded fp32 operations and integer sums; the
solve and the update are single rounded float64 operations in a fixed order."""
import numpy as np
import pytest
import torch

import fuse_views_case as K
import track_case as C
import track_ref as R
import tsdf_case as TC
import tsdf_ref as TR

pytestmark = pytest.mark.gpu

SMALL = 1 << 12                      # blocks: 48 MB of state
ROOM = 1 << 13                       # the room at 2 cm


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _t(a, d):
    return torch.from_numpy(np.array(a)).to(d)                   # a copy: the shared cases are read-only


def _depth(c, kind):
    return (c["depth_u16"], c.get("scale", C.DEPTH_SCALE)) if kind == "u16" else (c["depth_f32"], None)


def _volume(c, d, kind, views, capacity=SMALL, **tsdf_rule):
    """The device volume of the first `views` views at their true poses, and the restatement's."""
    from segdino3d_amd import lift2d, tsdf
    depth, scale = _depth(c, kind)
    vol = tsdf.TsdfVolume(capacity=capacity, **tsdf_rule)
    vol.add(lift2d.Views(_t(depth[:views], d), _t(c["intr"][:views], d), c["poses"][:views], scale), _t(c["colors"][:views], d))
    return vol, TR.integrate(depth[:views], scale, c["intr"][:views], c["poses"][:views], c["colors"][:views], **tsdf_rule)


def _iteration(vol, want_vol, depth, scale, intr, pose, stride, d, **kw):
    """One iteration at `stride` from `pose` float64 [3, 4] on the device and in the restatement; asserts the 29 sums, lost and the
    pose after the update.  -> (sums int64 [29], the restatement's new pose or None)."""
    from segdino3d_amd import ops, track
    tsdf_rule = {"voxel": vol.voxel, "trunc": vol.trunc, **vol.rule}
    t, r = R.split_rule(schedule=((stride, 1),), **kw, **tsdf_rule)
    k = R.constants(t, r)
    dd = R.FR.depth_metres(depth, scale)
    ok = R.FR.valid_pixels(dd, r["near"], r["far"], r["edge_abs"], r["edge_rel"])
    want = R.sums(*R.rows(want_vol, dd, ok, intr, pose, stride, k, t["track_min_weight"]))
    x = R.solve(want, k, t["min_samples"])
    want_pose = None if x is None else R.update(pose, x, k)

    p = track._Params("test", vol.voxel, vol.trunc, vol.rule["far"], ((stride, 1),), t["track_min_weight"], t["min_samples"], t["damping"],
                      t["max_rot"], t["max_trans"])
    state = ops.track_state(d)
    ops.track_pose_view(state).copy_(torch.from_numpy(np.array(pose, np.float64)))
    track._run_frame(p, vol, state, _t(depth, d), scale, _t(intr, d))
    got = ops.track_sums_view(state).cpu().numpy()
    got_pose, c2w, w2c, info = (a.cpu().numpy() for a in ops.track_end(state))
    what = (depth.shape, depth.dtype, stride, kw)
    assert np.array_equal(got, want), (what, got, want)
    assert info[0] == (want_pose is None) and info[1] == want[27] and info[2] == want[28], (what, info)
    after = ops.track_pose_view(state).cpu().numpy()
    if want_pose is None:
        assert np.isnan(got_pose).all() and np.isnan(c2w).all() and np.isnan(w2c).all(), what
        assert np.array_equal(after.view(np.uint64), np.array(pose, np.float64).view(np.uint64)), what      # the state went back
    else:
        assert np.array_equal(got_pose.view(np.uint64), want_pose.view(np.uint64)), (what, got_pose - want_pose)
        assert np.array_equal(after.view(np.uint64), want_pose.view(np.uint64)), what
        m = R.matrices(want_pose)
        assert np.array_equal(c2w.view(np.uint32), m[0].view(np.uint32)) and np.array_equal(w2c.view(np.uint32), m[1].view(np.uint32)), what
    return want, want_pose


def _moved(pose, shift=(0.004, -0.003, 0.002)):
    p = np.array(pose[:3], np.float64)
    p[:, 3] += shift
    return p


# ---------------------------------------------------------------------------------------------- one iteration's sums
@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("hw", [(5, 7), (9, 63), (9, 64), (9, 65), (17, 33)])
def test_one_iteration_on_small_and_odd_images(hw, kind):
    """The sums, the solve and the update at every stride, against a volume fused from one and from three views."""
    d = dev()
    c = K.noisy(hw[0], hw[1], V=3, seed=hw[1])
    depth, scale = _depth(c, kind)
    seen = 0
    for views in (1, 3):
        vol, want_vol = _volume(c, d, kind, views, min_weight=1)
        for stride in (1, 2, 4, 64):                                                   # 64: larger than the image, one sample at most
            want, _ = _iteration(vol, want_vol, depth[views - 1], scale, c["intr"][views - 1], _moved(c["poses"][views - 1]), stride, d,
                                 min_samples=4)
            seen += int(want[27])
            assert want[27] <= -(-hw[0] // stride) * -(-hw[1] // stride)
    assert seen > hw[0] * hw[1] // 4                                                   # the cases do hold samples


def test_block_faces_at_a_negative_coordinate():
    """The wall on the face between blocks -5 and -4, the image centred on y = z = 0: the eight corners of a sample straddle 2, 4 and 8
    blocks.  On the voxel centres phi == 0 exactly: e == 0, b == 0, and the pose does not move."""
    d = dev()
    c = TC.block_face_wall()
    vol, want_vol = _volume(c, d, "f32", 1, **TC.BLOCK_FACE_RULE)
    for stride in (1, 2):
        want, pose = _iteration(vol, want_vol, c["depth_f32"][0], None, c["intr"][0], _moved(c["poses"][0], (0.003, 0.0, 0.0)), stride, d,
                                min_samples=8)
        assert want[27] > 40 and want[28] > 0 and pose is not None
    t, r = R.split_rule(**TC.BLOCK_FACE_RULE)
    k = R.constants(t, r)
    vi, ui = np.nonzero(np.ones((16, 40), bool))                                       # the (y, z) cells of the samples, as step 3 makes them
    fx, fy, cx, cy = (np.float32(x) for x in c["intr"][0])
    py = (vi.astype(np.float32) - cy) * np.float32(0.5) / fy                          # camera y is world -z, camera x world -y
    px = (ui.astype(np.float32) - cx) * np.float32(0.5) / fx
    cells = np.floor(np.stack([-px, -py], 1) * k["inv_voxel"] - np.float32(0.5)).astype(np.int64)
    assert ((cells & 7) == 7).all(axis=1).any() and ((cells & 7) == 7).any(axis=1).sum() > 10      # 8 blocks, and 4
    c = TC.block_face_wall(on_centres=True)
    vol, want_vol = _volume(c, d, "f32", 1, **TC.BLOCK_FACE_RULE)
    want, pose = _iteration(vol, want_vol, c["depth_f32"][0], None, c["intr"][0], c["poses"][0][:3], 1, d, min_samples=8)
    assert want[27] > 40 and want[28] == 0 and not want[21:27].any()
    assert np.array_equal(pose[:, 3], c["poses"][0][:3, 3])


def test_unobserved_corners_and_the_min_samples_boundary():
    d = dev()
    c = K.noisy(9, 65, V=1, seed=5)
    depth, scale = _depth(c, "u16")
    vol, want_vol = _volume(c, d, "u16", 1, min_weight=1)
    start = _moved(c["poses"][0])
    # after one view nothing has W >= 2: every sample is dropped, the frame is lost, its pose is NaN and the state is unchanged
    want, pose = _iteration(vol, want_vol, depth[0], scale, c["intr"][0], start, 1, d, track_min_weight=2, min_samples=1)
    assert want[27] == 0 and pose is None and not want.any()
    # with W >= 1 the samples next to a hole of the volume drop out, the others stay
    want, pose = _iteration(vol, want_vol, depth[0], scale, c["intr"][0], start, 1, d, min_samples=1)
    n = int(want[27])
    valid = R.FR.valid_pixels(R.FR.depth_metres(depth[0], scale), 0.1, 6.0, 0.02, 0.02).sum()
    assert 20 < n < valid and pose is not None
    _, pose = _iteration(vol, want_vol, depth[0], scale, c["intr"][0], start, 1, d, min_samples=n)
    assert pose is not None
    _, pose = _iteration(vol, want_vol, depth[0], scale, c["intr"][0], start, 1, d, min_samples=n + 1)
    assert pose is None


# ---------------------------------------------------------------------------------------------- whole frames
def _tracker(c, d, **kw):
    from segdino3d_amd import track
    return track.Tracker(capacity=ROOM, first_pose=c["poses"][0], **C.ROOM_RULE, **kw)


def _equal_state(vol, want, what):
    keys, W, T, Cs = (x.cpu().numpy() for x in vol.state())
    assert np.array_equal(keys.view(np.uint64), want.keys), what
    assert np.array_equal(W, want.W) and np.array_equal(T, want.T) and np.array_equal(Cs, want.C), what


def _equal_track(tracker, want, n, what):
    poses, lost = tracker.poses()
    assert poses.dtype == np.float64 and poses.shape == (n, 4, 4) and lost.dtype == bool, what
    assert np.array_equal(lost, want["lost"][:n]), (what, lost)
    assert np.array_equal(poses.view(np.uint64)[~lost], want["poses"][:n].view(np.uint64)[~lost]), (what, poses - want["poses"][:n])
    assert np.isnan(poses[lost]).all(), what
    assert np.array_equal(tracker.info.count, want["count"][:n]) and np.array_equal(tracker.info.e, want["e"][:n]), (what, tracker.info)
    return poses, lost


def test_room_trajectory():
    """Every pose bit, lost, count and e, and the volume the frames were fused into."""
    d = dev()
    c, want = C.room_trajectory(), C.room_trajectory_ref()
    tracker = _tracker(c, d)
    tracker.add(_t(c["depth_u16"], d), _t(c["intr"], d), _t(c["colors"], d), C.DEPTH_SCALE)
    poses, lost = _equal_track(tracker, want, 5, "room")
    assert not lost.any() and C.pose_error(poses[4], c["poses"][4])[0] < 0.003
    _equal_state(tracker.volume, want["volume"], "room")
    assert tracker.volume.n_views == 5 and tracker.n_frames == 5


def test_cut_and_stream():
    """Frames added one at a time, all at once and on a side stream give the same bits."""
    d = dev()
    c, want = C.room_trajectory(), C.room_trajectory_ref()
    n = 3
    depth, intr, colors = _t(c["depth_u16"][:n], d), _t(c["intr"][:n], d), _t(c["colors"][:n], d)
    one = _tracker(c, d)
    for v in range(n):
        one.add(depth[v:v + 1], intr[v:v + 1], colors[v:v + 1], C.DEPTH_SCALE)
    _equal_track(one, want, n, "one at a time")
    whole = _tracker(c, d)
    whole.add(depth, intr, colors, C.DEPTH_SCALE)
    _equal_track(whole, want, n, "at once")
    side = torch.cuda.Stream(device=d)
    side.wait_stream(torch.cuda.current_stream(d))
    with torch.cuda.stream(side):
        other = _tracker(c, d)
        other.add(depth[:2], intr[:2], colors[:2], C.DEPTH_SCALE)
        other.add(depth[2:], intr[2:], colors[2:], C.DEPTH_SCALE)
        _equal_track(other, want, n, "side stream")
        state = [x.cpu().numpy() for x in other.volume.state()]
    torch.cuda.current_stream(d).wait_stream(side)
    for a, b in ((one, whole),):
        for x, y in zip(a.volume.state(), b.volume.state()):
            assert torch.equal(x, y)
    for x, y in zip(one.volume.state(), state):
        assert np.array_equal(x.cpu().numpy(), y)


def test_a_lost_frame_in_the_middle():
    """An all-zero depth frame is lost, leaves the voxel state untouched, and the next frame tracks from the last good pose."""
    d = dev()
    c = C.room_trajectory()
    order = [0, 1, 1, 2]
    depth = np.array(c["depth_u16"][order])
    depth[2] = 0
    intr, colors = c["intr"][order], c["colors"][order]
    want = R.track(depth, C.DEPTH_SCALE, intr, colors, first_pose=c["poses"][0], **C.ROOM_RULE)
    assert list(want["lost"]) == [False, False, True, False] and want["count"][2] == 0
    tracker = _tracker(c, d)
    tracker.add(_t(depth[:2], d), _t(intr[:2], d), _t(colors[:2], d), C.DEPTH_SCALE)
    before = [x.clone() for x in tracker.volume.state()]
    tracker.add(_t(depth[2:3], d), _t(intr[2:3], d), _t(colors[2:3], d), C.DEPTH_SCALE)
    for x, y in zip(before, tracker.volume.state()):
        assert torch.equal(x, y)
    tracker.add(_t(depth[3:], d), _t(intr[3:], d), _t(colors[3:], d), C.DEPTH_SCALE)
    poses, lost = _equal_track(tracker, want, 4, "lost frame")
    assert C.pose_error(poses[3], c["poses"][2])[0] < 0.004                            # 4 cm from the last good pose, and found
    _equal_state(tracker.volume, want["volume"], "lost frame")


def test_align_leaves_the_volume_alone():
    from segdino3d_amd import track
    d = dev()
    c = C.room_trajectory()
    vol, want_vol = _volume(c, d, "u16", 1, capacity=ROOM, **C.ROOM_RULE)
    before = [x.clone() for x in vol.state()]
    guess = c["poses"][0]
    pose, info = track.align(vol, _t(c["depth_u16"][1], d), _t(c["intr"][1], d), guess, C.DEPTH_SCALE, return_info=True)
    want, count, e, _ = R.track_frame(want_vol, c["depth_u16"][1], C.DEPTH_SCALE, c["intr"][1], guess[:3], **C.ROOM_RULE)
    assert pose.is_cuda and pose.dtype == torch.float64 and tuple(pose.shape) == (4, 4)
    got = pose.cpu().numpy()
    assert np.array_equal(got[:3].view(np.uint64), want.view(np.uint64)) and list(got[3]) == [0.0, 0.0, 0.0, 1.0]
    assert info.tolist() == [0, count, e]
    for x, y in zip(before, vol.state()):
        assert torch.equal(x, y)
    assert vol.n_views == 1
    lost = track.align(vol, torch.zeros(120, 160, dtype=torch.uint16).to(d), _t(c["intr"][1], d), guess, C.DEPTH_SCALE)
    assert torch.isnan(lost).all()


def test_tracked_poses_feed_the_rest_of_the_chain():
    from segdino3d_amd import lift2d, superpoints, track
    d = dev()
    c = C.room_trajectory()
    depth = np.array(c["depth_u16"])
    depth[3] = 0                                                                       # a lost frame: Views drops its NaN pose
    depth = _t(depth, d)
    poses, lost, volume = track.track_and_fuse(depth, _t(c["intr"], d), _t(c["colors"], d), C.DEPTH_SCALE, capacity=ROOM,
                                               first_pose=c["poses"][0], min_weight=1, **C.ROOM_RULE)
    assert list(lost) == [False, False, False, True, False]
    views = lift2d.Views(depth, _t(c["intr"], d), poses, C.DEPTH_SCALE)
    assert len(views) == 4 and list(views.kept) == [0, 1, 2, 4]
    vertices, faces, info = volume.mesh(return_info=True)
    assert info.vertices > 1000 and info.faces > 1000 and info.overflow == 0
    bits, count = lift2d.visibility(vertices[:, :3].contiguous(), views)
    assert (count > 0).float().mean().item() > 0.5                                     # the mesh is where the tracked views see it
    labels, sp = superpoints.mesh_superpoints(vertices[:, :3].contiguous(), faces, return_info=True)
    assert tuple(labels.shape) == (info.vertices,) and 1 <= sp.count < info.vertices


def test_device_argument_errors():
    from segdino3d_amd import ops, track, tsdf
    d = dev()
    depth, intr = torch.zeros(2, 4, 6, device=d), torch.ones(2, 4, device=d)
    colors = torch.zeros(2, 4, 6, 3, dtype=torch.uint8, device=d)
    t = track.Tracker(capacity=16)
    for args, err, match in (((depth[0], intr, colors), ValueError, r"\[V, Hd, Wd\]"), ((depth, intr[0], colors), ValueError, "intrinsics"),
                             ((depth, intr, colors[:1]), ValueError, "colors"), ((depth, intr, colors.float()), TypeError, "uint8"),
                             ((depth.double(), intr, colors), TypeError, "uint16 or fp32"), ((depth, intr.double(), colors), TypeError, "fp32"),
                             ((depth, intr, colors.cpu()), RuntimeError, "no CPU fallback")):
        with pytest.raises(err, match=match):
            t.add(*args)
    with pytest.raises(ValueError, match="depth_scale"):
        t.add(depth, intr, colors, 0.001)
    with pytest.raises(ValueError, match="depth_scale"):
        t.add(torch.zeros(2, 4, 6, dtype=torch.uint16).to(d), intr, colors)
    assert t.n_frames == 0
    with pytest.raises(RuntimeError, match="empty"):
        track.align(tsdf.TsdfVolume(capacity=16), depth[0], intr[0], np.eye(4))
    vol = tsdf.TsdfVolume(capacity=16)
    vol.add_posed(depth, None, intr, torch.zeros(2, 3, 4, device=d), torch.zeros(2, 3, 4, device=d), colors)
    with pytest.raises(ValueError, match="one frame"):
        track.align(vol, depth, intr[0], np.eye(4))
    with pytest.raises(ValueError, match="pose"):
        track.align(vol, depth[0], intr[0], np.eye(3))
    with pytest.raises(ValueError, match="colors"):
        vol.add_posed(depth, None, intr, torch.zeros(2, 3, 4, device=d), torch.zeros(2, 3, 4, device=d), colors[:1])
    # what only the C entry points see
    state = ops.track_state(d)
    with pytest.raises(RuntimeError, match="state"):
        ops.track_begin(state[:64])
    with pytest.raises(RuntimeError, match="workspace too small"):
        ops.track_iterate(depth[0], None, intr[0], state, vol._ws[:4096], 16, 1, 50.0, 0.02, 10.4)
    with pytest.raises(RuntimeError, match="workspace too small"):
        ops.track_iterate(depth[0], None, intr[0], state, vol._ws, 32, 1, 50.0, 0.02, 10.4)
    with pytest.raises(ValueError, match="capacity"):
        ops.track_iterate(depth[0], None, intr[0], state, vol._ws, 24, 1, 50.0, 0.02, 10.4)
    with pytest.raises(RuntimeError, match="int64 sums"):                               # past the Python check, the entry point's own
        ops._lib.check(ops._lib.load().sd3d_track_iterate(depth.data_ptr(), 0, 1.0, intr.data_ptr(), 4, 6, 1, 0.1, 6.0, 0.02, 0.02, 1, 50.0, 0.02,
                                                          1.0e9, 1, 1, 0.0, 0.5, 0.32, state.data_ptr(), state.numel(), vol._ws.data_ptr(),
                                                          vol._ws.numel(), 16, None), "track_iterate")
    with pytest.raises(TypeError, match="int64"):
        ops.track_end(state, info=torch.zeros(3, dtype=torch.int32, device=d))
    with pytest.raises(ValueError, match="pose"):
        ops.track_end(state, pose=torch.zeros(4, 4, dtype=torch.float64, device=d))
