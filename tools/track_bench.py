"""Times camera tracking against the TSDF volume (`segdino3d_amd/track.py`, csrc/track.hip) on a synthetic scene of real size, no files:
the closed-form room of tests/fuse_views_case.py scaled to a ScanNet-sized room, 480 x 640 uint16 depth and colour, rendered along the
trajectory of tests/track_case.py (2 cm and 0.7 degrees a frame).

    python tools/track_bench.py [--frames 12] [--reps 5] [--scale 1.5] [--iters 50] [--out profiles/track.json]

Reports: frames per second of track + fuse (a new `Tracker` over all frames, by HIP events, one host read at the end) and the pose
error against the rendered truth; the time of one iteration (accumulate + the one-lane solve) at strides 4, 2 and 1 and at a stride
larger than the image (one tile: what a launch pair costs with nothing to accumulate), each as `begin + iterate` minus `begin`; the
launches a frame makes; the touch + integrate time per frame, so that the reader sees what tracking adds to fusion; the bytes an
iteration must move; and, for context, the same alignment step written with torch tensor ops on the same device: a dense TSDF
tensor with its forward differences as channels, `grid_sample` for value, gradient and the observed mask, `J^T J` by matmul and
a float64 `linalg.solve` (no edge test, no fixed point: its time is what is compared, its result is not the rule's)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import fuse_views_case as K  # noqa: E402
import track_case as C  # noqa: E402


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=reps)


def dense_field(volume, lo, n):
    """The volume as a dense tensor [1, 5, Z, Y, X]: phi (units of trunc), its forward differences along x, y, z, and the observed mask."""
    keys, W, T, _ = volume.state()
    d = keys.device
    b = torch.stack([(keys >> 36) & 0x3FFFF, (keys >> 18) & 0x3FFFF, keys & 0x3FFFF], 1) - (1 << 17)
    loc = torch.arange(512, device=d)
    c = b[:, None, :] * 8 + torch.stack([loc >> 6, (loc >> 3) & 7, loc & 7], 1)[None] - torch.tensor(lo, device=d)
    inside = ((c >= 0) & (c < torch.tensor(n, device=d))).all(-1) & (W > 0)
    c, w, t = c[inside], W[inside], T[inside]
    phi = torch.zeros(n[2], n[1], n[0], device=d)
    mask = torch.zeros_like(phi)
    phi[c[:, 2], c[:, 1], c[:, 0]] = (t.double() / w.double()).float() / 4096.0
    mask[c[:, 2], c[:, 1], c[:, 0]] = 1.0
    gx, gy, gz = torch.zeros_like(phi), torch.zeros_like(phi), torch.zeros_like(phi)
    gx[:, :, :-1], gy[:, :-1, :], gz[:-1, :, :] = phi[:, :, 1:] - phi[:, :, :-1], phi[:, 1:, :] - phi[:, :-1, :], phi[1:, :, :] - phi[:-1, :, :]
    return torch.stack([phi, gx, gy, gz, mask])[None]


def torch_iteration(field, lo, n, depth_m, intr, pose, stride, voxel, near=0.1, far=6.0):
    """One alignment step with tensor ops: pose float64 [3, 4] on the device -> the new pose.  No host read."""
    d = depth_m[::stride, ::stride]
    H, W = d.shape
    v = torch.arange(H, device=d.device, dtype=torch.float32)[:, None] * stride
    u = torch.arange(W, device=d.device, dtype=torch.float32)[None, :] * stride
    p = torch.stack([(u - intr[2]) * d / intr[0], (v - intr[3]) * d / intr[1], d], -1).reshape(-1, 3)
    R, t = pose[:, :3].float(), pose[:, 3].float()
    y = p @ R.t()
    g = (y + t) / voxel - 0.5 - torch.tensor(lo, device=d.device, dtype=torch.float32)
    size = torch.tensor(n, device=d.device, dtype=torch.float32)
    s = torch.nn.functional.grid_sample(field, (2.0 * g / (size - 1.0) - 1.0).reshape(1, 1, 1, -1, 3), mode="bilinear", padding_mode="zeros",
                                        align_corners=True).reshape(5, -1)
    ok = ((d.reshape(-1) >= near) & (d.reshape(-1) <= far) & (s[4] > 0.999)).float()
    q = y / voxel
    nrm = s[1:4].t()
    J = torch.cat([torch.cross(q, nrm, dim=1), nrm], 1) * ok[:, None]
    A = (J.t() @ J).double()
    bb = (J.t() @ (s[0] * ok)).double()
    A = A + torch.diag(torch.diagonal(A) * 1e-6 + 1e-12)
    x = -torch.linalg.solve(A, bb)
    a = x[:3] / 2
    ax = torch.zeros(3, 3, dtype=torch.float64, device=d.device)
    ax[0, 1], ax[0, 2], ax[1, 0], ax[1, 2], ax[2, 0], ax[2, 1] = -a[2], a[1], a[2], -a[0], -a[1], a[0]
    aa = a @ a
    dR = ((1 - aa) * torch.eye(3, dtype=torch.float64, device=d.device) + 2 * torch.outer(a, a) + 2 * ax) / (1 + aa)
    return torch.cat([dR @ pose[:, :3], (pose[:, 3] + x[3:] * voxel)[:, None]], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--capacity", type=int, default=1 << 15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("track_bench: needs a HIP device (a measurement does not fall back to the CPU)")
    from segdino3d_amd import ops, track, tsdf
    d = torch.device("cuda:0")
    H, W, V = args.height, args.width, args.frames
    voxel, trunc = 0.02, 0.08
    t0 = time.perf_counter()
    c = C.trajectory(V, H, W, (H, W), scale=args.scale)
    print(f"{V} frames of {H} x {W} rendered on the host in {time.perf_counter() - t0:.1f} s", flush=True)
    depth, intr, colors = (torch.from_numpy(np.array(c[k])).to(d) for k in ("depth_u16", "intr", "colors"))
    kw = dict(voxel=voxel, trunc=trunc, capacity=args.capacity, first_pose=c["poses"][0])
    res = dict(depth=[H, W], frames=V, scale=args.scale, voxel=voxel, trunc=trunc, capacity=args.capacity, schedule=list(track.DEFAULT_SCHEDULE),
               device=torch.cuda.get_device_name(0))

    # ---- track + fuse, end to end
    def run():
        tr = track.Tracker(**kw)
        tr.add(depth, intr, colors, K.DEPTH_SCALE)
        return tr, tr.poses()

    tracker, (poses, lost) = run()
    res["lost"] = int(lost.sum())
    err = [C.pose_error(c["poses"][v], poses[v]) for v in range(V) if not lost[v]]
    res["pose_error_mm"] = dict(last=err[-1][0] * 1e3, max=max(e[0] for e in err) * 1e3)
    res["pose_error_deg"] = dict(last=err[-1][1], max=max(e[1] for e in err))
    res["count_stride1"] = int(tracker.info.count[-1])
    res["track_and_fuse"] = timed(run, args.reps)
    res["frames_per_s"] = (V - 1) / (res["track_and_fuse"]["median_ms"] * 1e-3)          # frame 0 is fused, not tracked
    iters = sum(n for _, n in track.DEFAULT_SCHEDULE)
    res["launches_per_frame"] = dict(begin=1, accumulate=iters, solve=iters, end=1, touch=1, integrate=1, memsets=1, kernels=2 * iters + 4)
    info = tracker.volume.mesh(return_info=True)[2]
    res["blocks"] = info.blocks

    # ---- what fusion alone costs: touch + integrate of the same frames with the tracked poses
    views_c2w = torch.from_numpy(np.ascontiguousarray(poses[:, :3].astype(np.float32))).to(d)
    views_w2c = torch.from_numpy(np.ascontiguousarray(np.linalg.inv(poses)[:, :3].astype(np.float32))).to(d)

    def fuse_only():
        vol = tsdf.TsdfVolume(voxel=voxel, trunc=trunc, capacity=args.capacity)
        for v in range(V):
            vol.add_posed(depth[v:v + 1], K.DEPTH_SCALE, intr[v:v + 1], views_c2w[v:v + 1], views_w2c[v:v + 1], colors[v:v + 1])

    if not lost.any():
        res["fuse_only"] = timed(fuse_only, args.reps)
        res["fuse_ms_per_frame"] = res["fuse_only"]["median_ms"] / V
        res["track_ms_per_frame"] = (res["track_and_fuse"]["median_ms"] - res["fuse_only"]["median_ms"]) / (V - 1)

    # ---- one iteration, per stride: the last frame against the fused volume, from its own (converged) pose
    vol, p = tracker.volume, tracker._p
    state = ops.track_state(d)
    start = torch.from_numpy(np.array(poses[-1][:3])).to(d)
    ops.track_pose_view(state).copy_(start)
    r = vol.rule
    n = args.iters

    def begin_only():
        for _ in range(n):
            ops.track_begin(state)

    def iterate(stride):
        def fn():
            for _ in range(n):
                ops.track_begin(state)
                ops.track_iterate(depth[-1], K.DEPTH_SCALE, intr[-1], state, vol._ws, vol.capacity, stride, vol.inv_voxel, vol.voxel, p.ymax,
                                  p.track_min_weight, p.min_samples, p.damping, p.max_rot, p.max_trans, r["near"], r["far"], r["edge_abs"],
                                  r["edge_rel"])
            ops.track_pose_view(state).copy_(start)
        return fn

    base = timed(begin_only, args.reps)
    res["begin_us"] = base["median_ms"] * 1e3 / n
    res["iteration_us"] = {}
    for stride in (4, 2, 1, 1024):
        m = timed(iterate(stride), args.reps)
        res["iteration_us"][str(stride)] = (m["median_ms"] - base["median_ms"]) * 1e3 / n
    samples = {s: -(-H // s) * -(-W // s) for s in (4, 2, 1)}
    # what an iteration must move: the depth pixel and its four neighbours (2 bytes each, shared between neighbours at stride 1), sixteen
    # 4-byte words of the volume per surviving sample (W and T of eight corners; neighbours share most of them), 29 64-bit atomics a tile
    res["bytes_per_iteration"] = {str(s): dict(depth=min(H * W, 5 * samples[s]) * 2, volume_gathered=samples[s] * 64,
                                               atomics=29 * (-(-(-(-H // s)) // 8) * -(-(-(-W // s)) // 32))) for s in (4, 2, 1)}
    res["volume_GBps_gathered"] = {str(s): samples[s] * 64 / (max(res["iteration_us"][str(s)] - res["iteration_us"]["1024"], 1e-3) * 1e-6) / 1e9
                                   for s in (4, 2, 1)}

    # ---- the same step in torch
    lo = [int(np.floor(float(x) * args.scale / voxel)) - 8 for x in K.ROOM_LO]
    hi = [int(np.ceil(float(x) * args.scale / voxel)) + 8 for x in K.ROOM_HI]
    dims = [hi[i] - lo[i] for i in range(3)]
    field = dense_field(vol, lo, dims)
    depth_m = depth[-1].view(torch.int16).float() * K.DEPTH_SCALE                       # below 32.768 m: the sign bit is clear
    guess = torch.from_numpy(np.array(poses[-2][:3])).to(d)
    pose_t = guess
    for stride, k in track.DEFAULT_SCHEDULE:
        for _ in range(k):
            pose_t = torch_iteration(field, lo, dims, depth_m, intr[-1], pose_t, stride, voxel)
    full = np.eye(4)
    full[:3] = pose_t.cpu().numpy()
    te = C.pose_error(c["poses"][-1], full)
    res["torch_pose_error_mm_deg"] = [te[0] * 1e3, te[1]]
    res["torch_iteration_us"] = {}
    for stride in (4, 2, 1):
        def fn(stride=stride):
            for _ in range(n):
                torch_iteration(field, lo, dims, depth_m, intr[-1], guess, stride, voxel)
        res["torch_iteration_us"][str(stride)] = timed(fn, max(2, args.reps // 2))["median_ms"] * 1e3 / n
    res["torch_dense_field_MB"] = field.numel() * 4 / 1e6
    res["torch_over_kernels"] = {s: res["torch_iteration_us"][s] / res["iteration_us"][s] for s in ("4", "2", "1")}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
