"""Times the multi-view lifting of 2D feature maps onto scene points (`segdino3d_amd/lift2d.py`, csrc/lift2d.hip) on a synthetic scene
of real size, no files: the analytic room of tests/lift2d_case.py scaled up - 150 k surface points, 480 x 640 uint16 depth ray-cast per
view, 60 x 80 x 256 fp16 feature maps (further scales at 30 x 40 and 15 x 20).

    python tools/lift_bench.py [--points 150000] [--views 256] [--reps 5] [--host-views 2] [--out profiles/lift_2d.json]

Reports, per number of scales (1 and 3): HIP-event times of visibility, accumulate (all passes) and finish; the bytes the accumulate
kernel gathers (visible pairs x 4 taps x C x element size per scale) and reads / writes of its running sum, and the rates they imply;
a sweep of `views_per_pass`; and two baselines on the same inputs - the numpy restatement (tests/lift2d_ref.py) on the host over
`--host-views` views, scaled to all views, and the plain torch formulation on the device (per view: project, depth test,
`grid_sample`, masked add).  The torch baseline's output is compared with the kernels' before anything is timed."""
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

import lift2d_case as K  # noqa: E402
import lift2d_ref as R  # noqa: E402

SCALE_SIZES = [(60, 80), (30, 40), (15, 20)]


def make_scene(n_points, n_views, H, W, seed=0, coherent=True):
    rng = np.random.default_rng(seed)
    poses, intr, depth = K.make_views(rng, n_views, H, W)
    depth_u16 = np.round(depth / K.DEPTH_SCALE).astype(np.uint16)
    pts = K.room_points(rng, n_points).astype(np.float32)
    if coherent:                                  # a scan's vertex order is spatially coherent: order by 0.25 m cell
        cell = np.floor(pts / 0.25).astype(np.int64)
        pts = pts[np.lexsort((cell[:, 0], cell[:, 1], cell[:, 2]))]
    return pts, poses, intr, depth_u16


def timed(fn, reps, warmup=2):
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


def torch_baseline(points, views, maps_list, near=0.05, tol_abs=0.05):
    """What a user would write with torch on the device: one view at a time, every scale sampled with `grid_sample`."""
    N = points.shape[0]
    Hd, Wd = views.height, views.width
    count = torch.zeros(N, device=points.device)
    sums = [torch.zeros(N, m.shape[-1], device=points.device) for m in maps_list]
    p = points[:, :3]
    for j in range(len(views)):
        m = views.world_to_cam[j]
        cam = p @ m[:, :3].T + m[:, 3]
        z = cam[:, 2]
        k = views.intrinsics[j]
        u, v = k[0] * cam[:, 0] / z + k[2], k[1] * cam[:, 1] / z + k[3]
        ui, vi = torch.floor(u + 0.5), torch.floor(v + 0.5)
        inside = (z > near) & (ui >= 0) & (ui < Wd) & (vi >= 0) & (vi < Hd)
        lin = torch.where(inside, vi * Wd + ui, torch.zeros_like(ui)).long()
        d = views.depth[j].view(torch.int16).reshape(-1)[lin].to(torch.int32).bitwise_and(0xFFFF).float() * views.depth_scale
        vis = inside & (d > 0) & ((d - z).abs() <= tol_abs)
        grid = torch.stack([(2 * u + 1) / Wd - 1, (2 * v + 1) / Hd - 1], -1).reshape(1, 1, N, 2)
        grid = torch.where(vis.reshape(1, 1, N, 1), grid, torch.zeros_like(grid))
        for s, fm in zip(sums, maps_list):
            samp = torch.nn.functional.grid_sample(fm[j].permute(2, 0, 1)[None].float(), grid, mode="bilinear", padding_mode="border",
                                                   align_corners=False)[0, :, 0].T
            s += torch.where(vis[:, None], samp, torch.zeros_like(samp))
        count += vis
    means = [torch.where(count[:, None] > 0, s / count[:, None].clamp(min=1), torch.zeros_like(s)) for s in sums]
    out = means[0]
    for mm in means[1:]:
        out = out + mm
    return out / len(means), count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-views", type=int, default=2)
    ap.add_argument("--sweep", default="8,16,32,64,128")
    ap.add_argument("--random-order", action="store_true", help="points in random order instead of a spatially coherent one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lift_2d.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lift_bench: needs a HIP device (a measurement does not fall back to the CPU)")
    from segdino3d_amd import lift2d, ops
    d = torch.device("cuda:0")
    H, W, C, V, N = 480, 640, args.channels, args.views, args.points
    t0 = time.perf_counter()
    pts, poses, intr, depth_u16 = make_scene(N, V, H, W, coherent=not args.random_order)
    print(f"scene built on the host in {time.perf_counter() - t0:.1f} s", flush=True)
    pts_d = torch.from_numpy(pts).to(d)
    views = lift2d.Views(torch.from_numpy(depth_u16).to(d), torch.from_numpy(intr).to(d), poses, K.DEPTH_SCALE)
    gen = torch.Generator(device=d).manual_seed(0)
    maps_all = [torch.randn(V, hf, wf, C, device=d, generator=gen).half() for hf, wf in SCALE_SIZES]
    hw = (H, W)
    res = dict(points=N, views=V, channels=C, depth=[H, W], map_sizes=SCALE_SIZES, order="random" if args.random_order else "coherent",
               device=torch.cuda.get_device_name(0))

    bits, count = lift2d.visibility(pts_d, views)
    pairs = int(count.sum().item())
    res["visible_pairs"] = pairs
    res["visible_pairs_per_point"] = pairs / N
    res["points_seen"] = int((count > 0).sum().item())
    res["visibility"] = timed(lambda: ops.lift_visibility(pts_d, views.world_to_cam, views.intrinsics, views.depth, views.depth_scale), args.reps)

    # correctness at this size first: the torch formulation on the same inputs
    got = lift2d.lift_point_features(pts_d, views, maps_all[:1])
    want, tcount = torch_baseline(pts_d, views, maps_all[:1])
    # the scene has no margin around its decisions: where torch's differently rounded projection decides a pair the other way the
    # two means are means over different views; every other point must agree to fp32 rounding
    same = tcount.int() == count
    res["torch_vs_kernels"] = dict(points_with_other_count=int((~same).sum().item()),
                                   max_abs_diff_same_count=float((got - want)[same].abs().max().item()),
                                   max_abs_diff_other_count=float((got - want)[~same].abs().max().item()) if bool((~same).any()) else 0.0)
    print(json.dumps(res), flush=True)

    for n_scales in (1, 3):
        maps = maps_all[:n_scales]
        default = lift2d.default_views_per_pass(V)
        sums = [torch.zeros(N, C, device=d) for _ in maps]

        def accumulate(step):
            for v0 in range(0, V, step):
                for s, m in zip(sums, maps):
                    ops.lift_accumulate(pts_d, views.world_to_cam, views.intrinsics, hw, bits, m, s, v0, min(V, v0 + step))

        def finish():
            acc = torch.empty_like(sums[0]) if n_scales > 1 else None
            for i, s in enumerate(sums):
                ops.lift_finish(s, count, i, n_scales, acc=acc, out_dtype=torch.float16)

        sweep = {}
        for step in sorted({int(x) for x in args.sweep.split(",")} | {default, V}):
            if step <= V:
                sweep[step] = timed(lambda: accumulate(step), args.reps)
        r = dict(default_views_per_pass=default, accumulate_sweep=sweep, finish=timed(finish, args.reps))
        best = min(sweep, key=lambda k: sweep[k]["median_ms"])
        gathered = pairs * 4 * C * 2 * n_scales
        r["gathered_bytes"] = gathered
        r["best_views_per_pass"] = best
        t_def = sweep[min(default, V)]["median_ms"] * 1e-3
        r["accumulate_ms_at_default"] = t_def * 1e3
        r["gather_rate_TBps_at_default"] = gathered / t_def / 1e12
        r["gather_rate_TBps_at_best"] = gathered / (sweep[best]["median_ms"] * 1e-3) / 1e12
        r["maps_bytes"] = sum(m.numel() * 2 for m in maps)
        r["one_shot"] = timed(lambda: lift2d.lift_point_features(pts_d, views, maps, out_dtype=torch.float16), args.reps)
        r["torch_baseline"] = timed(lambda: torch_baseline(pts_d, views, maps), max(2, args.reps // 2), warmup=1)
        r["torch_over_kernels"] = r["torch_baseline"]["median_ms"] / r["one_shot"]["median_ms"]
        hv = min(args.host_views, V)
        host_maps = [m[:hv].cpu().numpy() for m in maps]
        t = time.perf_counter()
        R.lift_point_features(pts, poses[:hv], intr[:hv], depth_u16[:hv], host_maps, K.DEPTH_SCALE)
        per_view = (time.perf_counter() - t) / hv
        r["numpy_restatement"] = dict(views_timed=hv, s_per_view=per_view, s_all_views_extrapolated=per_view * V)
        r["numpy_over_kernels"] = per_view * V * 1e3 / r["one_shot"]["median_ms"]
        res[f"scales_{n_scales}"] = r
        print(json.dumps({f"scales_{n_scales}": r}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
