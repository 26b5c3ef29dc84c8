"""Times the fusion of posed RGB-D frames into a point cloud (`segdino3d_amd/fuse_views.py`, csrc/fuse_views.hip) on a synthetic scene
of real size, no files: the closed-form room of tests/fuse_views_case.py scaled to a ScanNet-sized room, 480 x 640 uint16 depth and
480 x 640 colour, 64 distinct views (the 256-view run repeats them four times: the same cells, four times the observations), fed in
`add` calls of `--batch` views.

    python tools/fuse_bench.py [--views 256 64] [--batch 32] [--reps 5] [--scale 1.5] [--out profiles/fuse_views.json]

Reports, per view count: accumulate (all `add`s) and emit by HIP events around the queue of calls; pixels per second and the bytes
that must be read (2 + 3 per participating pixel) per second, against the time `torch.sum` takes to read the same two tensors; the
cells, the observations per cell and per (view, tile, cell) - the number of global update sets the on-chip combining leaves; and the
same fusion written with torch tensor ops on the same device (back-projection, `torch.unique(keys, return_inverse=True)`,
`index_add_`), whose cloud is compared with the kernels' before anything is timed."""
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
import fuse_views_ref as R  # noqa: E402

HBM_PEAK = 8.0e12
DISTINCT_VIEWS = 64


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


def torch_observations(views, colors, rule, voxel, first_view=0):
    """Steps 1-5 with tensor ops for one batch -> (key int64 [P], fixed int64 [P, 3], rgb int64 [P, 3], tile int64 [P]); `first_view`:
    the batch's first view in the scene, so that tiles of different batches get different numbers."""
    d = colors.device
    V, H, W = views.depth.shape
    z = views.depth.view(torch.int16).to(torch.int32).bitwise_and(0xFFFF).float() * views.depth_scale
    ok = (z > 0) & (z >= rule["near"]) & (z <= rule["far"])
    thr = rule["edge_abs"] + rule["edge_rel"] * z
    for dim, n in ((1, H), (2, W)):
        for lo in (0, 1):
            a, b = z.narrow(dim, lo, n - 1), z.narrow(dim, 1 - lo, n - 1)            # a pixel and its neighbour on one side
            ok.narrow(dim, lo, n - 1).logical_and_(~(~(b > 0) | ((b - a).abs() > thr.narrow(dim, lo, n - 1))))
    k, m = views.intrinsics, views.cam_to_world
    ui = torch.arange(W, device=d).float().view(1, 1, W)
    vi = torch.arange(H, device=d).float().view(1, H, 1)
    x = (ui - k[:, 2].view(V, 1, 1)) * z / k[:, 0].view(V, 1, 1)
    y = (vi - k[:, 3].view(V, 1, 1)) * z / k[:, 1].view(V, 1, 1)
    w = torch.stack([x, y, z], -1) @ m[:, :, :3].transpose(1, 2).unsqueeze(1) + m[:, :, 3].view(V, 1, 1, 3)
    ok &= (w.abs() < 2.0 ** 14).all(-1)
    c = torch.floor(w * (1.0 / voxel)).long() + (1 << 20)
    key = (c[..., 0] << 42) | (c[..., 1] << 21) | c[..., 2]
    tile = ((first_view + torch.arange(V, device=d)).view(V, 1, 1) * ((H + 7) // 8) + torch.arange(H, device=d).view(1, H, 1) // 8) * ((W + 31) // 32) + \
        torch.arange(W, device=d).view(1, 1, W) // 32
    fixed = torch.round(w.double() * 2.0 ** 20).long()
    Hc, Wc = colors.shape[1:3]
    if (Hc, Wc) != (H, W):
        colors = colors[:, ((2 * torch.arange(H, device=d) + 1) * Hc) // (2 * H)][:, :, ((2 * torch.arange(W, device=d) + 1) * Wc) // (2 * W)]
    return key[ok], fixed[ok], colors.long()[ok], tile.expand(V, H, W)[ok]


def torch_fusion(batches, rule, voxel, want_pairs=False):
    """The whole fusion with torch: the only formulation there was before csrc/fuse_views.hip."""
    parts, first = [], 0
    for v, c in batches:
        parts.append(torch_observations(v, c, rule, voxel, first))
        first += len(v)
    key, fixed, rgb, tile = (torch.cat([p[i] for p in parts]) for i in range(4))
    ukeys, inv = torch.unique(key, return_inverse=True)
    n = torch.zeros(len(ukeys), dtype=torch.int64, device=key.device).index_add_(0, inv, torch.ones_like(inv))
    S = torch.zeros(len(ukeys), 3, dtype=torch.int64, device=key.device).index_add_(0, inv, fixed)
    C = torch.zeros(len(ukeys), 3, dtype=torch.int64, device=key.device).index_add_(0, inv, rgb)
    keep = n >= rule["min_obs"]
    nd = n[keep].double().unsqueeze(1)
    points = torch.cat([(S[keep].double() / nd / 2.0 ** 20).float(), (C[keep].double() / nd).float()], 1)
    if not want_pairs:
        return points, n[keep]
    pairs = torch.unique(inv * (int(tile.max().item()) + 1) + tile).numel()
    return points, n[keep], int(key.numel()), int(ukeys.numel()), pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[256, 64])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--sweep", type=float, nargs="*", default=[0.02, 0.04, 0.08, 0.32, 1.28], help="voxel sizes of the sweep at the smaller view count")
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_views.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fuse_bench: needs a HIP device (a measurement does not fall back to the CPU)")
    from segdino3d_amd import fuse_views, lift2d, ops
    d = torch.device("cuda:0")
    H, W, B = args.height, args.width, args.batch
    rule, voxel = dict(fuse_views.RULE_DEFAULTS), 0.02
    t0 = time.perf_counter()
    n_distinct = min(DISTINCT_VIEWS, max(args.views))
    room = K.room(n_distinct, H, W, (H, W), scale=args.scale)
    print(f"{n_distinct} views of {H} x {W} rendered on the host in {time.perf_counter() - t0:.1f} s", flush=True)
    res = dict(depth=[H, W], colors=[H, W], views_per_add=B, scale=args.scale, voxel=voxel, rule=rule, device=torch.cuda.get_device_name(0),
               tile=[R.TILE_H, R.TILE_W])
    for V in args.views:
        batches = []
        for lo in range(0, V, B):
            idx = [(lo + i) % n_distinct for i in range(min(B, V - lo))]
            views = lift2d.Views(torch.from_numpy(room["depth_u16"][idx]).to(d), torch.from_numpy(room["intr"][idx]).to(d), room["poses"][idx],
                                 K.DEPTH_SCALE)
            batches.append((views, torch.from_numpy(room["colors"][idx]).to(d)))
        torch.cuda.synchronize()
        r = dict(views=V, pixels=V * H * W, bytes_needed=V * H * W * 5)
        fuser = fuse_views.PointCloudFuser(voxel=voxel)

        def accumulate():
            for v, c in batches:
                fuser.add(v, c)

        accumulate()
        points, obs, info = fuser.result(return_obs=True, return_info=True)
        r["info"] = info._asdict()
        # correctness at this size first: the torch formulation on the same views (its fp32 arithmetic is torch's own - a matrix
        # product, contracted or not - so a few observations land in a neighbouring cell; the clouds agree but for those)
        t_points, t_n, P, cells, pairs = torch_fusion(batches, rule, voxel, want_pairs=True)
        r["torch_vs_kernels"] = dict(points_kernels=int(points.shape[0]), points_torch=int(t_points.shape[0]), observations_torch=P,
                                     cells_torch=cells)
        if t_points.shape == points.shape:
            same = t_n == obs
            r["torch_vs_kernels"].update(cells_with_other_count=int((~same).sum().item()),
                                         max_abs_xyz_diff_same_count=float((t_points[same, :3] - points[same, :3]).abs().max().item()))
        r["observations_per_cell"] = P / max(cells, 1)
        r["observations_per_tile_cell_pair"] = P / max(pairs, 1)
        r["global_update_sets_per_pixel"] = pairs / r["pixels"]
        del t_points, t_n
        # the operator layer on the fuser's own workspace: a fuser counts its observations and refuses more than 2^28, a timing loop
        # over one table does not care (each run starts from an emptied table)
        ws, cap = fuser._ws, fuser.capacity

        def run():
            ops.fuse_reset(ws, cap)
            for v, c in batches:
                ops.fuse_accumulate(v.depth, v.depth_scale, v.intrinsics, v.cam_to_world, c, ws, cap, 1.0 / voxel, rule["stride"], rule["near"],
                                    rule["far"], rule["edge_abs"], rule["edge_rel"])

        r["reset"] = timed(lambda: ops.fuse_reset(ws, cap), args.reps)
        r["reset_and_accumulate"] = timed(run, args.reps)
        r["accumulate"] = {k: (x - r["reset"]["median_ms"] if k.endswith("_ms") else x) for k, x in r["reset_and_accumulate"].items()}
        r["emit"] = timed(lambda: fuser.result(), args.reps)
        again = fuser.result()
        assert torch.equal(again, points), "the timing runs changed the cloud"
        r["torch_sum_of_depth_and_colors"] = timed(lambda: [(v.depth.view(-1).view(torch.int64).sum(), c.view(-1).view(torch.int64).sum()) for v, c in batches],
                                                   args.reps)
        sec = r["accumulate"]["median_ms"] * 1e-3
        r["pixels_per_s"] = r["pixels"] / sec
        r["needed_TBps"] = r["bytes_needed"] / sec / 1e12
        r["needed_fraction_of_hbm_peak"] = r["bytes_needed"] / sec / HBM_PEAK
        r["torch_fusion"] = timed(lambda: torch_fusion(batches, rule, voxel), max(2, args.reps // 2))
        r["torch_over_kernels"] = r["torch_fusion"]["median_ms"] / (r["accumulate"]["median_ms"] + r["emit"]["median_ms"])
        if V == min(args.views):
            # what bounds accumulate: the same pixels into coarser and finer cells - the reads and the per-pixel arithmetic stay, the
            # distinct cells per tile (global update sets) and the pixels per cell (same-address LDS adds) move against each other
            r["voxel_sweep"] = []
            for vx in args.sweep:
                _, _, P2, cells2, pairs2 = torch_fusion(batches, rule, vx, want_pairs=True)
                voxel_now, voxel = voxel, vx
                t = timed(run, args.reps)
                voxel = voxel_now
                r["voxel_sweep"].append(dict(voxel=vx, cells=cells2, update_sets_per_pixel=pairs2 / r["pixels"],
                                             observations_per_tile_cell_pair=P2 / max(pairs2, 1),
                                             reset_and_accumulate_ms=t["median_ms"]))
            run()                                                                     # leave the table as the fuser's own again
        res[f"views_{V}"] = r
        print(json.dumps({f"views_{V}": r}), flush=True)
        del batches, fuser, points, obs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
