"""Times the nearest-point stage (`segdino3d_amd/transfer.py`, csrc/transfer.hip) on a synthetic scene of real size, no files: the
closed-form room of tests/fuse_views_case.py scaled to a ScanNet-sized room, 480 x 640 uint16 depth, 64 distinct views (the 256-view
run repeats them four times), fused by `fuse_views` into the cloud that is then searched.

    python tools/transfer_bench.py [--views 256] [--reps 7] [--radius 0.04] [--out profiles/transfer.json]

Reports (HIP events around the queue of calls; warm-up, then `--reps` runs: median, min, max):
  index build          at 150 k points and at the whole fused cloud;
  point form           M = N = 150 k (the cloud's own points, moved by a few millimetres) against `torch.cdist` in chunks + `min` on the
                       same device, whose indices are compared with the kernels' before anything is timed;
  pixel form           all views in one launch with L = 0 (index only), 1 and 5 label channels: ms per scene, queries per second, the
                       bytes that must be read and written (2 per depth pixel, 4 per output value) against the HBM peak; and, as the
                       measure of what the tile's shared table saves, the same queries of the distinct views through the point form,
                       which looks every bucket up per query;
  instance map         I = 100 and 600 masks over 150 k points against `(masks * scores[:, None]).argmax(0)` in torch."""
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

HBM_PEAK = 8.0e12
DISTINCT_VIEWS = 64


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


def cdist_nearest(src, queries, radius, chunk=8192):
    """The formulation there was before: distances of a chunk of queries to every source point, `min`, the radius test."""
    idx = torch.empty(queries.shape[0], dtype=torch.int64, device=queries.device)
    for lo in range(0, queries.shape[0], chunk):
        dist, j = torch.cdist(queries[lo:lo + chunk], src).min(dim=1)
        idx[lo:lo + chunk] = torch.where(dist <= radius, j, torch.full_like(j, -1))
    return idx


def back_project(views):
    """Every pixel of the views as a query, with tensor ops (NaN where the depth is 0) -> fp32 [V H W, 3]."""
    V, H, W = views.depth.shape
    d = views.depth.device
    z = views.depth.view(torch.int16).to(torch.int32).bitwise_and(0xFFFF).float() * views.depth_scale
    z = torch.where(z > 0, z, torch.full_like(z, float("nan")))
    k, m = views.intrinsics, views.cam_to_world
    x = (torch.arange(W, device=d).float().view(1, 1, W) - k[:, 2].view(V, 1, 1)) * z / k[:, 0].view(V, 1, 1)
    y = (torch.arange(H, device=d).float().view(1, H, 1) - k[:, 3].view(V, 1, 1)) * z / k[:, 1].view(V, 1, 1)
    w = torch.stack([x, y, z], -1) @ m[:, :, :3].transpose(1, 2).unsqueeze(1) + m[:, :, 3].view(V, 1, 1, 3)
    return w.reshape(-1, 3).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--radius", type=float, default=0.04)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transfer.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transfer_bench: needs a HIP device (a measurement does not fall back to the CPU)")
    from segdino3d_amd import fuse_views, lift2d, ops, transfer
    d = torch.device("cuda:0")
    H, W, V, r = args.height, args.width, args.views, args.radius
    t0 = time.perf_counter()
    n_distinct = min(DISTINCT_VIEWS, V)
    room = K.room(n_distinct, H, W, (H, W), scale=args.scale)
    print(f"{n_distinct} views of {H} x {W} rendered on the host in {time.perf_counter() - t0:.1f} s", flush=True)
    sel = [i % n_distinct for i in range(V)]
    distinct = lift2d.Views(torch.from_numpy(room["depth_u16"]).to(d), torch.from_numpy(room["intr"]).to(d), room["poses"], K.DEPTH_SCALE)
    views = lift2d.Views(torch.from_numpy(room["depth_u16"][sel]).to(d), torch.from_numpy(room["intr"][sel]).to(d), room["poses"][sel],
                         K.DEPTH_SCALE)
    cloud = fuse_views.fuse_views(distinct, torch.from_numpy(room["colors"]).to(d), voxel=0.02, min_obs=1)
    N = cloud.shape[0]
    res = dict(device=torch.cuda.get_device_name(0), depth=[H, W], views=V, distinct_views=n_distinct, radius=r, cloud_points=N,
               tile=[8, 32], hbm_peak=HBM_PEAK)
    print(f"fused cloud: {N} points", flush=True)

    # ---- index build
    n_small = min(args.points, N)
    pick = torch.randperm(N, device=d)[:n_small].sort().values
    small = cloud[pick, :3].contiguous()
    xyz = cloud[:, :3].contiguous()
    res["index_build"] = {str(n): timed(lambda p=p: ops.point_index_build(p, r), args.reps) for n, p in ((n_small, small), (N, xyz))}
    print(json.dumps(dict(index_build=res["index_build"])), flush=True)

    # ---- point form against chunked cdist
    g = torch.Generator(device=d).manual_seed(0)
    queries = (small + (torch.rand(small.shape, device=d, generator=g) - 0.5) * 0.01).contiguous()
    index = transfer.PointIndex(small, r)
    idx = index.nearest(queries)
    ref = cdist_nearest(small, queries, r)
    differ = int((idx.long() != ref).sum().item())                                    # cdist's own arithmetic may move a near-tie
    pt = dict(n=n_small, m=n_small, hits=int((idx >= 0).sum().item()), differ_from_cdist=differ)
    pt["kernel"] = timed(lambda: index.nearest(queries), args.reps)
    pt["cdist_chunks_min"] = timed(lambda: cdist_nearest(small, queries, r), max(3, args.reps // 2), warmup=1)
    pt["ns_per_query_kernel"] = pt["kernel"]["median_ms"] * 1e6 / n_small
    pt["ns_per_query_cdist"] = pt["cdist_chunks_min"]["median_ms"] * 1e6 / n_small
    pt["cdist_over_kernel"] = pt["cdist_chunks_min"]["median_ms"] / pt["kernel"]["median_ms"]
    res["point_form"] = pt
    print(json.dumps(dict(point_form=pt)), flush=True)
    del ref, idx

    # ---- pixel form
    index = transfer.PointIndex(xyz, r)
    M = V * H * W
    labels = torch.randint(0, 200, (5, N), dtype=torch.int32, device=d)
    px = dict(queries=M, n=N)
    hit = index.nearest_pixels(distinct)
    px["hit_share_of_distinct_views"] = float((hit >= 0).float().mean().item())
    px["valid_depth_share"] = float((distinct.depth.view(torch.int16) != 0).float().mean().item())
    del hit
    for L in (0, 1, 5):
        lab = labels[:L] if L else None
        t = timed(lambda: index.nearest_pixels(views, labels=lab, return_index=L == 0), args.reps)
        nbytes = M * (2 + 4 * max(L, 1))
        sec = t["median_ms"] * 1e-3
        px[f"L{L}"] = dict(t, bytes_needed=nbytes, queries_per_s=M / sec, ns_per_query=sec * 1e9 / M, needed_TBps=nbytes / sec / 1e12,
                           needed_fraction_of_hbm_peak=nbytes / sec / HBM_PEAK)
        print(json.dumps({f"pixel_form_L{L}": px[f"L{L}"]}), flush=True)
    # the same queries without the tile's table: the point form on the back-projected pixels of the distinct views
    w = back_project(distinct)
    a, b = index.nearest(w), index.nearest_pixels(distinct)
    px["point_form_vs_pixel_form_index_differs"] = int((a != b.reshape(-1)).sum().item())   # torch's back-projection contracts: a few may
    t_pt, t_px = timed(lambda: index.nearest(w), args.reps), timed(lambda: index.nearest_pixels(distinct), args.reps)
    px["distinct_views_point_form"], px["distinct_views_pixel_form"] = t_pt, t_px
    px["per_query_lookup_over_tile_table"] = t_pt["median_ms"] / t_px["median_ms"]
    px["ns_per_query_cdist_at_150k"] = pt["ns_per_query_cdist"]
    px["cdist_per_query_over_pixel_form_L1"] = pt["ns_per_query_cdist"] / px["L1"]["ns_per_query"]
    res["pixel_form"] = px
    print(json.dumps(dict(pixel_form_ablation={k: v for k, v in px.items() if not k.startswith("L")})), flush=True)
    del w, a, b, labels

    # ---- what the pixel form's time is made of, on the distinct views: the same launch with less and less to do
    parts = dict(queries=n_distinct * H * W)
    dark = lift2d.Views(torch.zeros_like(distinct.depth), distinct.intrinsics, room["poses"], K.DEPTH_SCALE)
    parts["no_valid_depth"] = timed(lambda: index.nearest_pixels(dark), args.reps)              # read depth, write -1
    far_away = transfer.PointIndex(torch.full((1, 3), 9000.0, device=d), r)
    parts["no_source_point_near"] = timed(lambda: far_away.nearest_pixels(distinct), args.reps)  # + back-projection, the box, its bucket lookups
    parts["radius_sweep"] = []
    for rr in (0.02, 0.03, 0.04, 0.06, 0.08):                                                   # + candidates: they grow with r^2 on a surface
        ix = transfer.PointIndex(xyz, rr)
        i2, d2 = ix.nearest_pixels(distinct, return_d2=True)
        t = timed(lambda: ix.nearest_pixels(distinct), args.reps)
        parts["radius_sweep"].append(dict(radius=rr, cell_m=(int(np.ceil(np.float32(rr) * 1024)) + 2) / 1024.0, median_ms=t["median_ms"],
                                          min_ms=t["min_ms"], max_ms=t["max_ms"], hit_share=float((i2 >= 0).float().mean().item())))
        del ix, i2, d2
    thin = xyz[::4].contiguous()                                                                # a quarter of the points at r = 0.04
    ix = transfer.PointIndex(thin, r)
    parts["quarter_of_the_points"] = timed(lambda: ix.nearest_pixels(distinct), args.reps)
    res["pixel_form_parts"] = parts
    print(json.dumps(dict(pixel_form_parts=parts)), flush=True)
    del ix, thin, dark, far_away

    # ---- instance map
    res["instance_map"] = {}
    for I in (100, 600):
        masks = torch.rand(I, n_small, device=d, generator=g) < 0.05
        scores = torch.rand(I, device=d, generator=g)
        got = transfer.instance_map(masks, scores)
        weighted = masks * scores[:, None]
        want = torch.where(weighted.max(0).values > 0, weighted.argmax(0), torch.full_like(got, -1, dtype=torch.int64))
        im = dict(differ_from_torch=int((got.long() != want).sum().item()), bytes_needed=I * n_small + 4 * n_small)
        im["kernel"] = timed(lambda: transfer.instance_map(masks, scores), args.reps)
        im["torch_mul_argmax"] = timed(lambda: (masks * scores[:, None]).argmax(0), args.reps)
        im["needed_TBps"] = im["bytes_needed"] / (im["kernel"]["median_ms"] * 1e-3) / 1e12
        im["torch_over_kernel"] = im["torch_mul_argmax"]["median_ms"] / im["kernel"]["median_ms"]
        res["instance_map"][str(I)] = im
        print(json.dumps({f"instance_map_{I}": im}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
