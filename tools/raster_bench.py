"""Times the mesh rasteriser (`segdino3d_amd/raster.py`, csrc/raster.hip) on synthetic scenes of real size, no files: the closed-form
room of tests/fuse_views_case.py scaled to a ScanNet-sized room, 64 distinct views of 480 x 640 (the 256-view run repeats them four
times), fused by `tsdf.TsdfVolume` into the two meshes that are then drawn: the room mesh of tools/tsdf_bench.py (2 cm voxels, about
448 k vertices and 938 k faces) and a scan-sized one (3.5 cm voxels, about 150 k vertices and 300 k faces).

    python tools/raster_bench.py [--views 256] [--reps 5] [--out profiles/raster.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/raster_bench.py --trace-run --reps 3     # a run of its own
    python tools/raster_bench.py --stages-from DIR/.../kernel_trace.csv --reps 3 --out profiles/raster_stages.json  # no device needed

The first form reports, per mesh and with 0 and 5 label channels (HIP events around the call; warm-up, then `--reps` runs: median,
min, max): ms per call and per view, (view, face) pairs and covered samples per second, the counters, the bytes that must move against
the HBM peak, and two comparison lines: the numpy restatement tests/raster_ref.py on the host over `--host-views` of the same views
(its time per view, EXTRAPOLATED to all views, and its exact count of samples = atomics issued, per pixel hit), and
`PointIndex.nearest_pixels` over the mesh vertices on the SENSOR depth of the same views, which does the same job where depth exists.
Kernel times come from a profiler run of their own (`--trace-run` issues the same calls in a fixed order and nothing else from this
library after the meshes are built); `--stages-from` cuts that trace's raster_* rows into calls by their fixed order and reports each
stage's time per call."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HBM_PEAK = 8.0e12
DISTINCT_VIEWS = 64
MESHES = (("room", 0.02), ("scan", 0.035))
LABELS = (0, 5)
STAGES = ("raster_setup_kernel", "raster_draw_small_kernel", "raster_draw_large_kernel", "raster_resolve_kernel")
WARMUP = 1


def timed(fn, reps, warmup=WARMUP):
    import torch
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


def stages_from(path, views, per_pass, reps):
    """The raster_* rows of a rocprofv3 kernel trace of a `--trace-run`, in start order, cut into calls: a call is ceil(views /
    per_pass) passes of the four kernels, and the run makes (WARMUP + reps) calls per (mesh, labels) in the order of MESHES x LABELS."""
    rows = list(csv.DictReader(open(path)))
    col = {k.lower(): k for k in rows[0]}
    name, start, end = col["kernel_name"], col["start_timestamp"], col["end_timestamp"]
    ours = sorted(((int(r[start]), int(r[end]), next(s for s in STAGES if s in r[name])) for r in rows if any(s in r[name] for s in STAGES)))
    passes = -(-views // per_pass)
    per_call = passes * len(STAGES)
    want = len(MESHES) * len(LABELS) * (WARMUP + reps) * per_call
    if len(ours) != want:
        raise SystemExit(f"raster_bench: {len(ours)} raster kernel rows in the trace, expected {want}: was it a --trace-run with the same --views and --reps?")
    out, at = {}, 0
    for mesh, _ in MESHES:
        for L in LABELS:
            calls = []
            for c in range(WARMUP + reps):
                chunk = ours[at:at + per_call]
                at += per_call
                if c >= WARMUP:
                    calls.append({s: sum(e - b for b, e, n in chunk if n == s) * 1e-6 for s in STAGES} | dict(span=(chunk[-1][1] - chunk[0][0]) * 1e-6))
            out[f"{mesh}_L{L}"] = {k: dict(median_ms=statistics.median(c[k] for c in calls), min_ms=min(c[k] for c in calls),
                                           max_ms=max(c[k] for c in calls)) for k in STAGES + ("span",)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--views-per-pass", type=int, default=32)
    ap.add_argument("--host-views", type=int, default=2)
    ap.add_argument("--radius", type=float, default=0.04)
    ap.add_argument("--trace-run", action="store_true", help="only the rasteriser calls, in a fixed order: for a profiler run")
    ap.add_argument("--stages-from", default=None, help="a kernel_trace.csv of a --trace-run: report stage times, no device needed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster.json"))
    args = ap.parse_args()
    if args.stages_from:
        res = dict(views=args.views, views_per_pass=args.views_per_pass, reps=args.reps,
                   stages=stages_from(args.stages_from, args.views, args.views_per_pass, args.reps))
        print(json.dumps(res, indent=1))
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        return
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("raster_bench: needs a HIP device (a measurement does not fall back to the CPU)")
    import fuse_views_case as K
    import raster_ref as R
    from segdino3d_amd import lift2d, ops, raster, transfer, tsdf
    d = torch.device("cuda:0")
    H, W, V = args.height, args.width, args.views
    t0 = time.perf_counter()
    n_distinct = min(DISTINCT_VIEWS, V)
    room = K.room(n_distinct, H, W, (H, W), scale=args.scale)
    print(f"{n_distinct} views of {H} x {W} rendered on the host in {time.perf_counter() - t0:.1f} s", flush=True)
    sel = [i % n_distinct for i in range(V)]
    poses, intr = room["poses"][sel], torch.from_numpy(room["intr"][sel]).to(d)
    res = dict(device=torch.cuda.get_device_name(0), image=[H, W], views=V, distinct_views=n_distinct, views_per_pass=args.views_per_pass,
               small_max_pixels=ops.RASTER_SMALL_MAX_PIXELS, hbm_peak=HBM_PEAK)
    meshes = {}
    for name, voxel in MESHES:
        vol = tsdf.TsdfVolume(voxel=voxel, trunc=4 * voxel, capacity=1 << 16)
        for lo in range(0, n_distinct, ops.TSDF_MAX_CALL_VIEWS):
            idx = list(range(lo, min(n_distinct, lo + ops.TSDF_MAX_CALL_VIEWS)))
            vol.add(lift2d.Views(torch.from_numpy(room["depth_u16"][idx]).to(d), torch.from_numpy(room["intr"][idx]).to(d), room["poses"][idx],
                                 K.DEPTH_SCALE), torch.from_numpy(room["colors"][idx]).to(d))
        vertices, faces = vol.mesh()
        meshes[name] = (vertices[:, :3].contiguous(), faces.contiguous())
        print(f"{name}: voxel {voxel}, {vertices.shape[0]} vertices, {faces.shape[0]} faces", flush=True)
        del vol
    torch.cuda.synchronize()
    for name, (vertices, faces) in meshes.items():
        Nv, F = vertices.shape[0], faces.shape[0]
        labels = torch.randint(0, 200, (5, Nv), dtype=torch.int32, device=d)
        for L in LABELS:
            def call(L=L):
                return raster.render_mesh(vertices, faces, intr, poses, H, W, vertex_labels=labels if L else None, views_per_pass=args.views_per_pass)
            t = timed(call, args.reps)
            if args.trace_run:
                continue
            out = call()
            info = out.read_info()
            sec = t["median_ms"] * 1e-3
            # what must move: the key image is cleared, read and resolved once (8 + 8 bytes a pixel and 4 per output image), a sample is one
            # 8-byte atomic, and every (view, face) pair reads its face (12 bytes; the vertices come from the cache) in setup; a drawn pair
            # writes and reads a record (16) and reads its face again
            outputs = 2 + L
            r = dict(t, vertices=Nv, faces=F, labels=L, info=info, ms_per_view=t["median_ms"] / V, pairs_per_s=V * F / sec,
                     pixels_per_s=V * H * W / sec, hit_share=info["pixels"] / (V * H * W))
            r["bytes_needed"] = V * H * W * (16 + 4 * outputs) + V * F * 12 + info["drawn"] * 28
            r["needed_TBps"] = r["bytes_needed"] / sec / 1e12
            r["needed_fraction_of_hbm_peak"] = r["bytes_needed"] / sec / HBM_PEAK
            res[f"{name}_L{L}"] = r
            print(json.dumps({f"{name}_L{L}": r}), flush=True)
        if args.trace_run:
            continue
        # the restatement on the host over a few of the same views: its exact sample count, and its time, extrapolated
        hv = min(args.host_views, V)
        t0 = time.perf_counter()
        ref = R.render_mesh(vertices.cpu().numpy(), faces.cpu().numpy(), room["intr"][sel][:hv], poses[:hv], H, W)
        host_s = time.perf_counter() - t0
        got = raster.render_mesh(vertices, faces, intr[:hv], poses[:hv], H, W)
        same = bool(np.array_equal(got.depth.cpu().numpy().view(np.uint32), ref["depth"].view(np.uint32)) and
                    np.array_equal(got.face.cpu().numpy(), ref["face"]) and got.read_info() == ref["info"])
        sec = res[f"{name}_L0"]["median_ms"] * 1e-3
        res[f"{name}_host"] = dict(views=hv, seconds=host_s, seconds_per_view=host_s / hv, extrapolated_seconds_all_views=host_s / hv * V,
                                   extrapolated_over_kernels=host_s / hv * V / sec, equal_bits=same, samples=ref["samples"],
                                   pixels=ref["info"]["pixels"], atomics_per_pixel_hit=ref["samples"] / max(ref["info"]["pixels"], 1),
                                   samples_per_s_extrapolated=ref["samples"] / hv * V / sec)
        print(json.dumps({f"{name}_host": res[f"{name}_host"]}), flush=True)
        # the same job where depth exists: the nearest vertex of every sensor-depth pixel
        views = lift2d.Views(torch.from_numpy(room["depth_u16"][sel]).to(d), intr, poses, K.DEPTH_SCALE)
        index = transfer.PointIndex(vertices, args.radius)
        for L in LABELS:
            t = timed(lambda L=L: index.nearest_pixels(views, labels=labels if L else None, return_index=L == 0), args.reps)
            res[f"{name}_nearest_pixels_L{L}"] = dict(t, ms_per_view=t["median_ms"] / V, radius=args.radius,
                                                      over_raster=t["median_ms"] / res[f"{name}_L{L}"]["median_ms"])
            print(json.dumps({f"{name}_nearest_pixels_L{L}": res[f"{name}_nearest_pixels_L{L}"]}), flush=True)
        del views, index, labels
    if args.trace_run:
        print("trace run done")
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
