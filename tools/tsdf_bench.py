"""Times the TSDF fusion of posed RGB-D frames and the surface-net mesh (`segdino3d_amd/tsdf.py`, csrc/tsdf.hip) on a synthetic scene
of real size, no files: the closed-form room of tests/fuse_views_case.py scaled to a ScanNet-sized room, 480 x 640 uint16 depth and
480 x 640 colour, 64 distinct views (the 256-view run repeats them four times: the same blocks, four times the updates), fed in
calls of 64 views, the most one touch / integrate pair takes.

    python tools/tsdf_bench.py [--views 256 64] [--reps 5] [--scale 1.5] [--torch-views 8] [--out profiles/tsdf_mesh.json]

Reports, per view count: touch (steps 1 and 2), integrate (step 3) and extract (steps 4 to 6 with the host read) by HIP events around
the queue of calls; voxel updates per second; the blocks used, the vertices and the faces; the bytes each stage must move; and, for
context, the same integration written with torch tensor ops on the same device - every voxel of a dense grid of the room's extent
projected into each view, then `index_add_` - over `--torch-views` views (it carves all the free space in front of a surface, not
only the touched blocks, so it makes more updates; its time per view is what is compared)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import fuse_views_case as K  # noqa: E402

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


def minus(a, b):
    return {k: (x - b["median_ms"] if k.endswith("_ms") else x) for k, x in a.items()}


def torch_integration(batches, vdepths, lo, hi, voxel, trunc):
    """Step 3 with tensor ops on a dense grid over [lo, hi): -> (W, T int32 [N], C int32 [N, 3], updates).  The validated depth of
    step 1 is taken from the kernels (`vdepths`): only the projection and the sums are torch's."""
    d = vdepths[0].device
    n = [int((hi[i] - lo[i]) / voxel) for i in range(3)]
    ax = [(torch.arange(n[i], device=d).float() + (0.5 + round(lo[i] / voxel))) * voxel for i in range(3)]
    p = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    N = p.shape[0]
    W, T = torch.zeros(N, dtype=torch.int32, device=d), torch.zeros(N, dtype=torch.int32, device=d)
    C = torch.zeros(N, 3, dtype=torch.int32, device=d)
    qscale = 4096.0 / trunc
    for (views, colors), vdepth in zip(batches, vdepths):
        V, H, Wd = vdepth.shape
        for v in range(V):
            m, k = views.world_to_cam[v], views.intrinsics[v]
            cam = p @ m[:, :3].t() + m[:, 3]
            z = cam[:, 2]
            u = torch.floor(k[0] * cam[:, 0] / z + k[2] + 0.5)
            w = torch.floor(k[1] * cam[:, 1] / z + k[3] + 0.5)
            ok = (z > 0) & (u >= 0) & (u < Wd) & (w >= 0) & (w < H)
            idx = torch.nonzero(ok).flatten()
            ui, vi = u[idx].long(), w[idx].long()
            dd = vdepth[v][vi, ui]
            sdf = dd - z[idx]
            keep = (dd > 0) & (sdf >= -trunc)
            idx, ui, vi, sdf = idx[keep], ui[keep], vi[keep], sdf[keep]
            q = torch.round(torch.clamp(sdf, max=trunc) * qscale).int()
            W.index_add_(0, idx, torch.ones_like(q))
            T.index_add_(0, idx, q)
            C.index_add_(0, idx, colors[v][vi, ui].int())
    return W, T, C, N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[256, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--torch-views", type=int, default=8)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--capacity", type=int, default=1 << 16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_mesh.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_bench: needs a HIP device (a measurement does not fall back to the CPU)")
    from segdino3d_amd import lift2d, ops, tsdf
    d = torch.device("cuda:0")
    H, W, B = args.height, args.width, ops.TSDF_MAX_CALL_VIEWS
    rule, voxel, trunc, cap = dict(tsdf.RULE_DEFAULTS), 0.02, 0.08, args.capacity
    t0 = time.perf_counter()
    n_distinct = min(DISTINCT_VIEWS, max(args.views))
    room = K.room(n_distinct, H, W, (H, W), scale=args.scale)
    print(f"{n_distinct} views of {H} x {W} rendered on the host in {time.perf_counter() - t0:.1f} s", flush=True)
    res = dict(depth=[H, W], colors=[H, W], views_per_call=B, scale=args.scale, voxel=voxel, trunc=trunc, rule=rule, capacity=cap,
               device=torch.cuda.get_device_name(0))
    for V in args.views:
        batches = []
        for lo in range(0, V, B):
            idx = [(lo + i) % n_distinct for i in range(min(B, V - lo))]
            views = lift2d.Views(torch.from_numpy(room["depth_u16"][idx]).to(d), torch.from_numpy(room["intr"][idx]).to(d), room["poses"][idx],
                                 K.DEPTH_SCALE)
            batches.append((views, torch.from_numpy(room["colors"][idx]).to(d)))
        torch.cuda.synchronize()
        r = dict(views=V, pixels=V * H * W)
        vol = tsdf.TsdfVolume(voxel=voxel, trunc=trunc, capacity=cap)
        for v, c in batches:
            vol.add(v, c)
        vertices, faces, info = vol.mesh(return_info=True)
        r["info"] = info._asdict()
        ws = vol._ws

        r["state_bytes"] = ws.numel()

        def reset():
            ops.tsdf_reset(ws, cap)

        def touch():
            return [ops.tsdf_touch(v.depth, v.depth_scale, v.intrinsics, v.cam_to_world, ws, cap, vol.inv_voxel, vol.half_step, rule["near"],
                                   rule["far"], rule["edge_abs"], rule["edge_rel"]) for v, _ in batches]

        def both():
            for v, c in batches:
                vd = ops.tsdf_touch(v.depth, v.depth_scale, v.intrinsics, v.cam_to_world, ws, cap, vol.inv_voxel, vol.half_step, rule["near"],
                                    rule["far"], rule["edge_abs"], rule["edge_rel"])
                ops.tsdf_integrate(vd, v.intrinsics, v.world_to_cam, c, ws, cap, voxel, trunc, vol.qscale)

        r["reset"] = timed(reset, args.reps)
        # touch alone leaves the `touched` words set, so a later touch of the same blocks lists nothing again: the list appends of the
        # repeated views (one per block and call) are missing from this figure; each timed run starts from an emptied table
        r["reset_and_touch"] = timed(lambda: (reset(), touch()), args.reps)
        r["reset_touch_integrate"] = timed(lambda: (reset(), both()), args.reps)
        r["touch"] = minus(r["reset_and_touch"], r["reset"])
        r["integrate"] = minus(r["reset_touch_integrate"], r["reset_and_touch"])
        r["extract_with_host_read"] = timed(lambda: vol.mesh(), args.reps)
        again_v, again_f, again = vol.mesh(return_info=True)
        assert torch.equal(again_v, vertices) and torch.equal(again_f, faces) and again == info, "the timing runs changed the mesh"
        blocks, updates = info.blocks, info.updates
        r["updates_per_s"] = updates / (r["integrate"]["median_ms"] * 1e-3)
        r["updates_per_block_voxel"] = updates / (blocks * 512)
        # what each stage must move: touch reads depth and writes the validated depth; integrate reads and writes each listed block once
        # per call (10 KiB each way) and one validated depth and one colour pixel per update; extract reads W and T of every block and
        # the keys of every slot, and sorts max_vertices (key, index) pairs in eight passes
        calls = len(batches)
        r["bytes"] = dict(touch=V * H * W * (2 + 4), integrate=calls * blocks * 2 * 10240 + updates * (4 + 3),
                          extract=blocks * 4096 + cap * 8 + info.vertices * (8 * 20 + 24 + 24) + info.faces * 12)
        for k in ("touch", "integrate"):
            r[f"{k}_TBps"] = r["bytes"][k] / (r[k]["median_ms"] * 1e-3) / 1e12
        r["extract_TBps"] = r["bytes"]["extract"] / (r["extract_with_host_read"]["median_ms"] * 1e-3) / 1e12
        if V == min(args.views) and args.torch_views > 0:
            n = min(args.torch_views, len(batches[0][0]))
            v0, c0 = batches[0]
            sub = lift2d.Views(v0.depth[:n], v0.intrinsics[:n], room["poses"][:n], K.DEPTH_SCALE)
            reset()
            vd = touch()[0][:n].contiguous()
            reset()
            both()
            lo = [float(x) * args.scale - 0.08 for x in K.ROOM_LO]
            hi = [float(x) * args.scale + 0.08 for x in K.ROOM_HI]
            Wt, _, _, N = torch_integration([(sub, c0[:n])], [vd], lo, hi, voxel, trunc)
            r["torch_integration"] = dict(views=n, grid_voxels=N, updates=int(Wt.sum().item()),
                                          **timed(lambda: torch_integration([(sub, c0[:n])], [vd], lo, hi, voxel, trunc), max(2, args.reps // 2)))
            r["torch_ms_per_view"] = r["torch_integration"]["median_ms"] / n
            r["kernels_ms_per_view"] = (r["touch"]["median_ms"] + r["integrate"]["median_ms"]) / V
            r["torch_over_kernels_per_view"] = r["torch_ms_per_view"] / r["kernels_ms_per_view"]
            del Wt
        res[f"views_{V}"] = r
        print(json.dumps({f"views_{V}": r}), flush=True)
        del batches, vol, vertices, faces
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
