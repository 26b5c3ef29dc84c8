"""Times the lifting of 2D detector queries to 3D centres (`segdino3d_amd/lift_queries.py`, csrc/lift_queries.hip) on a synthetic scene
of real size, no files: the analytic room of tests/lift2d_case.py, 256 views of 480 x 640 uint16 depth (32 distinct ray-cast views,
repeated), 100 queries per view with C = 256 fp16 features, masks at 480 x 640 and at 240 x 320, fed in `add` calls of 32 views.  A
query's mask is a random rectangle cut to the depth band of its centre pixel, plus the rectangle's two-pixel rim (a mask that leaks
onto the background).

    python tools/lift_queries_bench.py [--views 256] [--queries 100] [--reps 5] [--baseline-views 8] [--out profiles/lift_queries.json]

Reports, per mask resolution: milliseconds per scene (all `add`s + `result()`) by HIP events; the centre kernel alone, the bytes it
must read (every mask once, the depth pixels under the masks once) and the rate they imply against the 8 TB/s HBM peak; selection +
gather; and the baseline - the plain torch formulation on the same device, the way a user would write it today (per view and query:
boolean index, `torch.median`, gate, mean) - over `--baseline-views` views, scaled to all views.  The baseline's centres are compared
with the kernels' before anything is timed."""
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

HBM_PEAK = 8.0e12
DISTINCT_VIEWS = 32


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


def metres(depth_u16, scale):
    return depth_u16.view(torch.int16).to(torch.int32).bitwise_and(0xFFFF).float() * scale


def make_masks(depth_m, Q, gen):
    """depth_m fp32 [B, H, W] metres on the device -> uint8 [B, Q, H, W]."""
    B, H, W = depth_m.shape
    d = depth_m.device
    out = torch.empty(B, Q, H, W, dtype=torch.uint8, device=d)
    yy, xx = torch.arange(H, device=d).view(1, H, 1), torch.arange(W, device=d).view(1, 1, W)
    for b in range(B):
        cy, cx = torch.randint(0, H, (Q,), device=d, generator=gen), torch.randint(0, W, (Q,), device=d, generator=gen)
        hh, hw = torch.randint(8, 120, (Q,), device=d, generator=gen), torch.randint(8, 160, (Q,), device=d, generator=gen)
        dy, dx = (yy - cy.view(Q, 1, 1)).abs(), (xx - cx.view(Q, 1, 1)).abs()
        rect = (dy <= hh.view(Q, 1, 1)) & (dx <= hw.view(Q, 1, 1))
        rim = rect & ((dy > hh.view(Q, 1, 1) - 2) | (dx > hw.view(Q, 1, 1) - 2))
        dc = depth_m[b][cy, cx].view(Q, 1, 1)
        band = (depth_m[b].view(1, H, W) - dc).abs() <= 0.15 * dc + 0.05
        out[b] = (rect & band) | rim
    return out


def torch_baseline(views, masks, scores, feats, rule):
    """What a user would write with torch on the device: one view and one query at a time."""
    V, Q, Hm, Wm = masks.shape
    Hd, Wd, d = views.height, views.width, masks.device
    ym = ((2 * torch.arange(Hd, device=d) + 1) * Hm) // (2 * Hd)
    xm = ((2 * torch.arange(Wd, device=d) + 1) * Wm) // (2 * Wd)
    ui, vi = torch.arange(Wd, device=d).float().view(1, Wd), torch.arange(Hd, device=d).float().view(Hd, 1)
    centre, count = torch.zeros(V, Q, 3, device=d), torch.zeros(V, Q, dtype=torch.int64, device=d)
    for v in range(V):
        z = metres(views.depth[v], views.depth_scale)
        k, m = views.intrinsics[v], views.cam_to_world[v]
        world = torch.stack([(ui - k[2]) * z / k[0], (vi - k[3]) * z / k[1], z], -1) @ m[:, :3].T + m[:, 3]
        ok = (z > 0) & (z <= rule["far"])
        mv = masks[v] if (Hm, Wm) == (Hd, Wd) else masks[v][:, ym][:, :, xm]
        for q in range(Q):
            sel = (mv[q] != 0) & ok
            under = z[sel]
            if under.numel() == 0:
                continue
            med = under.median()                                                      # the lower median, as the rule's
            keep = sel & ((z - med).abs() <= rule["gate_abs"] + rule["gate_rel"] * med)
            pts = world[keep]
            centre[v, q], count[v, q] = pts.mean(0), pts.shape[0]
    valid = (scores >= rule["score_thr"]) & (count >= rule["min_pixels"])
    return feats[valid].float(), centre[valid], centre, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-views", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lift_queries.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lift_queries_bench: needs a HIP device (a measurement does not fall back to the CPU)")
    from segdino3d_amd import lift2d, lift_queries, ops
    d = torch.device("cuda:0")
    H, W, V, Q, C, B = 480, 640, args.views, args.queries, args.channels, args.batch
    rule = dict(lift_queries.RULE_DEFAULTS)
    t0 = time.perf_counter()
    n_distinct = min(DISTINCT_VIEWS, V)
    poses, intr, depth = K.make_views(np.random.default_rng(0), n_distinct, H, W)
    depth_u16 = np.round(depth / K.DEPTH_SCALE).astype(np.uint16)
    print(f"{n_distinct} views ray-cast on the host in {time.perf_counter() - t0:.1f} s", flush=True)
    gen = torch.Generator(device=d).manual_seed(0)
    res = dict(views=V, queries=Q, channels=C, depth=[H, W], views_per_add=B, device=torch.cuda.get_device_name(0), rule=rule)

    batches_full = []
    for lo in range(0, V, B):
        idx = [(lo + i) % n_distinct for i in range(min(B, V - lo))]
        views = lift2d.Views(torch.from_numpy(depth_u16[idx]).to(d), torch.from_numpy(intr[idx]).to(d), poses[idx], K.DEPTH_SCALE)
        masks = make_masks(metres(views.depth, K.DEPTH_SCALE), Q, gen)
        scores = torch.rand(len(idx), Q, device=d, generator=gen)
        feats = torch.randn(len(idx), Q, C, device=d, generator=gen).half()
        batches_full.append((views, masks, scores, feats))
    torch.cuda.synchronize()

    for name, step in (("masks_480x640", 1), ("masks_240x320", 2)):
        batches = [(v, m if step == 1 else m[:, :, ::step, ::step].contiguous(), s, f) for v, m, s, f in batches_full]
        r = dict(mask_size=list(batches[0][1].shape[2:]))

        def scene():
            lifter = lift_queries.QueryLifter(C)
            for b in batches:
                lifter.add(*b)
            return lifter, lifter.result()

        lifter, (qf, qp) = scene()
        r["queries_selected"] = int(qf.shape[0])
        r["mean_pixels_kept"] = float(lifter.counts().float().mean().item())
        # correctness at this size first: the torch formulation on the first views
        nb = min(args.baseline_views, len(batches[0][0]))
        v0, m0, s0, f0 = batches[0]
        sub = lift2d.Views(v0.depth[:nb], v0.intrinsics[:nb], poses[[i % n_distinct for i in range(nb)]], K.DEPTH_SCALE)
        _, _, t_centre, t_count = torch_baseline(sub, m0[:nb], s0[:nb], f0[:nb], rule)
        same = t_count == lifter.counts()[:nb]
        diff = (t_centre - lifter.centres()[:nb]).abs().amax(-1)
        # torch gates on metres, the rule on millimetre keys: a pixel on the gate's edge may fall either way, and the count with it
        r["torch_vs_kernels"] = dict(entries=int(same.numel()), entries_with_other_count=int((~same).sum().item()),
                                     max_abs_diff_same_count=float(diff[same].max().item()),
                                     max_abs_diff_other_count=float(diff[~same].max().item()) if bool((~same).any()) else 0.0)

        r["scene"] = timed(lambda: scene(), args.reps)
        outs = [(torch.empty(len(v), Q, 3, device=d), torch.empty(len(v), Q, dtype=torch.int32, device=d),
                 torch.empty(len(v), Q, dtype=torch.int32, device=d)) for v, _, _, _ in batches]

        def centres_only():
            for (v, m, _, _), (c, n, k) in zip(batches, outs):
                ops.lift_query_centres(v.depth, v.depth_scale, v.intrinsics, v.cam_to_world, m, 20000, 100, 50, c, n, k)

        r["centre_kernel"] = timed(centres_only, args.reps)
        mask_bytes = sum(m.numel() for _, m, _, _ in batches)
        set_pixels = sum(int((m != 0).sum().item()) for _, m, _, _ in batches) * step * step         # depth pixels under the masks
        r["bytes_masks"], r["bytes_depth_under_masks"] = mask_bytes, set_pixels * 2
        need = mask_bytes + set_pixels * 2
        rate = need / (r["centre_kernel"]["median_ms"] * 1e-3)
        r["centre_kernel_TBps_of_needed_bytes"] = rate / 1e12
        r["centre_kernel_fraction_of_hbm_peak"] = rate / HBM_PEAK
        # what bounds it: the same launches on empty masks (the pass over the masks alone, no sweeps), and a plain streaming read of
        # the same mask bytes (torch.sum over their int64 view)
        zero = torch.zeros_like(batches[0][1])

        def empty_masks():
            for (v, _, _, _), (c, n, k) in zip(batches, outs):
                if len(v) == zero.shape[0]:
                    ops.lift_query_centres(v.depth, v.depth_scale, v.intrinsics, v.cam_to_world, zero, 20000, 100, 50, c, n, k)

        r["centre_kernel_on_empty_masks"] = timed(empty_masks, args.reps)
        r["torch_sum_of_the_masks"] = timed(lambda: [m.view(torch.int64).sum() for _, m, _, _ in batches], args.reps)
        del zero

        def finish():
            return lifter.result()

        r["select_and_gather"] = timed(finish, args.reps)
        r["torch_baseline"] = timed(lambda: torch_baseline(sub, m0[:nb], s0[:nb], f0[:nb], rule), max(2, args.reps // 2))
        r["torch_baseline"]["views_timed"] = nb
        r["torch_baseline"]["ms_all_views_extrapolated"] = r["torch_baseline"]["median_ms"] * V / nb
        r["torch_over_kernels"] = r["torch_baseline"]["ms_all_views_extrapolated"] / r["scene"]["median_ms"]
        res[name] = r
        print(json.dumps({name: r}), flush=True)
        del batches, outs
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
