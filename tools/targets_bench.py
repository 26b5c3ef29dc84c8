"""Dataset targets on the device against the host route, on one scene of real size, in one process:
python tools/targets_bench.py [--reps 20] [--warmup 3] [--points 150000] [--superpoints 3000] [--instances 60] [--files 16]

The scene: synth.make_scene (150 k points, 3 000 superpoints) with superpoint-coherent raw labels of ~60 instances over 200
classes, stuff and unlabeled superpoints among them, 5 % of the points carrying another superpoint's label.
  (a) device: the two C calls of targets.build_targets (csrc/targets.hip), HIP events around each (train view), and the whole call
      on a host clock ending in a synchronise - it contains the one 16-byte read-back;
  (b) host: the CPU restatement of the reference's dataset code (tests/targets_ref.py: float one-hot matrices, scatter mean, the
      Python loop over instances) with 16 torch threads, host clock;
  (c) io_scene.ScenePrefetcher over `--files` copies of the packed scene, scenes/s with and without `labels`, alternating.
Every repetition is kept; the JSON line gives median / min / max per figure and whether (a) and (b) agree bit for bit."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from segdino3d_amd import ops
from segdino3d_amd.io_scene import ScenePrefetcher, pack_scene
from segdino3d_amd.synth import make_scene
from segdino3d_amd.targets import LabelSpec, build_targets


def labelled_scene(n_points, n_superpoints, n_inst, seed=0):
    pts, tgt = make_scene(seed, n_points=n_points, n_superpoints=n_superpoints)
    ef = tgt.extra_features
    sp = ef["super_point_masks"]
    g = torch.Generator().manual_seed(seed)
    owner = torch.randint(0, n_inst, (n_superpoints,), generator=g)
    rest = torch.rand(n_superpoints, generator=g) < 0.3                                  # walls, floor, unlabeled
    cls_of = torch.randint(2, 200, (n_inst,), generator=g)
    inst_sp = torch.where(rest, torch.full_like(owner, -1), owner * 7 + 3)
    sem_sp = torch.where(rest, torch.tensor([0, 1, 200])[torch.randint(0, 3, (n_superpoints,), generator=g)], cls_of[owner])
    src = torch.where(torch.rand(n_points, generator=g) < 0.05, torch.randint(0, n_superpoints, (n_points,), generator=g), sp)
    return dict(points=pts, super_points=sp, points_2dfeats=ef["points_2dfeats"], query2d_feats=ef["query2d_feats"],
                query2d_pos=ef["query2d_pos"], instance_mask=inst_sp[src], semantic_mask=sem_sp[src])


def stats(xs, unit="ms"):
    return {f"median_{unit}": round(statistics.median(xs), 4), f"min_{unit}": round(min(xs), 4), f"max_{unit}": round(max(xs), 4), "reps": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=150_000)
    ap.add_argument("--superpoints", type=int, default=3000)
    ap.add_argument("--instances", type=int, default=60)
    ap.add_argument("--files", type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("targets_bench: needs a HIP device (a measurement does not fall back to the CPU)")
    from targets_ref import targets_ref
    d = torch.device("cuda:0")
    scene = labelled_scene(a.points, a.superpoints, a.instances)
    spec = LabelSpec(200, np.arange(201), (0, 1), False, "bench", "cdn")
    inst, sem, sp = (scene[k].to(d) for k in ("instance_mask", "semantic_mask", "super_points"))
    lut = spec.table(d)

    scan, build, call = [], [], []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for it in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        ev[0].record()
        ws, header = ops.targets_scan(inst, sem, sp, lut, spec.n_classes, spec.stuff_ids, spec.swap_2_3)
        ev[1].record()
        hdr = header.wait()
        ev[2].record()
        out = ops.targets_build(ws, hdr, inst.numel(), spec.n_classes, spec.stuff_ids, val_view=False)
        ev[3].record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tgt = build_targets(inst, sem, sp, spec, "train")
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
        if it >= a.warmup:
            scan.append(ev[0].elapsed_time(ev[1])); build.append(ev[2].elapsed_time(ev[3])); call.append(ms)
    G, S = out["n_instances"], out["n_superpoints"]
    out_bytes = G * inst.numel() + (G + 201) * S
    result = dict(points=a.points, superpoints=S, instances=G, output_bytes=out_bytes,
                  device_scan=stats(scan), device_build=stats(build), build_targets_call_with_readback=stats(call))

    torch.set_num_threads(16)
    host = []
    args = [scene[k].numpy() for k in ("instance_mask", "semantic_mask", "super_points")]
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        ref = targets_ref(*args, np.arange(201), 200)
        host.append(1e3 * (time.perf_counter() - t0))
    result["host_restatement_16_threads"] = stats(host)
    result["same_bits"] = bool(all(np.array_equal(tgt[k].cpu().numpy(), ref[k]) for k in ("masks", "labels", "area", "sp_inst_sem_masks")))

    if a.files <= 0:                                                  # --files 0: the kernels alone
        print(json.dumps(result))
        return
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "scene.bin")
        pack_scene(path, scene)
        rates = {"labels": [], "no_labels": []}
        for it in range(2 + 6):
            for key, kw in (("no_labels", {}), ("labels", dict(labels=spec, scene_set="train"))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = sum(1 for _ in ScenePrefetcher([path] * a.files, d, **kw))
                torch.cuda.synchronize()
                if it >= 2:
                    rates[key].append(n / (time.perf_counter() - t0))
        result["prefetcher_scenes_per_s"] = {k: stats(v, "per_s") for k, v in rates.items()}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
