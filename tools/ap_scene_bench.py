"""Times per-scene instance AP on the device (`eval_ap_scene.SceneApAccumulator`, csrc/apeval_scene.hip) against the only per-scene
route there was before it: the host route `eval_ap.instance_seg_eval` called with one scene at a time, as the reference's
`compute_each_sample_metrics` does.  The scene is that of tools/ap_eval_bench.py: 150 k points, about 60 ground-truth instances of a
198-class label set, 100 / 600 predictions.

    python tools/ap_scene_bench.py [--out profiles/ap_per_scene.md] [--points 150000] [--scenes 312] [--host-scenes 16]

Device route: `--scenes` scenes into one accumulator (wall time of the adds with a synchronisation on either side), then
`scene_tables()` - HIP events around `ops.ap_finish_scenes` for the device time, wall time for the call with its read-back - and
`scene_results()`, which adds `compute_averages` per scene on the host; medians of `--repeats` runs.  Host route: wall time of
`instance_seg_eval` per scene (it synchronises), median over `--host-scenes` calls, times `--scenes` - an extrapolation, the full
pass takes minutes.  Both routes are compared on a scene before anything is timed.  Writes a markdown note."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from ap_eval_bench import make_scene  # noqa: E402
from segdino3d_amd import eval_ap, eval_ap_scene, ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ap_per_scene.md"))
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--scenes", type=int, default=312)
    ap.add_argument("--host-scenes", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ap_scene_bench: needs a HIP device (there is no CPU path to time)")
    if args.host_scenes < 16:
        raise SystemExit("ap_scene_bench: time the host route over at least 16 scenes")
    d = torch.device("cuda:0")
    N, S = args.points, args.scenes
    rows = []
    for n in (100, 600):
        valid, sem, inst, masks, labels, scores = make_scene(N, n, seed=n)
        class_labels = tuple(f"c{i}" for i in valid)
        sem, inst, masks, labels, scores = (t.to(d) for t in (sem, inst, masks, labels, scores))
        new = lambda: eval_ap_scene.SceneApAccumulator(valid, class_labels, device=d)       # noqa: E731

        def host_scene():
            return eval_ap.instance_seg_eval([sem], [inst], [masks], [labels], [scores], valid, class_labels)

        # both routes agree on a scene before anything is timed
        acc = new()
        acc.add_scene(sem, inst, masks, labels, scores, 0)
        acc.add_scene(sem, inst, masks, labels, scores, 1)
        got, want = acc.scene_results(), host_scene()
        for k in (0, 1):
            for name, v in want.items():
                if name != "classes":
                    assert (np.isnan(v) and np.isnan(got[k][name])) or abs(got[k][name] - v) <= 1e-12, (k, name, got[k][name], v)

        # the device route: a pass of S scenes
        acc = new()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for k in range(S):
            acc.add_scene(sem, inst, masks, labels, scores, k)
        torch.cuda.synchronize()
        t_adds = time.perf_counter() - t
        codes, counters = acc._store[:acc.used], acc._scene_rows[:S]
        ops.ap_finish_scenes(codes, acc._offsets, acc.n_classes, acc.n_overlaps, counters, acc.mask50, acc.mask25)      # workspace
        t_dev, t_tables, t_results = [], [], []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            ops.ap_finish_scenes(codes, acc._offsets, acc.n_classes, acc.n_overlaps, counters, acc.mask50, acc.mask25)
            b.record()
            b.synchronize()
            t_dev.append(a.elapsed_time(b) * 1e-3)
            t = time.perf_counter()
            acc.scene_tables()
            t_tables.append(time.perf_counter() - t)
            t = time.perf_counter()
            acc.scene_results()
            t_results.append(time.perf_counter() - t)

        # the host route, one scene at a time
        for _ in range(2):
            host_scene()
        t_host = []
        for _ in range(args.host_scenes):
            torch.cuda.synchronize()
            t = time.perf_counter()
            host_scene()
            t_host.append(time.perf_counter() - t)
        rows.append(dict(n=n, slots=acc.used, t_adds=t_adds, t_dev=statistics.median(t_dev), t_tables=statistics.median(t_tables),
                         t_results=statistics.median(t_results), t_host=statistics.median(t_host)))

    lines = ["# Per-scene instance AP scored on the device", "",
             f"`tools/ap_scene_bench.py`: N = {N} points, 198 classes, 60 ground-truth instances, 10 overlaps, min_region 100, {S} scenes "
             f"(the same scene {S} times, under {S} keys); device = {torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName}).  Seconds.  `adds`: wall time of every "
             "`add_scene` of the pass with a synchronisation on either side.  `finish (device)`: HIP events around "
             "`ops.ap_finish_scenes` - keys, sort, one workgroup per (scene, class, overlap), one wave per scene.  `scene_tables()`: wall "
             "time of the call with its one read-back.  `scene_results()`: the same plus `compute_averages` per scene on the host, the "
             f"dictionary `compute_each_sample_metrics` returns.  Medians of {args.repeats} runs.  Host route: wall time of "
             f"`eval_ap.instance_seg_eval` on one scene (it synchronises), median of {args.host_scenes} calls, and that time "
             f"MULTIPLIED by {S} - an extrapolation, not a measured pass.", "",
             "| predictions | slots | adds | finish (device) | scene_tables() | scene_results() | host route, one scene | "
             f"host route x {S} (extrapolated) |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} | {r['slots']} | {r['t_adds']:.3f} | {r['t_dev']:.4f} | {r['t_tables']:.4f} | {r['t_results']:.3f} | "
                     f"{r['t_host']:.3f} | {r['t_host'] * S:.1f} |")
    lines += ["", "The pass end to end, seconds, and how many times longer the (extrapolated) host route takes: to the tables (`adds` + "
              "`scene_tables()`: everything the device does, `summary` included) and to the dictionaries (`adds` + `scene_results()`).", "",
              "| predictions | device pass to the tables | host / device | device pass to the dictionaries | host / device |",
              "|---|---|---|---|---|"]
    for r in rows:
        to_tables, to_dicts, host_pass = r["t_adds"] + r["t_tables"], r["t_adds"] + r["t_results"], r["t_host"] * S
        lines.append(f"| {r['n']} | {to_tables:.3f} | {host_pass / to_tables:.0f}x | {to_dicts:.3f} | {host_pass / to_dicts:.1f}x |")
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
