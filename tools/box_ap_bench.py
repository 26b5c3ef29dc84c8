"""Times the 3D box AP / AR on the device (`eval_box.BoxApAccumulator`, csrc/boxeval.hip) against the numpy restatement of the same
protocol (tests/box_ap_ref.py) run on the host on the same data: 150 k points, about 60 ground-truth instances of a 198-class label
set, 100 / 600 predicted boxes scattered around the ground-truth boxes.

    python tools/box_ap_bench.py [--out profiles/box_ap.md] [--points 150000] [--scenes 312] [--host-scenes 4]

Per scene: `add()` (ground-truth boxes from the points + matching) in a queue of calls - HIP events around windows of back-to-back
calls and the host's wall time to enqueue them - against `gt_boxes` + `scene` of the restatement on host arrays (wall time; no
transfer is counted on either side).  Per validation pass: `--scenes` scenes into one accumulator and `tables()` (wall time with a
synchronisation on either side) against the restatement's per-scene time x scenes plus its `accumulate` + `finish` over the same
number of scene records.  Entries and tables of both routes are compared before anything is timed.  Writes a markdown note."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import box_ap_ref as R  # noqa: E402

THR = (0.25, 0.5)
VALID = tuple(range(2, 200))


def make_scene(N, n, n_inst=60, seed=0):
    """Host arrays: points [N, 6], semantic / instance ids (mapped already), predicted boxes, labels, scores."""
    rng = np.random.RandomState(seed)
    centre = rng.uniform(0.0, 8.0, size=(n_inst, 3))
    size = rng.uniform(0.4, 1.6, size=(n_inst, 3))
    owner = rng.randint(0, n_inst, size=N)
    pts = np.zeros((N, 6), dtype=np.float32)
    pts[:, :3] = centre[owner] + (rng.rand(N, 3) - 0.5) * size[owner]
    pts[:, 3:] = rng.rand(N, 3)
    sem_of = rng.randint(2, 200, size=n_inst)
    g = rng.randint(0, n_inst, size=n)
    boxes = np.concatenate([centre[g] + rng.normal(0.0, 0.1, (n, 3)) * size[g], size[g] * rng.uniform(0.75, 1.3, (n, 3))], axis=1).astype(np.float32)
    labels = np.where(rng.rand(n) < 0.85, sem_of[g] - 2, rng.randint(0, 198, size=n)).astype(np.int64)
    scores = rng.rand(n).astype(np.float32)
    return pts, sem_of[owner].astype(np.int64), owner.astype(np.int64), boxes, labels, scores


def host_scene(pts, sem, inst, boxes, labels, scores):
    corners, cls, _ = R.gt_boxes(pts, sem, inst, VALID)
    return R.scene(corners, cls, boxes, labels, scores, len(VALID), THR)


def event_window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    host = (time.perf_counter() - t) * 1e6 / iters
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_ap.md"))
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--scenes", type=int, default=312)
    ap.add_argument("--host-scenes", type=int, default=4)
    ap.add_argument("--iters", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("box_ap_bench: needs a HIP device (there is no CPU path to time)")
    from segdino3d_amd import eval_box
    d = torch.device("cuda:0")
    N, S = args.points, args.scenes
    class_labels = tuple(f"c{i}" for i in VALID)
    rows = []
    for n in (100, 600):
        host = make_scene(N, n, seed=n)
        pts, sem, inst, boxes, labels, scores = (torch.from_numpy(a).to(d) for a in host)
        ann = dict(pts_semantic_mask=sem, pts_instance_mask=inst)
        pred = dict(instance_boxes=boxes, instance_labels=labels, instance_scores=scores)
        new = lambda: eval_box.BoxApAccumulator(VALID, class_labels, iou_thr=THR, device=d)     # noqa: E731  (ids are mapped: no stuff shift)

        # both routes agree on two scenes before anything is timed (id_map of `add` with num_stuff 0 maps index -> id: feed indices)
        ann_idx = dict(pts_semantic_mask=sem - 2, pts_instance_mask=inst)
        acc = new()
        acc.add(ann_idx, pred, pts)
        acc.add(ann_idx, pred, pts)
        ref = host_scene(*host)
        want = R.accumulate([ref, ref], len(VALID))
        e = acc.entries()
        assert e["status"] == want[5] == 0 and np.array_equal(e["group"], want[0]) and np.array_equal(e["true"], want[2])
        assert e["score"].tobytes() == want[1].tobytes() and np.array_equal(e["npos"], want[3])
        got = acc.tables()
        tab = R.finish(want[0], want[1], want[2], want[3], len(THR))
        assert np.allclose(got[0], tab[0], rtol=0, atol=1e-12, equal_nan=True) and np.array_equal(np.nan_to_num(got[1], nan=-1), np.nan_to_num(tab[1], nan=-1))
        n_true = int(e["true"].sum()) // 2

        # per scene, device route
        win = []
        for _ in range(7):
            acc = new()
            acc.add(ann_idx, pred, pts)                                               # constants, first chunk of the store
            win.append(event_window(lambda: acc.add(ann_idx, pred, pts), args.iters))
        t_add, t_add_host = statistics.median(w[0] for w in win), statistics.median(w[1] for w in win)

        # per scene, restatement on the host
        host_scene(*host)
        t = time.perf_counter()
        for _ in range(args.host_scenes):
            host_scene(*host)
        t_host_scene = (time.perf_counter() - t) * 1e6 / args.host_scenes

        # a validation pass
        acc = new()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(S):
            acc.add(ann_idx, pred, pts)
        torch.cuda.synchronize()
        t_pass_add = time.perf_counter() - t
        t_tables = []
        for _ in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            acc.tables()
            t_tables.append(time.perf_counter() - t)
        t = time.perf_counter()
        w = R.accumulate([ref] * S, len(VALID))
        R.finish(w[0], w[1], w[2], w[3], len(THR))
        t_host_finish = time.perf_counter() - t
        rows.append(dict(n=n, true=n_true, slots=acc.used, t_add=t_add, t_add_host=t_add_host, t_host_scene=t_host_scene, t_pass_add=t_pass_add,
                         t_tables=statistics.median(t_tables), t_host_finish=t_host_finish))

    lines = ["# 3D box AP / AR accumulated and scored on the device", "",
             f"`tools/box_ap_bench.py`: N = {N} points, 198 classes, 60 ground-truth instances, thresholds 0.25 / 0.5; device = "
             f"{torch.cuda.get_device_name(0)}.  `add()`: HIP-event time per call in windows of {args.iters} back-to-back calls (median of 7 "
             "windows) and, in brackets, the host's wall time to enqueue one call.  Restatement: `gt_boxes` + `scene` of tests/box_ap_ref.py "
             f"in numpy on host arrays, wall time per scene (mean of {args.host_scenes}).  Microseconds per scene.", "",
             "| predictions | true positives per scene (0.25 + 0.5) | add() | numpy restatement | ratio |", "|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} | {r['true']} | {r['t_add']:.0f} ({r['t_add_host']:.0f}) | {r['t_host_scene']:.0f} | "
                     f"{r['t_host_scene'] / r['t_add']:.0f} x |")
    lines += ["", f"A validation pass of {S} scenes (the same scene {S} times), seconds of wall time: every `add` of the pass and a "
              "synchronisation, then `tables()` (sort + curves + the read-back; median of 3); the restatement is the per-scene time above x "
              f"{S} plus its `accumulate` + `finish` over {S} scene records.", "",
              "| predictions | slots in the store | adds | tables() | device route | restatement, scenes | restatement, accumulate + finish | "
              "restatement | ratio |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        dev_s = r["t_pass_add"] + r["t_tables"]
        host_s = r["t_host_scene"] * S * 1e-6
        lines.append(f"| {r['n']} | {r['slots']} | {r['t_pass_add']:.3f} | {r['t_tables']:.4f} | {dev_s:.3f} | {host_s:.2f} | {r['t_host_finish']:.2f} | "
                     f"{host_s + r['t_host_finish']:.2f} | {(host_s + r['t_host_finish']) / dev_s:.0f} x |")
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
