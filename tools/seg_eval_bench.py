"""Times the device-side semantic / panoptic evaluation (segdino3d_amd/eval_seg.py, csrc/segeval.hip) against the numpy restatement
of the two protocols (tests/segpan_ref.py) on one validation-sized scene: 150 k points, 200 classes + the ignored one, about 60
ground-truth instances and 100 / 600 predicted ones.

    python tools/seg_eval_bench.py [--out profiles/seg_pan_eval.md] [--points 150000] [--iters 50]

Device times are HIP-event times per call (windows of `--iters` back-to-back calls, median of 7 windows after a warm-up), the two kernel
families separately and `add()` as a whole; the restatement is timed with time.perf_counter (median of 3).  Results are checked against the restatement before
anything is timed.  Writes a markdown note."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import segpan_ref as R  # noqa: E402
from segdino3d_amd import eval_seg  # noqa: E402


def edges_of(n, n_runs, g):
    return [0] + np.sort(g.choice(np.arange(1, n), size=n_runs - 1, replace=False)).tolist() + [n]


def make_scene(n, n_classes, n_gt, n_pred, seed=0):
    """Contiguous runs (labels are superpoint-coherent): `n_gt` ground-truth runs, two stuff classes whose id is the class; `n_pred`
    predicted runs that take the class of the ground truth under their first point nine times out of ten."""
    g = np.random.default_rng(seed)
    gs, gi, ps, pi = (np.zeros(n, dtype=np.int64) for _ in range(4))
    nxt = 2
    for lo, hi in zip(*(lambda e: (e[:-1], e[1:]))(edges_of(n, n_gt, g))):
        c = int(g.integers(0, n_classes - 1))
        gs[lo:hi] = c
        gi[lo:hi] = c if c < 2 else nxt
        nxt += c >= 2
    nxt = 2
    for lo, hi in zip(*(lambda e: (e[:-1], e[1:]))(edges_of(n, n_pred, g))):
        c = int(gs[lo]) if g.random() < 0.9 else int(g.integers(0, n_classes - 1))
        ps[lo:hi] = c
        pi[lo:hi] = c if c < 2 else nxt
        nxt += c >= 2
    return gs, gi, ps, pi


def event_times(fn, iters, warmup=5, windows=7):
    """Microseconds per call: `windows` windows of `iters` back-to-back calls, one event pair around each window (the calls queue
    behind one another as they do in an evaluation loop) -> (median, minimum) of window time / iters."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return statistics.median(out), min(out)


def host_time(fn, reps=3):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_pan_eval.md"))
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_eval_bench: needs a HIP device (there is no CPU path to time)")
    d = torch.device("cuda:0")
    C, N = 201, args.points
    rows = []
    for n_pred in (100, 600):
        gs, gi, ps, pi = make_scene(N, C, 60, n_pred, seed=n_pred)
        tg = [torch.from_numpy(a).to(d) for a in (gs, gi, ps, pi)]
        ann = dict(pts_semantic_mask=tg[0], pts_instance_mask=tg[1])
        pred = dict(pts_semantic_mask=[tg[2], tg[2]], pts_instance_mask=[None, tg[3]])
        acc = eval_seg.SegPanAccumulator(C, [C - 1], [0, 1], list(range(2, C - 1)), 1)
        acc.add(ann, pred)
        got = acc.counts()
        conf = R.confusion([gs], [ps], C, C - 1)
        tp, fp, fn, iou, n_m = R.panoptic_counts([gs], [gi], [ps], [pi], C, [C - 1], 1)
        assert np.array_equal(got["confusion"], conf) and np.array_equal(got["tp"], tp) and np.array_equal(got["fp"], fp)
        assert np.array_equal(got["fn"], fn) and np.all(np.abs(got["iou_sum"] - iou) <= max(n_m, 1) * 2.0 ** -52 * np.abs(iou))
        t_sem, t_sem_min = event_times(lambda: acc.add_semantic(tg[2], tg[0]), args.iters)
        t_pan, t_pan_min = event_times(lambda: acc.add_panoptic(tg[2], tg[3], tg[0], tg[1]), args.iters)
        t_add, t_add_min = event_times(lambda: acc.add(ann, pred), args.iters)
        h_sem = host_time(lambda: R.confusion([gs], [ps], C, C - 1))
        h_pan = host_time(lambda: R.panoptic_counts([gs], [gi], [ps], [pi], C, [C - 1], 1))
        rows.append(dict(n_pred=n_pred, gt_seg=int(len(np.unique(gi[gi >= 0]))), pred_seg=int(len(np.unique(pi[pi >= 0]))), tp=int(tp.sum()),
                         fp=int(fp.sum()), fn=int(fn.sum()), t_sem=t_sem, t_sem_min=t_sem_min, t_pan=t_pan, t_pan_min=t_pan_min, t_add=t_add,
                         t_add_min=t_add_min, h_sem=h_sem * 1e6, h_pan=h_pan * 1e6))
    lines = ["# Semantic / panoptic evaluation on the device: one scene", "",
             f"`tools/seg_eval_bench.py`: N = {N} points, C = {C} classes (the last ignored), 60 ground-truth runs; device = "
             f"{torch.cuda.get_device_name(0)}; HIP-event time per call in windows of {args.iters} back-to-back calls, median (minimum) of 7 "
             "windows; host = numpy restatement "
             "(tests/segpan_ref.py), median of 3.  All times in microseconds per scene.", "",
             "| predicted runs | gt / pred segments | tp / fp / fn | confusion (device) | panoptic (device) | add() (device) | confusion (numpy) | panoptic (numpy) | numpy / add() |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n_pred']} | {r['gt_seg']} / {r['pred_seg']} | {r['tp']} / {r['fp']} / {r['fn']} | {r['t_sem']:.1f} ({r['t_sem_min']:.1f}) | "
                     f"{r['t_pan']:.1f} ({r['t_pan_min']:.1f}) | {r['t_add']:.1f} ({r['t_add_min']:.1f}) | {r['h_sem']:.0f} | {r['h_pan']:.0f} | "
                     f"{(r['h_sem'] + r['h_pan']) / r['t_add']:.0f} x |")
    lines.append("")
    lines.append("The device columns are the time per call in a queue of calls, the host's enqueue included (what a scene costs inside an "
                 "evaluation loop).  `add()` enqueues eight kernels and one fill; a kernel trace gives the kernels alone.")
    lines.append("")
    for r in rows:
        lines.append(f"Confusion call, {r['n_pred']} predicted runs: against the 4 x 8 x N = {32 * N} bytes of label arrays a scene brings "
                     f"(the confusion kernel itself reads two of the four, {16 * N} bytes), {r['t_sem']:.1f} us per call are "
                     f"{32 * N / r['t_sem'] / 1e3:.0f} GB/s ({16 * N / r['t_sem'] / 1e3:.0f} GB/s of bytes actually read).")
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
