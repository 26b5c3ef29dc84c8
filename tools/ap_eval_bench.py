"""Times the streamed instance AP (`eval_ap.ApAccumulator`, csrc/apeval.hip) against the host route it stands next to (`rename_gt` +
`assign_scene` per scene, `evaluate_records` at the end) on the scene of tests/perf_ap.py: 150 k points, about 60 ground-truth instances
of a 198-class label set, 100 / 600 predictions that each cover most of one instance plus noise.

    python tools/ap_eval_bench.py [--out profiles/ap_eval.md] [--points 150000] [--scenes 312] [--host-scenes 16]

Per scene: `add_scene()` in a queue of calls (HIP events around windows of back-to-back calls, and the host's wall time to enqueue
them), the C entry `ops.ap_scene` alone in the same way (no store growth, no argument handling), and the host route's `rename_gt` +
`assign_scene` (wall time; it synchronises).  Per validation pass: `--scenes` scenes into one accumulator and `tables()` (wall time
with a synchronisation on either side) against `evaluate_records` over `--host-scenes` records, extrapolated linearly to `--scenes`
(it is linear in the records; the full pass takes tens of seconds on one core).  The tables of both routes are compared before
anything is timed.  Writes a markdown note."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from segdino3d_amd import eval_ap, ops  # noqa: E402


def make_scene(N, n, n_inst=60, seed=0):
    gen = torch.Generator().manual_seed(seed)
    valid = tuple(range(2, 200))
    owner = torch.randint(0, n_inst, (N,), generator=gen)
    sem = torch.randint(0, 200, (n_inst,), generator=gen)
    masks = torch.zeros(n, N, dtype=torch.bool)
    for p in range(n):
        o = int(torch.randint(0, n_inst, (1,), generator=gen))
        masks[p] = ((owner == o) & (torch.rand(N, generator=gen) > 0.2)) | (torch.rand(N, generator=gen) > 0.995)
    labels = torch.tensor([max(0, min(len(valid) - 1, int(sem[int(torch.randint(0, n_inst, (1,), generator=gen))]) - 2)) for _ in range(n)])
    scores = torch.rand(n, generator=gen)
    return valid, sem[owner], owner, masks, labels, scores


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ap_eval.md"))
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--scenes", type=int, default=312)
    ap.add_argument("--host-scenes", type=int, default=16)
    ap.add_argument("--iters", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ap_eval_bench: needs a HIP device (there is no CPU path to time)")
    d = torch.device("cuda:0")
    N = args.points
    opts = eval_ap.get_options(None)
    rows = []
    for n in (100, 600):
        valid, sem, inst, masks, labels, scores = make_scene(N, n, seed=n)
        class_labels = tuple(f"c{i}" for i in valid)
        sem, inst, masks, labels, scores = (t.to(d) for t in (sem, inst, masks, labels, scores))
        new = lambda: eval_ap.ApAccumulator(valid, class_labels, device=d)       # noqa: E731

        def host_scene():
            return eval_ap.assign_scene(masks, labels, scores, eval_ap.rename_gt([sem], [inst], valid)[0], opts, valid)

        # both routes agree on two scenes before anything is timed
        acc = new()
        acc.add_scene(sem, inst, masks, labels, scores)
        acc.add_scene(sem, inst, masks, labels, scores)
        got = acc.tables()
        rec = host_scene()
        want = eval_ap.evaluate_records([rec, rec], class_labels, valid, opts)
        assert np.allclose(got[0], want[0], rtol=0, atol=1e-12, equal_nan=True) and np.allclose(got[1], want[1], rtol=0, atol=1e-12, equal_nan=True)
        n_entries = len(acc.entries()["group"]) // 2

        # per scene, device route
        win = []
        for _ in range(7):
            acc = new()
            acc.add_scene(sem, inst, masks, labels, scores)                       # constants, first chunk of the store
            win.append(event_window(lambda: acc.add_scene(sem, inst, masks, labels, scores), args.iters))
        t_add, t_add_host = statistics.median(w[0] for w in win), statistics.median(w[1] for w in win)
        acc = new()
        acc.add_scene(sem, inst, masks, labels, scores)
        v = acc._views(acc._counters)
        m8 = masks.view(torch.uint8)

        def entry():
            ops.ap_scene(sem, inst, m8, labels, scores, acc._const["lut"], acc.zero_class, acc.n_classes, acc._const["overlaps"], acc.slots,
                         acc.min_region, acc._store, 0, n * acc.slots_per_pred, v["hard_fn"], v["has_gt"], v["has_pred"], v["status"])
        entry()
        win = [event_window(entry, args.iters) for _ in range(7)]
        t_entry, t_entry_host = statistics.median(w[0] for w in win), statistics.median(w[1] for w in win)

        # per scene, host route (synchronises by itself)
        for _ in range(3):
            host_scene()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(10):
            host_scene()
        t_assign = (time.perf_counter() - t) * 1e6 / 10

        # a validation pass
        acc = new()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(args.scenes):
            acc.add_scene(sem, inst, masks, labels, scores)
        torch.cuda.synchronize()
        t_pass_add = time.perf_counter() - t
        t_tables = []
        for _ in range(3):
            torch.cuda.synchronize()
            t = time.perf_counter()
            acc.tables()
            t_tables.append(time.perf_counter() - t)
        recs = [rec] * args.host_scenes
        t = time.perf_counter()
        eval_ap.evaluate_records(recs, class_labels, valid, opts)
        t_records = (time.perf_counter() - t) * args.scenes / args.host_scenes
        rows.append(dict(n=n, entries=n_entries, slots=acc.used, t_add=t_add, t_add_host=t_add_host, t_entry=t_entry, t_entry_host=t_entry_host,
                         t_assign=t_assign, t_pass_add=t_pass_add, t_tables=statistics.median(t_tables), t_records=t_records))

    S = args.scenes
    lines = ["# Instance AP accumulated and scored on the device", "",
             f"`tools/ap_eval_bench.py`: N = {N} points, 198 classes, 60 ground-truth instances, 10 overlaps, min_region 100; device = "
             f"{torch.cuda.get_device_name(0)}.  Device columns: HIP-event time per call in windows of {args.iters} back-to-back calls "
             "(median of 7 windows) and, in brackets, the host's wall time to enqueue one call.  `assign_scene` (with `rename_gt`): wall "
             "time per scene, it synchronises.  Microseconds per scene.", "",
             "| predictions | entries per scene | add_scene() | ops.ap_scene alone | rename_gt + assign_scene (host route) |",
             "|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']} | {r['entries']} | {r['t_add']:.0f} ({r['t_add_host']:.0f}) | {r['t_entry']:.0f} ({r['t_entry_host']:.0f}) | "
                     f"{r['t_assign']:.0f} |")
    lines += ["", f"A validation pass of {S} scenes (the same scene {S} times), seconds of wall time: every `add_scene` of the pass and a "
              f"synchronisation, then `tables()` (sort + curves + the read-back; median of 3); the host route is {S} x the per-scene time "
              f"above plus `evaluate_records`, which was timed over {args.host_scenes} records and extrapolated linearly to {S}.", "",
              "| predictions | slots in the store | adds, device route | tables() | device route | assign_scene x scenes | evaluate_records | host route |",
              "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        host_assign = r["t_assign"] * S * 1e-6
        lines.append(f"| {r['n']} | {r['slots']} | {r['t_pass_add']:.3f} | {r['t_tables']:.3f} | {r['t_pass_add'] + r['t_tables']:.3f} | "
                     f"{host_assign:.3f} | {r['t_records']:.1f} | {host_assign + r['t_records']:.1f} |")
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
