"""Benchmark submission export (segdino3d_amd/submission.py, csrc/submit.hip) on scenes of real size:
python tools/submission_bench.py [--points 150000] [--instances 100,600] [--reps 5] [--writers 4] [--dir DIR] [--runner-scenes 12]
python tools/submission_bench.py --reference-route [--points 150000] [--instances 100,600] [--workers 16] [--dir DIR]

Per scene of `--points` points and each instance count (random masks, ScanNet200-like id tables):
  (a) the two kernels, HIP events: `ops.mask_text` over all rows, `ops.label_text` over the points;
  (b) the device -> pinned copy of that text, HIP events;
  (c) `SubmissionWriter` (instance + semantic tree) into a fresh temporary directory, a fresh writer per repetition, host clock from
      its construction to the end of `close()` (every file written), and to the return of `add`; one untimed writer first, so the
      pinned blocks come from the host allocator's cache;
  (d) the floor: the same bytes written to the same kind of directory from ordinary host memory by the same number of threads, no GPU
      work inside the timed region;
  (e) `PipelinedRunner` evaluation scenes/s on the structured synthetic scene with and without the writer attached, alternating.
`--reference-route` is a run of its own that never opens the GPU (it forks workers): `np.savetxt(path, mask, fmt='%d')` per mask
through a process pool of at most 16 workers, as the reference's save_pred_instances does with `mp.Pool()`.
Every temporary directory is removed.  One JSON line; every repetition is kept as median / min / max."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs, unit="ms"):
    return {f"median_{unit}": round(statistics.median(xs), 4), f"min_{unit}": round(min(xs), 4), f"max_{unit}": round(max(xs), 4), "reps": len(xs)}


def _savetxt_mask(path, mask):
    np.savetxt(path, mask, fmt="%d")


def reference_route(a):
    """No torch, no GPU: the reference's per-mask np.savetxt through a process pool."""
    import multiprocessing as mp
    workers = min(16, a.workers)
    result = dict(route="np.savetxt per mask, process pool", workers=workers, points=a.points)
    g = np.random.default_rng(0)
    for n in a.instances:
        masks = g.random((n, a.points)) < g.random((n, 1))
        times = []
        for _ in range(a.ref_reps):
            tmp = tempfile.mkdtemp(dir=a.dir)
            try:
                t0 = time.perf_counter()
                with mp.Pool(workers) as pool:
                    pool.starmap(_savetxt_mask, [(os.path.join(tmp, f"m_{i:03d}.txt"), masks[i]) for i in range(n)])
                times.append(time.perf_counter() - t0)
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
        t0 = time.perf_counter()
        f = os.path.join(tempfile.gettempdir(), f"sd3d_one_mask_{os.getpid()}.txt")
        _savetxt_mask(f, masks[0])
        one = time.perf_counter() - t0
        os.remove(f)
        result[f"instances_{n}"] = dict(wall=stats(times, "s"), one_mask_one_core_s=round(one, 4))
    print(json.dumps(result))


def floor_write(root, sid, mask_rows, nbytes, sem_text, index, writers):
    """The same files from ordinary host memory, `writers` threads."""
    os.makedirs(os.path.join(root, "inst", "predicted_masks"))
    os.makedirs(os.path.join(root, "sem"))
    jobs = [(os.path.join(root, "inst", "predicted_masks", f"{sid}_{i:03d}.txt"), mask_rows[i, :nbytes].data) for i in range(len(mask_rows))]
    jobs += [(os.path.join(root, "sem", f"{sid}.txt"), sem_text.data), (os.path.join(root, "inst", f"{sid}.txt"), index)]

    def work(k):
        for path, data in jobs[k::writers]:
            with open(path, "wb") as f:
                f.write(data)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(writers)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150_000)
    ap.add_argument("--instances", type=lambda s: [int(x) for x in s.split(",")], default=[100, 600])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--ref-reps", type=int, default=2)
    ap.add_argument("--writers", type=int, default=4)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--dir", default=None, help="where the temporary directories are made (default: the system's)")
    ap.add_argument("--runner-scenes", type=int, default=12, help="scenes per PipelinedRunner run (0: skip)")
    ap.add_argument("--runner-points", type=int, default=150_000)
    ap.add_argument("--reference-route", action="store_true")
    a = ap.parse_args()
    if a.reference_route:
        return reference_route(a)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("submission_bench: needs a HIP device (a measurement does not fall back to the CPU)")
    from segdino3d_amd import ops, submission
    d = torch.device("cuda:0")
    g = np.random.default_rng(0)
    inst_mapping = np.sort(g.choice(np.arange(1, 1192), size=198, replace=False))
    sem_mapping = np.sort(g.choice(np.arange(1, 1192), size=200, replace=False))
    sem = torch.from_numpy(g.integers(0, 200, size=a.points)).to(d)
    table = ops.LabelTable(sem_mapping, d)
    tmp_root = tempfile.mkdtemp(dir=a.dir)
    result = dict(points=a.points, writers=a.writers, directory=os.path.abspath(tmp_root).split(os.sep)[1])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn, reps):
        out = []
        for it in range(3 + reps):
            torch.cuda.synchronize()
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            if it >= 3:
                out.append(ev[0].elapsed_time(ev[1]))
        return out

    try:
        t_label = timed(lambda: ops.label_text(sem, table), a.kernel_reps)
        sem_text, info = ops.label_text(sem, table)
        sem_len = int(info.cpu()[0])
        result["label_text_kernels"] = dict(stats(t_label), text_bytes=sem_len)
        for n in a.instances:
            masks = torch.from_numpy((g.random((n, a.points)) < g.random((n, 1))).astype(np.uint8)).to(d)
            labels = torch.from_numpy(g.integers(0, 198, size=n)).to(d)
            scores = torch.from_numpy(g.random(n).astype(np.float32)).to(d)
            pred = dict(pts_instance_mask=[masks], pts_semantic_mask=[sem], instance_labels=labels, instance_scores=scores)
            r = dict(text_bytes=2 * a.points * n + sem_len)
            r["mask_text_kernel"] = stats(timed(lambda: ops.mask_text(masks), a.kernel_reps))
            text = ops.mask_text(masks)
            pinned = torch.empty(text.shape, dtype=torch.uint8, pin_memory=True)
            r["copy_to_pinned"] = stats(timed(lambda: pinned.copy_(text, non_blocking=True), a.kernel_reps))
            host_rows = np.array(pinned.numpy(), copy=True)                   # ordinary host memory for the floor
            host_sem = np.array(sem_text[:sem_len].cpu().numpy(), copy=True)
            index = submission.index_text("scene0000_00", labels.cpu().numpy(), scores.cpu().numpy(), inst_mapping)
            del text, pinned
            odd = masks[:, :a.points - 1].contiguous()                        # rows that start off an 8-byte boundary: byte loads
            r["mask_text_kernel_points_minus_1"] = stats(timed(lambda: ops.mask_text(odd), a.kernel_reps))
            del odd
            wall, issue, floor = [], [], []

            def export(root):
                """A fresh writer per scene: construction, `add` (returns once everything is queued on the stream), close."""
                t0 = time.perf_counter()
                with submission.SubmissionWriter(os.path.join(root, "inst"), os.path.join(root, "sem"), inst_mapping, sem_mapping,
                                                 writers=a.writers) as w:
                    w.add("scene0000_00", pred)
                    t1 = time.perf_counter()
                return 1e3 * (time.perf_counter() - t0), 1e3 * (t1 - t0)

            export(os.path.join(tmp_root, "warm"))        # untimed: the host allocator keeps the pinned blocks for the writers below
            shutil.rmtree(os.path.join(tmp_root, "warm"))
            for it in range(a.reps):                      # the writer and the floor alternate
                root = os.path.join(tmp_root, f"w{n}_{it}")
                torch.cuda.synchronize()
                ms, ms_add = export(root)
                wall.append(ms)
                issue.append(ms_add)
                shutil.rmtree(root)
                root = os.path.join(tmp_root, f"f{n}_{it}")
                t0 = time.perf_counter()
                floor_write(root, "scene0000_00", host_rows, 2 * a.points, host_sem, index, a.writers)
                floor.append(1e3 * (time.perf_counter() - t0))
                shutil.rmtree(root)
            r["writer_add_returns"] = stats(issue)
            r["writer_wall"], r["floor_wall"] = stats(wall), stats(floor)
            r["writer_over_floor"] = round(statistics.median(wall) / statistics.median(floor), 3)
            result[f"instances_{n}"] = r
            del masks, host_rows
        if a.runner_scenes > 0:
            result["runner"] = runner_rates(a, d, tmp_root, inst_mapping, sem_mapping)
    finally:
        shutil.rmtree(tmp_root, ignore_errors=True)
    print(json.dumps(result))


def runner_rates(a, d, tmp_root, inst_mapping, sem_mapping):
    import copy
    import torch
    import segdino3d_amd as seg
    from segdino3d_amd import submission
    from segdino3d_amd.configs import scannet200_model_cfg
    from segdino3d_amd.dist_eval import PipelinedRunner
    from segdino3d_amd.synth import make_scene, sharpen_random_model, structure_scene
    pts, tgt = make_scene(1, n_points=a.runner_points, n_superpoints=3000, n_query2d=300)
    structure_scene(pts, tgt)
    torch.manual_seed(0)
    model = sharpen_random_model(seg.build_architecture(scannet200_model_cfg(query_num=-1)).eval()).to(d)
    model.to_host = False
    scenes = [(pts.to(d), copy.copy(tgt).to(d)) for _ in range(a.runner_scenes)]
    ids = [f"scene{i:04d}_00" for i in range(a.runner_scenes)]
    runner = PipelinedRunner(model, n_streams=2)
    counts = []
    runner.run(scenes[:4], on_result=lambda i, r: counts.append(int(r[0].pred_pts_seg.pts_instance_mask[0].shape[0])), keep=False)
    rates = {"plain": [], "with_writer": []}
    for it in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        runner.run(scenes, keep=False)
        torch.cuda.synchronize()
        rates["plain"].append(len(scenes) / (time.perf_counter() - t0))
        root = os.path.join(tmp_root, f"r{it}")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with submission.SubmissionWriter(os.path.join(root, "inst"), os.path.join(root, "sem"), inst_mapping, sem_mapping, writers=a.writers) as w:
            runner.run(scenes, on_result=w.on_result(ids), keep=False)
        rates["with_writer"].append(len(scenes) / (time.perf_counter() - t0))
        shutil.rmtree(root)
    return dict(points=a.runner_points, scenes=len(scenes), instances_per_scene=counts[0], streams=2,
                scenes_per_s={k: stats(v, "per_s") for k, v in rates.items()})


if __name__ == "__main__":
    main()
