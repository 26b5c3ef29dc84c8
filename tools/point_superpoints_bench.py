"""Times the superpoints of a point cloud (`superpoints.point_superpoints`, csrc/superpoints.hip) on seeded synthetic clouds of real
size, no files: the vertices of the jittered height field with raised boxes of tests/superpoints_case.py at `--grid` x `--grid` points
(388: 150 544 points, the cloud of the mesh `tools/superpoints_bench.py` times), alone and as a batch of `--batch` clouds with
different seeds, `k = 16`, `radius = 0.1`.

    python tools/point_superpoints_bench.py [--grid 388] [--batch 32] [--reps 10] [--no-baseline] [--out profiles/point_superpoints.json]

Reports, by HIP events around single calls (medians over `--reps` after warm-up): the k-NN graph, the normals, the segmentation of the
graph with and without pass 2 (`min_verts = 1` launches pass 1 only, so the difference is the candidates and the sweep of pass 2), the
whole chain for one cloud and for the batch; the distance evaluations of the 27-cell search counted on the host from the rule's cells
(points hashed into a searched bucket from elsewhere add to them) and their rate; and two baselines: the restatement
tests/point_superpoints_ref.py on the host (brute force for `--sample` rows, scaled to all rows and said so; normals and the
segmentation in full) and, for the k-NN stage, `torch.cdist` + `topk` in chunks on the same device.  The kernels must equal the
restatement wherever it was computed, or nothing is timed.  Per-kernel times (grid build against search, weights and sort against the
sweeps) come from a kernel trace of this tool (`tools/profile_cmd.sh point_superpoints tools/point_superpoints_bench.py --no-baseline
--reps 3`)."""
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

import point_superpoints_ref as P  # noqa: E402
import superpoints_case as K  # noqa: E402


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


def evaluations_in_27_cells(p, radius):
    """The points in the 27 cells around every valid point's own, by the rule's fixed-point cells (host, integers)."""
    h = int(np.ceil(np.float32(radius) * np.float32(1024.0))) + 2
    cell = (np.rint(p * np.float32(1024.0)).astype(np.int64) + (1 << 24)) // h + 1
    assert cell.max() < (1 << 20) - 1
    key = (cell[:, 0] << 40) | (cell[:, 1] << 20) | cell[:, 2]
    uniq, count = np.unique(key, return_counts=True)
    total = 0
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                q = key + (dx << 40) + (dy << 20) + dz
                at = np.minimum(np.searchsorted(uniq, q), len(uniq) - 1)
                total += int(count[at][uniq[at] == q].sum())
    return total, len(uniq)


def cdist_topk(p, k, radius, chunk):
    """The torch formulation of the k-NN stage: distances of a chunk of rows to every point, the k + 1 smallest, the point itself and
    everything beyond the radius dropped.  Not the rule (other rounding, other ties): a timing baseline only."""
    out = torch.empty(p.shape[0], k, dtype=torch.int32, device=p.device)
    for s in range(0, p.shape[0], chunk):
        d, j = torch.cdist(p[s:s + chunk], p).topk(k + 1, dim=1, largest=False)
        out[s:s + chunk] = torch.where(d[:, 1:] <= radius, j[:, 1:], -1).to(torch.int32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=388)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--radius", type=float, default=0.1)
    ap.add_argument("--sample", type=int, default=1024, help="rows of the brute-force restatement")
    ap.add_argument("--chunk", type=int, default=4096, help="rows per torch.cdist call")
    ap.add_argument("--no-baseline", action="store_true", help="kernels only (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_superpoints.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("point_superpoints_bench: needs a HIP device (a measurement does not fall back to the CPU)")
    from segdino3d_amd import superpoints
    d = torch.device("cuda:0")
    k, radius = args.k, args.radius
    host = [np.ascontiguousarray(K.height_field(args.grid, seed)[0], dtype=np.float32) for seed in range(max(1, args.batch))]
    clouds = [torch.from_numpy(p).to(d) for p in host]
    p = clouds[0]
    N = p.shape[0]
    res = dict(device=torch.cuda.get_device_name(0), grid=args.grid, points=N, k=k, radius=radius, edges=N * k, batch=len(clouds))

    labels, info = superpoints.point_superpoints(p, k=k, radius=radius, debug=True)
    nbr, normals = info.nbr, info.normals
    edges = torch.stack([torch.arange(N, device=d).repeat_interleave(k), nbr.reshape(-1).long()], dim=1)
    settled = info.settled.tolist()
    evals, cells = evaluations_in_27_cells(host[0], radius)
    res["single"] = dict(superpoints=info.count, bad_edges=info.bad_edges, live_edges=N * k - info.bad_edges, occupied_cells=cells,
                         distance_evaluations_27_cells=evals, evaluations_per_point=evals / N,
                         settled_in_lds_pass1=settled[0], settled_in_lds_pass2=settled[1], settled_share_pass1=settled[0] / (N * k),
                         smallest_superpoint=int(torch.bincount(labels).min()))
    if not args.no_baseline:
        rows = np.random.default_rng(0).choice(N, size=min(args.sample, N), replace=False)
        t0 = time.perf_counter()
        keys = np.concatenate([np.sort(P.knn_keys(host[0], rows[s:s + 128], radius), axis=1)[:, :k] for s in range(0, len(rows), 128)])
        t_knn = (time.perf_counter() - t0) * 1e3
        want = np.where(keys != P.NO_KEY, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
        nbr_h = nbr.cpu().numpy()
        t0 = time.perf_counter()
        want_normals = P.estimate_normals(host[0], nbr_h)
        t_normals = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ref = P.graph_superpoints(host[0], want_normals, P.knn_edges(nbr_h), oriented=False, debug=True)
        t_graph = (time.perf_counter() - t0) * 1e3
        cmp_ = dict(knn_rows_compared=len(rows), neighbours_differing=int((nbr_h[rows] != want).sum()),
                    normal_components_differing=int((normals.cpu().numpy().view(np.uint32) != want_normals.view(np.uint32)).sum()),
                    weights_differing=int((info.weights.cpu().numpy().view(np.uint32) != ref.weights).sum()),
                    labels_differing=int((labels.cpu().numpy() != ref.labels).sum()), count_equal=info.count == ref.count)
        res["against_restatement"] = cmp_
        res["restatement_on_host_ms"] = dict(knn_sample_rows=len(rows), knn_sample=t_knn, knn_scaled_to_all_rows=t_knn * N / len(rows),
                                             normals=t_normals, graph=t_graph)
        print(json.dumps(dict(against_restatement=cmp_, restatement_on_host_ms=res["restatement_on_host_ms"])), flush=True)
        if any(cmp_[x] for x in ("neighbours_differing", "normal_components_differing", "weights_differing", "labels_differing")) \
                or not cmp_["count_equal"]:
            raise SystemExit("point_superpoints_bench: the kernels differ from the restatement; nothing is timed")
    s = res["single"]
    s["knn_graph"] = timed(lambda: superpoints.knn_graph(p, k=k, radius=radius), args.reps)
    s["estimate_normals"] = timed(lambda: superpoints.estimate_normals(p, nbr), args.reps)
    s["graph_superpoints"] = timed(lambda: superpoints.graph_superpoints(p, normals, edges, oriented=False), args.reps)
    s["graph_superpoints_pass1_only"] = timed(lambda: superpoints.graph_superpoints(p, normals, edges, oriented=False, min_verts=1), args.reps)
    s["chain"] = timed(lambda: superpoints.point_superpoints(p, k=k, radius=radius), args.reps)
    s["with_host_read"] = timed(lambda: superpoints.point_superpoints(p, k=k, radius=radius, return_info=True), args.reps)
    # what the mirrored copy of a mutual edge costs (the rule keeps both; not the rule's result): edge (i, j), i > j, dropped where
    # row j holds i, and the same call timed on the shorter list
    i_, j_ = edges[:, 0], edges[:, 1]
    mirrored = (j_ >= 0) & (i_ > j_) & (nbr[j_.clamp(min=0)] == i_[:, None]).any(dim=1)
    fewer = edges[~mirrored].contiguous()
    s["mutual_edge_copies"] = int(mirrored.sum())
    s["graph_superpoints_without_mirrored_copies"] = timed(lambda: superpoints.graph_superpoints(p, normals, fewer, oriented=False), args.reps)
    s["mirrored_copies_share_of_graph_time"] = 1.0 - s["graph_superpoints_without_mirrored_copies"]["median_ms"] / s["graph_superpoints"]["median_ms"]
    s["evaluations_per_second_knn_stage"] = evals / (s["knn_graph"]["median_ms"] * 1e-3)
    s["graph_share_of_chain"] = s["graph_superpoints"]["median_ms"] / s["chain"]["median_ms"]
    if not args.no_baseline:
        got = cdist_topk(p, k, radius, args.chunk)
        s["cdist_topk"] = timed(lambda: cdist_topk(p, k, radius, args.chunk), max(3, args.reps // 2), warmup=1)
        s["cdist_topk"]["rows_with_the_same_neighbour_set"] = int((got.sort(dim=1).values == nbr.sort(dim=1).values).all(dim=1).sum())
        s["cdist_topk_over_knn_graph"] = s["cdist_topk"]["median_ms"] / s["knn_graph"]["median_ms"]
    print(json.dumps(dict(single=s)), flush=True)

    if len(clouds) > 1:
        b_labels, b_infos = superpoints.point_superpoints_batch(clouds, k=k, radius=radius, debug=True)
        same = torch.equal(b_labels[0], labels) and all(torch.equal(b_labels[i], superpoints.point_superpoints(clouds[i], k=k, radius=radius))
                                                        for i in (1, len(clouds) - 1))
        if not same:
            raise SystemExit("point_superpoints_bench: a scene of the batch differs from its single run; nothing is timed")
        b = res["batched"] = dict(scenes=len(clouds), superpoints=[i.count for i in b_infos], equals_single_runs=True)
        b["chain"] = timed(lambda: superpoints.point_superpoints_batch(clouds, k=k, radius=radius), max(3, args.reps // 2), warmup=1)
        b["ms_per_scene"] = b["chain"]["median_ms"] / len(clouds)
        b["single_over_batched_per_scene"] = s["chain"]["median_ms"] / b["ms_per_scene"]
        print(json.dumps(dict(batched=b)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
