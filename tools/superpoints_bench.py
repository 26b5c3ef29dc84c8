"""Times the superpoint segmentation of a mesh (`superpoints.mesh_superpoints`, csrc/superpoints.hip) on seeded synthetic meshes of real
size, no files: the jittered height field with raised boxes of tests/superpoints_case.py at `--grid` x `--grid` vertices (388: 150 544
vertices, 299 538 faces, 898 614 edges - a ScanNet `_vh_clean_2` scan), alone and as a batch of `--batch` such meshes with different seeds.

    python tools/superpoints_bench.py [--grid 388] [--batch 32] [--reps 10] [--no-baseline] [--out profiles/superpoints.json]

Reports, by HIP events around a queue of calls (medians over `--reps`): the whole launch chain for one mesh and for the batch, the same
with the host read of {superpoints, ignored faces}, the superpoint counts, the edges the sweep settled in its LDS table (those whose
ends lay in different components when their batch of 512 began) as a share of all edges, and - the only comparison there is, never
a kernel - the restatement tests/superpoints_ref.py on the host for the same mesh, whose labels, vertex normals and edge-weight bits must
equal the kernels' (nothing is timed if they do not).  The chain is one C call: per-kernel times come from a kernel trace of this tool
(`tools/profile_cmd.sh superpoints tools/superpoints_bench.py --no-baseline --reps 3`)."""
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

import superpoints_case as K  # noqa: E402
import superpoints_ref as R  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=388)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-baseline", action="store_true", help="kernels only (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "superpoints.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("superpoints_bench: needs a HIP device (a measurement does not fall back to the CPU)")
    from segdino3d_amd import superpoints
    d = torch.device("cuda:0")
    host = [K.height_field(args.grid, seed) for seed in range(max(1, args.batch))]
    meshes = [(torch.from_numpy(v).to(d), torch.from_numpy(f).to(d)) for v, f in host]
    v, f = meshes[0]
    N, F = v.shape[0], f.shape[0]
    res = dict(device=torch.cuda.get_device_name(0), grid=args.grid, vertices=N, faces=F, edges=3 * F, batch=len(meshes))

    labels, info = superpoints.mesh_superpoints(v, f, debug=True)
    settled = info.settled.tolist()
    res["single"] = dict(superpoints=info.count, bad_faces=info.bad_faces, settled_in_lds_pass1=settled[0], settled_in_lds_pass2=settled[1],
                         settled_share_pass1=settled[0] / (3 * F), settled_share_pass2=settled[1] / (3 * F),
                         smallest_superpoint=int(torch.bincount(labels).min()))
    if not args.no_baseline:
        t0 = time.perf_counter()
        ref = R.mesh_superpoints(host[0][0], host[0][1], debug=True)
        res["restatement_on_host_ms"] = (time.perf_counter() - t0) * 1e3
        cmp_ = dict(normal_components_differing=int((info.normals.cpu().numpy().view(np.uint32) != ref.normals.view(np.uint32)).sum()),
                    weights_differing=int((info.weights.cpu().numpy().view(np.uint32) != ref.weights).sum()),
                    labels_differing=int((labels.cpu().numpy() != ref.labels).sum()), count_equal=info.count == ref.count)
        res["against_restatement"] = cmp_
        print(json.dumps(dict(against_restatement=cmp_, restatement_on_host_ms=res["restatement_on_host_ms"])), flush=True)
        if cmp_["normal_components_differing"] or cmp_["weights_differing"] or cmp_["labels_differing"] or not cmp_["count_equal"]:
            raise SystemExit("superpoints_bench: the kernels differ from the restatement; nothing is timed")
    res["single"]["chain"] = timed(lambda: superpoints.mesh_superpoints(v, f), args.reps)
    res["single"]["with_host_read"] = timed(lambda: superpoints.mesh_superpoints(v, f, return_info=True), args.reps)
    res["single"]["edges_per_second_whole_chain"] = 3 * F / (res["single"]["chain"]["median_ms"] * 1e-3)
    print(json.dumps(dict(single=res["single"])), flush=True)

    if len(meshes) > 1:
        b_labels, b_infos = superpoints.mesh_superpoints_batch(meshes, debug=True)
        same = torch.equal(b_labels[0], labels) and all(torch.equal(b_labels[i], superpoints.mesh_superpoints(*meshes[i]))
                                                        for i in (1, len(meshes) - 1))
        if not same:
            raise SystemExit("superpoints_bench: a scene of the batch differs from its single run; nothing is timed")
        tot1, tot2 = sum(int(i.settled[0]) for i in b_infos), sum(int(i.settled[1]) for i in b_infos)
        res["batched"] = dict(scenes=len(meshes), superpoints=[i.count for i in b_infos], equals_single_runs=True,
                              settled_share_pass1=tot1 / (3 * F * len(meshes)), settled_share_pass2=tot2 / (3 * F * len(meshes)))
        res["batched"]["chain"] = timed(lambda: superpoints.mesh_superpoints_batch(meshes), max(3, args.reps // 2), warmup=1)
        res["batched"]["with_host_read"] = timed(lambda: superpoints.mesh_superpoints_batch(meshes, return_info=True), max(3, args.reps // 2),
                                                 warmup=1)
        res["batched"]["ms_per_scene"] = res["batched"]["chain"]["median_ms"] / len(meshes)
        res["batched"]["edges_per_second_whole_chain"] = 3 * F * len(meshes) / (res["batched"]["chain"]["median_ms"] * 1e-3)
        res["batched"]["single_over_batched_per_scene"] = res["single"]["chain"]["median_ms"] / res["batched"]["ms_per_scene"]
        print(json.dumps(dict(batched=res["batched"])), flush=True)
    if not args.no_baseline:
        res["host_restatement_over_single_chain"] = res["restatement_on_host_ms"] / res["single"]["chain"]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
