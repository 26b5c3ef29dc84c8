"""Times connected components and the clean (`segdino3d_amd/components.py`, csrc/components.hip) on a synthetic scene of real size, no
files: the closed-form room of tests/fuse_views_case.py scaled to a ScanNet-sized room, 64 distinct views of 480 x 640 (the 256-view
fusion repeats them four times), fused by `tsdf.TsdfVolume` at 2 cm into the room mesh of tools/simplify_bench.py and by `fuse_views`
into the cloud of tools/transfer_bench.py, each with planted debris: floating triangles, fans of 19 vertices and grids of 40.

    python tools/components_bench.py [--views 256] [--reps 5] [--out profiles/mesh_components.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/components_bench.py --trace-run --reps 3      # a run of its own
    python tools/components_bench.py --stages-from DIR/.../kernel_trace.csv --reps 3 --out profiles/mesh_components_stages.json

The first form reports (HIP events around the call, the one host read included; warm-up, then `--reps` runs: median, min, max):
`clean_mesh` on the room with debris and the table form on the cloud at k = 16, whether the outputs equal the numpy restatement
tests/components_ref.py, the same result composed in torch on the same device (the yardstick: `scatter_reduce_(amin)` hooking plus
pointer jumping to a fixed point, its host reads counted), the restatement and `scipy.sparse.csgraph.connected_components` on the host,
one giant component against the same nodes cut into about 10^4, and `mesh_superpoints` before and after the clean.  Kernel times per
stage come from a profiler run of their own (`--trace-run` makes the same calls in a fixed order); `--stages-from` cuts that trace into
calls and stages by the order of the cc_* kernels: the library's sort and scan kernels between two of them belong to the stage that
launched them."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

DISTINCT_VIEWS = 64
WARMUP = 1
MIN_FACES = 30
MIN_POINTS = 30
PLANE = 670                         # the giant component: a 670 x 670 grid, 448 900 vertices - the room's size
TILE = 7                            # ... cut into 96 x 96 = 9 216 tiles of 7 x 7 vertices
CASES = ("room_clean_mesh", "cloud_table_k16", "one_giant_component", "cut_into_1e4")
# the first kernel of each stage; everything up to the next marker belongs to it, cc_info_kernel ends a call
MARKERS = (("cc_init_kernel", "hook"), ("cc_flatten_kernel", "flatten_number"), ("cc_label_kernel", "node_sort_stats"),
           ("cc_verify_kernel", "verify_link_sort_stats"), ("cc_finish_kernel", "keep_compact"))
STAGES = tuple(s for _, s in MARKERS)
LAST = "cc_info_kernel"


def timed(fn, reps, warmup=WARMUP):
    import torch
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


def short(name):
    """`void cc_hook_kernel<0>(...)` -> `cc_hook_kernel<0>`."""
    name = name.split("(")[0].strip()
    return name.split(" ")[-1]


def stages_from(path, reps):
    """The kernel rows of a rocprofv3 trace of a `--trace-run`, in start order, cut into calls and stages by MARKERS; the run makes
    (WARMUP + reps) calls per case in the order of CASES."""
    rows = list(csv.DictReader(open(path)))
    col = {k.lower(): k for k in rows[0]}
    name, start, end = col["kernel_name"], col["start_timestamp"], col["end_timestamp"]
    rows = sorted((int(r[start]), int(r[end]), r[name]) for r in rows)
    calls, stage = [], None
    for b, e, n in rows:
        for marker, s in MARKERS:
            if marker in n:
                stage = s
                if s == STAGES[0]:
                    calls.append(dict({k: 0.0 for k in STAGES}, kernels=0, begin=b, by_kernel={}))
        if stage is None:
            continue
        ms = (e - b) * 1e-6
        calls[-1][stage] += ms
        calls[-1]["kernels"] += 1
        calls[-1]["by_kernel"][short(n)] = calls[-1]["by_kernel"].get(short(n), 0.0) + ms
        if LAST in n:
            calls[-1]["span"] = (e - calls[-1].pop("begin")) * 1e-6
            stage = None
    want = len(CASES) * (WARMUP + reps)
    if len(calls) != want or any("span" not in c for c in calls):
        raise SystemExit(f"components_bench: {len(calls)} calls in the trace, expected {want}: was it a --trace-run with the same --reps?")
    out = {}
    for i, case in enumerate(CASES):
        mine = calls[i * (WARMUP + reps) + WARMUP:(i + 1) * (WARMUP + reps)]
        out[case] = {k: dict(median_ms=statistics.median(c[k] for c in mine), min_ms=min(c[k] for c in mine), max_ms=max(c[k] for c in mine))
                     for k in STAGES + ("span",)}
        out[case]["kernels_per_call"] = mine[0]["kernels"]
        out[case]["by_kernel_median_ms"] = {k: statistics.median(c["by_kernel"].get(k, 0.0) for c in mine) for k in sorted(mine[0]["by_kernel"])}
    return out


def debris(rng, lo, hi, pieces, channels):
    """`pieces` floating pieces inside the box lo .. hi, a third each: one triangle, a fan of 19 vertices (17 faces), a grid of 40
    vertices (56 faces) -> (vertices fp32 [., channels], faces int32 relative to the first debris vertex)."""
    import numpy as np
    import simplify_case as SK
    fan = np.concatenate([[[0, 0, 0]], 0.04 * np.stack([np.cos(np.arange(18) / 3.0), np.sin(np.arange(18) / 3.0), np.zeros(18)], axis=1)])
    fan_f = np.stack([np.zeros(17, np.int64), np.arange(1, 18), np.arange(2, 19)], axis=1)
    grid, grid_f = SK.plane(7, 0.02)
    grid, grid_f = grid[:40], grid_f[(grid_f < 40).all(axis=1)]
    shapes = [(np.array([[0, 0, 0], [0.02, 0, 0], [0, 0.02, 0]]), np.array([[0, 1, 2]])), (fan, fan_f), (grid, grid_f)]
    vs, fs, base = [], [], 0
    for i in range(pieces):
        v, f = shapes[i % 3]
        vs.append(v + rng.uniform(lo, hi)[None])
        fs.append(f + base)
        base += len(v)
    v = np.concatenate(vs).astype(np.float32)
    return np.concatenate([v, np.full((len(v), channels - 3), 128.0, np.float32)], axis=1), np.concatenate(fs).astype(np.int32)


def torch_baseline(coords, pairs, n):
    """The same components composed in torch on the device: good nodes by tensor arithmetic, then rounds of `scatter_reduce_(amin)`
    hooking of the ends' current roots and pointer jumping to a fixed point, until no link has two roots; numbering by a cumulative sum
    of the root flags, sizes by `bincount`.  -> (labels int64 [n], n_nodes, n_links, host reads made)."""
    import torch
    d = pairs.device
    good = (coords.abs() < 16384.0).all(dim=1) if coords is not None else torch.ones(n, dtype=torch.bool, device=d)
    inside = ((pairs >= 0) & (pairs < n)).all(dim=1)
    ok = inside & good[pairs.clamp(0, max(n - 1, 0))].all(dim=1)
    a, b = pairs[ok, 0], pairs[ok, 1]
    parent = torch.arange(n, device=d)
    reads = 1                                                                           # the mask indexing above synchronises
    while True:
        pa, pb = parent[a], parent[b]
        low = torch.minimum(pa, pb)
        parent.scatter_reduce_(0, pa, low, "amin")
        parent.scatter_reduce_(0, pb, low, "amin")
        while True:
            up = parent[parent]
            reads += 1
            if bool((up == parent).all()):
                break
            parent = up
        reads += 1
        if bool((parent[a] == parent[b]).all()):
            break
    is_root = good & (parent == torch.arange(n, device=d))
    number = torch.cumsum(is_root, 0) - 1
    labels = torch.where(good, number[parent], torch.full_like(parent, -1))
    k = int(is_root.sum())
    reads += 1
    n_nodes = torch.bincount(labels[good], minlength=k)
    n_links = torch.bincount(labels[a], minlength=k)
    return labels, n_nodes, n_links, reads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--pieces", type=int, default=300, help="floating pieces planted in the mesh; three times as many points in the cloud")
    ap.add_argument("--trace-run", action="store_true", help="only the component calls, in a fixed order: for a profiler run")
    ap.add_argument("--stages-from", default=None, help="a kernel_trace.csv of a --trace-run: report stage times, no device needed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_components.json"))
    args = ap.parse_args()
    if args.stages_from:
        res = dict(reps=args.reps, cases=list(CASES), stages=stages_from(args.stages_from, args.reps))
        print(json.dumps(res, indent=1))
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        return
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("components_bench: needs a HIP device (a measurement does not fall back to the CPU)")
    import components_ref as R
    import fuse_views_case as K
    import simplify_case as SK
    from segdino3d_amd import components, fuse_views, lift2d, ops, superpoints, tsdf
    d = torch.device("cuda:0")
    H, W, V = args.height, args.width, args.views
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    n_distinct = min(DISTINCT_VIEWS, V)
    room = K.room(n_distinct, H, W, (H, W), scale=args.scale)
    print(f"{n_distinct} views of {H} x {W} rendered on the host in {time.perf_counter() - t0:.1f} s", flush=True)
    sel = [i % n_distinct for i in range(V)]
    vol = tsdf.TsdfVolume(voxel=args.voxel, trunc=4 * args.voxel, capacity=1 << 16)
    for lo in range(0, V, ops.TSDF_MAX_CALL_VIEWS):
        idx = sel[lo:lo + ops.TSDF_MAX_CALL_VIEWS]
        vol.add(lift2d.Views(torch.from_numpy(room["depth_u16"][idx]).to(d), torch.from_numpy(room["intr"][idx]).to(d), room["poses"][idx],
                             K.DEPTH_SCALE), torch.from_numpy(room["colors"][idx]).to(d))
    rv, rf = vol.mesh()
    del vol
    distinct = lift2d.Views(torch.from_numpy(room["depth_u16"]).to(d), torch.from_numpy(room["intr"]).to(d), room["poses"], K.DEPTH_SCALE)
    rc = fuse_views.fuse_views(distinct, torch.from_numpy(room["colors"]).to(d), voxel=args.voxel, min_obs=1)
    C = rv.shape[1]
    lo, hi = rv[:, :3].min(dim=0).values.cpu().numpy() + 0.3, rv[:, :3].max(dim=0).values.cpu().numpy() - 0.3
    dv, df = debris(rng, lo, hi, args.pieces, C)
    vertices = torch.cat([rv, torch.from_numpy(dv).to(d)]).contiguous()
    faces = torch.cat([rf, torch.from_numpy(df).to(d) + rv.shape[0]]).contiguous()
    cv, _ = debris(rng, lo, hi, 3 * args.pieces, rc.shape[1])
    cloud = torch.cat([rc, torch.from_numpy(cv).to(d)]).contiguous()
    nbr = superpoints.knn_graph(cloud[:, :3].contiguous(), 16, 0.1)
    pv, pf = SK.plane(PLANE, 0.01)
    tile = (pf // PLANE // TILE) * PLANE + (pf % PLANE) // TILE
    whole = (tile == tile[:, :1]).all(axis=1)
    cut = np.where(whole[:, None], pf, pf[:, :1])                                       # a face across a border shrinks to its first corner
    pv, pf, cut = torch.from_numpy(pv).to(d), torch.from_numpy(pf).to(d), torch.from_numpy(np.ascontiguousarray(cut)).to(d)
    Nv, F, N = vertices.shape[0], faces.shape[0], cloud.shape[0]
    print(f"room mesh: {rv.shape[0]} + {len(dv)} vertices, {rf.shape[0]} + {len(df)} faces, {C} channels; cloud: {rc.shape[0]} + {len(cv)} points, k = 16; "
          f"plane: {pv.shape[0]} vertices, {pf.shape[0]} faces", flush=True)
    res = dict(device=torch.cuda.get_device_name(0), image=[H, W], views=V, distinct_views=n_distinct, voxel=args.voxel, room_vertices=rv.shape[0],
               room_faces=rf.shape[0], debris_pieces=args.pieces, vertices=Nv, faces=F, channels=C, cloud_points=N, room_cloud_points=rc.shape[0], k=16,
               radius=0.1, plane=[PLANE, PLANE], tile=TILE)

    def table():
        out = ops.components("table", nbr, N, cloud, min_nodes=MIN_POINTS, clean=True)
        return out, components.ComponentsInfo(*out["info"].tolist())

    calls = {"room_clean_mesh": lambda: components.clean_mesh(vertices, faces, min_faces=MIN_FACES, return_info=True),
             "cloud_table_k16": table,
             "one_giant_component": lambda: components.mesh_components(pv, pf, return_info=True),
             "cut_into_1e4": lambda: components.mesh_components(pv, cut, return_info=True)}
    if args.trace_run:
        for case in CASES:
            timed(calls[case], args.reps)
        torch.cuda.synchronize()
        print("trace run done")
        return
    for case in CASES:
        res[case] = timed(calls[case], args.reps)
        res[case]["info"] = calls[case]()[1]._asdict()
        print(json.dumps({case: res[case]}), flush=True)
    res["mesh_components"] = timed(lambda: components.mesh_components(vertices, faces), args.reps)
    res["clean_points_with_knn"] = timed(lambda: components.clean_points(cloud, k=16, radius=0.1, min_points=MIN_POINTS), args.reps)
    res["knn_graph_alone"] = timed(lambda: superpoints.knn_graph(cloud[:, :3].contiguous(), 16, 0.1), args.reps)

    # ---- the restatement and scipy on the host
    vn, fn, cn, tn = vertices.cpu().numpy(), faces.cpu().numpy(), cloud.cpu().numpy(), nbr.cpu().numpy()
    mesh, info = calls["room_clean_mesh"]()
    t0 = time.perf_counter()
    want = R.components_ref(Nv, fn, "faces", vn, min_links=MIN_FACES, min_nodes=1)
    host_mesh = time.perf_counter() - t0
    same = bool(info._asdict() == want.info and all(
        np.array_equal(g.cpu().numpy().view(np.uint32), np.ascontiguousarray(w).view(np.uint32))
        for g, w in zip(mesh, (want.nodes, want.links, want.node_map, want.link_source, want.labels_out))))
    res["room_clean_mesh"].update(equal_bits=same, restatement_seconds=host_mesh, kept_faces_by_component=sorted(want.n_links[want.keep > 0].tolist(), reverse=True)[:8])
    out, tinfo = table()
    t0 = time.perf_counter()
    want = R.components_ref(N, tn, "table", cn, min_nodes=MIN_POINTS)
    host_cloud = time.perf_counter() - t0
    nn = tinfo.nodes
    same = bool(tinfo._asdict() == want.info and np.array_equal(out["labels"].cpu().numpy(), want.labels) and
                np.array_equal(out["node_map"].cpu().numpy(), want.node_map) and np.array_equal(out["links"][:nn].cpu().numpy(), want.links) and
                np.array_equal(out["nodes"][:nn].cpu().numpy().view(np.uint32), want.nodes.view(np.uint32)) and
                np.array_equal(out["labels_out"][:nn].cpu().numpy(), want.labels_out))
    res["cloud_table_k16"].update(equal_bits=same, restatement_seconds=host_cloud)
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import connected_components
        t0 = time.perf_counter()
        a = np.concatenate([fn[:, 0], fn[:, 1]]).astype(np.int64)
        b = np.concatenate([fn[:, 1], fn[:, 2]]).astype(np.int64)
        k_mesh, _ = connected_components(sp.coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(Nv, Nv)).tocsr(), directed=False)
        s_mesh = time.perf_counter() - t0
        t0 = time.perf_counter()
        rows = np.repeat(np.arange(N, dtype=np.int64), tn.shape[1])
        live = tn.reshape(-1) >= 0
        k_cloud, _ = connected_components(sp.coo_matrix((np.ones(int(live.sum()), np.int8), (rows[live], tn.reshape(-1)[live])), shape=(N, N)).tocsr(), directed=False)
        s_cloud = time.perf_counter() - t0
        res["scipy"] = dict(mesh_seconds=s_mesh, mesh_components=int(k_mesh), cloud_seconds=s_cloud, cloud_components=int(k_cloud),
                            note="labels only: no sizes, boxes, thresholds or compaction")
    except ImportError:
        res["scipy"] = "not installed: not measured"
    print(json.dumps({k: res[k] for k in ("room_clean_mesh", "cloud_table_k16", "scipy")}), flush=True)

    # ---- the yardstick: torch on the device
    pairs_mesh = torch.cat([faces[:, :2], faces[:, 1:]]).long()
    pairs_cloud = torch.stack([torch.arange(N, device=d).repeat_interleave(nbr.shape[1]), nbr.reshape(-1).long()], dim=1)
    pairs_cloud = pairs_cloud[pairs_cloud[:, 1] >= 0]
    for name, coords, pairs, n, labels in (("room_clean_mesh", vertices, pairs_mesh, Nv, components.mesh_components(vertices, faces).labels),
                                           ("cloud_table_k16", cloud, pairs_cloud, N, out["labels"])):
        t = timed(lambda: torch_baseline(coords, pairs, n), args.reps)
        bl, bn, _, reads = torch_baseline(coords, pairs, n)
        res[name]["torch_baseline"] = dict(t, over_call=t["median_ms"] / res[name]["median_ms"], host_reads=reads,
                                           labels_agree=bool(torch.equal(bl.int(), labels)), note="labels and sizes only: no boxes, thresholds or compaction")
        print(json.dumps({name: res[name]["torch_baseline"]}), flush=True)

    # ---- downstream: the superpoint sweep before and after the clean
    xyz = vertices[:, :3].contiguous()
    small = mesh.vertices[:, :3].contiguous()
    before, after = superpoints.mesh_superpoints(xyz, faces, return_info=True)[1], superpoints.mesh_superpoints(small, mesh.faces, return_info=True)[1]
    res["mesh_superpoints"] = dict(before=dict(timed(lambda: superpoints.mesh_superpoints(xyz, faces), args.reps), superpoints=before.count),
                                   after=dict(timed(lambda: superpoints.mesh_superpoints(small, mesh.faces), args.reps), superpoints=after.count))
    print(json.dumps({"mesh_superpoints": res["mesh_superpoints"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
