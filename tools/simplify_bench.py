"""Times mesh decimation (`segdino3d_amd/simplify.py`, csrc/simplify.hip) on a synthetic scene of real size, no files: the closed-form
room of tests/fuse_views_case.py scaled to a ScanNet-sized room, 64 distinct views of 480 x 640 (the 256-view fusion repeats them four
times), fused by `tsdf.TsdfVolume` at 2 cm into the room mesh of tools/tsdf_bench.py, which is then decimated at each `cell`.

    python tools/simplify_bench.py [--views 256] [--reps 5] [--out profiles/simplify.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/simplify_bench.py --trace-run --reps 3      # a run of its own
    python tools/simplify_bench.py --stages-from DIR/.../kernel_trace.csv --reps 3 --out profiles/simplify_stages.json  # no device needed

The first form reports per `cell` (HIP events around the call, the one host read included; warm-up, then `--reps` runs: median, min,
max): the call, the output sizes and counters, whether the outputs equal the numpy restatement tests/simplify_ref.py, the same result
composed in torch on the same device (the yardstick: `torch.unique(return_inverse=True)` + `index_add_` + a second `unique` over
packed face rows), the bytes each stage must move against the HBM peak, and downstream `mesh_superpoints` and `render_mesh` on the full
against the decimated mesh.  `--count-cells` lists further cells for which only the output sizes are taken.  Kernel times per stage
come from a profiler run of their own (`--trace-run` makes the same decimation calls in a fixed order); `--stages-from` cuts that
trace into calls and stages by the order of the sm_* kernels: the library's sort and scan kernels between two of them belong to the
stage that launched them."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HBM_PEAK = 8.0e12
DISTINCT_VIEWS = 64
CELLS = (0.03, 0.04, 0.06)
TARGET_VERTICES = 150544            # ScanNet's decimated scan, the benchmark scene of this repository
WARMUP = 1
# the first kernel of each stage; everything up to the next marker belongs to it, sm_cells_kernel ends a call
MARKERS = (("sm_vkey_kernel", "vertex_sort"), ("sm_vheads_kernel", "reduce"), ("sm_fkey_kernel", "face_sort"), ("sm_fheads_kernel", "compact"))
STAGES = tuple(s for _, s in MARKERS)
LAST = "sm_cells_kernel"


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


def stages_from(path, reps):
    """The kernel rows of a rocprofv3 trace of a `--trace-run`, in start order, cut into calls and stages by MARKERS; the run makes
    (WARMUP + reps) calls per cell in the order of CELLS."""
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
                    calls.append(dict({k: 0.0 for k in STAGES}, kernels=0, begin=b))
        if stage is None:
            continue
        calls[-1][stage] += (e - b) * 1e-6
        calls[-1]["kernels"] += 1
        if LAST in n:
            calls[-1]["span"] = (e - calls[-1].pop("begin")) * 1e-6
            stage = None
    want = len(CELLS) * (WARMUP + reps)
    if len(calls) != want or any("span" not in c for c in calls):
        raise SystemExit(f"simplify_bench: {len(calls)} decimation calls in the trace, expected {want}: was it a --trace-run with the same --reps?")
    out = {}
    for i, cell in enumerate(CELLS):
        mine = calls[i * (WARMUP + reps) + WARMUP:(i + 1) * (WARMUP + reps)]
        out[f"cell_{cell}"] = {k: dict(median_ms=statistics.median(c[k] for c in mine), min_ms=min(c[k] for c in mine), max_ms=max(c[k] for c in mine))
                               for k in STAGES + ("span",)} | dict(kernels_per_call=mine[0]["kernels"])
    return out


def bytes_needed(V, F, C, Vn, Fn):
    """What each stage must move at the least, from the shapes alone: every input it reads once, every output it writes once, and for a
    sort one read and one write of its (key, index) pairs - a lower bound that no multi-pass radix sort reaches (the library's makes 8
    passes over 64-bit keys, each reading the keys twice and the indices once and writing both: 32 bytes an element and pass)."""
    pair = 12
    return dict(
        vertex_sort=V * C * 4 + V * 8 + 2 * V * pair,                                 # rows in, keys out; the pairs in and out
        reduce=V * pair + V * C * 4 + V * 4 + Vn * (C + 1) * 8,                         # sorted pairs, rows again, vertex_map, the sums
        face_sort=F * 12 + 3 * F * 4 + F * 8 + 2 * F * pair,                            # faces, three map reads, keys out; the pairs in and out
        compact=F * pair + 2 * F * 4 + Fn * (12 + 12 + 4 + 16) + Vn * ((C + 1) * 8 + C * 4),   # sorted pairs, flags, kept faces, output rows
    )


def torch_baseline(vertices, faces, inv_cell):
    """The same result composed in torch (fp32 sums: the yardstick is not bit-exact) -> (vertices, faces, vertex_map, face_source)."""
    import torch
    V = vertices.shape[0]
    ok = (vertices.abs() < 16384.0).all(dim=1)
    k = torch.floor(vertices[:, :3] * inv_cell).long() + (1 << 20)
    key = (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]
    key = torch.where(ok, key, torch.full_like(key, -1))
    ukeys, inverse = torch.unique(key, return_inverse=True)
    if bool((~ok).any()):
        inverse = torch.where(ok, inverse - 1, torch.full_like(inverse, -1))
        ukeys = ukeys[1:]
    n_cells = ukeys.shape[0]
    live = inverse.clamp_min(0)
    sums = torch.zeros(n_cells, vertices.shape[1], device=vertices.device).index_add_(0, live, torch.where(ok[:, None], vertices, torch.zeros_like(vertices)))
    count = torch.zeros(n_cells, device=vertices.device).index_add_(0, live, ok.float())
    out_v = sums / count[:, None]
    f = faces.long()
    inside = ((f >= 0) & (f < V)).all(dim=1)
    m = inverse[f.clamp(0, max(V - 1, 0))]
    good = inside & (m >= 0).all(dim=1) & (m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2])
    src = torch.nonzero(good).flatten()
    m = m[src]
    shift = m.argmin(dim=1)
    cols = (shift[:, None] + torch.arange(3, device=m.device)[None]) % 3
    rot = torch.gather(m, 1, cols)
    tkey = (rot[:, 0] << 42) | (rot[:, 1] << 21) | rot[:, 2]
    ukey, inv = torch.unique(tkey, return_inverse=True)                                 # the second unique: over the packed face rows
    first = torch.full((ukey.shape[0],), src.shape[0], device=m.device, dtype=torch.long).scatter_reduce_(0, inv, torch.arange(src.shape[0], device=m.device), "amin")
    first = torch.sort(first).values
    return out_v, rot[first].int(), inverse.int(), src[first].int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--count-cells", type=float, nargs="*", default=[0.025, 0.0325, 0.035, 0.0375, 0.045, 0.05])
    ap.add_argument("--trace-run", action="store_true", help="only the decimation calls, in a fixed order: for a profiler run")
    ap.add_argument("--stages-from", default=None, help="a kernel_trace.csv of a --trace-run: report stage times, no device needed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify.json"))
    args = ap.parse_args()
    if args.stages_from:
        res = dict(reps=args.reps, cells=list(CELLS), stages=stages_from(args.stages_from, args.reps))
        print(json.dumps(res, indent=1))
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        return
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("simplify_bench: needs a HIP device (a measurement does not fall back to the CPU)")
    import fuse_views_case as K
    import simplify_ref as R
    from segdino3d_amd import lift2d, ops, raster, simplify, superpoints, tsdf
    d = torch.device("cuda:0")
    H, W, V = args.height, args.width, args.views
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
    vertices, faces = vol.mesh()
    del vol
    Nv, F, C = vertices.shape[0], faces.shape[0], vertices.shape[1]
    print(f"room mesh: voxel {args.voxel}, {V} views, {Nv} vertices, {F} faces, {C} channels", flush=True)
    res = dict(device=torch.cuda.get_device_name(0), image=[H, W], views=V, distinct_views=n_distinct, voxel=args.voxel, vertices=Nv, faces=F,
               channels=C, hbm_peak=HBM_PEAK)
    if args.trace_run:
        for cell in CELLS:
            timed(lambda cell=cell: simplify.simplify_mesh(vertices, faces, cell=cell), args.reps)
        torch.cuda.synchronize()
        print("trace run done")
        return
    vn, fn = vertices.cpu().numpy(), faces.cpu().numpy()
    poses, intr = room["poses"][sel], torch.from_numpy(room["intr"][sel]).to(d)
    xyz = vertices[:, :3].contiguous()
    full = dict(mesh_superpoints=timed(lambda: superpoints.mesh_superpoints(xyz, faces), args.reps),
                render_mesh=timed(lambda: raster.render_mesh(xyz, faces, intr, poses, H, W), args.reps))
    res["full_mesh"] = full
    print(json.dumps({"full_mesh": full}), flush=True)
    for cell in CELLS:
        t = timed(lambda: simplify.simplify_mesh(vertices, faces, cell=cell), args.reps)
        near = timed(lambda: simplify.simplify_mesh(vertices, faces, cell=cell, placement="nearest", keep_unreferenced=False), args.reps)
        got, info = simplify.simplify_mesh(vertices, faces, cell=cell, return_info=True)
        t0 = time.perf_counter()
        want = R.simplify_ref(vn, fn, cell=cell)
        host_s = time.perf_counter() - t0
        same = bool(np.array_equal(got.vertices.cpu().numpy().view(np.uint32), want.vertices.view(np.uint32)) and
                    np.array_equal(got.faces.cpu().numpy(), want.faces) and np.array_equal(got.vertex_map.cpu().numpy(), want.vertex_map) and
                    np.array_equal(got.face_source.cpu().numpy(), want.face_source) and info._asdict() == want.info)
        inv = float(np.float32(1.0 / cell))
        base = timed(lambda: torch_baseline(vertices, faces, inv), args.reps)
        bv, bf, bm, bs = torch_baseline(vertices, faces, inv)
        base_same = dict(faces=bool(torch.equal(bf, got.faces)), vertex_map=bool(torch.equal(bm, got.vertex_map)),
                         face_source=bool(torch.equal(bs, got.face_source)), max_vertex_diff=float((bv - got.vertices).abs().max()))
        need = bytes_needed(Nv, F, C, info.vertices, info.faces)
        sec = t["median_ms"] * 1e-3
        small_xyz = got.vertices[:, :3].contiguous()
        r = dict(t, cell=cell, info=info._asdict(), nearest_dropping=near, equal_bits=same, restatement_seconds=host_s,
                 torch_baseline=dict(base, over_kernels=base["median_ms"] / t["median_ms"], agrees=base_same),
                 bytes_needed=need, bytes_needed_total=sum(need.values()), needed_TBps=sum(need.values()) / sec / 1e12,
                 needed_fraction_of_hbm_peak=sum(need.values()) / sec / HBM_PEAK,
                 mesh_superpoints=timed(lambda: superpoints.mesh_superpoints(small_xyz, got.faces), args.reps),
                 render_mesh=timed(lambda: raster.render_mesh(small_xyz, got.faces, intr, poses, H, W), args.reps))
        res[f"cell_{cell}"] = r
        print(json.dumps({f"cell_{cell}": r}), flush=True)
    counts = {c: res[f"cell_{c}"]["info"]["vertices"] for c in CELLS}
    for cell in args.count_cells:
        counts[cell] = simplify.simplify_mesh(vertices, faces, cell=cell, return_info=True)[1].vertices
    res["vertices_by_cell"] = {str(c): counts[c] for c in sorted(counts)}
    best = min(CELLS, key=lambda c: abs(counts[c] - TARGET_VERTICES))
    res["nearest_to_target"] = dict(target=TARGET_VERTICES, cell_of_the_three=best, cell_of_all=min(counts, key=lambda c: abs(counts[c] - TARGET_VERTICES)))
    print(json.dumps({k: res[k] for k in ("vertices_by_cell", "nearest_to_target")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
