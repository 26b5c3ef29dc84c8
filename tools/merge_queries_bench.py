"""Times the merging of lifted 2D queries across views (`lift_queries.merge_queries`, csrc/merge_queries.hip) on synthetic scenes of real
size, no files: `M` valid rows (2 000, 8 000, 16 384) of C = 256 fp16 features, 100 query slots per frame, drawn from M / 40 objects
scattered over an 8 x 8 x 2.5 m room with 4 cm of centre noise and feature noise of a tenth of the signal - every object is in about
forty rows, as the object in front of the camera is.

    python tools/merge_queries_bench.py [--sizes 2000 8000 16384] [--channels 256] [--reps 20] [--out profiles/merge_queries.json]

Reports per size, by HIP events around a queue of calls (medians over `--reps`): the four stages - adjacency (validity, ranking, codes
and the Gram kernel), sweep, reduce, emit - and `merge_queries` as a whole with its host read; the int8 operations of the Gram
product over the upper triangle of 64 x 64 tile pairs and the share of the 5 P op/s int8 matrix peak they would be if the adjacency call
were the Gram kernel alone (a lower bound of the kernel's share; `tools/profile_cmd.sh` gives the kernel's own time).  Baselines, never
the kernels themselves: the torch formulation on the same device the way a user would write it today (`cdist`, a normalised matmul,
a greedy loop over seeds, `index_add_` for the means), and the restatement tests/merge_queries_ref.py on the host.  The cluster counts
of all three are printed first; the restatement's labels must equal the kernels'."""
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

import merge_queries_ref as R  # noqa: E402

INT8_PEAK = 5.0e15             # dense int8 MFMA, operations per second: twice the bf16 rate
ROWS_PER_OBJECT = 40
QUERIES_PER_VIEW = 100


def timed(fn, reps, warmup=2, inner=1):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), reps=reps, calls_per_rep=inner)


def make_rows(M, C, seed):
    rng = np.random.default_rng(seed)
    K = max(1, M // ROWS_PER_OBJECT)
    oc = rng.uniform((0, 0, 0), (8, 8, 2.5), (K, 3))
    of = rng.standard_normal((K, C))
    obj = rng.integers(0, K, M)
    centre = (oc[obj] + rng.uniform(-0.04, 0.04, (M, 3))).astype(np.float32)
    feats = (of[obj] + 0.1 * rng.standard_normal((M, C))).astype(np.float16)
    scores = rng.uniform(0.3, 1.0, M).astype(np.float32)
    count = rng.integers(16, 3000, M).astype(np.int32)
    return feats, centre, scores, count, K


def torch_baseline(feats, centre, scores, count, radius, sim):
    """cdist + normalised matmul + a greedy loop over seeds, one host read per seed; weighted means by index_add_."""
    M = scores.shape[0]
    order = torch.argsort(scores, descending=True, stable=True)
    c, f, w = centre[order], torch.nn.functional.normalize(feats[order].float(), dim=1), count[order].float()
    adj = (torch.cdist(c, c) <= radius) & (f @ f.T >= sim)
    free = torch.ones(M, dtype=torch.bool, device=scores.device)
    label = torch.full((M,), -1, dtype=torch.int64, device=scores.device)
    n_seeds = 0
    while True:
        rest = torch.nonzero(free)
        if rest.numel() == 0:
            break
        a = int(rest[0])                                                              # the host read of the loop
        take = adj[a] & free
        take[a] = True
        label[take] = n_seeds
        free &= ~take
        n_seeds += 1
    pos = torch.zeros(n_seeds, 3, device=scores.device).index_add_(0, label, c * w[:, None])
    out = torch.zeros(n_seeds, feats.shape[1], device=scores.device).index_add_(0, label, feats[order].float() * w[:, None])
    wsum = torch.zeros(n_seeds, device=scores.device).index_add_(0, label, w)
    return out / wsum[:, None], pos / wsum[:, None], n_seeds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 8000, 16384])
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-baseline", action="store_true", help="kernels only (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_queries.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("merge_queries_bench: needs a HIP device (a measurement does not fall back to the CPU)")
    from segdino3d_amd import lift_queries, ops
    d = torch.device("cuda:0")
    C = args.channels
    rule = lift_queries._merge_rule({}, lift_queries.RULE_DEFAULTS["score_thr"], lift_queries.RULE_DEFAULTS["min_pixels"])
    res = dict(channels=C, device=torch.cuda.get_device_name(0), rule={k: rule[k] for k in ("radius", "sim", "min_views", "reduce")}, sizes={})
    for M in args.sizes:
        feats_h, centre_h, scores_h, count_h, K = make_rows(M, C, seed=M)
        feats, centre, scores, count = (torch.from_numpy(x).to(d) for x in (feats_h, centre_h, scores_h, count_h))
        merged = lift_queries.merge_queries(feats, centre, scores, count, QUERIES_PER_VIEW)
        r = dict(rows=M, objects=K, clusters=int(merged.feats.shape[0]))
        if not args.no_baseline:
            t0 = time.perf_counter()
            ref = R.merge(feats_h, centre_h, scores_h, count_h, QUERIES_PER_VIEW, feat_dtype=np.float32)
            r["restatement_on_host_ms"] = (time.perf_counter() - t0) * 1e3
            same = np.array_equal(ref["labels"], merged.labels.cpu().numpy()) and np.array_equal(ref["pos"], merged.pos.cpu().numpy()) \
                and np.array_equal(ref["feats"], merged.feats.cpu().numpy())
            r["equals_restatement"] = bool(same)
            if not same:
                raise SystemExit(f"merge_queries_bench: the kernels differ from the restatement at M = {M}; nothing is timed")
            r["torch_clusters"] = torch_baseline(feats, centre, scores, count, rule["radius"], rule["sim"])[2]

        def stages():
            ws = ops.merge_queries_adjacency(feats, centre, scores, count, rule["score_thr"], rule["min_pixels"], rule["radius_q"], rule["sim_q"])
            return ws

        ws = stages()
        k_dev = ops.merge_queries_reduce(scores, count, C, QUERIES_PER_VIEW, rule["score_thr"], rule["min_views"], None, ws)
        Kout = int(k_dev.item())
        inner = 5
        r["adjacency"] = timed(stages, args.reps, inner=inner)
        r["sweep"] = timed(lambda: ops.merge_queries_sweep(M, C, ws), args.reps, inner=inner)
        r["reduce"] = timed(lambda: ops.merge_queries_reduce(scores, count, C, QUERIES_PER_VIEW, rule["score_thr"], rule["min_views"], None, ws),
                            args.reps, inner=inner)
        r["emit"] = timed(lambda: ops.merge_queries_emit(feats, scores, count, Kout, False, ws), args.reps, inner=inner)
        r["merge_queries_with_host_read"] = timed(lambda: lift_queries.merge_queries(feats, centre, scores, count, QUERIES_PER_VIEW), args.reps)
        r["stages_sum_ms"] = sum(r[k]["median_ms"] for k in ("adjacency", "sweep", "reduce", "emit"))
        tiles = (M + 63) // 64
        cp = (C + 63) // 64 * 64
        r["gram_int8_ops"] = 2 * (tiles * (tiles + 1) // 2) * 64 * 64 * cp
        r["gram_share_of_int8_peak_if_adjacency_were_gram_alone"] = r["gram_int8_ops"] / (r["adjacency"]["median_ms"] * 1e-3) / INT8_PEAK
        r["bit_matrix_bytes"] = tiles * 64 * tiles * 8
        if not args.no_baseline:
            r["torch_baseline"] = timed(lambda: torch_baseline(feats, centre, scores, count, rule["radius"], rule["sim"]), max(3, args.reps // 4), warmup=1)
            r["torch_over_kernels"] = r["torch_baseline"]["median_ms"] / r["merge_queries_with_host_read"]["median_ms"]
            r["host_restatement_over_kernels"] = r["restatement_on_host_ms"] / r["merge_queries_with_host_read"]["median_ms"]
        res["sizes"][str(M)] = r
        print(json.dumps({str(M): r}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
