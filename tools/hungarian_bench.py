"""Hungarian matching of one training step, host route against device route, in one process:
python tools/hungarian_bench.py [--reps 30] [--warmup 5] [--route both|device|host]

Problems: seeded training-shaped costs, the recipe of tests/test_gpu_criterion.py::_training_size_case (2250 queries, 3000 superpoints,
120 objects, five cost weights) through the criterion's own cost kernel: 7 prediction sets of one scene, and of a batch of 4 scenes (28).
  (a) host route, what the criterion did before the device solver (SD3D_HUNGARIAN=host): per problem `cost.cpu()`,
      scipy.optimize.linear_sum_assignment, index scatter into the match matrix; host clock, ending in a synchronise.
  (b) device route: ONE ops.hungarian_match call over the set (csrc/assign.hip); HIP events around the call.
The two routes alternate, after a warm-up, and every repetition is kept: the JSON line gives median, min, max and the spread
(max - min) per route and set, and whether the two routes returned the same matches.  `--route device` runs (b) alone, for a
kernel trace (rocprofv3 --kernel-trace --stats -- python tools/hungarian_bench.py --route device)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from segdino3d_amd import ops
from segdino3d_amd.criterion import ScanNetUnifiedCriterion, _SceneTruth
from tests.test_gpu_criterion import _training_size_case

Q, S, G, N_CLS, N_SEM, SETS = 2250, 3000, 120, 198, 200, 7
COSTS = ["QueryClassificationCost", "MaskBCECost", "MaskDiceCost", "CenterL1Cost", "SizeL1Cost"]
WEIGHTS = [0.5, 1.0, 1.0, 0.5, 0.5]


def scene_costs(seed, d):
    """The [Q, G] cost matrices of the SETS prediction sets of one seeded scene, computed by sd3d_match_costs."""
    crit = ScanNetUnifiedCriterion(
        num_semantic_classes=N_SEM, sem_criterion=dict(type="ScanNetSemanticCriterion", ignore_index=N_SEM, loss_weight=0.5),
        inst_criterion=dict(type="InstanceCriterion", matcher=dict(type="HungarianMatcher", costs=[dict(type=t, weight=w) for t, w in zip(COSTS, WEIGHTS)]),
                            loss_weight=[0.5, 1.0, 1.0, 0.5, 0.5, 0.5], num_classes=N_CLS, non_object_weight=0.1, fix_dice_loss_weight=True,
                            iter_matcher=True, fix_mean_loss=True))
    t, layers = _training_size_case(seed, Q, S, G, N_CLS, N_SEM, n_layers=SETS)
    truth = _SceneTruth({k: v.to(d) for k, v in t.items()}, N_SEM)
    out = []
    for layer in layers:
        layer = {k: [None if v is None else v.to(d) for v in lst] for k, lst in layer.items()}
        out.append(crit.inst_criterion.costs(layer, 0, truth))
    torch.cuda.synchronize()
    return out


def host_route(costs):
    from scipy.optimize import linear_sum_assignment
    t0 = time.perf_counter()
    out = []
    for cost in costs:
        match = torch.zeros(cost.shape, dtype=torch.uint8, device=cost.device)
        q_ids, g_ids = linear_sum_assignment(cost.cpu().numpy())
        match[torch.as_tensor(q_ids, device=cost.device), torch.as_tensor(g_ids, device=cost.device)] = 1
        out.append(match)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def device_route(costs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = ops.hungarian_match(costs)
    e1.record()
    host_ms = 1e3 * (time.perf_counter() - t0)                  # the enqueue alone: what the host pays
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), host_ms, out


def stats(xs):
    return dict(median_ms=round(statistics.median(xs), 4), min_ms=round(min(xs), 4), max_ms=round(max(xs), 4),
                spread_ms=round(max(xs) - min(xs), 4), reps=len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--route", choices=["both", "device", "host"], default="both")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hungarian_bench: needs a HIP device (a measurement does not fall back to the CPU)")
    d = torch.device("cuda:0")
    costs = [c for seed in range(4) for c in scene_costs(seed, d)]
    result = dict(Q=Q, S=S, G=G, route=a.route)
    for n in (SETS, 4 * SETS):
        sub = costs[:n]
        host, dev, enq, same = [], [], [], True
        for it in range(a.warmup + a.reps):
            mh = md = None
            if a.route in ("both", "host"):
                ms, mh = host_route(sub)
                if it >= a.warmup:
                    host.append(ms)
            if a.route in ("both", "device"):
                ms, hms, md = device_route(sub)
                if it >= a.warmup:
                    dev.append(ms); enq.append(hms)
            if mh is not None and md is not None:
                same = same and all(torch.equal(x, y) for x, y in zip(mh, md))
        r = {}
        if host:
            r["host"] = stats(host)
        if dev:
            r["device"] = stats(dev)
            r["device_enqueue_host"] = stats(enq)
        if host and dev:
            r["same_matches"] = bool(same)
        result[f"problems_{n}"] = r
    print(json.dumps(result))


if __name__ == "__main__":
    main()
