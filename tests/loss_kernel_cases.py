"""Inputs for the direct tests of `segdino3d_amd/csrc/loss.hip` (tests/test_gpu_loss_kernels.py) and their float64 references.

A case is one scene of one prediction set: fp32 tensors on the CPU (so their float64 copies are exact) in the shapes the oracle
(`oracle/loss_ref.py`) takes.  Seeded builders make ordinary cases; the planting helpers put the decisive situations into them (exact
ties, exact-zero logits, IoUs that are small-integer ratios, saturated mask and class logits).  The adapters turn a case into the
oracle's arguments and the oracle's `(iq, ig)` into the byte match matrix `sd3d_instance_loss` takes, and back.  No GPU is needed to
import or to run anything here; tests/test_loss_kernel_cases.py checks the planted properties and the adapters on the CPU.

Tolerance rule (`float_bound`): an error is measured in units of the entry's own scale - the largest magnitude among the terms that
are summed into it, taken from the float64 reference.  The bound is max(8 ulp of fp32, 4 x e32) of that scale, where e32 is the error of
the SAME oracle evaluated in fp32 on the CPU, measured the same way; on top of it no entry may be further than 2e-5 of the largest
reference entry from the reference (the bound of tests/test_gpu_criterion.py).  The kernel's own output never enters."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from oracle import loss_ref

ULP32 = 2.0 ** -23
CAP = 2e-5                  # of the largest reference entry (tests/test_gpu_criterion.py)
FLOOR = 1e-37               # absolute: values that underflow in fp32
MIN_GAP = 1e-4              # 5 x the 2e-5 cost bound at the O(1) cost scale of these cases
INF_COST = loss_ref.INF_COST
COST_WEIGHTS = [0.5, 1.0, 1.0, 0.5, 0.5]
LOSS_WEIGHT = [0.5, 1.0, 1.0, 0.5, 0.5, 0.5]
NON_OBJECT_WEIGHT = 0.1


# ---- seeded cases -----------------------------------------------------------------------------------------------------------------------
def make_case(seed, Q, S, G, n_cls1, boxes=True, scores=True):
    """One scene: objects own random superpoints (owner G = background), every query sits on a superpoint and may be matched to the
    object that owns it plus a quarter of the others; mask logits lean towards the query's own object.  Labels are distinct while
    G <= number of classes, the ground-truth boxes always are."""
    g = torch.Generator().manual_seed(seed)
    n_cls = n_cls1 - 1
    owner = torch.randint(0, G + 1, (S,), generator=g)
    gt = torch.stack([owner == k for k in range(G)]) if G else torch.zeros(0, S, dtype=torch.bool)
    home = torch.randint(0, S, (Q,), generator=g)
    qm = gt[:, home] | (torch.rand(G, Q, generator=g) < 0.25)
    same = (owner[home][:, None] == owner[None, :]) & (owner[home][:, None] < G)
    c = SimpleNamespace(name=f"seed{seed} Q{Q} S{S} G{G} C{n_cls1}", Q=Q, S=S, G=G, n_cls1=n_cls1)
    c.masks = (same.float() * 2 - 1) * 1.5 + 2.0 * torch.randn(Q, S, generator=g)
    c.cls = torch.randn(Q, n_cls1, generator=g)
    c.scores = torch.rand(Q, 1, generator=g) if scores else None
    c.centers = torch.rand(Q, 3, generator=g) * 6 if boxes else None
    c.sizes = torch.rand(Q, 3, generator=g) * 2 if boxes else None
    c.labels = (torch.randperm(max(G, 1), generator=g)[:G] % n_cls).long()
    c.gt_masks, c.query_masks = gt, qm
    c.gt_centers = torch.rand(G, 3, generator=g) * 6
    c.gt_sizes = torch.rand(G, 3, generator=g) * 2
    c.match = None
    c.ties = []
    return c


def random_match(case, seed, p=0.02):
    """An explicit [Q, G] byte match: a sprinkle of pairs, every object matched at least once when Q allows."""
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(case.Q, case.G, generator=g) < p).to(torch.uint8)
    for k in range(min(case.G, case.Q)):
        m[(7 * k + 3) % case.Q, k] = 1
    return m


# ---- planting helpers -------------------------------------------------------------------------------------------------------------------
def duplicate_query(case, src, dst):
    """Query dst becomes query src bit for bit (class row, mask row, score, box, admissibility column)."""
    for k in ("cls", "masks", "scores", "centers", "sizes"):
        v = getattr(case, k)
        if v is not None:
            v[dst] = v[src]
    case.query_masks[:, dst] = case.query_masks[:, src]
    if case.match is not None:
        case.match[dst] = case.match[src]
    case.ties.append((src, dst))


def zero_logits(case, q, cols):
    case.masks[q, cols] = 0.0


def plant_iou(case, q, g, inside, target, outside, seed=0):
    """Object g gets exactly `target` superpoints (the first ones), mask row q is positive on `inside` of them and on `outside`
    superpoints behind them, negative elsewhere: IoU(q, g) = inside / (target + outside), exactly."""
    assert inside <= target and target + outside <= case.S
    gen = torch.Generator().manual_seed(seed + 1000 * q + g)
    mag = 0.5 + torch.rand(case.S, generator=gen) * 3
    pos = torch.zeros(case.S, dtype=torch.bool)
    pos[:inside] = True
    pos[target:target + outside] = True
    case.gt_masks[g] = False
    case.gt_masks[g, :target] = True
    case.masks[q] = torch.where(pos, mag, -mag)
    return inside / (target + outside)


def saturate(case, q, g, level, agree=True, jitter=0.05):
    """Mask row q = +-level * (1 + jitter * U(0, 1)): the sign of object g's mask (agree) or its opposite.  The jitter keeps the sums
    over the row from being exact in fp32, which equal magnitudes would make them."""
    gen = torch.Generator().manual_seed(7919 * q + g)
    sign = case.gt_masks[g].float() * 2 - 1
    case.masks[q] = (sign if agree else -sign) * float(level) * (1 + jitter * torch.rand(case.S, generator=gen))


def extreme_cls(case, q, seed=0):
    """+-80 in class row q (with both signs present whenever there are two columns)."""
    gen = torch.Generator().manual_seed(seed + q)
    row = torch.where(torch.rand(case.n_cls1, generator=gen) < 0.5, 80.0, -80.0)
    row[0], row[-1] = 80.0, -80.0
    case.cls[q] = row


def equal_cls(case, q, value=1.25):
    case.cls[q] = value


# ---- adapters ---------------------------------------------------------------------------------------------------------------------------
def _cast(v, dtype):
    return None if v is None else v.to(dtype)


def cfg_for(case, topk=1, cost_weights=None, loss_weight=None, fix_dice=True):
    return dict(matcher="sparse", topk=topk, cost_weights=list(cost_weights or COST_WEIGHTS), loss_weight=list(loss_weight or LOSS_WEIGHT),
                num_classes=case.n_cls1 - 1, non_object_weight=NON_OBJECT_WEIGHT, fix_dice_loss_weight=fix_dice, iter_matcher=True,
                fix_mean_loss=True)


def oracle_layer(cases, dtype, requires_grad=False):
    """-> (layer, insts) in the shape `instance_layer_loss` takes, one list entry per case (= scene)."""
    layer = {k: [] for k in ("cls_preds", "masks", "scores", "centers", "sizes")}
    insts = []
    for c in cases:
        for key, v in (("cls_preds", c.cls), ("masks", c.masks), ("scores", c.scores), ("centers", c.centers), ("sizes", c.sizes)):
            v = _cast(v, dtype)
            if v is not None and requires_grad:
                v = v.clone().requires_grad_(True)
            layer[key].append(v)
        insts.append(dict(labels=c.labels, sp_masks=c.gt_masks, query_masks=c.query_masks, instance_centers=c.gt_centers.to(dtype),
                          instance_sizes=c.gt_sizes.to(dtype)))
    return layer, insts


def indices_from_match(match):
    """Byte matrix [Q, G] -> the oracle's (iq, ig), query-major like `sparse_match`'s argwhere."""
    ids = torch.argwhere(match.cpu() != 0)
    return ids[:, 0], ids[:, 1]


def match_from_indices(iq, ig, Q, G):
    m = torch.zeros(Q, G, dtype=torch.uint8)
    m[iq, ig] = 1
    return m


def oracle_costs(case, dtype=torch.float64, weights=None, sparse=True, boxes=True):
    """[Q, G] costs of `match_costs`, excluded pairs at 1e8 when `sparse`."""
    w = list(weights or COST_WEIGHTS)
    cost = loss_ref.match_costs(case.cls.to(dtype), case.masks.to(dtype), _cast(case.centers, dtype) if boxes else None,
                                _cast(case.sizes, dtype) if boxes else None, case.labels, case.gt_masks, case.gt_centers.to(dtype),
                                case.gt_sizes.to(dtype), w)
    if sparse:
        cost = torch.where(case.query_masks.T, cost, torch.full_like(cost, INF_COST))
    return cost


def cost_scale(case, weights=None, boxes=True):
    """[Q, G] float64: the largest magnitude among the terms `match_costs` sums into each entry (the 1 of the dice term included)."""
    w = list(weights or COST_WEIGHTS)
    x, t = case.masks.double(), case.gt_masks.double()
    scale = (w[0] * case.cls.double().softmax(-1)[:, case.labels]).abs()
    bce = (F.softplus(-x) @ t.T + F.softplus(x) @ (1 - t).T) / case.S
    scale = torch.maximum(scale, abs(w[1]) * bce)
    scale = torch.maximum(scale, torch.full_like(scale, abs(w[2])))
    if boxes and case.centers is not None and w[3] != 0:
        scale = torch.maximum(scale, abs(w[3]) * (case.centers.double()[:, None] - case.gt_centers.double()[None]).abs().sum(-1))
    if boxes and case.sizes is not None and w[4] != 0:
        scale = torch.maximum(scale, abs(w[4]) * (case.sizes.double()[:, None] - case.gt_sizes.double()[None]).abs().sum(-1))
    return scale


def oracle_instance_raw(cases, matches, dtype, last, cfg=None, requires_grad=True):
    """`instance_layer_loss` fed explicit indices -> (loss, parts, layer): the tensors as the oracle returns them."""
    cfg = cfg or cfg_for(cases[0])
    layer, insts = oracle_layer(cases, dtype, requires_grad=requires_grad)
    loss, _, parts = loss_ref.instance_layer_loss(layer, insts, cfg, last, indices=[indices_from_match(m) for m in matches])
    return loss, parts, layer


def oracle_instance(cases, matches, dtype, last, cfg=None):
    """-> (parts: 6 floats, grads: per case a dict of d loss / d prediction, None where the layer predicts nothing)."""
    loss, parts, layer = oracle_instance_raw(cases, matches, dtype, last, cfg)
    leaves = [v for k in layer for v in layer[k] if v is not None]
    got = torch.autograd.grad(loss, leaves, allow_unused=True)
    by_id = {id(v): (torch.zeros_like(v) if g is None else g) for v, g in zip(leaves, got)}
    grads = [{k: (None if layer[k][i] is None else by_id[id(layer[k][i])].detach()) for k in layer} for i in range(len(cases))]
    return [float(p.detach()) for p in parts], grads


def case_from_scene(target, layer, b, n_sem):
    """Scene b of a prediction set in `unified_criterion`'s layout -> a case."""
    labels = target["labels"]
    G = int(labels.shape[0])
    sp, qm = target["sp_inst_sem_masks"], target["query_inst_sem_masks"]
    assert sp.shape[0] == G + n_sem + 1
    c = SimpleNamespace(name=f"scene{b}", Q=int(qm.shape[1]), S=int(sp.shape[1]), G=G, n_cls1=int(layer["cls_preds"][b].shape[1]))
    c.cls, c.masks, c.scores = layer["cls_preds"][b], layer["masks"][b], layer["scores"][b]
    c.centers, c.sizes = layer["centers"][b], layer["sizes"][b]
    c.labels, c.gt_masks, c.query_masks = labels, sp[:G].bool(), qm[:G].bool()
    zeros = torch.zeros(G, 3, dtype=c.masks.dtype)
    c.gt_centers = target["instance_centers"] if target.get("instance_centers") is not None else zeros
    c.gt_sizes = target["instance_sizes"] if target.get("instance_sizes") is not None else zeros
    c.sem, c.sem_masks = layer.get("sem_preds", [None] * (b + 1))[b], qm[qm.shape[0] - n_sem - 1:].bool()
    c.match, c.ties = None, []
    return c


def part_scales(parts64):
    """Scale of each of the six parts: means of non-negative terms carry their own magnitude, the dice term is 1 - fraction."""
    s = [abs(p) for p in parts64]
    s[2] = max(s[2], 1.0)
    return s


def make_sem_case(seed, Q, C, ignore_last=True):
    """Semantic logits [Q, C] and masks [C, Q]: a sixth of the queries have no row set (target 0), a third have several (the first
    wins); with `ignore_last` a tenth carry the last class alone and are ignored."""
    g = torch.Generator().manual_seed(seed)
    c = SimpleNamespace(name=f"sem seed{seed} Q{Q} C{C}", Q=Q, C=C, ignore_index=C - 1 if ignore_last else -1)
    c.sem = 2.0 * torch.randn(Q, C, generator=g)
    first = torch.randint(0, C, (Q,), generator=g)
    m = torch.zeros(C, Q, dtype=torch.bool)
    m[first, torch.arange(Q)] = True
    more = torch.rand(Q, generator=g) < 1 / 3
    extra = torch.rand(C, Q, generator=g) < 0.3
    m |= extra & more[None, :] & (torch.arange(C)[:, None] > first[None, :])
    m[:, torch.rand(Q, generator=g) < 1 / 6] = False
    if ignore_last:
        lastonly = torch.rand(Q, generator=g) < 0.1
        m[:, lastonly] = False
        m[C - 1, lastonly] = True
    c.sem_masks = m
    return c


def oracle_semantic(case, dtype, loss_weight=0.5):
    """-> (loss, d loss / d sem [Q, C]) of `semantic_loss` for one scene."""
    sem = case.sem.to(dtype).clone().requires_grad_(True)
    loss = loss_ref.semantic_loss([sem], [case.sem_masks], case.ignore_index, loss_weight)
    grad, = torch.autograd.grad(loss, [sem], allow_unused=True)
    return float(loss.detach()), (torch.zeros_like(sem) if grad is None else grad).detach()


# ---- conditions on the inputs -----------------------------------------------------------------------------------------------------------
def check_gaps(cost64, query_masks, topk):
    """Smallest distance, over the object columns, between the (topk + 1)-th smallest float64 cost of the column (excluded pairs at 1e8)
    and its DISTINCT neighbours below and above.  Values exactly equal to it - planted ties - are not neighbours."""
    c = torch.where(query_masks.T, cost64.double(), torch.full_like(cost64.double(), INF_COST))
    gap = float("inf")
    for g in range(c.shape[1]):
        col = torch.sort(c[:, g])[0]
        kth = col[topk]
        below, above = col[col < kth], col[col > kth]
        if below.numel():
            gap = min(gap, float(kth - below[-1]))
        if above.numel():
            gap = min(gap, float(above[0] - kth))
    return gap


# ---- the tolerance rule -----------------------------------------------------------------------------------------------------------------
def _arr(v):
    return torch.as_tensor(v).detach().cpu().double().reshape(-1)


def scaled_error(a, ref64, scale):
    """Largest (|a - ref64| - FLOOR)+ / scale over the finite entries of ref64."""
    a, ref64 = _arr(a), _arr(ref64)
    scale = _arr(scale).expand_as(ref64) if _arr(scale).numel() == 1 else _arr(scale)
    ok = torch.isfinite(ref64) & (scale > 0)
    if not bool(ok.any()):
        return 0.0
    return float((((a[ok] - ref64[ok]).abs() - FLOOR).clamp(min=0) / scale[ok]).max())


def float_bound(ref64, ref32, scale):
    """-> (bound, e32) in units of `scale` (module docstring)."""
    e32 = scaled_error(ref32, ref64, scale)
    return max(8 * ULP32, 4 * e32), e32


RECORDS = []


def check_float(family, case, got, ref64, ref32, scale=None):
    """Assert the tolerance rule; non-finite entries must be the reference's.  `scale` defaults to the largest reference entry."""
    got, r64, r32 = _arr(got), _arr(ref64), _arr(ref32)
    assert got.shape == r64.shape, (family, case, got.shape, r64.shape)
    fin = torch.isfinite(r64)
    top = float(r64[fin].abs().max()) if bool(fin.any()) else 0.0
    if scale is None:
        scale = torch.tensor(top)
    sc = _arr(scale).expand_as(r64) if _arr(scale).numel() == 1 else _arr(scale)
    bound, e32 = float_bound(r64, r32, sc)
    kerr = scaled_error(got, r64, sc)
    worst = float((got[fin] - r64[fin]).abs().max()) if bool(fin.any()) else 0.0
    line = f"[loss-kernel-error] {family} | {case} | kernel {kerr:.3e} | e32 {e32:.3e} | bound {bound:.3e} | abs {worst:.3e} | cap {CAP * top:.3e}"
    print(line)
    RECORDS.append(line)
    assert torch.equal(torch.isnan(got), torch.isnan(r64)), (family, case, "NaN set")
    inf = torch.isinf(r64)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], r64[inf]), (family, case, "infinities")
    assert bool(((got[fin] - r64[fin]).abs() <= bound * sc[fin] + FLOOR).all()), (family, case, kerr, bound)
    assert worst <= CAP * top + FLOOR, (family, case, worst, CAP * top)
    return kerr, e32, bound


# ---- the cases the GPU file uses (shared with the CPU test of their conditions) -------------------------------------------------------------
COST_SHAPES = [  # (Q, S, G, n_cls1): every S, Q, G and class count of the cost kernel's strides
    (1, 1, 1, 2), (1, 33, 3, 199), (65, 33, 4, 257), (65, 257, 5, 300), (1, 257, 9, 2), (65, 3000, 67, 199), (65, 257, 67, 300),
]


@lru_cache(maxsize=None)
def cost_case(Q, S, G, n_cls1):
    """Cost-kernel case with an empty object, an object covering everything, a centre equal to its ground truth, +-80 and constant
    class rows."""
    c = make_case(101 + Q + 7 * S + 13 * G + n_cls1, Q, S, G, n_cls1)
    if G >= 3:
        c.gt_masks[1] = False
        c.gt_masks[2] = True
    c.centers[0] = c.gt_centers[0]
    c.sizes[Q - 1] = c.gt_sizes[G - 1]
    extreme_cls(c, 0)
    if Q > 2:
        equal_cls(c, 2)
    return c


MATCH_SHAPES = [  # (Q, S, G, n_cls1, topk, seed) for sparse_match on device-computed costs; every one passes check_gaps
    (65, 33, 4, 257, 1, 0), (65, 257, 5, 300, 2, 0), (200, 257, 9, 19, 1, 0), (200, 33, 67, 199, 3, 0),
]


@lru_cache(maxsize=None)
def match_case(Q, S, G, n_cls1, topk, seed):
    """Case for the matcher: query Q-1 duplicates query 0 and both saturate towards object 0 with its label, so that they are the two
    cheapest of column 0 - an exact tie at the threshold for topk = 1 and below it for topk >= 2."""
    c = make_case(9000 + seed + Q + 7 * S + 13 * G + n_cls1, Q, S, G, n_cls1)
    saturate(c, 0, 0, 15.0)
    c.cls[0] = 0.0
    c.cls[0, c.labels[0]] = 12.0
    c.centers[0], c.sizes[0] = c.gt_centers[0], c.gt_sizes[0]
    c.query_masks[0, 0] = True
    duplicate_query(c, 0, Q - 1)
    return c


def chain_case(seed=3, Q=300, S=1000, G=12, n_cls=18, n_sem=20, n_layers=2):
    """Saturated 'late training' scene for the chain test: +-15 mask logits that agree with the owner of the query's superpoint except
    for 2 % flips, plus unit noise; confident class rows.  -> (target dict, layers, cfg) as `unified_criterion` takes them."""
    g = torch.Generator().manual_seed(seed)
    owner = torch.randint(0, G + 1, (S,), generator=g)
    inst = torch.stack([owner == k for k in range(G)])
    sem_id = torch.randint(0, n_sem + 1, (S,), generator=g)
    sem = torch.stack([sem_id == k for k in range(n_sem + 1)])
    sp = torch.cat([inst, sem])
    ids = torch.randperm(S, generator=g)[:Q]
    labels = torch.randperm(n_cls, generator=g)[:G]
    t = dict(sp_inst_sem_masks=sp, query_inst_sem_masks=sp[:, ids], labels=labels, instance_centers=torch.rand(G, 3, generator=g) * 6,
             instance_sizes=torch.rand(G, 3, generator=g) * 2)
    own = owner[ids]
    same = (own[:, None] == owner[None, :]) & (own[:, None] < G)
    layers = []
    for l in range(n_layers):
        flip = torch.rand(Q, S, generator=g) < 0.02
        sign = torch.where(same ^ flip, 1.0, -1.0)
        cls = torch.randn(Q, n_cls + 1, generator=g)
        tgt = torch.where(own < G, labels[own.clamp(max=G - 1)], torch.full_like(own, n_cls))
        cls[torch.arange(Q), tgt] += 8.0 * torch.rand(Q, generator=g)
        layers.append(dict(cls_preds=[cls], sem_preds=[3.0 * torch.randn(Q, n_sem + 1, generator=g)],
                           masks=[sign * 15.0 + torch.randn(Q, S, generator=g)], scores=[torch.rand(Q, 1, generator=g)],
                           centers=[torch.rand(Q, 3, generator=g) * 6 if l else None], sizes=[torch.rand(Q, 3, generator=g) * 2 if l else None]))
    cfg = dict(matcher="sparse", topk=2, cost_weights=list(COST_WEIGHTS), loss_weight=list(LOSS_WEIGHT), num_classes=n_cls,
               num_semantic_classes=n_sem, sem_ignore_index=n_sem, sem_loss_weight=0.5, non_object_weight=NON_OBJECT_WEIGHT,
               fix_dice_loss_weight=True, iter_matcher=True, fix_mean_loss=True)
    return t, layers, cfg


def chain_gap(t, layers, cfg):
    """check_gaps of every layer of a chain case."""
    G = t["labels"].shape[0]
    gap = float("inf")
    for layer in layers:
        cost = loss_ref.match_costs(layer["cls_preds"][0].double(), layer["masks"][0].double(), _cast(layer["centers"][0], torch.float64),
                                    _cast(layer["sizes"][0], torch.float64), t["labels"], t["sp_inst_sem_masks"][:G],
                                    t["instance_centers"].double(), t["instance_sizes"].double(), cfg["cost_weights"])
        gap = min(gap, check_gaps(cost, t["query_inst_sem_masks"][:G], cfg["topk"]))
    return gap


# ---- hand-built cost matrices for the matcher -------------------------------------------------------------------------------------------
def hand_costs(Q, topk, seed=0):
    """[Q, n] fp32 costs of small integers, 1e8 and infinities (exact in fp32 and float64), one situation per column; -> (cost, dict
    column name -> expected number of matches or None where the oracle alone decides)."""
    g = torch.Generator().manual_seed(seed + 31 * Q + topk)
    cols, expect = [], {}

    def add(name, col, n=None):
        expect[name] = (len(cols), n)
        cols.append(col.float())

    def distinct():
        return (10 + torch.randperm(Q, generator=g)).float()

    add("distinct", distinct(), topk)
    add("all_excluded", torch.full((Q,), INF_COST), 0)
    add("all_equal", torch.full((Q,), 7.0), 0)
    for r in (2, 3, max(2, Q // 2)):
        add(f"random_range{r}", torch.randint(0, r, (Q,), generator=g).float())
    col = torch.full((Q,), INF_COST)                           # exactly topk admissible queries: all of them match
    col[torch.randperm(Q, generator=g)[:topk]] = torch.arange(topk).float()
    add("exactly_topk_admissible", col, topk)
    col = distinct()                                           # infinities
    col[0] = float("-inf")
    if Q > 2:
        col[Q // 2] = float("inf")
        col[Q - 1] = float("-inf")
    add("infinities", col)
    add("all_minus_inf", torch.full((Q,), float("-inf")), 0)
    col = torch.full((Q,), float("inf"))
    col[Q - 1] = 3.0
    add("plus_inf_but_one", col, min(topk, 1))
    if topk >= 1 and Q >= topk + 1:
        for name, a, b in (("tie_at_threshold_neighbours", 0, 1), ("tie_at_threshold_same_lane", 0, 64), ("tie_at_threshold_far", 5, Q - 1)):
            if b >= Q or a >= b:
                continue
            col = 1000 + distinct()
            others = [q for q in torch.randperm(Q, generator=g).tolist() if q not in (a, b)][:topk - 1]
            col[others] = torch.arange(len(others)).float()
            col[a] = col[b] = 500.0                            # sorted: 0 .. topk-2, 500, 500, ...: the threshold is 500, the tie stays out
            add(name, col, topk - 1)
    if topk >= 2:
        for name, a, b in (("tie_below_threshold_neighbours", 0, 1), ("tie_below_threshold_same_lane", 1, 65)):
            if b >= Q:
                continue
            col = 1000 + distinct()
            col[a] = col[b] = 1.0
            others = [q for q in torch.randperm(Q, generator=g).tolist() if q not in (a, b)][:topk - 2]
            col[others] = 2.0 + torch.arange(len(others)).float()
            add(name, col, topk)
    return torch.stack(cols, 1).contiguous(), expect


def hand_topks(Q):
    return sorted({k for k in (0, 1, 2, Q - 1) if 0 <= k and k + 1 <= Q})


def packbits_rows(m, words):
    """numpy reference of `sd3d_pack_mask_bits`: [n_rows, words] uint32 little-endian bit rows of the non-zero bytes, and the counts."""
    m = np.asarray(m) != 0
    n_rows, n_cols = m.shape
    padded = np.zeros((n_rows, words * 32), dtype=bool)
    padded[:, :n_cols] = m
    bits = np.packbits(padded, axis=1, bitorder="little").view("<u4").reshape(n_rows, words)
    return bits, m.sum(1).astype(np.int32)


# ---- cases of sd3d_instance_loss --------------------------------------------------------------------------------------------------------
INST_SHAPES = [  # (Q, S, G, n_cls1): every Q, S and class count of the strides, LOSS_MAX_S at Q = 3
    (1, 1, 1, 2), (65, 33, 5, 257), (1023, 257, 9, 300), (1024, 33, 4, 2), (1025, 3000, 7, 257), (3, 12288, 5, 300),
]


@lru_cache(maxsize=None)
def inst_case(Q, S, G, n_cls1, boxes=True, scores=True):
    """Explicit match with: a query matched to three objects of different labels, an object matched by several queries, a matched pair
    whose predicted box equals the ground truth in one coordinate each, exact-zero logits inside and outside a matched object."""
    c = make_case(500 + Q + 7 * S + 13 * G + n_cls1, Q, S, G, n_cls1, boxes=boxes, scores=scores)
    c.match = random_match(c, 77 + Q + S)
    q0 = 3 % Q
    if G >= 3:
        c.match[q0, :3] = 1                                    # three objects on one query
    for q in (0, Q // 2, Q - 1):
        c.match[q, G - 1] = 1                                  # several queries on one object
    if boxes:
        c.centers[q0, 1] = c.gt_centers[0, 1]                  # zero differences in the box terms
        c.sizes[q0, 2] = c.gt_sizes[0, 2]
    inside = torch.nonzero(c.gt_masks[0])[:2, 0]
    outside = torch.nonzero(~c.gt_masks[0])[:2, 0]
    zero_logits(c, q0, inside)
    zero_logits(c, q0, outside)
    return c


@lru_cache(maxsize=None)
def score_case():
    """Planted IoUs (S = 257, one object per query): 2/3 and 51/101 are kept, 1/2 and 50/101 are not; exact-zero logits decide two
    more: query 4 reaches 3/4 only because its zero logit inside the object counts as inside, query 5 stays at 2/4 only because its
    zero logit outside counts as predicted.  -> case; case.iou = {q: (IoU, kept)}."""
    c = make_case(4242, 8, 257, 6, 19)
    c.match = torch.zeros(c.Q, c.G, dtype=torch.uint8)
    c.iou = {}
    for q, (inside, target, outside) in enumerate([(2, 3, 0), (2, 4, 0), (51, 101, 0), (50, 101, 0)]):
        v = plant_iou(c, q, q, inside, target, outside)
        c.match[q, q] = 1
        c.iou[q] = (v, v > 0.5)
    plant_iou(c, 4, 4, 2, 4, 0)
    zero_logits(c, 4, [2])                                     # inside the object: 3 / 4
    c.match[4, 4] = 1
    c.iou[4] = (0.75, True)
    plant_iou(c, 5, 5, 2, 3, 0)
    zero_logits(c, 5, [200])                                   # outside the object: 2 / (3 + 1)
    c.match[5, 5] = 1
    c.iou[5] = (0.5, False)
    return c


@lru_cache(maxsize=None)
def no_keep_case():
    """Scores present, every matched pair below IoU 0.5 (the matched rows predict nothing): score part 0, score gradient 0."""
    c = make_case(4343, 65, 33, 4, 19)
    c.match = random_match(c, 5, p=0.05)
    rows = c.match.bool().any(1)
    c.masks[rows] = -c.masks[rows].abs() - 0.25
    return c


SAT_LEVELS = (15.0, 30.0, 100.0)


@lru_cache(maxsize=None)
def sat_case(level, agree, ordinary_every=0, Q=65, S=3000, G=5, n_cls1=19):
    """Query q is matched to object q % G alone and its row is +-level: the object's mask (agree) or its inverse.  With
    `ordinary_every` = n every n-th row keeps its ordinary logits: the gradient arrays of sd3d_instance_loss then have entries of their
    usual size next to the saturated ones (rows that agree at +-30 alone make an array of 1e-18s, which no fp32 sigmoid resolves)."""
    c = make_case(int(level) * 10 + int(agree), Q, S, G, n_cls1)
    c.name = f"+-{level:g} {'agree' if agree else 'disagree'} Q{Q} S{S} G{G}" + (f" ordinary rows {ordinary_every}" if ordinary_every else "")
    c.match = torch.zeros(Q, G, dtype=torch.uint8)
    for q in range(Q):
        if not (ordinary_every and q % ordinary_every == 0):
            saturate(c, q, q % G, level, agree)
        c.match[q, q % G] = 1
    c.query_masks[:] = True
    return c
