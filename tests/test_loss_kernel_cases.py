"""tests/loss_kernel_cases.py on the CPU: the conditions the GPU tests of csrc/loss.hip put on their inputs hold, the planted properties are
what they claim in float64 and in the oracle's float32, and the adapters reassemble `unified_criterion` from its pieces exactly."""
import numpy as np
import pytest
import torch

from oracle import loss_ref
from tests import loss_kernel_cases as K
from tests.loss_cases import as_pred, load_case


# ---- conditions on the inputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", K.MATCH_SHAPES)
def test_match_cases_have_gaps_and_their_planted_tie(shape):
    Q, S, G, n_cls1, topk, seed = shape
    c = K.match_case(*shape)
    for dtype in (torch.float64, torch.float32):
        cost = K.oracle_costs(c, dtype, sparse=False)
        assert torch.equal(cost[0], cost[Q - 1])                               # the duplicated query: an exact tie in every column
        col = torch.where(c.query_masks[0], cost[:, 0], torch.full_like(cost[:, 0], K.INF_COST))
        assert set(torch.argsort(col)[:2].tolist()) == {0, Q - 1}              # ... and the two cheapest of column 0
    gap = K.check_gaps(K.oracle_costs(c, sparse=False), c.query_masks, topk)
    print(f"[loss-case-gap] {c.name} topk={topk}: {gap:.3e}")
    assert gap >= K.MIN_GAP
    iq, ig = loss_ref.sparse_match(K.oracle_costs(c, sparse=False), c.query_masks, topk)
    m = K.match_from_indices(iq, ig, Q, G)
    assert int(m[0, 0]) == int(m[Q - 1, 0]) == (0 if topk == 1 else 1)         # at the threshold: neither; below it: both


def test_chain_case_has_gaps():
    t, layers, cfg = K.chain_case()
    gap = K.chain_gap(t, layers, cfg)
    print(f"[loss-case-gap] chain: {gap:.3e}")
    assert gap >= K.MIN_GAP


def test_check_gaps_itself():
    qm = torch.ones(1, 5, dtype=torch.bool)
    cost = torch.tensor([[1.0], [2.0], [2.0], [2.5], [9.0]], dtype=torch.float64)
    assert K.check_gaps(cost, qm, 0) == 1.0                                    # threshold 1: nothing below, 2 above
    assert K.check_gaps(cost, qm, 1) == 0.5                                    # threshold 2 (a tie): 1 below, 2.5 above; the other 2 is no neighbour
    assert K.check_gaps(cost, qm, 2) == 0.5
    assert K.check_gaps(cost, qm, 3) == 0.5                                    # threshold 2.5: 2 below
    qm[0, 4] = False                                                           # 9.0 -> 1e8
    assert K.check_gaps(cost, qm, 4) == 1e8 - 2.5
    assert K.check_gaps(torch.full((5, 1), 3.0, dtype=torch.float64), ~qm | qm, 2) == float("inf")


# ---- planted properties -----------------------------------------------------------------------------------------------------------------
def test_planted_ious_fall_on_their_sides():
    c = K.score_case()
    for dtype in (torch.float64, torch.float32):
        for q, (iou, kept) in c.iou.items():
            got = float(loss_ref._iou(c.masks[q:q + 1].to(dtype), c.gt_masks[q:q + 1].to(dtype)))
            assert abs(got - iou) < 1e-6 and (got > 0.5) == kept, (dtype, q, got, iou)
    assert sorted(v for v, _ in c.iou.values()) == sorted([2 / 3, 1 / 2, 51 / 101, 50 / 101, 3 / 4, 1 / 2])
    # the exact-zero logits binarise to "inside": without them query 4 has 2 / 4 and query 5 has 2 / 3
    assert float(c.masks[4, 2]) == 0.0 and bool(c.gt_masks[4, 2]) and float(c.masks[5, 200]) == 0.0 and not bool(c.gt_masks[5, 200])
    for dtype in (torch.float64, torch.float32):
        assert bool((torch.zeros(1, dtype=dtype).sigmoid() >= 0.5).all())
    parts, _ = K.oracle_instance([c], [c.match], torch.float64, True)
    assert parts[3] > 0


def test_no_keep_case_keeps_nothing():
    c = K.no_keep_case()
    iq, ig = K.indices_from_match(c.match)
    assert iq.numel() > 0
    for dtype in (torch.float64, torch.float32):
        assert float(loss_ref._iou(c.masks[iq].to(dtype), c.gt_masks[ig].to(dtype)).max()) == 0.0


@pytest.mark.parametrize("shape", K.INST_SHAPES)
def test_instance_cases_hold_their_match_shapes(shape):
    Q, S, G, n_cls1 = shape
    c = K.inst_case(*shape)
    per_query, per_object = c.match.sum(1), c.match.sum(0)
    assert int(per_object.min()) >= 1 or Q < G
    if G >= 3:
        q0 = 3 % Q
        assert int(per_query[q0]) >= 3
        if n_cls1 - 1 >= 3:
            assert len(set(c.labels[:3].tolist())) == 3                        # three different labels: the last one is the class target
    if Q >= 3:
        assert int(per_object[G - 1]) >= 3
    q0 = 3 % Q
    assert int((c.masks[q0] == 0).sum()) == min(2, int(c.gt_masks[0].sum())) + min(2, int((~c.gt_masks[0]).sum()))
    assert float(c.centers[q0, 1]) == float(c.gt_centers[0, 1]) and float(c.sizes[q0, 2]) == float(c.gt_sizes[0, 2])


@pytest.mark.parametrize("level", K.SAT_LEVELS)
@pytest.mark.parametrize("agree", [True, False])
def test_saturated_cases(level, agree):
    c = K.sat_case(level, agree)
    assert float(c.masks.abs().min()) >= level and float(c.masks.abs().max()) <= 1.05 * level + 1e-3
    for q in (0, 7, c.Q - 1):
        assert torch.equal(c.masks[q] > 0, c.gt_masks[q % c.G] if agree else ~c.gt_masks[q % c.G])
    assert len(torch.unique(c.masks.abs())) > c.S                              # the magnitudes differ: the row sums are not exact in fp32
    m = K.sat_case(level, agree, 8)                                            # the instance-loss variant: every 8th row ordinary
    assert float(m.masks[0].abs().min()) < 1.0 and float(m.masks[1].abs().min()) >= level and torch.equal(m.masks[1], c.masks[1])


def test_duplicate_query_is_bit_for_bit():
    c = K.make_case(1, 9, 33, 3, 5)
    c.match = K.random_match(c, 1)
    K.duplicate_query(c, 2, 7)
    for k in ("cls", "masks", "scores", "centers", "sizes", "match"):
        assert torch.equal(getattr(c, k)[2], getattr(c, k)[7]), k
    assert torch.equal(c.query_masks[:, 2], c.query_masks[:, 7]) and c.ties == [(2, 7)]


def test_class_rows():
    c = K.cost_case(65, 257, 5, 300)
    assert set(c.cls[0].tolist()) == {80.0, -80.0} and len(set(c.cls[2].tolist())) == 1
    assert int(c.gt_masks[1].sum()) == 0 and int(c.gt_masks[2].sum()) == c.S
    assert torch.equal(c.centers[0], c.gt_centers[0])


# ---- adapters ---------------------------------------------------------------------------------------------------------------------------
def test_match_adapters_round_trip():
    m = (torch.rand(17, 5, generator=torch.Generator().manual_seed(0)) < 0.2).to(torch.uint8)
    iq, ig = K.indices_from_match(m)
    assert torch.equal(K.match_from_indices(iq, ig, 17, 5), m)
    flat = iq * 5 + ig
    assert bool((flat[1:] > flat[:-1]).all())                                  # query-major, objects ascending: the last one is the largest


def test_packbits_rows():
    m = np.zeros((2, 33), dtype=np.uint8)
    m[0, [0, 31, 32]] = (1, 2, 255)
    bits, counts = K.packbits_rows(m, 3)
    assert bits.tolist() == [[0x80000001, 1, 0], [0, 0, 0]] and counts.tolist() == [3, 0]


def test_hand_costs_expectations_hold_in_the_oracle():
    for Q in (1, 63, 64, 65, 200):
        for topk in K.hand_topks(Q):
            cost, expect = K.hand_costs(Q, topk)
            assert torch.equal(cost.double().float(), cost)
            iq, ig = loss_ref.sparse_match(cost.double(), torch.ones(cost.shape[1], Q, dtype=torch.bool), topk)
            m = K.match_from_indices(iq, ig, Q, cost.shape[1])
            iq32, ig32 = loss_ref.sparse_match(cost, torch.ones(cost.shape[1], Q, dtype=torch.bool), topk)
            assert torch.equal(K.match_from_indices(iq32, ig32, Q, cost.shape[1]), m)
            for name, (col, n) in expect.items():
                if n is not None:
                    assert int(m[:, col].sum()) == n, (Q, topk, name)
    assert K.hand_topks(1) == [0] and K.hand_topks(200) == [0, 1, 2, 199]
    names = set(K.hand_costs(200, 2)[1])
    assert {"tie_at_threshold_same_lane", "tie_at_threshold_neighbours", "tie_below_threshold_same_lane", "all_excluded",
            "exactly_topk_admissible", "infinities"} <= names


@pytest.mark.parametrize("name", ["s200", "base"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_pieces_reassemble_the_unified_criterion(name, dtype):
    """match_costs -> sparse_match -> byte matrix -> indices -> instance_layer_loss, layer by layer, plus semantic_loss: the same numbers,
    bit for bit, as `unified_criterion`, and the golden losses within the bounds of tests/test_loss_oracle.py."""
    cfg, targets, layers, exp = load_case(name, dtype)
    ref = loss_ref.unified_criterion(as_pred(layers), targets, cfg)
    n_sem, n_b = cfg["num_semantic_classes"], len(targets)
    cw = list(cfg["cost_weights"]) + [0.0] * (5 - len(cfg["cost_weights"]))
    order = [layers[-1]] + layers[:-1]                                         # the last layer first, then the auxiliary ones
    inst_loss, all_parts = None, []
    for li, layer in enumerate(order):
        cases = [K.case_from_scene(targets[b], layer, b, n_sem) for b in range(n_b)]
        matches = []
        for c in cases:
            cost = K.oracle_costs(c, dtype, weights=cw, sparse=False)
            iq, ig = loss_ref.sparse_match(cost, c.query_masks, cfg["topk"])
            matches.append(K.match_from_indices(iq, ig, c.Q, c.G))
        if li == 0:
            for (iq, ig), (rq, rg) in zip([K.indices_from_match(m) for m in matches], ref["_indices"]):
                assert torch.equal(iq, rq) and torch.equal(ig, rg)
        loss, parts, _ = K.oracle_instance_raw(cases, matches, dtype, last=li == 0, cfg=cfg, requires_grad=False)
        inst_loss = loss if inst_loss is None else inst_loss + loss
        all_parts.append(parts)
    cases = [K.case_from_scene(targets[b], layers[-1], b, n_sem) for b in range(n_b)]
    seg_loss = loss_ref.semantic_loss([c.sem for c in cases], [c.sem_masks for c in cases], cfg["sem_ignore_index"], cfg["sem_loss_weight"])
    assert torch.equal(seg_loss, ref["seg_loss"]) and torch.equal(inst_loss, ref["inst_loss"])
    for mine, theirs in zip(all_parts, ref["_parts"]):
        for a, b in zip(mine, theirs):
            assert torch.equal(a, b)
    assert abs(float(seg_loss) - exp["seg_loss"]) < 2e-6 * max(1.0, abs(exp["seg_loss"]))
    assert abs(float(inst_loss) - exp["inst_loss"]) < 3e-6 * abs(exp["inst_loss"])


# ---- the tolerance rule -----------------------------------------------------------------------------------------------------------------
def test_check_float_rule():
    ref64 = torch.tensor([1.0, 100.0, float("nan")], dtype=torch.float64)
    ref32 = ref64 + torch.tensor([1e-7, 0.0, 0.0], dtype=torch.float64)
    scale = torch.tensor([1.0, 100.0, 1.0])
    bound, e32 = K.float_bound(ref64, ref32, scale)
    assert abs(e32 - 1e-7) < 1e-12 and bound == 8 * K.ULP32
    K.check_float("rule", "inside", ref64 + torch.tensor([9e-7, 9e-5, 0.0]), ref64, ref32, scale)
    with pytest.raises(AssertionError):
        K.check_float("rule", "outside", ref64 + torch.tensor([1e-6, 0.0, 0.0]), ref64, ref32, scale)
    with pytest.raises(AssertionError):
        K.check_float("rule", "nan set", torch.tensor([1.0, 100.0, 0.0]), ref64, ref32, scale)
    with pytest.raises(AssertionError):                                        # inside 4 x e32 but beyond 2e-5 of the largest entry
        K.check_float("rule", "cap", torch.tensor([1.0, 100.003]), ref64[:2], ref64[:2] + torch.tensor([0.0, 1e-3]), scale[:2])
