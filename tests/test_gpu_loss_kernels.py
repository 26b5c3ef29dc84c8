"""The five C entry points of `segdino3d_amd/csrc/loss.hip` - sd3d_pack_mask_bits, sd3d_match_costs, sd3d_sparse_match, sd3d_instance_loss,
sd3d_semantic_loss - called directly through ctypes (so that the leading dimensions can differ from the widths), each against the float64
oracle `oracle/loss_ref.py` of the same operation, at the sizes the launch geometry cares about: 256 threads over S and the class columns,
64 lanes over Q in the matcher, 1024 threads over Q in the target / final kernels, 4 waves over G in the cost kernel, 32-bit mask words,
and LOSS_MAX_S = 12288.

Inputs, planted situations, adapters and the tolerance rule live in tests/loss_kernel_cases.py (checked on the CPU by
tests/test_loss_kernel_cases.py).  Discrete outputs - bit rows, counts, match bytes, matched / kept counts, excluded costs - are exact.
Float outputs: `check_float`, whose bound comes from the fp32 evaluation of the oracle on the CPU.  Every output buffer carries 64
sentinel elements behind its end which must come back untouched; padded input columns hold NaN (bytes: 255), so a read behind a row
shows.  Every case prints a `[loss-kernel-error]` line; profiles/loss_kernel_errors.md holds the table."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import loss_ref
from tests import loss_kernel_cases as K
from tests.helpers import Out, wide
from tests.loss_kernel_cases import check_float

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32


def _dev():
    return torch.device("cuda:0")


def _ids(shape):
    return "-".join(str(v) for v in shape)


def _lib():
    from segdino3d_amd import _lib as L
    return L, L.load()


def _stream():
    from segdino3d_amd import ops
    return ops._stream()


def up(t):
    return None if t is None else t.contiguous().to(_dev())


def ptr(t):
    return None if t is None else t.data_ptr()


# ---- sd3d_pack_mask_bits ------------------------------------------------------------------------------------------------------------------
def pack(m_dev, ld, n_rows, n_cols, words):
    L, lib = _lib()
    bits, counts = Out(max(n_rows, 1) * words, torch.int32), Out(max(n_rows, 1), torch.int32)
    rc = lib.sd3d_pack_mask_bits(m_dev.data_ptr(), ld, n_rows, n_cols, bits.ptr, words, counts.ptr, _stream())
    return rc, bits, counts


@pytest.mark.parametrize("n_cols", [1, 31, 32, 33, 255, 256, 257, 8193])
def test_pack_mask_bits(n_cols):
    L, lib = _lib()
    need = (n_cols + 31) // 32
    for n_rows in (1, 5):
        for pad, extra in ((0, 0), (3, 0), (0, 2), (5, 300)):
            g = torch.Generator().manual_seed(n_cols + 10 * n_rows + pad + extra)
            m = torch.tensor([0, 1, 2, 255], dtype=torch.uint8)[torch.randint(0, 4, (n_rows, n_cols), generator=g)]
            m[0, n_cols - 1] = 2                                            # the last column counts, with a byte that is not 1
            if n_rows > 1:
                m[1] = 0
                m[2] = 255
            dm, ld = wide(m, pad, 255)                                      # bytes behind the row are non-zero: reading them sets bits
            words = need + extra
            rc, bits, counts = pack(dm, ld, n_rows, n_cols, words)
            L.check(rc, "pack_mask_bits")
            ref_bits, ref_counts = K.packbits_rows(m.numpy(), words)
            got = bits.get(n_rows, words).numpy().view(np.uint32)
            assert np.array_equal(got, ref_bits), (n_rows, n_cols, pad, extra)
            assert np.array_equal(counts.get(n_rows).numpy(), ref_counts)
            assert not got[:, need:].any()                                  # words beyond the row: 0
            if n_cols % 32:
                assert not (got[:, need - 1] >> (n_cols % 32)).any()        # unused high bits of the last word: 0
    m = torch.ones(2, n_cols, dtype=torch.uint8)
    rc, bits, counts = pack(up(m), n_cols, 0, n_cols, need)                 # no rows: nothing happens
    assert rc == 0 and bits.untouched() and counts.untouched()
    rc, bits, counts = pack(up(m), n_cols, 2, n_cols, need - 1)             # too few words: refused
    assert rc != 0 and bits.untouched() and counts.untouched()
    with pytest.raises(RuntimeError):
        L.check(rc, "pack_mask_bits")


class Truth:
    """Ground truth of a case on the device, packed by the kernel under test (and compared with numpy on the way)."""

    def __init__(self, c, pad=0):
        L, lib = _lib()
        self.words = (c.S + 31) // 32 + (1 if pad else 0)
        gm = c.gt_masks.to(torch.uint8)
        self.n = max(c.G, 1)
        if c.G:
            rc, bits, counts = pack(up(gm), c.S, c.G, c.S, self.words)
            L.check(rc, "pack_mask_bits")
            ref_bits, ref_counts = K.packbits_rows(gm.numpy(), self.words)
            assert np.array_equal(bits.get(c.G, self.words).numpy().view(np.uint32), ref_bits)
            assert np.array_equal(counts.get(c.G).numpy(), ref_counts)
            self.bits, self.count = bits.buf, counts.buf
        else:
            self.bits = torch.zeros(self.words, dtype=torch.int32, device=_dev())
            self.count = torch.zeros(1, dtype=torch.int32, device=_dev())
        self.labels = up(c.labels) if c.G else torch.zeros(1, dtype=torch.int64, device=_dev())
        if c.G:
            self.gc, self.ld_gc = wide(c.gt_centers, pad)
            self.gs, self.ld_gs = wide(c.gt_sizes, 2 * pad)
        else:
            self.gc = self.gs = torch.zeros(1, 3, device=_dev())
            self.ld_gc = self.ld_gs = 3
        self.qm = up(c.query_masks.to(torch.uint8))


# ---- sd3d_match_costs ---------------------------------------------------------------------------------------------------------------------
def device_costs(c, sparse=True, boxes=True, weights=None, pad=0, truth=None):
    """-> (rc, Out) of sd3d_match_costs on case c; `pad` widens every leading dimension."""
    L, lib = _lib()
    th = truth or Truth(c, pad)
    cls, ld_cls = wide(c.cls, pad)
    masks, ld_masks = wide(c.masks, 3 * pad)
    ctr, size = (up(c.centers), up(c.sizes)) if boxes else (None, None)
    cost = Out(c.Q * c.G)
    w5 = (ctypes.c_float * 5)(*(weights or K.COST_WEIGHTS))
    rc = lib.sd3d_match_costs(cls.data_ptr(), ld_cls, c.n_cls1, masks.data_ptr(), ld_masks, c.Q, c.S, ptr(ctr), ptr(size), th.labels.data_ptr(),
                              th.bits.data_ptr(), th.words, th.count.data_ptr(), c.G, th.gc.data_ptr(), th.ld_gc, th.gs.data_ptr(), th.ld_gs,
                              th.qm.data_ptr() if sparse else None, w5, cost.ptr, _stream())
    torch.cuda.synchronize()
    return rc, cost


def check_costs(family, c, sparse=True, boxes=True, weights=None, pad=0):
    L, lib = _lib()
    rc, cost = device_costs(c, sparse, boxes, weights, pad)
    L.check(rc, "match_costs")
    got = cost.get(c.Q, c.G)
    r64 = K.oracle_costs(c, F64, weights, sparse, boxes)
    r32 = K.oracle_costs(c, F32, weights, sparse, boxes)
    scale = K.cost_scale(c, weights, boxes)
    excluded = r64 == K.INF_COST
    if sparse:
        assert torch.equal(excluded, ~c.query_masks.T)
        assert bool((got[excluded] == np.float32(1e8)).all())               # excluded pairs: exactly 1e8
    else:
        assert not bool(excluded.any())
    keep = ~excluded
    case = f"{c.name} sparse={int(sparse)} boxes={int(boxes)} pad={pad}" + (f" w={weights}" if weights else "")
    if bool(keep.any()):
        check_float(family, case, got[keep], r64[keep], r32[keep], scale[keep])
    return got


@pytest.mark.parametrize("shape", K.COST_SHAPES, ids=_ids)
def test_match_costs(shape):
    c = K.cost_case(*shape)
    check_costs("match_costs", c, sparse=True, boxes=True, pad=0)
    got = check_costs("match_costs", c, sparse=False, boxes=True, pad=2)    # the Hungarian route; every leading dimension wider than its row
    assert bool(torch.isfinite(got).all())
    check_costs("match_costs", c, sparse=True, boxes=False, pad=1)          # no predicted boxes
    check_costs("match_costs", c, sparse=False, boxes=True, weights=[0.5, 1.0, 1.0, 0.0, 0.5])      # centres present, w_ctr = 0
    check_costs("match_costs", c, sparse=False, boxes=True, weights=[0.0, 1.0, 0.0, 0.0, 0.0])      # the BCE term alone
    check_costs("match_costs", c, sparse=False, boxes=True, weights=[0.0, 0.0, 1.0, 0.0, 0.0])      # the dice term alone


def test_match_costs_objects_are_told_apart():
    """Distinct masks, labels and boxes: every column of the cost matrix differs from every other, in the oracle and on the device."""
    c = K.cost_case(65, 257, 67, 300)
    got = check_costs("match_costs", c, sparse=False)
    r64 = K.oracle_costs(c, F64, sparse=False)
    d = (r64[:, :, None] - r64[:, None, :]).abs().amax(0) + torch.eye(c.G) * 1e9
    assert float(d.min()) > 1e-3
    dg = (got.double()[:, :, None] - got.double()[:, None, :]).abs().amax(0) + torch.eye(c.G) * 1e9
    assert float(dg.min()) > 1e-3


def test_match_costs_at_the_largest_superpoint_count():
    L, lib = _lib()
    c = K.make_case(12288, 3, 12288, 5, 19)
    check_costs("match_costs", c, sparse=True, pad=0)
    check_costs("match_costs", c, sparse=False, pad=1)
    big = K.make_case(12289, 3, 12289, 5, 19)                               # one more superpoint than the LDS staging holds: refused
    rc, cost = device_costs(big)
    assert rc != 0 and cost.untouched()
    with pytest.raises(RuntimeError, match="superpoint"):
        L.check(rc, "match_costs")


@pytest.mark.parametrize("level", K.SAT_LEVELS)
@pytest.mark.parametrize("agree", [True, False], ids=["agree", "disagree"])
def test_match_costs_saturated(level, agree):
    """Rows of +-level against the object they repeat (agree) or invert, with all five terms and with the BCE term alone.  The agreeing
    rows are where `(sum softplus(x) - sum_t x) / S` cancels: that form was off by 1.76 (+-15) and 1.4e7 (+-30) of the BCE-alone cost
    and by 1.26e-6 of the scale at +-100 with all terms (bounds 1.6e-6 and 1.1e-6); the sum of non-negative terms the kernel uses now
    measures 1.4e-7, 1.1e-7 and 2.0e-7 (profiles/loss_kernel_errors.md)."""
    c = K.sat_case(level, agree)
    check_costs("match_costs saturated", c, sparse=False)
    check_costs("match_costs saturated", c, sparse=False, boxes=False, weights=[0.0, 1.0, 0.0, 0.0, 0.0])


# ---- sd3d_sparse_match --------------------------------------------------------------------------------------------------------------------
def device_match(cost_dev, Q, G, topk):
    L, lib = _lib()
    match = Out(Q * G, torch.uint8)
    rc = lib.sd3d_sparse_match(cost_dev.data_ptr(), Q, G, topk, match.ptr, _stream())
    torch.cuda.synchronize()
    return rc, match


@pytest.mark.parametrize("Q", [1, 63, 64, 65, 200])
def test_sparse_match_hand_built(Q):
    L, lib = _lib()
    for topk in K.hand_topks(Q):
        cost, expect = K.hand_costs(Q, topk)
        G = cost.shape[1]
        rc, match = device_match(up(cost), Q, G, topk)
        L.check(rc, "sparse_match")
        got = match.get(Q, G)
        iq, ig = loss_ref.sparse_match(cost.double(), torch.ones(G, Q, dtype=torch.bool), topk)
        ref = K.match_from_indices(iq, ig, Q, G)
        for name, (col, n) in expect.items():
            assert torch.equal(got[:, col], ref[:, col]), (Q, topk, name, got[:, col].nonzero().flatten().tolist(), ref[:, col].nonzero().flatten().tolist())
            if n is not None:
                assert int(got[:, col].sum()) == n, (Q, topk, name)
    rc, match = device_match(up(cost), Q, G, Q)                             # topk + 1 > Q: refused
    assert rc != 0 and match.untouched()
    with pytest.raises(RuntimeError, match="topk"):
        L.check(rc, "sparse_match")


@pytest.mark.parametrize("shape", K.MATCH_SHAPES, ids=_ids)
def test_sparse_match_on_device_costs(shape):
    L, lib = _lib()
    Q, S, G, n_cls1, topk, seed = shape
    c = K.match_case(*shape)
    c64 = K.oracle_costs(c, F64, sparse=False)
    gap = K.check_gaps(c64, c.query_masks, topk)
    assert gap >= K.MIN_GAP, gap                                            # a condition on the inputs (also checked on the CPU)
    rc, cost = device_costs(c, sparse=True)
    L.check(rc, "match_costs")
    rc, match = device_match(cost.buf, Q, G, topk)
    L.check(rc, "sparse_match")
    iq, ig = loss_ref.sparse_match(c64, c.query_masks, topk)
    ref = K.match_from_indices(iq, ig, Q, G)
    got = match.get(Q, G)
    assert torch.equal(got, ref)
    got_cost = cost.get(Q, G)
    assert torch.equal(got_cost[0], got_cost[Q - 1])                        # the duplicated query: bit-identical costs, an exact tie
    assert int(got[0, 0]) == int(got[Q - 1, 0]) == (0 if topk == 1 else 1)


# ---- sd3d_instance_loss -------------------------------------------------------------------------------------------------------------------
def criterion_for(c, cfg=None):
    from segdino3d_amd.criterion import InstanceCriterion
    cfg = cfg or K.cfg_for(c)
    names = ["QueryClassificationCost", "MaskBCECost", "MaskDiceCost", "CenterL1Cost", "SizeL1Cost"]
    matcher = dict(type="SparseMatcher", topk=cfg["topk"], costs=[dict(type=t, weight=w) for t, w in zip(names, cfg["cost_weights"])])
    return InstanceCriterion(matcher=matcher, loss_weight=cfg["loss_weight"], non_object_weight=cfg["non_object_weight"],
                             num_classes=cfg["num_classes"], fix_dice_loss_weight=cfg["fix_dice_loss_weight"], iter_matcher=cfg["iter_matcher"],
                             fix_mean_loss=cfg["fix_mean_loss"])


def device_instance(c, match, coef6, pad=0, ws_short=0):
    """-> (rc, dict of Out) of sd3d_instance_loss.  Outputs for predictions the case does not have are passed all the same and must stay untouched."""
    L, lib = _lib()
    th = Truth(c, pad)
    cls, ld_cls = wide(c.cls, pad)
    masks, ld_masks = wide(c.masks, 3 * pad)
    score, ctr, size = up(None if c.scores is None else c.scores.reshape(-1)), up(c.centers), up(c.sizes)
    m = up(match) if c.G else torch.zeros(1, dtype=torch.uint8, device=_dev())
    cw = torch.tensor([1.0] * (c.n_cls1 - 1) + [K.NON_OBJECT_WEIGHT], device=_dev())
    o = dict(cls_preds=Out(c.Q * c.n_cls1), masks=Out(c.Q * c.S), scores=Out(c.Q), centers=Out(c.Q * 3), sizes=Out(c.Q * 3), parts=Out(8))
    ws_bytes = lib.sd3d_instance_loss_ws_bytes(c.Q)
    ws = Out(ws_bytes, torch.uint8)
    c6 = (ctypes.c_float * 6)(*coef6)
    rc = lib.sd3d_instance_loss(cls.data_ptr(), ld_cls, c.n_cls1, masks.data_ptr(), ld_masks, c.Q, c.S, ptr(score), ptr(ctr), ptr(size),
                                th.labels.data_ptr(), th.bits.data_ptr(), th.words, th.count.data_ptr(), c.G, th.gc.data_ptr(), th.ld_gc,
                                th.gs.data_ptr(), th.ld_gs, m.data_ptr(), cw.data_ptr(), c6, o["cls_preds"].ptr, o["masks"].ptr, o["scores"].ptr,
                                o["centers"].ptr, o["sizes"].ptr, o["parts"].ptr, ws.ptr, ws_bytes - ws_short, _stream())
    torch.cuda.synchronize()
    o["ws"] = ws
    return rc, o


SHAPE_OF = dict(cls_preds=lambda c: (c.Q, c.n_cls1), masks=lambda c: (c.Q, c.S), scores=lambda c: (c.Q, 1), centers=lambda c: (c.Q, 3),
                sizes=lambda c: (c.Q, 3))
PRESENT = dict(cls_preds=lambda c: True, masks=lambda c: True, scores=lambda c: c.scores is not None, centers=lambda c: c.centers is not None,
               sizes=lambda c: c.sizes is not None)


def assemble(parts_per_scene, coef, w, has):
    """The six layer terms from the per-scene parts, as `ScanNetUnifiedCriterion.__call__` forms them (float64 on the host)."""
    P = np.asarray(parts_per_scene, dtype=np.float64)
    n_b = P.shape[0]
    return [P[:, 0].mean(), P[:, 1].sum() * coef[1] / w[1], P[:, 2].sum() * coef[2] / w[2], P[:, 3].sum() / n_b if has["scores"] else 0.0,
            P[:, 4].mean() if has["centers"] else 0.0, P[:, 5].mean() if has["sizes"] else 0.0]


def check_instance(family, cases, last, pad=0, cfg=None, twice=False):
    """sd3d_instance_loss on every case (= scene) against one oracle call over all of them."""
    L, lib = _lib()
    cfg = cfg or K.cfg_for(cases[0])
    n_b = len(cases)
    coef = criterion_for(cases[0], cfg).scene_coefficients(n_b, last)
    matches = [c.match for c in cases]
    p64, g64 = K.oracle_instance(cases, matches, F64, last, cfg)
    p32, g32 = K.oracle_instance(cases, matches, F32, last, cfg)
    outs = []
    for c in cases:
        rc, o = device_instance(c, c.match, coef, pad)
        L.check(rc, "instance_loss")
        o["ws"].get(o["ws"].n)                                              # the workspace was not overrun either
        if twice:
            rc, o2 = device_instance(c, c.match, coef, pad)
            L.check(rc, "instance_loss")
            for k in ("cls_preds", "masks", "scores", "centers", "sizes", "parts"):
                assert torch.equal(o[k].buf.view(torch.int32), o2[k].buf.view(torch.int32)), ("second call differs", k)
        outs.append(o)
    name = " + ".join(c.name for c in cases) + f" last={int(last)} pad={pad}"
    parts = [o["parts"].get(8).double().numpy() for o in outs]
    for c, p in zip(cases, parts):                                          # discrete: matched pairs and kept scores
        iq, ig = K.indices_from_match(c.match)
        assert p[6] == float(iq.numel()), (name, p[6], iq.numel())
        kept = 0
        if c.scores is not None and iq.numel():
            kept = int((loss_ref._iou(c.masks[iq].double(), c.gt_masks[ig].double()) > 0.5).sum())
        assert p[7] == float(kept), (name, p[7], kept)
    has = {k: PRESENT[k](cases[0]) for k in PRESENT}
    got = assemble(parts, coef, cfg["loss_weight"] + [0.0] * (6 - len(cfg["loss_weight"])), has)
    check_float(family, name + " parts", torch.tensor(got), torch.tensor(p64), torch.tensor(p32), torch.tensor(K.part_scales(p64)))
    for i, (c, o) in enumerate(zip(cases, outs)):
        for k in SHAPE_OF:
            if not PRESENT[k](c):
                assert o[k].untouched(), (name, k, "written although the layer does not predict it")
                continue
            g = o[k].get(*SHAPE_OF[k](c))
            assert bool(torch.isfinite(g).all()), (name, k)
            check_float(family, f"{name} scene{i} d_{k}", g, g64[i][k], g32[i][k])
    return parts, outs


@pytest.mark.parametrize("last", [True, False], ids=["last", "aux"])
@pytest.mark.parametrize("shape", K.INST_SHAPES, ids=_ids)
def test_instance_loss(shape, last):
    c = K.inst_case(*shape)
    big = c.Q * c.S > 1_000_000
    check_instance("instance_loss", [c], last, pad=0 if last else 2, twice=last and not big)


def test_instance_loss_class_target_is_the_last_matched_object():
    """Query 3 of the case is matched to objects 0, 1, 2 of three different labels: the class gradient is -k at the label of object 2."""
    c = K.inst_case(65, 33, 5, 257)
    assert int(c.match[3, 3:].sum()) == 0 and len(set(c.labels[:3].tolist())) == 3
    parts, outs = check_instance("instance_loss", [c], True)
    d = outs[0]["cls_preds"].get(c.Q, c.n_cls1)[3]
    assert int(d.argmin()) == int(c.labels[2]) and float(d[c.labels[0]]) > 0 and float(d[c.labels[1]]) > 0


def test_instance_loss_without_scores_or_boxes():
    c = K.inst_case(65, 257, 5, 19, boxes=False, scores=False)
    parts, _ = check_instance("instance_loss", [c], True)
    assert parts[0][3] == 0.0 and parts[0][4] == 0.0 and parts[0][5] == 0.0


def test_instance_loss_planted_ious():
    c = K.score_case()
    for last in (True, False):
        parts, outs = check_instance("instance_loss scores", [c], last)
        assert parts[0][7] == 3.0                                           # 2/3, 51/101 and the 3/4 of the zero logit; not 1/2, 50/101, 2/4
        d = outs[0]["scores"].get(c.Q)
        assert [bool(v != 0) for v in d.tolist()] == [True, False, True, False, True, False, False, False]


def test_instance_loss_no_pair_above_half():
    c = K.no_keep_case()
    parts, outs = check_instance("instance_loss scores", [c], True)
    assert parts[0][3] == 0.0 and parts[0][7] == 0.0 and bool((outs[0]["scores"].get(c.Q) == 0).all())


def test_instance_loss_empty_match_and_no_objects():
    """No matched pair: the mask and box terms are means over nothing - NaN, like the oracle's - and the class gradients stay finite."""
    c = K.make_case(31, 65, 33, 4, 19)
    c.match = torch.zeros(c.Q, c.G, dtype=torch.uint8)
    parts, outs = check_instance("instance_loss empty", [c], True)
    assert np.isnan(parts[0][1]) and np.isnan(parts[0][2]) and np.isfinite(parts[0][0]) and parts[0][6] == 0.0
    assert bool((outs[0]["masks"].get(c.Q, c.S) == 0).all())
    c0 = K.make_case(32, 65, 33, 0, 19)
    c0.match = torch.zeros(c0.Q, 0, dtype=torch.uint8)
    parts, outs = check_instance("instance_loss empty", [c0], False)
    assert np.isnan(parts[0][1]) and np.isfinite(parts[0][0])
    assert float(outs[0]["cls_preds"].get(c0.Q, c0.n_cls1).abs().max()) > 0


def test_instance_loss_two_scenes():
    """Coefficients of a batch of two: two calls with `scene_coefficients(2, last)` against one two-scene oracle call."""
    a, b = K.inst_case(65, 33, 5, 257), K.make_case(2, 65, 257, 9, 257)
    b.match = K.random_match(b, 3, p=0.05)
    for last in (True, False):
        check_instance("instance_loss two scenes", [a, b], last)


@pytest.mark.parametrize("level", K.SAT_LEVELS)
@pytest.mark.parametrize("agree", [True, False], ids=["agree", "disagree"])
def test_instance_loss_saturated(level, agree):
    check_instance("instance_loss saturated", [K.sat_case(level, agree, 8)], True, twice=True)


def test_instance_loss_refusals():
    L, lib = _lib()
    c = K.inst_case(65, 33, 5, 257)
    coef = criterion_for(c).scene_coefficients(1, True)
    rc, o = device_instance(c, c.match, coef, ws_short=1)                   # workspace one byte short
    assert rc != 0 and all(o[k].untouched() for k in o)
    with pytest.raises(RuntimeError, match="workspace"):
        L.check(rc, "instance_loss")
    big = K.make_case(12289, 3, 12289, 2, 5)
    big.match = K.random_match(big, 0)
    rc, o = device_instance(big, big.match, coef)
    assert rc != 0 and all(o[k].untouched() for k in o)


# ---- sd3d_semantic_loss -------------------------------------------------------------------------------------------------------------------
def device_semantic(c, n_logits, pad=0, pad_d=0, loss_weight=0.5, ws_short=0, ld=None):
    L, lib = _lib()
    sem, ld_in = wide(c.sem, pad)
    ld_d = c.C + pad_d
    d_sem, loss = Out(c.Q * ld_d), Out(1)
    ws_bytes = lib.sd3d_semantic_loss_ws_bytes(c.Q)
    ws = Out(ws_bytes, torch.uint8)
    sm = up(c.sem_masks.to(torch.uint8))
    rc = lib.sd3d_semantic_loss(sem.data_ptr(), ld_in if ld is None else ld, c.Q, c.C, n_logits, sm.data_ptr(), c.ignore_index, loss_weight,
                                d_sem.ptr, ld_d, loss.ptr, ws.ptr, ws_bytes - ws_short, _stream())
    torch.cuda.synchronize()
    return rc, d_sem, loss, ws, ld_d


def check_semantic(c, pad=0, pad_d=0, loss_weight=0.5):
    L, lib = _lib()
    n_logits = c.C - 1 if c.ignore_index >= 0 else c.C
    rc, d_sem, loss, ws, ld_d = device_semantic(c, n_logits, pad, pad_d, loss_weight)
    L.check(rc, "semantic_loss")
    ws.get(ws.n)
    l64, g64 = K.oracle_semantic(c, F64, loss_weight)
    l32, g32 = K.oracle_semantic(c, F32, loss_weight)
    name = f"{c.name} ignore={c.ignore_index} ld={c.C + pad} ld_d={ld_d}"
    check_float("semantic_loss", name + " loss", loss.get(1).double() * loss_weight, torch.tensor([l64]), torch.tensor([l32]))
    g = d_sem.get(c.Q, ld_d)
    assert bool(torch.isfinite(g).all())
    assert bool((g[:, n_logits:] == 0).all())                               # columns from n_logits on: zero
    check_float("semantic_loss", name + " d_sem", g[:, :c.C], g64, g32)
    return loss.get(1), g


@pytest.mark.parametrize("C", [2, 21, 201, 257, 300])
@pytest.mark.parametrize("ignore_last", [True, False], ids=["ignore_n", "ignore_none"])
def test_semantic_loss(C, ignore_last):
    for Q in (1, 1023, 1025):
        c = K.make_sem_case(C + Q, Q, C, ignore_last)
        if Q > 1:
            n_set = c.sem_masks.sum(0)
            assert int((n_set == 0).sum()) > 0 and int((n_set > 1).sum()) > 0       # queries with no row set, and with several
            g = torch.Generator().manual_seed(C)
            c.sem[5] = torch.where(torch.rand(C, generator=g) < 0.5, 80.0, -80.0)   # +-80 logits
            c.sem[6, :] = -80.0
            c.sem[6, min(1, C - 2) if ignore_last else C - 1] = 80.0
        else:
            c.sem_masks[:, 0] = False
            c.sem_masks[0, 0] = True                                        # the single query counts (the last class would be ignored)
        check_semantic(c)
        check_semantic(c, pad=3, pad_d=5)


def test_semantic_loss_every_query_ignored():
    c = K.make_sem_case(9, 65, 21, True)
    c.sem_masks[:] = False
    c.sem_masks[c.C - 1] = True
    loss, g = check_semantic(c, pad=1, pad_d=2)
    assert bool(torch.isnan(loss).all()) and bool((g == 0).all())
    l64, _ = K.oracle_semantic(c, F64)
    assert np.isnan(l64)


def test_semantic_loss_refusals():
    c = K.make_sem_case(10, 65, 21, True)
    rc, d_sem, loss, ws, _ = device_semantic(c, c.C - 1, ws_short=1)
    assert rc != 0 and d_sem.untouched() and loss.untouched() and ws.untouched()
    rc, d_sem, loss, ws, _ = device_semantic(c, c.C + 1, pad=4, pad_d=4, ld=c.C)     # n_logits > ld alone (ld_d and the buffers are wide enough)
    assert rc != 0 and d_sem.untouched() and loss.untouched()


# ---- chain --------------------------------------------------------------------------------------------------------------------------------
def test_chain_on_a_saturated_scene():
    """_SceneTruth -> InstanceCriterion.costs / .match / .layer_terms -> ScanNetSemanticCriterion.scene_terms on a 'late training' scene
    (+-15 mask logits that mostly agree with their objects), against `unified_criterion` in float64."""
    from segdino3d_amd.criterion import ScanNetSemanticCriterion, _SceneTruth
    t, layers, cfg = K.chain_case()
    assert K.chain_gap(t, layers, cfg) >= K.MIN_GAP
    d = _dev()
    G, n_sem = int(t["labels"].shape[0]), cfg["num_semantic_classes"]

    def oracle(dtype):
        tt = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in t.items()}
        ll = [{k: [None if v is None else v.to(dtype).clone().requires_grad_(True) for v in lst] for k, lst in layer.items()} for layer in layers]
        pred = dict(ll[-1])
        pred["aux_outputs"] = ll[:-1]
        out = loss_ref.unified_criterion(pred, [tt], cfg)
        (out["seg_loss"] + out["inst_loss"]).backward()
        grads = [{k: (None if layer[k][0] is None else (layer[k][0].grad if layer[k][0].grad is not None else torch.zeros_like(layer[k][0])))
                  for k in layer} for layer in ll]
        return out, grads

    r64, g64 = oracle(F64)
    r32, g32 = oracle(F32)
    ic = criterion_for(None, cfg)
    sc = ScanNetSemanticCriterion(cfg["sem_ignore_index"], cfg["sem_loss_weight"])
    truth = _SceneTruth({k: v.to(d) for k, v in t.items()}, n_sem)
    order = [len(layers) - 1] + list(range(len(layers) - 1))                # the last layer first, as the criterion walks them
    w = cfg["loss_weight"]
    inst_loss = 0.0
    for pos, li in enumerate(order):
        last = pos == 0
        layer = {k: [None if v is None else v.to(d) for v in lst] for k, lst in layers[li].items()}
        m = ic.match(layer, 0, truth).cpu()
        c = K.case_from_scene(t, layers[li], 0, n_sem)
        iq, ig = loss_ref.sparse_match(K.oracle_costs(c, F64, cfg["cost_weights"], sparse=False), c.query_masks, cfg["topk"])
        assert torch.equal(m, K.match_from_indices(iq, ig, c.Q, G)), f"layer {li}: matches differ"
        if last:
            assert torch.equal(iq, r64["_indices"][0][0]) and torch.equal(ig, r64["_indices"][0][1])
        coef = ic.scene_coefficients(1, last)
        parts, grads = ic.layer_terms(layer, 0, truth, m.to(d), coef)
        has = {k: PRESENT[k](c) for k in PRESENT}
        terms = assemble([parts.cpu().double().numpy()], coef, w, has)
        p64, p32 = [float(v) for v in r64["_parts"][pos]], [float(v) for v in r32["_parts"][pos]]
        check_float("chain", f"layer {li} parts", torch.tensor(terms), torch.tensor(p64), torch.tensor(p32), torch.tensor(K.part_scales(p64)))
        inst_loss += sum(wi * ti for wi, ti in zip(w, terms))
        for k in PRESENT:
            if has[k]:
                check_float("chain", f"layer {li} d_{k}", grads[k], g64[li][k], g32[li][k])
    check_float("chain", "inst_loss", torch.tensor([inst_loss]), r64["inst_loss"].detach().reshape(1), r32["inst_loss"].detach().reshape(1))
    loss, grad = sc.scene_terms(layers[-1]["sem_preds"][0].to(d), truth, 1)
    check_float("chain", "seg_loss", loss.cpu().double() * cfg["sem_loss_weight"], r64["seg_loss"].detach().reshape(1), r32["seg_loss"].detach().reshape(1))
    check_float("chain", "d_sem_preds", grad, g64[-1]["sem_preds"], g32[-1]["sem_preds"])
