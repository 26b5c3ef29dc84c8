"""tests/post_ref.py (the restatements the GPU kernel tests compare against) pinned to `oracle.postprocess_ref` on the CPU:
the pieces, reassembled, must give what the oracle gives - discrete outputs exactly, scores to 1e-5 relative (fp32 oracle against
the float64 pieces).  Also here: the conditions of the GPU chain test, which need no GPU."""
import dataclasses

import numpy as np
import pytest
import torch

import post_ref as R
from oracle import postprocess_ref as P

# (seed, Q, C, grid, N, n_peaked, cfg): two small scenes; the second has one stuff class list of its own and no score normalisation
SCENES = [
    (1, 14, 18, (5, 6), 1501, 10, P.TestCfg(topk_insts=60, npoint_thr=20)),
    (2, 20, 7, (4, 9), 2003, 13, P.TestCfg(topk_insts=90, npoint_thr=35, pan_score_thr=0.3, stuff_classes=[3, 0, 5])),
]
CHAIN = R.CHAIN


def _scene(i):
    seed, Q, C, grid, N, n_peaked, cfg = SCENES[i]
    return R.chain_scene(seed, Q, C, grid, N, n_peaked), C, cfg


def _same_instances(ref, got):
    assert ref["scores"].shape[0] == got["scores"].shape[0] >= 5
    assert torch.equal(ref["labels"], got["labels"])
    assert torch.equal(ref["record"], got["record"])
    assert np.array_equal(ref["masks"].numpy().astype(np.uint8), got["masks"])
    assert R.max_rel_err(ref["scores"], got["scores"]) <= 1e-5


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("kernel", ["linear", "gaussian"])
@pytest.mark.parametrize("box_filter", [False, True])
def test_reassembled_instances_equal_the_oracle(i, kernel, box_filter):
    s, C, cfg = _scene(i)
    cfg = dataclasses.replace(cfg, matrix_nms_kernel=kernel)
    args = (s["cls_preds"], s["masks"], s["superpoints"], s["points"][:, :3], s["centers"], s["sizes"], C, cfg)
    for thr in (cfg.inst_score_thr, cfg.pan_score_thr):
        ref = P.predict_instance(*args, thr, box_filter)
        _same_instances(ref, R.predict_instance_ref(*args, thr, box_filter))
    if box_filter:
        assert ref["masks"].sum() < P.predict_instance(*args, thr, False)["masks"].sum()        # the filter cuts something


def test_reassembled_instances_without_nms_and_normalisation():
    s, C, cfg = _scene(0)
    cfg = dataclasses.replace(cfg, nms=False, obj_normalization=False)
    args = (s["cls_preds"], s["masks"], s["superpoints"], s["points"][:, :3], s["centers"], s["sizes"], C, cfg)
    _same_instances(P.predict_instance(*args, 0.0, True), R.predict_instance_ref(*args, 0.0, True))


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("query_num", [-1, 200])
def test_reassembled_semantic_and_panoptic_equal_the_oracle(i, query_num):
    s, C, cfg = _scene(i)
    sp = s["superpoints"]
    am = R.row_argmax_ref(s["sem_preds"], ncols=s["sem_preds"].shape[1] - 1)
    sem = am[sp] if query_num == -1 else am[torch.zeros_like(sp)]
    assert torch.equal(sem, P.predict_semantic(s["sem_preds"], sp, None, query_num))
    args = (s["cls_preds"], s["sem_preds"], s["masks"], sp, s["points"][:, :3], s["centers"], s["sizes"], C, cfg, True, query_num)
    ref_sem, ref_inst = P.predict_panoptic(*args)
    got_sem, got_inst = R.predict_panoptic_ref(*args)
    assert np.array_equal(ref_sem.numpy(), got_sem) and np.array_equal(ref_inst.numpy(), got_inst)
    assert len(np.unique(got_inst)) > len(cfg.stuff_classes) + 2                                  # some instances are painted


@pytest.mark.parametrize("kernel,sigma", [("linear", 2.0), ("gaussian", 2.0), ("gaussian", 0.5)])
@pytest.mark.parametrize("n,S", [(17, 40), (130, 96)])
def test_nms_decay_piece_equals_matrix_nms(kernel, sigma, n, S):
    """`matrix_nms` on sigmoid rows == first sort, `nms_decay_ref` on the fp32 intersection matrix, second sort."""
    g = torch.Generator().manual_seed(n)
    masks = torch.rand(n, S, generator=g)
    labels = torch.randint(0, 5, (n,), generator=g)
    scores = torch.rand(n, generator=g)
    ref_scores, ref_labels, _, ref_record, _ = P.matrix_nms(masks, labels, scores, kernel=kernel, sigma=sigma)
    order = torch.sort(scores, descending=True)[1]
    m = masks[order]
    decayed = R.nms_decay_ref(m @ m.t(), m.sum(1), labels[order], scores[order], kernel, sigma)
    order2 = torch.sort(decayed, descending=True, stable=True)[1]
    assert torch.equal(order[order2], ref_record) and torch.equal(labels[order][order2], ref_labels)
    assert R.max_rel_err(ref_scores, decayed[order2]) <= 1e-5
    # something is decayed: U(0,1) rows have IoU about 1/3, the mildest kernel gives exp(-0.5 / 9) = 0.946 there
    assert float((decayed / scores[order].double()).min()) < 0.97


def test_argmax_piece_returns_the_first_maximum_and_the_first_nan():
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([[1.0, 3.0, 3.0, 2.0], [nan, nan, nan, nan], [5.0, nan, 7.0, nan], [-inf, -inf, -inf, -inf]])
    assert R.row_argmax_ref(x).tolist() == [1, 0, 1, 0]
    assert R.row_argmax_ref(x, ncols=1).tolist() == [0, 0, 0, 0]
    assert R.row_argmax_ref(x, cols=[3, 2, 1]).tolist() == [1, 0, 0, 0]


def test_expand_piece_edges():
    """Out-of-range superpoint ids give 0, a value equal to the threshold is not set, a point on a box face is inside."""
    thr = np.float32(0.4)
    sig = np.array([[0.5, thr, np.nextafter(thr, np.float32(1))]], dtype=np.float32)
    sp = np.array([0, 1, 2, -1, 3, 0])
    pts = np.array([[1.0, 1, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1], [2.25, 1, 1]], dtype=np.float32)
    m, c = R.expand_masks_ref(sig, [0], sp, pts, thr)
    assert m.tolist() == [[1, 0, 1, 0, 0, 1]] and c.tolist() == [3]
    box = np.array([[1.0, 1, 1, 1, 1, 1]], dtype=np.float32)                                      # faces at 1 +- 1.25
    m, c = R.expand_masks_ref(sig, [0], sp, pts, thr, box)
    assert m.tolist() == [[1, 0, 1, 0, 0, 1]] and c.tolist() == [3]
    pts[5, 0] = np.nextafter(np.float32(2.25), np.float32(3))
    assert R.expand_masks_ref(sig, [0], sp, pts, thr, box)[0].tolist() == [[1, 0, 1, 0, 0, 0]]


@pytest.mark.parametrize("kernel", ["linear", "gaussian"])
@pytest.mark.parametrize("query_num", [-1, 200])
def test_chain_scene_meets_the_conditions_of_the_gpu_chain_test(kernel, query_num):
    """The constructed decoder outputs of `test_gpu_post_kernels.py::test_chain_*`: >= 10 panoptic candidates, >= 3 demoted by NMS,
    scores apart from each other and from the thresholds by > 1e-3 relative, no logit / sigmoid within 1e-4 of its threshold."""
    cfg = P.TestCfg(matrix_nms_kernel=kernel)
    res, m = R.chain_conditions(P, R.chain_scene(**CHAIN), CHAIN["C"], cfg, True, query_num)
    print(f"[chain conditions, {kernel}] {m}")
    assert len(np.unique(res["pts_instance_mask"][1].numpy())) > 8
