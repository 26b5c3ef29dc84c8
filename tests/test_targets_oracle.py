"""tests/targets_ref.py (the CPU restatement the GPU tests compare against) pinned to tests/golden/targets.npz, which the
reference's own dataset classes and preparer produced (tests/golden/make_golden_targets.py).  Exact equality throughout."""
import os

import numpy as np
import pytest

from targets_ref import coherent_scene, targets_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(ds, k, view) for ds in ("scannet200", "scannet") for k in (0, 1) for view in ("train", "val")]


def load_fixture():
    return np.load(os.path.join(HERE, "golden", "targets.npz"))


def dataset_spec(Z, ds):
    """(lut, n_classes, swap_2_3) of a fixture dataset, built the way the reference builds them."""
    if ds == "scannet200":
        return Z["scannet200/lut"], 200, True
    lut = np.full(42, 20, dtype=np.int64)
    lut[Z["scannet/valid_cat_ids"]] = np.arange(20)
    return lut, 20, False


def expected(Z, key):
    out = {}
    for name in ("masks", "sp_inst_sem_masks"):
        shape = tuple(Z[f"{key}/{name}_shape"])
        out[name] = np.unpackbits(Z[f"{key}/{name}"])[: int(np.prod(shape))].reshape(shape).astype(bool)
    for name in ("labels", "area", "iscrowd", "orig_size", "size"):
        out[name] = Z[f"{key}/{name}"]
    return out


@pytest.mark.parametrize("ds,k,view", CASES)
def test_restatement_equals_the_reference_fixture(ds, k, view):
    Z = load_fixture()
    lut, C, swap = dataset_spec(Z, ds)
    got = targets_ref(Z[f"{ds}/s{k}/instance_mask"], Z[f"{ds}/s{k}/semantic_mask"], Z[f"{ds}/s{k}/super_points"], lut, C, (0, 1), swap, view)
    exp = expected(Z, f"{ds}/s{k}/{view}")
    for name, e in exp.items():
        assert got[name].shape == e.shape, (name, got[name].shape, e.shape)
        assert got[name].dtype == e.dtype, (name, got[name].dtype, e.dtype)
        assert np.array_equal(got[name], e), name
    assert exp["masks"].shape[0] > 0 and exp["sp_inst_sem_masks"][: -(C + 1)].sum() > 20       # the fixture is not degenerate


def test_fixture_covers_the_quirk_and_the_views():
    """Scene 1 has no background point: one instance fewer than distinct raw ids; val rows = train rows + present stuff classes."""
    Z = load_fixture()
    for ds in ("scannet200", "scannet"):
        lut, C, swap = dataset_spec(Z, ds)
        assert len(np.unique(Z[f"{ds}/s1/instance_mask"])) == len(Z[f"{ds}/s1/train/labels"]) + 1
        assert len(Z[f"{ds}/s0/val/labels"]) == len(Z[f"{ds}/s0/train/labels"]) + 2
        assert tuple(Z[f"{ds}/s0/val/labels"][:2]) == (0, 1)
        assert Z[f"{ds}/s0/val/sp_inst_sem_masks_shape"][0] == len(Z[f"{ds}/s0/train/labels"]) + C + 1
    assert list(Z["scannet200/s0/train/strings"]) == ["scene0000_00", "scannet200_InstanceSeg3D:0", "cdn", "text"]
    assert list(Z["scannet/s1/val/strings"]) == ["scene0001_00", "scannet_train_mask3d:1", "None", "text"]


def test_integer_majority_equals_the_float_vote():
    """2 k > n decides what the restatement's fp32 `scatter_mean > 0.5` decides, also for superpoints split exactly in half."""
    inst, sem, sp = coherent_scene(3)
    lut = np.arange(42) % 21
    got = targets_ref(inst, sem, sp, lut, 20)["sp_inst_sem_masks"]
    cls = lut[sem]
    S = sp.max() + 1
    for c in range(21):
        k = np.bincount(sp[cls == c], minlength=S)
        n = np.bincount(sp, minlength=S)
        own = 2 * k > n
        if c == 20:
            own |= ~np.stack([2 * np.bincount(sp[cls == d], minlength=S) > n for d in range(21)]).any(0)
        assert np.array_equal(got[got.shape[0] - 21 + c], own), c


def test_label_spec_constructors():
    from segdino3d_amd.targets import LabelSpec
    Z = load_fixture()
    s200 = LabelSpec.scannet200(Z["scannet200/lut"])
    assert (s200.n_classes, s200.bg_class_id, s200.stuff_ids, s200.swap_2_3, s200.loss_branch) == (200, 200, (0, 1), True, "cdn")
    assert np.array_equal(s200.seg_label_mapping.numpy(), Z["scannet200/lut"])
    s20 = LabelSpec.scannet(Z["scannet/valid_cat_ids"])
    assert np.array_equal(s20.seg_label_mapping.numpy(), dataset_spec(Z, "scannet")[0]) and not s20.swap_2_3 and s20.loss_branch is None
    with pytest.raises(ValueError):
        LabelSpec(20, np.array([0, 21]))                       # a class above the background class
    with pytest.raises(ValueError):
        LabelSpec.scannet([1, 2, 3])


def test_cpu_tensors_are_refused():
    import torch
    from segdino3d_amd.targets import LabelSpec, build_targets
    z = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        build_targets(z, z, z, LabelSpec(20, np.arange(21)), "train")
