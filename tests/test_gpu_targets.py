"""Dataset targets on the device (segdino3d_amd/targets.py, csrc/targets.hip) against the reference fixture and the CPU
restatement (tests/targets_ref.py).  Every comparison is exact equality on bool / int outputs."""
import numpy as np
import pytest
import torch

from targets_ref import coherent_scene, targets_ref
from test_targets_oracle import CASES, expected, load_fixture

pytestmark = pytest.mark.gpu

FIELDS = ("masks", "labels", "area", "iscrowd", "sp_inst_sem_masks")
LUT = np.arange(42) % 21                                     # raw id -> class 0..20 (0, 1 stuff, 20 background); raw 2.. 19 are plain classes


def dev():
    return torch.device("cuda:0")


def spec20():
    from segdino3d_amd.targets import LabelSpec
    return LabelSpec(20, LUT, (0, 1), False, "unit", None)


def on_device(inst, sem, sp, spec, view, **kw):
    from segdino3d_amd.targets import build_targets
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev())
    return build_targets(t(inst), t(sem), t(sp), spec, view, **kw)


def assert_equal(tgt, ref, what=""):
    for name in FIELDS:
        got = tgt[name].cpu().numpy()
        assert got.dtype == ref[name].dtype, (what, name, got.dtype)
        assert got.shape == ref[name].shape, (what, name, got.shape, ref[name].shape)
        assert np.array_equal(got, ref[name]), (what, name)
    assert tgt["size"].tolist() == ref["size"].tolist() and tgt["orig_size"].tolist() == ref["orig_size"].tolist()


def check(inst, sem, sp, views=("train", "val"), what=""):
    refs = {}
    for view in views:
        refs[view] = targets_ref(inst, sem, sp, LUT, 20, (0, 1), False, view)
        assert_equal(on_device(inst, sem, sp, spec20(), view), refs[view], (what, view))
    return refs


@pytest.mark.parametrize("ds,k,view", CASES)
def test_fixture_cases(ds, k, view):
    """Both datasets, both views, against what the reference's dataset classes + preparer produced."""
    from segdino3d_amd.targets import LabelSpec
    Z = load_fixture()
    spec = LabelSpec.scannet200(Z["scannet200/lut"]) if ds == "scannet200" else LabelSpec.scannet(Z["scannet/valid_cat_ids"])
    sid = f"scene{k:04d}_00"
    tgt = on_device(Z[f"{ds}/s{k}/instance_mask"], Z[f"{ds}/s{k}/semantic_mask"], Z[f"{ds}/s{k}/super_points"], spec, view, scene_id=sid, index=k)
    assert_equal(tgt, expected(Z, f"{ds}/s{k}/{view}"), (ds, k, view))
    assert [str(tgt["scene_id"]), str(tgt["data_source"]), str(tgt["loss_branch"]), str(tgt["prompt_type"])] == list(Z[f"{ds}/s{k}/{view}/strings"])


def test_exact_half_owns_nothing():
    inst, sem, sp = coherent_scene(1)
    members = np.nonzero(sp == 17)[0]
    members = members[: len(members) // 2 * 2]
    sp[np.setdiff1d(np.nonzero(sp == 17)[0], members)] = 18
    half = len(members) // 2
    assert half >= 2
    inst[members[:half]], inst[members[half:]] = 3, 4
    sem[members[:half]], sem[members[half:]] = 5, 6
    refs = check(inst, sem, sp, what="half")
    col = refs["train"]["sp_inst_sem_masks"][:, 17]
    assert col[:-21].sum() == 0 and col[-21:].tolist() == [False] * 20 + [True]


def test_superpoint_id_gap_and_one_point_superpoints():
    inst, sem, sp = coherent_scene(2)
    sp[sp >= 100] += 7                                          # ids 100..106 have no points
    sp[-10:] = sp.max() + 1 + np.arange(10)                     # ten superpoints of one point each
    refs = check(inst, sem, sp, what="gap")
    empty = refs["train"]["sp_inst_sem_masks"][:, 100:107]
    assert empty[:-1].sum() == 0 and empty[-1].all()


def test_one_superpoint_of_5000_points():
    inst, sem, sp = coherent_scene(3)
    g = np.random.default_rng(0)
    big_inst = np.where(g.random(5000) < 0.55, 2, g.integers(-1, 20, 5000))
    inst, sp = np.concatenate([inst, big_inst]), np.concatenate([sp, np.full(5000, 41)])
    sem = np.concatenate([sem, np.where(big_inst == 2, 7, g.integers(0, 42, 5000))])
    refs = check(inst, sem, sp, what="big")
    assert refs["train"]["sp_inst_sem_masks"][:-21, 41].sum() == 1


def test_70_instances():
    inst, sem, sp = coherent_scene(4, n_inst=70)
    inst[:70], sem[:70] = np.arange(70), 2 + np.arange(70) % 18
    refs = check(inst, sem, sp, what="G70")
    assert refs["train"]["labels"].shape[0] == 70


def test_more_instances_than_the_lds_tables_hold():
    """Above 2048 mask rows area / first index are accumulated in global memory instead of LDS."""
    inst, sem, sp = coherent_scene(5)
    inst = np.arange(len(inst)) % 2101 - 1
    sem = 2 + (inst + 1) % 18
    refs = check(inst, sem, sp, views=("val",), what="G2100")
    assert refs["val"]["labels"].shape[0] == 2100


def test_sparse_raw_instance_ids():
    inst, sem, sp = coherent_scene(6)
    inst = np.where(inst == 0, 3, np.where(inst == 1, 70_000, np.where(inst >= 0, inst + 100, -1)))
    check(inst, sem, sp, what="sparse ids")


def test_no_background_point_keeps_the_quirk():
    inst, sem, sp = coherent_scene(7, frac_bg=0.0)
    inst, sem = np.where(inst < 0, 0, inst) + 5, 2 + sem % 18
    refs = check(inst, sem, sp, what="quirk")
    assert refs["train"]["labels"].shape[0] == len(np.unique(inst)) - 1


def test_no_instance_at_all():
    inst, sem, sp = coherent_scene(8)
    refs = check(inst, np.full_like(sem, 20), sp, what="all background")
    assert refs["train"]["masks"].shape == (0, len(inst), 1) and refs["val"]["masks"].shape[0] == 0
    refs = check(inst, sem % 2, sp, what="all stuff")
    assert refs["train"]["labels"].shape[0] == 0 and refs["val"]["labels"].tolist() == [0, 1]


def test_range_errors_name_the_status():
    inst, sem, sp = coherent_scene(9)
    for bad in (42, -1):
        s = sem.copy()
        s[1234] = bad
        with pytest.raises(RuntimeError, match="status 1.*semantic id"):
            on_device(inst, s, sp, spec20(), "train")
    for bad in (-2, 1 << 20):
        i = inst.copy()
        i[77] = bad
        with pytest.raises(RuntimeError, match="status 2.*instance id"):
            on_device(i, sem, sp, spec20(), "val")
    p = sp.copy()
    p[5] = -3
    with pytest.raises(RuntimeError, match="status 4.*superpoint id"):
        on_device(inst, sem, p, spec20(), "train")
    assert_equal(on_device(inst, sem, sp, spec20(), "train"), targets_ref(inst, sem, sp, LUT, 20), "after the errors")


def test_two_runs_give_identical_bits():
    inst, sem, sp = coherent_scene(10, n_inst=40)
    a, b = on_device(inst, sem, sp, spec20(), "val"), on_device(inst, sem, sp, spec20(), "val")
    for name in FIELDS:
        assert torch.equal(a[name], b[name]), name


def test_cpu_tensors_are_refused():
    from segdino3d_amd import ops
    from segdino3d_amd.targets import build_targets, drop_2d_queries
    from segdino3d_amd.gtypes import GD3DTarget
    z = torch.zeros(16, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        build_targets(z, z, z, spec20(), "train")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.targets_scan(z, z, z, spec20().seg_label_mapping, 20, (0, 1), False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        drop_2d_queries(GD3DTarget(extra_features={"query2d_pos": torch.zeros(5, 3), "query2d_feats": torch.zeros(5, 4)}), 0.7)


def test_drop_2d_queries_draws_the_reference_indices():
    from segdino3d_amd.gtypes import GD3DTarget
    from segdino3d_amd.targets import drop_2d_queries
    Z = load_fixture()
    M, rate = int(Z["dropout/M"]), float(Z["dropout/rate"])
    for seed in (0, 1, 2):
        pos = torch.arange(M, dtype=torch.float32)[:, None].repeat(1, 3).to(dev())
        feats = torch.arange(M, dtype=torch.float32)[:, None].repeat(1, 4).to(dev()) * 2
        tgt = GD3DTarget(extra_features={"query2d_pos": pos, "query2d_feats": feats})
        np.random.seed(seed)
        drop_2d_queries(tgt, rate)
        exp = Z[f"dropout/seed{seed}"]
        assert len(exp) == int(M * (1 - rate))
        assert tgt.extra_features["query2d_pos"][:, 0].cpu().long().tolist() == exp.tolist()
        assert tgt.extra_features["query2d_feats"][:, 3].cpu().long().tolist() == (2 * exp).tolist()
        assert tgt.extra_features["query2d_pos"].is_cuda


def test_eval_ann_info_of_a_val_target():
    from segdino3d_amd.eval_ap import eval_ann_info
    from segdino3d_amd.gtypes import GD3DTarget
    inst, sem, sp = coherent_scene(11)
    ref = targets_ref(inst, sem, sp, LUT, 20, (0, 1), False, "val")
    tgt = on_device(inst, sem, sp, spec20(), "val", target=GD3DTarget(extra_features={"super_point_masks": torch.from_numpy(sp).to(dev())}),
                    scene_id="s")
    ref_t = GD3DTarget(masks=torch.from_numpy(ref["masks"]), labels=torch.from_numpy(ref["labels"]), scene_id="s",
                       extra_features={"super_point_masks": torch.from_numpy(sp)})
    a, b = eval_ann_info(tgt, 20), eval_ann_info(ref_t, 20)
    for key in ("pts_instance_mask", "pts_semantic_mask", "sp_pts_mask"):
        assert torch.equal(a[key].cpu(), b[key]), key
    assert a["lidar_idx"] == b["lidar_idx"] and int(b["pts_instance_mask"].max()) == ref["labels"].shape[0] - 1


# ---------------------------------------------------------------------------------------------- packed files -> prefetcher
def labelled_scene(seed, n_points=20000, n_superpoints=150, n_inst=8, empty=False):
    """A synthetic scene with superpoint-coherent raw labels (identity lookup table over 201 raw ids)."""
    from segdino3d_amd.synth import make_scene
    pts, tgt = make_scene(seed, n_points=n_points, n_superpoints=n_superpoints, n_query2d=20)
    ef = tgt.extra_features
    sp = ef["super_point_masks"]
    g = torch.Generator().manual_seed(seed)
    owner = torch.randint(-1, n_inst, (n_superpoints,), generator=g)
    owner[:n_inst] = torch.arange(n_inst)
    cls_of = torch.cat([torch.randint(2, 200, (n_inst,), generator=g), torch.tensor([1])])      # the rest is floor
    inst, sem = torch.where(owner[sp] >= 0, owner[sp] * 3 + 5, -1), cls_of[owner[sp]]
    if empty:
        sem = torch.full_like(sem, 200)
    return dict(points=pts, super_points=sp, points_2dfeats=ef["points_2dfeats"], query2d_feats=ef["query2d_feats"],
                query2d_pos=ef["query2d_pos"], instance_mask=inst, semantic_mask=sem)


def spec201():
    from segdino3d_amd.targets import LabelSpec
    return LabelSpec(200, np.arange(201), (0, 1), False, "unit", "cdn")


def test_prefetcher_without_labels_keeps_the_placeholder(tmp_path):
    from segdino3d_amd.io_scene import ScenePrefetcher, pack_scene
    scene = labelled_scene(1, n_points=3000, n_superpoints=40)
    path = str(tmp_path / "a.bin")
    pack_scene(path, scene)
    pts, tgt = next(ScenePrefetcher([path], dev(), depth=1, readers=1))
    torch.cuda.synchronize()
    assert torch.equal(tgt["masks"].cpu(), torch.ones(1, 3000, 1, dtype=torch.bool)) and tgt["labels"].cpu().tolist() == [0]
    assert set(tgt.keys()) == {"labels", "size", "positive_map", "scene_id", "data_source", "prompt_type", "loss_branch", "area", "orig_size",
                               "iscrowd", "masks", "extra_features", "gt_instance_mask", "gt_semantic_mask"}
    assert tgt["area"] is None and tgt["size"] is None and tgt["iscrowd"] == 0 and tgt["scene_id"] is None
    assert torch.equal(tgt["gt_instance_mask"].cpu(), scene["instance_mask"]) and torch.equal(pts.cpu(), scene["points"])


def test_prefetcher_skips_scenes_without_instances_in_the_train_view(tmp_path):
    from segdino3d_amd.io_scene import ScenePrefetcher, pack_scene
    paths = []
    for k, empty in enumerate((False, True, False)):
        paths.append(str(tmp_path / f"scene{k}.bin"))
        pack_scene(paths[-1], labelled_scene(k, n_points=3000, n_superpoints=40, empty=empty))
    pf = ScenePrefetcher(paths, dev(), depth=2, readers=2, labels=spec201(), scene_set="train", dropout_rate_2dfeats=0.7)
    out = list(pf)
    assert [t["scene_id"] for _, t in out] == ["scene0", "scene2"] and pf.skipped == 1
    assert [t["data_source"] for _, t in out] == ["unit:0", "unit:2"]
    assert all(t.extra_features["query2d_pos"].shape[0] == int(20 * (1 - 0.7)) for _, t in out)
    val = list(ScenePrefetcher(paths, dev(), depth=2, readers=1, labels=spec201(), scene_set="val"))
    assert len(val) == 3 and val[1][1]["masks"].shape == (0, 3000, 1)


def test_training_losses_from_a_packed_file_equal_those_from_the_restatement(tmp_path):
    """packed file -> ScenePrefetcher(labels, "train") -> forward + criterion: the losses have the bits of a run on the restatement's
    targets moved to the device (same weights, same host RNG state)."""
    import segdino3d_amd as seg
    from segdino3d_amd.configs import scannet200_model_cfg
    from segdino3d_amd.gtypes import GD3DTarget
    from segdino3d_amd.io_scene import ScenePrefetcher, pack_scene
    d = dev()
    scene = labelled_scene(21)
    path = str(tmp_path / "scene21.bin")
    pack_scene(path, scene)
    ref = targets_ref(scene["instance_mask"].numpy(), scene["semantic_mask"].numpy(), scene["super_points"].numpy(), np.arange(201), 200)
    pts, tgt = next(ScenePrefetcher([path], d, depth=1, readers=1, labels=spec201(), scene_set="train"))
    assert_equal(tgt, ref, "prefetcher")
    assert ref["labels"].shape[0] == 8
    torch.manual_seed(0)
    model = seg.build_architecture(scannet200_model_cfg(query_num=-1)).to(d).train()
    ref_tgt = GD3DTarget(masks=torch.from_numpy(ref["masks"]).to(d), labels=torch.from_numpy(ref["labels"]).to(d),
                         sp_inst_sem_masks=torch.from_numpy(ref["sp_inst_sem_masks"]).to(d),
                         extra_features={k: v.clone() for k, v in tgt.extra_features.items()})
    losses = []
    for t in (tgt, ref_tgt):
        torch.manual_seed(7)
        out = model([pts.clone()], [t])
        losses.append({k: out[k].detach().cpu() for k in ("seg_loss", "inst_loss")})
    print("losses from the prefetcher's targets:", {k: float(v) for k, v in losses[0].items()})
    for k in ("seg_loss", "inst_loss"):
        assert torch.isfinite(losses[0][k]).all() and float(losses[0][k]) > 0
        assert torch.equal(losses[0][k], losses[1][k]), (k, losses[0][k], losses[1][k])
