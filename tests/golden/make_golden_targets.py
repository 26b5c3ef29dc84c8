"""Generates tests/golden/targets.npz by running the REFERENCE's own dataset classes - ScanNet200InstanceSeg3D and
ScanNetInstanceSeg3D (/root/reference/segdino3d/datasets/dataset/{scannet200,scannet}.py), train and val - followed by its
InstanceSeg3DDataPreparer (datasets/preparer/instance_seg_3d_preparer.py) on seeded synthetic scene files written to a temporary
directory, with /root/reference as the working directory (scannet200.py loads its lookup table from there).  Runs in the build
container only; the fixture it writes is data: the inputs, the lookup tables, the expected target fields and, from a dataset with
dropout_rate_2dfeats = 0.7, the indices numpy.random.choice drew under three seeds.
Third-party imports of those files are stubbed: the `segdino3d` package root (registries whose decorators return the class,
`build_transform` = the reference's preparer) and torch_scatter.scatter_mean (an fp32 index_add_ sum divided by clamp(count, 1),
which is what the library computes for float input)."""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class _Registry:
    def register_module(self, *a, **k):
        return lambda f: f


def scatter_mean(src, index, dim=0):
    assert dim == 0 and src.dtype == torch.float32
    size = int(index.max()) + 1
    out = torch.zeros(size, src.shape[1], dtype=src.dtype).index_add_(0, index, src)
    count = torch.zeros(size, dtype=src.dtype).index_add_(0, index, torch.ones(index.shape[0], dtype=src.dtype))
    return out / count.clamp(min=1)[:, None]


_stub("torch_scatter", scatter_mean=scatter_mean)
_PREP = {}
seg = _stub("segdino3d", DATASETS=_Registry(), PREPARERS=_Registry(), build_transform=lambda cfg: _PREP["prep"])
seg.__path__ = []
_load("segdino3d.gtypes", f"{REF}/segdino3d/gtypes.py")
P = _load("segdino3d.datasets.preparer.instance_seg_3d_preparer", f"{REF}/segdino3d/datasets/preparer/instance_seg_3d_preparer.py")
_PREP["prep"] = P.InstanceSeg3DDataPreparer()
D200 = _load("segdino3d.datasets.dataset.scannet200", f"{REF}/segdino3d/datasets/dataset/scannet200.py")
D20 = _load("segdino3d.datasets.dataset.scannet", f"{REF}/segdino3d/datasets/dataset/scannet.py")


def scene_labels(seed, n, n_sp, n_inst, raw_inst_classes, raw_rest, frac_noise=0.08, frac_rest=0.3):
    """Mostly coherent superpoints: each belongs to one instance (one raw class per instance, sparse raw instance ids) or to "the rest"
    (walls, floor, unlabeled: one raw class per superpoint, raw instance ids of their own or -1); some points carry another label."""
    g = np.random.default_rng(seed)
    sp = g.integers(0, n_sp, n)
    sp[:n_sp] = np.arange(n_sp)
    owner = g.integers(0, n_inst, n_sp)
    rest = g.random(n_sp) < frac_rest
    raw_id_of = np.sort(g.choice(4 * n_inst, n_inst, replace=False)) + 1
    cls_of = g.choice(raw_inst_classes, n_inst)
    inst_sp = np.where(rest, np.where(g.random(n_sp) < 0.5, -1, 4 * n_inst + 7 + g.integers(0, 3, n_sp)), raw_id_of[owner])
    sem_sp = np.where(rest, g.choice(raw_rest, n_sp), cls_of[owner])
    inst, sem = inst_sp[sp], sem_sp[sp]
    noisy = g.random(n) < frac_noise
    other = g.integers(0, n_sp, n)
    inst[noisy], sem[noisy] = inst_sp[other[noisy]], sem_sp[other[noisy]]
    return inst.astype(np.int64), sem.astype(np.int64), sp.astype(np.int64)


def write_scene(root, feats_root, sid, inst, sem, sp, m, seed):
    g = np.random.default_rng(seed + 1000)
    n = len(inst)
    for sub in ("points", "instance_mask", "semantic_mask", "super_points", "meta_data"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    g.random((n, 6)).astype(np.float32).tofile(os.path.join(root, "points", f"{sid}.bin"))
    inst.tofile(os.path.join(root, "instance_mask", f"{sid}.bin"))
    sem.tofile(os.path.join(root, "semantic_mask", f"{sid}.bin"))
    sp.tofile(os.path.join(root, "super_points", f"{sid}.bin"))
    os.makedirs(feats_root, exist_ok=True)
    torch.save([torch.zeros(n, 2), torch.ones(n, 2)], os.path.join(feats_root, f"{sid}.pth"))
    torch.save(torch.arange(m, dtype=torch.float32)[:, None].repeat(1, 2), os.path.join(feats_root, f"{sid}_query_feats.pth"))
    torch.save(torch.arange(m, dtype=torch.float32)[:, None].repeat(1, 3), os.path.join(feats_root, f"{sid}_query_3dctr.pth"))


def record(blob, key, target):
    t = target
    blob[f"{key}/masks"] = np.packbits(t["masks"].numpy().astype(bool), axis=None)
    blob[f"{key}/masks_shape"] = np.array(t["masks"].shape)
    blob[f"{key}/labels"] = t["labels"].numpy()
    blob[f"{key}/area"] = t["area"].numpy()
    blob[f"{key}/iscrowd"] = t["iscrowd"].numpy()
    blob[f"{key}/sp_inst_sem_masks"] = np.packbits(t["sp_inst_sem_masks"].numpy().astype(bool), axis=None)
    blob[f"{key}/sp_inst_sem_masks_shape"] = np.array(t["sp_inst_sem_masks"].shape)
    blob[f"{key}/orig_size"], blob[f"{key}/size"] = t["orig_size"].numpy(), t["size"].numpy()
    blob[f"{key}/strings"] = np.array([str(t["scene_id"]), str(t["data_source"]), str(getattr(t, "loss_branch", None)), str(t["prompt_type"])])
    assert t["masks"].dtype == torch.bool and t["labels"].dtype == torch.int64 and t["area"].dtype == torch.int64


def main():
    os.chdir(REF)
    lut200 = np.load("scannet200_seg_label_mapping.npy", allow_pickle=True)
    lut20 = D20.ScanNetInstanceSeg3D.get_seg_label_mapping(types.SimpleNamespace(bg_class_id=20))
    valid20 = np.array([int(np.nonzero(lut20 == c)[0][0]) for c in range(20)])                          # the 20 valid raw ids, in class order
    fg200 = np.nonzero((lut200 >= 0) & (lut200 < 200))[0]
    bg200 = np.nonzero(lut200 == 200)[0]
    g = np.random.default_rng(7)
    datasets = {
        # raw classes of instances (stuff raw ids 1..3 among them: the 2 <-> 3 swap and stuff-class instances), raw classes of the rest
        "scannet200": (D200.ScanNet200InstanceSeg3D, np.concatenate([[1, 2, 3], g.choice(fg200[fg200 > 3], 30, replace=False)]),
                       np.array([1, 3, 0, int(bg200[-1]), 2])),
        "scannet": (D20.ScanNetInstanceSeg3D, np.concatenate([valid20[:2], valid20]), np.array([1, 2, 0, 13, 40, 3])),
    }
    blob = {"scannet200/lut": lut200.astype(np.int64), "scannet/valid_cat_ids": valid20}
    M = 37
    with tempfile.TemporaryDirectory() as tmp:
        for name, (cls, raw_cls, raw_rest) in datasets.items():
            root, feats = os.path.join(tmp, name), os.path.join(tmp, name + "_2d")
            # scene 0: ordinary; scene 1: no background point at all (the smallest instance becomes -1) and a gap in the superpoint ids
            scenes = []
            inst, sem, sp = scene_labels(11, 4000, 120, 24, raw_cls, raw_rest)
            scenes.append((inst, sem, sp))
            inst, sem, sp = scene_labels(12, 3901, 90, 17, raw_cls[4:], raw_rest, frac_rest=0.0)
            sp[sp >= 40] += 5
            scenes.append((inst, sem, sp))
            ids = [f"scene{k:04d}_00" for k in range(len(scenes))]
            for k, (inst, sem, sp) in enumerate(scenes):
                write_scene(root, feats, ids[k], inst, sem, sp, M, k)
                blob[f"{name}/s{k}/instance_mask"], blob[f"{name}/s{k}/semantic_mask"], blob[f"{name}/s{k}/super_points"] = inst, sem, sp
            for split in ("train", "val"):
                with open(os.path.join(root, "meta_data", f"scannetv2_{split}.txt"), "w") as f:
                    f.write("\n".join(ids) + "\n")
                ds = cls(split, root, use_super_points=True, root_points_2dfeats=feats, transform_cfg={})
                for k in range(len(scenes)):
                    _, tgt = ds[k]
                    record(blob, f"{name}/s{k}/{split}", tgt)
                    print(name, k, split, "G", tuple(tgt["masks"].shape), "sp", tuple(tgt["sp_inst_sem_masks"].shape),
                          "true votes", int(tgt["sp_inst_sem_masks"][: -(ds.bg_class_id + 1)].sum()), "labels", tgt["labels"][:6].tolist())
            if name == "scannet200":
                assert np.array_equal(ds.seg_label_mapping, lut200)
                drop = cls("train", root, use_super_points=True, root_points_2dfeats=feats, transform_cfg={}, dropout_rate_2dfeats=0.7)
                for seed in (0, 1, 2):
                    np.random.seed(seed)
                    _, tgt = drop[0]
                    blob[f"dropout/seed{seed}"] = tgt["extra_features"]["query2d_pos"][:, 0].numpy().astype(np.int64)
                blob["dropout/M"], blob["dropout/rate"] = np.array(M), np.array(0.7)
            else:
                assert np.array_equal(ds.seg_label_mapping[valid20], np.arange(20))
    path = os.path.join(HERE, "targets.npz")
    np.savez_compressed(path, **blob)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
