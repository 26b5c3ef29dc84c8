"""CPU restatement of the label side of the reference's dataset classes, step by step as the reference does it (float one-hot
matrices, an fp32 scatter mean, a Python loop over instances): `scannet200.py:155-193, 243-253, 291-326`, `scannet.py` likewise,
and `instance_seg_3d_preparer.py`.  Test infrastructure: tests/test_targets_oracle.py pins it to the fixture the reference's own
classes produced (tests/golden/targets.npz); the GPU tests compare `segdino3d_amd.targets` against it on further scenes."""
import numpy as np
import torch
import torch.nn.functional as F


def scatter_mean(src: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """torch_scatter.scatter_mean(src, index, dim=0) for float src: an fp32 index_add sum divided by clamp(count, 1)."""
    size = int(index.max()) + 1
    out = torch.zeros(size, src.shape[1], dtype=src.dtype).index_add_(0, index, src)
    count = torch.zeros(size, dtype=src.dtype).index_add_(0, index, torch.ones(index.shape[0], dtype=src.dtype))
    return out / count.clamp(min=1)[:, None]


def targets_ref(instance_mask, semantic_mask, super_points, lut, n_classes, stuff_ids=(0, 1), swap_2_3=False, scene_set="train"):
    """numpy int64 [N] arrays -> dict of numpy arrays: masks [G, N, 1] bool, labels / area / iscrowd [G] int64,
    sp_inst_sem_masks [G' + C + 1, S] bool, orig_size / size [1]."""
    inst = np.asarray(instance_mask, dtype=np.int64).reshape(-1, 1).copy()
    sem = np.asarray(semantic_mask, dtype=np.int64).reshape(-1, 1).copy()
    sp = np.asarray(super_points, dtype=np.int64).reshape(-1)
    lut = np.asarray(lut, dtype=np.int64)
    n_stuff = len(stuff_ids)
    # adjust_class_ids_
    if swap_2_3:
        swapped = sem.copy()
        swapped[sem == 2] = 3
        swapped[sem == 3] = 2
        sem = swapped
    assert sem.min() >= 0 and sem.max() < len(lut), "raw semantic id outside the table"
    sem = lut[sem]
    # exclude_stuffs_
    for c in stuff_ids:
        inst[sem == c] = -1
    inst[sem == n_classes] = -1
    ids = np.unique(inst)
    mapping = np.zeros(inst.max() + 2)
    mapping[ids] = np.arange(len(ids)) - 1
    inst = mapping[inst]                                               # float64, like the reference
    # superpoint votes
    inst_t = torch.LongTensor(inst)
    inst_t[inst_t == -1] = int(inst_t.max() + 1)
    onehot = F.one_hot(inst_t.squeeze(-1))[:, :-1]
    sp_t = torch.tensor(sp)
    sp_inst = scatter_mean(onehot.float(), sp_t) > 0.5
    sem_onehot = F.one_hot(torch.LongTensor(sem).squeeze(-1), num_classes=n_classes + 1)
    sp_sem = scatter_mean(sem_onehot.float(), sp_t) > 0.5
    sp_sem[sp_sem.sum(dim=-1) == 0, -1] = True
    sp_inst_sem = torch.cat([sp_inst, sp_sem], dim=-1)
    # merge_stuffs_
    if scene_set != "train":
        inst[inst != -1] += n_stuff
        for k, c in enumerate(stuff_ids):
            inst[sem == c] = k
    # split_instance_gt + InstanceSeg3DDataPreparer
    inst_t, sem_t = torch.tensor(inst), torch.tensor(sem)
    uniq = torch.unique(inst_t)
    uniq = uniq[uniq >= 0]
    masks, labels, area = [], [], []
    for i in uniq:
        m = inst_t == i
        cat = sem_t[m][0].item()
        if scene_set == "train":
            cat = cat - n_stuff
        masks.append(m)
        labels.append(cat)
        area.append(int(m.sum()))
    N = inst.shape[0]
    masks = torch.stack(masks, dim=0) if masks else torch.zeros(0, N, 1, dtype=torch.bool)
    return dict(masks=masks.numpy(), labels=np.asarray(labels, dtype=np.int64), area=np.asarray(area, dtype=np.int64),
                iscrowd=np.zeros(len(labels), dtype=np.int64), sp_inst_sem_masks=sp_inst_sem.T.contiguous().numpy(),
                orig_size=np.array([N]), size=np.array([N]))


def coherent_scene(seed, n=4099, n_sp=300, n_inst=20, lut_len=42, n_classes=20, frac_noise=0.08, frac_bg=0.15):
    """Seeded labels whose superpoints are mostly coherent (random labels give no majority anywhere): every superpoint belongs to one
    instance or to the background, every instance to one raw class; a fraction of the points gets another instance's label."""
    g = np.random.default_rng(seed)
    sp = g.integers(0, n_sp, n)
    sp[:n_sp] = np.arange(n_sp)                                        # every id occurs
    owner = g.integers(0, n_inst, n_sp)
    owner[g.random(n_sp) < frac_bg] = -1
    inst = owner[sp]
    noisy = g.random(n) < frac_noise
    inst[noisy] = g.integers(-1, n_inst, int(noisy.sum()))
    raw_of = g.integers(0, lut_len, n_inst + 1)                        # raw class per instance; the last entry: background points
    sem = raw_of[inst]
    return inst.astype(np.int64), sem.astype(np.int64), sp.astype(np.int64)
