"""The host side of `eval_ap_scene.SceneApAccumulator` without a device: the state rows (pack, merge, parse on CPU tensors), the scene
keys, and the dictionary `scene_results` builds from tables."""
import numpy as np
import pytest
import torch

VALID = (2, 3, 4)
LABELS = ("chair", "table", "door")


def _new(**kw):
    from segdino3d_amd import eval_ap_scene
    return eval_ap_scene.SceneApAccumulator(VALID, LABELS, groups={}, **kw)


def _scenes(seed, keys, slot_counts, n_counters, sentinel):
    g = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(slot_counts)])
    counters = torch.from_numpy(g.integers(0, 50, (len(keys), n_counters)))
    codes = g.integers(0, sentinel, int(offsets[-1]))
    codes[g.random(len(codes)) < 0.3] = sentinel                               # slots without an entry
    return list(keys), offsets, counters, torch.from_numpy(codes)


def test_state_rows_pack_merge_and_parse_on_cpu_tensors():
    from segdino3d_amd.eval_ap_scene import SceneApAccumulator as S
    acc = _new()
    n, W = acc.n_counters, acc.STATE_WIDTH
    assert n == 3 * 10 + 6 and acc.sentinel == 30 << 33
    # slot counts on both sides of a row of W - 2 codes, and none at all
    a = _scenes(1, [40, 7, 2 ** 31 - 1], [W - 2, 0, 5], n, acc.sentinel)
    b = _scenes(2, [8, 0], [2 * (W - 2) + 1, 13], n, acc.sentinel)
    sa = S._pack(*a, torch.tensor([4]))
    sb = S._pack(*b, torch.tensor([16]))
    empty = _new().state()
    for s in (sa, sb, empty):
        assert s.dtype == torch.float64 and s.dim() == 2 and s.shape[1] == W and float(s.max()) < 2.0 ** 53
    assert empty.shape[0] == 1 and sa.shape[0] == 1 + 3 + 2 and sb.shape[0] == 1 + 2 + 4
    rows = torch.cat([sa, empty, sb])
    rows = rows[torch.randperm(rows.shape[0], generator=torch.Generator().manual_seed(3))]
    merged = S.merge([rows[:5], rows[5:]])
    assert merged.shape == (1 + 5 + 6, W) and merged[0, 0] == 3 and merged[0, 1] == 20
    for state in (merged, rows):
        keys, offsets, codes, counters, status = acc._parse_scenes(state)
        assert status == 4 | 16
        assert keys.tolist() == [0, 7, 8, 40, 2 ** 31 - 1]
        assert np.diff(offsets).tolist() == [W - 2, 0, 3 * (W - 2), W - 2, W - 2]
        assert codes.dtype == torch.int64 and counters.dtype == torch.int64 and counters.shape == (5, n)
        for src in (a, b):
            for s, key in enumerate(src[0]):
                at = keys.tolist().index(key)
                assert torch.equal(counters[at], src[2][s])
                mine = codes[offsets[at]:offsets[at + 1]]
                want = src[3][src[1][s]:src[1][s + 1]]
                assert (mine[mine != acc.sentinel].sort().values.tolist() == want[want != acc.sentinel].sort().values.tolist())
    with pytest.raises(ValueError, match="scene key 7 is present in two states"):
        S.merge([sa, sb, sa])
    with pytest.raises(ValueError, match="present in two states"):
        acc._parse_scenes(torch.cat([sa, sa]))
    with pytest.raises(ValueError, match="entry rows of a scene without counter rows"):
        acc._parse_scenes(sb[sb[:, 0] != 4])
    other = S((2, 3), ("a", "b"), options=dict(overlaps=np.array([0.5])))
    with pytest.raises(ValueError, match="do not belong to an accumulator of this shape"):
        S(tuple(range(200)), tuple(str(i) for i in range(200)))._parse_scenes(sa)
    assert other.mask50 == 1 and other.mask25 == 0 and acc.mask50 == 1 and acc.mask25 == 1 << 9


def test_scene_keys_are_checked_on_the_host_before_anything_else():
    acc = _new()
    cpu = (torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), torch.zeros(1, 4, dtype=torch.bool),
           torch.zeros(1, dtype=torch.int64), torch.zeros(1))
    for bad in (-1, 2 ** 31, 1.5, "3", None, True):
        with pytest.raises(ValueError, match="scene_key"):
            acc.add_scene(*cpu, bad)
        with pytest.raises(ValueError, match="scene_key"):
            acc.add(dict(pts_semantic_mask=cpu[0], pts_instance_mask=cpu[1]), dict(pts_instance_mask=[cpu[2]], instance_labels=cpu[3],
                                                                                 instance_scores=cpu[4]), bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                  # a good key: the tensors are looked at next
        acc.add_scene(*cpu, np.int64(2 ** 31 - 1))
    assert acc._keys == [] and acc._offsets == [0]
    acc._record(12)                                                            # what a successful add leaves
    with pytest.raises(ValueError, match="scene_key 12 was added before"):
        acc.add_scene(*cpu, 12)


def test_ops_refuse_cpu_tensors():
    from segdino3d_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ap_finish_scenes(torch.zeros(4, dtype=torch.int64), [0, 4], 3, 10, torch.zeros(1, 36, dtype=torch.int64), 1, 512)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ap_reduce_counters(torch.zeros(2, 36, dtype=torch.int64), 3, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ap_reduce_counters(torch.zeros(0, 36, dtype=torch.int64), 3, 10)


def test_scene_results_from_hand_made_tables():
    from segdino3d_amd import eval_ap
    acc = _new()
    g = np.random.default_rng(0)
    keys = np.array([2, 5, 9])
    ap, pr_rc = g.random((3, 3, 10)), g.random((2, 3, 3, 10))
    ap[1, 2] = np.nan
    ap[2] = np.nan
    pr_rc[:, 2] = np.nan
    got = acc.results_from_tables(keys, ap, pr_rc, names={2: "scene0002_00", 9: "scene0009_01"})
    assert list(got) == ["scene0002_00", 5, "scene0009_01"]
    for s, name in enumerate(got):
        d = got[name]
        assert set(d) == {"all_ap", "all_ap_50%", "all_ap_25%", "all_prec_50%", "all_rec_50%", "classes"}
        assert set(d["classes"]) == set(LABELS) and set(d["classes"]["door"]) == {"ap", "ap50%", "ap25%", "prec50%", "rec50%"}
        want = eval_ap.compute_averages(ap[s:s + 1], pr_rc[:, s], acc.options, LABELS, {})
        assert all(np.array_equal(d[k], want[k], equal_nan=True) for k in want if k != "classes")
    assert abs(got["scene0002_00"]["all_ap_50%"] - np.mean(ap[0, :, 0])) < 1e-15 and got["scene0002_00"]["classes"]["table"]["ap25%"] == ap[0, 1, 9]
    assert np.isnan(got[5]["classes"]["door"]["ap"]) and np.isfinite(got[5]["all_ap"]) and np.isnan(got["scene0009_01"]["all_ap"])
