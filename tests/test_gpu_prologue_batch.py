"""The forward prologue at batch sizes: the radix sort with per-pass digit bases, the hierarchy kernel maps that stage each parent's
neighbourhood once per workgroup, and pair lists built from the block counts the map kernel leaves.  Integer work: everything is
compared bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RS_TILE = 2048          # csrc/sort_scan.hip: keys per workgroup of a digit pass
RS_BASES_MIN_NB = 32    # ... and the tile count above which a pass reduces the histogram once (rs_bases) instead of in every workgroup


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------
# sort
# ------------------------------------------------------------------------------------------------
def _sort_keys(n, seed):
    g = torch.Generator().manual_seed(seed)
    keys = torch.randint(0, 1 << 50, (n,), generator=g, dtype=torch.int64)
    keys[::3] = keys[0]                                   # a third of the keys are one value, spread over every tile
    keys[n // 4:n // 4 + min(n // 2, 5000)] = keys[1]     # and one long contiguous run (several tiles at the larger sizes)
    vals = torch.randint(0, 1 << 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    return keys, vals


_SORT_SIZES = [4097, 3 * RS_TILE + 1, 40_000,
               RS_BASES_MIN_NB * RS_TILE, RS_BASES_MIN_NB * RS_TILE + 1]      # the last tile count of the per-workgroup walk, the first of rs_bases


@pytest.mark.parametrize("n", _SORT_SIZES)
def test_sort_matches_stable_cpu_sort(n):
    from segdino3d_amd import ops
    d = dev()
    keys, vals = _sort_keys(n, n)
    for b, e in ((0, 20), (0, 48), (3, 35)):              # 3, 6 and 4 digit passes; none of the ranges ends on a digit
        masked = (keys >> b) & ((1 << (e - b)) - 1)
        order = torch.sort(masked, stable=True)[1]
        for with_vals in (False, True):
            sk, sv = ops.sort_pairs(keys.to(d).clone(), vals.to(d).clone() if with_vals else None, b, e)
            assert torch.equal(sk.cpu(), keys[order]), f"keys differ: n={n} bits=[{b},{e}) vals={with_vals}"
            want = vals[order] if with_vals else order.to(torch.int32)
            assert torch.equal(sv.cpu().to(torch.int32), want), f"values / stability differ: n={n} bits=[{b},{e}) vals={with_vals}"


def test_sort_histogram_rows_longer_than_one_scan_round():
    """More than 2048 tiles: a digit's histogram row takes more than one 2048-entry round of the workgroup that reduces it."""
    from segdino3d_amd import ops
    d = dev()
    n = 2048 * RS_TILE + 1
    keys, _ = _sort_keys(n, 7)
    masked = keys & ((1 << 20) - 1)
    order = torch.sort(masked, stable=True)[1]
    sk, sv = ops.sort_pairs(keys.to(d).clone(), None, 0, 20)
    assert torch.equal(sk.cpu(), keys[order])
    assert torch.equal(sv.cpu().to(torch.int32), order.to(torch.int32))


# ------------------------------------------------------------------------------------------------
# hierarchy maps + block counts
# ------------------------------------------------------------------------------------------------
def _points_of(coords):
    c = torch.as_tensor(np.unique(coords, axis=0), dtype=torch.float32)
    return torch.cat([(c + 0.5) * 0.02, torch.rand(c.shape[0], 3, generator=torch.Generator().manual_seed(1))], 1)


def _grid(lo, w):
    r = np.arange(lo, lo + w)
    return np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)


def _scene_coords():
    """Two scenes of one point per voxel (integer voxel coordinates).  A: a filled 9^3 block at an odd corner (its interior voxels find all
    125 neighbours; its faces cut sibling groups), a sprinkle around it (irregular sibling groups), one voxel far from everything.  B:
    smaller, and it shares the block's corner region and the far voxel with A."""
    rng = np.random.RandomState(3)
    far = np.array([[60, 61, 62]])
    a = np.concatenate([_grid(3, 9), rng.randint(0, 26, (700, 3)), far])
    b = np.concatenate([_grid(3, 6), rng.randint(0, 14, (250, 3)), far])
    return a, b


@pytest.fixture(scope="module")
def built():
    """Per case ("a", "b": one scene each; "ab": the batch of both): the maps through the hierarchy with block counts, the hash-probed
    maps, and the level arrays.  Built once, read by every test below."""
    from segdino3d_amd import ops, sparse
    from segdino3d_amd.sparse import BatchSceneMaps, SceneMaps, inv27_table, offsets_device
    d = dev()
    ca, cb = _scene_coords()
    pa, pb = _points_of(ca).to(d), _points_of(cb).to(d)
    out = {}
    for name in ("a", "b", "ab"):
        def make():
            return BatchSceneMaps([pa, pb], 0.02, 3) if name == "ab" else SceneMaps(pa if name == "a" else pb, 0.02, 3)
        m = make()
        L = len(m.keys)
        pc = torch.zeros(L + 1, 64, dtype=torch.int32, device=d)
        counts = {}
        nbr3, nbr5, _ = ops.kernel_maps_hier(m.keys, m.parents, m.n_vox, offsets_device(3, m.order, d), offsets_device(5, m.order, d),
                                             inv27_table(m.order), pc, block_counts=counts)
        old = sparse.HIER_MAPS
        sparse.HIER_MAPS = False                              # the hash-probe path (ops.kernel_map)
        try:
            h = make()
            probed = {(l, 3): h.same(l, 3) for l in range(L)}
            probed[(0, 5)] = h.same(0, 5)
            assert h._hash and not h._hier_built
        finally:
            sparse.HIER_MAPS = old
        tables = {(l, 3): nbr3[l] for l in range(L)}
        tables[(0, 5)] = nbr5
        out[name] = dict(maps=m, tables=tables, probed=probed, pair_counts=pc, counts=counts, points=(pa, pb))
    return out


def test_scenes_hold_the_cases_they_are_built_for(built):
    for name, lo, hi in (("a", 300, 2000), ("b", 300, 2000)):
        m = built[name]["maps"]
        assert len(m.n_vox) == 3 and lo <= m.n_vox[0] <= hi, m.n_vox
    for name in ("a", "b", "ab"):
        m, t = built[name]["maps"], built[name]["tables"]
        assert all(n % 256 for n in m.n_vox), m.n_vox
        assert m.n_vox[0] > 256, "more than one workgroup on level 0"
        n5 = (t[(0, 5)] >= 0).sum(0)
        assert int(n5.max()) == 125, "a voxel inside a filled 5^3 block"
        assert int(n5.min()) == 1 and int((t[(0, 3)] >= 0).sum(0).min()) == 1, "a voxel whose only entry is itself"
    split = [int(l) for l in (0, 1) for m in [built["ab"]["maps"]] for r in range(256, m.n_vox[l], 256)
             if int(m.parents[l][r - 1]) == int(m.parents[l][r])]
    assert split, "no sibling group crosses a 256-row boundary"
    assert built["a"]["maps"].n_vox[0] != built["b"]["maps"].n_vox[0]


@pytest.mark.parametrize("name", ["a", "b", "ab"])
def test_hierarchy_maps_equal_the_hash_probed_maps(built, name):
    b = built[name]
    L = len(b["maps"].keys)
    for key, t in b["tables"].items():
        assert torch.equal(t, b["probed"][key]), key
        row = L if key[1] == 5 else key[0]
        assert int(b["pair_counts"][row].sum()) == int((t >= 0).sum()), key


@pytest.mark.parametrize("name", ["a", "b"])
def test_hierarchy_maps_equal_the_oracle(built, name):
    from oracle import sparse_ref as R
    from helpers import device_level_coords, match_rows, pairs_from_nbr
    b = built[name]
    m = b["maps"]
    pts = b["points"][0 if name == "a" else 1].cpu()
    uc, _ = R.unique_voxels(R.floor_voxel(pts[:, :3], 0.02))
    lv = R.MinkLevels(uc)
    for (l, k), t in b["tables"].items():
        perm = match_rows(device_level_coords(m, l), lv.coords[1 << l])
        got = [set(zip(perm[i].tolist(), perm[o].tolist())) for (i, o) in pairs_from_nbr(t)]
        ref = [set(zip(i.tolist(), o.tolist())) for (i, o) in lv.same(1 << l, k)]
        assert got == ref, (l, k)


def test_batch_tables_are_the_scenes_tables_side_by_side(built):
    """No entry crosses scenes: the batch's table is scene A's, then scene B's with its rows shifted by A's row count."""
    a, b, ab = built["a"], built["b"], built["ab"]
    for key in ab["tables"]:
        na = a["maps"].n_vox[key[0]]
        tb = b["tables"][key]
        want = torch.cat([a["tables"][key], torch.where(tb >= 0, tb + na, tb)], 1)
        assert torch.equal(ab["tables"][key], want), key
        scene = ab["maps"].keys[key[0]] >> 48
        t = ab["tables"][key]
        src = scene[t.clamp(min=0).long()]
        assert bool(((src == scene[None, :]) | (t < 0)).all()), key


@pytest.mark.parametrize("name", ["a", "ab"])
def test_block_counts_are_the_count_pass(built, name):
    """counts[k, b] = entries of offset k in rows [256 b, 256 b + 256): what the row-block count pass (`pair_count_rows_body`) computes."""
    b = built[name]
    L = len(b["maps"].keys)
    assert set(b["counts"]) == {(l, 3) for l in range(L - 1)} | {(0, 5)}
    for key, c in b["counts"].items():
        t = b["tables"][key]
        K, M = t.shape
        nblk = (M + 255) // 256
        hit = torch.zeros(K, nblk * 256, dtype=torch.int32, device=t.device)
        hit[:, :M] = (t >= 0).to(torch.int32)
        assert torch.equal(c, hit.view(K, nblk, 256).sum(2).to(torch.int32)), key


def _real(pl):
    """The written part of lean lists: the real tiles, their offsets and the tile count (the capacity behind them stays unwritten)."""
    nt = int(pl.tile_k[pl.p_cap // 128])
    return nt, pl.in_idx[:nt * 128], pl.tile_k[:nt], None if pl.out_idx is None else pl.out_idx[:nt * 128]


def _rlist_equal(a, b):
    """Per-row lists {count, list positions}: the count and the first `count` positions of every row (the rest of a row is not written)."""
    if a is None or b is None:
        return a is None and b is None
    live = torch.arange(a.shape[1] - 1, device=a.device)[None, :] < a[:, :1]
    return torch.equal(a[:, 0], b[:, 0]) and bool(((a[:, 1:] == b[:, 1:]) | ~live).all())


@pytest.mark.parametrize("name", ["a", "ab"])
@pytest.mark.parametrize("key", [(0, 5), (0, 3), (1, 3)])
@pytest.mark.parametrize("direct", [False, True])
def test_lists_from_block_counts_equal_lists_from_the_count_launch(built, name, key, direct):
    """Lean plain lists of a 5^3 and of 3^3 tables, from the map kernel's counts and from the builder's own count launch: in_idx, tile_k,
    the tile count, rlist (direct=False) / out_idx (direct=True: the builder's other optional product) are identical."""
    from segdino3d_amd import ops
    b = built[name]
    t = b["tables"][key]
    n_pairs = int((t >= 0).sum())
    counts = b["counts"][key].clone()                       # (consumed by the build: the fixture's tensor stays as it is)
    with_counts, = ops.pair_lists_batch([(t, n_pairs, -1, direct, True, counts)])
    with_launch, = ops.pair_lists_batch([(t, n_pairs, -1, direct, True)])
    # ... and mixed in one call with a table that counts for itself (its workgroups are numbered without the other's)
    other = b["tables"][(1, 3) if key != (1, 3) else (0, 3)]
    mixed = ops.pair_lists_batch([(other, int((other >= 0).sum()), -1, False, True),
                                  (t, n_pairs, -1, direct, True, b["counts"][key].clone()),
                                  (other, int((other >= 0).sum()), -1, False, True)])
    ref_other, = ops.pair_lists_batch([(other, int((other >= 0).sum()), -1, False, True)])
    n_other = int((other >= 0).sum())
    for got, want, pairs in ((with_counts, with_launch, n_pairs), (mixed[1], with_launch, n_pairs), (mixed[0], ref_other, n_other),
                             (mixed[2], ref_other, n_other)):
        (gn, gi, gt, go), (wn, wi, wt, wo) = _real(got), _real(want)
        assert gn == wn and int((gi >= 0).sum()) == pairs
        assert torch.equal(gi, wi) and torch.equal(gt, wt)
        assert (go is None) == (wo is None) and (go is None or torch.equal(go, wo))
        assert _rlist_equal(got.rlist, want.rlist)


def test_counts_are_refused_where_the_builder_cannot_take_them(built):
    from segdino3d_amd import ops
    b = built["a"]
    t = b["tables"][(0, 3)]
    n_pairs = int((t >= 0).sum())
    with pytest.raises(ValueError, match="block counts"):
        ops.pair_lists_batch([(t, n_pairs, -1, False, False, b["counts"][(0, 3)].clone())])              # with a position table
    with pytest.raises(ValueError, match="block counts"):
        ops.pair_lists_batch([(t, n_pairs, ops.PAIR_CHAINED, False, True, b["counts"][(0, 3)].clone())])  # chained
