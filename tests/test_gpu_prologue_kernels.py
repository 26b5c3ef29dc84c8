"""The prologue kernels of `segdino3d_amd/csrc/voxel.hip` - scene statistics, voxel keys, the run-length unique per level (with and
without spconv's output-extent clip), stride-2 maps, per-voxel feature means, segment starts, superpoint pooling - each called through
its `segdino3d_amd.ops` wrapper on inputs the test builds itself, against the references of tests/prologue_kernel_cases.py, at the sizes
the launch geometry cares about: 256-thread workgroups and the grid-stride loop of the statistics, runs of equal keys across workgroup
boundaries, voxels of 1 .. 700 points around the four-at-a-time loop of `voxel_mean_body` and both sides of its `ld_out > 320` branch,
superpoints around the 64-point passes and 256-point chunks of `pool_superpoints_kernel`.  The superpoint ids' key builder
`sd3d_keys_from_i64` (`csrc/sort_scan.hip`) is called through ctypes, so that its refusals of NULL pointers can be seen.

Integer outputs are compared exactly; means and sums against the derived bounds of the cases file (`check_bound`, which prints one
`[prologue-kernel-error]` line per float case; profiles/prologue_kernels.md holds the table).  Padded columns and the rows of empty
superpoints must be exactly 0.  Inputs go in contiguous and as row-strided views over NaN-poisoned storage."""
import numpy as np
import pytest
import torch

from oracle import sparse_ref as R
from tests import prologue_kernel_cases as K
from tests.helpers import match_rows, morton_decode_np, wide
from tests.prologue_kernel_cases import check_bound

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _dev():
    return torch.device("cuda:0")


def _ops():
    from segdino3d_amd import ops
    return ops


def up(t):
    """CPU tensor / numpy array -> contiguous device tensor."""
    if t is None:
        return None
    return (torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t.contiguous()).to(_dev())


def strided(t, pad):
    """[R, W] -> the same rows as a view over [R, W + pad] storage whose extra columns hold NaN (pad 0: contiguous)."""
    if pad == 0:
        return up(t)
    full, _ = wide(t, pad)
    return full[:, :t.shape[1]]


def host(t):
    return t.cpu().numpy()


# ---- 1. scene_stats ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", K.STATS_N)
@pytest.mark.parametrize("width,pad", [(6, 0), (9, 0), (6, 3)])
def test_scene_stats(n, width, pad):
    p = K.stats_case(n, width)
    got = _ops().scene_stats(strided(p, pad)).cpu()
    r64, r32 = K.stats_ref(p), K.stats_ref(p, F32)
    assert torch.equal(got[:6], r32[:6]), "min / max are exact"
    check_bound("scene_stats", f"n {n} row of {width + pad} floats", got[6:], r64[6:], r32[6:], K.stats_sum_bound(p))


def test_scene_stats_writes_the_row_it_is_given():
    p = K.stats_case(257, 6)
    buf = torch.full((3, 9), -777.25, device=_dev())
    _ops().scene_stats(up(p), out=buf[1])
    assert torch.equal(buf[1], _ops().scene_stats(up(p))) and bool((buf[0] == -777.25).all()) and bool((buf[2] == -777.25).all())


# ---- 2. voxel_keys -----------------------------------------------------------------------------------------------------------------------
def _device_keys(pts_dev, inv, stats, shift, batch):
    keys, ic, origin, err = _ops().voxel_keys(pts_dev, inv, up(stats), shift_to_min=shift, batch_index=batch)
    torch.cuda.synchronize()
    return host(keys), host(ic), host(origin), int(err.item())


@pytest.mark.parametrize("inv_voxel", K.INV_VOXELS)
@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("pad", [0, 2])
def test_voxel_keys(inv_voxel, shift, pad):
    pts = K.keys_case(inv_voxel)
    stats = K.stats_ref(pts[:, :3], F32)
    ref = K.voxel_keys_ref(pts[:, :3].numpy(), inv_voxel, stats.numpy(), shift, 5)
    keys, ic, origin, err = _device_keys(strided(pts, pad), inv_voxel, stats, shift, 5)
    assert np.array_equal(ic, ref["icoords"]) and np.array_equal(origin, ref["origin"])
    assert np.array_equal(keys, ref["keys"]) and err == ref["flag"] == 0
    assert (origin % 16 == 0).all() and (origin <= ic.min(0) - 32).all()
    assert np.array_equal(morton_decode_np(keys), ic.astype(np.int64) - origin) and ((keys >> K.MORTON_BITS) == 5).all()
    want = R.floor_voxel(pts[:, :3] - pts[:, :3].min(0)[0] if shift else pts[:, :3], float(np.float32(1.0) / np.float32(inv_voxel)))
    assert np.array_equal(ic, want)


def test_voxel_keys_without_icoords_and_with_a_shared_flag():
    ops = _ops()
    pts = K.keys_case(50.0)
    stats = up(K.stats_ref(pts[:, :3], F32))
    keys, ic, origin, err = ops.voxel_keys(up(pts), 50.0, stats, want_icoords=False)
    assert ic is None and np.array_equal(host(keys), K.voxel_keys_ref(pts[:, :3].numpy(), 50.0, host(stats), False, 0)["keys"])
    flag = torch.full((1,), 4, dtype=torch.int32, device=_dev())            # the flag is OR-ed into
    ops.voxel_keys(up(pts), 50.0, stats, err=flag)
    assert int(flag.item()) == 4


@pytest.mark.parametrize("rel,axis,want", [(65536 - 65, 0, 2), (65536 - 64, 0, 3), (65536 - 65, 1, 2), (65536 - 64, 1, 3), (65536 - 65, 2, 2),
                                           (65536 - 64, 2, 3), (2047, 0, 0), (2048, 0, 2), (2047, 1, 0), (2048, 1, 2), (1023, 2, 0), (1024, 2, 2)])
def test_voxel_keys_error_flags_at_their_limits(rel, axis, want):
    """Bit 1: a coordinate 65536 - 64 voxels or more above the key origin; bit 2: a Z-order code of more than 32 bits (bit 10 of z,
    bit 11 of x or y)."""
    pts = K.flag_case(rel, axis)
    stats = K.stats_ref(pts[:, :3], F32)
    ref = K.voxel_keys_ref(pts[:, :3].numpy(), 1.0, stats.numpy(), True, 0)
    keys, ic, origin, err = _device_keys(up(pts), 1.0, stats, True, 0)
    assert origin.tolist() == [-32, -32, -32] and int(ic[1, axis]) + 32 == rel
    assert err == ref["flag"] == want and np.array_equal(keys, ref["keys"])


# ---- 3. unique_sorted, voxel_levels_all, voxelise_scene ---------------- -------------------------------------------------------------------
def _route_per_level(skeys, sidx, L, n_cap=None, n_dev=None):
    """Level 0 and every coarser level by one `unique_sorted` each (the route the clipped levels take)."""
    ops = _ops()
    N = skeys.numel() if n_cap is None else n_cap
    uk, seg, inv, n_prev = ops.unique_sorted(skeys, sidx, N, n_dev, 0, want_seg_start=True, want_map=True, map_size=N)
    keys_l, parents, counts = [uk], [], [n_prev]
    for _ in range(1, L):
        uk, _, par, n_prev = ops.unique_sorted(keys_l[-1], None, N, n_prev, 3, want_seg_start=False, want_map=True)
        keys_l.append(uk)
        parents.append(par)
        counts.append(n_prev)
    return dict(ukeys=keys_l, seg_start=seg, inverse=inv, parents=parents, counts=[int(c.item()) for c in counts])


def _route_all(skeys, sidx, L):
    counts = torch.full((L,), -1, dtype=torch.int32, device=_dev())
    uks, seg, inv, parents = _ops().voxel_levels_all(skeys, sidx, L, counts)
    return dict(ukeys=uks, seg_start=seg, inverse=inv, parents=parents, counts=counts.tolist())


def _assert_levels(got, ref, L, n_points, what):
    counts = ref["counts"][:L].tolist()
    assert got["counts"] == counts, (what, got["counts"], counts)
    for l in range(L):
        assert np.array_equal(host(got["ukeys"][l])[:counts[l]], ref["ukeys"][l]), (what, "keys", l)
        if l:
            assert np.array_equal(host(got["parents"][l - 1])[:counts[l - 1]], ref["parents"][l - 1]), (what, "parents", l)
    assert np.array_equal(host(got["seg_start"])[:counts[0] + 1], ref["seg_start"]), (what, "seg_start with its closing entry")
    assert np.array_equal(host(got["inverse"])[:n_points], ref["inverse"]), (what, "inverse")


@pytest.mark.parametrize("kind", ["runs", "one", "equal", "distinct"])
@pytest.mark.parametrize("L", [1, 2, 5])
def test_unique_routes_on_built_keys(kind, L):
    keys, src = K.sorted_keys_case(kind)
    ref = K.levels_ref(keys, src, L)
    skeys, sidx = up(keys), up(src)
    routes = {"per level": _route_per_level(skeys, sidx, L), "all levels": _route_all(skeys, sidx, L)}
    for what, got in routes.items():
        _assert_levels(got, ref, L, len(keys), (kind, L, what))
    assert torch.equal(skeys, up(keys)) and torch.equal(sidx, up(src)), "the inputs are read only"


@pytest.mark.parametrize("n_dev,n_cap", [(1000, 1500), (1, 700), (256, 257), (1500, 1500)])
def test_unique_capacity_tail_is_not_data(n_dev, n_cap):
    """`n_dev < n_cap`: the rows behind the device-side count hold further sorted keys, which must not be read as data."""
    keys = K.sorted_keys_case("runs")[0][2000:2000 + n_cap]
    ref = K.levels_ref(keys[:n_dev], None, 5)
    n = torch.tensor([n_dev], dtype=torch.int32, device=_dev())
    _assert_levels(_route_per_level(up(keys), None, 5, n_cap=n_cap, n_dev=n), ref, 5, n_dev, ("per level", n_dev, n_cap))
    # a count above the capacity is clamped to it
    big = torch.tensor([n_cap + 77], dtype=torch.int32, device=_dev())
    _assert_levels(_route_per_level(up(keys), None, 2, n_cap=n_cap, n_dev=big), K.levels_ref(keys, None, 2), 2, n_cap, "clamped")


@pytest.mark.parametrize("L", [1, 2, 5])
@pytest.mark.parametrize("shift,pad", [(False, 0), (True, 3)])
def test_voxelise_scene_equals_the_chain_and_the_reference(L, shift, pad):
    """Points -> every level: `voxelise_scene` (one C call), the op-by-op chain with each of the two level routes, and numpy."""
    ops = _ops()
    pts = K.level_scene()
    pd = strided(pts, pad)
    kref = K.voxel_keys_ref(pts[:, :3].numpy(), 50.0, K.stats_ref(pts[:, :3], F32).numpy(), shift, 0)
    order = np.argsort(kref["keys"], kind="stable")
    ref = K.levels_ref(kref["keys"][order], order, L)
    v = ops.voxelise_scene(pd, 50.0, shift, 32, L)
    rb = v["readback"].tolist()
    assert rb[:L] == ref["counts"].tolist() and rb[L] == 0
    assert torch.equal(v["stats"][:6].cpu(), K.stats_ref(pts[:, :3], F32)[:6])
    assert np.array_equal(host(v["origin"]), kref["origin"]) and np.array_equal(host(v["icoords"]), kref["icoords"])
    assert np.array_equal(host(v["skeys"]), kref["keys"][order]) and np.array_equal(host(v["sidx"]), order), "a stable sort"
    one_call = dict(ukeys=v["ukeys"], seg_start=v["seg_start"], inverse=v["inverse"], parents=v["parents"], counts=rb[:L])
    _assert_levels(one_call, ref, L, len(pts), "voxelise_scene")
    stats = ops.scene_stats(pd)
    assert torch.equal(stats, v["stats"])
    keys, ic, origin, err = ops.voxel_keys(pd, 50.0, stats, shift_to_min=shift)
    skeys, sidx = ops.sort_pairs(keys, None, 0, 32)
    assert torch.equal(skeys, v["skeys"]) and torch.equal(sidx, v["sidx"]) and int(err.item()) == 0
    routes = {"per level": _route_per_level(skeys, sidx, L), "all levels": _route_all(skeys, sidx, L)}
    for what, got in routes.items():
        _assert_levels(got, ref, L, len(pts), what)


# ---- 4. the extent clip ------------------------------------------------------------------------------------------------------------------
_CLIPPED = {}


def _clipped_levels(name):
    """Grid `name` at unit voxels through scene_stats, voxel_keys, the sort and one clipped `unique_sorted` per level
    -> (keys per level, parents per level pair, counts)."""
    if name not in _CLIPPED:
        ops = _ops()
        pts, _ = K.grid_points(K.clip_grid(name), 1.0)
        pd = up(pts)
        stats = ops.scene_stats(pd)
        keys, _, origin, err = ops.voxel_keys(pd, 1.0, stats, shift_to_min=True)
        assert int(err.item()) == 0 and origin.tolist() == [-32, -32, -32]
        skeys, sidx = ops.sort_pairs(keys, None, 0, 32)
        N = pts.shape[0]
        uk, _, _, n_prev = ops.unique_sorted(skeys, sidx, N, None, 0, want_seg_start=True, want_map=True, map_size=N)
        keys_l, parents, counts = [uk], [], [int(n_prev.item())]
        for lvl in range(1, K.CLIP_LEVELS):
            uk, _, par, n_prev = ops.unique_sorted(keys_l[-1], None, N, n_prev, 3, want_map=True, clip=(stats, 1.0, lvl, K.CLIP_MIN))
            keys_l.append(uk)
            parents.append(par)
            counts.append(int(n_prev.item()))
        _CLIPPED[name] = ([k[:c].contiguous() for k, c in zip(keys_l, counts)], [p[:c].contiguous() for p, c in zip(parents, counts)], counts)
    return _CLIPPED[name]


def _level_coords(keys, level):
    """Coordinates, in voxels of the level, of shift_to_min keys (key origin -32 level-0 voxels)."""
    return morton_decode_np(host(keys)) - (32 >> level)


@pytest.mark.parametrize("name", list(K.CLIP_GRIDS))
def test_extent_clip_of_unique_sorted(name):
    uc = K.clip_grid(name)
    coords, parents = K.clipped_levels_ref(uc, K.CLIP_LEVELS)
    sp = R.SpLevels(uc, K.CLIP_LEVELS, min_spatial_shape=K.CLIP_MIN)
    keys_l, par_l, counts = _clipped_levels(name)
    assert counts == [len(c) for c in coords] == [len(c) for c in sp.coords]
    for l in range(K.CLIP_LEVELS):
        got = _level_coords(keys_l[l], l)
        assert np.array_equal(got, coords[l]), (name, l, "surviving coordinates")
        perm = match_rows(got, sp.coords[l])
        if l:
            par = host(par_l[l - 1])
            assert np.array_equal(par, parents[l - 1]), (name, l, "parent map with its -1 entries")
            kept = np.concatenate([p[0] for p in sp.pairs_down[l - 1]])
            fine_perm = match_rows(_level_coords(keys_l[l - 1], l - 1), sp.coords[l - 1])
            assert sorted(fine_perm[par >= 0].tolist()) == sorted(kept.tolist()), "exactly the children without a pair are dropped"
            assert np.array_equal(sp.coords[l][perm[par[par >= 0]]], sp.coords[l - 1][fine_perm[par >= 0]] // 2)


@pytest.mark.parametrize("names", [("all", "even"), ("even", "all"), ("level2", "narrow")])
def test_batch_scene_maps_clip_each_scene_by_its_own_statistics(names):
    """Two scenes of different extents in one batch: the batch bits of a key select the statistics row of its scene.  `even` is wider
    than `all` on every axis and loses nothing; under the other scene's row it would lose its voxels at x >= 128, and `all` none."""
    from segdino3d_amd.sparse import BatchSceneMaps
    offs = [(3.0, -2.0, 1.0), (-4.0, 0.5, 2.0)]
    grids = [K.clip_grid(n) for n in names]
    pts = [K.grid_points(g, 0.02, o, seed=i)[0] for i, (g, o) in enumerate(zip(grids, offs))]
    maps = BatchSceneMaps([up(p) for p in pts], 0.02, K.CLIP_LEVELS, shift_to_min=True, order="z_fastest", clip_min_shape=K.CLIP_MIN)
    refs = [K.clipped_levels_ref(g, K.CLIP_LEVELS) for g in grids]
    for i, g in enumerate(grids):
        assert np.array_equal(host(maps.icoords[maps.point_off[i]:maps.point_off[i + 1]]), g[K.grid_points(g, 0.02, offs[i], seed=i)[1]])
    rows = []
    for l in range(K.CLIP_LEVELS):
        keys = host(maps.keys[l])
        scene = keys >> K.MORTON_BITS
        assert (np.diff(scene) >= 0).all() and maps.n_vox[l] == sum(len(r[0][l]) for r in refs)
        rows.append([np.nonzero(scene == i)[0] for i in range(2)])
        for i in range(2):
            coords, parents = refs[i]
            sp = R.SpLevels(grids[i], K.CLIP_LEVELS, min_spatial_shape=K.CLIP_MIN)
            got = morton_decode_np(keys[rows[l][i]]) - (32 >> l)
            assert np.array_equal(got, coords[l]), (names, "scene", i, "level", l)
            match_rows(got, sp.coords[l])
            if l:
                par = host(maps.parents[l - 1])[rows[l - 1][i]].astype(np.int64)
                base = int(rows[l][i][0])
                assert np.array_equal(np.where(par >= 0, par - base, -1), parents[l - 1]), (names, "scene", i, "parents of level", l - 1)
    dropped = [[int((p < 0).sum()) for p in r[1]] for r in refs]
    assert {n: any(d) for n, d in zip(names, dropped)} == {n: n not in ("even", "narrow") for n in names}


# ---- 5. stride_maps on clipped parents, and the convolution over them --------------------------------------------------------------------
@pytest.mark.parametrize("order", ["x_fastest", "z_fastest"])
def test_stride_maps_on_clipped_parents(order):
    from segdino3d_amd.sparse import child_perm
    uc = K.clip_grid("all")
    coords, parents = K.clipped_levels_ref(uc, K.CLIP_LEVELS)
    sp = R.SpLevels(uc, K.CLIP_LEVELS, min_spatial_shape=K.CLIP_MIN)
    keys_l, par_l, counts = _clipped_levels("all")
    perm8 = up(child_perm(order))
    for l in range(K.CLIP_LEVELS - 1):
        down, upt = _ops().stride_maps(keys_l[l], par_l[l], counts[l], counts[l + 1], perm8)
        want_down, want_up = K.stride_tables_ref(coords[l], coords[l + 1], parents[l], order)
        assert np.array_equal(host(down), want_down) and np.array_equal(host(upt), want_up), (order, l)
        dropped = parents[l] < 0
        assert dropped.any() and (host(upt)[:, dropped] == -1).all() and not np.isin(host(down), np.nonzero(dropped)[0]).any()
        only_up = _ops().stride_maps(keys_l[l], par_l[l], counts[l], counts[l + 1], perm8, want_down=False)
        assert only_up[0] is None and torch.equal(only_up[1], upt)
        if order == "z_fastest":                                # SpLevels' pairs, offset by offset
            fine_perm, coarse_perm = match_rows(coords[l], sp.coords[l]), match_rows(coords[l + 1], sp.coords[l + 1])
            for k, (i_k, o_k) in enumerate(sp.pairs_down[l]):
                rows = np.nonzero(host(upt)[k] >= 0)[0]
                assert sorted(zip(fine_perm[rows].tolist(), coarse_perm[host(upt)[k][rows]].tolist())) == sorted(zip(i_k.tolist(), o_k.tolist()))


@pytest.mark.parametrize("cin,cout", [(32, 32), (64, 96)])
def test_transposed_convolution_over_a_clipped_table(cin, cout):
    """A fine voxel whose parent was dropped has no pair at all: its row is relu(shift + res).  Pair-major and output-stationary."""
    from segdino3d_amd.sparse import child_perm
    ops = _ops()
    keys_l, par_l, counts = _clipped_levels("all")
    _, upt = ops.stride_maps(keys_l[0], par_l[0], counts[0], counts[1], up(child_perm("z_fastest")))
    nbr = host(upt)
    lone = np.nonzero((nbr >= 0).sum(0) == 0)[0]
    assert len(lone) >= 3 and ((nbr >= 0).sum(0) <= 1).all()
    g = K.gen(401, cin, cout)
    x = torch.randn(counts[1], cin, generator=g)
    w = torch.randn(8, cout, cin, generator=g) * (3.0 * cin ** -0.5)
    scale, shift = 0.5 + torch.rand(cout, generator=g), 0.1 * torch.randn(cout, generator=g)
    res = torch.randn(counts[0], cout, generator=g)
    ref = K.conv_ref(x, w, nbr, scale, shift, res)
    mag = ref.abs().amax(1, keepdim=True).clamp(min=1.0)
    pl = ops.pair_lists(upt, int((nbr >= 0).sum()))
    kw = dict(scale=up(scale), shift=up(shift), res=up(res), act="relu")
    outs = {"pair_conv": ops.pair_conv(up(x), up(w), pl, **kw), "gather_gemm": ops.gather_gemm(up(x), up(w), nbr=upt, **kw)}
    for what, y in outs.items():
        y = y.cpu()
        assert torch.equal(y[lone], torch.relu(shift[None, :] + res[lone])), (what, "rows without a pair")
        assert float(((y.double() - ref).abs() / mag).max()) < 2e-6, what


# ---- 6. voxel_mean -----------------------------------------------------------------------------------------------------------------------
def _device_voxel_mean(sc, f2d, mode, ld_out, pad=0):
    ops = _ops()
    pts = strided(sc["pts"], pad)
    stats = ops.scene_stats(pts)
    out = ops.voxel_mean(pts, up(f2d), mode, stats, up(sc["sidx"]), up(sc["seg_start"]), sc["n_vox"], ld_out)
    torch.cuda.synchronize()
    return out.cpu()


def _check_voxel_mean(case, out, sc, f2d, mode, ld_out):
    C = K.vm_channels(mode, 0 if f2d is None else f2d.shape[1])
    assert out.shape == (sc["n_vox"], ld_out)
    assert bool((out[:, C:] == 0.0).all()) and not bool(torch.signbit(out[:, C:]).any()), "padded columns are exactly 0.0"
    check_bound("voxel_mean", case, out[:, :C], K.vm_ref(sc, f2d, mode), K.vm_ref(sc, f2d, mode, F32), K.vm_bound(sc, f2d, mode))


VM_CASES = [(m, F, K.round_up(K.vm_channels(m, F), 32)) for m, F in K.VM_SHAPES] + [(m, F, ld) for (m, F), ld in K.VM_BRANCH] \
    + [K.VM_GENERIC + (K.round_up(K.vm_channels(*K.VM_GENERIC), 32),)]


@pytest.mark.parametrize("mode,F,ld_out", VM_CASES)
@pytest.mark.parametrize("pad", [0, 3])
def test_voxel_mean(mode, F, ld_out, pad):
    sc = K.vm_scene()
    f2d = K.vm_feats(sc["n"], F) if F else None
    out = _device_voxel_mean(sc, f2d, mode, ld_out, pad)
    _check_voxel_mean(f"mode {mode} C {K.vm_channels(mode, F)} ld_out {ld_out} point rows of {6 + pad}", out, sc, f2d, mode, ld_out)


def test_voxel_mean_is_the_same_on_both_sides_of_the_branch():
    """The two paths add a voxel's points in the same (ascending) order: the same C at ld_out = 320 and 352 gives the same bits."""
    sc = K.vm_scene()
    for mode, F in {s for s, _ in K.VM_BRANCH}:
        f2d = K.vm_feats(sc["n"], F)
        C = K.vm_channels(mode, F)
        a, b = _device_voxel_mean(sc, f2d, mode, 320), _device_voxel_mean(sc, f2d, mode, 352)
        assert torch.equal(a[:, :C], b[:, :C]), (mode, F)


# ---- 7. voxel_mean_batch -----------------------------------------------------------------------------------------------------------------
VMB_POPULATIONS = [tuple(K.VM_POPULATIONS), (3, 1, 5, 2, 66, 1, 4), (1,) * 7 + (130, 4, 9)]


@pytest.mark.parametrize("mode,F,ld_out", [(2, 59, 96), (0, 317, 352), (1, 0, 32)])
def test_voxel_mean_batch(mode, F, ld_out):
    ops = _ops()
    scenes = [K.vm_scene(i, VMB_POPULATIONS[i]) for i in range(3)]
    feats = [K.vm_feats(sc["n"], F, i) if F else None for i, sc in enumerate(scenes)]
    pts = [strided(sc["pts"], 3 * (i % 2)) for i, sc in enumerate(scenes)]
    stats = torch.stack([ops.scene_stats(p) for p in pts])
    off = np.concatenate([[0], np.cumsum([sc["n"] for sc in scenes])])
    voff = np.concatenate([[0], np.cumsum([sc["n_vox"] for sc in scenes])])
    sidx = np.concatenate([sc["sidx"].astype(np.int64) + off[i] for i, sc in enumerate(scenes)]).astype(np.int32)
    seg = np.concatenate([sc["seg_start"][:-1].astype(np.int64) + off[i] for i, sc in enumerate(scenes)] + [[off[-1]]]).astype(np.int32)
    ukeys = np.concatenate([np.arange(sc["n_vox"], dtype=np.int64) * 8 + 5 + (np.int64(i) << K.MORTON_BITS) for i, sc in enumerate(scenes)])
    fd = [up(f) for f in feats]
    batch = ops.voxel_mean_batch([(pts[i], fd[i], stats[i], int(off[i])) for i in range(3)], mode, up(ukeys), up(sidx), up(seg), int(voff[-1]), ld_out)
    torch.cuda.synchronize()
    assert batch.shape == (int(voff[-1]), ld_out)
    for i, sc in enumerate(scenes):
        single = ops.voxel_mean(pts[i], fd[i], mode, stats[i], up(sc["sidx"]), up(sc["seg_start"]), sc["n_vox"], ld_out)
        rows = batch[voff[i]:voff[i + 1]]
        assert torch.equal(rows.view(torch.int32), single.view(torch.int32)), ("scene", i, "differs from its single-scene launch")
        _check_voxel_mean(f"batch scene {i} (point_off {off[i]}) mode {mode} ld_out {ld_out}", rows.cpu(), sc, feats[i], mode, ld_out)


# ---- 8. segment_starts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,S", [(255, 300), (256, 300), (257, 300), (600, 1), (1, 1), (1000, 40), (5000, 2000)])
def test_segment_starts(n, S):
    ids = K.seg_ids_case(n, S)
    got = _ops().segment_starts(up(ids), n, S)
    assert np.array_equal(host(got), K.segment_starts_ref(ids, S))
    if S > 1:                                                   # ids above S count as S: everything in front of them is unchanged
        over = np.concatenate([ids, [S, S + 5, S + 1000]])
        got = _ops().segment_starts(up(over), len(over), S)
        assert np.array_equal(host(got), K.segment_starts_ref(over, S)) and int(got[S]) == n


@pytest.mark.parametrize("sizes", [((255, 300), (257, 40)), ((256, 60), (1, 1), (700, 300)), ((600, 1), (256, 300))])
def test_segment_starts_batch(sizes):
    ids = [K.seg_ids_case(n, S, seed=i) for i, (n, S) in enumerate(sizes)]
    off = np.concatenate([[0], np.cumsum([S for _, S in sizes])])
    keys = np.concatenate([(np.int64(i) << 32) | v for i, v in enumerate(ids)])
    dense = np.concatenate([v + off[i] for i, v in enumerate(ids)])
    n, S = len(keys), int(off[-1])
    got = _ops().segment_starts_batch(up(keys), n, S, off[:-1].tolist())
    assert np.array_equal(host(got), K.segment_starts_ref(dense, S))
    for i in range(len(sizes)):                                 # every scene's slice is its own segment_starts, moved by its points
        own = K.segment_starts_ref(ids[i], sizes[i][1])[:-1] + sum(s[0] for s in sizes[:i])
        assert np.array_equal(host(got)[off[i]:off[i + 1]], own)


# ---- 9. pool_superpoints -----------------------------------------------------------------------------------------------------------------
def _pool_feat(c, layout):
    if layout == "contiguous":
        return up(c["feat"])
    if layout == "slice of 128":
        big = torch.full((K.POOL_VOX, 128), float("nan"))
        big[:, :c["C"]] = c["feat"]
        return big.to(_dev())[:, :c["C"]]
    return strided(c["feat"], int(layout))


@pytest.mark.parametrize("C,layout", [(4, "contiguous"), (4, "4"), (32, "contiguous"), (32, "12"), (64, "contiguous"), (64, "4"),
                                      (96, "contiguous"), (96, "slice of 128"), (96, "8")])
def test_pool_superpoints(C, layout):
    ops = _ops()
    c = K.pool_case(C)
    feat = _pool_feat(c, layout)
    assert feat.stride(0) % 4 == 0
    start = ops.segment_starts(up(np.repeat(np.arange(c["S"]), c["sizes"]).astype(np.int64)), c["n"], c["S"])
    assert np.array_equal(host(start), c["start"])
    of, op = ops.pool_superpoints(feat, C, up(c["inverse"]), up(c["icoords"]), K.VS, up(c["sidx"]), start, c["S"])
    torch.cuda.synchronize()
    of, op = of.cpu(), op.cpu()
    empty = np.nonzero(c["sizes"] == 0)[0]
    for t in (of, op):
        assert bool((t[empty] == 0.0).all()) and not bool(torch.signbit(t[empty]).any()), "an empty superpoint's rows are exactly 0.0"
    (f64, p64), (f32, p32), (bf, bp) = K.pool_ref(c), K.pool_ref(c, F32), K.pool_bound(c)
    check_bound("pool_superpoints features", f"C {C} {layout}", of, f64, f32, bf)
    check_bound("pool_superpoints positions", f"C {C} {layout}", op, p64, p32, bp)
    one = np.nonzero(c["sizes"] == 1)[0]
    p = c["sidx"][c["start"][one]]
    assert torch.equal(of[one], c["feat"][c["inverse"][p].astype(np.int64)]), "a superpoint of one point is its voxel's row"


# ---- 10. keys_from_i64 -------------------------------------------------------------------------------------------------------------------
KEY_FILL, ERR_ARG = -0x0123456789ABCDEF, -1


def _keys64_lib():
    from segdino3d_amd import _lib
    return _lib.load(), torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("n", K.KEYS64_N[1:])
def test_keys_from_i64(n):
    """Every (id pattern, position, add, bits, preset of the maximum) at n ids: keys, flag word and maximum equal the numpy model written
    from the header.  All cases of one n are launched on rows of shared buffers (sentinels behind every key row, the flag and maximum
    words of the cases side by side) and read back once."""
    lib, st = _keys64_lib()
    P, V = K.KEYS64_FLAG_PRESET, K.KEYS64_FLAG_VALUE
    cases = [(name, at, add, bits, preset) for name in K.KEYS64_IDS for at in (K.keys64_positions(n) if name != "zeros" else [0])
             for add in K.KEYS64_ADD for bits in K.KEYS64_BITS for preset in K.KEYS64_MAX_PRESETS]
    xs = np.stack([K.keys64_case(n, name, at) for name, at, *_ in cases])
    x = up(xs)
    ld = n + 64
    keys = torch.full((len(cases), ld), KEY_FILL, dtype=torch.int64, device=_dev())
    flag = torch.full((len(cases),), P, dtype=torch.int32, device=_dev())
    mx = up(np.array([c[4] for c in cases], dtype=np.int32))
    for i, (name, at, add, bits, preset) in enumerate(cases):
        rc = lib.sd3d_keys_from_i64(x.data_ptr() + 8 * n * i, n, add, keys.data_ptr() + 8 * ld * i, bits, flag.data_ptr() + 4 * i, V,
                                    mx.data_ptr() + 4 * i, st)
        assert rc == 0, (cases[i], lib.sd3d_last_error())
    torch.cuda.synchronize()
    keys, flag, mx = host(keys), host(flag), host(mx)
    assert (keys[:, n:] == KEY_FILL).all(), "sentinels behind the keys were overwritten"
    for i, (name, at, add, bits, preset) in enumerate(cases):
        rk, rf, rm = K.keys_from_i64_ref(xs[i], add, bits, V, P, preset)
        assert np.array_equal(keys[i, :n].view(np.uint64), rk), cases[i]
        assert (int(flag[i]), int(mx[i])) == (rf, rm), (cases[i], int(flag[i]), int(mx[i]), rf, rm)


def test_keys_from_i64_no_ids_and_refusals():
    lib, st = _keys64_lib()
    x = up(K.keys64_case(257, "negative", 256))
    keys = torch.full((257 + 64,), KEY_FILL, dtype=torch.int64, device=_dev())
    words = torch.tensor([K.KEYS64_FLAG_PRESET, 7], dtype=torch.int32, device=_dev())
    flag, mx = words.data_ptr(), words.data_ptr() + 4

    def untouched():
        torch.cuda.synchronize()
        return bool((keys == KEY_FILL).all()) and words.tolist() == [K.KEYS64_FLAG_PRESET, 7]
    assert lib.sd3d_keys_from_i64(x.data_ptr(), 0, 5 << 32, keys.data_ptr(), 16, flag, 4, mx, st) == 0 and untouched()      # no ids: nothing written
    for f, m, bits in ((None, mx, 16), (flag, None, 16), (flag, mx, 0), (flag, mx, 65)):
        assert lib.sd3d_keys_from_i64(x.data_ptr(), 257, 0, keys.data_ptr(), bits, f, 4, m, st) == ERR_ARG and untouched(), (f, m, bits)


# ---- 11. refusals ------------------------------------------------------------------------------------------------------------------------
def _valid_call_still_works():
    p = K.stats_case(257, 6)
    got = _ops().scene_stats(up(p)).cpu()
    assert torch.equal(got[:6], K.stats_ref(p, F32)[:6])
    c = K.pool_case(4)
    of, _ = _ops().pool_superpoints(up(c["feat"]), 4, up(c["inverse"]), up(c["icoords"]), K.VS, up(c["sidx"]), up(c["start"]), c["S"])
    assert K.inside(of, K.pool_ref(c)[0], K.pool_bound(c)[0])


def test_refusals_on_the_device():
    ops = _ops()
    d = _dev()
    empty = torch.empty(0, 6, device=d)
    with pytest.raises(RuntimeError, match="empty scene"):
        ops.scene_stats(empty)
    with pytest.raises(RuntimeError, match="empty scene"):
        ops.voxel_keys(empty, 50.0, torch.zeros(9, device=d))
    sc = K.vm_scene()
    for mode in (0, 2):
        with pytest.raises(RuntimeError, match="2D features missing"):
            ops.voxel_mean(up(sc["pts"]), None, mode, torch.zeros(9, device=d), up(sc["sidx"]), up(sc["seg_start"]), sc["n_vox"], 32)
        with pytest.raises(RuntimeError, match="2D features missing"):
            ops.voxel_mean_batch([(up(sc["pts"]), None, torch.zeros(9, device=d), 0)], mode, torch.zeros(sc["n_vox"], dtype=torch.int64, device=d),
                                 up(sc["sidx"]), up(sc["seg_start"]), sc["n_vox"], 32)
    with pytest.raises(RuntimeError, match="need the voxel keys"):     # only one scene may come without them
        ops.voxel_mean_batch([(up(sc["pts"]), None, torch.zeros(9, device=d), 0)] * 2, 1, None, up(sc["sidx"]), up(sc["seg_start"]), sc["n_vox"], 32)
    c = K.pool_case(96)
    args = (up(c["inverse"]), up(c["icoords"]), K.VS, up(c["sidx"]), up(c["start"]), c["S"])
    wide104 = torch.zeros(K.POOL_VOX, 104, device=d)
    for C in (98, 100):
        with pytest.raises(RuntimeError, match="multiple of 4 and <= 96"):
            ops.pool_superpoints(wide104[:, :C], C, *args)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.pool_superpoints(torch.zeros(K.POOL_VOX, 98, device=d)[:, :96], 96, *args)
    keys = up(K.sorted_keys_case("distinct")[0])
    for n_levels in (0, 9):
        with pytest.raises(RuntimeError, match="1..8 levels"):
            ops.voxel_levels_all(keys, None, n_levels, torch.zeros(9, dtype=torch.int32, device=d))
    with pytest.raises(RuntimeError, match="1..16 scenes"):
        ops.segment_starts_batch(torch.zeros(4, dtype=torch.int64, device=d), 4, 17, list(range(17)))
    torch.cuda.synchronize()
    _valid_call_still_works()


def test_cpu_tensors_are_refused():
    ops = _ops()
    d = _dev()
    sc, c = K.vm_scene(), K.pool_case(4)
    pts, keys = sc["pts"], torch.from_numpy(K.sorted_keys_case("distinct")[0])
    i32 = torch.zeros(700, dtype=torch.int32)
    calls = [lambda: ops.scene_stats(pts),
             lambda: ops.voxel_keys(pts, 50.0, torch.zeros(9, device=d)),
             lambda: ops.voxel_keys(up(pts), 50.0, torch.zeros(9)),
             lambda: ops.unique_sorted(keys, None, 700),
             lambda: ops.unique_sorted(up(keys), i32, 700),
             lambda: ops.voxel_levels_all(keys, None, 2, torch.zeros(2, dtype=torch.int32, device=d)),
             lambda: ops.voxelise_scene(pts, 50.0, False, 32, 2),
             lambda: ops.stride_maps(keys, up(i32), 700, 700, up(np.arange(8, dtype=np.int32))),
             lambda: ops.voxel_mean(pts, None, 1, torch.zeros(9, device=d), up(sc["sidx"]), up(sc["seg_start"]), sc["n_vox"], 32),
             lambda: ops.voxel_mean(up(pts), None, 1, torch.zeros(9, device=d), torch.from_numpy(sc["sidx"]), up(sc["seg_start"]), sc["n_vox"], 32),
             lambda: ops.voxel_mean_batch([(pts, None, torch.zeros(9, device=d), 0)], 1, up(keys), up(sc["sidx"]), up(sc["seg_start"]), sc["n_vox"], 32),
             lambda: ops.segment_starts(keys, 700, 10),
             lambda: ops.segment_starts_batch(keys, 700, 10, [0]),
             lambda: ops.pool_superpoints(c["feat"], 4, up(c["inverse"]), up(c["icoords"]), K.VS, up(c["sidx"]), up(c["start"]), c["S"]),
             lambda: ops.pool_superpoints(up(c["feat"]), 4, torch.from_numpy(c["inverse"]), up(c["icoords"]), K.VS, up(c["sidx"]), up(c["start"]), c["S"])]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    torch.cuda.synchronize()
    _valid_call_still_works()
