"""tests/prologue_kernel_cases.py on the CPU: the integer references agree with `oracle/sparse_ref.py` (`floor_voxel`, `unique_voxels`,
`segment_mean`, `MinkLevels`, `SpLevels(min_spatial_shape=...)`) on the same inputs, the planted situations are present, the fp32
evaluation of every float reference stays inside its bound, and a reference that drops or double-counts one member of the largest
segment does not - the bounds can see the bugs the GPU tests exist for."""
import numpy as np
import pytest
import torch

from oracle import sparse_ref as R
from tests import prologue_kernel_cases as K
from tests.helpers import match_rows, morton_decode_np

F32 = torch.float32


# ---- keys --------------------------------------------------------------------------------------------------------------------------------
def test_morton_codec_round_trip():
    rng = np.random.default_rng(0)
    r = rng.integers(0, 65536, (2000, 3))
    m = K.morton_encode_np(r)
    assert np.array_equal(morton_decode_np(m), r)
    assert K.morton_encode_np(np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0]])).tolist() == [1, 2, 4, 8]
    k = m | (np.int64(5) << K.MORTON_BITS)
    assert np.array_equal(K.level_key(k, 3), (m >> 3) | (np.int64(5) << K.MORTON_BITS))


@pytest.mark.parametrize("inv_voxel", K.INV_VOXELS)
@pytest.mark.parametrize("shift", [False, True])
def test_voxel_keys_reference_equals_the_oracle(inv_voxel, shift):
    pts = K.keys_case(inv_voxel)
    xyz = pts[:, :3]
    stats = K.stats_ref(xyz, F32).numpy()
    ref = K.voxel_keys_ref(xyz.numpy(), inv_voxel, stats, shift, 3)
    voxel = float(np.float32(1.0) / np.float32(inv_voxel))
    assert float(np.float32(1.0) / np.float32(voxel)) == inv_voxel, "floor_voxel must arrive at the same reciprocal"
    want = R.floor_voxel(xyz - xyz.min(0)[0] if shift else xyz, voxel)
    assert np.array_equal(ref["icoords"], want)
    # the planted situations: multiples of the voxel size are where the reciprocal and a true division part ways
    x32 = (xyz - xyz.min(0)[0] if shift else xyz).numpy()
    divided = np.floor((x32 / np.float32(voxel)).astype(np.float32)).astype(np.int64)
    assert (divided != ref["icoords"]).sum() >= 10, "no coordinate at which a true fp32 division quantises differently"
    if not shift:
        assert bool(((xyz == 0) & torch.signbit(xyz)).any()) and bool((xyz < 0).any())
    # origin: a multiple of 16, at least 32 below the smallest coordinate; keys decode to icoords - origin; the scene bits
    cmin = ref["icoords"].min(0)
    assert (ref["origin"] % 16 == 0).all() and (ref["origin"] <= cmin - 32).all() and (ref["origin"] > cmin - 48).all()
    assert np.array_equal(morton_decode_np(ref["keys"]), ref["icoords"].astype(np.int64) - ref["origin"])
    assert ((ref["keys"] >> K.MORTON_BITS) == 3).all() and ref["flag"] == 0


def test_key_range_flags_of_the_reference():
    def flag(rel, axis):
        p = K.flag_case(rel, axis)
        ref = K.voxel_keys_ref(p[:, :3].numpy(), 1.0, K.stats_ref(p[:, :3], F32).numpy(), True, 0)
        assert ref["origin"].tolist() == [-32, -32, -32] and int(ref["icoords"][1, axis]) - int(ref["origin"][axis]) == rel
        return ref["flag"]
    assert [flag(65536 - 65, a) for a in range(3)] == [2, 2, 2] and [flag(65536 - 64, a) for a in range(3)] == [3, 3, 3]
    # Z-order bit 32 is bit 10 of z; bits 33 and 34 are bit 11 of x and y
    assert [flag(2047, 0), flag(2048, 0), flag(2047, 1), flag(2048, 1), flag(1023, 2), flag(1024, 2)] == [0, 2, 0, 2, 0, 2]


def test_keys_from_i64_reference():
    """The numpy model of `sd3d_keys_from_i64` on its planted ids: what each of them must and must not raise, hand-stated."""
    P, V = K.KEYS64_FLAG_PRESET, K.KEYS64_FLAG_VALUE
    assert V & P == 0 and 8 & (P | V) == 0 and K.KEYS64_N[0] == 0
    assert {n % 64 for n in K.KEYS64_N} >= {0, 1, 63} and {n % 256 for n in K.KEYS64_N if n > 64} >= {0, 1, 255} and max(K.KEYS64_N) > 4 * 256
    # id -> (flag bits beyond the preset at bits = 16, at bits = 64, the maximum it brings)
    want = {"zeros": (0, 0, 0), "fits16": (0, 0, 65535), "over16": (V, 0, 65536), "below_limit": (V, 0, 0x7FFFFFFE), "limit": (V | 8, 8, 0x7FFFFFFF),
            "negative": (V | 8, 8, 0x7FFFFFFF)}
    assert set(want) == set(K.KEYS64_IDS)
    for n in K.KEYS64_N[1:]:
        pos = K.keys64_positions(n)
        assert pos[0] == 0 and pos[-1] == n - 1 and (n < 3 or 0 < pos[1] < n - 1)
        for name in K.KEYS64_IDS:
            for at in pos:
                x = K.keys64_case(n, name, at)
                small = np.delete(x, at)
                assert (small >= 0).all() and (small < 100).all() and (name == "zeros" or x[at] == K.KEYS64_IDS[name])
                for add in K.KEYS64_ADD:
                    for bi, bits in enumerate(K.KEYS64_BITS):
                        for preset in K.KEYS64_MAX_PRESETS:
                            keys, flag, mx = K.keys_from_i64_ref(x, add, bits, V, P, preset)
                            assert keys.dtype == np.uint64 and keys.tolist() == [(int(v) + add) % (1 << 64) for v in x]
                            assert flag == P | want[name][bi], (n, name, at, bits)
                            top = want[name][2] if name == "zeros" or n == 1 else max(want[name][2], int(small.max()))
                            assert mx == max(preset, top), (n, name, at, preset)
    assert K.keys_from_i64_ref(np.zeros(0, np.int64), 5 << 32, 16, V, P, 7)[1:] == (P, 7)                # no ids: nothing changes
    # the checks see the id, not the key: an offset above 16 bits raises nothing
    assert K.keys_from_i64_ref(np.array([3], np.int64), 5 << 32, 16, V, P, 0)[1:] == (P, 3)


# ---- levels ------------------------------------------------------------------------------------------------------------------------------
def _scene_keys(pts, inv_voxel=50.0, shift=False):
    ref = K.voxel_keys_ref(pts[:, :3].numpy(), inv_voxel, K.stats_ref(pts[:, :3], F32).numpy(), shift, 0)
    order = np.argsort(ref["keys"], kind="stable")
    return ref, ref["keys"][order], order.astype(np.int32)


def test_levels_reference_equals_the_oracle():
    pts = K.level_scene()
    ref, skeys, sidx = _scene_keys(pts)
    lv = K.levels_ref(skeys, sidx, 5)
    uc, inv = R.unique_voxels(ref["icoords"])
    mine = morton_decode_np(lv["ukeys"][0]) + ref["origin"][None, :].astype(np.int64)
    perm = match_rows(mine, uc)
    assert np.array_equal(perm[lv["inverse"]], inv), "the point -> voxel map"
    assert lv["counts"][0] == len(uc) < len(pts) and lv["seg_start"][-1] == len(pts)
    assert np.array_equal(np.diff(lv["seg_start"]), np.bincount(lv["inverse"], minlength=len(uc)))
    mink = R.MinkLevels(uc)
    for l in range(5):
        c = (morton_decode_np(lv["ukeys"][l]) << l) + ref["origin"][None, :].astype(np.int64)
        match_rows(c, mink.coords[1 << l])
        if l:
            fine = (morton_decode_np(lv["ukeys"][l - 1]) << (l - 1)) + ref["origin"][None, :].astype(np.int64)
            assert np.array_equal(c[lv["parents"][l - 1]], np.floor_divide(fine, 1 << l) << l), "a voxel's parent holds it"
    assert lv["counts"].tolist() == [mink.n(1 << l) for l in range(5)] and lv["counts"][4] < lv["counts"][0]


@pytest.mark.parametrize("kind", ["runs", "one", "equal", "distinct"])
def test_sorted_key_cases(kind):
    keys, src = K.sorted_keys_case(kind)
    assert (np.diff(keys) >= 0).all() and sorted(src.tolist()) == list(range(len(keys)))
    lv = K.levels_ref(keys, src, 5)
    uk, first, cnt = np.unique(keys, return_index=True, return_counts=True)
    assert np.array_equal(lv["ukeys"][0], uk) and np.array_equal(lv["seg_start"][:-1], first) and lv["seg_start"][-1] == len(keys)
    assert np.array_equal(lv["ukeys"][0][lv["inverse"][src]], keys)
    for l in range(1, 5):
        assert np.array_equal(lv["ukeys"][l], np.unique(K.level_key(keys, 3 * l)))
        assert np.array_equal(lv["ukeys"][l][lv["parents"][l - 1]], K.level_key(lv["ukeys"][l - 1], 3))
    if kind == "runs":
        seg = lv["seg_start"]
        crossing = ((seg[:-1] // 256) != ((seg[1:] - 1) // 256)).sum()
        assert crossing >= 10 and cnt.max() == 600 and (lv["ukeys"][0] >> K.MORTON_BITS).max() == 1
        assert lv["counts"][4] < lv["counts"][2] < lv["counts"][0]


# ---- extent clip -------------------------------------------------------------------------------------------------------------------------
DROPS = {"narrow": [0, 0, 0], "level1": [1, 0, 0], "level2": [0, 1, 0], "level3": [0, 0, 1], "all": [1, 1, 1], "even": [0, 0, 0]}


@pytest.mark.parametrize("name", list(K.CLIP_GRIDS))
def test_clipped_levels_reference_equals_the_oracle(name):
    uc = K.clip_grid(name)
    assert (uc.min(0) == 0).all() and (uc.max(0) + 1 == np.array(K.CLIP_GRIDS[name])).all()
    coords, parents = K.clipped_levels_ref(uc, K.CLIP_LEVELS)
    sp = R.SpLevels(uc, K.CLIP_LEVELS, min_spatial_shape=K.CLIP_MIN)
    for l in range(K.CLIP_LEVELS):
        perm = match_rows(coords[l], sp.coords[l])
        if l == 0:
            continue
        dropped = parents[l - 1] < 0
        assert bool(dropped.any()) == bool(DROPS[name][l - 1]), (name, l, int(dropped.sum()))
        # exactly the children outside SpLevels' pairs are dropped, and the others have SpLevels' parent
        fine_perm = match_rows(coords[l - 1], sp.coords[l - 1])
        i_idx = np.concatenate([p[0] for p in sp.pairs_down[l - 1]])
        o_idx = np.concatenate([p[1] for p in sp.pairs_down[l - 1]])
        want = np.full(len(sp.coords[l - 1]), -1, dtype=np.int64)
        want[i_idx] = o_idx
        got = parents[l - 1].astype(np.int64)
        assert np.array_equal(np.where(got >= 0, perm[np.maximum(got, 0)], -1), want[fine_perm])
        for order in ("x_fastest", "z_fastest"):
            down, up = K.stride_tables_ref(coords[l - 1], coords[l], parents[l - 1], order)
            assert ((up >= 0).sum(0) == (~dropped)).all() and (down >= 0).sum() == (~dropped).sum()
            if order == "z_fastest":
                for k, (i_k, o_k) in enumerate(sp.pairs_down[l - 1]):
                    rows = np.nonzero(up[k] >= 0)[0]
                    assert sorted(zip(fine_perm[rows].tolist(), perm[up[k][rows]].tolist())) == sorted(zip(i_k.tolist(), o_k.tolist()))
                    assert np.array_equal(down[k][up[k][rows]], rows)


def test_grid_points_quantise_to_their_voxels():
    for name, vs, off in (("all", 1.0, (0, 0, 0)), ("all", 0.02, (3.0, -2.0, 1.0)), ("even", 0.02, (-4.0, 0.5, 2.0))):
        uc = K.clip_grid(name)
        pts, vox = K.grid_points(uc, vs, off)
        inv = float(np.float32(1.0) / np.float32(vs))
        ref = K.voxel_keys_ref(pts[:, :3].numpy(), inv, K.stats_ref(pts[:, :3], F32).numpy(), True, 0)
        assert np.array_equal(ref["icoords"], uc[vox]) and ref["flag"] == 0
        st = K.stats_ref(pts[:, :3], F32).numpy()
        D = np.floor((st[3:6] - st[0:3]).astype(np.float32) * np.float32(inv)).astype(np.int64) + 1      # the clip's own extent
        assert D.tolist() == list(K.CLIP_GRIDS[name])


# ---- scene statistics --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", K.STATS_N)
def test_stats_bound(n):
    p = K.stats_case(n, 6)
    r64, r32 = K.stats_ref(p), K.stats_ref(p, F32)
    assert torch.equal(r64[:6], r32[:6].double()) and float(r64[0]) == -1600.0 and float(r64[4]) == 90.0
    b = K.stats_sum_bound(p)
    assert K.inside(r32[6:], r64[6:], b)
    if n > 1:                                                   # one point left out / counted twice
        for sign in (-1.0, 1.0):
            assert not K.inside(r64[6:] + sign * p[n // 3, :3].double(), r64[6:], b)
    else:
        assert float(b.max()) == 0.0


# ---- voxel means -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,F", K.VM_SHAPES + [K.VM_GENERIC])
def test_voxel_mean_bound(mode, F):
    sc = K.vm_scene()
    f2d = K.vm_feats(sc["n"], F) if F else None
    assert K.vm_channels(mode, F) == K.vm_rows(sc["pts"], f2d, mode).shape[1]
    r64, r32, b = K.vm_ref(sc, f2d, mode), K.vm_ref(sc, f2d, mode, F32), K.vm_bound(sc, f2d, mode)
    assert K.inside(r32, r64, b)
    ones = np.nonzero(np.array(K.VM_POPULATIONS) == 1)[0]
    if mode != 2:
        assert float(b[ones].max()) <= K.U * float(r64[ones].abs().max())           # a voxel of one point: its row, once rounded at most
    v = sc["largest"]
    assert K.VM_POPULATIONS[v] == 700
    rows = K.vm_rows(sc["pts"], f2d, mode)
    for double in (False, True):
        wrong = K.drop_or_double(rows, sc["vox"], sc["n_vox"], v, double)
        assert not K.inside(wrong, r64[v], b[v]), (mode, F, double)
        if F:                                                   # ... in the 2D feature columns, not only in some column
            assert not K.inside(wrong[-F:], r64[v, -F:], b[v, -F:])
    if mode == 2:                                               # the centring matters: uncentred coordinates are nowhere near
        assert float(r64[:, 3:6].abs().max()) < 2.0 and float(sc["pts"][:, :3].abs().min()) > 25.0
        assert float((K.vm_centre32(sc["pts"]).double() - sc["pts"][:, :3].double().mean(0)).abs().max()) <= float(K.centre_bound(sc["pts"]).max())


def test_voxel_mean_reference_is_the_oracles_feature_assembly():
    """mode 0 / 2 rows are what `mink_forward_wrapper` / `spconv_forward_wrapper` assemble in front of `segment_mean`."""
    sc = K.vm_scene()
    f2d = K.vm_feats(sc["n"], 5)
    p = sc["pts"].double()
    assert torch.equal(K.vm_rows(sc["pts"], f2d, 0), torch.cat([p[:, 3:], f2d.double()], 1))
    assert torch.equal(K.vm_rows(sc["pts"], f2d, 2), torch.cat([p[:, 3:], p[:, :3] - p[:, :3].mean(0), f2d.double()], 1))
    assert np.array_equal(np.diff(sc["seg_start"]), np.array(K.VM_POPULATIONS))
    assert np.array_equal(sc["vox"][sc["sidx"]], np.repeat(np.arange(sc["n_vox"]), K.VM_POPULATIONS))
    for v in range(sc["n_vox"]):
        members = sc["sidx"][sc["seg_start"][v]:sc["seg_start"][v + 1]]
        assert (np.diff(members) > 0).all()


# ---- segment starts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,S", [(255, 300), (256, 300), (257, 300), (600, 1), (1000, 40)])
def test_segment_starts_reference(n, S):
    ids = K.seg_ids_case(n, S)
    start = K.segment_starts_ref(ids, S)
    assert start[0] == 0 and start[S] == n and (np.diff(start) >= 0).all()
    assert np.array_equal(np.diff(start), np.bincount(ids, minlength=S))
    if S > 1:
        assert ids.min() >= 7 and ids.max() < S - 9 and np.diff(np.unique(ids)).max() > 1
    clamped = np.concatenate([ids, [S + 5]])
    assert K.segment_starts_ref(clamped, S)[S] == n


# ---- pooling -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", K.POOL_C)
def test_pool_bound(C):
    c = K.pool_case(C)
    assert sorted(set(c["sizes"].tolist())) == sorted(K.POOL_SIZES) and c["sizes"][0] > 0 and c["sizes"][-1] == 0
    assert np.array_equal(c["seg"][c["sidx"]], np.repeat(np.arange(c["S"]), c["sizes"])) and (c["icoords"] < 0).any()
    (f64, p64), (f32, p32), (bf, bp) = K.pool_ref(c), K.pool_ref(c, F32), K.pool_bound(c)
    assert K.inside(f32, f64, bf) and K.inside(p32, p64, bp)
    empty = np.nonzero(c["sizes"] == 0)[0]
    assert len(empty) == 3 and float(f64[empty].abs().max()) == 0.0 and float(bf[empty].max()) == 0.0 and float(bp[empty].max()) == 0.0
    s = c["largest"]
    members = np.nonzero(c["seg"] == s)[0]
    assert len(members) == 700 and (c["inverse"][members] == 17).sum() >= 350
    f, pos = K.pool_terms(c)
    for double in (False, True):
        assert not K.inside(K.drop_or_double(f, c["seg"], c["S"], s, double), f64[s], bf[s])
        assert not K.inside(K.drop_or_double(pos, c["seg"], c["S"], s, double), p64[s], bp[s])
    # the oracle's pooled positions: segment_mean(icoords.float() * voxel_size)
    want = R.segment_mean(torch.from_numpy(c["icoords"]).float() * 0.02, c["seg"], c["S"])
    assert torch.equal(p32, want)
