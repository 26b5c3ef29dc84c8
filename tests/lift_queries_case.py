"""Test cases of the query lifting (segdino3d_amd/lift_queries.py), built on the CPU.

Room case: the analytic room of tests/lift2d_case.py (floor z = 0, back wall y = 4, one box), 70 random views with 24 x 32 depth, and six
queries per view whose masks are ray-cast at the mask's own resolution - box, floor, wall, box dilated by 2 mask pixels (it leaks onto
the background and exercises the gate), empty, whole image (more pixels than a workgroup has lanes).  Hand-built case: identity pose,
fx = fy = 1, cx = cy = 0 (so w = (ui d, vi d, d)), 8 x 8 depth, medians computable by hand.

`python tests/lift_queries_case.py` prints DEV32, the largest centre deviation of the float32 restatement from the float64 one."""
import functools

import numpy as np

import lift_queries_ref as R
from lift2d_case import BOX, WALL_Y, look_at_pose, make_views  # noqa: F401  (look_at_pose: for the tests)

DEV32 = 9.537e-07      # `python tests/lift_queries_case.py`; profiles/lift_queries.md, "tolerance"
DEPTH_SCALE = 0.001
SEED = 3
N_VIEWS, HD, WD = 70, 24, 32
MASK_SIZES = [(24, 32), (12, 16), (48, 64), (17, 23)]          # the depth's own, half, double, a non-integer ratio
ROOM_RULE = dict(min_pixels=4)
Q_BOX, Q_FLOOR, Q_WALL, Q_DILATED, Q_EMPTY, Q_WHOLE = range(6)
FLOOR, WALL, BOX_ID = 1, 2, 3


def surface_ids(pose, intr, Hd, Wd, Hm, Wm):
    """Which surface the ray through the centre of every MASK pixel hits first (0 nothing, FLOOR, WALL, BOX_ID): int [Hm, Wm].  Mask pixel
    (ym, xm) has its centre at (xm + 0.5) Wd / Wm - 0.5 in pixels of the depth image."""
    fx, fy, cx, cy = (float(x) for x in intr)
    ym, xm = np.meshgrid(np.arange(Hm, dtype=np.float64), np.arange(Wm, dtype=np.float64), indexing="ij")
    u, v = (xm + 0.5) * Wd / Wm - 0.5, (ym + 0.5) * Hd / Hm - 0.5
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1) @ pose[:3, :3].T
    o = pose[:3, 3]
    best, ids = np.full((Hm, Wm), np.inf), np.zeros((Hm, Wm), np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (BOX[0] - o) / d, (BOX[1] - o) / d
        tmin, tmax = np.nanmax(np.minimum(ta, tb), axis=-1), np.nanmin(np.maximum(ta, tb), axis=-1)
        for t, ok, sid in ((-o[2] / d[..., 2], True, FLOOR), ((WALL_Y - o[1]) / d[..., 1], True, WALL), (tmin, tmax >= tmin, BOX_ID)):
            hit = (t > 0) & np.isfinite(t) & ok & (t < best)
            best, ids = np.where(hit, t, best), np.where(hit, sid, ids)
    return ids


def dilate(mask, r):
    """Binary dilation by a (2 r + 1)-square."""
    H, W = mask.shape
    pad = np.zeros((H + 2 * r, W + 2 * r), bool)
    pad[r:r + H, r:r + W] = mask
    out = np.zeros_like(mask)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= pad[dy:dy + H, dx:dx + W]
    return out


def room_masks(poses, intr, Hm, Wm):
    """uint8 [V, 6, Hm, Wm]: non-zero = set, with values other than 1 among them."""
    V = len(poses)
    masks = np.zeros((V, 6, Hm, Wm), np.uint8)
    for v in range(V):
        if not np.isfinite(poses[v]).all():
            continue
        ids = surface_ids(poses[v], intr[v].astype(np.float64), HD, WD, Hm, Wm)
        masks[v, Q_BOX], masks[v, Q_FLOOR], masks[v, Q_WALL] = ids == BOX_ID, (ids == FLOOR) * 255, (ids == WALL) * 2
        masks[v, Q_DILATED] = dilate(ids == BOX_ID, 2)
        masks[v, Q_WHOLE] = 7
    return masks


def score_table(V, Q):
    """A fixed table: 17 levels 0.025 + 0.05 j (none within 0.019 of the default threshold 0.3) plus 0.002 (v % 4), so equal values
    abound; one NaN."""
    v, q = np.meshgrid(np.arange(V), np.arange(Q), indexing="ij")
    s = (0.025 + 0.05 * ((7 * v + 13 * q) % 17) + 0.002 * (v % 4)).astype(np.float32)
    s[min(2, V - 1), 0] = np.nan
    return s


def box_distance(p):
    """Distance of points [.., 3] to the box."""
    return np.linalg.norm(np.maximum(np.maximum(BOX[0] - p, p - BOX[1]), 0.0), axis=-1)


@functools.lru_cache(maxsize=None)
def room_case(n_bad_poses=0):
    """-> dict(poses, intr, depth_u16, depth_f32, kept, c2w, scores [V, 6], masks {size: uint8 [V, 6, Hm, Wm]}, ref {size: (centre,
    count, median, n_valid) of the kept views in float64}, dev32).  Shared by the tests: treat it as read-only."""
    rng = np.random.default_rng(SEED)
    poses, intr, depth = make_views(rng, N_VIEWS, HD, WD, n_bad_poses)
    depth_u16 = np.round(depth / DEPTH_SCALE).astype(np.uint16)
    depth_f32 = (depth_u16.astype(np.float32) * np.float32(DEPTH_SCALE)).astype(np.float32)
    c2w, kept = R.cam_to_world(poses)
    r = R.rule(**ROOM_RULE)
    args = (r["far_mm"], r["gate_mm"], r["gate_permille"])
    masks, ref, dev32 = {}, {}, 0.0
    small = large = False
    for size in MASK_SIZES:
        m = masks[size] = room_masks(poses, intr, *size)
        a = ref[size] = R.centres(depth_u16[kept], DEPTH_SCALE, intr[kept], c2w, m[kept], *args)
        b = R.centres(depth_u16[kept], DEPTH_SCALE, intr[kept], c2w, m[kept], *args, dtype=np.float32)
        assert np.array_equal(a[1], b[1]), "the float32 and float64 restatements count differently: choose another seed"
        dev32 = max(dev32, float(np.abs(a[0].astype(np.float64) - b[0]).max()))
        centre, count, _, n_valid = a
        lost = 1.0 - count[:, Q_DILATED].sum() / n_valid[:, Q_DILATED].sum()
        assert 0.2 <= lost <= 0.8, f"the dilated query loses {lost:.0%} of its pixels to the gate at {size}: choose another seed"
        small |= bool(((count > 0) & (count < r["min_pixels"])).any())
        large |= bool((count >= 512).any())
        on_box = count[:, Q_BOX] >= 4
        assert on_box.sum() >= 10, "too few views see the box: choose another seed"
        far = box_distance(centre[:, Q_BOX][on_box].astype(np.float64)).max()
        assert far <= 0.02, f"a box-query centre lies {far:.3f} m off the box at {size}: choose another seed"
        assert not count[:, Q_EMPTY].any() and not a[2][:, Q_EMPTY].any()
    assert small, "no (view, query) has 0 < count < min_pixels: choose another seed"
    assert large, "no count reaches 512: choose another seed"
    scores = score_table(N_VIEWS, 6)
    for x in [poses, intr, depth_u16, depth_f32, c2w, kept, scores] + list(masks.values()) + [y for t in ref.values() for y in t]:
        x.setflags(write=False)
    return dict(poses=poses, intr=intr, depth_u16=depth_u16, depth_f32=depth_f32, kept=kept, c2w=c2w, scores=scores, masks=masks, ref=ref,
                dev32=dev32)


def make_feats(seed, V, Q, C, dtype):
    """Random [V, Q, C] in `dtype` (fp16 values convert to fp32 exactly)."""
    return np.random.default_rng(seed).uniform(-2, 2, (V, Q, C)).astype(dtype)


# ---------------------------------------------------------------------------------------------- the hand-built case
HAND_RULE = dict(far=65.535, min_pixels=1, score_thr=0.0)


def _mask(*pixels, rows=()):
    m = np.zeros((8, 8), np.uint8)
    for y, x in pixels:
        m[y, x] = 1
    for y in rows:
        m[y, :] = 1
    return m


def hand_case_u16():
    """Five views x two queries, uint16 millimetres (depth_scale 0.001), masks 8 x 8 -> (depth, intr, poses, masks).  The last view's
    pose is finite with translation 1e30: every pixel of it is dropped at step 5."""
    depth = np.zeros((5, 8, 8), np.uint16)
    masks = np.zeros((5, 2, 8, 8), np.uint8)
    depth[0, 0, :3] = (255, 256, 257)                                  # keys across a high-byte boundary; the rest of the row is raw 0
    depth[0, 1, :2] = (511, 512)                                       # even n: the lower median
    masks[0, 0], masks[0, 1] = _mask(rows=(0,)), _mask((1, 0), (1, 1))
    depth[1, 3, 4], depth[1, 0, 0], depth[1, 7, 7] = 2000, 1000, 3000
    masks[1, 0], masks[1, 1] = _mask((3, 4)), _mask((0, 0), (7, 7))    # a single pixel; two pixels 2 m apart
    depth[2] = 1500                                                    # all 64 pixels on one key
    masks[2, 0] = 1                                                    # (query 1: empty)
    depth[3, 0, :2] = (1, 65535)                                       # the ends of the key range
    masks[3, 0], masks[3, 1] = _mask((0, 0), (0, 1)), _mask((0, 1))
    depth[4] = 1500
    masks[4, 0], masks[4, 1] = 1, _mask((2, 2))
    poses = np.stack([np.eye(4)] * 5)
    poses[4, :3, 3] = 1e30
    intr = np.tile(np.array([1, 1, 0, 0], np.float32), (5, 1))
    return depth, intr, poses, masks


# (rule, {(view, query): (median_mm, count, centre)}); w = (ui d, vi d, d) with the identity pose
HAND_EXPECT_U16 = [
    (dict(), {
        (0, 0): (256, 3, (0.77 / 3, 0.0, 0.256)), (0, 1): (511, 2, (0.256, 0.5115, 0.5115)),
        (1, 0): (2000, 1, (8.0, 6.0, 2.0)), (1, 1): (1000, 1, (0.0, 0.0, 1.0)),               # 1000 * 2000 > 1000 * 100 + 50 * 1000
        (2, 0): (1500, 64, (5.25, 5.25, 1.5)), (2, 1): (0, 0, (0.0, 0.0, 0.0)),
        (3, 0): (1, 1, (0.0, 0.0, 0.001)), (3, 1): (65535, 1, (65.535, 0.0, 65.535)),
        (4, 0): (1500, 0, (0.0, 0.0, 0.0)), (4, 1): (1500, 0, (0.0, 0.0, 0.0))}),
    (dict(gate_abs=0.0, gate_rel=0.0), {                                                       # only pixels at the median key survive
        (0, 0): (256, 1, (0.256, 0.0, 0.256)), (0, 1): (511, 1, (0.0, 0.511, 0.511)), (2, 0): (1500, 64, (5.25, 5.25, 1.5))}),
    (dict(far=2.0), {                                                                          # far_mm cuts the 3000 and the 65535 off
        (1, 0): (2000, 1, (8.0, 6.0, 2.0)), (1, 1): (1000, 1, (0.0, 0.0, 1.0)), (3, 0): (1, 1, (0.0, 0.0, 0.001)),
        (3, 1): (0, 0, (0.0, 0.0, 0.0))}),
    (dict(gate_abs=2.0), {(1, 1): (1000, 2, (10.5, 10.5, 2.0))}),                              # both pixels: (0 + 7 * 3) / 2
]


def hand_case_f32():
    """One view x two queries in fp32 metres: NaN, inf, -1 and 70.0 are invalid, 1.25 and 1.75 are not."""
    depth = np.zeros((1, 8, 8), np.float32)
    depth[0, 0, :6] = (np.nan, np.inf, -1.0, 70.0, 1.25, 1.75)
    masks = np.zeros((1, 2, 8, 8), np.uint8)
    masks[0, 0], masks[0, 1] = _mask(rows=(0,)), _mask((0, 0), (0, 1), (0, 2), (0, 3))
    return depth, np.array([[1, 1, 0, 0]], np.float32), np.eye(4)[None], masks


HAND_EXPECT_F32 = [
    (dict(gate_abs=1.0), {(0, 0): (1250, 2, ((4 * 1.25 + 5 * 1.75) / 2, 0.0, 1.5)), (0, 1): (0, 0, (0.0, 0.0, 0.0))}),
    (dict(), {(0, 0): (1250, 1, (5.0, 0.0, 1.25))}),                                           # 1000 * 500 > 1000 * 100 + 50 * 1250
]


def hand_ref(depth, depth_scale, intr, poses, masks, dtype=np.float64, **kw):
    r = R.rule(**{**HAND_RULE, **kw})
    c2w, kept = R.cam_to_world(poses)
    return R.centres(depth[kept], depth_scale, intr[kept], c2w, masks[kept], r["far_mm"], r["gate_mm"], r["gate_permille"], dtype)


def dev32():
    """The largest centre deviation of the float32 restatement from the float64 one over the room and the hand-built cases."""
    worst = room_case()["dev32"]
    for case, scale, expect in ((hand_case_u16(), DEPTH_SCALE, HAND_EXPECT_U16), (hand_case_f32(), None, HAND_EXPECT_F32)):
        for kw, _ in expect:
            a, b = hand_ref(case[0], scale, *case[1:], **kw), hand_ref(case[0], scale, *case[1:], dtype=np.float32, **kw)
            assert np.array_equal(a[1], b[1])
            worst = max(worst, float(np.abs(a[0].astype(np.float64) - b[0]).max()))
    return worst


if __name__ == "__main__":                     # the figures of profiles/lift_queries.md, "tolerance"
    c = room_case()
    for size in MASK_SIZES:
        centre, count, _, n_valid = c["ref"][size]
        lost = 1.0 - count[:, Q_DILATED].sum() / n_valid[:, Q_DILATED].sum()
        print(f"masks {size}: largest count {count.max()}, dilated query loses {lost:.0%}, "
              f"{int(((count > 0) & (count < 4)).sum())} entries with 0 < count < 4, {int((count[:, Q_BOX] >= 4).sum())} box centres")
    d = dev32()
    print(f"DEV32 = {d:.3e}; bound of the centre comparisons = 4 x that = {4 * d:.3e}")
