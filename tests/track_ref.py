"""The rule of segdino3d_amd/track.py (include/segdino3d_hip.h, "Camera tracking ...") restated in numpy: what csrc/track.hip is tested
against, bit for bit.  The steps carry the numbers of the module's docstring.  Every float operation of steps 1 to 4 is a single
float32 numpy operation in the stated order; the sums are int64 matrix products of integers (numpy multiplies integers itself, no
BLAS); the solve and the update are `np.float64` SCALAR operations, one rounding each - no `@`, `dot` or `linalg` there, which may fuse.

A volume is a `tsdf_ref.Volume`.  A pose is float64 [3, 4] = [R | t], cam_to_world."""
import math

import numpy as np

import fuse_views_ref as FR
import tsdf_ref as TR

F32, F64 = np.float32, np.float64
DEFAULT_SCHEDULE = ((4, 3), (2, 3), (1, 3))
RULE_DEFAULTS = dict(track_min_weight=1, min_samples=64, damping=1e-6, max_rot=0.5, max_trans=None, schedule=DEFAULT_SCHEDULE)
TSDF_KEYS = ("voxel", "trunc", "near", "far", "edge_abs", "edge_rel", "min_weight")
TRI = [(i, j) for i in range(6) for j in range(i, 6)]                                  # the 21 sums of A: the upper triangle, row-major


def split_rule(**kw):
    """-> (tracker parameters, TSDF rule) with the defaults filled in."""
    t = {**RULE_DEFAULTS, **{k: v for k, v in kw.items() if k in RULE_DEFAULTS}}
    r = TR.rule(**{k: v for k, v in kw.items() if k not in RULE_DEFAULTS})
    if t["max_trans"] is None:
        t["max_trans"] = 4.0 * float(r["trunc"])
    return t, r


def constants(t, r):
    """The host constants: each made in float64 and rounded ONCE to fp32; the solve widens them again."""
    k = TR.constants(r)
    k["ymax"] = F32(float(r["far"]) * math.sqrt(3.0))
    k["damping"], k["max_rot"], k["max_trans"] = F32(t["damping"]), F32(t["max_rot"]), F32(t["max_trans"])
    return k


def lookup(vol, c):
    """voxel coordinates int64 [N, 3], all inside [-2^20, 2^20) -> (W, T int64 [N]), 0 for a voxel of no block."""
    if len(vol.keys) == 0:
        return np.zeros(len(c), np.int64), np.zeros(len(c), np.int64)
    key = TR.block_keys(c >> 3)
    loc = ((c[:, 0] & 7) << 6) | ((c[:, 1] & 7) << 3) | (c[:, 2] & 7)
    pos = np.minimum(np.searchsorted(vol.keys, key), len(vol.keys) - 1)
    hit = vol.keys[pos] == key
    return np.where(hit, vol.W[pos, loc], 0), np.where(hit, vol.T[pos, loc], 0)


def _lerp(a, b, f):
    return a + (b - a) * f


def rows(vol, d, ok, intr, pose, stride, k, track_min_weight=1):
    """Steps 1 to 4 of one iteration up to the integer rows: d fp32 [Hd, Wd] and `ok` from step 1 of the TSDF rule, pose float64 [3, 4]
    -> (Jq int64 [N, 6], rq int64 [N]), one row per sample that survives, in row-major pixel order."""
    sel = np.zeros_like(ok)
    sel[::stride, ::stride] = True
    vi, ui = np.nonzero(ok & sel)
    fx, fy, cx, cy = (F32(x) for x in intr)
    M = np.asarray(pose, F64).astype(F32)                                               # the fp32 rounding of the state
    with np.errstate(all="ignore"):
        dd = d[vi, ui]
        px = (ui.astype(F32) - cx) * dd / fx
        py = (vi.astype(F32) - cy) * dd / fy
        y = np.stack([(M[i, 0] * px + M[i, 1] * py) + M[i, 2] * dd for i in range(3)], axis=1)
        w = y + M[:, 3][None]
        fine = (np.abs(w) < F32(2 ** TR.WORLD_BITS)).all(axis=1) & (np.abs(y) <= k["ymax"]).all(axis=1)      # a NaN fails
        g = w * k["inv_voxel"] - F32(0.5)
        c = np.floor(g)
        f = g - c
        fine &= ((c >= F32(-2 ** TR.CELL_BITS)) & (c + F32(1) < F32(2 ** TR.CELL_BITS))).all(axis=1)
    y, c, f = y[fine], c[fine].astype(np.int64), f[fine]
    val = {}
    seen = np.ones(len(c), dtype=bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                W, T = lookup(vol, c + np.array([dx, dy, dz]))
                seen &= W >= track_min_weight
                with np.errstate(all="ignore"):
                    val[dx, dy, dz] = (T.astype(F64) / W.astype(F64)).astype(F32) * F32(1.0 / 4096.0)
    y, f = y[seen], f[seen]
    v = {key: a[seen] for key, a in val.items()}
    fx_, fy_, fz_ = f[:, 0], f[:, 1], f[:, 2]
    # phi: along x, then y, then z
    cx_ = {(b, e): _lerp(v[0, b, e], v[1, b, e], fx_) for b in (0, 1) for e in (0, 1)}
    cy_ = {e: _lerp(cx_[0, e], cx_[1, e], fy_) for e in (0, 1)}
    phi = _lerp(cy_[0], cy_[1], fz_)
    # the gradient: the same lerps over the four corner differences along each axis
    dx_ = {(b, e): v[1, b, e] - v[0, b, e] for b in (0, 1) for e in (0, 1)}
    nx = _lerp(_lerp(dx_[0, 0], dx_[1, 0], fy_), _lerp(dx_[0, 1], dx_[1, 1], fy_), fz_)
    dy_ = {(a, e): v[a, 1, e] - v[a, 0, e] for a in (0, 1) for e in (0, 1)}
    ny = _lerp(_lerp(dy_[0, 0], dy_[1, 0], fx_), _lerp(dy_[0, 1], dy_[1, 1], fx_), fz_)
    dz_ = {(a, b): v[a, b, 1] - v[a, b, 0] for a in (0, 1) for b in (0, 1)}
    nz = _lerp(_lerp(dz_[0, 0], dz_[1, 0], fx_), _lerp(dz_[0, 1], dz_[1, 1], fx_), fy_)
    q = y * k["inv_voxel"]
    J = np.stack([q[:, 1] * nz - q[:, 2] * ny, q[:, 2] * nx - q[:, 0] * nz, q[:, 0] * ny - q[:, 1] * nx, nx, ny, nz], axis=1)
    Jq = np.rint(J * F32(1024)).astype(np.int64).reshape(-1, 6)
    rq = np.rint(phi * F32(16384)).astype(np.int64)
    return Jq, rq


def sums(Jq, rq):
    """The 29 integer sums -> int64 [29]: A (21, the upper triangle row-major), b (6), count, e."""
    A = Jq.T @ Jq                                                                       # int64 x int64: exact, numpy's own loop
    b = Jq.T @ rq
    return np.concatenate([np.array([A[i, j] for i, j in TRI], np.int64), b, np.array([len(rq), int((rq * rq).sum())], np.int64)])


def solve(s, k, min_samples):
    """Step 5 -> x as six np.float64, or None when the iteration is lost."""
    if int(s[27]) < min_samples:
        return None
    A = [[F64(0)] * 6 for _ in range(6)]
    for n, (i, j) in enumerate(TRI):
        A[i][j] = A[j][i] = F64(int(s[n]))
    b = [F64(int(s[21 + i])) for i in range(6)]
    scale = F64(1) + F64(k["damping"])
    for i in range(6):
        A[i][i] = F64(1) if int(s[TRI.index((i, i))]) == 0 else A[i][i] * scale          # a variable no sample moves with: x_i = 0
    L = [[F64(0)] * 6 for _ in range(6)]
    D = [F64(0)] * 6
    with np.errstate(all="ignore"):
        for j in range(6):
            dj = A[j][j]
            for m in range(j):
                dj = dj - L[j][m] * (L[j][m] * D[m])
            if not dj > 0:
                return None
            D[j] = dj
            for i in range(j + 1, 6):
                t = A[i][j]
                for m in range(j):
                    t = t - L[j][m] * (L[i][m] * D[m])
                L[i][j] = t / dj
        z = [F64(0)] * 6
        for i in range(6):
            t = b[i]
            for m in range(i):
                t = t - L[i][m] * z[m]
            z[i] = t
        x = [F64(0)] * 6
        for i in range(5, -1, -1):
            t = z[i] / D[i]
            for m in range(i + 1, 6):
                t = t - L[m][i] * x[m]
            x[i] = t
        x = [-(xi * F64(0.0625)) for xi in x]
        if not all(abs(xi) <= F64(np.finfo(np.float64).max) for xi in x):
            return None
        vox = F64(k["voxel"])
        tv = [x[3 + i] * vox for i in range(3)]
        rot2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]
        tr2 = (tv[0] * tv[0] + tv[1] * tv[1]) + tv[2] * tv[2]
        if rot2 > F64(k["max_rot"]) * F64(k["max_rot"]) or tr2 > F64(k["max_trans"]) * F64(k["max_trans"]):
            return None
    return x


def update(pose, x, k):
    """Step 6 -> the new pose float64 [3, 4]."""
    P = [[F64(pose[i][j]) for j in range(4)] for i in range(3)]
    a = [x[i] * F64(0.5) for i in range(3)]
    aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    den, one, two = F64(1) + aa, F64(1) - aa, F64(2)
    p01, p02, p12 = two * (a[0] * a[1]), two * (a[0] * a[2]), two * (a[1] * a[2])
    dR = [[(one + two * (a[0] * a[0])) / den, (p01 - two * a[2]) / den, (p02 + two * a[1]) / den],
          [(p01 + two * a[2]) / den, (one + two * (a[1] * a[1])) / den, (p12 - two * a[0]) / den],
          [(p02 - two * a[1]) / den, (p12 + two * a[0]) / den, (one + two * (a[2] * a[2])) / den]]
    vox = F64(k["voxel"])
    out = np.zeros((3, 4), F64)
    for i in range(3):
        for j in range(3):
            out[i, j] = (dR[i][0] * P[0][j] + dR[i][1] * P[1][j]) + dR[i][2] * P[2][j]
        out[i, 3] = P[i][3] + x[3 + i] * vox
    return out


def matrices(pose):
    """pose float64 [3, 4] -> (cam_to_world, world_to_cam) fp32 [3, 4]: world_to_cam = [R^T | -(R^T t)], the translation as
    -((R_0i t_0 + R_1i t_1) + R_2i t_2) in float64, every entry rounded once."""
    P = np.asarray(pose, F64)
    w2c = np.zeros((3, 4), F64)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                w2c[i, j] = P[j, i]
            w2c[i, 3] = -((P[0, i] * P[0, 3] + P[1, i] * P[1, 3]) + P[2, i] * P[2, 3])
    return P.astype(F32), w2c.astype(F32)


def track_frame(vol, depth, depth_scale, intr, pose, **kw):
    """One frame against `vol` from `pose` float64 [3, 4] -> (pose or None when lost, count, e of the last iteration that ran,
    trace = [(stride, count, e)] of every iteration that ran)."""
    t, r = split_rule(**kw)
    k = constants(t, r)
    d = FR.depth_metres(depth, depth_scale)
    ok = FR.valid_pixels(d, r["near"], r["far"], r["edge_abs"], r["edge_rel"])
    cur, trace = np.array(pose, F64), []
    for stride, iters in t["schedule"]:
        for _ in range(iters):
            s = sums(*rows(vol, d, ok, intr, cur, stride, k, t["track_min_weight"]))
            trace.append((stride, int(s[27]), int(s[28])))
            x = solve(s, k, t["min_samples"])
            if x is None:
                return None, int(s[27]), int(s[28]), trace
            cur = update(cur, x, k)
    return cur, trace[-1][1], trace[-1][2], trace


def track(depth, depth_scale, intr, colors, first_pose=None, **kw):
    """An ordered stream of frames -> dict(poses float64 [V, 4, 4] with NaN for lost frames, lost bool [V], count, e int64 [V],
    volume = the tsdf_ref.Volume after all frames, c2w, w2c fp32 [V, 3, 4])."""
    t, r = split_rule(**kw)
    V = depth.shape[0]
    state = np.array(np.eye(4) if first_pose is None else first_pose, F64)[:3]
    vol = TR.empty()
    poses, lost = np.full((V, 4, 4), np.nan), np.zeros(V, bool)
    count, e = np.zeros(V, np.int64), np.zeros(V, np.int64)
    c2w, w2c = np.zeros((V, 3, 4), F32), np.zeros((V, 3, 4), F32)
    for v in range(V):
        emitted = state
        if v > 0:
            got, count[v], e[v], _ = track_frame(vol, depth[v], depth_scale, intr[v], state, **kw)
            lost[v] = got is None
            emitted = np.full((3, 4), np.nan) if got is None else got
            state = state if got is None else got
        if not lost[v]:
            poses[v, :3], poses[v, 3] = emitted, [0.0, 0.0, 0.0, 1.0]
        c2w[v], w2c[v] = matrices(emitted)
        vol = TR.merge(vol, TR.integrate_kept(depth[v:v + 1], depth_scale, intr[v:v + 1], c2w[v:v + 1], w2c[v:v + 1], colors[v:v + 1], **r))
    return dict(poses=poses, lost=lost, count=count, e=e, volume=vol, c2w=c2w, w2c=w2c)
