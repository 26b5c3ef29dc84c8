"""The rule of segdino3d_amd/raster.py (include/segdino3d_hip.h, "Mesh rasteriser") restated in numpy: what csrc/raster.hip is tested
against, bit for bit, since the reference ships no rasteriser.  No torch, no device code, no record lists, no size classes and no
passes: every drawn face of every view is walked over its clamped bounding box, in ascending face order, into one key image.

  1-4. `setup`: fp32 with one rounding per operation (numpy rounds every float32 operation on its own), the snap to 1/256 pixel, the
       int64 area and the clamped bounding box, for all faces of one view at once -> the class of every (view, face) pair.
  4-6. `weights`, `depth_of`, `draw`: int64 edge functions, float64 depth rounded once to fp32, the key (bits of d << 32) | face.
  7.   `resolve`: depth, face, vertex (the weights recomputed for the winning face), label images.
  8.   the counters, plus `samples`: the covered in-range samples, which is the number of atomics the kernels issue.

`reverse_ties=True` prefers the HIGHER face index among equal depths (not the rule: it exists so that a test can show that the ties
exist and matter)."""
import numpy as np

import lift2d_ref as LR

F32 = np.float32
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
LIMIT = F32(16384.0)
SUB = 256
DRAWN, NEAR, GUARD, EMPTY, BAD = range(5)
INFO = ("drawn", "near", "guard", "empty", "bad", "pixels")

world_to_cam = LR.world_to_cam                          # float64 inverse of the finite poses, each entry rounded once -> (fp32 [K, 3, 4], kept)


def edge(ax, ay, bx, by, px, py):
    """E(a, b, P) on int64 arrays."""
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def setup(vertices, faces, w2c, intr, near, H, W):
    """Steps 1 to 4 up to the bounding box for all faces of ONE view (w2c fp32 [3, 4], intr fp32 [4]) -> dict(cls int [F], X, Y int64
    [F, 3], q float64 [F, 3], A int64 [F], x0, x1, y0, y1 int64 [F]); only the rows with cls == DRAWN mean anything."""
    v = np.ascontiguousarray(np.asarray(vertices)[:, :3], dtype=F32)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    F, Nv = len(f), len(v)
    r, k = np.asarray(w2c, dtype=F32), np.asarray(intr, dtype=F32)
    near = F32(near)
    index_ok = ((f >= 0) & (f < Nv)).all(axis=1)
    safe = np.where(index_ok[:, None], f, 0)
    p = v[safe] if Nv else np.zeros((F, 3, 3), F32)                                    # [F, corner, axis]
    with np.errstate(all="ignore"):
        bad = ~index_ok | ~(np.abs(p) < LIMIT).all(axis=(1, 2))                        # a NaN or an infinity fails
        x, y, z = p[..., 0], p[..., 1], p[..., 2]
        cam = [((r[i, 0] * x + r[i, 1] * y) + r[i, 2] * z) + r[i, 3] for i in range(3)]
        xc, yc, zc = cam
        behind = (zc < near).any(axis=1)
        u = (k[0] * xc) / zc + k[2]
        w = (k[1] * yc) / zc + k[3]
        inside = ((np.abs(u) < LIMIT) & (np.abs(w) < LIMIT)).all(axis=1)
        usable = ~bad & ~behind & inside
        X = np.where(usable[:, None], np.rint(u * F32(SUB)), 0).astype(np.int64)
        Y = np.where(usable[:, None], np.rint(w * F32(SUB)), 0).astype(np.int64)
        q = 1.0 / zc.astype(np.float64)
    A = edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
    x0, x1 = np.maximum((X.min(axis=1) + (SUB - 1)) >> 8, 0), np.minimum(X.max(axis=1) >> 8, W - 1)
    y0, y1 = np.maximum((Y.min(axis=1) + (SUB - 1)) >> 8, 0), np.minimum(Y.max(axis=1) >> 8, H - 1)
    empty = (A == 0) | (x0 > x1) | (y0 > y1)
    cls = np.where(bad, BAD, np.where(behind, NEAR, np.where(~inside, GUARD, np.where(empty, EMPTY, DRAWN))))
    return dict(cls=cls, X=X, Y=Y, q=q, A=A, x0=x0, x1=x1, y0=y0, y1=y1, faces=f)


def weights(X, Y, A, px, py):
    """Step 4: X, Y [..., 3] and A [...] broadcast against px, py (int64, already times 256) -> (w0, w1, w2)."""
    s = np.where(A < 0, -1, 1)
    return (s * edge(X[..., 1], Y[..., 1], X[..., 2], Y[..., 2], px, py), s * edge(X[..., 2], Y[..., 2], X[..., 0], Y[..., 0], px, py),
            s * edge(X[..., 0], Y[..., 0], X[..., 1], Y[..., 1], px, py))


def depth_of(w, q, A):
    """Step 5: float64, one rounding per operation, rounded once to fp32."""
    with np.errstate(all="ignore"):
        num = (w[0].astype(np.float64) * q[..., 0] + w[1].astype(np.float64) * q[..., 1]) + w[2].astype(np.float64) * q[..., 2]
        return (np.abs(A).astype(np.float64) / num).astype(F32)


def box_pixels(s):
    """The clamped bounding-box area of every face of a `setup` (what splits the kernels' records into small and large)."""
    return (s["x1"] - s["x0"] + 1) * (s["y1"] - s["y0"] + 1)


CHUNK = 1 << 20                                         # box pixels evaluated at once


def draw(s, near, far, H, W, reverse_ties=False):
    """Steps 4 to 6 of one view: the drawn faces of `setup`'s result into a key image -> (keys uint64 [H, W], samples).  Every pixel
    centre of every face's clamped bounding box is evaluated; the boxes are laid end to end and cut into chunks of about CHUNK
    pixels (a larger box goes alone), which only bounds the memory: the image is a minimum over all samples."""
    keys = np.full(H * W, NO_KEY, dtype=np.uint64)
    near, far, samples = F32(near), F32(far), 0
    ids = np.flatnonzero(s["cls"] == DRAWN)
    area, ends = box_pixels(s)[ids], np.cumsum(box_pixels(s)[ids])
    start = 0
    while start < len(ids):
        done = ends[start - 1] if start else 0
        stop = max(start + 1, int(np.searchsorted(ends, done + CHUNK, side="right")))
        f, a = ids[start:stop], area[start:stop]
        face = np.repeat(f, a)
        off = np.arange(int(a.sum()), dtype=np.int64) - np.repeat(np.cumsum(a) - a, a)  # the pixel's number inside its own box, row-major
        bw = (s["x1"] - s["x0"] + 1)[face]
        ui, vi = s["x0"][face] + off % bw, s["y0"][face] + off // bw
        w = weights(s["X"][face], s["Y"][face], s["A"][face], ui * SUB, vi * SUB)
        assert ((w[0] + w[1] + w[2]) == np.abs(s["A"][face])).all()
        d = depth_of(w, s["q"][face], s["A"][face])
        with np.errstate(invalid="ignore"):
            keep = (w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0) & (d >= near) & (d <= far)
        low = ((0xFFFFFFFE - face) if reverse_ties else face).astype(np.uint64)
        key = (np.ascontiguousarray(d).view(np.uint32).astype(np.uint64) << np.uint64(32)) | low
        np.minimum.at(keys, (vi * W + ui)[keep], key[keep])
        samples += int(keep.sum())
        start = stop
    return keys.reshape(H, W), samples


def resolve(keys, s, reverse_ties=False):
    """Step 7 of one view -> (depth fp32 [H, W], face int32 [H, W], vertex int32 [H, W])."""
    H, W = keys.shape
    hit = keys != NO_KEY
    low = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    face = np.where(hit, 0xFFFFFFFE - low if reverse_ties else low, -1)
    depth = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(F32), F32(0))
    vertex = np.full((H, W), -1, dtype=np.int64)
    if hit.any():
        vi, ui = np.nonzero(hit)
        f = face[vi, ui]
        w = np.stack(weights(s["X"][f], s["Y"][f], s["A"][f], ui.astype(np.int64) * SUB, vi.astype(np.int64) * SUB), axis=1)
        assert (w >= 0).all()
        vertex[vi, ui] = s["faces"][f, np.argmax(w, axis=1)]                           # the first of equal maxima: the lowest corner
    return depth.astype(F32), face.astype(np.int32), vertex.astype(np.int32)


def take(labels, idx, fill):
    """labels int [L, n] or [n] read at idx (any shape), `fill` where idx < 0 -> int32 [L, ...] or [...]."""
    lab = np.asarray(labels).astype(np.int64)
    if lab.shape[-1] == 0:
        return np.full(lab.shape[:-1] + idx.shape, fill, dtype=np.int32)
    return np.where(idx >= 0, lab[..., np.where(idx >= 0, idx, 0)], fill).astype(np.int32)


def render_kept(vertices, faces, intr, w2c, H, W, near=0.1, far=6.0, face_labels=None, vertex_labels=None, fill=-1, reverse_ties=False):
    """The rule over kept views (intr fp32 [K, 4], w2c fp32 [K, 3, 4]) -> dict(depth fp32 [K, H, W], face, vertex int32 [K, H, W], info
    dict, samples int, classes int [K, F], face_label_images / vertex_label_images int32 [L, K, H, W] or [K, H, W] or None)."""
    K, F = len(w2c), len(np.asarray(faces).reshape(-1, 3))
    depth, face, vertex = np.zeros((K, H, W), F32), np.full((K, H, W), -1, np.int32), np.full((K, H, W), -1, np.int32)
    classes, samples = np.zeros((K, F), dtype=np.int64), 0
    for v in range(K):
        s = setup(vertices, faces, w2c[v], np.asarray(intr, dtype=F32)[v], near, H, W)
        keys, n = draw(s, near, far, H, W, reverse_ties)
        depth[v], face[v], vertex[v] = resolve(keys, s, reverse_ties)
        classes[v], samples = s["cls"], samples + n
    info = {name: int((classes == c).sum()) for c, name in enumerate(INFO[:5])}
    info["pixels"] = int((face >= 0).sum())
    return dict(depth=depth, face=face, vertex=vertex, info=info, samples=samples, classes=classes,
                face_label_images=None if face_labels is None else take(face_labels, face, fill),
                vertex_label_images=None if vertex_labels is None else take(vertex_labels, vertex, fill))


def render_mesh(vertices, faces, intr, cam_to_world, H, W, **kw):
    """The same from poses [V, 4, 4]: non-finite poses dropped -> the dict of `render_kept` plus `kept`."""
    w2c, kept = world_to_cam(cam_to_world)
    out = render_kept(vertices, faces, np.asarray(intr, dtype=F32)[kept], w2c, H, W, **kw)
    out["kept"] = kept
    return out
