"""Inputs shared by the TSDF tests (tests/test_tsdf_ref.py, tests/test_gpu_tsdf.py): the scenes of tests/fuse_views_case.py with the
parameters the TSDF tests run them at, and the restatement's result for each, computed once and read-only.  No file is read."""
import functools

import numpy as np

import fuse_views_case as K
import fuse_views_ref as FR
import tsdf_ref as R

DEPTH_SCALE = K.DEPTH_SCALE
ROOM_RULE = dict(voxel=0.05, trunc=0.08)            # the room of the tests: 8 x 120 x 160 at 5 cm


def depth_of(c, kind):
    """-> (depth, depth_scale) of a case for `kind` in ("u16", "f32")."""
    return (c["depth_u16"], c.get("scale", DEPTH_SCALE)) if kind == "u16" else (c["depth_f32"], None)


def ref(c, kind="u16", **kw):
    """The restatement on a case -> (Volume, Mesh)."""
    depth, scale = depth_of(c, kind)
    return R.tsdf_mesh(depth, scale, c["intr"], c["poses"], c["colors"], **kw)


def _freeze(x):
    for a in x:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def room_ref(color_hw=(60, 80)):
    """(Volume, Mesh) of the room at ROOM_RULE.  Shared by the tests: read-only."""
    vol, mesh = ref(K.room_case(color_hw), **ROOM_RULE)
    return _freeze(vol), _freeze(mesh)


def block_face_wall(on_centres=False):
    """A wall of 16 x 40 pixels half a metre in front of the camera, at world x = -1 exactly: with voxel = 2^-5 that is the face
    between blocks -5 and -4, and the image is centred on y = z = 0, so cells and quads straddle two, four and eight blocks.
    `on_centres`: the wall moves half a voxel, onto the voxel centres, where sdf == 0 exactly.  fp32 depth only."""
    c = K.wall(16, 40, 0.5, plane_x=-1.0 + (2.0 ** -6 if on_centres else 0.0))
    return {**c, "depth_f32": np.full((1, 16, 40), 0.5, np.float32)}


BLOCK_FACE_RULE = dict(voxel=2.0 ** -5, trunc=0.125, min_weight=1)

# one partial tile of the kernels' 8 x 32 pixels; a row that crosses the 32-wide tile edge and the 64 lanes of a wave
PIXEL_RULE_SIZES = ((5, 7), (9, 65))
PIXEL_RULE_EDGES = (dict(edge_abs=0.02, edge_rel=0.02), dict(edge_abs=0.02, edge_rel=None))


def pixel_rule_case(H, W, kind):
    """One view of `K.noisy` (holes and steps at random) with what steps 2 and 3 of the pixel rule must decide planted into it: a
    zero at (1, 1), a pixel exactly at `near` at (2, 2) and one exactly at `far` at (3, 4), each with its four neighbours at the same
    depth, a step edge of 0.6 m before and after columns 5 and 6 (but for (3, 5), which belongs to a flat cross) and, for fp32, a NaN
    at (0, 3).  `near` and `far` ARE the metres of the two planted pixels.  -> the case with `depth` and `scale` of `kind`, `near`,
    `far` and `metres` fp32 [H, W]."""
    c = K.noisy(H, W, seed=H)
    raw = np.array(c["depth_u16"])                                                     # 900 .. 1700 mm
    raw[0, :, 5:7] += 600
    for (y, x), mm in (((2, 2), 905), ((3, 4), 1500)):                                 # each in a flat cross: no edge test drops it
        raw[0, y - 1:y + 2, x] = raw[0, y, x - 1:x + 2] = mm
    raw[0, 1, 1] = 0
    if kind == "u16":
        depth, scale = raw, DEPTH_SCALE
    else:
        depth, scale = raw.astype(np.float32) * np.float32(DEPTH_SCALE), None
        depth[0, 0, 3] = np.nan
    metres = FR.depth_metres(depth, scale)[0]
    return {**c, "depth": depth, "scale": scale, "metres": metres, "near": float(metres[2, 2]), "far": float(metres[3, 4])}


def pixel_rule_valid(c, edge_abs, edge_rel):
    """The restatement's steps 2 and 3 on a `pixel_rule_case` -> bool [H, W]."""
    return FR.valid_pixels(c["metres"], c["near"], c["far"], edge_abs, edge_rel)


def edge_use(faces):
    """faces int [F, 3] -> (directed edges int64 [3 F] as a * 2^32 + b, undirected likewise with a < b)."""
    f = np.asarray(faces, dtype=np.int64)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    return (a << 32) | b, (np.minimum(a, b) << 32) | np.maximum(a, b)


def face_normals(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)[:, :3]
    f = np.asarray(faces, dtype=np.int64)
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])


if __name__ == "__main__":
    vol, mesh = room_ref()
    _, und = edge_use(mesh.faces)
    _, n = np.unique(und, return_counts=True)
    print(f"room 8 x 120 x 160 at 5 cm: {len(vol.keys)} blocks, {mesh.voxels_observed} voxels observed, {vol.updates} updates, "
          f"{len(mesh.vertices)} vertices, {len(mesh.faces)} faces; edges with two faces: {(n == 2).mean():.4f}, with more: {(n > 2).sum()}")
