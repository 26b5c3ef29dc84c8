"""Inputs shared by the TSDF tests (tests/test_tsdf_ref.py, tests/test_gpu_tsdf.py): the scenes of tests/fuse_views_case.py with the
parameters the TSDF tests run them at, and the restatement's result for each, computed once and read-only.  No file is read."""
import functools

import numpy as np

import fuse_views_case as K
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
