"""Inputs shared by the rasteriser tests (tests/test_raster_ref.py, tests/test_gpu_raster.py) and the restatement's result for the
larger ones, computed once.  No file is read; everything is cached and read-only.

The hand-built cases use an identity pose (camera at the origin, x right, y down, z forward) and power-of-two intrinsics, so that
every fp32 operation of steps 2 and 3 is exact and a case is what its name says."""
import functools

import numpy as np

import fuse_views_case as FK
import raster_ref as R
import tsdf_case as TK

F32 = np.float32
IDENTITY = np.eye(4)[None]


def _ro(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def pixel_mesh(corners_px, z=2.0, f=64.0, cx=0.0, cy=0.0):
    """Triangles given by their corners in PIXELS, [F, 3, 2] as (u, v), on the plane z_c = `z` of an identity-pose camera with
    fx = fy = `f` -> (vertices fp32 [3 F, 3], faces int32 [F, 3], intr fp32 [1, 4]).  With `z` and `f` powers of two and corners that
    are multiples of 1/256 (below 2^14) every operation of the projection is exact: the snapped corner IS 256 times the given one."""
    c = np.asarray(corners_px, dtype=np.float64).reshape(-1, 3, 2)
    xyz = np.concatenate([(c - [cx, cy]) * (z / f), np.full(c.shape[:2] + (1,), z)], axis=2).reshape(-1, 3)
    faces = np.arange(len(xyz), dtype=np.int32).reshape(-1, 3)
    assert np.array_equal(xyz.astype(F32).astype(np.float64), xyz), "the case must be exact in fp32"
    return xyz.astype(F32), faces, np.array([[f, f, cx, cy]], dtype=F32)


def box_triangle(x0, y0, bw, bh):
    """One triangle in pixels whose bounding box holds exactly the pixel centres [x0, x0 + bw) x [y0, y0 + bh): its corners lie a
    quarter pixel inside the outer centres' far side, so the clamped box is bw x bh and its area bw * bh."""
    return [[x0, y0], [x0 + bw - 1 + 0.25, y0], [x0, y0 + bh - 1 + 0.25]]


@functools.lru_cache(maxsize=None)
def soup():
    """2 000 random triangles plus three wall-sized ones seen by 3 cameras of 64 x 80, the pose of the second NaN: triangles of every
    size class, some behind the camera, some beyond `far`, some off the image, and depth ties wherever the coincident pair of walls shows.  -> dict
    (vertices, faces, intr, poses, H, W, face_labels [3, F], vertex_labels [5, Nv])."""
    rng = np.random.default_rng(5)
    n = 2000
    centre = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2.5, 2.5, n), rng.uniform(-0.5, 7.0, n)], axis=1)
    size = rng.choice([0.03, 0.1, 0.4, 1.0], n, p=[0.45, 0.35, 0.17, 0.03])[:, None, None]
    tri = centre[:, None, :] + rng.uniform(-1, 1, (n, 3, 3)) * size
    walls = np.array([[[-40, -40, 5.5], [40, -40, 5.5], [0, 50, 5.5]],                 # covers every image whole
                      [[-10, -10, 2.0], [-10, 10, 2.0], [10, 10, 2.0]],                # half of the image, in front of it ...
                      [[-10, -10, 2.0], [10, 10, 2.0], [-10, 10, 2.0]]])               # ... and the same again, wound the other way: ties
    vertices = np.concatenate([tri.reshape(-1, 3), walls.reshape(-1, 3)]).astype(F32)
    faces = np.arange(len(vertices), dtype=np.int32).reshape(-1, 3)
    faces = faces[rng.permutation(len(faces))]
    poses = np.stack([np.eye(4), np.eye(4), FK.look_at(np.array([0.5, -0.2, 0.3]), np.array([0.3, 0.1, 4.0]))])
    poses[1, 2, 3] = np.nan
    H, W = 64, 80
    intr = np.array([[64, 64, 40, 32], [64, 64, 40, 32], [70.5, 69.25, 38.7, 30.9]], dtype=F32)
    return freeze(dict(vertices=vertices, faces=faces, intr=intr, poses=poses, H=H, W=W,
                       face_labels=rng.integers(-1, 40, (3, len(faces))).astype(np.int32),
                       vertex_labels=rng.integers(-1, 40, (5, len(vertices))).astype(np.int32)))


@functools.lru_cache(maxsize=None)
def soup_ref(fill=-1, reverse_ties=False):
    c = soup()
    out = R.render_mesh(c["vertices"], c["faces"], c["intr"], c["poses"], c["H"], c["W"], face_labels=c["face_labels"],
                        vertex_labels=c["vertex_labels"], fill=fill, reverse_ties=reverse_ties)
    return freeze(out)


@functools.lru_cache(maxsize=None)
def room():
    """The surface-net mesh of tests/tsdf_case.room_ref() and two of the room's own poses at 120 x 160 -> dict."""
    _, mesh = TK.room_ref()
    c = FK.room_case()
    return freeze(dict(vertices=np.ascontiguousarray(mesh.vertices[:, :3], dtype=F32), faces=np.ascontiguousarray(mesh.faces, dtype=np.int32),
                       intr=np.ascontiguousarray(c["intr"][[0, 5]]), poses=np.ascontiguousarray(c["poses"][[0, 5]]), H=120, W=160))


@functools.lru_cache(maxsize=None)
def room_ref():
    c = room()
    return freeze(R.render_mesh(c["vertices"], c["faces"], c["intr"], c["poses"], c["H"], c["W"]))


@functools.lru_cache(maxsize=None)
def random_mesh():
    """A small random mesh for the ray-caster comparison: 10 triangles with edges of 6 px and far more, at depths 1.5 .. 4 and tilted
    in depth, seen by one slightly turned camera of 96 x 128.  Few and large, so that most hit pixels lie more than a pixel from
    every projected edge -> dict."""
    rng = np.random.default_rng(11)
    n = 10
    z = rng.uniform(1.5, 4.0, n)
    centre = np.stack([rng.uniform(-0.35, 0.35, n) * z, rng.uniform(-0.25, 0.25, n) * z, z], axis=1)
    tri = centre[:, None, :] + rng.uniform(-1, 1, (n, 3, 3)) * (0.3 * z)[:, None, None] * np.array([1, 1, 0.5])
    vertices = tri.reshape(-1, 3).astype(F32)
    faces = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
    poses = FK.look_at(np.array([0.05, -0.03, -0.1]), np.array([0.0, 0.02, 3.0]))[None]
    return freeze(dict(vertices=vertices, faces=faces, intr=np.array([[120.0, 122.0, 63.5, 47.5]], dtype=F32), poses=poses, H=96, W=128))
