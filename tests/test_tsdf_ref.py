"""Properties of tests/tsdf_ref.py, the numpy restatement of the TSDF rule that csrc/tsdf.hip must EQUAL (tests/test_gpu_tsdf.py):
what makes it worth equalling.  No GPU."""
import numpy as np
import pytest

import fuse_views_case as K
import tsdf_case as C
import tsdf_ref as R


# ---------------------------------------------------------------------------------------------- a plane comes out as a plane
@pytest.mark.parametrize("V, min_weight", [(1, 1), (8, 2)])
def test_wall_vertices_lie_on_the_plane_and_faces_look_at_the_camera(V, min_weight):
    """A fronto-parallel wall at camera-z d: sdf = d - z is the exact distance to the plane in every voxel, quantised to q with a
    step of trunc / 4096, so each end of an interpolated edge is off by at most half a step and a crossing, and the mean of
    crossings, by no more than 2 steps; to that comes the fp32 spacing of the products (c + 0.5 + m) * voxel near |x| = d, a few
    ulps.  Measured: 0 (the quantisation errors of the two ends of an edge are equal and cancel on this wall)."""
    trunc = 0.08
    c = K.wall(24, 32, 1.0, V=V)
    vol, mesh = C.ref(c, "f32", trunc=trunc, min_weight=min_weight)
    d = float(c["depth_f32"][0, 0, 0])
    assert len(mesh.vertices) > 1000 and len(mesh.faces) > 2000
    err = np.abs(mesh.vertices[:, 0].astype(np.float64) - d).max()
    print(f"wall, {V} views: max |x - d| = {err:.3e}")
    assert err <= 2 * trunc / 4096 + 4 * np.spacing(np.float32(d))
    n = C.face_normals(mesh.vertices, mesh.faces)
    assert (n[:, 0] < 0).all()                                                         # the camera looks along +x from x = 0
    assert mesh.vertices[:, 3:].min() >= 0 and mesh.vertices[:, 3:].max() <= 255
    assert vol.updates == int(vol.W.sum()) and mesh.voxels_observed == int((vol.W >= min_weight).sum())


# ---------------------------------------------------------------------------------------------- orientation and manifoldness
def test_room_mesh_is_oriented_and_manifold():
    vol, mesh = C.room_ref()
    V, F = len(mesh.vertices), len(mesh.faces)
    assert V > 3000 and F > 5000 and len(vol.keys) > 200
    directed, undirected = C.edge_use(mesh.faces)
    assert len(np.unique(directed)) == len(directed)                                  # every directed edge at most once
    _, uses = np.unique(undirected, return_counts=True)
    assert uses.max() <= 2
    # measured once on the restatement: 93.20 % of the edges have two faces; the others bound the holes that the views leave (the room
    # is seen from four standpoints, and a quad needs all four of its cells fully observed)
    share = (uses == 2).mean()
    print(f"room: edges with two faces {share:.4f}")
    assert abs(share - 0.9320) < 5e-4
    # the normals point into the room's free space: away from the walls, towards the standpoints
    n = C.face_normals(mesh.vertices, mesh.faces)
    centre = mesh.vertices[mesh.faces.astype(np.int64)][:, :, :3].mean(axis=1)
    floor = np.abs(centre[:, 2] - K.ROOM_LO[2]) < 0.03
    assert floor.sum() > 100 and (n[floor, 2] > 0).all()


def test_indices_and_order():
    _, mesh = C.room_ref()
    f = mesh.faces.astype(np.int64)
    assert f.min() >= 0 and f.max() < len(mesh.vertices)
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
    assert (np.diff(mesh.keys.astype(np.int64)) > 0).all()                            # ascending cell key, one vertex per cell
    assert np.isfinite(mesh.vertices).all() and len(f) % 2 == 0
    # the two triangles of a quad are adjacent and share their diagonal
    assert (f[0::2, 0] == f[1::2, 0]).all()


def test_block_face_wall_straddles_blocks_and_holds_zero_sums():
    vol, mesh = C.ref(C.block_face_wall(), "f32", **C.BLOCK_FACE_RULE)
    b = R.block_coords(vol.keys)
    assert sorted(set(b[:, 0])) == [-5, -4] and b[:, 1].min() < 0 <= b[:, 1].max() and b[:, 2].min() < 0 <= b[:, 2].max()
    assert (mesh.vertices[:, 0] == -1.0).all() and len(mesh.faces) > 50
    cells = (mesh.keys[:, None] >> np.array([42, 21, 0], np.uint64)) & np.uint64((1 << 21) - 1)
    assert ((cells.astype(np.int64) - (1 << 20)) % 8 == 7).all(axis=1).any()          # a cell whose corners lie in eight blocks
    vol, mesh = C.ref(C.block_face_wall(on_centres=True), "f32", **C.BLOCK_FACE_RULE)
    assert ((vol.W > 0) & (vol.T == 0)).sum() > 50                                    # T == 0 is outside: the crossing is at that voxel
    assert (mesh.vertices[:, 0] == np.float32(-1.0 + 2.0 ** -6)).all()


# ---------------------------------------------------------------------------------------------- set semantics
def test_merge_of_parts_is_the_volume_of_the_union():
    c = K.room_case()
    whole, _ = C.room_ref()
    parts = [R.integrate(c["depth_u16"][i], K.DEPTH_SCALE, c["intr"][i], c["poses"][i], c["colors"][i], **C.ROOM_RULE)
             for i in (np.array([5, 2]), np.array([7, 0, 3]), np.array([6, 1, 4]))]
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        vol = R.empty()
        for i in order:
            vol = R.merge(vol, parts[i])
        for got, want in zip(vol, whole):
            assert np.array_equal(got, want), order
    got = R.extract(R.merge(R.merge(parts[1], parts[2]), parts[0]), **C.ROOM_RULE)
    _, want = C.room_ref()
    assert np.array_equal(got.vertices.view(np.uint32), want.vertices.view(np.uint32)) and np.array_equal(got.faces, want.faces)


def test_nothing_to_fuse():
    c = K.wall(1, 1, 1.0)
    vol, mesh = C.ref(c, min_weight=1)
    # one pixel with fx = 1 is a frustum a metre wide: every voxel of the touched blocks inside it sees that pixel
    assert len(mesh.vertices) > 0 and len(mesh.faces) > 0 and (mesh.vertices[:, 0] == np.float32(c["depth_f32"][0, 0, 0])).all()
    dark = {**c, "depth_u16": np.zeros_like(c["depth_u16"])}
    vol, mesh = C.ref(dark, min_weight=1)
    assert len(vol.keys) == 0 and vol.updates == 0 and mesh.vertices.shape == (0, 6)


# ---------------------------------------------------------------------------------------------- the pixel-rule images decide something
@pytest.mark.parametrize("edges", C.PIXEL_RULE_EDGES, ids=("edges", "no-edges"))
@pytest.mark.parametrize("kind", ("u16", "f32"))
@pytest.mark.parametrize("H, W", C.PIXEL_RULE_SIZES)
def test_pixel_rule_images_have_valid_and_invalid_pixels(H, W, kind, edges):
    """What tests/test_gpu_tsdf.py compares `vdepth` against cannot be all zeros or all depth: every image has pixels of both kinds,
    the planted zero (and NaN) is invalid, the pixels exactly at `near` and `far` are valid where no edge test can drop them, and
    the planted step drops pixels only with the edge test on."""
    c = C.pixel_rule_case(H, W, kind)
    ok = C.pixel_rule_valid(c, **edges)
    assert ok.shape == (H, W) and ok.any() and not ok.all()
    assert not ok[1, 1] and c["metres"][1, 1] == 0
    if kind == "f32":
        assert np.isnan(c["metres"][0, 3]) and not ok[0, 3]
    assert (c["metres"][ok] >= np.float32(c["near"])).all() and (c["metres"][ok] <= np.float32(c["far"])).all()
    off = C.pixel_rule_valid(c, edge_abs=0.02, edge_rel=None)
    assert off[2, 2] and off[3, 4] and c["metres"][2, 2] == np.float32(c["near"]) and c["metres"][3, 4] == np.float32(c["far"])
    below, above = c["metres"] < np.float32(c["near"]), c["metres"] > np.float32(c["far"])
    assert (below & (c["metres"] > 0)).any() and above.any() and not off[below | above].any()
    on = C.pixel_rule_valid(c, edge_abs=0.02, edge_rel=0.02)
    assert (off & ~on).any() and not (on & ~off).any()                                 # the edge test only drops pixels
    assert on[2, 2] and on[3, 4]                                                       # >= near and <= far hold in both variants
    step = off[:, 7 if W > 7 else 4] & ~on[:, 7 if W > 7 else 4]                       # a column beside the planted step
    assert step.any()
