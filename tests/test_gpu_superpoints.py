"""csrc/superpoints.hip + `segdino3d_amd.superpoints` against the restatement tests/superpoints_ref.py (the reference has no counterpart).

No tolerance anywhere: a segmentation is discontinuous in its weights, so labels, `count` and `bad_faces` must EQUAL the restatement,
and so must the intermediate values the Python layer can reach (`debug=True`): the vertex normals and the edge weights, compared as bit
patterns.  If labels ever differ, the first thing to know is whether a weight differed by a bit."""
import functools

import numpy as np
import pytest
import torch

import superpoints_case as K
import superpoints_ref as R

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _hand_cases():
    tri = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]], dtype=np.float32), np.array([[0, 1, 2]]))
    v8, f8 = K.flat_grid(8)
    bad = (v8, np.concatenate([np.array([[0, 1, 64]]), f8, np.array([[-1, 2, 3], [5, 6, 1 << 40]])]))
    vp, fp = K.boxes_on_plane(24, 5)
    degenerate = (vp, np.concatenate([np.array([[0, 1, 2], [5, 9, 20], [3, 3, 7], [9, 4, 4], [2, 2, 2]]), fp]))
    vn, fn = K.height_field(12, 6)
    vn = vn.copy()
    vn[5] = np.nan
    vn[40, 2] = np.inf
    vn[77] = (-np.inf, np.inf, 3.0e38)
    vn[100] = 3.0e38
    return {"triangle": tri, "flat60": K.flat_grid(60), "crease": K.crease(8, 8), "tail_attached": K.grid_with_tail(True),
            "tail_detached": K.grid_with_tail(False), "bad_faces": bad, "degenerate": degenerate, "nan_inf": (vn, fn),
            "one_vertex": (np.zeros((1, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int64)),
            "no_vertex": (np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int64)),
            "no_vertex_faces": (np.zeros((0, 3), dtype=np.float32), np.array([[0, 0, 0], [0, 1, 2]])),
            "no_faces": (np.arange(21, dtype=np.float32).reshape(7, 3), np.zeros((0, 3), dtype=np.int64))}


HAND = _hand_cases()


@functools.lru_cache(maxsize=None)
def mesh(name):
    """The shared meshes, built once and never written to."""
    if name in HAND:
        v, f = HAND[name]
    else:
        kind, n, seed = name.split(":")
        v, f = (K.height_field if kind == "field" else K.boxes_on_plane)(int(n), int(seed))
    v, f = np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int64)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f


@functools.lru_cache(maxsize=None)
def reference(name, k_thresh=0.01, min_verts=20):
    v, f = mesh(name)
    return R.mesh_superpoints(v, f, k_thresh=k_thresh, min_verts=min_verts, debug=True)


def _run(name, d, faces_dtype=torch.int64, **kw):
    from segdino3d_amd import superpoints
    v, f = mesh(name)
    ft = torch.from_numpy(f.copy())
    if faces_dtype == torch.int32:
        ft = ft.clamp(-(1 << 31), (1 << 31) - 1).to(torch.int32)                      # an index out of range stays out of range
    return superpoints.mesh_superpoints(torch.from_numpy(v.copy()).to(d), ft.to(d), debug=True, **kw)


def _check(name, d, faces_dtype=torch.int64, **kw):
    want = reference(name, **kw)
    labels, info = _run(name, d, faces_dtype, **kw)
    v, f = mesh(name)
    assert labels.dtype == torch.int64 and labels.is_cuda and tuple(labels.shape) == (len(v),)
    got_n, got_w = info.normals.cpu().numpy(), info.weights.cpu().numpy().view(np.uint32)
    nd = int((got_n.view(np.uint32) != want.normals.view(np.uint32)).sum())
    wd = int((got_w != want.weights).sum())
    ld = int((labels.cpu().numpy() != want.labels).sum())
    print(f"{name} {kw}: N {len(v)} E {3 * len(f)} S {want.count}: normals differing {nd}, weights differing {wd}, labels differing {ld}, "
          f"settled {info.settled.tolist()}")
    assert nd == 0, f"{name}: {nd} vertex normal components differ in their bits"
    assert wd == 0, f"{name}: {wd} edge weights differ in their bits"
    assert torch.equal(labels.cpu(), torch.from_numpy(want.labels)), name
    assert info.count == want.count and info.bad_faces == want.bad_faces, name
    return labels, info


@pytest.mark.parametrize("name", sorted(HAND))
def test_edge_shapes_equal_the_restatement(name):
    d = dev()
    labels, info = _check(name, d)
    if name == "triangle":
        assert labels.tolist() == [0, 0, 0, 1]
    if name == "no_faces":
        assert labels.tolist() == list(range(7)) and info.count == 7
    if name == "no_vertex_faces":
        assert info.count == 0 and info.bad_faces == 2
    if name == "bad_faces":
        assert info.bad_faces == 3


@pytest.mark.parametrize("name", ["field:40:1", "field:120:1", "plane:80:1"])
def test_meshes_equal_the_restatement(name):
    """1 600 vertices / several sweep batches; 14 400 vertices / 85 k edges, batches whose every edge survives into the LDS table; the
    noise-free case where nearly every weight ties and the order among equals decides (tests/test_superpoints_ref.py shows it does)."""
    d = dev()
    _, info = _check(name, d)
    assert info.count > 2
    assert int(info.settled[0]) > 512                                                 # more than one batch's worth went through the table


@pytest.mark.parametrize("kw", [dict(min_verts=1), dict(min_verts=200), dict(k_thresh=0.0), dict(k_thresh=0.5)],
                         ids=["min_verts1", "min_verts200", "k0", "k0.5"])
def test_rule_parameters(kw):
    d = dev()
    _, info = _check("field:40:1", d, **kw)
    if kw.get("min_verts") == 1:
        assert int(info.settled[1]) == 0                                              # pass 2 has nothing to do


@pytest.mark.parametrize("name", ["field:40:1", "bad_faces", "plane:80:1"])
def test_int32_faces(name):
    _check(name, dev(), faces_dtype=torch.int32)


@pytest.mark.parametrize("order", [(0, 1, 2, 3), (3, 1, 0, 2)])
def test_batch_equals_the_single_runs(order):
    from segdino3d_amd import superpoints
    d = dev()
    names = ["field:40:1", "no_faces", "plane:80:1", "tail_attached"]
    meshes = [(torch.from_numpy(mesh(n)[0].copy()).to(d), torch.from_numpy(mesh(n)[1].copy()).to(d)) for n in names]
    single = [superpoints.mesh_superpoints(v, f, debug=True) for v, f in meshes]
    labels, infos = superpoints.mesh_superpoints_batch([meshes[i] for i in order], debug=True)
    assert len(labels) == 4
    for slot, i in enumerate(order):
        s_labels, s_info = single[i]
        assert torch.equal(labels[slot], s_labels), names[i]
        assert torch.equal(infos[slot].normals.view(torch.int32), s_info.normals.view(torch.int32)), names[i]
        assert torch.equal(infos[slot].weights, s_info.weights), names[i]
        assert (infos[slot].count, infos[slot].bad_faces) == (s_info.count, s_info.bad_faces), names[i]
        assert torch.equal(labels[slot].cpu(), torch.from_numpy(reference(names[i]).labels)), names[i]
    plain = superpoints.mesh_superpoints_batch([meshes[i] for i in order])
    assert all(torch.equal(a, b) for a, b in zip(plain, labels))


def test_other_stream_and_reused_workspace_give_the_same_bits():
    from segdino3d_amd import superpoints
    d = dev()
    v, f = (torch.from_numpy(a.copy()).to(d) for a in mesh("field:40:1"))
    v2, f2 = (torch.from_numpy(a.copy()).to(d) for a in mesh("plane:80:1"))
    first, info = superpoints.mesh_superpoints(v, f, return_info=True)
    other = superpoints.mesh_superpoints(v2, f2)                                      # a larger mesh through the same workspace
    again = superpoints.mesh_superpoints(v, f)
    assert torch.equal(first, again)
    assert torch.equal(other.cpu(), torch.from_numpy(reference("plane:80:1").labels))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        streamed, info_s = superpoints.mesh_superpoints(v, f, return_info=True)
    s.synchronize()
    assert torch.equal(first, streamed) and (info.count, info.bad_faces) == (info_s.count, info_s.bad_faces)
    assert info.count == reference("field:40:1").count


def test_argument_errors():
    from segdino3d_amd import superpoints
    d = dev()
    v, f = (torch.from_numpy(a.copy()).to(d) for a in mesh("tail_attached"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        superpoints.mesh_superpoints(v.cpu(), f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        superpoints.mesh_superpoints(v, f.cpu())
    for bad_v in (v.double(), v.half(), v[:, :2], v.reshape(-1)):
        with pytest.raises(ValueError):
            superpoints.mesh_superpoints(bad_v, f)
    for bad_f in (f.to(torch.int16), f.float(), f[:, :2], f.reshape(-1)):
        with pytest.raises(ValueError):
            superpoints.mesh_superpoints(v, bad_f)
    for k in (float("nan"), float("inf"), -0.01, 1e39):
        with pytest.raises(ValueError):
            superpoints.mesh_superpoints(v, f, k_thresh=k)
    for m in (0, -3, 2.5):
        with pytest.raises(ValueError):
            superpoints.mesh_superpoints(v, f, min_verts=m)
    with pytest.raises(ValueError, match="2\\^24"):
        superpoints.mesh_superpoints(torch.empty(1 << 24, 3, device=d), f)
    with pytest.raises(ValueError):
        superpoints.mesh_superpoints_batch([])
    with pytest.raises(ValueError):
        superpoints.mesh_superpoints_batch([(v, f), (v, f.to(torch.int32))])
