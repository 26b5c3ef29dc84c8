"""Benchmark submission export on the device: `ops.mask_text` / `ops.label_text` against `np.savetxt(..., fmt='%d')`, the tree of
tests/golden/submission.npz (written by the reference's own evaluator) through `SubmissionWriter` and the three drop-ins, and an
end-to-end export behind `PipelinedRunner`.  Every expected byte comes from numpy / the golden, never from the package."""
import copy
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "submission.npz")
LT_TILE = 256                                                    # values per workgroup of the label kernels (csrc/submit.hip)


def savetxt(a):
    f = io.BytesIO()
    np.savetxt(f, a, fmt="%d")
    return f.getvalue()


def read_tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for fn in files:
            full = os.path.join(d, fn)
            with open(full, "rb") as f:
                out[os.path.relpath(full, root).replace(os.sep, "/")] = f.read()
    return out


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    files = {str(p): bytes(g["file_bytes"][g["file_off"][i]:g["file_off"][i + 1]]) for i, p in enumerate(g["paths"])}
    n = int(g["n"])
    scenes = []
    for si, sid in enumerate(g["scan_ids"]):
        bits = g[f"s{si}_masks"]
        masks = np.unpackbits(bits, axis=1, bitorder="little")[:, :n].astype(bool)
        scenes.append(dict(scan_id=str(sid), masks=masks, bits=bits, labels=g[f"s{si}_labels"], scores=g[f"s{si}_scores"], sem=g[f"s{si}_sem"]))
    return dict(files=files, scenes=scenes, inst_mapping=g["inst_mapping"], sem_mapping=g["sem_mapping"], n=n)


# ------------------------------------------------------------------------------------------ mask_text
@pytest.mark.parametrize("n", [0, 1, 13])
@pytest.mark.parametrize("N", [1, 7, 8, 9, 15, 16, 17, 1003, 4101])
def test_mask_text_matches_savetxt(N, n):
    from segdino3d_amd import ops
    d = torch.device("cuda:0")
    g = np.random.default_rng(1000 * N + n)
    a = (g.random((n, N)) < g.random((n, 1))).astype(np.uint8)
    if n >= 2:
        a[0], a[n - 1] = 0, 1                                     # an all-zero row and an all-one row
    if n >= 3:
        a[1] *= g.integers(1, 256, size=N).astype(np.uint8)       # any non-zero byte prints 1
    want = [savetxt(row != 0) for row in a]
    got = ops.mask_text(torch.from_numpy(a).to(d))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, (2 * N + 15) // 16 * 16)
    got = got.cpu().numpy()
    for r in range(n):
        assert got[r, :2 * N].tobytes() == want[r], (N, r)
    got_b = ops.mask_text(torch.from_numpy(a.astype(bool)).to(d)).cpu().numpy()
    assert np.array_equal(got_b[:, :2 * N], got[:, :2 * N])
    if n:
        rows = np.array([n - 1, 0, 0, n // 2, n - 1, 0] + list(range(n - 1, -1, -2)), dtype=np.int32)
        got = ops.mask_text(torch.from_numpy(a).to(d), torch.from_numpy(rows).to(d)).cpu().numpy()
        assert got.shape[0] == len(rows)
        for i, r in enumerate(rows):
            assert got[i, :2 * N].tobytes() == want[r], (N, i, r)


def test_mask_text_refuses_bad_shapes():
    from segdino3d_amd import _lib, ops
    d = torch.device("cuda:0")
    lib = _lib.load()
    m = torch.zeros(2, 24, dtype=torch.uint8, device=d)
    out = torch.full((2, 64), 0xAB, dtype=torch.uint8, device=d)
    s = torch.cuda.current_stream().cuda_stream
    assert lib.sd3d_mask_text(m.data_ptr(), 24, None, 2, out.data_ptr(), 32, s) < 0          # pitch < 2 N
    assert lib.sd3d_mask_text(m.data_ptr(), 24, None, 2, out.data_ptr(), 56, s) < 0          # pitch % 16
    assert lib.sd3d_mask_text(m.data_ptr(), 0, None, 2, out.data_ptr(), 64, s) < 0           # N <= 0
    assert lib.sd3d_mask_text(m.data_ptr(), 24, None, -1, out.data_ptr(), 64, s) < 0         # negative count
    assert lib.sd3d_mask_text(m.data_ptr(), 24, None, 0, out.data_ptr(), 64, s) == 0         # no rows: nothing happens
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())
    assert lib.sd3d_mask_text(m.data_ptr(), 24, None, 2, out.data_ptr(), 64, s) == 0
    got = out.cpu().numpy()
    assert got[:, :48].tobytes() == b"0\n" * 48 and (got[:, 48:] == 0xAB).all()              # nothing behind 2 N
    with pytest.raises(TypeError):
        ops.mask_text(torch.zeros(2, 8, dtype=torch.int32, device=d))


# ------------------------------------------------------------------------------------------ label_text
VALUES = np.array([0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 2 ** 31 - 1, -1, -2 ** 31], dtype=np.int64)


def _text(text, info):
    from segdino3d_amd import ops
    n = ops.label_text_check(info.cpu().numpy())
    return text[:n].cpu().numpy().tobytes(), n


@pytest.mark.parametrize("N", [1, 17, 1003])
def test_label_text_covers_int32(N):
    from segdino3d_amd import ops
    d = torch.device("cuda:0")
    for shift in (0, N):
        v = np.resize(np.roll(VALUES, shift), N)
        want = savetxt(v)
        text, info = ops.label_text(torch.from_numpy(v).to(d))
        assert text.numel() == 12 * N
        got, n = _text(text, info)
        assert n == len(want) and got == want
        # the same values through a table
        idx = np.resize(np.roll(np.arange(len(VALUES)), shift), N)
        got, n = _text(*ops.label_text(torch.from_numpy(idx).to(d), VALUES))
        assert n == len(want) and got == want


def test_label_text_table_at_300001():
    from segdino3d_amd import ops
    d = torch.device("cuda:0")
    g = np.random.default_rng(200)
    table = np.sort(g.choice(np.arange(1, 1192), size=200, replace=False)).astype(np.int64)     # ScanNet200-like ids of 1 - 4 digits
    idx = g.integers(0, 200, size=300001).astype(np.int64)
    want = savetxt(table[idx])
    lens = np.char.str_len(table.astype(str))[idx] + 1
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1][::LT_TILE]
    assert set((starts % 16).tolist()) == set(range(16))              # tiles whose text starts at every residue modulo 16
    lut = ops.LabelTable(table, d)
    assert lut.width == 5
    text, info = ops.label_text(torch.from_numpy(idx).to(d), lut)
    assert text.numel() == 5 * 300001
    got, n = _text(text, info)
    assert n == len(want)
    assert got == want


def test_label_text_past_the_one_workgroup_scan():
    """More than 16 384 tiles: the exclusive scan over the tile totals takes its tiled path (a single workgroup below that).  The
    values repeat with a period of three tiles, so the expected text is np.savetxt of one period, repeated."""
    from segdino3d_amd import ops
    d = torch.device("cuda:0")
    period, reps = 3 * LT_TILE, 5462
    assert period * reps // LT_TILE > 16384
    g = np.random.default_rng(9)
    table = np.array([7, 42, 155, 1164], dtype=np.int64)
    idx = g.integers(0, 4, size=period).astype(np.int64)
    want = savetxt(table[idx]) * reps
    text, info = ops.label_text(torch.from_numpy(idx).to(d).repeat(reps), table)
    got, n = _text(text, info)
    assert n == len(want)
    assert got == want


def test_label_text_empty():
    from segdino3d_amd import ops
    d = torch.device("cuda:0")
    text, info = ops.label_text(torch.zeros(0, dtype=torch.int64, device=d))
    assert info.cpu().tolist() == [0, 0] and _text(text, info) == (b"", 0)
    text, info = ops.label_text(torch.zeros(0, dtype=torch.int64, device=d), [1, 2, 3])
    assert info.cpu().tolist() == [0, 0] and _text(text, info) == (b"", 0)


def test_label_text_status_and_bounds():
    from segdino3d_amd import ops
    d = torch.device("cuda:0")
    table = np.array([3, 40, 500, 6000], dtype=np.int64)
    g = np.random.default_rng(5)
    idx = g.integers(0, 4, size=1003).astype(np.int64)
    cap = 5 * 1003

    def run(values, lut, out_cap):
        buf = torch.full((cap + 4096,), 0xAB, dtype=torch.uint8, device=d)
        text, info = ops.label_text(torch.from_numpy(values).to(d), lut, out=buf[:out_cap])
        return buf.cpu().numpy(), info.cpu().numpy()

    # an index outside the table, on either side: the line is left out (no clamp, no wrap), the status says so
    for bad in (-1, 4, 2 ** 40):
        v = idx.copy()
        v[[0, 500, 1002]] = bad
        buf, info = run(v, table, cap)
        with pytest.raises(RuntimeError, match="outside the label table"):
            ops.label_text_check(info)
        want = savetxt(table[np.delete(v, [0, 500, 1002])])
        assert info[0] == len(want) and buf[:len(want)].tobytes() == want
        assert (buf[cap:] == 0xAB).all()
    # a value outside int32 without a table
    for bad in (2 ** 31, -2 ** 31 - 1, 2 ** 62):
        v = table[idx]
        v[[1, 777]] = bad
        buf, info = run(v, None, cap)
        with pytest.raises(RuntimeError, match="outside int32"):
            ops.label_text_check(info)
        want = savetxt(np.delete(v, [1, 777]))
        assert info[0] == len(want) and buf[:len(want)].tobytes() == want
        assert (buf[cap:] == 0xAB).all()
    # a buffer that is too short: cut at out_cap, nothing behind it (a cut inside a 16-byte chunk, on a chunk border, an empty buffer)
    want = savetxt(table[idx])
    for short in (len(want) - 1, 1001, 1024, 16, 0):
        buf, info = run(idx, table, short)
        with pytest.raises(RuntimeError, match="does not fit"):
            ops.label_text_check(info)
        assert info[0] == len(want)
        assert buf[:short].tobytes() == want[:short]
        assert (buf[short:] == 0xAB).all()
    buf, info = run(idx, table, len(want))                        # exactly enough
    assert ops.label_text_check(info) == len(want) and buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAB).all()
    with pytest.raises(ValueError, match="2\\^31"):
        ops.label_text(torch.zeros(1, dtype=torch.int64, device=d).expand(2 ** 28))


# ------------------------------------------------------------------------------------------ the golden tree
def _pred(scene, how, d):
    from segdino3d_amd.architecture import PackedMasks
    if how == "device":
        conv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)                       # noqa: E731
        masks = conv(scene["masks"])
    elif how == "host":
        conv = lambda a: a                                                                     # noqa: E731
        masks = scene["masks"]
    else:
        conv = lambda a: a                                                                     # noqa: E731
        masks = PackedMasks(scene["bits"], scene["masks"].shape[1])
    sem = conv(scene["sem"])
    return dict(pts_semantic_mask=[sem, sem], pts_instance_mask=[masks, sem], instance_labels=conv(scene["labels"]),
                instance_scores=conv(scene["scores"]))


@pytest.mark.parametrize("how", ["device", "host", "packed"])
def test_golden_tree(golden, tmp_path, how):
    from segdino3d_amd import submission
    from segdino3d_amd.architecture import PointData
    d = torch.device("cuda:0")
    preds = [_pred(s, how, d) for s in golden["scenes"]]
    # the writer, given PointData
    with submission.SubmissionWriter(str(tmp_path / "a" / "inst"), str(tmp_path / "a" / "sem"), golden["inst_mapping"],
                                     golden["sem_mapping"]) as w:
        for s, p in zip(golden["scenes"], preds):
            w.add(s["scan_id"], PointData(**p))
    assert read_tree(tmp_path / "a") == golden["files"]
    # a pool smaller than a scene
    with submission.SubmissionWriter(str(tmp_path / "b" / "inst"), str(tmp_path / "b" / "sem"), golden["inst_mapping"],
                                     golden["sem_mapping"], writers=2, max_pinned_bytes=16 << 10) as w:
        for s, p in zip(golden["scenes"], preds):
            w.add(s["scan_id"], p)
        assert w.pool.total <= 16 << 10
    assert read_tree(tmp_path / "b") == golden["files"]
    # the drop-ins
    os.makedirs(tmp_path / "c")
    results = [(dict(lidar_idx=s["scan_id"]), p) for s, p in zip(golden["scenes"], preds)]
    submission.format_results_instance(results, str(tmp_path / "c" / "inst"), golden["inst_mapping"])
    submission.format_results_semantic(results, str(tmp_path / "c" / "sem"), golden["sem_mapping"])
    assert read_tree(tmp_path / "c") == golden["files"]
    with pytest.raises(FileExistsError):
        submission.format_results_instance(results, str(tmp_path / "c" / "inst"), golden["inst_mapping"])
    submission.save_pred_instances(str(tmp_path / "d" / "inst"), [s["scan_id"] for s in golden["scenes"]],
                                   [(p["pts_instance_mask"][0], p["instance_labels"], p["instance_scores"]) for p in preds],
                                   golden["inst_mapping"])
    assert read_tree(tmp_path / "d") == {k: v for k, v in golden["files"].items() if k.startswith("inst/")}


def test_half_precision_scores_are_cast_on_the_device(golden, tmp_path):
    from segdino3d_amd import submission
    d = torch.device("cuda:0")
    s = golden["scenes"][0]
    p = _pred(s, "device", d)
    p["instance_scores"] = p["instance_scores"].to(torch.bfloat16)
    p["instance_labels"] = p["instance_labels"].to(torch.int32)
    with submission.SubmissionWriter(str(tmp_path / "inst"), None, golden["inst_mapping"], None) as w:
        w.add(s["scan_id"], p)
    want = "".join(f"predicted_masks/{s['scan_id']}_{k:03d}.txt {golden['inst_mapping'][lab]} {float(sc):.4f}\n"
                   for k, (lab, sc) in enumerate(zip(s["labels"], torch.from_numpy(s["scores"]).to(torch.bfloat16).float().numpy()))).encode()
    assert (tmp_path / "inst" / f"{s['scan_id']}.txt").read_bytes() == want


def test_a_bad_class_index_names_the_scene(golden, tmp_path):
    from segdino3d_amd import submission
    d = torch.device("cuda:0")
    p = _pred(golden["scenes"][0], "device", d)
    p["pts_semantic_mask"][0] = p["pts_semantic_mask"][0].clone()
    p["pts_semantic_mask"][0][17] = len(golden["sem_mapping"])
    w = submission.SubmissionWriter(None, str(tmp_path / "sem"), None, golden["sem_mapping"])
    w.add("scene0707_00", p)
    with pytest.raises(RuntimeError, match="scene0707_00.*outside the label table"):
        w.close()


# ------------------------------------------------------------------------------------------ end to end
def test_export_behind_the_pipelined_runner(tmp_path):
    import segdino3d_amd as seg
    from segdino3d_amd import submission
    from segdino3d_amd.configs import scannet200_model_cfg
    from segdino3d_amd.dist_eval import PipelinedRunner
    from segdino3d_amd.synth import make_scene, sharpen_random_model, structure_scene
    d = torch.device("cuda:0")
    pts, tgt = make_scene(1, n_points=8000, n_superpoints=64, n_query2d=8)                     # the scene of smoke()
    structure_scene(pts, tgt)
    cfg = scannet200_model_cfg(query_num=-1)
    cfg["test_cfg"]["npoint_thr"] = 20
    torch.manual_seed(0)
    model = sharpen_random_model(seg.build_architecture(cfg).eval()).to(d)
    model.to_host = False
    scenes = [(pts.to(d), copy.copy(tgt).to(d)) for _ in range(2)]
    ids = ["scene0001_00", "scene0002_00"]
    g = np.random.default_rng(0)
    inst_mapping = np.sort(g.choice(np.arange(1, 1192), size=model.num_classes, replace=False))
    sem_mapping = np.sort(g.choice(np.arange(1, 1192), size=model.num_classes + 2, replace=False))
    seen = {}
    with submission.SubmissionWriter(str(tmp_path / "inst"), str(tmp_path / "sem"), inst_mapping, sem_mapping) as w:
        write = w.on_result(ids)

        def on_result(i, result):
            p = result[0].pred_pts_seg
            seen[i] = (p.pts_instance_mask[0].cpu().numpy(), p.instance_labels.cpu().numpy(), p.instance_scores.cpu().numpy(),
                       p.pts_semantic_mask[0].cpu().numpy())
            write(i, result)

        out = PipelinedRunner(model, n_streams=2).run(scenes, on_result=on_result, keep=False)
    assert out == [None, None] and sorted(seen) == [0, 1]
    want = {}
    for i, sid in enumerate(ids):
        masks, labels, scores, sem = seen[i]
        assert masks.shape[0] >= 10 and masks.any() and masks.shape[1] == 8000
        want[f"sem/{sid}.txt"] = savetxt(sem_mapping[sem])
        want[f"inst/{sid}.txt"] = "".join(f"predicted_masks/{sid}_{k:03d}.txt {inst_mapping[lab]} {sc:.4f}\n"
                                          for k, (lab, sc) in enumerate(zip(labels, scores))).encode()
        for k, m in enumerate(masks):
            want[f"inst/predicted_masks/{sid}_{k:03d}.txt"] = savetxt(m)
    assert read_tree(tmp_path) == want
