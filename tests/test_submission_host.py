"""Benchmark submission export, host side (no GPU): the index file, the directory rules, and `SubmissionWriter`'s threading, chunking
and path logic driven through a numpy stand-in for the device formatter, against the tree the reference's own evaluator wrote
(tests/golden/submission.npz, made by tests/golden/make_golden_submission.py)."""
import os

import numpy as np
import pytest
import torch

from segdino3d_amd import ops, submission

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "submission.npz")


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    files = {str(p): bytes(g["file_bytes"][g["file_off"][i]:g["file_off"][i + 1]]) for i, p in enumerate(g["paths"])}
    n = int(g["n"])
    scenes = []
    for si, sid in enumerate(g["scan_ids"]):
        masks = np.unpackbits(g[f"s{si}_masks"], axis=1, bitorder="little")[:, :n].astype(bool)
        scenes.append(dict(scan_id=str(sid), masks=masks, labels=g[f"s{si}_labels"], scores=g[f"s{si}_scores"], sem=g[f"s{si}_sem"]))
    return dict(files=files, scenes=scenes, inst_mapping=g["inst_mapping"], sem_mapping=g["sem_mapping"], n=n)


def read_tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for fn in files:
            full = os.path.join(d, fn)
            with open(full, "rb") as f:
                out[os.path.relpath(full, root).replace(os.sep, "/")] = f.read()
    return out


def pred_of(scene):
    return dict(pts_semantic_mask=[scene["sem"], np.zeros_like(scene["sem"])], pts_instance_mask=[scene["masks"], np.zeros_like(scene["sem"])],
                instance_labels=scene["labels"], instance_scores=scene["scores"])


class _Dev:
    """A "device" array of the stand-in: only `copy` may look inside."""

    def __init__(self, a):
        self.a, self.dtype = a, a.dtype

    def __len__(self):
        return len(self.a)


class NumpyFormatter:
    """Host stand-in for submission.DeviceFormatter: numpy restatements of the two kernels (padding bytes poisoned), plain arrays as
    pinned buffers, and a record of what was allocated."""

    def __init__(self):
        self.allocated, self.peak, self.allocs, self.copies = 0, 0, 0, 0

    def masks(self, x):
        return np.ascontiguousarray(np.asarray(x) != 0).astype(np.uint8)

    def values(self, x):
        return np.asarray(x).astype(np.int64).ravel()

    def small(self, x, dtype):
        return _Dev(np.ascontiguousarray(np.asarray(x)).astype(dtype))

    def is_device(self, x):
        return isinstance(x, _Dev)

    def mask_text(self, masks, r0, r1):
        n_pts = masks.shape[1]
        out = np.full((r1 - r0, (2 * n_pts + 15) // 16 * 16), 0xEE, dtype=np.uint8)
        out[:, 0:2 * n_pts:2] = ord("0") + masks[r0:r1]
        out[:, 1:2 * n_pts:2] = ord("\n")
        return out

    def label_text(self, values, mapping):
        mapping = np.asarray(mapping)
        text = "".join(f"{int(mapping[v])}\n" for v in values).encode()
        out = np.full(len(values) * (max(len(str(int(m))) for m in mapping) + 1), 0xEE, dtype=np.uint8)
        out[:len(text)] = np.frombuffer(text, dtype=np.uint8)
        return out, np.array([len(text), 0], dtype=np.int32)

    def pinned(self, nbytes):
        self.allocs += 1
        return np.full(int(nbytes), 0xDD, dtype=np.uint8)

    def copy(self, buf, off, src):
        b = np.ascontiguousarray(src.a if isinstance(src, _Dev) else src).view(np.uint8).ravel()
        assert off + b.size <= buf.size
        buf[off:off + b.size] = b
        self.copies += 1

    def event(self):
        return None

    def wait(self, ev):
        pass

    def view(self, buf):
        return buf


def test_index_text_equals_the_reference(golden):
    for s in golden["scenes"]:
        want = golden["files"][f"inst/{s['scan_id']}.txt"]
        assert submission.index_text(s["scan_id"], s["labels"], s["scores"], golden["inst_mapping"]) == want
        assert submission.index_text(s["scan_id"], torch.from_numpy(s["labels"]), torch.from_numpy(s["scores"]), list(golden["inst_mapping"])) == want
    assert b" 0.9999\n" in golden["files"]["inst/scene0707_00.txt"] and b" 0.1235\n" in golden["files"]["inst/scene0707_00.txt"]
    assert submission.index_text("s", [], [], golden["inst_mapping"]) == b""


def test_writer_reproduces_the_golden_tree(golden, tmp_path):
    fmt = NumpyFormatter()
    with submission.SubmissionWriter(str(tmp_path / "inst"), str(tmp_path / "sem"), golden["inst_mapping"], golden["sem_mapping"],
                                     formatter=fmt) as w:
        for s in golden["scenes"]:
            w.add(s["scan_id"], pred_of(s))
    assert read_tree(tmp_path) == golden["files"]
    assert fmt.allocs <= 2                                       # one staged batch per scene, buffers recycled


def test_pool_smaller_than_a_scene(golden, tmp_path):
    """A scene is 13 rows of 2 x 1003 bytes plus 5 KB of semantic text, 31 KB: a bound of 16 KB gives two buffers of 8 KB, four rows each."""
    fmt = NumpyFormatter()
    bound = 16 << 10
    w = submission.SubmissionWriter(str(tmp_path / "inst"), str(tmp_path / "sem"), golden["inst_mapping"], golden["sem_mapping"], writers=2,
                                    max_pinned_bytes=bound, formatter=fmt)
    with w:
        for s in golden["scenes"]:
            w.add(s["scan_id"], pred_of(s))
        assert w.pool.total <= bound
    assert read_tree(tmp_path) == golden["files"]
    assert w.pool.total <= bound and fmt.allocs == 2 and fmt.copies > 2 * 4      # recycled buffers, several chunks per scene
    with pytest.raises(ValueError, match="max_pinned_bytes"):
        with submission.SubmissionWriter(str(tmp_path / "inst2"), None, golden["inst_mapping"], None, max_pinned_bytes=2000, formatter=fmt) as w2:
            w2.add("scene0707_00", pred_of(golden["scenes"][0]))


def test_drop_ins_follow_the_reference_directory_rules(golden, tmp_path):
    results = [(dict(lidar_idx=s["scan_id"]), pred_of(s)) for s in golden["scenes"]]
    inst, sem = str(tmp_path / "inst"), str(tmp_path / "sem")
    submission.format_results_instance(results, inst, golden["inst_mapping"], formatter=NumpyFormatter())
    submission.format_results_semantic(results, sem, golden["sem_mapping"], formatter=NumpyFormatter())
    assert read_tree(tmp_path) == golden["files"]
    with pytest.raises(FileExistsError):                         # os.makedirs(prefix) of the reference
        submission.format_results_instance(results, inst, golden["inst_mapping"], formatter=NumpyFormatter())
    with pytest.raises(FileExistsError):
        submission.format_results_semantic(results, sem, golden["sem_mapping"], formatter=NumpyFormatter())
    # save_pred_instances: exist_ok, and it overwrites
    submission.save_pred_instances(inst, [s["scan_id"] for s in golden["scenes"]],
                                   [(s["masks"], s["labels"], s["scores"]) for s in golden["scenes"]], golden["inst_mapping"],
                                   formatter=NumpyFormatter())
    assert read_tree(tmp_path) == golden["files"]


def test_writer_thread_error_surfaces_in_close(golden, tmp_path):
    class Broken(NumpyFormatter):
        def wait(self, ev):
            raise OSError("disk on fire")

    w = submission.SubmissionWriter(str(tmp_path / "inst"), None, golden["inst_mapping"], None, formatter=Broken())
    w.add("scene0707_00", pred_of(golden["scenes"][0]))
    with pytest.raises(RuntimeError, match="scene0707_00.*disk on fire"):
        w.close()

    class BadStatus(NumpyFormatter):
        def label_text(self, values, mapping):
            text, info = super().label_text(values, mapping)
            info[1] = 1
            return text, info

    w = submission.SubmissionWriter(None, str(tmp_path / "sem"), None, golden["sem_mapping"], formatter=BadStatus())
    w.add("scene0708_00", pred_of(golden["scenes"][1]))
    with pytest.raises(RuntimeError, match="scene0708_00.*outside the label table"):
        w.close()
    assert not os.path.exists(tmp_path / "sem" / "scene0708_00.txt")
    with pytest.raises(RuntimeError, match="after close"):
        w.add("scene0707_00", pred_of(golden["scenes"][0]))


def test_ops_refuse_cpu_tensors():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mask_text(torch.zeros(2, 10, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.label_text(torch.zeros(10, dtype=torch.int64))
