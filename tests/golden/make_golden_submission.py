"""Generates tests/golden/submission.npz by running the REFERENCE's evaluator with both submission prefixes set
(/root/reference/evaluation/evaluator_3d.py: InstanceSeg3DEvaluator.compute_metrics :115-120 -> format_results_instance /
format_results_semantic / save_pred_instances :351-396) on two seeded synthetic scenes, and recording every file it writes
(relative path + bytes) next to the inputs.  Runs in the build container only; the third-party imports are stubbed by
make_golden_evaluator.py, which this script imports for its stubs and its loaded `evaluation.evaluator_3d` module."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_evaluator as mge  # noqa: E402 - installs the stubs, loads the reference module

ev = mge.ev
N, G = 1003, 13
SCAN_IDS = ("scene0707_00", "scene0708_00")
# ids of 1, 2, 3 and 4 digits, as in ScanNet200
SEM_MAPPING = (1, 2, 3, 5, 18, 42, 155, 370, 1164, 1191)
INST_MAPPING = SEM_MAPPING[mge.N_STUFF:]


def make_scene(seed):
    g = np.random.default_rng(seed)
    masks = g.random((G, N)) < g.random((G, 1))
    masks[3] = False                                           # an empty mask and a full one
    masks[7] = True
    labels = g.integers(0, len(INST_MAPPING), size=G).astype(np.int64)
    labels[:len(INST_MAPPING)] = g.permutation(len(INST_MAPPING))          # every id width occurs
    scores = np.round(g.random(G), 5).astype(np.float32)
    scores[0], scores[1], scores[2] = 0.99995, 0.12345, 1.0
    sem = g.integers(0, len(SEM_MAPPING), size=N).astype(np.int64)
    sem[:len(SEM_MAPPING)] = np.arange(len(SEM_MAPPING))
    return masks, labels, scores, sem


def main():
    scenes = [make_scene(707 + s) for s in range(len(SCAN_IDS))]
    e = object.__new__(ev.InstanceSeg3DEvaluator)
    e.debug = False
    e.dataset_meta = dict(seg_valid_class_ids=list(mge.VALID_IDS))
    e.metric_meta = dict(label2cat={i: c for i, c in enumerate(mge.CLASSES)}, ignore_index=[len(mge.CLASSES) - 1], classes=list(mge.CLASSES),
                         dataset_name="ScanNet")
    e.thing_class_inds = list(range(mge.N_STUFF, len(mge.CLASSES) - 1))
    e.stuff_class_inds = list(range(mge.N_STUFF))
    e.inst_mapping = np.array(INST_MAPPING)
    e.sem_mapping = np.array(SEM_MAPPING)
    out = {"scan_ids": np.array(SCAN_IDS), "inst_mapping": np.array(INST_MAPPING), "sem_mapping": np.array(SEM_MAPPING), "n": np.array(N)}
    with tempfile.TemporaryDirectory() as tmp:
        e.submission_prefix_instance = os.path.join(tmp, "inst")
        e.submission_prefix_semantic = os.path.join(tmp, "sem")
        results = []
        for sid, (masks, labels, scores, sem) in zip(SCAN_IDS, scenes):
            ann = dict(lidar_idx=sid)
            pred = dict(pts_semantic_mask=[sem, np.zeros_like(sem)], pts_instance_mask=[masks, np.zeros_like(sem)],
                        instance_labels=labels, instance_scores=scores)
            results.append((ann, pred))
        assert e.compute_metrics(results) == {}
        paths, blobs = [], []
        for root, _, files in sorted(os.walk(tmp)):
            for fn in sorted(files):
                full = os.path.join(root, fn)
                paths.append(os.path.relpath(full, tmp).replace(os.sep, "/"))
                with open(full, "rb") as f:
                    blobs.append(np.frombuffer(f.read(), dtype=np.uint8))
    out["paths"] = np.array(paths)
    out["file_off"] = np.cumsum([0] + [len(b) for b in blobs]).astype(np.int64)
    out["file_bytes"] = np.concatenate(blobs)
    for si, (masks, labels, scores, sem) in enumerate(scenes):
        out[f"s{si}_masks"] = np.packbits(masks, axis=1, bitorder="little")
        out[f"s{si}_labels"], out[f"s{si}_scores"], out[f"s{si}_sem"] = labels, scores, sem
    path = os.path.join(HERE, "submission.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(paths), "files")


if __name__ == "__main__":
    main()
