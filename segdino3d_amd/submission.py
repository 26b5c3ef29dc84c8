"""ScanNet benchmark submission export: the text files of the reference evaluator's submission exit
(evaluation/evaluator_3d.py:115-120, 351-396), formatted on the device.

The reference writes one `np.savetxt(path, mask, fmt='%d')` per instance mask (0.29 s for 150 k points) behind an `mp.Pool()`.
Here the per-point text is made by two kernels (`ops.mask_text`, `ops.label_text`), copied into pinned buffers of a bounded pool and
handed to a few writer threads whose only work is `write()`; the index file's one line per instance is formatted by Python.

    with SubmissionWriter(instance_root=..., semantic_root=..., inst_mapping=..., sem_mapping=...) as w:
        PipelinedRunner(model, n_streams=2).run(scenes, on_result=w.on_result(scan_ids), keep=False)      # model.to_host = False

`format_results_instance`, `format_results_semantic` and `save_pred_instances` keep the reference's call shapes and directory rules.
"""
from __future__ import annotations

import os
import queue
import threading

import numpy as np

__all__ = ["index_text", "SubmissionWriter", "DeviceFormatter", "format_results_instance", "format_results_semantic", "save_pred_instances"]


def index_text(scan_id, labels, scores, mapping) -> bytes:
    """The per-scene index file (save_single_instance, :383): `predicted_masks/{scan_id}_{i:03d}.txt {mapping[label]} {score:.4f}`
    per instance, the score formatted as the reference's f-string formats an np.float32 (through its exact double value)."""
    mapping = np.asarray(mapping)
    labels = np.asarray(labels).astype(np.int64).ravel()
    scores = np.asarray(scores).astype(np.float32).ravel()
    lines = [f"predicted_masks/{scan_id}_{i:03d}.txt {int(mapping[int(lab)])} {float(sc):.4f}\n" for i, (lab, sc) in enumerate(zip(labels, scores))]
    return "".join(lines).encode()


class DeviceFormatter:
    """What `SubmissionWriter` needs from the device, on the caller's current stream.  Tests drive the writer's threading, chunking and
    path logic through a host stand-in with these methods."""

    def __init__(self, device=None):
        import torch
        from . import ops
        self.torch, self.ops = torch, ops
        self.device = device
        self._tables = {}

    def _dev(self):
        return self.device if self.device is not None else self.torch.device("cuda", self.torch.cuda.current_device())

    def _upload(self, x):
        torch = self.torch
        if isinstance(x, torch.Tensor):
            return x if x.is_cuda else x.to(self._dev())
        return torch.from_numpy(np.ascontiguousarray(np.asarray(x))).to(self._dev())

    def masks(self, x):
        """[n, N] instance masks (device / host tensor, array, PackedMasks) -> uint8 [n, N] on the device."""
        t = self._upload(x)
        if t.dtype == self.torch.bool:
            t = t.view(self.torch.uint8)
        elif t.dtype != self.torch.uint8:
            t = (t != 0).view(self.torch.uint8)
        return t.contiguous()

    def values(self, x):
        """[N] class indices -> int64 on the device."""
        return self._upload(x).reshape(-1).long().contiguous()

    def small(self, x, dtype):
        """labels ("int64") / scores ("float32") of the index file: device tensors travel with the text, cast to `dtype` on the device
        (whatever precision the model scored in); host arrays stay where they are."""
        if isinstance(x, self.torch.Tensor):
            if x.is_cuda:
                return x.reshape(-1).to(getattr(self.torch, dtype)).contiguous()
            return x.float().numpy() if x.is_floating_point() else x.numpy()
        return np.asarray(x)

    def mask_text(self, masks, r0, r1):
        return self.ops.mask_text(masks[r0:r1])

    def label_text(self, values, mapping):
        key = (id(mapping), str(values.device))
        table = self._tables.get(key)
        if table is None:                                      # one upload per table and device
            table = self._tables[key] = (mapping, self.ops.LabelTable(mapping, values.device))
        return self.ops.label_text(values, table[1])

    def pinned(self, nbytes):
        return self.torch.empty(int(nbytes), dtype=self.torch.uint8, pin_memory=True)

    def copy(self, buf, off, src):
        """Asynchronous copy of `src` (device tensor) to buf[off : off + bytes]."""
        nb = src.numel() * src.element_size()
        if nb:
            buf[off:off + nb].view(src.dtype).view(src.shape).copy_(src, non_blocking=True)

    def event(self):
        return self.ops.stream_event()

    def wait(self, ev):
        self.ops.wait_event(ev)                                  # polled: a writer thread never sits inside a blocking HIP call

    def view(self, buf):
        return buf.numpy()

    def is_device(self, x):
        return isinstance(x, self.torch.Tensor) and x.is_cuda


class _PinnedPool:
    """At most `count` pinned buffers of ONE size, allocated when first needed and recycled for the writer's life: nothing is ever given
    back to (and kept pinned by) the host allocator, so count x size bounds the pinned memory this writer causes.  `acquire` waits for
    a release when all are in use, with the caller's issue baton handed on meanwhile."""

    def __init__(self, count, size, alloc):
        self.count, self.size, self.alloc = int(count), int(size), alloc
        self.free, self.made = [], 0
        self.cv = threading.Condition()

    @property
    def total(self):
        """Pinned bytes allocated so far."""
        return self.made * self.size

    def _try(self):
        """(buffer | None, allocate?): called with the lock held."""
        if self.free:
            return self.free.pop(), False
        if self.made < self.count:
            self.made += 1
            return None, True
        return None, False

    def acquire(self):
        from . import ops
        with self.cv:
            b, grow = self._try()
        if b is None and not grow:
            with ops.baton_released():                           # (the pool lock is taken and left inside the scope)
                with self.cv:
                    while True:
                        b, grow = self._try()
                        if b is not None or grow:
                            break
                        self.cv.wait()
        if b is None:
            try:
                b = self.alloc(self.size)
            except BaseException:
                with self.cv:
                    self.made -= 1
                    self.cv.notify_all()
                raise
        return b

    def release(self, b):
        with self.cv:
            self.free.append(b)
            self.cv.notify_all()


class _Job:
    __slots__ = ("scan_id", "event", "buf", "index", "sem", "rows")

    def __init__(self, scan_id):
        self.scan_id, self.event, self.buf = scan_id, None, None
        self.index = None        # (labels, scores): arrays, or (offset, dtype, count) into the buffer
        self.sem = None          # (text offset, cap, info offset)
        self.rows = None         # (offset, first row, n rows, pitch, 2 N)


def _field(pred, key):
    return pred[key] if isinstance(pred, dict) else getattr(pred, key)


def _nbytes(x):
    return int(x.numel() * x.element_size()) if hasattr(x, "element_size") else int(x.nbytes)


def _align(x, a=64):
    return (x + a - 1) // a * a


class SubmissionWriter:
    """Writes the submission tree of the scenes given to `add`:

        instance_root/{scan_id}.txt                           index_text
        instance_root/predicted_masks/{scan_id}_{i:03d}.txt   one "0\\n" / "1\\n" line per point
        semantic_root/{scan_id}.txt                           sem_mapping[class] per point

    A root that is None switches that part off.  `writers` threads call write(); the text is staged in max(2, writers)
    pinned buffers of one power-of-two size, together at most `max_pinned_bytes`, allocated once and recycled; a scene whose text is
    larger than a buffer goes through them in chunks of mask rows.  An error status of a kernel or an exception in a
    writer thread is raised from the next `add` or from `close()`, naming the scene."""

    def __init__(self, instance_root=None, semantic_root=None, inst_mapping=None, sem_mapping=None, writers=4, max_pinned_bytes=256 << 20,
                 formatter=None):
        if instance_root is not None and inst_mapping is None:
            raise ValueError("SubmissionWriter: instance_root needs inst_mapping")
        if semantic_root is not None and sem_mapping is None:
            raise ValueError("SubmissionWriter: semantic_root needs sem_mapping")
        self.instance_root, self.semantic_root = instance_root, semantic_root
        self.inst_mapping = None if inst_mapping is None else np.asarray(inst_mapping)
        self.sem_mapping = None if sem_mapping is None else np.asarray(sem_mapping)
        self.fmt = formatter if formatter is not None else DeviceFormatter()
        self.max_pinned_bytes = int(max_pinned_bytes)
        # one buffer per writer thread (two at least: one being copied into while one is being written), all of one size: the largest
        # power of two that fits, because the pinned host allocator rounds a request up to one
        n_buf = max(2, int(writers))
        self.chunk_bytes = 1 << max(0, (self.max_pinned_bytes // n_buf).bit_length() - 1) if self.max_pinned_bytes >= n_buf else 0
        self.pool = _PinnedPool(n_buf, max(self.chunk_bytes, 1), self.fmt.pinned)
        if instance_root is not None:
            os.makedirs(instance_root, exist_ok=True)
            os.makedirs(os.path.join(instance_root, "predicted_masks"), exist_ok=True)
        if semantic_root is not None:
            os.makedirs(semantic_root, exist_ok=True)
        self.jobs = queue.Queue()
        self.errors = []
        self.closed = False
        self.threads = [threading.Thread(target=self._writer, name=f"sd3d-submit-{k}", daemon=True) for k in range(max(1, int(writers)))]
        for t in self.threads:
            t.start()

    # ------------------------------------------------------------------ caller side
    def add(self, scan_id, pred):
        """One scene's post-processed output (a model output or its `pred_pts_seg`: `PointData` / dict; device tensors with `model.to_host = False`, host arrays and
        `PackedMasks` are uploaded).  Formats on the current stream, stages the text and returns without waiting for the GPU."""
        pred = getattr(pred, "pred_pts_seg", pred)
        self._add(scan_id,
                  masks=_field(pred, "pts_instance_mask")[0] if self.instance_root is not None else None,
                  labels=_field(pred, "instance_labels") if self.instance_root is not None else None,
                  scores=_field(pred, "instance_scores") if self.instance_root is not None else None,
                  sem=_field(pred, "pts_semantic_mask")[0] if self.semantic_root is not None else None)

    def _add(self, scan_id, masks=None, labels=None, scores=None, sem=None):
        if self.closed:
            raise RuntimeError("SubmissionWriter: add() after close()")
        self._raise_errors()
        fmt = self.fmt
        sem_text = sem_info = None
        head = 0                                                 # bytes of the first job in front of its mask rows
        if sem is not None:
            sem_text, sem_info = fmt.label_text(fmt.values(sem), self.sem_mapping)
            head = _align(_nbytes(sem_text)) + 64
        n = N = pitch = 0
        small = []
        if masks is not None:
            masks = fmt.masks(masks)
            n, N = int(masks.shape[0]), int(masks.shape[1])
            pitch = (2 * N + 15) // 16 * 16
            labels, scores = fmt.small(labels, "int64"), fmt.small(scores, "float32")
            if len(labels) != n or len(scores) != n:
                raise ValueError(f"submission: scene {scan_id}: {n} masks, {len(labels)} labels, {len(scores)} scores")
            small = [x for x in (labels, scores) if fmt.is_device(x)]
            head += sum(_align(8 * n) for _ in small)
        if head > self.chunk_bytes or pitch > self.chunk_bytes:
            raise ValueError(f"submission: scene {scan_id}: max_pinned_bytes = {self.max_pinned_bytes} gives staging buffers of "
                             f"{self.chunk_bytes} bytes; {max(head, pitch)} are needed (a mask row, or the semantic text)")
        r0, first = 0, True
        while first or r0 < n:
            rows = 0
            if pitch:
                rows = min(n - r0, (self.chunk_bytes - (head if first else 0)) // pitch)
            if not first and rows == 0:
                break
            job = _Job(scan_id)
            job.buf = self.pool.acquire()                        # (head + rows x pitch <= chunk_bytes)
            try:
                off = 0
                if first:
                    if sem_text is not None:
                        cap = _nbytes(sem_text)
                        fmt.copy(job.buf, 0, sem_text)
                        fmt.copy(job.buf, _align(cap), sem_info)
                        job.sem = (0, cap, _align(cap))
                        off = _align(cap) + 64
                    if masks is not None:
                        parts = []
                        for x, dtype in ((labels, "int64"), (scores, "float32")):
                            if fmt.is_device(x):
                                fmt.copy(job.buf, off, x)
                                parts.append((off, dtype, n))
                                off += _align(8 * n)
                            else:
                                parts.append(x)
                        job.index = tuple(parts)
                if rows:
                    text = fmt.mask_text(masks, r0, r0 + rows)
                    fmt.copy(job.buf, off, text)
                    job.rows = (off, r0, rows, pitch, 2 * N)
                job.event = fmt.event()
            except BaseException:
                self.pool.release(job.buf)
                raise
            self.jobs.put(job)
            r0 += rows
            first = False

    def on_result(self, scan_ids):
        """The callback of `PipelinedRunner.run(scenes, on_result=..., keep=False)`: scene i is written as `scan_ids[i]`."""
        def callback(i, result):
            pred = result
            while isinstance(pred, (list, tuple)):
                pred = pred[0]
            self.add(scan_ids[i], pred)                          # (a model output: add() reads its `pred_pts_seg`)
        return callback

    def _raise_errors(self):
        if self.errors:
            scan_id, exc = self.errors[0]
            raise RuntimeError(f"submission: scene {scan_id}: {type(exc).__name__}: {exc}") from exc

    def flush(self):
        """Waits until every scene added so far is written; raises the first error of a writer thread."""
        from . import ops
        with ops.baton_released():
            self.jobs.join()
        self._raise_errors()

    def close(self):
        """Waits until every file is written; raises the first error of a writer thread."""
        if not self.closed:
            self.closed = True
            for _ in self.threads:
                self.jobs.put(None)
            for t in self.threads:
                t.join()
        self._raise_errors()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is not None:                                 # do not hide the caller's exception behind ours
            try:
                self.close()
            except Exception:  # noqa: BLE001
                pass
            return False
        self.close()
        return False

    # ------------------------------------------------------------------ writer threads
    def _writer(self):
        while True:
            job = self.jobs.get()
            if job is None:
                self.jobs.task_done()
                return
            try:
                if not self.errors:
                    self._write(job)
            except BaseException as e:  # noqa: BLE001 - raised from add() / close()
                self.errors.append((job.scan_id, e))
            finally:
                try:
                    self.fmt.wait(job.event)                     # the buffer is free only once its copies have landed
                except BaseException as e:  # noqa: BLE001
                    self.errors.append((job.scan_id, e))
                self.pool.release(job.buf)
                self.jobs.task_done()

    def _write(self, job):
        self.fmt.wait(job.event)
        host = self.fmt.view(job.buf)
        sid = job.scan_id
        if job.sem is not None:
            off, cap, info_off = job.sem
            info = host[info_off:info_off + 8].view(np.int32)
            from .ops import label_text_check
            length = label_text_check(info, "semantic label text")
            if length > cap:
                raise RuntimeError(f"semantic label text of {length} bytes in a buffer of {cap}")
            with open(os.path.join(self.semantic_root, f"{sid}.txt"), "wb") as f:
                f.write(host[off:off + length].data)
        if job.index is not None:
            arrs = []
            for part in job.index:
                if isinstance(part, tuple):
                    o, dtype, count = part
                    dt = np.dtype(dtype)
                    part = host[o:o + dt.itemsize * count].view(dt)
                arrs.append(part)
            with open(os.path.join(self.instance_root, f"{sid}.txt"), "wb") as f:
                f.write(index_text(sid, arrs[0], arrs[1], self.inst_mapping))
        if job.rows is not None:
            off, r0, rows, pitch, nbytes = job.rows
            table = host[off:off + rows * pitch].reshape(rows, pitch)
            root = os.path.join(self.instance_root, "predicted_masks")
            for k in range(rows):
                with open(os.path.join(root, f"{sid}_{r0 + k:03d}.txt"), "wb") as f:
                    f.write(table[k, :nbytes].data)


# ---------------------------------------------------------------------- the reference's call shapes
def save_pred_instances(root, scan_ids, pred_insts, mapping, **writer_args):
    """save_pred_instances (:389-396): pred_insts[i] = (masks [n, N], labels [n], scores [n]) of scan_ids[i]; device tensors, host
    arrays or `PackedMasks`.  Threads instead of the reference's process pool."""
    os.makedirs(root, exist_ok=True)
    with SubmissionWriter(instance_root=root, inst_mapping=mapping, **writer_args) as w:
        for sid, (masks, labels, scores) in zip(scan_ids, pred_insts):
            w._add(sid, masks=masks, labels=labels, scores=scores)


def format_results_instance(results, submission_prefix, inst_mapping, **writer_args):
    """InstanceSeg3DEvaluator.format_results_instance (:363-376) over `results` = [(eval_ann, single_pred_results)]: fails when the
    prefix exists, as the reference's `os.makedirs` does."""
    os.makedirs(submission_prefix)
    scan_ids, preds = [], []
    for eval_ann, pred in results:
        scan_ids.append(eval_ann["lidar_idx"])
        preds.append((_field(pred, "pts_instance_mask")[0], _field(pred, "instance_labels"), _field(pred, "instance_scores")))
    save_pred_instances(submission_prefix, scan_ids, preds, inst_mapping, **writer_args)


def format_results_semantic(results, submission_prefix, sem_mapping, **writer_args):
    """InstanceSeg3DEvaluator.format_results_semantic (:351-361): `{prefix}/{scan_id}.txt` = sem_mapping[pts_semantic_mask[0]]."""
    os.makedirs(submission_prefix)
    with SubmissionWriter(semantic_root=submission_prefix, sem_mapping=sem_mapping, **writer_args) as w:
        for eval_ann, pred in results:
            w._add(eval_ann["lidar_idx"], sem=_field(pred, "pts_semantic_mask")[0])
