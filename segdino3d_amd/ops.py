"""Python operator layer over the C ABI: torch tensors in, torch tensors out.

torch is used here for device memory (caching allocator) and the current HIP stream only; all
arithmetic happens in libsegdino3d_hip.so.  Every op raises if a tensor is not on a HIP device -
there is deliberately no CPU path (the CPU restatement is oracle/, test infrastructure).
"""
from __future__ import annotations

import ctypes
import threading
from collections import OrderedDict as _collections_od
from typing import Optional

import numpy as np
import torch

from . import _lib

ACT = {None: 0, "none": 0, "relu": 1, "gelu": 2, "sigmoid": 3}

# Optional instrumentation for bench.py: an object with before(meta: dict) / after() called around
# every gather_gemm launch on the current stream (meta: K, Cin, Cout, M, nbr tensor or None).
GG_HOOK = None
import os as _os


_STREAM_TLS = threading.local()


def _stream():
    s = getattr(_STREAM_TLS, "handle", None)
    return s if s is not None else torch.cuda.current_stream().cuda_stream


class stream_scope:
    """Binds this thread's current HIP stream handle for the duration of a forward.

    torch.cuda.current_stream() costs ~8 us per lookup on the host - more than the launch it precedes,
    and a forward makes ~360 of them.  Inside the scope every op enqueues on the stream that was current
    when the outermost scope was entered; do not switch torch streams inside it."""

    def __enter__(self):
        self.prev = getattr(_STREAM_TLS, "handle", None)
        if self.prev is None:
            _STREAM_TLS.handle = torch.cuda.current_stream().cuda_stream
        return self

    def __exit__(self, *exc):
        _STREAM_TLS.handle = self.prev
        return False


class use_stream:
    """Issue on `stream` (a torch.cuda.Stream) inside the scope: torch's current stream AND the bound handle of this thread's
    ops move together.  The caller orders the streams (`stream.wait_stream(...)` before, `....wait_stream(stream)` after)."""

    def __init__(self, stream):
        self.stream = stream
        self.ctx = torch.cuda.stream(stream)

    def __enter__(self):
        self.prev = getattr(_STREAM_TLS, "handle", None)
        self.ctx.__enter__()
        _STREAM_TLS.handle = self.stream.cuda_stream
        return self

    def __exit__(self, *exc):
        _STREAM_TLS.handle = self.prev
        return self.ctx.__exit__(*exc)


def bound_stream(fn):
    """Decorator form of stream_scope for the public forward entry points."""
    import functools

    @functools.wraps(fn)
    def wrapped(*a, **kw):
        with stream_scope():
            return fn(*a, **kw)
    return wrapped


def _ptr(t: Optional[torch.Tensor], dtype=None, name="tensor"):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor on the HIP device, got {t.device} (no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t.data_ptr()


def _rows(t: torch.Tensor, name="tensor"):
    """2-D fp32 tensor whose rows may be strided (last dim contiguous) -> (ptr, ld)."""
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor on the HIP device, got {t.device} (no CPU fallback)")
    if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: expected a 2-D fp32 tensor with contiguous rows")
    return t.data_ptr(), t.stride(0)


def _want_shape(t, shapes, name):
    """ValueError unless t's shape is one of `shapes` (a -1 entry takes any extent >= 1): the kernels index by these shapes unchecked."""
    got = tuple(t.shape)
    for want in shapes:
        if len(got) == len(want) and all(g == w or (w == -1 and g >= 1) for g, w in zip(got, want)):
            return
    raise ValueError(f"{name}: expected shape {' or '.join(str(list(w)).replace('-1', 'n_scenes') for w in shapes)}, got {list(got)}")


def _want_ranges(rng, row_scene, n, name):
    """rng [6] for one scene's rows; [n_scenes, 6] and row_scene [n] for the rows of several."""
    if row_scene is None:
        _want_shape(rng, [(6,)], f"{name}: rng (one scene)")
    else:
        _want_shape(rng, [(-1, 6)], f"{name}: rng (with row_scene)")
        _want_shape(row_scene, [(n,)], f"{name}: row_scene")


def _want_box_shapes(ref_points, d_center, size_prev, d_size, rng, row_scene=None):
    """The shapes `box_refine` indexes by -> Q."""
    Q = ref_points.shape[0]
    _want_shape(ref_points, [(Q, 3)], "box_refine: ref_points")
    _want_shape(d_center, [(Q, 3)], "box_refine: d_center")
    if d_size is not None:
        _want_shape(d_size, [(Q, 3)], "box_refine: d_size")
        if size_prev is None:
            raise ValueError("box_refine: d_size given without size_prev")
    if size_prev is not None:
        _want_shape(size_prev, [(3,), (Q, 3)], "box_refine: size_prev")
    _want_ranges(rng, row_scene, Q, "box_refine")
    return Q


class HostRead:
    """Small device -> host read: asynchronous copy into pinned memory + an event the caller waits on through
    `wait_event` (which hands the issue baton of the pipelined runner to another scene's thread meanwhile)."""

    __slots__ = ("buf", "event")

    def __init__(self, dev_tensor: torch.Tensor):
        self.buf = torch.empty(dev_tensor.shape, dtype=dev_tensor.dtype, pin_memory=True)
        self.buf.copy_(dev_tensor, non_blocking=True)
        self.event = stream_event()

    def wait(self):
        wait_event(self.event)
        return self.buf


_BATON_TLS = threading.local()


def set_baton(lock):
    """Install (or clear, with None) this thread's issue baton: the pipelined runner lets only the baton
    holder run Python; a thread hands the baton over exactly while it waits for the GPU (wait_event)."""
    _BATON_TLS.lock = lock


import collections as _collections
_BATON_WAITERS = _collections.deque()                          # append / pop are atomic: threads that want the baton back


def baton_yield():
    """Called between the big issue blocks of a forward (decoder layers, post-processing): if another scene's
    thread has finished waiting for the GPU and wants to issue its next (short) phase, let it go first - its
    stream is empty, ours still has milliseconds of queued work."""
    baton = getattr(_BATON_TLS, "lock", None)
    if baton is not None and _BATON_WAITERS:
        import time
        baton.release()
        time.sleep(0)
        _BATON_WAITERS.append(1)
        baton.acquire()
        _BATON_WAITERS.pop()


def wait_event(ev):
    """Wait for `ev` without keeping other scene threads from issuing."""
    import time
    baton = getattr(_BATON_TLS, "lock", None)
    if baton is not None:
        baton.release()
        try:
            ev.synchronize()                                   # blocks inside HIP with the GIL released
        finally:
            _BATON_WAITERS.append(1)
            baton.acquire()
            _BATON_WAITERS.pop()
        return
    spins = 0
    while not ev.query():
        spins += 1
        time.sleep(0 if spins < 200 else 5e-5)


class baton_released:
    """A host wait that is no GPU wait (a free staging buffer, a queue): this thread's issue baton goes to the other scene threads
    for the duration of the scope, as in `wait_event`.  Take no lock inside that a baton holder may want while it is held on exit."""

    def __enter__(self):
        self.baton = getattr(_BATON_TLS, "lock", None)
        if self.baton is not None:
            self.baton.release()
        return self

    def __exit__(self, *exc):
        if self.baton is not None:
            _BATON_WAITERS.append(1)
            self.baton.acquire()
            _BATON_WAITERS.pop()
        return False


def stream_event():
    # hipEventBlockingSync: a thread waiting for its scene sleeps instead of spinning on a core (8 ranks x 4 scene threads
    # share one host in the multi-GPU runs)
    ev = torch.cuda.Event(blocking=True)
    ev.record()
    return ev


class Workspace:
    """Grow-only scratch buffer (bytes) per device."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes: int, device):
        nbytes = max(int(nbytes), 256)
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != torch.device(device):
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self.buf


class _PerThread:
    """One scratch buffer per (host thread, HIP stream): each worker thread of the pipelined runner drives its own stream, a
    thread may move to another stream (`use_stream`), and scratch must never be shared between streams."""

    def __init__(self):
        self._tls = threading.local()

    def get(self, nbytes: int, device):
        by_stream = getattr(self._tls, "ws", None)
        if by_stream is None:
            by_stream = self._tls.ws = {}
        key = _stream()
        ws = by_stream.get(key)
        if ws is None:
            ws = by_stream[key] = Workspace()
        return ws.get(nbytes, device)


_WS = _PerThread()
_WS2 = _PerThread()       # split-K partial sums of gather_gemm
_WS3 = _PerThread()       # partial products of pair_conv
_WS4 = _PerThread()       # pair_lists scratch
_WS6 = _PerThread()       # attention key-split partial states


# --------------------------------------------------------------------------------------------
# sort / scan
# --------------------------------------------------------------------------------------------
def sort_pairs(keys: torch.Tensor, vals: Optional[torch.Tensor] = None, begin_bit=0, end_bit=64):
    """Stable ascending sort of uint64-as-int64 keys; returns (sorted_keys, sorted_vals[int32]).
    `keys` (int64 storage of u64 bit patterns) and `vals` are clobbered.  No padding pass: after an even number of 8-bit radix passes
    the result sits in the input / scratch buffers and those are what is returned (`sd3d_sort_pairs_u64_ex`)."""
    lib = _lib.load()
    n = keys.numel()
    dev = keys.device
    keys_out = torch.empty_like(keys)
    vals_out = torch.empty(n, dtype=torch.int32, device=dev)
    scratch = torch.empty(n, dtype=torch.int32, device=dev) if vals is None else None
    ws = _WS.get(lib.sd3d_sort_ws_bytes(n), dev)
    landed = ctypes.c_int(0)
    _lib.check(lib.sd3d_sort_pairs_u64_ex(_ptr(keys, torch.int64, "keys"), _ptr(vals, torch.int32, "vals"),
                                          _ptr(keys_out), _ptr(vals_out), _ptr(scratch), n, begin_bit, end_bit,
                                          ws.data_ptr(), ws.numel(), ctypes.addressof(landed), _stream()), "sort_pairs")
    if landed.value:
        return keys, (vals if vals is not None else scratch)
    return keys_out, vals_out


def scan_exclusive(x: torch.Tensor):
    lib = _lib.load()
    n = x.numel()
    out = torch.empty_like(x)
    total = torch.empty(1, dtype=torch.int32, device=x.device)
    ws = _WS.get(lib.sd3d_scan_ws_bytes(n), x.device)
    _lib.check(lib.sd3d_scan_exclusive_i32(_ptr(x, torch.int32, "x"), _ptr(out), n, _ptr(total), ws.data_ptr(),
                                           ws.numel(), _stream()), "scan_exclusive")
    return out, total


def keys_from_f32(x: torch.Tensor, descending=False):
    lib = _lib.load()
    keys = torch.empty(x.numel(), dtype=torch.int64, device=x.device)
    _lib.check(lib.sd3d_keys_from_f32(_ptr(x, torch.float32, "x"), x.numel(), int(descending), _ptr(keys), _stream()),
               "keys_from_f32")
    return keys


def keys_from_i64(x: torch.Tensor, check, max_out, add: int = 0, out=None):
    """keys[i] = x[i] + add (add: the scene's bits of a batch-wide key).  check = (bits, flag int32 [1], value): flag |= value when an id
    needs more than `bits` bits (bits = 64 for no width check).  max_out int32 [1] (zeroed by the caller): receives the largest id.  Check
    and maximum are taken on x[i].  out: the caller's contiguous int64 slice of a batch-wide key buffer (default: a new tensor)."""
    lib = _lib.load()
    if out is None:
        out = torch.empty(x.numel(), dtype=torch.int64, device=x.device)
    elif out.numel() != x.numel():
        raise ValueError("keys_from_i64: output slice has another length")
    bits, flag, value = check
    _lib.check(lib.sd3d_keys_from_i64(_ptr(x, torch.int64, "x"), x.numel(), int(add), _ptr(out, torch.int64, "out"), int(bits),
                                      _ptr(flag, torch.int32, "flag"), int(value), _ptr(max_out, torch.int32, "max_out"), _stream()),
               "keys_from_i64")
    return out


# --------------------------------------------------------------------------------------------
# voxelisation / coordinate maps
# --------------------------------------------------------------------------------------------
def scene_stats(points: torch.Tensor, out: Optional[torch.Tensor] = None):
    """points [N, >=3] fp32 -> stats[9] = (min xyz, max xyz, sum xyz); `out`: a contiguous fp32 [9] row to write into."""
    lib = _lib.load()
    p, ld = _rows(points, "points")
    stats = torch.empty(9, dtype=torch.float32, device=points.device) if out is None else out
    ws = _WS.get(lib.sd3d_scene_stats_ws_bytes(), points.device)
    _lib.check(lib.sd3d_scene_stats(p, ld, points.shape[0], _ptr(stats), ws.data_ptr(), ws.numel(), _stream()),
               "scene_stats")
    return stats


def voxel_keys(points, inv_voxel: float, stats, shift_to_min=False, batch_index=0, want_icoords=True, out=None, err=None):
    """`out` = (keys [n] int64, icoords [n, 3] int32 | None, err [1] int32): slices of batch-wide buffers to write into
    (the error flag is OR-ed, so several scenes may share it)."""
    lib = _lib.load()
    p, ld = _rows(points, "points")
    n = points.shape[0]
    dev = points.device
    if out is not None:
        keys, icoords, err = out
    else:
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        icoords = torch.empty(n, 3, dtype=torch.int32, device=dev) if want_icoords else None
        if err is None:
            err = torch.zeros(1, dtype=torch.int32, device=dev)
    origin = torch.empty(3, dtype=torch.int32, device=dev)
    _lib.check(lib.sd3d_voxel_keys(p, ld, n, float(inv_voxel), _ptr(stats, torch.float32, "stats"), int(shift_to_min),
                                   int(batch_index), _ptr(origin), _ptr(keys), _ptr(icoords), _ptr(err), _stream()),
               "voxel_keys")
    return keys, icoords, origin, err


def unique_sorted(keys, src_idx, n_cap, n_dev=None, shift=0, want_seg_start=False, want_map=True, map_size=None,
                  clip=None, nuniq_out=None):
    """Run-length unique over sorted keys.  Returns (ukeys[n_cap], seg_start[n_cap+1]|None, map|None, n_unique[1])."""
    lib = _lib.load()
    dev = keys.device
    ukeys = torch.empty(n_cap, dtype=torch.int64, device=dev)
    seg = torch.empty(n_cap + 1, dtype=torch.int32, device=dev) if want_seg_start else None
    mp = torch.empty(map_size if map_size is not None else n_cap, dtype=torch.int32, device=dev) if want_map else None
    nuniq = torch.empty(1, dtype=torch.int32, device=dev) if nuniq_out is None else nuniq_out
    ws = _WS.get(lib.sd3d_unique_ws_bytes(n_cap), dev)
    _lib.check(lib.sd3d_unique_sorted(_ptr(keys, torch.int64, "keys"), _ptr(src_idx, torch.int32, "src_idx"), n_cap,
                                      _ptr(n_dev, torch.int32, "n_dev"), shift, _ptr(ukeys), _ptr(seg), _ptr(mp),
                                      _ptr(nuniq), ws.data_ptr(), ws.numel(),
                                      _ptr(clip[0], torch.float32, "clip stats") if clip else None,
                                      float(clip[1]) if clip else 0.0, int(clip[2]) if clip else 0,
                                      int(clip[3]) if clip else 0, _stream()), "unique_sorted")
    return ukeys, seg, mp, nuniq


def voxel_levels_all(skeys, sidx, n_levels: int, counts_out):
    """Every level of a (batch of) scene(s) from its sorted point keys in four launches (`sd3d_voxel_levels_all`): what
    `unique_sorted(skeys, sidx, N, None, 0, want_seg_start=True, want_map=True)` followed by `unique_sorted(shift=3)` level after level returns -
    (ukeys [L x [N]], seg_start [N + 1], inverse [N], parents [(L - 1) x [N]]); counts_out int32 [L] receives the voxels per level."""
    lib = _lib.load()
    N, dev, L = skeys.numel(), skeys.device, int(n_levels)
    uk = torch.empty(L, N, dtype=torch.int64, device=dev)
    par = torch.empty(max(1, L - 1), N, dtype=torch.int32, device=dev)
    seg = torch.empty(N + 1, dtype=torch.int32, device=dev)
    inv = torch.empty(N, dtype=torch.int32, device=dev)
    ws = _WS.get(lib.sd3d_voxel_levels_all_ws_bytes(N, L), dev)
    up = (ctypes.c_void_p * L)(*[uk.data_ptr() + 8 * N * l for l in range(L)])
    pp = (ctypes.c_void_p * max(1, L - 1))(*[par.data_ptr() + 4 * N * l for l in range(L - 1)])
    _lib.check(lib.sd3d_voxel_levels_all(_ptr(skeys, torch.int64, "skeys"), _ptr(sidx, torch.int32, "sidx"), N, L, ctypes.addressof(up), _ptr(seg),
                                         _ptr(inv), ctypes.addressof(pp), _ptr(counts_out, torch.int32, "counts_out"), ws.data_ptr(), ws.numel(),
                                         _stream()), "voxel_levels_all")
    return [uk[l] for l in range(L)], seg, inv, [par[l] for l in range(L - 1)]


_VOX_DESC_DT = np.dtype([("points", "<u8"), ("n", "<i8"), ("ld", "<i4"), ("shift_to_min", "<i4"), ("inv_voxel", "<f4"), ("key_bits", "<i4"),
                         ("n_levels", "<i4"), ("sp_bits", "<i4"), ("stats", "<u8"), ("origin", "<u8"), ("icoords", "<u8"),
                         ("keys_a", "<u8"), ("keys_b", "<u8"), ("vals_a", "<u8"), ("vals_b", "<u8"), ("ukeys0", "<u8"),
                         ("seg_start", "<u8"), ("inverse", "<u8"), ("ukeys", "<u8"), ("parents", "<u8"), ("readback", "<u8"),
                         ("superpoints", "<u8"), ("sp_keys", "<u8"), ("ws", "<u8"), ("ws_bytes", "<u8")], align=True)      # sd3d_voxelise_desc
assert _VOX_DESC_DT.itemsize == 176, _VOX_DESC_DT.itemsize


def voxelise_scene(points, inv_voxel: float, shift_to_min: bool, key_bits: int, n_levels: int, superpoints=None, sp_bits: int = 64):
    """One scene's voxelisation chain from ONE C call (`sd3d_voxelise_scene`): what scene_stats + voxel_keys + sort_pairs + unique_sorted
    (segment starts, point -> voxel map, then the coarser levels) + keys_from_i64(max_out) give when called one after the other - the same kernels
    in the same order, issued from C instead of from ~10 Python calls in front of everything else the scene needs.
    -> dict(stats, origin, icoords, skeys, sidx, ukeys [L x [N]], seg_start, inverse, parents [L-1 x [N]], readback int32 [L + 2], sp_keys | None)"""
    lib = _lib.load()
    p, ld = _rows(points, "points")
    N, dev, L = points.shape[0], points.device, int(n_levels)
    Np = (N + 63) // 64 * 64                                                                                 # (every array keeps the alignment of an allocation of its own)
    i64 = torch.empty(L + 2 + (1 if superpoints is not None else 0), Np, dtype=torch.int64, device=dev)[:, :N]   # key ping-pong, unique keys per level, id keys
    i32 = torch.empty(L + 2, Np, dtype=torch.int32, device=dev)[:, :N]                                       # value ping-pong, map, parents per level
    icoords = torch.empty(N, 3, dtype=torch.int32, device=dev)
    seg = torch.empty(N + 1, dtype=torch.int32, device=dev)
    stats = torch.empty(9, dtype=torch.float32, device=dev)
    small = torch.empty(3 + L + 2, dtype=torch.int32, device=dev)                                            # origin, read-back
    origin, rb = small[:3], small[3:]
    uk_ptr = (ctypes.c_void_p * max(1, L - 1))(*[i64[3 + l].data_ptr() for l in range(L - 1)])
    par_ptr = (ctypes.c_void_p * max(1, L - 1))(*[i32[3 + l].data_ptr() for l in range(L - 1)])
    ws = _WS.get(lib.sd3d_voxelise_scene_ws_bytes(N, L), dev)
    sp_keys = i64[L + 2] if superpoints is not None else None
    d = np.zeros(1, dtype=_VOX_DESC_DT)
    d[0] = (p, N, ld, int(bool(shift_to_min)), float(inv_voxel), int(key_bits), L, int(sp_bits), stats.data_ptr(), origin.data_ptr(), icoords.data_ptr(),
            i64[0].data_ptr(), i64[1].data_ptr(), i32[0].data_ptr(), i32[1].data_ptr(), i64[2].data_ptr(), seg.data_ptr(), i32[2].data_ptr(),
            ctypes.addressof(uk_ptr), ctypes.addressof(par_ptr), rb.data_ptr(),
            0 if superpoints is None else _ptr(superpoints, torch.int64, "superpoints"), 0 if sp_keys is None else sp_keys.data_ptr(),
            ws.data_ptr(), ws.numel())
    in_a = ctypes.c_int(0)
    _lib.check(lib.sd3d_voxelise_scene(d.ctypes.data, ctypes.addressof(in_a), _stream()), "voxelise_scene")
    a = 0 if in_a.value else 1
    return dict(stats=stats, origin=origin, icoords=icoords, skeys=i64[a], sidx=i32[a], ukeys=[i64[2]] + [i64[3 + l] for l in range(L - 1)],
                seg_start=seg, inverse=i32[2], parents=[i32[3 + l] for l in range(L - 1)], readback=rb, sp_keys=sp_keys)


def hash_build(ukeys: torch.Tensor, n: int):
    lib = _lib.load()
    cap = 1
    while cap < 2 * n + 2:
        cap *= 2
    tk = torch.empty(cap, dtype=torch.int64, device=ukeys.device)
    tv = torch.empty(cap, dtype=torch.int32, device=ukeys.device)
    _lib.check(lib.sd3d_hash_build(_ptr(ukeys, torch.int64, "ukeys"), n, _ptr(tk), _ptr(tv), cap, _stream()), "hash_build")
    return tk, tv


def kernel_map(out_keys, n_out, table, offsets_i8, pair_count=None, mirrored=False):
    """offsets_i8: int8 [K,3] device tensor.  Returns nbr int32 [K, n_out].  pair_count: optional int32 [64]
    device counters (pre-zeroed) whose sum is the rulebook size.  mirrored: the table is the voxel set's own and
    offsets[K-1-k] == -offsets[k] (centred odd kernel) - half the probes."""
    lib = _lib.load()
    tk, tv = table
    K = offsets_i8.shape[0]
    nbr = torch.empty(K, n_out, dtype=torch.int32, device=out_keys.device)
    _lib.check(lib.sd3d_kernel_map(_ptr(out_keys, torch.int64, "out_keys"), n_out, _ptr(tk), _ptr(tv), tk.numel(),
                                   _ptr(offsets_i8, torch.int8, "offsets"), K, 1 if mirrored else 0, _ptr(nbr),
                                   _ptr(pair_count, torch.int32, "pair_count"), _stream()), "kernel_map")
    return nbr


def kernel_maps_hier(keys, parents, n_vox, offs3, offs5, inv27, pair_counts=None, perm8=None, block_counts=None):
    """The 3^3 kernel maps of every level (+ the 5^3 map of level 0 when `offs5` is given) from ONE call, through the level hierarchy of
    the sorted keys instead of hash tables (`sd3d_kernel_maps_hier`).  keys: per level int64 [n_l] (finest first); parents: per level
    but the last int32 [n_l]; offs3 / offs5: device int8 [27, 3] / [125, 3]; inv27: numpy int8 [27] ((dx+1) + 3 (dy+1) + 9 (dz+1) -> row
    of offs3).  pair_counts: zeroed int32 [(L + 1), 64] or None.  perm8 (int32 [8], as `stride_maps`): the stride-2 maps of every level
    pair come out of the same launches.  block_counts: a dict that receives {(level, 3 | 5): int32 [K, ceil(n_l / 256)]}, the tables' entry
    counts per (offset, 256-row block) for `pair_lists_batch` (every level but the coarsest, and the 5^3 table).
    -> ([nbr3 per level], nbr5 | None, [(nbr_down, nbr_up) per level pair] | None)"""
    lib = _lib.load()
    L = len(keys)
    dev = keys[0].device
    n = (ctypes.c_int64 * L)(*[int(v) for v in n_vox])
    nbr3 = [torch.empty(27, int(n_vox[l]), dtype=torch.int32, device=dev) for l in range(L)]
    nbr5 = torch.empty(125, int(n_vox[0]), dtype=torch.int32, device=dev) if offs5 is not None else None
    kp = (ctypes.c_void_p * L)(*[_ptr(keys[l], torch.int64, "keys") for l in range(L)])
    pp = (ctypes.c_void_p * L)(*[(_ptr(parents[l], torch.int32, "parent") if l + 1 < L else None) for l in range(L)])
    np_ = (ctypes.c_void_p * L)(*[t.data_ptr() for t in nbr3])
    inv = (ctypes.c_int8 * 27)(*[int(v) for v in inv27])
    strides, dp, up = None, None, None
    if perm8 is not None and L > 1:
        strides = [(torch.empty(8, int(n_vox[l + 1]), dtype=torch.int32, device=dev), torch.empty(8, int(n_vox[l]), dtype=torch.int32, device=dev))
                   for l in range(L - 1)]
        dp = (ctypes.c_void_p * L)(*([t[0].data_ptr() for t in strides] + [None]))
        up = (ctypes.c_void_p * L)(*([t[1].data_ptr() for t in strides] + [None]))
    c3, c5 = None, None
    if block_counts is not None:
        for l in range(L - 1):
            block_counts[(l, 3)] = torch.empty(27, (int(n_vox[l]) + 255) // 256, dtype=torch.int32, device=dev)
        c3 = (ctypes.c_void_p * L)(*([block_counts[(l, 3)].data_ptr() for l in range(L - 1)] + [None]))
        if nbr5 is not None and L > 1:
            block_counts[(0, 5)] = c5 = torch.empty(125, (int(n_vox[0]) + 255) // 256, dtype=torch.int32, device=dev)
    ws = _WS.get(lib.sd3d_kernel_maps_hier_ws_bytes(L, ctypes.addressof(n)), dev)
    _lib.check(lib.sd3d_kernel_maps_hier(L, ctypes.addressof(kp), ctypes.addressof(pp), ctypes.addressof(n), ctypes.addressof(np_),
                                         _ptr(nbr5), _ptr(offs3, torch.int8, "offs3"), _ptr(offs5, torch.int8, "offs5"),
                                         ctypes.addressof(inv), _ptr(pair_counts, torch.int32, "pair_counts"),
                                         _ptr(perm8, torch.int32, "perm8") if strides is not None else None,
                                         ctypes.addressof(dp) if strides is not None else None,
                                         ctypes.addressof(up) if strides is not None else None,
                                         ctypes.addressof(c3) if c3 is not None else None, _ptr(c5),
                                         ws.data_ptr(), ws.numel(), _stream()), "kernel_maps_hier")
    return nbr3, nbr5, strides


def stride_maps(fine_keys, parent, n_fine, n_coarse, perm8, want_down=True, want_up=True):
    lib = _lib.load()
    dev = fine_keys.device
    down = torch.empty(8, n_coarse, dtype=torch.int32, device=dev) if want_down else None
    up = torch.empty(8, n_fine, dtype=torch.int32, device=dev) if want_up else None
    _lib.check(lib.sd3d_stride_maps(_ptr(fine_keys, torch.int64, "fine_keys"), _ptr(parent, torch.int32, "parent"),
                                    n_fine, n_coarse, _ptr(perm8, torch.int32, "perm8"), _ptr(down), _ptr(up),
                                    _stream()), "stride_maps")
    return down, up


_SCENE_SRC_DT = np.dtype([("points", "<u8"), ("feats2d", "<u8"), ("stats", "<u8"), ("point_off", "<i8"), ("n_points", "<i8"),
                          ("ld_points", "<i4"), ("pad_", "<i4")], align=True)                                              # sd3d_scene_src
assert _SCENE_SRC_DT.itemsize == 48


def voxel_mean_batch(scenes, mode, ukeys, sorted_idx, seg_start, n_vox, ld_out):
    """scenes: [(points [N_i, >=6], feats2d [N_i, F] | None, stats [9], point_off)] of one batch (sparse.BatchSceneMaps);
    one launch over the voxels of all scenes."""
    lib = _lib.load()
    tab = np.zeros(len(scenes), dtype=_SCENE_SRC_DT)
    F = 0
    for i, (pts, f2d, stats, off) in enumerate(scenes):
        p, ld = _rows(pts, "points")
        if f2d is not None:
            if F and f2d.shape[1] != F:
                raise ValueError("voxel_mean_batch: every scene must carry the same number of 2D feature channels")
            F = f2d.shape[1]
        tab[i] = (p, 0 if f2d is None else _ptr(f2d, torch.float32, "feats2d"), _ptr(stats, torch.float32, "stats"), int(off),
                  pts.shape[0], ld, 0)
    dev = scenes[0][0].device
    out = torch.empty(n_vox, ld_out, dtype=torch.float32, device=dev)
    _lib.check(lib.sd3d_voxel_mean_batch(tab.ctypes.data, len(scenes), F, mode, _ptr(ukeys, torch.int64, "ukeys"),
                                         _ptr(sorted_idx, torch.int32, "sorted_idx"), _ptr(seg_start, torch.int32, "seg_start"),
                                         n_vox, _ptr(out), ld_out, _stream()), "voxel_mean_batch")
    return out


def voxel_mean(points, feats2d, mode, stats, sorted_idx, seg_start, n_vox, ld_out):
    """One scene: a batch of one, whose voxel keys are not needed."""
    return voxel_mean_batch([(points, feats2d, stats, 0)], mode, None, sorted_idx, seg_start, n_vox, ld_out)


def segment_starts_batch(sorted_ids, n, S, id_off):
    """sorted (scene << 32 | id) keys -> start[S + 1] over the dense ids id_off[scene] + id."""
    import ctypes as C
    lib = _lib.load()
    start = torch.empty(S + 1, dtype=torch.int32, device=sorted_ids.device)
    offs = (C.c_int32 * len(id_off))(*[int(v) for v in id_off])
    _lib.check(lib.sd3d_segment_starts_batch(_ptr(sorted_ids, torch.int64, "sorted_ids"), n, S, offs, len(id_off), _ptr(start),
                                             _stream()), "segment_starts_batch")
    return start


def segment_starts(sorted_ids, n, S):
    """One scene: plain sorted ids (below 2^32) -> start[S + 1]."""
    return segment_starts_batch(sorted_ids, n, S, [0])


def pool_superpoints(feat, C, inverse, icoords, voxel_size, sorted_idx, start, S):
    lib = _lib.load()
    f, ld = _rows(feat, "feat")
    out_feat = torch.empty(S, C, dtype=torch.float32, device=feat.device)
    out_pos = torch.empty(S, 3, dtype=torch.float32, device=feat.device)
    _lib.check(lib.sd3d_pool_superpoints(f, ld, C, _ptr(inverse, torch.int32, "inverse"),
                                         _ptr(icoords, torch.int32, "icoords"), float(voxel_size),
                                         _ptr(sorted_idx, torch.int32, "sorted_idx"), _ptr(start, torch.int32, "start"),
                                         S, _ptr(out_feat), _ptr(out_pos), _stream()), "pool_superpoints")
    return out_feat, out_pos


# --------------------------------------------------------------------------------------------
# gather-GEMM
# --------------------------------------------------------------------------------------------
# The gather-GEMM is exact fp32 MFMA unless the bf16 decoder scope or an explicit `wt_split` asks for the split-bf16 kernel
# (csrc/gather_gemm_split.hip: fp32 products evaluated as 1 / 3 / 6 bf16 MFMA products with fp32 accumulation).
_SPLIT_CACHE = _collections_od()
_BF16_TLS = threading.local()
# projections of fewer rows are launch-latency bound and measured FASTER on the exact fp32 small-M kernel (200-query decoder:
# 2.6 ms fp32, 3.5 ms with every Linear on the bf16 kernel); exact fp32 is never less precise than the bf16 the mode allows
BF16_MIN_ROWS = int(_os.environ.get("SD3D_BF16_MIN_ROWS", "1024"))


class bf16_decoder_scope:
    """BASELINE config #3 ("bf16 decoder"): inside the scope every dense projection (`linear`, `gather_gemm` without a
    neighbour table and without `exact=True`) runs with bf16 operands and fp32 accumulation, and `attention` runs its two
    contractions on the bf16 MFMA.  LayerNorm, softmax, the positional encodings, the mask head's logits and every
    threshold stay fp32 ("bf16 decoder").  Per thread; nests."""

    def __init__(self, enabled=True):
        self.enabled = bool(enabled)

    def __enter__(self):
        self.prev = getattr(_BF16_TLS, "on", False)
        _BF16_TLS.on = self.enabled or self.prev
        return self

    def __exit__(self, *exc):
        _BF16_TLS.on = self.prev
        return False


def bf16_decoder_active() -> bool:
    return getattr(_BF16_TLS, "on", False)


def split_weights(wt, terms):
    """fp32 [K, Cout, Cin] -> bf16 [terms_per_operand, K, Cout, Cin] with wt = sum of the terms (to ~2^-17 / 2^-25)."""
    ns = {1: 1, 3: 2, 6: 3}[terms]
    if ns == 1:                                          # plain rounding: one conversion kernel (training re-rounds live weights per step)
        return wt.detach().to(torch.bfloat16).unsqueeze(0).contiguous()
    r = wt.detach().to(torch.float32).clone()
    parts = []
    for _ in range(ns):
        t = r.to(torch.bfloat16)
        parts.append(t)
        r = r - t.to(torch.float32)
    return torch.stack(parts).contiguous()


_SPLIT_CACHE_MAX = 1024          # a decoder forward touches ~110 distinct Linear weights in the bf16 mode (17 per layer + heads); owners clear on change
_SPLIT_LOCK = threading.Lock()   # the scene threads of dist_eval.PipelinedRunner share the cache


def _cached_split(wt, terms):
    """bf16 rounding(s) of a weight tensor, cached.  An entry keeps its SOURCE tensor alive, so the address in the key
    cannot be handed to another tensor while the entry exists (the caching allocator reuses addresses of freed blocks: a
    rebuilt set of packed weights lands where the old one was); in-place updates move `_version`.  Least-recently-used
    entries are dropped beyond _SPLIT_CACHE_MAX; owners drop everything with clear_split_cache() when their weights change.
    Lookups, insertions and evictions happen under one lock (a hit moves the entry to the end, nothing is popped on the way)."""
    key = (wt.data_ptr(), tuple(wt.shape), tuple(wt.stride()), terms, wt._version)
    with _SPLIT_LOCK:
        hit = _SPLIT_CACHE.get(key)
        if hit is not None:
            _SPLIT_CACHE.move_to_end(key)
            return hit[0]
    made = (split_weights(wt, terms), wt)                 # outside the lock: a conversion launch; a racing thread makes an equal copy
    with _SPLIT_LOCK:
        hit = _SPLIT_CACHE.setdefault(key, made)
        _SPLIT_CACHE.move_to_end(key)
        while len(_SPLIT_CACHE) > _SPLIT_CACHE_MAX:
            _SPLIT_CACHE.popitem(last=False)
    return hit[0]


_IN_FLIGHT = [1]


def scenes_in_flight_now() -> int:
    """How many independent scenes the caller keeps in flight on this GPU (set by `scenes_in_flight`, default 1)."""
    return _IN_FLIGHT[0]


class scenes_in_flight:
    """Context: tell the launchers that `n` independent scenes run concurrently on this GPU (sd3d_set_scenes_in_flight)."""

    def __init__(self, n):
        self.n = int(n)

    def __enter__(self):
        self.prev = _lib.load().sd3d_set_scenes_in_flight(self.n)
        self.prev_py, _IN_FLIGHT[0] = _IN_FLIGHT[0], self.n
        return self

    def __exit__(self, *exc):
        _lib.load().sd3d_set_scenes_in_flight(self.prev)
        _IN_FLIGHT[0] = self.prev_py
        return False


def clear_split_cache():
    with _SPLIT_LOCK:
        _SPLIT_CACHE.clear()


class PairLists:
    """Offset-major layout of one neighbour table (csrc/pair_gemm.hip): shared by every convolution that uses it.
    Optional products (sd3d_pair_lists_desc): `rlist` [M, rl_stride] per-row partial-product lists, `center` = -1 (plain lists) or
    PAIR_CHAINED (mirror offsets + centre share one partial product), `direct` = every output row has exactly one pair (`out_idx`
    is then built and pass 1 writes the output rows itself)."""
    __slots__ = ("pos", "in_idx", "tile_k", "p_cap", "K", "M", "out_idx", "rlist", "rl_stride", "center", "direct")

    def __init__(self, pos, in_idx, tile_k, p_cap, K, M, rlist=None, rl_stride=0, center=-1, out_idx=None, direct=False):
        self.pos, self.in_idx, self.tile_k, self.p_cap, self.K, self.M = pos, in_idx, tile_k, p_cap, K, M
        self.out_idx = out_idx                            # output row of every pair; built on demand otherwise (train_ops.pair_out_rows)
        self.rlist, self.rl_stride, self.center, self.direct = rlist, rl_stride, center, direct


def pair_lists(nbr, n_pairs, center=-1, direct=False):
    """nbr int32 [K, M]; n_pairs = number of entries >= 0 (host int, e.g. from kernel_map's pair counter).  `center` / `direct`:
    see PairLists (the caller vouches for them: an odd stride-1 table of a voxel set onto itself / a one-pair-per-row table)."""
    return pair_lists_batch([(nbr, n_pairs, center, direct)])[0]


# Sparse convolutions run pair-major (pair_conv) whenever the caller hands over the table's PairLists;
# SD3D_PAIR_CONV=0 keeps the output-stationary gather_gemm kernels (tuning / ablation).
PAIR_CONV = _os.environ.get("SD3D_PAIR_CONV", "1") != "0"
_PAIR_DESC_DT = np.dtype([("nbr", "<u8"), ("pos", "<u8"), ("in_idx", "<u8"), ("tile_k", "<u8"), ("rlist", "<u8"), ("out_idx", "<u8"),
                          ("M", "<i8"), ("p_cap", "<i8"), ("K", "<i4"), ("center", "<i4"), ("rl_stride", "<i4"), ("meta", "<i4")],
                         align=True)                                                                                       # sd3d_pair_table_desc
assert _PAIR_DESC_DT.itemsize == 80


PAIR_CHAINED = -2          # SD3D_PAIR_CHAINED: `center` value of a chained table (include/segdino3d_hip.h)


def pair_lists_batch(tables):
    """tables: list of (nbr int32 [K, M], n_pairs[, center[, direct[, lean[, counts]]]]) -> list of PairLists, built by ONE launch set
    (csrc/pair_gemm.hip: count, scan, fill, per-row lists).  center = PAIR_CHAINED: chained lists (a stride-1 table of a voxel set
    onto itself, odd symmetric kernel): the entries of a row's mirror groups and its centre share partial products.  counts (a lean
    plain table only): int32 [K, ceil(M / 256)] from `kernel_maps_hier(block_counts=...)`; the table is not read again to count, and
    the tensor is consumed (scanned in place)."""
    lib = _lib.load()
    out = []
    for start in range(0, len(tables), 16):
        chunk = tables[start:start + 16]
        dev = chunk[0][0].device
        desc = np.zeros(len(chunk), dtype=_PAIR_DESC_DT)
        res, nb = [], 0
        given = (ctypes.c_void_p * len(chunk))()
        for i, t in enumerate(chunk):
            nbr, n_pairs = t[0], t[1]
            center = int(t[2]) if len(t) > 2 else -1
            direct = bool(t[3]) if len(t) > 3 else False
            lean = bool(t[4]) if len(t) > 4 else False            # evaluation: no [K, M] position table, the unused capacity stays unwritten
            K, M = nbr.shape
            chained = center == PAIR_CHAINED
            if chained:
                if direct or K % 2 == 0:
                    raise ValueError("pair_lists: chained lists need an odd symmetric kernel")
                p_cap = (int(n_pairs) + 127 * (11 * (K // 2) + 1) + 127) // 128 * 128
                pos = torch.empty(0, dtype=torch.int32, device=dev)       # (a chained table has no [K, M] position table: its rows' partial positions are `rlist`)
            else:
                p_cap = (int(n_pairs) + 127 * K + 127) // 128 * 128
                lean = lean and K <= 128
                pos = None if lean else torch.empty(K, M, dtype=torch.int32, device=dev)
            in_idx = torch.empty(p_cap, dtype=torch.int32, device=dev)
            tile_k = torch.empty(p_cap // 128 + 3, dtype=torch.int32, device=dev)     # [p_cap / 128]: number of real tiles, then the centre run
            # per-row list {count, partial positions}: K entries at most - K / 2 + 1 (mirror groups + the lone centre) for a chained table
            rl_stride = ((K // 2 + 2) + 3) // 4 * 4 if chained else (K + 4 + 3) // 4 * 4
            rlist = None if direct else torch.empty(M, rl_stride, dtype=torch.int32, device=dev)
            out_idx = torch.empty(p_cap, dtype=torch.int32, device=dev) if direct else None
            desc[i] = (_ptr(nbr, torch.int32, "nbr"), 0 if pos is None else pos.data_ptr(), in_idx.data_ptr(), tile_k.data_ptr(),
                       0 if rlist is None else rlist.data_ptr(), 0 if out_idx is None else out_idx.data_ptr(), M, p_cap, K, center,
                       rl_stride, 3 if lean else 1)
            counts = t[5] if len(t) > 5 else None
            if counts is not None:
                if not lean or chained or tuple(counts.shape) != (K, (M + 255) // 256):
                    raise ValueError("pair_lists: block counts go with a lean plain table, int32 [K, ceil(M / 256)]")
                given[i] = _ptr(counts, torch.int32, "counts")
            nb += (lib.sd3d_pair_lists_ws_bytes(K, M) + 255) // 256 * 256
            res.append(PairLists(pos, in_idx, tile_k, p_cap, K, M, rlist=rlist, rl_stride=rl_stride, center=center, out_idx=out_idx,
                                 direct=direct))
        ws = _WS4.get(nb, dev)
        _lib.check(lib.sd3d_pair_lists_desc(len(chunk), desc.ctypes.data, ctypes.addressof(given) if any(given) else None,
                                            ws.data_ptr(), ws.numel(), _stream()), "pair_lists_desc")
        out += res
    return out


def pair_conv(x, wt, pairs, x2=None, scale=None, shift=None, res=None, act=None, out=None, mirror_w=False):
    """Same contract as gather_gemm(x, wt, nbr=...) for the table `pairs` was built from.
    mirror_w: offset k multiplies wt[K - 1 - k] (SD3D_PAIR_MIRROR_W: the input gradient of a stride-1 convolution on its own table with
    the parameter in its native [K, Cin, Cout] layout, train_ops.SparseConvNative)."""
    lib = _lib.load()
    K, Cout, Cin = wt.shape
    if K != pairs.K:
        raise ValueError(f"weights have {K} offsets, the pair lists {pairs.K}")
    p0, ld0 = _rows(x, "x")
    C0 = x.shape[1]
    p1, ld1 = (None, 0)
    if x2 is not None:
        p1, ld1 = _rows(x2, "x2")
        if C0 + x2.shape[1] != Cin:
            raise ValueError(f"concat channels {C0}+{x2.shape[1]} != Cin {Cin}")
    elif C0 != Cin:
        raise ValueError(f"input channels {C0} != Cin {Cin}")
    M = pairs.M
    if out is None:
        out = torch.empty(M, Cout, dtype=torch.float32, device=x.device)
    po, ldo = _rows(out, "out")
    pr, ldr = (None, 0)
    if res is not None:
        pr, ldr = _rows(res, "res")
    part = _WS3.get(pairs.p_cap * Cout * 4, x.device)
    hook = GG_HOOK
    if hook is not None:
        hook.before(dict(K=K, Cin=Cin, Cout=Cout, M=M, nbr=None, pairs=pairs))
    _lib.check(lib.sd3d_pair_conv_ex(p0, ld0, C0, p1, ld1, pairs.in_idx.data_ptr(), pairs.tile_k.data_ptr(), pairs.p_cap,
                                     None if pairs.pos is None else pairs.pos.data_ptr(), None if pairs.rlist is None else pairs.rlist.data_ptr(), pairs.rl_stride,
                                     pairs.center - 2 if mirror_w else pairs.center, pairs.out_idx.data_ptr() if pairs.direct else None,
                                     _ptr(wt, torch.float32, "wt"), K, Cin, Cout, M,
                                     _ptr(scale, torch.float32, "scale"), _ptr(shift, torch.float32, "shift"), pr, ldr, po, ldo,
                                     ACT[act], part.data_ptr(), part.numel(), _stream()), "pair_conv")
    if hook is not None:
        hook.after()
    return out


_LINEAR_JOB_DT = np.dtype([("in0", "<u8"), ("in1", "<u8"), ("wt", "<u8"), ("shift", "<u8"), ("res", "<u8"), ("out", "<u8"),
                           ("M", "<i8"), ("ld0", "<i4"), ("C0", "<i4"), ("ld1", "<i4"), ("Cin", "<i4"), ("Cout", "<i4"),
                           ("ld_res", "<i4"), ("ld_out", "<i4"), ("act", "<i4")], align=True)                              # sd3d_linear_job
assert _LINEAR_JOB_DT.itemsize == 88


def dense_code(rows: int, cin: int, cout: int) -> int:
    """Tiling code of sd3d_gather_gemm that reproduces, for ANY number of rows, the kernel its heuristic picks for a plain Linear
    on `rows` rows (sd3d_dense_plan_code - the C library's own answer): the batched decoder passes it so that the rows of several
    scenes run on the SAME kernel - same summation order - as one scene's rows.  0 = the lock-step kernel (>= 64 row tiles: its order
    does not depend on the row count), -1 = one 32-column tile per wave with the contraction split over the four waves of a
    workgroup, n > 0 = n column tiles per wave, no split."""
    return _lib.load().sd3d_dense_plan_code(int(rows), int(cin), int(cout))


def small_rows_code(cin: int) -> int:
    """dense_code for <= 512 rows and <= 1024 output columns (the decoder's query tensors)."""
    return -1 if cin // 32 >= 8 else 1


def linear_group(jobs, force_small=False):
    """jobs: list of (x, weight [Cout, Cin], bias | None, act | None, res | None, x2 | None) - INDEPENDENT plain Linears on a few
    hundred rows each; returns their outputs.  Up to 8 per launch (csrc/gather_gemm.hip gather_gemm_group_kernel).  Jobs on
    >= 2017 rows each go out together as well, every one on the lock-step tiling its own launch would use
    (gather_gemm_lds_group_kernel: same bits).  Mixed sizes, the bf16 decoder scope on >= BF16_MIN_ROWS rows and the
    instrumentation hook run one by one.
    force_small: the rows are several scenes' few-hundred-row tensors back to back - always the group kernel."""
    if GG_HOOK is not None:
        if force_small:
            return [gather_gemm(x, w, x2=x2, shift=b, act=act, res=res, nt=-1, exact=True) for (x, w, b, act, res, x2) in jobs]
        return [gather_gemm(x, w, x2=x2, shift=b, act=act, res=res) for (x, w, b, act, res, x2) in jobs]
    if len(jobs) == 1:
        x, w, b, act, res, x2 = jobs[0]
        if force_small:                                         # the kernel the heuristic picks for ONE scene's rows
            return [gather_gemm(x, w, x2=x2, shift=b, act=act, res=res, nt=small_rows_code(w.shape[-1]), exact=True)]
        return [gather_gemm(x, w, x2=x2, shift=b, act=act, res=res)]
    bf16 = getattr(_BF16_TLS, "on", False)
    # (an empty job - no rows or no output columns - goes out alone: sd3d_linear_group refuses it, sd3d_gather_gemm launches nothing for it)
    small = [(force_small or (x.shape[0] < 2048 and not (bf16 and x.shape[0] >= BF16_MIN_ROWS) and x.shape[0] > 0)) and w.shape[0] > 0
             for (x, w, *_r) in jobs]
    # a few thousand rows each (one query per superpoint): the lock-step kernel of the single launch, several jobs per launch
    large = not bf16 and not force_small and all(w.dim() == 2 and w.shape[1] % 32 == 0 and dense_code(x.shape[0], w.shape[1], w.shape[0]) == 0
                                                   for (x, w, *_r) in jobs)
    if not all(small) and not large:
        return [gather_gemm(x, w, x2=x2, shift=b, act=act, res=res) for (x, w, b, act, res, x2) in jobs]
    lib = _lib.load()
    outs = []
    for start in range(0, len(jobs), 8):
        chunk = jobs[start:start + 8]
        tab = np.zeros(len(chunk), dtype=_LINEAR_JOB_DT)
        for i, (x, w, b, act, res, x2) in enumerate(chunk):
            if not (x.is_cuda and w.is_cuda) or x.dtype is not torch.float32 or w.dtype is not torch.float32 or x.dim() != 2 \
                    or x.stride(1) != 1 or not w.is_contiguous() or w.dim() != 2:
                raise ValueError("linear_group: expected 2-D fp32 device tensors with contiguous rows")
            M, C0 = x.shape
            Cout, Cin = w.shape
            if (x2 is None and C0 != Cin) or (x2 is not None and (C0 + x2.shape[1] != Cin or x2.stride(1) != 1 or x2.shape[0] != M)):
                raise ValueError(f"linear_group: input channels do not match Cin {Cin}")
            out = torch.empty(M, Cout, dtype=torch.float32, device=x.device)
            if res is not None and (res.shape != out.shape or res.stride(1) != 1 or res.dtype is not torch.float32):
                raise ValueError("linear_group: residual must be an fp32 [rows, Cout] tensor")
            if b is not None and (b.numel() != Cout or not b.is_contiguous() or b.dtype is not torch.float32):
                raise ValueError("linear_group: bias must be a contiguous fp32 [Cout] tensor")
            tab[i] = (x.data_ptr(), 0 if x2 is None else x2.data_ptr(), w.data_ptr(), 0 if b is None else b.data_ptr(),
                      0 if res is None else res.data_ptr(), out.data_ptr(), M, x.stride(0), C0, 0 if x2 is None else x2.stride(0), Cin, Cout,
                      0 if res is None else res.stride(0), Cout, ACT[act])
            outs.append(out)
        rc = lib.sd3d_linear_group(len(chunk), tab.ctypes.data, _stream())
        if rc:
            _lib.check(rc, "linear_group")
    return outs


def _dense_linear(x, wt, x2, shift, res, act):
    """Short host path of the plain Linear y = act(x wt^T + shift + res) on [x | x2] (the decoder issues ~150 of them per
    forward; the general entry below spends ~14 us of Python per call, this one ~4): same kernel, same checks that matter -
    device tensors, fp32, contiguous rows, matching widths."""
    if not (x.is_cuda and wt.is_cuda):
        raise RuntimeError("gather_gemm: expected tensors on the HIP device (no CPU fallback)")
    if x.dtype is not torch.float32 or wt.dtype is not torch.float32 or x.dim() != 2 or x.stride(1) != 1 or not wt.is_contiguous():
        raise ValueError("gather_gemm: expected 2-D fp32 tensors with contiguous rows")
    rows, C0 = x.shape
    Cout, Cin = wt.shape
    p1, ld1 = None, 0
    if x2 is not None:
        if x2.dtype is not torch.float32 or x2.stride(1) != 1 or not x2.is_cuda or C0 + x2.shape[1] != Cin:
            raise ValueError(f"gather_gemm: bad second source for Cin {Cin}")
        p1, ld1 = x2.data_ptr(), x2.stride(0)
    elif C0 != Cin:
        raise ValueError(f"input channels {C0} != Cin {Cin}")
    pr, ldr = None, 0
    if res is not None:
        if res.dtype is not torch.float32 or res.stride(1) != 1 or not res.is_cuda or res.shape[0] != rows or res.shape[1] != Cout:
            raise ValueError("gather_gemm: residual must be an fp32 [rows, Cout] device tensor")
        pr, ldr = res.data_ptr(), res.stride(0)
    ps = None
    if shift is not None:
        if not shift.is_cuda or shift.dtype is not torch.float32 or shift.numel() != Cout or not shift.is_contiguous():
            raise ValueError("gather_gemm: shift must be a contiguous fp32 [Cout] device tensor")
        ps = shift.data_ptr()
    out = torch.empty((rows, Cout), dtype=torch.float32, device=x.device)
    rc = _lib.load().sd3d_gather_gemm(x.data_ptr(), x.stride(0), C0, p1, ld1, None, wt.data_ptr(), 1, Cin, Cout, rows, None, ps, pr, ldr,
                                      out.data_ptr(), Cout, ACT[act], 0, None, 0, _stream())
    if rc:
        _lib.check(rc, "gather_gemm")
    return out


def gather_gemm(x, wt, nbr=None, x2=None, scale=None, shift=None, res=None, act=None, out=None, M=None, nt=0,
                density=None, wt_split=None, pairs=None, exact=False):
    """out[r, n] = act(scale[n] * sum_k sum_c X[nbr[k, r], c] * wt[k, n, c] + shift[n] + res[r, n]).

    x [V_in, C0] (rows may be strided), optional x2 [V_in, C1] = concatenated channels,
    wt [K, Cout, Cin] contiguous, nbr int32 [K, M] or None (identity rows, K = 1).  With `pairs` (the table's
    PairLists) a sparse convolution runs pair-major (pair_conv); `density` is informational (kept for callers that
    pass SceneMaps.conv_table(...) as keyword arguments)."""
    if nbr is None and pairs is None and GG_HOOK is None and scale is None and out is None and wt_split is None and nt == 0 \
            and M is None and wt.dim() == 2 and not getattr(_BF16_TLS, "on", False):
        return _dense_linear(x, wt, x2, shift, res, act)
    lib = _lib.load()
    if wt.dim() == 2:
        wt = wt.unsqueeze(0)
    if pairs is not None and PAIR_CONV and nt == 0 and wt_split is None and wt.shape[1] % 4 == 0:
        return pair_conv(x, wt, pairs, x2=x2, scale=scale, shift=shift, res=res, act=act, out=out)
    K, Cout, Cin = wt.shape
    p0, ld0 = _rows(x, "x")
    C0 = x.shape[1]
    p1, ld1 = (None, 0)
    if x2 is not None:
        p1, ld1 = _rows(x2, "x2")
        if C0 + x2.shape[1] != Cin:
            raise ValueError(f"concat channels {C0}+{x2.shape[1]} != Cin {Cin}")
    elif C0 != Cin:
        raise ValueError(f"input channels {C0} != Cin {Cin}")
    if M is None:
        M = nbr.shape[1] if nbr is not None else x.shape[0]
    if nbr is not None and (nbr.shape[0] != K or nbr.shape[1] != M):
        raise ValueError(f"nbr shape {tuple(nbr.shape)} != ({K}, {M})")
    if out is None:
        out = torch.empty(M, Cout, dtype=torch.float32, device=x.device)
    po, ldo = _rows(out, "out")
    pr, ldr = (None, 0)
    if res is not None:
        pr, ldr = _rows(res, "res")
    terms = 0
    if wt_split is not None:
        terms = {1: 1, 2: 3, 3: 6}[wt_split.shape[0]]
    elif nbr is None and not exact and bf16_decoder_active() and M >= BF16_MIN_ROWS and Cin % 32 == 0 and (x2 is None or C0 % 32 == 0):
        terms = 1                                  # bf16 decoder: plain bf16 operands (weights rounded once, cached)
        wt_split = _cached_split(wt, terms)
    hook = GG_HOOK
    if hook is not None:
        hook.before(dict(K=K, Cin=Cin, Cout=Cout, M=M, nbr=nbr))
    ws_ptr, ws_n = None, 0
    if nbr is not None and K >= 8 and M * Cout <= (1 << 22):      # small launch: allow split-K partials
        ws = _WS2.get(8 * M * Cout * 4, x.device)
        ws_ptr, ws_n = ws.data_ptr(), ws.numel()
    if terms:
        if wt_split.dtype != torch.bfloat16 or not wt_split.is_contiguous() or tuple(wt_split.shape[1:]) != (K, Cout, Cin):
            raise ValueError("wt_split must be contiguous bf16 [1|2|3, K, Cout, Cin]")
        _lib.check(lib.sd3d_gather_gemm_split(p0, ld0, C0, p1, ld1, _ptr(nbr, torch.int32, "nbr"), wt_split.data_ptr(),
                                              terms, K, Cin, Cout, M, _ptr(scale, torch.float32, "scale"),
                                              _ptr(shift, torch.float32, "shift"), pr, ldr, po, ldo, ACT[act],
                                              max(nt, 0), ws_ptr, ws_n, _stream()), "gather_gemm_split")
        if hook is not None:
            hook.after()
        return out
    _lib.check(lib.sd3d_gather_gemm(p0, ld0, C0, p1, ld1, _ptr(nbr, torch.int32, "nbr"), _ptr(wt, torch.float32, "wt"),
                                    K, Cin, Cout, M, _ptr(scale, torch.float32, "scale"),
                                    _ptr(shift, torch.float32, "shift"), pr, ldr, po, ldo, ACT[act], nt, ws_ptr, ws_n,
                                    _stream()), "gather_gemm")
    if hook is not None:
        hook.after()
    return out


def linear(x, weight, bias=None, act=None, res=None, out=None):
    """y = act(x @ weight.T + bias (+ res)); weight [Cout, Cin] as stored by nn.Linear."""
    return gather_gemm(x, weight, shift=bias, act=act, res=res, out=out)


# --------------------------------------------------------------------------------------------
# decoder ops
# --------------------------------------------------------------------------------------------
def layernorm(x, weight, bias, res=None, act=None, eps=1e-5, out=None):
    lib = _lib.load()
    px, ldx = _rows(x, "x")
    pr, ldr = (None, 0) if res is None else _rows(res, "res")
    if out is None:
        out = torch.empty(x.shape[0], x.shape[1], dtype=torch.float32, device=x.device)
    po, ldo = _rows(out, "out")
    _lib.check(lib.sd3d_layernorm(px, ldx, pr, ldr, _ptr(weight, torch.float32, "weight"), _ptr(bias, torch.float32, "bias"),
                                  float(eps), x.shape[0], x.shape[1], po, ldo, ACT[act], _stream()), "layernorm")
    return out


LINEAR_LN_MAX_ROWS = int(_os.environ.get("SD3D_LINEAR_LN_MAX_ROWS", "512"))      # 0 switches the fused launch off


def linear_layernorm(x, weight, bias, ln_weight, ln_bias, res=None, act=None, eps=1e-5, max_rows=None):
    """act(LayerNorm(x @ weight^T + bias + res) * ln_weight + ln_bias).  Few rows and a 256-wide output (the decoder's query tensors):
    one fused launch (sd3d_linear_layernorm); anything else - or an instrumented run - is the projection followed
    by the LayerNorm kernel."""
    M, Cin = x.shape
    # (measured at 200 rows: Cin = 256 14.5 us fused vs 21.9 us in two launches; Cin = 1024 39.9 vs 22.2 - a 16-row workgroup walks
    # the whole contraction alone - so long contractions keep the two launches)
    # max_rows: the rows of several scenes of <= LINEAR_LN_MAX_ROWS rows each take the fused launch too (16-row workgroups:
    # per row the same arithmetic whatever M is - the batched decoder must not switch kernels with the batch size)
    if (M > (LINEAR_LN_MAX_ROWS if max_rows is None else max_rows) or Cin > 512 or weight.shape[0] != 256 or Cin % 16 or GG_HOOK is not None
            or not weight.is_contiguous() or (res is not None and res.stride(1) != 1)):
        return layernorm(gather_gemm(x, weight, shift=bias, res=res), ln_weight, ln_bias, act=act, eps=eps)
    lib = _lib.load()
    px, ldx = _rows(x, "x")
    pr, ldr = (None, 0) if res is None else _rows(res, "res")
    out = torch.empty(M, 256, dtype=torch.float32, device=x.device)
    _lib.check(lib.sd3d_linear_layernorm(px, ldx, M, Cin, _ptr(weight, torch.float32, "weight"), 256,
                                         None if bias is None else _ptr(bias, torch.float32, "bias"), pr, ldr,
                                         _ptr(ln_weight, torch.float32, "ln_weight"), _ptr(ln_bias, torch.float32, "ln_bias"), float(eps), ACT[act],
                                         out.data_ptr(), 256, _stream()), "linear_layernorm")
    return out


def sine_pe(xyz, rng, dim_t, axis, mod_num=None, mod_den=None, row_scene=None):
    """xyz [n,3]; rng [6] = (lo, hi); dim_t [d] fp32, axis [d] int8 -> [n, d].  row_scene int32 [n]: rows of several scenes,
    rng is then [n_scenes, 6] and row r uses rng[row_scene[r]]."""
    n, d = xyz.shape[0], dim_t.numel()
    _want_ranges(rng, row_scene, n, "sine_pe")
    if mod_num is not None:
        if mod_den is None:
            raise ValueError("sine_pe: mod_num given without mod_den")
        _want_shape(mod_num, [(n, 3)], "sine_pe: mod_num")
        _want_shape(mod_den, [(3,), (n, 3)], "sine_pe: mod_den")
    lib = _lib.load()
    px, ldx = _rows(xyz, "xyz")
    out = torch.empty(n, d, dtype=torch.float32, device=xyz.device)
    pn, ldn, pd, ldd = None, 0, None, 0
    if mod_num is not None:
        pn, ldn = _rows(mod_num, "mod_num")
        if mod_den.dim() == 1:
            pd, ldd = _ptr(mod_den, torch.float32, "mod_den"), 0
        else:
            pd, ldd = _rows(mod_den, "mod_den")
    _lib.check(lib.sd3d_sine_pe(px, ldx, n, _ptr(rng, torch.float32, "rng"), _ptr(row_scene, torch.int32, "row_scene"),
                                _ptr(dim_t, torch.float32, "dim_t"), _ptr(axis, torch.int8, "axis"), d, pn, ldn, pd, ldd,
                                _ptr(out), d, _stream()), "sine_pe")
    return out


def fourier_pe(xyz, rng, gauss_b, d_pos, row_scene=None):
    """xyz [n,3]; rng [6] = (lo, hi); gauss_b [3, >= d_pos / 2] fp32 -> [n, d_pos] = [sin | cos] (utils.py:107-142)."""
    n = xyz.shape[0]
    _want_ranges(rng, row_scene, n, "fourier_pe")
    lib = _lib.load()
    px, ldx = _rows(xyz, "xyz")
    pb, ldb = _rows(gauss_b, "gauss_b")
    if gauss_b.shape[0] != 3 or gauss_b.shape[1] < d_pos // 2:
        raise ValueError("fourier_pe: gauss_b must be [3, >= d_pos / 2]")
    out = torch.empty(n, d_pos, dtype=torch.float32, device=xyz.device)
    _lib.check(lib.sd3d_fourier_pe(px, ldx, n, _ptr(rng, torch.float32, "rng"), _ptr(row_scene, torch.int32, "row_scene"), pb, ldb,
                                   d_pos, _ptr(out), d_pos, _stream()), "fourier_pe")
    return out


HEAD_WIDTHS = (32, 64)                                          # channels per attention head the kernels are built for


def head_width(q, v, num_heads, name):
    """Channels per head of an attention over `num_heads` heads (q and v hold the heads side by side): 32 or 64, else ValueError."""
    D = q.shape[1] // max(int(num_heads), 1)
    if D not in HEAD_WIDTHS or q.shape[1] != num_heads * D or v.shape[1] != num_heads * D:
        raise ValueError(f"{name}: head slices must be 32 or 64 channels wide (got {q.shape[1]} / {v.shape[1]} channels for {num_heads} heads)")
    return D


def attention_launch_config(Lq, Lk, num_heads, head_dim=32):
    """(waves per workgroup, key split) the attention launcher chooses for this shape with its full split workspace."""
    import ctypes as C
    lib = _lib.load()
    nw, ks = C.c_int(0), C.c_int(0)
    _lib.check(lib.sd3d_attention_config(Lq, Lk, num_heads, head_dim, lib.sd3d_attention_ws_bytes(Lq, num_heads, head_dim),
                                         C.byref(nw), C.byref(ks)), "attention_launch_config")
    return nw.value, ks.value


def attention(q, k, v, num_heads, scale, mask_bits=None, q2=None, k2=None, out=None):
    """q/k [L, H*D] (+ optional second source concatenated per head), v [Lk, H*D] -> [Lq, H*D] (`out`: rows to write into); D = 32 or 64."""
    lib = _lib.load()
    pq, ldq = _rows(q, "q")
    pk, ldk = _rows(k, "k")
    pv, ldv = _rows(v, "v")
    pq2, ldq2, pk2, ldk2 = None, 0, None, 0
    if q2 is not None:
        pq2, ldq2 = _rows(q2, "q2")
        pk2, ldk2 = _rows(k2, "k2")
    Lq, Lk = q.shape[0], k.shape[0]
    D = head_width(q, v, num_heads, "attention")
    if mask_bits is not None and tuple(mask_bits.shape) != (Lq, (Lk + 31) // 32):
        raise ValueError(f"attention: mask bits shape {tuple(mask_bits.shape)} != ({Lq}, {(Lk + 31) // 32})")
    if out is None:
        out = torch.empty(Lq, num_heads * D, dtype=torch.float32, device=q.device)
    elif tuple(out.shape) != (Lq, num_heads * D) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("attention: `out` must be a contiguous fp32 [Lq, H * D] tensor")
    ws = _WS6.get(lib.sd3d_attention_ws_bytes(Lq, num_heads, D), q.device)
    _lib.check(lib.sd3d_attention(pq, ldq, pq2, ldq2, pk, ldk, pk2, ldk2, pv, ldv, _ptr(mask_bits, torch.int32, "mask_bits"),
                                  Lq, Lk, num_heads, D, float(scale), _ptr(out), out.shape[1], None, 1 if bf16_decoder_active() else 0,
                                  ws.data_ptr(), ws.numel(), None, 0, 0.0, _stream()), "attention")
    return out


_ATTN_JOB_DT = np.dtype([("q0", "<u8"), ("q1", "<u8"), ("k0", "<u8"), ("k1", "<u8"), ("v", "<u8"), ("bits", "<u8"), ("out", "<u8"),
                         ("ldq0", "<i4"), ("ldq1", "<i4"), ("ldk0", "<i4"), ("ldk1", "<i4"), ("ldv", "<i4"), ("ldo", "<i4"),
                         ("Lq", "<i4"), ("Lk", "<i4")], align=True)                                                        # sd3d_attn_job
assert _ATTN_JOB_DT.itemsize == 88


def _attn_job_table(jobs, num_heads, name, strided_out):
    """Validates the jobs of `attention_batch` / `attention_parts` (`name`: the caller, for the messages) and fills their sd3d_attn_job
    table -> (table, bytes of split workspace, head width).  strided_out: `out` may be a view with strided rows; otherwise it must be
    contiguous.  All jobs share one head width (32 or 64 channels)."""
    lib = _lib.load()
    tab = np.zeros(len(jobs), dtype=_ATTN_JOB_DT)
    nb = 0
    width = None
    for i, (q, k, v, bits, q2, k2, out) in enumerate(jobs):
        pq, ldq = _rows(q, "q")
        pk, ldk = _rows(k, "k")
        pv, ldv = _rows(v, "v")
        pq2 = pk2 = ldq2 = ldk2 = 0
        if q2 is not None:
            pq2, ldq2 = _rows(q2, "q2")
            pk2, ldk2 = _rows(k2, "k2")
        Lq, Lk = q.shape[0], k.shape[0]
        D = head_width(q, v, num_heads, name)
        if width not in (None, D):
            raise ValueError(f"{name}: all jobs must have the same head width")
        width = D
        if bits is not None and tuple(bits.shape) != (Lq, (Lk + 31) // 32):
            raise ValueError(f"{name}: mask bits shape mismatch")
        if strided_out:
            po, ldo = _rows(out, "out")
            if out.shape[0] != Lq or out.shape[1] != num_heads * D:
                raise ValueError(f"{name}: `out` must be fp32 [Lq, H * D] rows")
        else:
            if tuple(out.shape) != (Lq, num_heads * D) or not out.is_contiguous() or out.dtype != torch.float32:
                raise ValueError(f"{name}: `out` must be a contiguous fp32 [Lq, H * D] tensor")
            po, ldo = out.data_ptr(), out.stride(0)
        tab[i] = (pq, pq2, pk, pk2, pv, 0 if bits is None else _ptr(bits, torch.int32, "mask_bits"), po, ldq, ldq2, ldk, ldk2, ldv, ldo, Lq, Lk)
        nb += lib.sd3d_attention_ws_bytes(Lq, num_heads, D)
    return tab, nb, width


def attention_dropout_keep(key, call, H, Lq, Lk, p):
    """The keep mask of attention dropout (csrc/attention.h) as bool [H, Lq, Lk]: what `train_dec.attention(..., dropout_p=p,
    key=key, call=call)` keeps inside its kernels.  key: two int32 words on the device."""
    if not 0.0 <= float(p) < 1.0:
        raise ValueError(f"attention_dropout_keep: p must lie in [0, 1), got {p}")
    _want_shape(key, [(2,)], "attention_dropout_keep: key")
    lib = _lib.load()
    keep = torch.empty(int(H), int(Lq), int(Lk), dtype=torch.uint8, device=key.device)
    _lib.check(lib.sd3d_attention_dropout_keep(_ptr(key, torch.int32, "key"), int(call), int(H), int(Lq), int(Lk), float(p), keep.data_ptr(),
                                               _stream()), "attention_dropout_keep")
    return keep.bool()


def attention_batch(jobs, num_heads, scale):
    """jobs: list of (q, k, v, mask_bits | None, q2 | None, k2 | None, out) - the same attention for several scenes in ONE launch
    (sd3d_attention_batch): per scene the rows are the bits of `attention` on that scene alone."""
    lib = _lib.load()
    tab, nb, D = _attn_job_table(jobs, num_heads, "attention_batch", strided_out=False)
    ws = _WS6.get(nb, jobs[0][0].device)
    _lib.check(lib.sd3d_attention_batch(len(jobs), tab.ctypes.data, num_heads, D, float(scale), 1 if bf16_decoder_active() else 0,
                                        ws.data_ptr(), ws.numel(), _stream()), "attention_batch")


def attention_parts(jobs, num_heads, scale):
    """`attention_batch` WITHOUT the pass that combines the key splits (sd3d_attention_batch_parts): returns (ws, [(ksplit, part_off)])
    - scene i's rows are final in its `out` where ksplit == 1, else its partial softmax states wait at ws (a uint8 tensor) + part_off
    floats for the consumer that combines them (rowchain MERGE).  jobs as in `attention_batch`."""
    import ctypes as C
    lib = _lib.load()
    n = len(jobs)
    tab, nb, D = _attn_job_table(jobs, num_heads, "attention_parts", strided_out=True)
    if D != 32:
        raise ValueError("attention_parts: head slices must be 32 channels wide (the row-chain decoder is built for 32-channel heads)")
    ws = _WS6.get(nb, jobs[0][0].device)                 # consumed by the next launch on this stream, before the next attention refills it
    ks = (C.c_int32 * n)()
    off = (C.c_int64 * n)()
    _lib.check(lib.sd3d_attention_batch_parts(n, tab.ctypes.data, num_heads, float(scale), 1 if bf16_decoder_active() else 0,
                                              ws.data_ptr(), ws.numel(), ks, off, _stream()), "attention_parts")
    return ws, [(int(ks[i]), int(off[i])) for i in range(n)]


def mask_bits_batch(logits_list, S_list, thr, out=None):
    """mask_bits for several scenes' logit matrices in one launch -> list of bit tensors (`out`: contiguous int32 [Q_i, ceil(S_i / 32)]
    tensors to write into, e.g. slices of one buffer)."""
    import ctypes as C
    lib = _lib.load()
    n = len(logits_list)
    given, out = out, []
    P, I, L = (C.c_void_p * n), (C.c_int * n), (C.c_int64 * n)
    lp, ld, Q, S, bp, nw = P(), I(), L(), I(), P(), I()
    for i, (lg, s) in enumerate(zip(logits_list, S_list)):
        lp[i], ld[i] = _rows(lg, "logits")
        Q[i], S[i] = lg.shape[0], int(s)
        nw[i] = (int(s) + 31) // 32
        if given is not None:
            bits = given[i]
            if tuple(bits.shape) != (lg.shape[0], nw[i]) or not bits.is_contiguous() or bits.dtype != torch.int32 or not bits.is_cuda:
                raise ValueError("mask_bits_batch: `out` entries must be contiguous int32 [Q, ceil(S / 32)] device tensors")
        else:
            bits = torch.empty(lg.shape[0], nw[i], dtype=torch.int32, device=lg.device)
        bp[i] = bits.data_ptr()
        out.append(bits)
    _lib.check(lib.sd3d_mask_bits_batch(n, lp, ld, Q, S, bp, nw, float(thr), _stream()), "mask_bits_batch")
    return out


def dinox_mask_bits_batch(blocked_list, near_list):
    """dinox_mask_bits for several scenes in one launch -> list of bit tensors."""
    import ctypes as C
    lib = _lib.load()
    n = len(blocked_list)
    P, I, L = (C.c_void_p * n), (C.c_int * n), (C.c_int64 * n)
    bl, nr, nw, Q, Mq, op, nwo = P(), P(), I(), L(), L(), P(), I()
    out = []
    for i, (b, nearb) in enumerate(zip(blocked_list, near_list)):
        bl[i], nr[i] = _ptr(b, torch.int32, "blocked"), _ptr(nearb, torch.int32, "near")
        Q[i], nw[i] = b.shape
        Mq[i] = nearb.shape[0]
        nwo[i] = (nearb.shape[0] + 1 + 31) // 32
        o = torch.empty(b.shape[0], nwo[i], dtype=torch.int32, device=b.device)
        op[i] = o.data_ptr()
        out.append(o)
    _lib.check(lib.sd3d_dinox_mask_bits_batch(n, bl, nr, nw, Q, Mq, op, nwo, _stream()), "dinox_mask_bits_batch")
    return out


def mask_bits(logits, S, thr):
    """One scene: a batch of one."""
    return mask_bits_batch([logits], [S], thr)[0]


def near_bits(sp_pos, centers, thr):
    lib = _lib.load()
    S, M = sp_pos.shape[0], centers.shape[0]
    nw = (S + 31) // 32
    near = torch.empty(M, nw, dtype=torch.int32, device=sp_pos.device)
    _lib.check(lib.sd3d_near_bits(_ptr(sp_pos, torch.float32, "sp_pos"), S, _ptr(centers, torch.float32, "centers"), M,
                                  float(thr), _ptr(near), nw, _stream()), "near_bits")
    return near


def dinox_mask_bits(blocked, near):
    """One scene: a batch of one."""
    return dinox_mask_bits_batch([blocked], [near])[0]


def box_refine(ref_points, d_center, size_prev, d_size, rng, normalize, row_scene=None):
    """ref_points, d_center, d_size [Q, 3]; size_prev [3] (one row for all queries) or [Q, 3]; rng [6].
    row_scene int32 [Q]: rows of several scenes, rng [n_scenes, 6]."""
    Q = _want_box_shapes(ref_points, d_center, size_prev, d_size, rng, row_scene)
    lib = _lib.load()
    dev = ref_points.device
    center = torch.empty(Q, 3, dtype=torch.float32, device=dev)
    size = size_metric = None
    ps, lds = None, 0
    if d_size is not None:
        size = torch.empty(Q, 3, dtype=torch.float32, device=dev)
        size_metric = torch.empty(Q, 3, dtype=torch.float32, device=dev)
        ps = _ptr(size_prev, torch.float32, "size_prev")
        lds = 0 if size_prev.dim() == 1 else 3
    _lib.check(lib.sd3d_box_refine(_ptr(ref_points, torch.float32, "ref_points"), _ptr(d_center, torch.float32, "d_center"),
                                   ps, lds, _ptr(d_size, torch.float32, "d_size"), _ptr(rng, torch.float32, "rng"),
                                   _ptr(row_scene, torch.int32, "row_scene"), int(normalize), Q, _ptr(center), _ptr(size),
                                   _ptr(size_metric), _stream()), "box_refine")
    return center, size, size_metric


# --------------------------------------------------------------------------------------------
# post-processing ops
# --------------------------------------------------------------------------------------------
def class_scores(cls, C, want_scores=True, want_rowmax=False):
    lib = _lib.load()
    pc, ld = _rows(cls, "cls")
    Q = cls.shape[0]
    scores = torch.empty(Q * C, dtype=torch.float32, device=cls.device) if want_scores else None
    rowmax = torch.empty(Q, dtype=torch.float32, device=cls.device) if want_rowmax else None
    _lib.check(lib.sd3d_class_scores(pc, ld, Q, C, _ptr(scores), _ptr(rowmax), _stream()), "class_scores")
    return scores, rowmax


def mask_scores(masks, S, flat_idx, score_in, C, normalize):
    lib = _lib.load()
    pm, ld = _rows(masks, "masks")
    n = flat_idx.numel()
    dev = masks.device
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    qidx = torch.empty(n, dtype=torch.int32, device=dev)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.check(lib.sd3d_mask_scores(pm, ld, S, _ptr(flat_idx, torch.int32, "flat_idx"), _ptr(score_in, torch.float32, "score_in"),
                                    n, C, int(bool(normalize)), _ptr(labels), _ptr(qidx), _ptr(out), _stream()), "mask_scores")
    return labels, qidx, out


TOPK_SELECT_MAX_N = 40 * 1024    # what the one workgroup of the select holds in registers; above it: the radix sort


def topk_desc(x: torch.Tensor, k: int):
    """int32 [k]: the first k indices of the stable descending sort of the fp32 vector x (`sd3d_topk_desc_f32`: one launch)."""
    lib = _lib.load()
    out = torch.empty(k, dtype=torch.int32, device=x.device)
    _lib.check(lib.sd3d_topk_desc_f32(_ptr(x, torch.float32, "x"), x.numel(), int(k), _ptr(out), _stream()), "topk_desc")
    return out


def take_f32(src, idx):
    """src[idx] for an int32 index vector, one launch (ATen: `.long()` + index)."""
    lib = _lib.load()
    n = idx.numel()
    out = torch.empty(n, dtype=torch.float32, device=src.device)
    _lib.check(lib.sd3d_take_f32(_ptr(src, torch.float32, "src"), _ptr(idx, torch.int32, "idx"), n, _ptr(out), _stream()), "take_f32")
    return out


def select_instances(scores, count, thr0, thr1, npoint_thr):
    """Row selections for the two score thresholds on the device (`sd3d_select_instances`).  Returns (buffers, counts): `buffers` =
    (keep, pkeep, union, keep_u, pkeep_u int32 [k]; score_mask, npoint_mask uint8 [k]), `counts` int32 [4] for one small host read."""
    lib = _lib.load()
    k = scores.numel()
    dev = scores.device
    ints = torch.empty(5, max(k, 1), dtype=torch.int32, device=dev)
    bytes_ = torch.empty(2, max(k, 1), dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    ip, bp = ints.data_ptr(), bytes_.data_ptr()
    st = 4 * max(k, 1)
    _lib.check(lib.sd3d_select_instances(_ptr(scores, torch.float32, "scores"), _ptr(count, torch.int32, "count"), k, float(thr0), float(thr1),
                                         int(npoint_thr), ip, ip + st, ip + 2 * st, ip + 3 * st, ip + 4 * st, bp, bp + max(k, 1),
                                         _ptr(counts), _stream()), "select_instances")
    return (ints, bytes_), counts


def take_instances(keep, labels, scores, boxes=None):
    """(labels[keep] as int64, scores[keep], boxes[keep] | None) in one launch."""
    lib = _lib.load()
    m = keep.numel()
    dev = keep.device
    lo = torch.empty(m, dtype=torch.int64, device=dev)
    so = torch.empty(m, dtype=torch.float32, device=dev)
    bo = torch.empty(m, 6, dtype=torch.float32, device=dev) if boxes is not None else None
    _lib.check(lib.sd3d_take_instances(_ptr(keep, torch.int32, "keep"), m, _ptr(labels, torch.int32, "labels"), _ptr(scores, torch.float32, "scores"),
                                       _ptr(boxes, torch.float32, "boxes"), _ptr(lo), _ptr(so), _ptr(bo), _stream()), "take_instances")
    return lo, so, bo


def take_pair(order, labels, scores):
    """(labels[order], scores[order]) in one launch."""
    lib = _lib.load()
    n = order.numel()
    lo = torch.empty(n, dtype=torch.int32, device=order.device)
    so = torch.empty(n, dtype=torch.float32, device=order.device)
    _lib.check(lib.sd3d_take_pair(_ptr(order, torch.int32, "order"), _ptr(labels, torch.int32, "labels"), _ptr(scores, torch.float32, "scores"), n,
                                  _ptr(lo), _ptr(so), _stream()), "take_pair")
    return lo, so


def nms_finish(order2, scores2, labels1, order1, qidx, centers=None, sizes=None):
    """-> (final_scores, final_labels int32, record int64, boxes [n, 6] | None): the selections behind matrix-NMS's final sort in one launch."""
    lib = _lib.load()
    n = order2.numel()
    dev = order2.device
    fs = torch.empty(n, dtype=torch.float32, device=dev)
    fl = torch.empty(n, dtype=torch.int32, device=dev)
    rec = torch.empty(n, dtype=torch.int64, device=dev)
    boxes = torch.empty(n, 6, dtype=torch.float32, device=dev) if centers is not None and sizes is not None else None
    _lib.check(lib.sd3d_nms_finish(_ptr(order2, torch.int32, "order2"), _ptr(scores2, torch.float32, "scores2"), _ptr(labels1, torch.int32, "labels1"),
                                   _ptr(order1, torch.int32, "order1"), _ptr(qidx, torch.int32, "qidx"),
                                   _ptr(centers, torch.float32, "centers") if boxes is not None else None,
                                   _ptr(sizes, torch.float32, "sizes") if boxes is not None else None, n, _ptr(fs), _ptr(fl), _ptr(rec), _ptr(boxes),
                                   _stream()), "nms_finish")
    return fs, fl, rec, boxes


def gather_sigmoid(masks, S, qidx, order, ld_out):
    lib = _lib.load()
    pm, ld = _rows(masks, "masks")
    n = order.numel()
    sig = torch.empty(n, ld_out, dtype=torch.float32, device=masks.device)
    area = torch.empty(n, dtype=torch.float32, device=masks.device)
    _lib.check(lib.sd3d_gather_sigmoid(pm, ld, S, _ptr(qidx, torch.int32, "qidx"), _ptr(order, torch.int32, "order"), n,
                                       _ptr(sig), ld_out, _ptr(area), _stream()), "gather_sigmoid")
    return sig, area


def nms_decay(inter, area, labels, score_in, kernel="linear", sigma=2.0):
    lib = _lib.load()
    pi, ld = _rows(inter, "inter")
    n = area.numel()
    comp = torch.empty(n, dtype=torch.float32, device=inter.device)
    out = torch.empty(n, dtype=torch.float32, device=inter.device)
    if kernel not in ("linear", "gaussian"):
        raise NotImplementedError(f"{kernel} kernel is not supported in matrix nms!")
    _lib.check(lib.sd3d_nms_decay(pi, ld, _ptr(area, torch.float32, "area"), _ptr(labels, torch.int32, "labels"), n,
                                  int(kernel == "gaussian"), float(sigma), _ptr(score_in, torch.float32, "score_in"),
                                  _ptr(comp), _ptr(out), _stream()), "nms_decay")
    return out


class MaskBits:
    """Step 1 of the point-mask expansion (`sd3d_mask_rowbits`): the thresholded rows as a bit table over the superpoints + the point
    count of every row.  `rows(list)` expands a list of rows to [m, N] bytes (`sd3d_expand_rows`): only the instances that survive."""

    def __init__(self, sig, src_row, superpoints, points, sp_thr, boxes=None, loose_ratio=1.5):
        lib = _lib.load()
        ps, lds = _rows(sig, "sig")
        self.n, self.N, self.lds = src_row.numel(), superpoints.numel(), lds
        self.superpoints, self.points, self.boxes, self.loose = superpoints, points, boxes, float(loose_ratio)
        # (a tensor of its own, not the per-stream workspace: the table must survive until the rows are expanded, after the host read)
        self.ws = torch.empty(lib.sd3d_expand_masks_ws_bytes(self.n, lds), dtype=torch.uint8, device=sig.device)
        # the point counts sit right behind the table's superpoint sizes: the library zeroes both with one memset launch
        c0 = 4 * lds * ((self.n + 31) // 32 + 1)
        self.count = self.ws[c0:c0 + 4 * self.n].view(torch.int32)
        _lib.check(lib.sd3d_mask_rowbits(ps, lds, _ptr(src_row, torch.int32, "src_row"), self.n, _ptr(superpoints, torch.int64, "superpoints"),
                                         self.N, float(sp_thr), _ptr(self.count), self.ws.data_ptr(), self.ws.numel(), _stream()), "mask_rowbits")

    def rows(self, rows):
        lib = _lib.load()
        m = rows.numel()
        out = torch.empty(m, self.N, dtype=torch.uint8, device=self.ws.device)
        if m:
            pp, ldp = _rows(self.points, "points")
            _lib.check(lib.sd3d_expand_rows(self.ws.data_ptr(), self.n, self.lds, _ptr(rows, torch.int32, "rows"), m,
                                            _ptr(self.superpoints, torch.int64, "superpoints"), pp, ldp, self.N,
                                            _ptr(self.boxes, torch.float32, "boxes"), self.loose, _ptr(out), _stream()), "expand_rows")
        return out


def pack_mask_rows(masks_u8, rows=None):
    """masks_u8 [n, N] uint8 (0 / 1) -> bit-packed uint8 [len(rows) | n, ceil(N / 8)] of the selected rows (int32 `rows`, or all):
    bit j of byte b = masks[row][8 b + j] (numpy bitorder "little").  The device half of the host-output path."""
    lib = _lib.load()
    n, N = masks_u8.shape
    n_rows = n if rows is None else rows.numel()
    nb = (N + 7) // 8
    out = torch.empty(n_rows, nb, dtype=torch.uint8, device=masks_u8.device)
    _lib.check(lib.sd3d_pack_mask_rows(_ptr(masks_u8, torch.uint8, "masks"), N, _ptr(rows, torch.int32, "rows"), n_rows, _ptr(out), nb,
                                       _stream()), "pack_mask_rows")
    return out


class _HostPool:
    """Recycles the big host arrays of the unpacked instance masks: a fresh 90 MB numpy array per scene is 22 k page faults (20 - 40 ms
    on the evaluation hosts, more than the forward itself); an array handed out here returns its memory to the pool when the LAST
    reference to it (or to a view of it) dies.  A caller that keeps every scene's masks (the reference's evaluator until
    `evaluate()`) simply never gives anything back - then this is `np.empty`."""

    class _Lease:
        __slots__ = ("buf", "pool", "__array_interface__")

        def __init__(self, buf, pool, shape):
            self.buf, self.pool = buf, pool
            self.__array_interface__ = {"shape": shape, "typestr": "|b1", "data": (buf.ctypes.data, False), "version": 3}

        def __del__(self):
            try:
                self.pool._give_back(self.buf)
            except Exception:  # noqa: BLE001 - interpreter shutdown
                pass

    def __init__(self, max_free_bytes=None):
        # SD3D_HOST_POOL_BYTES: most freed host bytes the pool keeps for the life of the process (default 512 MiB = five 90 MB mask
        # arrays, one per scene in flight plus one; 0 switches the recycling off)
        if max_free_bytes is None:
            max_free_bytes = int(_os.environ.get("SD3D_HOST_POOL_BYTES", str(512 << 20)))
        self.free, self.lock, self.max_free = [], threading.Lock(), max_free_bytes

    def _give_back(self, buf):
        with self.lock:
            if sum(b.nbytes for b in self.free) + buf.nbytes <= self.max_free:
                self.free.append(buf)

    def bool_array(self, shape):
        need = int(np.prod(shape))
        if need < (1 << 20):                                     # small arrays: the allocator's own free lists do this already
            return np.empty(shape, dtype=np.bool_)
        buf = None
        with self.lock:
            fit = [i for i, b in enumerate(self.free) if need <= b.nbytes <= need + need // 4 + (4 << 20)]
            if fit:
                buf = self.free.pop(min(fit, key=lambda i: self.free[i].nbytes))
        if buf is None:
            buf = np.empty((need + (4 << 20) - 1) // (4 << 20) * (4 << 20), dtype=np.uint8)
        return np.asarray(self._Lease(buf, self, tuple(int(v) for v in shape)))


_HOST_POOL = _HostPool()


def unpack_bits_host(packed, n_points: int):
    """HOST arrays: packed uint8 [n, ceil(N / 8)] (numpy) -> bool [n, N] (pageable; large ones come from a recycling pool, `_HostPool`).
    Runs in the C library with the GIL released (sd3d_unpack_bits_host): the other scene threads keep issuing while this one expands
    its masks."""
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    n, nb = packed.shape
    if nb != (n_points + 7) // 8:
        raise ValueError(f"unpack_bits_host: {nb} bytes per row cannot hold {n_points} points")
    out = _HOST_POOL.bool_array((n, n_points))
    _lib.check(_lib.load_nogil().sd3d_unpack_bits_host(packed.ctypes.data, n, n_points, nb, out.ctypes.data), "unpack_bits_host")
    return out


class PinnedStaging:
    """One grow-only pinned host buffer per (host thread): the staging area of a forward's device -> host copies.  The outputs
    handed to the caller are pageable copies made from it, so nothing page-locked outlives the forward (a long evaluation keeps
    every scene's outputs until `evaluate()`: ~100 MB of pinned memory per scene otherwise)."""

    def __init__(self):
        self._tls = threading.local()

    def get(self, nbytes: int):
        buf = getattr(self._tls, "buf", None)
        if buf is None or buf.numel() < nbytes:
            buf = self._tls.buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, pin_memory=True)
        return buf


_STAGING = PinnedStaging()


def to_host_arrays(tensors):
    """Device tensors -> pageable numpy arrays through ONE pinned staging buffer: asynchronous copies, one polled wait (the issue
    baton goes to another scene's thread meanwhile), then host copies out of the staging area."""
    offs, total = [], 0
    for t in tensors:
        total = (total + 63) // 64 * 64
        offs.append(total)
        total += t.numel() * t.element_size()
    stage = _STAGING.get(total)
    views = []
    for t, o in zip(tensors, offs):
        nb = t.numel() * t.element_size()
        v = stage[o:o + nb].view(t.dtype).view(t.shape) if nb else torch.empty(t.shape, dtype=t.dtype)
        if nb:
            v.copy_(t.contiguous(), non_blocking=True)
        views.append(v)
    wait_event(stream_event())
    return [np.array(v.numpy(), copy=True) for v in views]


def row_argmax(x, ncols=None, cols=None):
    lib = _lib.load()
    px, ld = _rows(x, "x")
    Q = x.shape[0]
    out = torch.empty(Q, dtype=torch.int64, device=x.device)
    nc = cols.numel() if cols is not None else (ncols if ncols is not None else x.shape[1])
    _lib.check(lib.sd3d_row_argmax(px, ld, Q, _ptr(cols, torch.int32, "cols"), nc, _ptr(out), _stream()), "row_argmax")
    return out


def gather_i64(table, idx, use_index=True):
    lib = _lib.load()
    N = idx.numel()
    out = torch.empty(N, dtype=torch.int64, device=idx.device)
    _lib.check(lib.sd3d_gather_i64(_ptr(table, torch.int64, "table"), _ptr(idx, torch.int64, "idx"), N, int(use_index),
                                   _ptr(out), _stream()), "gather_i64")
    return out


def panoptic(masks_u8, rows_desc, labels_desc, n_stuff, npoint_thr, sem_stuff):
    lib = _lib.load()
    N = masks_u8.shape[1]
    n = rows_desc.numel()
    dev = masks_u8.device
    inst_ws = torch.empty(N, dtype=torch.int32, device=dev)
    hist = torch.empty(n + n_stuff + 1, dtype=torch.int32, device=dev)
    sem_map = torch.empty(N, dtype=torch.int64, device=dev)
    inst_map = torch.empty(N, dtype=torch.int64, device=dev)
    _lib.check(lib.sd3d_panoptic(_ptr(masks_u8, torch.uint8, "masks"), N, _ptr(rows_desc, torch.int32, "rows"),
                                 _ptr(labels_desc, torch.int32, "labels"), n, n_stuff, int(npoint_thr),
                                 _ptr(sem_stuff, torch.int64, "sem_stuff"), _ptr(inst_ws), _ptr(hist), _ptr(sem_map),
                                 _ptr(inst_map), _stream()), "panoptic")
    return sem_map, inst_map


def instance_boxes(points, masks_bool, mode):
    """masks_bool [n_inst, N] torch.bool -> (centers [n,3], sizes [n,3])."""
    lib = _lib.load()
    pp, ld = _rows(points, "points")
    n, N = masks_bool.shape
    m = masks_bool.contiguous().view(torch.uint8)
    centers = torch.zeros(n, 3, dtype=torch.float32, device=points.device)
    sizes = torch.zeros(n, 3, dtype=torch.float32, device=points.device)
    ws = _WS.get(lib.sd3d_instance_boxes_ws_bytes(n), points.device)
    _lib.check(lib.sd3d_instance_boxes(pp, ld, N, _ptr(m, torch.uint8, "masks"), N, n, 0 if mode == "mean" else 1,
                                       _ptr(centers), _ptr(sizes), ws.data_ptr(), ws.numel(), _stream()), "instance_boxes")
    return centers, sizes


def scale_shift_act(x, scale, shift, act=None, x2=None, add=None):
    """act(cat[x, x2] * scale + shift) (+ add, AFTER the activation) -> new contiguous [M, C] tensor."""
    lib = _lib.load()
    p0, ld0 = _rows(x, "x")
    C0 = x.shape[1]
    p1, ld1, C = None, 0, C0
    if x2 is not None:
        p1, ld1 = _rows(x2, "x2")
        C = C0 + x2.shape[1]
    pa, lda = (None, 0) if add is None else _rows(add, "add")
    if add is not None and tuple(add.shape) != (x.shape[0], C):
        raise ValueError(f"scale_shift_act: add must be [{x.shape[0]}, {C}], got {tuple(add.shape)}")
    out = torch.empty(x.shape[0], C, dtype=torch.float32, device=x.device)
    _lib.check(lib.sd3d_scale_shift_act_add(p0, ld0, C0, p1, ld1, _ptr(scale, torch.float32, "scale"),
                                            _ptr(shift, torch.float32, "shift"), ACT[act], x.shape[0], C, pa, lda, _ptr(out), C,
                                            _stream()), "scale_shift_act")
    return out


def hungarian_match(costs, check=False, return_status=False):
    """Minimum-cost one-to-one assignment (scipy.optimize.linear_sum_assignment, the reference's HungarianMatcher) of every
    [Q_i, G_i] fp32 cost matrix of `costs` in ONE C call (csrc/assign.hip: one workgroup per problem) -> list of [Q_i, G_i] byte
    matrices with min(Q_i, G_i) ones, at most one per row and per column.  Where the optimum is not unique the pairs may differ
    from scipy's; the total cost does not.  `check=True` reads the status words back (a synchronisation) and raises ValueError
    where scipy would (NaN / -inf entries, no finite assignment); `check=False` never reads the device.
    `return_status=True` -> (matches, int32 device tensor of the status words)."""
    import ctypes as C
    lib = _lib.load()
    costs = list(costs)
    n = len(costs)
    if n == 0:
        return ([], None) if return_status else []
    P, I = (C.c_void_p * n), (C.c_int * n)
    cp, mp, Q, G = P(), P(), I(), I()
    out = []
    dev = costs[0].device
    for i, c in enumerate(costs):
        if c.dim() != 2:
            raise ValueError(f"hungarian_match: costs[{i}] must be a [Q, G] matrix, got {tuple(c.shape)}")
        cp[i] = _ptr(c, torch.float32, f"hungarian_match: costs[{i}]")
        if c.device != dev:
            raise ValueError("hungarian_match: all cost matrices must live on one device")
        Q[i], G[i] = c.shape
        m = torch.empty(c.shape, dtype=torch.uint8, device=dev)
        mp[i] = m.data_ptr()
        out.append(m)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    ws_bytes = lib.sd3d_hungarian_match_ws_bytes(n, Q, G)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.sd3d_hungarian_match_batch(n, cp, Q, G, mp, status.data_ptr(), ws.data_ptr(), ws_bytes, _stream()), "hungarian_match")
    if check:
        bad = torch.nonzero(status).reshape(-1).tolist()
        if bad:
            raise ValueError(f"hungarian_match: cost matrix {bad[0]} contains invalid numeric entries or has no finite assignment")
    return (out, status) if return_status else out


# --------------------------------------------------------------------------------------------
# dataset targets (csrc/targets.hip)
# --------------------------------------------------------------------------------------------
def _stuff_array(stuff_ids):
    return (ctypes.c_int32 * max(1, len(stuff_ids)))(*stuff_ids)


def targets_scan(instance_mask, semantic_mask, super_points, lut, n_classes: int, stuff_ids, swap_2_3: bool):
    """Pass 1 of `sd3d_targets_scan` on int64 [N] label arrays: returns (workspace, HostRead of the 4-word header
    {status, G', S, present stuff bits}).  The workspace belongs to this scene until `targets_build` has run on it."""
    lib = _lib.load()
    n = instance_mask.numel()
    if semantic_mask.numel() != n or super_points.numel() != n:
        raise ValueError("targets_scan: instance_mask, semantic_mask and super_points must have one entry per point")
    dev = instance_mask.device
    ws = torch.empty(lib.sd3d_targets_ws_bytes(n), dtype=torch.uint8, device=dev)
    _lib.check(lib.sd3d_targets_scan(_ptr(instance_mask, torch.int64, "instance_mask"), _ptr(semantic_mask, torch.int64, "semantic_mask"),
                                     _ptr(super_points, torch.int64, "super_points"), n, _ptr(lut, torch.int64, "seg_label_mapping"), lut.numel(),
                                     int(n_classes), _stuff_array(stuff_ids), len(stuff_ids), int(bool(swap_2_3)), ws.data_ptr(), ws.numel(),
                                     _stream()), "targets_scan")
    return ws, HostRead(ws[:16].view(torch.int32))


def targets_build(ws, header, n: int, n_classes: int, stuff_ids, val_view: bool):
    """Pass 2 (`sd3d_targets_build`) from the header as read back (int32 [4] on the host): allocates and fills masks [G, N] uint8,
    labels / area [G] int64, sp_inst / sp_sem [S] int32 and sp_masks [G' + C + 1, S] uint8.  Raises on a range status."""
    lib = _lib.load()
    dev = ws.device
    hdr = (ctypes.c_int32 * 4)(*[int(v) for v in header.tolist()])
    stuff = _stuff_array(stuff_ids)
    if hdr[0] != 0:                                          # a range status: the C call names it (outputs are not touched)
        _lib.check(lib.sd3d_targets_build(n, hdr, int(n_classes), stuff, len(stuff_ids), int(bool(val_view)), None, None, None, None, None, None,
                                          None, ws.data_ptr(), ws.numel(), _stream()), "targets_build")
    G1, S = int(hdr[1]), int(hdr[2])
    G = lib.sd3d_targets_rows(hdr, len(stuff_ids), int(bool(val_view)))
    if G < 0:
        _lib.check(G, "targets_rows")
    masks = torch.empty((G, n), dtype=torch.uint8, device=dev)
    labels = torch.empty(G, dtype=torch.int64, device=dev)
    area = torch.empty_like(labels)
    seg_start = torch.empty(S + 1, dtype=torch.int32, device=dev)
    sp_inst = torch.empty(S, dtype=torch.int32, device=dev)
    sp_sem = torch.empty(S, dtype=torch.int32, device=dev)
    sp_masks = torch.empty((G1 + n_classes + 1, S), dtype=torch.uint8, device=dev)
    _lib.check(lib.sd3d_targets_build(n, hdr, int(n_classes), stuff, len(stuff_ids), int(bool(val_view)), _ptr(masks), _ptr(labels), _ptr(area),
                                      _ptr(seg_start), _ptr(sp_inst), _ptr(sp_sem), _ptr(sp_masks), ws.data_ptr(), ws.numel(), _stream()),
               "targets_build")
    return dict(masks=masks, labels=labels, area=area, sp_inst=sp_inst, sp_sem=sp_sem, sp_masks=sp_masks, n_instances=G1, n_superpoints=S)


# --------------------------------------------------------------------------------------------
# benchmark submission text (csrc/submit.hip)
# --------------------------------------------------------------------------------------------
def mask_text(masks, rows=None):
    """masks [n, N] uint8 / bool -> uint8 [len(rows) | n, pitch], pitch = 2 N rounded up to 16: the first 2 N bytes of row r are what
    `np.savetxt(f, masks[rows[r]], fmt='%d')` writes ("0\\n" / "1\\n" per point); the bytes behind them are not initialised."""
    if not masks.is_cuda:
        raise RuntimeError(f"masks: expected a tensor on the HIP device, got {masks.device} (no CPU fallback)")
    lib = _lib.load()
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    n, N = masks.shape
    n_rows = n if rows is None else rows.numel()
    pitch = (2 * N + 15) // 16 * 16
    out = torch.empty(n_rows, pitch, dtype=torch.uint8, device=masks.device)
    if n_rows == 0 or N == 0:
        return out
    _lib.check(lib.sd3d_mask_text(_ptr(masks, torch.uint8, "masks"), N, _ptr(rows, torch.int32, "rows"), n_rows, _ptr(out), pitch, _stream()),
               "mask_text")
    return out


LABEL_TEXT_STATUS = ((1, "an index lies outside the label table"), (2, "a value lies outside int32"),
                     (4, "the text does not fit the output buffer"))


class LabelTable:
    """An id table of `label_text` on the device: int32 entries and the bytes of its widest line."""

    def __init__(self, mapping, device):
        m = np.asarray(mapping).astype(np.int64).ravel()
        if m.size and (m.min() < -2 ** 31 or m.max() > 2 ** 31 - 1):
            raise ValueError("label table: entries must fit int32")
        self.width = max((len(str(int(v))) for v in (m.min(), m.max())), default=1) + 1 if m.size else 1
        self.dev = torch.from_numpy(m.astype(np.int32)).to(device)


def label_text(values, lut=None, out=None):
    """values int64 [N] -> (text uint8 [cap], info int32 [2]), both on the device: `np.savetxt(f, lut[values], fmt='%d')` as one byte
    string of info[0] bytes; info[1] is a status the reader of `info` checks with `label_text_check` (nothing is read back here).
    lut: None (the values themselves, which must fit int32), a `LabelTable`, or an id array (uploaded).  cap = N x the widest line
    (12 bytes without a table); `out`: a caller's uint8 buffer to use instead - a text that does not fit it sets the status."""
    if not values.is_cuda:
        raise RuntimeError(f"values: expected a tensor on the HIP device, got {values.device} (no CPU fallback)")
    lib = _lib.load()
    dev = values.device
    N = values.numel()
    if lut is not None and not isinstance(lut, LabelTable):
        lut = LabelTable(lut, dev)
    cap = N * (12 if lut is None else lut.width)
    if cap > 2 ** 31 - 1:
        raise ValueError(f"label_text: {cap} bytes of text exceed 2^31 - 1; split the values")
    if out is None:
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    ws = _WS.get(lib.sd3d_label_text_ws_bytes(N), dev)
    _lib.check(lib.sd3d_label_text(_ptr(values, torch.int64, "values"), N, _ptr(lut.dev, torch.int32, "lut") if lut is not None else None,
                                   lut.dev.numel() if lut is not None else 0, _ptr(out, torch.uint8, "out"), out.numel(), _ptr(info),
                                   ws.data_ptr(), ws.numel(), _stream()), "label_text")
    return out, info


def label_text_check(info_host, what="label_text"):
    """Raises when the status word of a `label_text` info pair (read back by the caller) is set; returns the length of the text."""
    status = int(info_host[1])
    if status:
        raise RuntimeError(f"{what}: status {status}: " + "; ".join(msg for bit, msg in LABEL_TEXT_STATUS if status & bit))
    return int(info_host[0])


# --------------------------------------------------------------------------------------------
# semantic and panoptic evaluation (csrc/segeval.hip)
# --------------------------------------------------------------------------------------------
SEG_EVAL_STATUS = ((1, "a semantic prediction lies outside [0, n_classes) on a counted point"),
                   (2, "a shifted instance id lies outside [0, 2^16)"),
                   (4, "a scene has more than 65536 segments on one side"))
_WS_SEG = _PerThread()   # panoptic_accumulate: presence bits, segment tables and per-point keys of one scene


def _labels1d(t: torch.Tensor, name: str):
    """int64 [N] label array, read in place whatever its element stride -> (ptr, stride)."""
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a tensor on the HIP device, got {t.device} (no CPU fallback)")
    if t.dtype != torch.int64 or t.dim() != 1:
        raise TypeError(f"{name}: expected a 1-D int64 tensor, got {t.dtype} with {t.dim()} dimensions")
    return t.data_ptr(), (t.stride(0) if t.numel() > 1 else 1)


def _accumulator(t: torch.Tensor, dtype, numel: int, name: str):
    p = _ptr(t, dtype, name)
    if t.numel() != numel:
        raise ValueError(f"{name}: expected {numel} elements, got {t.numel()}")
    return p


def semantic_confusion(pred_sem, gt_sem, n_classes: int, ignore_index: int, confusion, status):
    """confusion[gt, pred] += 1 per counted point (`sd3d_semantic_confusion`): int64 [N] labels with any element stride,
    `confusion` int64 [C, C] and `status` int64 [1] are device accumulators that persist across calls.  Enqueues only."""
    lib = _lib.load()
    pp, sp = _labels1d(pred_sem, "pred_sem")
    pg, sg = _labels1d(gt_sem, "gt_sem")
    n = gt_sem.numel()
    if pred_sem.numel() != n:
        raise ValueError("semantic_confusion: pred_sem and gt_sem must have one entry per point")
    C = int(n_classes)
    _lib.check(lib.sd3d_semantic_confusion(pp, sp, pg, sg, n, C, int(ignore_index), _accumulator(confusion, torch.int64, C * C, "confusion"),
                                           _accumulator(status, torch.int64, 1, "status"), _stream()), "semantic_confusion")


def panoptic_accumulate(pred_sem, pred_inst, gt_sem, gt_inst, n_classes: int, ignore_ids, min_num_points: int, tp, fp, fn, iou_sum, status):
    """One scene of the panoptic protocol (`sd3d_panoptic_accumulate`) added into tp / fp / fn int64 [C], iou_sum float64 [C] and
    status int64 [1] on the device.  Labels: int64 [N] with any element stride.  Enqueues only; scratch comes from a per-stream buffer."""
    lib = _lib.load()
    arrs = [_labels1d(t, nm) for t, nm in ((pred_sem, "pred_sem"), (pred_inst, "pred_inst"), (gt_sem, "gt_sem"), (gt_inst, "gt_inst"))]
    n = gt_sem.numel()
    if any(t.numel() != n for t in (pred_sem, pred_inst, gt_inst)):
        raise ValueError("panoptic_accumulate: the four label arrays must have one entry per point")
    C = int(n_classes)
    ignore_ids = [int(v) for v in ignore_ids]
    if len(ignore_ids) > 8 or any(abs(v) >= 2 ** 31 for v in ignore_ids):
        raise ValueError("panoptic_accumulate: at most 8 ignored classes, each an int32")
    nb = lib.sd3d_seg_eval_ws_bytes(n, C)
    if nb == 0:
        raise ValueError(f"panoptic_accumulate: unsupported size (n = {n}, n_classes = {C})")
    ws = _WS_SEG.get(nb, gt_sem.device)
    ign = (ctypes.c_int32 * max(1, len(ignore_ids)))(*ignore_ids)
    args = [v for pair in arrs for v in pair]
    _lib.check(lib.sd3d_panoptic_accumulate(*args, n, C, ign, len(ignore_ids), int(min_num_points), _accumulator(tp, torch.int64, C, "tp"),
                                            _accumulator(fp, torch.int64, C, "fp"), _accumulator(fn, torch.int64, C, "fn"),
                                            _accumulator(iou_sum, torch.float64, C, "iou_sum"), _accumulator(status, torch.int64, 1, "status"),
                                            ws.data_ptr(), ws.numel(), _stream()), "panoptic_accumulate")


# --------------------------------------------------------------------------------------------
# streamed ScanNet instance AP (csrc/apeval.hip)
# --------------------------------------------------------------------------------------------
AP_STATUS = ((1, "a ground-truth instance index lies outside [-1, 1000)"),
             (2, "a ground-truth instance spans two semantic classes"),
             (4, "a prediction label lies outside [0, n_classes)"),
             (8, "a prediction score is not finite"),
             (16, "the entry store is too small for the scenes it was given"))
AP_MAX_PREDS = 4096
_WS_AP = _PerThread()    # ap_scene: columns, count matrix and per-class lists of one scene
_WS_AP_FIN = _PerThread()   # ap_finish: sort buffers and the curve points


def ap_slots_per_prediction(overlaps) -> list:
    """Entries one prediction can emit at each overlap: IoU > th needs inter > th * |pred| and ground truths are disjoint, so at
    most ceil(1 / th) - 1 of them can pass (3 at 0.25, 1 from 0.5 up); a prediction that passes none emits at most one false positive."""
    return [max(1, int(np.ceil(1.0 / float(th))) - 1) for th in overlaps]


def ap_scene(gt_sem, gt_inst, masks, labels, scores, class_lut, zero_class: int, n_classes: int, overlaps, slots, min_region: int, store,
             slot_begin: int, slot_cap: int, hard_fn, has_gt, has_pred, status, id_map=None, num_stuff: int = 0):
    """One scene of the streamed AP protocol (`sd3d_ap_scene`): association, greedy matching per (class, overlap) and the scene's
    entries written into its slots `store[slot_begin : slot_begin + n * sum(slots)]` (those below `slot_begin + slot_cap`).
    gt_sem / gt_inst int64 [N] (any element stride), masks uint8 [n, N] with contiguous rows (any pitch), labels int64 [n],
    scores fp32 [n], class_lut int32 [lut_len], overlaps float64 [O] on the device, slots the host list of
    `ap_slots_per_prediction`; hard_fn int64 [C * O], has_gt / has_pred int64 [C] and status int64 [1] persist across calls.
    Enqueues only; scratch comes from a per-stream buffer."""
    lib = _lib.load()
    ps, ss = _labels1d(gt_sem, "gt_sem")
    pi, si = _labels1d(gt_inst, "gt_inst")
    N = gt_sem.numel()
    if gt_inst.numel() != N:
        raise ValueError("ap_scene: gt_sem and gt_inst must have one entry per point")
    if not masks.is_cuda:
        raise RuntimeError(f"masks: expected a tensor on the HIP device, got {masks.device} (no CPU fallback)")
    if masks.dtype != torch.uint8 or masks.dim() != 2 or (masks.shape[1] > 1 and masks.stride(1) != 1):
        raise TypeError("masks: expected uint8 [n, N] with contiguous rows")
    n = masks.shape[0]
    if masks.shape[1] != N:
        raise ValueError("ap_scene: masks must have one column per point")
    if n > AP_MAX_PREDS:
        raise ValueError(f"ap_scene: at most {AP_MAX_PREDS} predictions per scene, got {n}")
    if labels.numel() != n or scores.numel() != n:
        raise ValueError("ap_scene: labels and scores must have one entry per prediction")
    C, O = int(n_classes), overlaps.numel()
    slots = [int(k) for k in slots]
    if len(slots) != O:
        raise ValueError("ap_scene: one slot count per overlap")
    nb = lib.sd3d_ap_scene_ws_bytes(N, n)
    if nb == 0:
        raise ValueError(f"ap_scene: unsupported size (N = {N}, n = {n})")
    ws = _WS_AP.get(nb, gt_sem.device)
    slots_c = (ctypes.c_int32 * O)(*slots)
    pitch = masks.stride(0) if n > 1 else max(N, 1)
    _lib.check(lib.sd3d_ap_scene(ps, ss, pi, si, N, _ptr(id_map, torch.int64, "id_map"), id_map.numel() if id_map is not None else 0,
                                 int(num_stuff), masks.data_ptr() if n else None, pitch, n, _ptr(labels, torch.int64, "labels") if n else None,
                                 _ptr(scores, torch.float32, "scores") if n else None, _ptr(class_lut, torch.int32, "class_lut"),
                                 class_lut.numel(), int(zero_class), C, _ptr(overlaps, torch.float64, "overlaps"), slots_c, O, int(min_region),
                                 _ptr(store, torch.int64, "store"), int(slot_begin), int(slot_cap),
                                 _accumulator(hard_fn, torch.int64, C * O, "hard_fn"), _accumulator(has_gt, torch.int64, C, "has_gt"),
                                 _accumulator(has_pred, torch.int64, C, "has_pred"), _accumulator(status, torch.int64, 1, "status"),
                                 ws.data_ptr(), ws.numel(), _stream()), "ap_scene")


def ap_finish(codes, n_classes: int, n_overlaps: int, hard_fn, has_gt, has_pred):
    """AP [C * O] and best-F1 precision / recall [2, C * O] (float64, on the device) from the entry codes of all scenes
    (`sd3d_ap_finish`; `codes` int64 is clobbered) and the counters.  Enqueues only."""
    lib = _lib.load()
    C, O = int(n_classes), int(n_overlaps)
    dev = hard_fn.device
    n = codes.numel()
    ap = torch.empty(C * O, dtype=torch.float64, device=dev)
    pr_rc = torch.empty(2, C * O, dtype=torch.float64, device=dev)
    nb = lib.sd3d_ap_finish_ws_bytes(n)
    if nb == 0:
        raise ValueError(f"ap_finish: unsupported size (n_slots = {n})")
    ws = _WS_AP_FIN.get(nb, dev)
    _lib.check(lib.sd3d_ap_finish(_ptr(codes, torch.int64, "codes") if n else None, n, C, O, _accumulator(hard_fn, torch.int64, C * O, "hard_fn"),
                                  _accumulator(has_gt, torch.int64, C, "has_gt"), _accumulator(has_pred, torch.int64, C, "has_pred"),
                                  _ptr(ap), _ptr(pr_rc), ws.data_ptr(), ws.numel(), _stream()), "ap_finish")
    return ap, pr_rc


# --------------------------------------------------------------------------------------------
# ScanNet instance AP per scene (csrc/apeval_scene.hip)
# --------------------------------------------------------------------------------------------
AP_SCENE_KEY_LIMIT = 1 << 30    # scenes * (classes * overlaps + 1) must stay below this: the scene prefix shares a 63-bit sort key
_WS_AP_SCN = _PerThread()       # ap_finish_scenes: composite keys, sort buffers and the curve points


def ap_finish_scenes(codes, slot_offsets, n_classes: int, n_overlaps: int, counters, mask50: int, mask25: int):
    """Per-scene AP [S, C, O], best-F1 precision / recall [2, S, C, O] and the five means of `compute_averages` [S, 5] (float64, on
    the device) from the store's entry codes (`sd3d_ap_finish_scenes`; `codes` int64 is only read), the host list `slot_offsets`
    [S + 1] (scene s owns the slots [off[s], off[s + 1]); a device int64 tensor is taken as it is) and the per-scene counters int64
    [S, C * O + 2 * C].  mask50 / mask25: bit o set = overlap o belongs to the 0.5 / 0.25 set.  Enqueues only."""
    lib = _lib.load()
    C, O = int(n_classes), int(n_overlaps)
    for t, name in ((codes, "codes"), (counters, "counters")):
        if not t.is_cuda:
            raise RuntimeError(f"{name}: expected a tensor on the HIP device, got {t.device} (no CPU fallback)")
    if counters.dim() != 2:
        raise ValueError("ap_finish_scenes: counters must be [S, C * O + 2 * C]")
    S, n = counters.shape[0], codes.numel()
    if S < 1:
        raise ValueError("ap_finish_scenes: at least one scene")
    if S * (C * O + 1) >= AP_SCENE_KEY_LIMIT:
        raise ValueError(f"ap_finish_scenes: scenes * (classes * overlaps + 1) = {S * (C * O + 1)} must stay below 2^30 (the sort key)")
    dev = counters.device
    if torch.is_tensor(slot_offsets):
        off = slot_offsets
    else:
        host = np.ascontiguousarray(slot_offsets, dtype=np.int64).reshape(-1)
        if len(host) != S + 1 or host[0] != 0 or host[-1] != n or np.any(np.diff(host) < 0):
            raise ValueError("ap_finish_scenes: slot_offsets must ascend from 0 to the number of slots, one more than there are scenes")
        off = torch.from_numpy(host).pin_memory().to(dev, non_blocking=True)
    if off.numel() != S + 1:
        raise ValueError("ap_finish_scenes: one slot offset more than there are scenes")
    ap = torch.empty(S, C, O, dtype=torch.float64, device=dev)
    pr_rc = torch.empty(2, S, C, O, dtype=torch.float64, device=dev)
    summary = torch.empty(S, 5, dtype=torch.float64, device=dev)
    nb = lib.sd3d_ap_finish_scenes_ws_bytes(n)
    if nb == 0:
        raise ValueError(f"ap_finish_scenes: unsupported size (n_slots = {n})")
    ws = _WS_AP_SCN.get(nb, dev)
    _lib.check(lib.sd3d_ap_finish_scenes(_ptr(codes, torch.int64, "codes") if n else None, n, _ptr(off, torch.int64, "slot_offsets"), S, C, O,
                                         _accumulator(counters, torch.int64, S * (C * O + 2 * C), "counters"), int(mask50), int(mask25),
                                         _ptr(ap), _ptr(pr_rc), _ptr(summary), ws.data_ptr(), ws.numel(), _stream()), "ap_finish_scenes")
    return ap, pr_rc, summary


def ap_reduce_counters(counters, n_classes: int, n_overlaps: int):
    """Per-scene counters int64 [S, C * O + 2 * C] reduced to the [C * O + 2 * C] an `ApAccumulator` fed the same scenes holds
    (`sd3d_ap_reduce_counters`: hard_fn added, has_gt / has_pred OR-ed, integers only).  S = 0 gives zeros.  Enqueues only."""
    lib = _lib.load()
    C, O = int(n_classes), int(n_overlaps)
    n = C * O + 2 * C
    if counters.dim() != 2 or counters.shape[1] != n:
        raise ValueError(f"ap_reduce_counters: counters must be [S, {n}]")
    S = counters.shape[0]
    if S:
        p = _accumulator(counters, torch.int64, S * n, "counters")
    elif not counters.is_cuda:
        raise RuntimeError(f"counters: expected a tensor on the HIP device, got {counters.device} (no CPU fallback)")
    else:
        p = None
    out = torch.empty(n, dtype=torch.int64, device=counters.device)
    _lib.check(lib.sd3d_ap_reduce_counters(p, S, C, O, _ptr(out), _stream()), "ap_reduce_counters")
    return out


# --------------------------------------------------------------------------------------------
# streamed 3D box AP / AR (csrc/boxeval.hip)
# --------------------------------------------------------------------------------------------
BOX_AP_STATUS = AP_STATUS + ((32, "a ground-truth instance has a non-finite coordinate (or a ground-truth box a bad corner)"),
                             (64, "a predicted box has a negative or non-finite size or a non-finite centre"))
BOX_AP_INSTANCE_COLS = 1000
_WS_BOX_GT = _PerThread()     # gt_boxes: per-column integer partials of one scene
_WS_BOX = _PerThread()        # box_ap_scene: best ground truth per prediction, first prediction per (ground truth, threshold)
_WS_BOX_FIN = _PerThread()    # box_ap_finish: sort buffers


def gt_boxes(points, gt_sem, gt_inst, class_lut, n_classes: int, status, id_map=None, num_stuff: int = 0):
    """Ground-truth boxes of one scene (`sd3d_gt_boxes`): points fp32 [N, >= 3] with contiguous rows (any pitch), gt_sem / gt_inst
    int64 [N] (any element stride) read by the id rule of `ap_scene` -> (corners fp32 [1000, 6] = min xyz, max xyz per instance
    column, cls int32 [1000], -1 = no such instance).  `status` int64 [1] persists across calls.  Enqueues only."""
    lib = _lib.load()
    pp, ld = _rows(points, "points")
    ps, ss = _labels1d(gt_sem, "gt_sem")
    pi, si = _labels1d(gt_inst, "gt_inst")
    N = gt_sem.numel()
    if gt_inst.numel() != N or points.shape[0] != N or points.shape[1] < 3:
        raise ValueError("gt_boxes: points [N, >= 3], gt_sem and gt_inst must have one entry per point")
    dev = gt_sem.device
    corners = torch.empty(BOX_AP_INSTANCE_COLS, 6, dtype=torch.float32, device=dev)
    cls = torch.empty(BOX_AP_INSTANCE_COLS, dtype=torch.int32, device=dev)
    ws = _WS_BOX_GT.get(lib.sd3d_gt_boxes_ws_bytes(), dev)
    _lib.check(lib.sd3d_gt_boxes(pp if N else None, max(ld, 3), N, ps if N else None, ss, pi if N else None, si,
                                 _ptr(id_map, torch.int64, "id_map"), id_map.numel() if id_map is not None else 0, int(num_stuff),
                                 _ptr(class_lut, torch.int32, "class_lut"), class_lut.numel(), int(n_classes), _ptr(corners), _ptr(cls),
                                 _accumulator(status, torch.int64, 1, "status"), ws.data_ptr(), ws.numel(), _stream()), "gt_boxes")
    return corners, cls


def box_ap_scene(boxes, labels, scores, gt_corners, gt_cls, n_classes: int, thresholds, store, slot_begin: int, slot_cap: int, npos,
                 has_pred, status):
    """One scene of the streamed box AP protocol (`sd3d_box_ap_scene`): boxes fp32 [n, 6] (centre, size), labels int64 [n] class
    index, scores fp32 [n], gt_corners fp32 [G, 6], gt_cls int32 [G] (-1 = none), thresholds float64 [T] on the device.  One entry per
    (threshold, prediction) into `store[slot_begin + o * n + r]` (those below `slot_begin + slot_cap`); npos / has_pred int64 [C] and
    status int64 [1] persist across calls.  Enqueues only; scratch comes from a per-stream buffer."""
    lib = _lib.load()
    n, G = labels.numel(), gt_cls.numel()
    if n > AP_MAX_PREDS:
        raise ValueError(f"box_ap_scene: at most {AP_MAX_PREDS} predictions per scene, got {n}")
    if G > BOX_AP_INSTANCE_COLS:
        raise ValueError(f"box_ap_scene: at most {BOX_AP_INSTANCE_COLS} ground-truth boxes per scene, got {G}")
    if tuple(boxes.shape) != (n, 6) or scores.numel() != n:
        raise ValueError("box_ap_scene: boxes [n, 6], labels and scores must have one entry per prediction")
    if tuple(gt_corners.shape) != (G, 6):
        raise ValueError("box_ap_scene: gt_corners [G, 6] and gt_cls [G] must have one entry per ground truth")
    C, T = int(n_classes), thresholds.numel()
    nb = lib.sd3d_box_ap_scene_ws_bytes(n, G, T)
    if nb == 0:
        raise ValueError(f"box_ap_scene: unsupported size (n = {n}, G = {G}, T = {T})")
    ws = _WS_BOX.get(nb, npos.device)
    _lib.check(lib.sd3d_box_ap_scene(_ptr(boxes, torch.float32, "boxes") if n else None, n, _ptr(labels, torch.int64, "labels") if n else None,
                                     _ptr(scores, torch.float32, "scores") if n else None,
                                     _ptr(gt_corners, torch.float32, "gt_corners") if G else None, _ptr(gt_cls, torch.int32, "gt_cls") if G else None,
                                     G, C, _ptr(thresholds, torch.float64, "thresholds"), T, _ptr(store, torch.int64, "store"), int(slot_begin),
                                     int(slot_cap), _accumulator(npos, torch.int64, C, "npos"), _accumulator(has_pred, torch.int64, C, "has_pred"),
                                     _accumulator(status, torch.int64, 1, "status"), ws.data_ptr(), ws.numel(), _stream()), "box_ap_scene")


def box_ap_finish(codes, n_classes: int, n_overlaps: int, npos):
    """AP [C * T] and AR [C * T] (float64, on the device) from the entry codes of all scenes (`sd3d_box_ap_finish`; `codes` int64 is
    clobbered) and the ground-truth counts.  Enqueues only."""
    lib = _lib.load()
    C, T = int(n_classes), int(n_overlaps)
    dev = npos.device
    n = codes.numel()
    ap = torch.empty(C * T, dtype=torch.float64, device=dev)
    ar = torch.empty(C * T, dtype=torch.float64, device=dev)
    nb = lib.sd3d_box_ap_finish_ws_bytes(n)
    if nb == 0:
        raise ValueError(f"box_ap_finish: unsupported size (n_slots = {n})")
    ws = _WS_BOX_FIN.get(nb, dev)
    _lib.check(lib.sd3d_box_ap_finish(_ptr(codes, torch.int64, "codes") if n else None, n, C, T, _accumulator(npos, torch.int64, C, "npos"),
                                      _ptr(ap), _ptr(ar), ws.data_ptr(), ws.numel(), _stream()), "box_ap_finish")
    return ap, ar


# ---------------------------------------------------------------------------------------------- multi-view lifting (csrc/lift2d.hip)
LIFT_MAX_CHANNELS = 1024


def _lift_views(points, world_to_cam, intrinsics, name):
    """The shapes the lifting kernels index by -> (points ptr, ld, N, V)."""
    pp, ld = _rows(points, f"{name}: points")
    N = points.shape[0]
    if points.shape[1] < 3:
        raise ValueError(f"{name}: points must be fp32 [N, >= 3]")
    if world_to_cam.dim() != 3 or tuple(world_to_cam.shape[1:]) != (3, 4) or world_to_cam.shape[0] < 1:
        raise ValueError(f"{name}: world_to_cam must be [V, 3, 4] with V >= 1, got {list(world_to_cam.shape)}")
    V = world_to_cam.shape[0]
    _want_shape(intrinsics, [(V, 4)], f"{name}: intrinsics")
    return pp, max(ld, 3), N, V


def lift_visibility(points, world_to_cam, intrinsics, depth, depth_scale=None, near=0.05, border=0, tol_abs=0.05, tol_rel=0.0, count=None):
    """Depth-tested visibility of every point in every view (`sd3d_lift_visibility`): points fp32 [N, >= 3], world_to_cam fp32
    [V, 3, 4], intrinsics fp32 [V, 4] (fx, fy, cx, cy), depth uint16 [V, Hd, Wd] with `depth_scale` or fp32 metres ->
    (bits int32 [N, ceil(V / 32)], the words of the point-major mask, and count int32 [N]).  With `count` given the set bits are
    added to it.  Enqueues only."""
    lib = _lib.load()
    pp, ld, N, V = _lift_views(points, world_to_cam, intrinsics, "lift_visibility")
    if depth.dim() != 3 or depth.shape[0] != V or depth.shape[1] < 1 or depth.shape[2] < 1:
        raise ValueError(f"lift_visibility: depth must be [V = {V}, Hd, Wd], got {list(depth.shape)}")
    u16, scale = _depth_arg(depth, depth_scale, "lift_visibility", max_dim=None)
    if int(border) != border or border < 0 or not near >= 0.0 or not tol_abs >= 0.0 or not tol_rel >= 0.0:
        raise ValueError("lift_visibility: border must be an integer >= 0; near, tol_abs and tol_rel must be >= 0")
    W = (V + 31) // 32
    bits = torch.empty(N, W, dtype=torch.int32, device=points.device)
    add = count is not None
    if add:
        _accumulator(count, torch.int32, N, "lift_visibility: count")
    else:
        count = torch.empty(N, dtype=torch.int32, device=points.device)
    _lib.check(lib.sd3d_lift_visibility(pp if N else None, ld, N, _ptr(world_to_cam, torch.float32, "lift_visibility: world_to_cam"),
                                        _ptr(intrinsics, torch.float32, "lift_visibility: intrinsics"), _ptr(depth, None, "lift_visibility: depth"),
                                        u16, scale, V, depth.shape[1], depth.shape[2], float(near), int(border), float(tol_abs), float(tol_rel),
                                        _ptr(bits) if N else None, _ptr(count) if N else None, int(add), _stream()), "lift_visibility")
    return bits, count


def lift_accumulate(points, world_to_cam, intrinsics, depth_hw, bits, maps, sum, v0: int = 0, v1: Optional[int] = None):
    """Adds the bilinear samples of the visible views [v0, v1) to `sum` fp32 [N, C] in ascending view order
    (`sd3d_lift_accumulate`): bits int32 [N, ceil(V / 32)] as `lift_visibility` returns them, maps fp16 or fp32 [V, Hf, Wf, C]
    channels-last with C a multiple of 64 up to 1024, depth_hw = (Hd, Wd) of the depth images the intrinsics refer to.  Enqueues
    only."""
    lib = _lib.load()
    pp, ld, N, V = _lift_views(points, world_to_cam, intrinsics, "lift_accumulate")
    Hd, Wd = int(depth_hw[0]), int(depth_hw[1])
    if maps.dim() != 4 or maps.shape[0] != V or maps.shape[1] < 1 or maps.shape[2] < 1:
        raise ValueError(f"lift_accumulate: maps must be channels-last [V = {V}, Hf, Wf, C], got {list(maps.shape)}")
    if maps.dtype not in (torch.float16, torch.float32):
        raise TypeError(f"lift_accumulate: maps must be fp16 or fp32, got {maps.dtype}")
    C = maps.shape[3]
    if C < 64 or C > LIFT_MAX_CHANNELS or C % 64:
        raise ValueError(f"lift_accumulate: C must be a multiple of 64 up to {LIFT_MAX_CHANNELS}, got {C}")
    if N:
        _want_shape(bits, [(N, (V + 31) // 32)], "lift_accumulate: bits")
        _want_shape(sum, [(N, C)], "lift_accumulate: sum")
    v1 = V if v1 is None else int(v1)
    if not 0 <= v0 <= v1 <= V:
        raise ValueError(f"lift_accumulate: need 0 <= v0 <= v1 <= V, got [{v0}, {v1}) of {V}")
    _lib.check(lib.sd3d_lift_accumulate(pp if N else None, ld, N, _ptr(world_to_cam, torch.float32, "lift_accumulate: world_to_cam"),
                                        _ptr(intrinsics, torch.float32, "lift_accumulate: intrinsics"), V, Hd, Wd,
                                        _ptr(bits, torch.int32, "lift_accumulate: bits") if N else None, _ptr(maps, None, "lift_accumulate: maps"),
                                        int(maps.dtype == torch.float16), maps.shape[1], maps.shape[2], C, int(v0), v1,
                                        _ptr(sum, torch.float32, "lift_accumulate: sum") if N else None, _stream()), "lift_accumulate")


def lift_finish(sum, count, scale_index: int = 0, n_scales: int = 1, acc=None, out=None, out_dtype=torch.float32):
    """mean = sum / count (0 where count == 0) of one scale, added to `acc` fp32 [N, C] over the scales; the last scale returns
    (acc + mean) / n_scales as fp32 or fp16 [N, C], earlier ones return None (`sd3d_lift_finish`).  Enqueues only."""
    lib = _lib.load()
    if not sum.is_cuda:
        raise RuntimeError(f"lift_finish: sum: expected a tensor on the HIP device, got {sum.device} (no CPU fallback)")
    if sum.dim() != 2:
        raise ValueError("lift_finish: sum must be fp32 [N, C]")
    N, C = sum.shape
    if C < 64 or C > LIFT_MAX_CHANNELS or C % 64:
        raise ValueError(f"lift_finish: C must be a multiple of 64 up to {LIFT_MAX_CHANNELS}, got {C}")
    if not 0 <= scale_index < n_scales:
        raise ValueError("lift_finish: need 0 <= scale_index < n_scales")
    _want_shape(count, [(N,)], "lift_finish: count")
    last = scale_index == n_scales - 1
    if n_scales > 1:
        if acc is None:
            raise ValueError("lift_finish: several scales need the fp32 [N, C] accumulator `acc`")
        _want_shape(acc, [(N, C)], "lift_finish: acc")
    if last:
        if out_dtype not in (torch.float32, torch.float16):
            raise TypeError(f"lift_finish: out_dtype must be fp32 or fp16, got {out_dtype}")
        if out is None:
            out = torch.empty(N, C, dtype=out_dtype, device=sum.device)
        else:
            _want_shape(out, [(N, C)], "lift_finish: out")
            out_dtype = out.dtype
    _lib.check(lib.sd3d_lift_finish(_ptr(sum, torch.float32, "lift_finish: sum") if N else None, _ptr(count, torch.int32, "lift_finish: count") if N else None,
                                    N, C, int(scale_index), int(n_scales), _ptr(acc, torch.float32, "lift_finish: acc") if N else None,
                                    _ptr(out, out_dtype, "lift_finish: out") if last and N else None, int(last and out_dtype == torch.float16),
                                    _stream()), "lift_finish")
    return out if last else None


# --------------------------------------------------------------------------------------------
# lifting of 2D detector queries to 3D centres (csrc/lift_queries.hip; the rule: include/segdino3d_hip.h, segdino3d_amd/lift_queries.py)
# --------------------------------------------------------------------------------------------
LIFTQ_MAX_PIXELS = 1 << 28


def lift_query_centres(depth, depth_scale, intrinsics, cam_to_world, masks, far_mm, gate_mm, gate_permille, centre, count, median_mm):
    """Robust 3D centre of every (view, query) (`sd3d_lift_query_centres`): depth uint16 [V, Hd, Wd] with `depth_scale` or fp32 metres,
    intrinsics fp32 [V, 4], cam_to_world fp32 [V, 3, 4], masks bool or uint8 [V, Q, Hm, Wm] -> written into centre fp32 [V, Q, 3],
    count int32 [V, Q] and median_mm int32 [V, Q] (contiguous, e.g. slices of a store).  Enqueues only."""
    lib = _lib.load()
    if depth.dim() != 3 or depth.shape[0] < 1:
        raise ValueError(f"lift_query_centres: depth must be [V >= 1, Hd, Wd], got {list(depth.shape)}")
    V, Hd, Wd = depth.shape
    if Hd < 1 or Wd < 1 or Hd * Wd > LIFTQ_MAX_PIXELS:
        raise ValueError(f"lift_query_centres: depth images must have 1 .. 2^28 pixels (the int64 sums cannot overflow then), got {Hd} x {Wd}")
    u16, scale = _depth_arg(depth, depth_scale, "lift_query_centres", max_dim=None)
    _want_shape(intrinsics, [(V, 4)], "lift_query_centres: intrinsics")
    _want_shape(cam_to_world, [(V, 3, 4)], "lift_query_centres: cam_to_world")
    if masks.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"lift_query_centres: masks must be bool or uint8, got {masks.dtype}")
    if masks.dim() != 4 or masks.shape[0] != V or masks.shape[2] < 1 or masks.shape[3] < 1:
        raise ValueError(f"lift_query_centres: masks must be [V = {V}, Q, Hm, Wm], got {list(masks.shape)}")
    Q, Hm, Wm = masks.shape[1:]
    _want_shape(centre, [(V, Q, 3)], "lift_query_centres: centre")
    _want_shape(count, [(V, Q)], "lift_query_centres: count")
    _want_shape(median_mm, [(V, Q)], "lift_query_centres: median_mm")
    for name, x, lowest in (("far_mm", far_mm, 1), ("gate_mm", gate_mm, 0), ("gate_permille", gate_permille, 0)):
        if int(x) != x or not lowest <= x <= 65535:
            raise ValueError(f"lift_query_centres: {name} must be an integer in [{lowest}, 65535], got {x}")
    if Q == 0:
        return
    _lib.check(lib.sd3d_lift_query_centres(_ptr(depth, None, "lift_query_centres: depth"), u16, scale,
                                           _ptr(intrinsics, torch.float32, "lift_query_centres: intrinsics"),
                                           _ptr(cam_to_world, torch.float32, "lift_query_centres: cam_to_world"),
                                           _ptr(masks, None, "lift_query_centres: masks"), V, Q, Hd, Wd, Hm, Wm, int(far_mm), int(gate_mm),
                                           int(gate_permille), _ptr(centre, torch.float32, "lift_query_centres: centre"),
                                           _ptr(count, torch.int32, "lift_query_centres: count"),
                                           _ptr(median_mm, torch.int32, "lift_query_centres: median_mm"), _stream()), "lift_query_centres")


def lift_query_select(scores, count, score_thr, min_pixels, max_queries=None):
    """The rows with score >= score_thr and count >= min_pixels, all of them or the `max_queries` best by score (ties to the lower row),
    in ascending row order (`sd3d_lift_query_select`): scores fp32 [n], count int32 [n] -> (rows int32 [min(max_queries, n)], m int32
    [1] = how many of them are written, on the device).  Enqueues only."""
    lib = _lib.load()
    if scores.dim() != 1:
        raise ValueError(f"lift_query_select: scores must be fp32 [n], got {list(scores.shape)}")
    n = scores.shape[0]
    _want_shape(count, [(n,)], "lift_query_select: count")
    if int(min_pixels) != min_pixels or min_pixels < 1:
        raise ValueError(f"lift_query_select: min_pixels must be an integer >= 1, got {min_pixels}")
    if max_queries is not None and (int(max_queries) != max_queries or max_queries < 0):
        raise ValueError(f"lift_query_select: max_queries must be None or an integer >= 0, got {max_queries}")
    sp, cp = _ptr(scores, torch.float32, "lift_query_select: scores"), _ptr(count, torch.int32, "lift_query_select: count")
    cap = n if max_queries is None else min(int(max_queries), n)
    rows = torch.empty(cap, dtype=torch.int32, device=scores.device)
    m = torch.empty(1, dtype=torch.int32, device=scores.device)
    ws = _WS.get(lib.sd3d_lift_query_select_ws_bytes(n), scores.device)
    _lib.check(lib.sd3d_lift_query_select(sp if n else None, cp if n else None, n, float(score_thr), int(min_pixels),
                                          -1 if max_queries is None else int(max_queries), _ptr(rows) if cap else None, cap, _ptr(m),
                                          ws.data_ptr(), ws.numel(), _stream()), "lift_query_select")
    return rows, m


def lift_query_gather(feats, centre, rows, M: int):
    """(fp32 [M, C], fp32 [M, 3]) = rows `rows[:M]` of feats fp16 or fp32 [n, C] (C a multiple of 8) and of centre fp32 [n, 3]
    (`sd3d_lift_query_gather`).  Enqueues only."""
    lib = _lib.load()
    if feats.dtype not in (torch.float16, torch.float32):
        raise TypeError(f"lift_query_gather: feats must be fp16 or fp32, got {feats.dtype}")
    if feats.dim() != 2 or feats.shape[1] < 8 or feats.shape[1] % 8:
        raise ValueError(f"lift_query_gather: feats must be [n, C] with C a multiple of 8, got {list(feats.shape)}")
    n, C = feats.shape
    _want_shape(centre, [(n, 3)], "lift_query_gather: centre")
    M = int(M)
    if not 0 <= M <= rows.numel() or M > n or rows.dim() != 1:
        raise ValueError(f"lift_query_gather: need 0 <= M <= len(rows) and M <= n, got M = {M}, rows {list(rows.shape)}, n = {n}")
    out_feats = torch.empty(M, C, dtype=torch.float32, device=feats.device)
    out_pos = torch.empty(M, 3, dtype=torch.float32, device=feats.device)
    fp, cp, rp = _ptr(feats, None, "lift_query_gather: feats"), _ptr(centre, torch.float32, "lift_query_gather: centre"), \
        _ptr(rows, torch.int32, "lift_query_gather: rows")
    if M:
        _lib.check(lib.sd3d_lift_query_gather(fp, int(feats.dtype == torch.float16), cp, rp, n, M, C, _ptr(out_feats), _ptr(out_pos), _stream()),
                   "lift_query_gather")
    return out_feats, out_pos


# --------------------------------------------------------------------------------------------
# merging of lifted queries across views (csrc/merge_queries.hip; the rule: include/segdino3d_hip.h, segdino3d_amd/lift_queries.py)
# --------------------------------------------------------------------------------------------
MERGE_MAX_ROWS = 1 << 14
MERGE_MAX_CHANNELS = 1024
_WS_MERGE = _PerThread()  # merge_queries: codes, bit matrix, labels and cluster tables, alive from the adjacency call to the emit call


def _merge_rows(feats, centre, scores, count, who):
    """The checks the four calls share -> (n, C, pointers of feats, centre, scores, count)."""
    if feats.dtype not in (torch.float16, torch.float32):
        raise TypeError(f"{who}: feats must be fp16 or fp32, got {feats.dtype}")
    if feats.dim() != 2 or not 1 <= feats.shape[1] <= MERGE_MAX_CHANNELS:
        raise ValueError(f"{who}: feats must be [n, C] with 1 <= C <= {MERGE_MAX_CHANNELS} (the int64 cosine test is exact up to there), "
                         f"got {list(feats.shape)}")
    n, C = feats.shape
    if centre is not None:
        _want_shape(centre, [(n, 3)], f"{who}: centre")
    _want_shape(scores, [(n,)], f"{who}: scores")
    _want_shape(count, [(n,)], f"{who}: count")
    return n, C, _ptr(feats, None, f"{who}: feats"), _ptr(centre, torch.float32, f"{who}: centre"), \
        _ptr(scores, torch.float32, f"{who}: scores"), _ptr(count, torch.int32, f"{who}: count")


def _merge_ws(lib, n, C, ws, who):
    need = lib.sd3d_merge_queries_ws_bytes(n, C)
    if not isinstance(ws, torch.Tensor) or not ws.is_cuda or ws.dtype != torch.uint8 or ws.numel() < need:
        raise ValueError(f"{who}: ws must be the workspace merge_queries_adjacency returned for these rows ({need} bytes)")
    return ws


def merge_queries_adjacency(feats, centre, scores, count, score_thr, min_pixels, radius_q, sim_q):
    """Steps 1 to 5 of the merging rule (`sd3d_merge_queries_adjacency`): the valid rows ranked by score, their int8 codes and
    fixed-point centres, and the adjacency bit matrix of the ranks, all left in the workspace that is returned and that the sweep, the
    reduction and the emit calls take.  feats fp16 or fp32 [n, C <= 1024], centre fp32 [n, 3], scores fp32 [n], count int32 [n];
    radius_q = round(radius * 1024) in 1 .. 2^20, sim_q = round(sim * 128) in 1 .. 128 or 0 for distance only.  Enqueues only."""
    lib = _lib.load()
    who = "merge_queries_adjacency"
    n, C, fp, cp, sp, np_ = _merge_rows(feats, centre, scores, count, who)
    if int(min_pixels) != min_pixels or min_pixels < 1:
        raise ValueError(f"{who}: min_pixels must be an integer >= 1, got {min_pixels}")
    if int(radius_q) != radius_q or not 1 <= radius_q <= 1 << 20:
        raise ValueError(f"{who}: radius_q must be an integer in [1, 2^20], got {radius_q}")
    if int(sim_q) != sim_q or not 0 <= sim_q <= 128:
        raise ValueError(f"{who}: sim_q must be an integer in [0, 128], got {sim_q}")
    ws = _WS_MERGE.get(lib.sd3d_merge_queries_ws_bytes(n, C), feats.device)
    if n:
        _lib.check(lib.sd3d_merge_queries_adjacency(fp, int(feats.dtype == torch.float16), cp, sp, np_, n, C, float(score_thr), int(min_pixels),
                                                    int(radius_q), int(sim_q), ws.data_ptr(), ws.numel(), _stream()), who)
    return ws


def merge_queries_adjacency_read(n: int, C: int, ws):
    """What `merge_queries_adjacency` left in `ws` -> (rank_row int32 [Mp]: the row of each rank, -1 beyond the entering rows; adj int64
    [Mp, Mp / 64]: bit b % 64 of word [a, b / 64] = ranks a < b are adjacent), Mp = min(n, 16384) rounded up to 64.  For tests and tools."""
    lib = _lib.load()
    n, C = int(n), int(C)
    mp = (min(max(n, 1), MERGE_MAX_ROWS) + 63) // 64 * 64
    rank_row = torch.full((mp,), -1, dtype=torch.int32, device=ws.device)
    adj = torch.zeros(mp, mp // 64, dtype=torch.int64, device=ws.device)
    if n:
        ws = _merge_ws(lib, n, C, ws, "merge_queries_adjacency_read")
        _lib.check(lib.sd3d_merge_queries_adjacency_read(n, C, ws.data_ptr(), ws.numel(), _ptr(rank_row), _ptr(adj), _stream()),
                   "merge_queries_adjacency_read")
    return rank_row, adj


def merge_queries_sweep(n: int, C: int, ws):
    """Step 6 (`sd3d_merge_queries_sweep`): the leader clustering over the bit matrix in `ws`.  Enqueues only."""
    lib = _lib.load()
    if int(n):
        ws = _merge_ws(lib, int(n), int(C), ws, "merge_queries_sweep")
        _lib.check(lib.sd3d_merge_queries_sweep(int(n), int(C), ws.data_ptr(), ws.numel(), _stream()), "merge_queries_sweep")


def merge_queries_reduce(scores, count, C: int, queries_per_view: int, score_thr, min_views, max_queries, ws):
    """Steps 7 and 8 but the features (`sd3d_merge_queries_reduce`) -> k int32 [1] on the device: the number of emitted clusters.
    Enqueues only."""
    lib = _lib.load()
    who = "merge_queries_reduce"
    if scores.dim() != 1:
        raise ValueError(f"{who}: scores must be fp32 [n], got {list(scores.shape)}")
    n = scores.shape[0]
    _want_shape(count, [(n,)], f"{who}: count")
    if int(queries_per_view) != queries_per_view or queries_per_view < 1:
        raise ValueError(f"{who}: queries_per_view must be an integer >= 1, got {queries_per_view}")
    if int(min_views) != min_views or min_views < 1:
        raise ValueError(f"{who}: min_views must be an integer >= 1, got {min_views}")
    if max_queries is not None and (int(max_queries) != max_queries or max_queries < 0):
        raise ValueError(f"{who}: max_queries must be None or an integer >= 0, got {max_queries}")
    sp, np_ = _ptr(scores, torch.float32, f"{who}: scores"), _ptr(count, torch.int32, f"{who}: count")
    k = torch.zeros(1, dtype=torch.int32, device=scores.device)
    if n:
        ws = _merge_ws(lib, n, int(C), ws, who)
        _lib.check(lib.sd3d_merge_queries_reduce(sp, np_, n, int(C), int(queries_per_view), float(score_thr), int(min_views),
                                                 -1 if max_queries is None else int(max_queries), _ptr(k), ws.data_ptr(), ws.numel(), _stream()),
                   who)
    return k


def merge_queries_emit(feats, scores, count, K: int, best: bool, ws):
    """The emitted clusters (`sd3d_merge_queries_emit`), K = the value read from `merge_queries_reduce` -> (feats fp32 [K, C], pos fp32
    [K, 3], scores fp32 [K], views int32 [K], labels int32 [n]).  Enqueues only."""
    lib = _lib.load()
    who = "merge_queries_emit"
    n, C, fp, _, sp, np_ = _merge_rows(feats, None, scores, count, who)
    K = int(K)
    if not 0 <= K <= min(n, MERGE_MAX_ROWS):
        raise ValueError(f"{who}: need 0 <= K <= min(n, {MERGE_MAX_ROWS}), got K = {K}, n = {n}")
    dev = feats.device
    out = (torch.empty(K, C, dtype=torch.float32, device=dev), torch.empty(K, 3, dtype=torch.float32, device=dev),
           torch.empty(K, dtype=torch.float32, device=dev), torch.empty(K, dtype=torch.int32, device=dev),
           torch.empty(n, dtype=torch.int32, device=dev))
    if n:
        ws = _merge_ws(lib, n, C, ws, who)
        _lib.check(lib.sd3d_merge_queries_emit(fp, int(feats.dtype == torch.float16), sp, np_, n, C, K, int(bool(best)),
                                               *(_ptr(t) if t.numel() else None for t in out[:4]), _ptr(out[4]), ws.data_ptr(), ws.numel(),
                                               _stream()), who)
    return out


# --------------------------------------------------------------------------------------------
# superpoints from a mesh (csrc/superpoints.hip; the rule: include/segdino3d_hip.h, segdino3d_amd/superpoints.py)
# --------------------------------------------------------------------------------------------
SUPERPOINTS_MAX_VERTICES = 1 << 24      # per scene
_WS_SP = _PerThread()    # mesh_superpoints: normal sums, edge keys and sort buffers, the forest and the label tables


def mesh_superpoints(vertices, faces, vertex_offsets, face_offsets, k_thresh: float, min_verts: int, debug: bool = False):
    """Graph segmentation of a batch of concatenated meshes (`sd3d_mesh_superpoints`): vertices fp32 [N, 3], faces int32 or int64
    [F, 3] with indices local to each scene, vertex_offsets / face_offsets int64 [n_scenes + 1] on the device -> (labels int64 [N],
    info int32 [n_scenes, 2] = {superpoints, ignored faces} per scene, on the device), and with `debug` also (normals fp32 [N, 3],
    weight bits int32 [3 F], sweep_stats int64 [n_scenes, 2]).  Enqueues only."""
    lib = _lib.load()
    who = "mesh_superpoints"
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"{who}: vertices must be fp32 [N, 3], got {list(vertices.shape)}")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{who}: faces must be int32 or int64 [F, 3], got {list(faces.shape)}")
    if vertices.dtype != torch.float32:
        raise ValueError(f"{who}: vertices must be fp32, got {vertices.dtype}")
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{who}: faces must be int32 or int64, got {faces.dtype}")
    N, F = vertices.shape[0], faces.shape[0]
    S = vertex_offsets.numel() - 1
    if S < 1 or face_offsets.numel() != S + 1:
        raise ValueError(f"{who}: vertex_offsets and face_offsets must both be int64 [n_scenes + 1] with n_scenes >= 1")
    if 3 * F >= 1 << 31 or N >= 1 << 31:
        raise ValueError(f"{who}: need N < 2^31 and 3 F < 2^31 over the batch, got N = {N}, F = {F}")
    if not (np.isfinite(k_thresh) and k_thresh >= 0):
        raise ValueError(f"{who}: k_thresh must be finite and >= 0, got {k_thresh}")
    if int(min_verts) != min_verts or min_verts < 1:
        raise ValueError(f"{who}: min_verts must be an integer >= 1, got {min_verts}")
    vp, fp = _ptr(vertices, torch.float32, f"{who}: vertices"), _ptr(faces, None, f"{who}: faces")
    vo, fo = _ptr(vertex_offsets, torch.int64, f"{who}: vertex_offsets"), _ptr(face_offsets, torch.int64, f"{who}: face_offsets")
    dev = vertices.device
    labels = torch.empty(N, dtype=torch.int64, device=dev)
    info = torch.empty(S, 2, dtype=torch.int32, device=dev)
    extra = ()
    if debug:
        extra = (torch.empty(N, 3, dtype=torch.float32, device=dev), torch.empty(3 * F, dtype=torch.int32, device=dev),
                 torch.empty(S, 2, dtype=torch.int64, device=dev))
    need = lib.sd3d_superpoints_ws_bytes(N, F, S)
    if need == 0:
        raise ValueError(f"{who}: sizes out of range (N = {N}, F = {F}, n_scenes = {S})")
    ws = _WS_SP.get(need, dev)
    _lib.check(lib.sd3d_mesh_superpoints(vp if N else None, fp if F else None, int(faces.dtype == torch.int64), vo, fo, N, F, S, float(k_thresh),
                                         int(min_verts), _ptr(labels) if N else None, _ptr(info),
                                         *((_ptr(t) if t.numel() else None for t in extra) if debug else (None, None, None)),
                                         ws.data_ptr(), ws.numel(), _stream()), who)
    return (labels, info) + tuple(extra)


# --------------------------------------------------------------------------------------------
# superpoints from a point cloud: k-NN graph, normals, segmentation of a general edge list (csrc/superpoints.hip)
# --------------------------------------------------------------------------------------------
KNN_MAX_K = 64
KNN_MAX_RADIUS = 4.0
_WS_KNN = _PerThread()   # knn_graph: bucket keys and sort buffers, the points in bucket order, the bucket ranges
_WS_GSP = _PerThread()   # graph_superpoints: edge keys and sort buffers, the forest and the label tables


def _scene_count(vertex_offsets, who):
    S = vertex_offsets.numel() - 1
    if S < 1:
        raise ValueError(f"{who}: vertex_offsets must be int64 [n_scenes + 1] with n_scenes >= 1")
    return S


def knn_graph(points, vertex_offsets, k: int, radius: float, return_d2: bool = False):
    """The exact k-NN graph of a batch of concatenated clouds (`sd3d_knn_graph`): points fp32 [N, 3], vertex_offsets int64
    [n_scenes + 1] on the device -> nbr int32 [N, k] with indices local to each scene (-1: no neighbour), and with `return_d2` the
    squared distances fp32 [N, k] (+inf: no neighbour).  Enqueues only."""
    lib = _lib.load()
    who = "knn_graph"
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError(f"{who}: points must be fp32 [N, 3], got {points.dtype} {list(points.shape)}")
    if int(k) != k or k < 1 or k > KNN_MAX_K:
        raise ValueError(f"{who}: k must be an integer in [1, {KNN_MAX_K}], got {k}")
    if not (np.isfinite(radius) and 0 < radius <= KNN_MAX_RADIUS):
        raise ValueError(f"{who}: radius must lie in (0, {KNN_MAX_RADIUS}], got {radius}")
    N, S = points.shape[0], _scene_count(vertex_offsets, who)
    if N * int(k) >= 1 << 31:
        raise ValueError(f"{who}: need N k < 2^31, got N = {N}, k = {k}")
    pp, vo = _ptr(points, torch.float32, f"{who}: points"), _ptr(vertex_offsets, torch.int64, f"{who}: vertex_offsets")
    dev = points.device
    nbr = torch.empty(N, int(k), dtype=torch.int32, device=dev)
    d2 = torch.empty(N, int(k), dtype=torch.float32, device=dev) if return_d2 else None
    need = lib.sd3d_knn_graph_ws_bytes(N, S)
    if need == 0:
        raise ValueError(f"{who}: sizes out of range (N = {N}, n_scenes = {S})")
    ws = _WS_KNN.get(need, dev)
    _lib.check(lib.sd3d_knn_graph(pp if N else None, vo, N, S, int(k), float(radius), _ptr(nbr) if N else None,
                                  _ptr(d2) if return_d2 and N else None, ws.data_ptr(), ws.numel(), _stream()), who)
    return (nbr, d2) if return_d2 else nbr


def point_normals(points, nbr, vertex_offsets, viewpoint=None):
    """Normals from each point's neighbourhood (`sd3d_point_normals`): points fp32 [N, 3], nbr int32 [N, k], viewpoint None (the
    canonical sign), fp32 [n_scenes, 3] or fp32 [N, 3] -> normals fp32 [N, 3].  Enqueues only."""
    lib = _lib.load()
    who = "point_normals"
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError(f"{who}: points must be fp32 [N, 3], got {points.dtype} {list(points.shape)}")
    N, S = points.shape[0], _scene_count(vertex_offsets, who)
    if nbr.dim() != 2 or nbr.shape[0] != N or nbr.dtype != torch.int32 or not 1 <= nbr.shape[1] <= KNN_MAX_K:
        raise ValueError(f"{who}: nbr must be int32 [N, k] with 1 <= k <= {KNN_MAX_K}, got {nbr.dtype} {list(nbr.shape)}")
    k = nbr.shape[1]
    per_point = 0
    if viewpoint is not None:
        if viewpoint.dtype != torch.float32 or tuple(viewpoint.shape) not in ((S, 3), (N, 3)):
            raise ValueError(f"{who}: viewpoint must be fp32 [n_scenes, 3] or [N, 3], got {viewpoint.dtype} {list(viewpoint.shape)}")
        per_point = int(tuple(viewpoint.shape) != (S, 3))
    pp, vo = _ptr(points, torch.float32, f"{who}: points"), _ptr(vertex_offsets, torch.int64, f"{who}: vertex_offsets")
    normals = torch.empty(N, 3, dtype=torch.float32, device=points.device)
    if N:
        _lib.check(lib.sd3d_point_normals(pp, _ptr(nbr, torch.int32, f"{who}: nbr"), vo, N, S, k,
                                          None if viewpoint is None else _ptr(viewpoint, torch.float32, f"{who}: viewpoint"), per_point,
                                          _ptr(normals), _stream()), who)
    return normals


def graph_superpoints(points, normals, ea, eb, vertex_offsets, edge_offsets, oriented: bool, k_thresh: float, min_verts: int,
                      debug: bool = False):
    """Graph segmentation of a batch of concatenated clouds over a given edge list (`sd3d_graph_superpoints`): points, normals fp32
    [N, 3], ea, eb int32 [E] with indices local to each scene, vertex_offsets / edge_offsets int64 [n_scenes + 1] on the device ->
    (labels int64 [N], info int32 [n_scenes, 2] = {superpoints, ignored edges} per scene, on the device), and with `debug` also
    (weight bits int32 [E], sweep_stats int64 [n_scenes, 2]).  Enqueues only."""
    lib = _lib.load()
    who = "graph_superpoints"
    for t, name in ((points, "points"), (normals, "normals")):
        if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float32:
            raise ValueError(f"{who}: {name} must be fp32 [N, 3], got {t.dtype} {list(t.shape)}")
    N, E = points.shape[0], ea.numel()
    if normals.shape[0] != N:
        raise ValueError(f"{who}: normals must have one row per point, got {normals.shape[0]} for {N}")
    if ea.dim() != 1 or eb.dim() != 1 or eb.numel() != E or ea.dtype != torch.int32 or eb.dtype != torch.int32:
        raise ValueError(f"{who}: ea and eb must both be int32 [E], got {ea.dtype} {list(ea.shape)} and {eb.dtype} {list(eb.shape)}")
    S = _scene_count(vertex_offsets, who)
    if edge_offsets.numel() != S + 1:
        raise ValueError(f"{who}: vertex_offsets and edge_offsets must both be int64 [n_scenes + 1]")
    if E >= 1 << 31 or N >= 1 << 31:
        raise ValueError(f"{who}: need N < 2^31 and E < 2^31 over the batch, got N = {N}, E = {E}")
    if not (np.isfinite(k_thresh) and k_thresh >= 0):
        raise ValueError(f"{who}: k_thresh must be finite and >= 0, got {k_thresh}")
    if int(min_verts) != min_verts or min_verts < 1:
        raise ValueError(f"{who}: min_verts must be an integer >= 1, got {min_verts}")
    pp, np_ = _ptr(points, torch.float32, f"{who}: points"), _ptr(normals, torch.float32, f"{who}: normals")
    ap, bp = _ptr(ea, torch.int32, f"{who}: ea"), _ptr(eb, torch.int32, f"{who}: eb")
    vo, eo = _ptr(vertex_offsets, torch.int64, f"{who}: vertex_offsets"), _ptr(edge_offsets, torch.int64, f"{who}: edge_offsets")
    dev = points.device
    labels = torch.empty(N, dtype=torch.int64, device=dev)
    info = torch.empty(S, 2, dtype=torch.int32, device=dev)
    extra = ()
    if debug:
        extra = (torch.empty(E, dtype=torch.int32, device=dev), torch.empty(S, 2, dtype=torch.int64, device=dev))
    need = lib.sd3d_graph_superpoints_ws_bytes(N, E, S)
    if need == 0:
        raise ValueError(f"{who}: sizes out of range (N = {N}, E = {E}, n_scenes = {S})")
    ws = _WS_GSP.get(need, dev)
    _lib.check(lib.sd3d_graph_superpoints(pp if N else None, np_ if N else None, ap if E else None, bp if E else None, vo, eo, N, E, S,
                                          int(bool(oriented)), float(k_thresh), int(min_verts), _ptr(labels) if N else None, _ptr(info),
                                          *((_ptr(t) if t.numel() else None for t in extra) if debug else (None, None)),
                                          ws.data_ptr(), ws.numel(), _stream()), who)
    return (labels, info) + tuple(extra)


# --------------------------------------------------------------------------------------------
# fusion of posed RGB-D frames into a point cloud (csrc/fuse_views.hip; the rule: include/segdino3d_hip.h, segdino3d_amd/fuse_views.py)
# --------------------------------------------------------------------------------------------
FUSE_MIN_CAPACITY = 16
FUSE_MAX_CAPACITY = 1 << 24
FUSE_MAX_DIM = 16384
FUSE_INFO = ("n", "cells", "pixels_used", "out_of_range", "overflow")


# The argument checks the stages that start from a depth pixel share (csrc/depth_pixel.h has the C side), one per rule.
def _depth_arg(depth, depth_scale, who, dims=3, max_dim=FUSE_MAX_DIM):
    """depth of rank `dims`, uint16 with a `depth_scale` or fp32 metres without one -> (u16, scale) as the C calls take them."""
    if depth.dim() != dims:
        raise ValueError(f"{who}: depth must be {'[V, Hd, Wd]' if dims == 3 else '[Hd, Wd], one frame'}, got {list(depth.shape)}")
    Hd, Wd = depth.shape[-2:]
    if max_dim is not None and not (1 <= Hd <= max_dim and 1 <= Wd <= max_dim):
        raise ValueError(f"{who}: depth images must be 1 .. {max_dim} a side, got {Hd} x {Wd}")
    if depth.dtype == torch.uint16:
        if depth_scale is None or not float(depth_scale) > 0.0:
            raise ValueError(f"{who}: uint16 depth needs a depth_scale > 0 (ScanNet: 0.001)")
        return 1, float(depth_scale)
    if depth.dtype == torch.float32:
        if depth_scale is not None:
            raise ValueError(f"{who}: fp32 depth is in metres and takes no depth_scale")
        return 0, 1.0
    raise TypeError(f"{who}: depth must be uint16 or fp32, got {depth.dtype}")


def _range_args(near, far, edge_abs, edge_rel, who):
    """-> (near, far, edge_abs, edge_rel, use_edges) as the C calls take them; `edge_rel=None` turns the edge test off."""
    if not (float(near) >= 0.0 and float(far) >= float(near)):
        raise ValueError(f"{who}: need 0 <= near <= far, got near = {near}, far = {far}")
    if edge_rel is None:
        return float(near), float(far), 0.0, 0.0, 0
    if not (float(edge_abs) >= 0.0 and float(edge_rel) >= 0.0):
        raise ValueError(f"{who}: edge_abs and edge_rel must be >= 0 (edge_rel=None: no edge test), got {edge_abs}, {edge_rel}")
    return float(near), float(far), float(edge_abs), float(edge_rel), 1


def _colors_arg(colors, V, who):
    """colors uint8 [V, Hc, Wc, 3] -> (Hc, Wc)."""
    if colors.dtype != torch.uint8:
        raise TypeError(f"{who}: colors must be uint8, got {colors.dtype}")
    if colors.dim() != 4 or colors.shape[0] != V or colors.shape[3] != 3 or not (1 <= colors.shape[1] <= FUSE_MAX_DIM and
                                                                                  1 <= colors.shape[2] <= FUSE_MAX_DIM):
        raise ValueError(f"{who}: colors must be [V = {V}, Hc, Wc, 3] with 1 .. {FUSE_MAX_DIM} a side, got {list(colors.shape)}")
    return colors.shape[1], colors.shape[2]


def _pow2_capacity(capacity, lo, hi, who, what=""):
    if int(capacity) != capacity or not lo <= capacity <= hi or capacity & (capacity - 1):
        raise ValueError(f"{who}: capacity must be a power of two in [{lo}, 2^{hi.bit_length() - 1}]{what}, got {capacity}")
    return int(capacity)


def _positive_f32(x, name, who):
    x32 = float(np.float32(x))
    if not (x32 > 0.0 and np.isfinite(x32)):
        raise ValueError(f"{who}: {name} must be positive and finite in fp32, got {x}")
    return x32


def fuse_workspace(capacity: int, device):
    """The caller-owned state of one fusion: an emptied table of `capacity` slots (a power of two) with zeroed counters, as a uint8
    device tensor (`sd3d_fuse_ws_bytes`, `sd3d_fuse_reset`).  Enqueues only."""
    lib = _lib.load()
    capacity = _pow2_capacity(capacity, FUSE_MIN_CAPACITY, FUSE_MAX_CAPACITY, "fuse_workspace")
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"fuse_workspace: expected the HIP device, got {device} (no CPU fallback)")
    ws = torch.empty(lib.sd3d_fuse_ws_bytes(int(capacity)), dtype=torch.uint8, device=device)
    fuse_reset(ws, capacity)
    return ws


def fuse_reset(ws, capacity: int):
    """Empties the table and zeroes the counters (`sd3d_fuse_reset`).  Enqueues only."""
    lib = _lib.load()
    _lib.check(lib.sd3d_fuse_reset(_ptr(ws, torch.uint8, "fuse_reset: ws"), ws.numel(), int(capacity), _stream()), "fuse_reset")


def fuse_accumulate(depth, depth_scale, intrinsics, cam_to_world, colors, ws, capacity: int, inv_voxel: float, stride=1, near=0.1, far=6.0,
                    edge_abs=0.02, edge_rel=0.02):
    """Steps 1 to 6 of the fusion rule for V views into the table of `ws` (`sd3d_fuse_accumulate`): depth uint16 [V, Hd, Wd] with
    `depth_scale` or fp32 metres, intrinsics fp32 [V, 4], cam_to_world fp32 [V, 3, 4], colors uint8 [V, Hc, Wc, 3]; `inv_voxel` is
    rounded to fp32 here; `edge_rel=None` turns the edge test off.  Enqueues only."""
    lib = _lib.load()
    who = "fuse_accumulate"
    u16, scale = _depth_arg(depth, depth_scale, who)
    V, Hd, Wd = depth.shape
    _want_shape(intrinsics, [(V, 4)], f"{who}: intrinsics")
    _want_shape(cam_to_world, [(V, 3, 4)], f"{who}: cam_to_world")
    Hc, Wc = _colors_arg(colors, V, who)
    if int(stride) != stride or not 1 <= stride <= FUSE_MAX_DIM:
        raise ValueError(f"{who}: stride must be an integer in [1, {FUSE_MAX_DIM}], got {stride}")
    rng = _range_args(near, far, edge_abs, edge_rel, who)
    inv32 = _positive_f32(inv_voxel, "inv_voxel", who)
    dp, ip = _ptr(depth, None, f"{who}: depth"), _ptr(intrinsics, torch.float32, f"{who}: intrinsics")
    cp, kp = _ptr(cam_to_world, torch.float32, f"{who}: cam_to_world"), _ptr(colors, torch.uint8, f"{who}: colors")
    wp = _ptr(ws, torch.uint8, f"{who}: ws")
    if V == 0:
        return
    _lib.check(lib.sd3d_fuse_accumulate(dp, u16, scale, ip, cp, kp, V, Hd, Wd, Hc, Wc, int(stride), *rng, inv32, wp, ws.numel(), int(capacity),
                                        _stream()), who)


def fuse_emit(ws, capacity: int, min_obs: int, out_cap: int, want_keys: bool = False):
    """Step 7 (`sd3d_fuse_emit`) -> (points fp32 [out_cap, 6], obs int32 [out_cap], keys int64 [out_cap] or None, info int64 [5] =
    FUSE_INFO on the device): the first min(info[0], out_cap) rows are written, in ascending key order.  Enqueues only."""
    lib = _lib.load()
    if int(min_obs) != min_obs or not 1 <= min_obs <= 0x7FFFFFFF:
        raise ValueError(f"fuse_emit: min_obs must be an integer >= 1, got {min_obs}")
    out_cap = int(out_cap)
    if out_cap < 0:
        raise ValueError(f"fuse_emit: out_cap >= 0, got {out_cap}")
    dev = ws.device
    points = torch.empty(out_cap, 6, dtype=torch.float32, device=dev)
    obs = torch.empty(out_cap, dtype=torch.int32, device=dev)
    keys = torch.empty(out_cap, dtype=torch.int64, device=dev) if want_keys else None
    info = torch.empty(len(FUSE_INFO), dtype=torch.int64, device=dev)
    _lib.check(lib.sd3d_fuse_emit(_ptr(ws, torch.uint8, "fuse_emit: ws"), ws.numel(), int(capacity), int(min_obs),
                                  _ptr(points) if out_cap else None, _ptr(obs) if out_cap else None,
                                  _ptr(keys) if want_keys and out_cap else None, out_cap, _ptr(info), _stream()), "fuse_emit")
    return points, obs, keys, info


# --------------------------------------------------------------------------------------------
# TSDF fusion and the surface-net mesh (csrc/tsdf.hip; the rule: include/segdino3d_hip.h, segdino3d_amd/tsdf.py)
# --------------------------------------------------------------------------------------------
TSDF_MIN_CAPACITY = 16
TSDF_MAX_CAPACITY = 1 << 20
TSDF_MAX_CALL_VIEWS = 64
TSDF_MAX_VERTICES = 1 << 26
TSDF_VOXEL_WORDS = 5
TSDF_INFO = ("vertices", "faces", "blocks", "voxels_observed", "updates", "out_of_range", "overflow")


def _tsdf_capacity(capacity, who):
    return _pow2_capacity(capacity, TSDF_MIN_CAPACITY, TSDF_MAX_CAPACITY, who, " (blocks of 8 x 8 x 8 voxels)")


def tsdf_workspace(capacity: int, device):
    """The caller-owned state of one volume: an emptied block table of `capacity` blocks (a power of two) with zeroed voxels and
    counters, as a uint8 device tensor (`sd3d_tsdf_ws_bytes`, `sd3d_tsdf_reset`).  Enqueues only."""
    lib = _lib.load()
    capacity = _tsdf_capacity(capacity, "tsdf_workspace")
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"tsdf_workspace: expected the HIP device, got {device} (no CPU fallback)")
    ws = torch.empty(lib.sd3d_tsdf_ws_bytes(capacity), dtype=torch.uint8, device=device)
    tsdf_reset(ws, capacity)
    return ws


def tsdf_reset(ws, capacity: int):
    """Empties the block table and zeroes the voxels and the counters (`sd3d_tsdf_reset`).  Enqueues only."""
    lib = _lib.load()
    _lib.check(lib.sd3d_tsdf_reset(_ptr(ws, torch.uint8, "tsdf_reset: ws"), ws.numel(), _tsdf_capacity(capacity, "tsdf_reset"), _stream()),
               "tsdf_reset")


def tsdf_state_views(ws, capacity: int):
    """The parts of a volume's workspace as views of it, by the layout include/segdino3d_hip.h gives: (counters int64 [7], block keys
    int64 [capacity], voxels int32 [capacity, 5, 512])."""
    capacity = _tsdf_capacity(capacity, "tsdf_state_views")
    up = lambda n: -(-n // 256) * 256                                                    # noqa: E731
    o_keys = up(7 * 8)
    o_vox = o_keys + 2 * up(capacity * 8) + up(capacity * 4)
    n_vox = capacity * TSDF_VOXEL_WORDS * 512 * 4
    if ws.dtype != torch.uint8 or ws.numel() < o_vox + n_vox:
        raise RuntimeError("tsdf_state_views: workspace too small (sd3d_tsdf_ws_bytes)")
    return (ws[:56].view(torch.int64), ws[o_keys:o_keys + capacity * 8].view(torch.int64),
            ws[o_vox:o_vox + n_vox].view(torch.int32).view(capacity, TSDF_VOXEL_WORDS, 512))


def _tsdf_depth(depth, depth_scale, who):
    """`_depth_arg` and the view limit of one touch / integrate call (a bit per view in the `touched` words)."""
    u16, scale = _depth_arg(depth, depth_scale, who)
    if depth.shape[0] > TSDF_MAX_CALL_VIEWS:
        raise ValueError(f"{who}: at most {TSDF_MAX_CALL_VIEWS} views a call, got {depth.shape[0]}")
    return u16, scale


def tsdf_touch(depth, depth_scale, intrinsics, cam_to_world, ws, capacity: int, inv_voxel: float, half_step: float, near=0.1, far=6.0,
               edge_abs=0.02, edge_rel=0.02):
    """Steps 1 and 2 of the TSDF rule for V <= 64 views (`sd3d_tsdf_touch`): marks the blocks each view touches in the table of `ws`
    and -> vdepth fp32 [V, Hd, Wd], the depth of each valid pixel and 0 elsewhere, for `tsdf_integrate` of the same views.
    `inv_voxel` and `half_step` (= trunc / 2) are rounded to fp32 here; `edge_rel=None` turns the edge test off.  Enqueues only."""
    lib = _lib.load()
    who = "tsdf_touch"
    u16, scale = _tsdf_depth(depth, depth_scale, who)
    V, Hd, Wd = depth.shape
    _want_shape(intrinsics, [(V, 4)], f"{who}: intrinsics")
    _want_shape(cam_to_world, [(V, 3, 4)], f"{who}: cam_to_world")
    rng = _range_args(near, far, edge_abs, edge_rel, who)
    inv32, h32 = _positive_f32(inv_voxel, "inv_voxel", who), _positive_f32(half_step, "half_step", who)
    dp, ip = _ptr(depth, None, f"{who}: depth"), _ptr(intrinsics, torch.float32, f"{who}: intrinsics")
    cp, wp = _ptr(cam_to_world, torch.float32, f"{who}: cam_to_world"), _ptr(ws, torch.uint8, f"{who}: ws")
    vdepth = torch.empty(V, Hd, Wd, dtype=torch.float32, device=depth.device)
    _lib.check(lib.sd3d_tsdf_touch(dp if V else None, u16, scale, ip if V else None, cp if V else None, V, Hd, Wd, *rng, inv32, h32,
                                   _ptr(vdepth) if V else None, wp, ws.numel(), _tsdf_capacity(capacity, who), _stream()), who)
    return vdepth


def tsdf_integrate(vdepth, intrinsics, world_to_cam, colors, ws, capacity: int, voxel: float, trunc: float, qscale: float):
    """Step 3 of the TSDF rule (`sd3d_tsdf_integrate`) for the views of the `tsdf_touch` that made `vdepth` fp32 [V, Hd, Wd]:
    intrinsics fp32 [V, 4], world_to_cam fp32 [V, 3, 4], colors uint8 [V, Hc, Wc, 3]; `voxel`, `trunc` and `qscale` (= 4096 / trunc) are
    rounded to fp32 here.  Enqueues only."""
    lib = _lib.load()
    who = "tsdf_integrate"
    u16, _ = _tsdf_depth(vdepth, None, who)
    if u16:
        raise TypeError(f"{who}: vdepth must be the fp32 output of tsdf_touch")
    V, Hd, Wd = vdepth.shape
    _want_shape(intrinsics, [(V, 4)], f"{who}: intrinsics")
    _want_shape(world_to_cam, [(V, 3, 4)], f"{who}: world_to_cam")
    Hc, Wc = _colors_arg(colors, V, who)
    v32, t32, q32 = _positive_f32(voxel, "voxel", who), _positive_f32(trunc, "trunc", who), _positive_f32(qscale, "qscale", who)
    if not t32 >= v32:
        raise ValueError(f"{who}: need voxel <= trunc, got {voxel}, {trunc}")
    dp, ip = _ptr(vdepth, torch.float32, f"{who}: vdepth"), _ptr(intrinsics, torch.float32, f"{who}: intrinsics")
    mp, kp = _ptr(world_to_cam, torch.float32, f"{who}: world_to_cam"), _ptr(colors, torch.uint8, f"{who}: colors")
    wp = _ptr(ws, torch.uint8, f"{who}: ws")
    if V == 0:
        return
    _lib.check(lib.sd3d_tsdf_integrate(dp, ip, mp, kp, V, Hd, Wd, Hc, Wc, v32, t32, q32, wp, ws.numel(), _tsdf_capacity(capacity, who),
                                       _stream()), who)


def tsdf_mesh(ws, capacity: int, min_weight: int, voxel: float, max_vertices: int, want_keys: bool = False):
    """Steps 4 to 6 of the TSDF rule (`sd3d_tsdf_mesh`) -> (vertices fp32 [max_vertices, 6], keys int64 [max_vertices] or None, faces
    int32 [6 * max_vertices, 3], info int64 [7] = TSDF_INFO on the device): the first min(info[0], max_vertices) vertices and the
    first info[1] faces are written.  The volume is left as it is.  Enqueues only."""
    lib = _lib.load()
    who = "tsdf_mesh"
    if int(min_weight) != min_weight or not 1 <= min_weight <= 0x7FFFFFFF:
        raise ValueError(f"{who}: min_weight must be an integer >= 1, got {min_weight}")
    if int(max_vertices) != max_vertices or not 1 <= max_vertices <= TSDF_MAX_VERTICES:
        raise ValueError(f"{who}: max_vertices must be an integer in [1, 2^26], got {max_vertices}")
    max_vertices = int(max_vertices)
    v32 = _positive_f32(voxel, "voxel", who)
    wp = _ptr(ws, torch.uint8, f"{who}: ws")
    dev = ws.device
    scratch = torch.empty(lib.sd3d_tsdf_mesh_ws_bytes(max_vertices), dtype=torch.uint8, device=dev)
    vertices = torch.empty(max_vertices, 6, dtype=torch.float32, device=dev)
    keys = torch.empty(max_vertices, dtype=torch.int64, device=dev) if want_keys else None
    faces = torch.empty(6 * max_vertices, 3, dtype=torch.int32, device=dev)
    info = torch.empty(len(TSDF_INFO), dtype=torch.int64, device=dev)
    _lib.check(lib.sd3d_tsdf_mesh(wp, ws.numel(), _tsdf_capacity(capacity, who), int(min_weight), v32, max_vertices, scratch.data_ptr(),
                                  scratch.numel(), _ptr(vertices), _ptr(keys) if want_keys else None, _ptr(faces), _ptr(info), _stream()),
               who)
    return vertices, keys, faces, info


# --------------------------------------------------------------------------------------------
# camera tracking against the TSDF volume (csrc/track.hip; the rule: include/segdino3d_hip.h, segdino3d_amd/track.py)
# --------------------------------------------------------------------------------------------
TRACK_SUMS = 29
TRACK_INFO = ("lost", "count", "e")
TRACK_MAX_STRIDE = 16384


def track_state(device):
    """The caller-owned state of one tracker (`sd3d_track_state_bytes`), zeroed, as a uint8 device tensor; `track_pose_view` is the
    pose inside it.  Enqueues only."""
    lib = _lib.load()
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"track_state: expected the HIP device, got {device} (no CPU fallback)")
    return torch.zeros(lib.sd3d_track_state_bytes(), dtype=torch.uint8, device=device)


def track_pose_view(state):
    """The current cam_to_world float64 [3, 4] of a tracker's state, as a view of it: the caller writes the first pose here."""
    if not isinstance(state, torch.Tensor) or state.dtype != torch.uint8 or state.dim() != 1 or state.numel() < 96:
        raise TypeError("track_pose_view: state must be the uint8 tensor of track_state")
    return state[:96].view(torch.float64).view(3, 4)


def track_sums_view(state):
    """The 29 integer sums of the last iteration that ran (A: 21, the upper triangle row-major; b: 6; count; e) as an int64 [29] view
    of a tracker's state: for inspection and the tests."""
    if not isinstance(state, torch.Tensor) or state.dtype != torch.uint8 or state.dim() != 1 or state.numel() < (64 + TRACK_SUMS) * 8:
        raise TypeError("track_sums_view: state must be the uint8 tensor of track_state")
    return state[512:512 + TRACK_SUMS * 8].view(torch.int64)


def track_begin(state):
    """Opens a frame (`sd3d_track_begin`): remembers the pose, clears `lost` and the sums.  Enqueues only."""
    lib = _lib.load()
    _lib.check(lib.sd3d_track_begin(_ptr(state, torch.uint8, "track_begin: state"), state.numel(), _stream()), "track_begin")


def track_iterate(depth, depth_scale, intrinsics, state, ws, capacity: int, stride: int, inv_voxel: float, voxel: float, ymax: float,
                  track_min_weight: int = 1, min_samples: int = 64, damping: float = 1e-6, max_rot: float = 0.5, max_trans: float = 0.32,
                  near=0.1, far=6.0, edge_abs=0.02, edge_rel=0.02):
    """One iteration of the tracking rule (`sd3d_track_iterate`) for ONE frame - depth uint16 [Hd, Wd] with `depth_scale` or fp32
    metres, intrinsics fp32 [4] - against the volume in `ws` (read only): the accumulate launch and the one-lane solve + update.  The
    float parameters are rounded to fp32 here.  Enqueues only."""
    lib = _lib.load()
    who = "track_iterate"
    u16, scale = _depth_arg(depth, depth_scale, who, dims=2)
    Hd, Wd = depth.shape
    _want_shape(intrinsics, [(4,)], f"{who}: intrinsics")
    if int(stride) != stride or not 1 <= stride <= TRACK_MAX_STRIDE:
        raise ValueError(f"{who}: stride must be an integer in [1, {TRACK_MAX_STRIDE}], got {stride}")
    rng = _range_args(near, far, edge_abs, edge_rel, who)
    if int(track_min_weight) != track_min_weight or not 1 <= track_min_weight <= 0x7FFFFFFF:
        raise ValueError(f"{who}: track_min_weight must be an integer >= 1, got {track_min_weight}")
    if int(min_samples) != min_samples or not 1 <= min_samples <= 0x7FFFFFFF:
        raise ValueError(f"{who}: min_samples must be an integer >= 1, got {min_samples}")
    if not 0.0 <= float(damping) <= 1.0:
        raise ValueError(f"{who}: damping must lie in [0, 1], got {damping}")
    inv32, v32, y32 = _positive_f32(inv_voxel, "inv_voxel", who), _positive_f32(voxel, "voxel", who), _positive_f32(ymax, "ymax", who)
    r32, t32 = _positive_f32(max_rot, "max_rot", who), _positive_f32(max_trans, "max_trans", who)
    samples = -(-Hd // int(stride)) * -(-Wd // int(stride))
    jq = 4096.0 * (y32 * inv32) * 1.001 + 2.0
    if not (jq < 2.0 ** 31 and jq * jq * samples < 9.0e18):
        raise ValueError(f"{who}: (4096 ymax inv_voxel + 2)^2 * samples must stay below 2^63 (the int64 sums), got ymax = {ymax}, "
                         f"inv_voxel = {inv_voxel}, {samples} samples")
    dp, ip = _ptr(depth, None, f"{who}: depth"), _ptr(intrinsics, torch.float32, f"{who}: intrinsics")
    sp, wp = _ptr(state, torch.uint8, f"{who}: state"), _ptr(ws, torch.uint8, f"{who}: ws")
    _lib.check(lib.sd3d_track_iterate(dp, u16, scale, ip, Hd, Wd, int(stride), *rng, inv32, v32, y32, int(track_min_weight), int(min_samples),
                                      float(np.float32(damping)), r32, t32, sp, state.numel(), wp, ws.numel(), _tsdf_capacity(capacity, who),
                                      _stream()), who)


def track_end(state, pose=None, cam_to_world=None, world_to_cam=None, info=None):
    """Closes a frame (`sd3d_track_end`) -> (pose float64 [3, 4], NaN when lost; cam_to_world and world_to_cam fp32 [3, 4] as
    `tsdf_touch` / `tsdf_integrate` take them; info int64 [3] = TRACK_INFO), written into the given tensors or into new ones.  A lost
    frame puts the state's pose back.  Enqueues only."""
    lib = _lib.load()
    who = "track_end"
    sp = _ptr(state, torch.uint8, f"{who}: state")
    dev = state.device
    pose = torch.empty(3, 4, dtype=torch.float64, device=dev) if pose is None else pose
    cam_to_world = torch.empty(3, 4, dtype=torch.float32, device=dev) if cam_to_world is None else cam_to_world
    world_to_cam = torch.empty(3, 4, dtype=torch.float32, device=dev) if world_to_cam is None else world_to_cam
    info = torch.empty(len(TRACK_INFO), dtype=torch.int64, device=dev) if info is None else info
    for t, name in ((pose, "pose"), (cam_to_world, "cam_to_world"), (world_to_cam, "world_to_cam")):
        _want_shape(t, [(3, 4)], f"{who}: {name}")
    _want_shape(info, [(len(TRACK_INFO),)], f"{who}: info")
    _lib.check(lib.sd3d_track_end(sp, state.numel(), _ptr(pose, torch.float64, f"{who}: pose"),
                                  _ptr(cam_to_world, torch.float32, f"{who}: cam_to_world"),
                                  _ptr(world_to_cam, torch.float32, f"{who}: world_to_cam"), _ptr(info, torch.int64, f"{who}: info"),
                                  _stream()), who)
    return pose, cam_to_world, world_to_cam, info


# --------------------------------------------------------------------------------------------
# nearest point: results of a forward carried onto other points and onto frames (csrc/transfer.hip; the rule: include/segdino3d_hip.h,
# segdino3d_amd/transfer.py)
# --------------------------------------------------------------------------------------------
NEAREST_MAX_LABELS = 8


def _nearest_radius(radius, who):
    if not (np.isfinite(radius) and 0 < radius <= KNN_MAX_RADIUS):
        raise ValueError(f"{who}: radius must lie in (0, {KNN_MAX_RADIUS}], got {radius}")
    return float(radius)


def point_index_build(points, radius: float):
    """The grid of `knn_graph` over one cloud (`sd3d_point_index_build`): points fp32 [N, 3] -> the caller-owned index, a uint8 device
    tensor that `nearest_points` / `nearest_pixels` read with the same `N` and `radius`.  Enqueues only."""
    lib = _lib.load()
    who = "point_index_build"
    radius = _nearest_radius(radius, who)
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError(f"{who}: points must be fp32 [N, 3], got {points.dtype} {list(points.shape)}")
    N = points.shape[0]
    if N >= 1 << 31:
        raise ValueError(f"{who}: need N < 2^31, got {N}")
    pp = _ptr(points, torch.float32, f"{who}: points")
    ws = torch.empty(lib.sd3d_point_index_ws_bytes(N), dtype=torch.uint8, device=points.device)
    _lib.check(lib.sd3d_point_index_build(pp if N else None, N, radius, ws.data_ptr(), ws.numel(), _stream()), who)
    return ws


def _nearest_outputs(shape, N, labels, fill, return_index, return_d2, dev, who):
    """-> (L, labels pointer, fill, idx, d2, out): the optional outputs of one query call over `shape` queries."""
    L = 0
    if labels is not None:
        if labels.dim() != 2 or labels.shape[1] != N or not 1 <= labels.shape[0] <= NEAREST_MAX_LABELS:
            raise ValueError(f"{who}: labels must be int32 [L, N = {N}] with 1 <= L <= {NEAREST_MAX_LABELS}, got {list(labels.shape)}")
        L = labels.shape[0]
    if int(fill) != fill or not -(1 << 31) <= fill < 1 << 31:
        raise ValueError(f"{who}: fill must be an int32, got {fill}")
    lp = _ptr(labels, torch.int32, f"{who}: labels") if L else None
    idx = torch.empty(shape, dtype=torch.int32, device=dev) if return_index else None
    d2 = torch.empty(shape, dtype=torch.float32, device=dev) if return_d2 else None
    out = torch.empty((L,) + tuple(shape), dtype=torch.int32, device=dev) if L else None
    return L, lp, int(fill), idx, d2, out


def nearest_points(queries, index, n_points: int, radius: float, labels=None, fill: int = -1, return_index: bool = True,
                   return_d2: bool = False):
    """The nearest source point within `radius` of each query (`sd3d_nearest_points`): queries fp32 [M, 3], `index` from
    `point_index_build`, labels int32 [L, N] or None -> (idx int32 [M] or None, d2 fp32 [M] or None, out int32 [L, M] or None).
    Enqueues only."""
    lib = _lib.load()
    who = "nearest_points"
    radius = _nearest_radius(radius, who)
    if queries.dim() != 2 or queries.shape[1] != 3 or queries.dtype != torch.float32:
        raise ValueError(f"{who}: queries must be fp32 [M, 3], got {queries.dtype} {list(queries.shape)}")
    M, N = queries.shape[0], int(n_points)
    if M >= 1 << 31:
        raise ValueError(f"{who}: need M < 2^31, got {M}")
    qp, wp = _ptr(queries, torch.float32, f"{who}: queries"), _ptr(index, torch.uint8, f"{who}: index")
    L, lp, fill, idx, d2, out = _nearest_outputs((M,), N, labels, fill, return_index, return_d2, queries.device, who)
    if M:
        _lib.check(lib.sd3d_nearest_points(qp, M, wp, index.numel(), N, radius, lp if N else None, L, fill, _ptr(idx), _ptr(d2), _ptr(out),
                                           _stream()), who)
    return idx, d2, out


def nearest_pixels(depth, depth_scale, intrinsics, cam_to_world, index, n_points: int, radius: float, labels=None, fill: int = -1,
                   return_index: bool = True, return_d2: bool = False, near=0.1, far=6.0):
    """The nearest source point within `radius` of each back-projected depth pixel (`sd3d_nearest_pixels`): depth uint16 [V, Hd, Wd] with
    `depth_scale` or fp32 metres, intrinsics fp32 [V, 4], cam_to_world fp32 [V, 3, 4] -> (idx int32 [V, Hd, Wd] or None, d2 fp32
    [V, Hd, Wd] or None, out int32 [L, V, Hd, Wd] or None).  One launch; enqueues only."""
    lib = _lib.load()
    who = "nearest_pixels"
    radius = _nearest_radius(radius, who)
    u16, scale = _depth_arg(depth, depth_scale, who)
    V, Hd, Wd = depth.shape
    _want_shape(intrinsics, [(V, 4)], f"{who}: intrinsics")
    _want_shape(cam_to_world, [(V, 3, 4)], f"{who}: cam_to_world")
    near, far = _range_args(near, far, None, None, who)[:2]
    N = int(n_points)
    dp, ip = _ptr(depth, None, f"{who}: depth"), _ptr(intrinsics, torch.float32, f"{who}: intrinsics")
    cp, wp = _ptr(cam_to_world, torch.float32, f"{who}: cam_to_world"), _ptr(index, torch.uint8, f"{who}: index")
    L, lp, fill, idx, d2, out = _nearest_outputs((V, Hd, Wd), N, labels, fill, return_index, return_d2, depth.device, who)
    if V:
        _lib.check(lib.sd3d_nearest_pixels(dp, u16, scale, ip, cp, V, Hd, Wd, near, far, wp, index.numel(), N, radius,
                                           lp if N else None, L, fill, _ptr(idx), _ptr(d2), _ptr(out), _stream()), who)
    return idx, d2, out


def instance_map(masks, scores, score_thr: float = 0.0):
    """Overlapping instance masks as one map (`sd3d_instance_map`): masks bool / uint8 [I, N], scores fp32 [I] -> int32 [N], per point
    the instance of the largest score >= `score_thr` whose mask holds it (ties: the lower index), -1 if none.  Enqueues only."""
    lib = _lib.load()
    who = "instance_map"
    if masks.dim() != 2 or masks.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"{who}: masks must be bool or uint8 [I, N], got {masks.dtype} {list(masks.shape)}")
    I, N = masks.shape
    if scores.dtype != torch.float32 or tuple(scores.shape) != (I,):
        raise TypeError(f"{who}: scores must be fp32 [I = {I}], got {scores.dtype} {list(scores.shape)}")
    if score_thr != score_thr:
        raise ValueError(f"{who}: score_thr must not be a NaN")
    if N >= 1 << 31:
        raise ValueError(f"{who}: need N < 2^31, got {N}")
    mp, sp = _ptr(masks, None, f"{who}: masks"), _ptr(scores, torch.float32, f"{who}: scores")
    out = torch.empty(N, dtype=torch.int32, device=masks.device)
    if N:
        _lib.check(lib.sd3d_instance_map(mp if I else None, sp if I else None, I, N, float(score_thr), _ptr(out), _stream()), who)
    return out


# --------------------------------------------------------------------------------------------
# mesh rasteriser: a triangle mesh drawn into posed views (csrc/raster.hip; the rule: include/segdino3d_hip.h, segdino3d_amd/raster.py)
# --------------------------------------------------------------------------------------------
RASTER_MAX_LABELS = 8
RASTER_SMALL_MAX_PIXELS = 64     # SD3D_RASTER_SMALL_MAX_PIXELS: up to this clamped bounding-box area one lane draws a face, above it one wave
RASTER_MAX_DIM = 16384
RASTER_INFO = ("drawn", "near", "guard", "empty", "bad", "pixels")
_WS_RASTER = _PerThread()        # raster_views: the key buffer of one pass, its records and their counts


def raster_views(vertices, faces, world_to_cam, intrinsics, height: int, width: int, near=0.1, far=6.0, views_per_pass: int = 32,
                 face_labels=None, vertex_labels=None, fill: int = -1, return_depth: bool = True, return_face: bool = True,
                 return_vertex: bool = False):
    """A mesh drawn into V posed views (`sd3d_raster_views`): vertices fp32 [Nv, 3], faces int32 [F, 3], world_to_cam fp32 [V, 3, 4],
    intrinsics fp32 [V, 4], face_labels int32 [Lf, F] or None, vertex_labels int32 [Lv, Nv] or None -> (depth fp32 [V, H, W] or None,
    face int32 [V, H, W] or None, vertex int32 [V, H, W] or None, face label images int32 [Lf, V, H, W] or None, vertex label images
    int32 [Lv, V, H, W] or None, info int64 [len(RASTER_INFO)]).  Enqueues only."""
    lib = _lib.load()
    who = "raster_views"
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise ValueError(f"{who}: vertices must be fp32 [Nv, 3], got {vertices.dtype} {list(vertices.shape)}")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"{who}: faces must be int32 [F, 3], got {faces.dtype} {list(faces.shape)}")
    Nv, F, V, H, W = vertices.shape[0], faces.shape[0], world_to_cam.shape[0], int(height), int(width)
    if Nv >= 1 << 31 or F >= 1 << 31:
        raise ValueError(f"{who}: need Nv, F < 2^31, got {Nv}, {F}")
    if not (1 <= H <= RASTER_MAX_DIM and 1 <= W <= RASTER_MAX_DIM):
        raise ValueError(f"{who}: images must be 1 .. {RASTER_MAX_DIM} a side, got {H} x {W}")
    _want_shape(world_to_cam, [(V, 3, 4)], f"{who}: world_to_cam")
    _want_shape(intrinsics, [(V, 4)], f"{who}: intrinsics")
    if not (float(near) > 0.0 and float(far) >= float(near)):
        raise ValueError(f"{who}: need 0 < near <= far, got near = {near}, far = {far}")
    if int(views_per_pass) != views_per_pass or views_per_pass < 1:
        raise ValueError(f"{who}: views_per_pass must be an integer >= 1, got {views_per_pass}")
    if int(fill) != fill or not -(1 << 31) <= fill < 1 << 31:
        raise ValueError(f"{who}: fill must be an int32, got {fill}")
    Lf = Lv = 0
    if face_labels is not None:
        _want_shape(face_labels, [(face_labels.shape[0], F)], f"{who}: face_labels")
        Lf = face_labels.shape[0]
    if vertex_labels is not None:
        _want_shape(vertex_labels, [(vertex_labels.shape[0], Nv)], f"{who}: vertex_labels")
        Lv = vertex_labels.shape[0]
    if Lf + Lv > RASTER_MAX_LABELS:
        raise ValueError(f"{who}: at most {RASTER_MAX_LABELS} label channels in one call, got {Lf} + {Lv}")
    dev = vertices.device
    vp, fp = _ptr(vertices, torch.float32, f"{who}: vertices"), _ptr(faces, torch.int32, f"{who}: faces")
    cp, ip = _ptr(world_to_cam, torch.float32, f"{who}: world_to_cam"), _ptr(intrinsics, torch.float32, f"{who}: intrinsics")
    flp = _ptr(face_labels, torch.int32, f"{who}: face_labels") if Lf else None
    vlp = _ptr(vertex_labels, torch.int32, f"{who}: vertex_labels") if Lv else None
    shape = (V, H, W)
    depth = torch.empty(shape, dtype=torch.float32, device=dev) if return_depth else None
    face = torch.empty(shape, dtype=torch.int32, device=dev) if return_face else None
    vertex = torch.empty(shape, dtype=torch.int32, device=dev) if return_vertex else None
    fout = torch.empty((Lf,) + shape, dtype=torch.int32, device=dev) if Lf else None
    vout = torch.empty((Lv,) + shape, dtype=torch.int32, device=dev) if Lv else None
    info = torch.zeros(len(RASTER_INFO), dtype=torch.int64, device=dev)
    if V:
        per_pass = min(int(views_per_pass), V)
        need = lib.sd3d_raster_ws_bytes(F, per_pass, H, W)
        if need == 0:
            raise ValueError(f"{who}: views_per_pass * F must stay below 2^31, got {per_pass} * {F}; lower views_per_pass")
        ws = _WS_RASTER.get(need, dev)
        _lib.check(lib.sd3d_raster_views(vp if Nv else None, Nv, fp if F else None, F, cp, ip, V, H, W, float(near), float(far), per_pass,
                                         flp if F else None, Lf, vlp if Nv else None, Lv, int(fill), _ptr(depth), _ptr(face), _ptr(vertex),
                                         _ptr(fout), _ptr(vout), _ptr(info), ws.data_ptr(), ws.numel(), _stream()), who)
    return depth, face, vertex, fout, vout, info


# --------------------------------------------------------------------------------------------
# mesh decimation: vertex clustering on a grid (csrc/simplify.hip; the rule: include/segdino3d_hip.h, segdino3d_amd/simplify.py)
# --------------------------------------------------------------------------------------------
SIMPLIFY_MAX_CHANNELS = 11
SIMPLIFY_MAX_INV_CELL = 64.0     # cell >= 2^-6: with |x| < 2^14 every cell index fits 21 bits
SIMPLIFY_MAX_CELLS = 1 << 21     # the oriented triple of a face packs into one 63-bit sort key
SIMPLIFY_INFO = ("vertices", "faces", "bad_vertices", "bad_faces", "collapsed", "duplicates", "unreferenced")
_WS_SIMPLIFY = _PerThread()      # simplify_mesh: the sort buffers, the per-cell sums and the flags of one call


def simplify_mesh(vertices, faces, inv_cell: float, nearest: bool = False, keep_unreferenced: bool = True):
    """A mesh clustered on a grid (`sd3d_simplify_mesh`): vertices fp32 [V, C] with 3 <= C <= 11, faces int32 [F, 3], `inv_cell` =
    1 / cell -> (vertices fp32 [V, C], faces int32 [F, 3] and face_source int32 [F] at capacity, vertex_map int32 [V], info int64
    [len(SIMPLIFY_INFO)] on the device): the first info[0] vertices and the first info[1] faces are written.  Enqueues only."""
    lib = _lib.load()
    who = "simplify_mesh"
    if vertices.dim() != 2 or vertices.dtype != torch.float32 or not 3 <= vertices.shape[1] <= SIMPLIFY_MAX_CHANNELS:
        raise ValueError(f"{who}: vertices must be fp32 [V, C] with 3 <= C <= {SIMPLIFY_MAX_CHANNELS}, got {vertices.dtype} {list(vertices.shape)}")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"{who}: faces must be int32 [F, 3], got {faces.dtype} {list(faces.shape)}")
    V, C, F = vertices.shape[0], vertices.shape[1], faces.shape[0]
    if V >= 1 << 31 or F >= 1 << 31:
        raise ValueError(f"{who}: need V, F < 2^31, got {V}, {F}")
    inv32 = _positive_f32(inv_cell, "inv_cell", who)
    if inv32 > SIMPLIFY_MAX_INV_CELL:
        raise ValueError(f"{who}: inv_cell must be at most {SIMPLIFY_MAX_INV_CELL} (cell >= 2^-6), got {inv_cell}")
    dev = vertices.device
    vp, fp = _ptr(vertices, torch.float32, f"{who}: vertices"), _ptr(faces, torch.int32, f"{who}: faces")
    vout = torch.empty(V, C, dtype=torch.float32, device=dev)
    fout = torch.empty(F, 3, dtype=torch.int32, device=dev)
    vmap = torch.empty(V, dtype=torch.int32, device=dev)
    fsrc = torch.empty(F, dtype=torch.int32, device=dev)
    info = torch.zeros(len(SIMPLIFY_INFO), dtype=torch.int64, device=dev)
    need = lib.sd3d_simplify_ws_bytes(V, F, C)
    if need == 0:
        raise ValueError(f"{who}: a mesh of {V} vertices and {F} faces does not fit the workspace sizes")
    ws = _WS_SIMPLIFY.get(need, dev)
    _lib.check(lib.sd3d_simplify_mesh(vp if V else None, V, C, fp if F else None, F, inv32, int(bool(nearest)), int(bool(keep_unreferenced)),
                                      _ptr(vout) if V else None, _ptr(fout) if F else None, _ptr(vmap) if V else None,
                                      _ptr(fsrc) if F else None, _ptr(info), ws.data_ptr(), ws.numel(), _stream()), who)
    return vout, fout, vmap, fsrc, info


# --------------------------------------------------------------------------------------------
# connected components and the clean (csrc/components.hip; the rule: include/segdino3d_hip.h, segdino3d_amd/components.py)
# --------------------------------------------------------------------------------------------
COMPONENTS_MAX_CHANNELS = 11
COMPONENTS_SOURCES = ("faces", "edges", "table")        # SD3D_COMPONENTS_FACES, _EDGES, _TABLE
COMPONENTS_INFO = ("components", "kept", "nodes", "links", "bad_nodes", "bad_links", "isolated", "unsettled")
_WS_COMPONENTS = _PerThread()    # components: the sort buffers, the union-find and the flags of one call


def components(source: str, links, n: int, coords=None, min_nodes: int = 0, min_links: int = 0, min_extent: float = 0.0, keep_largest: int = 0,
               clean: bool = False):
    """The components of `n` nodes under `links` (`sd3d_components`): source "faces" int32 [F, 3], "edges" int32 [E, 2] or "table" int32
    [n, k]; `coords` fp32 [n, C] with 3 <= C <= 11 or None (the graph form) -> a dict of device tensors at capacity: labels int32 [n],
    n_nodes and n_links int32 [n], box fp32 [n, 6], keep uint8 [n], info int64 [len(COMPONENTS_INFO)] (the first info[0] components are
    written), and with `clean` nodes fp32 [n, C] (None without coords), node_map int32 [n], links (the shape of `links`), link_source
    int32 [rows] (None for a table), labels_out int32 [n]: the first info[2] nodes and info[3] links are written (a table: info[2]
    rows).  Enqueues only."""
    lib = _lib.load()
    who = "components"
    if source not in COMPONENTS_SOURCES:
        raise ValueError(f"{who}: source must be one of {COMPONENTS_SOURCES}, got {source!r}")
    src = COMPONENTS_SOURCES.index(source)
    if links.dim() != 2 or links.dtype != torch.int32 or (src == 0 and links.shape[1] != 3) or (src == 1 and links.shape[1] != 2) or \
            (src == 2 and (links.shape[0] != n or links.shape[1] < 1)):
        raise ValueError(f"{who}: links must be int32 [F, 3] (faces), [E, 2] (edges) or [n, k] (table), got {links.dtype} {list(links.shape)} as {source} with n = {n}")
    if coords is not None and (coords.dim() != 2 or coords.dtype != torch.float32 or coords.shape[0] != n or not 3 <= coords.shape[1] <= COMPONENTS_MAX_CHANNELS):
        raise ValueError(f"{who}: coords must be fp32 [n, C] with 3 <= C <= {COMPONENTS_MAX_CHANNELS}, got {coords.dtype} {list(coords.shape)}")
    rows, width = links.shape
    L = rows * width if src == 2 else rows
    if n < 0 or n >= 1 << 31 or L >= 1 << 31:
        raise ValueError(f"{who}: need 0 <= n < 2^31 and fewer than 2^31 links, got {n} nodes, {L} links")
    min_extent32 = float(np.float32(min_extent))
    if min_nodes < 0 or min_links < 0 or keep_largest < 0 or not (min_extent32 >= 0.0 and np.isfinite(min_extent32)):
        raise ValueError(f"{who}: min_nodes, min_links, keep_largest must be >= 0 and min_extent finite and >= 0, got {min_nodes}, {min_links}, "
                         f"{keep_largest}, {min_extent}")
    dev = links.device
    lp = _ptr(links, torch.int32, f"{who}: links")
    cp = _ptr(coords, torch.float32, f"{who}: coords")
    C = coords.shape[1] if coords is not None else 0
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    out = dict(labels=new((n,), torch.int32), n_nodes=new((n,), torch.int32), n_links=new((n,), torch.int32), box=new((n, 6), torch.float32),
               keep=new((n,), torch.uint8), info=torch.zeros(len(COMPONENTS_INFO), dtype=torch.int64, device=dev),
               nodes=None, node_map=None, links=None, link_source=None, labels_out=None)
    if clean:
        out.update(nodes=new((n, C), torch.float32) if coords is not None else None, node_map=new((n,), torch.int32),
                   links=new((rows, width), torch.int32), link_source=new((rows,), torch.int32) if src != 2 else None,
                   labels_out=new((n,), torch.int32))
    need = lib.sd3d_components_ws_bytes(n, L, width, C)
    if need == 0:
        raise ValueError(f"{who}: {n} nodes and {L} links do not fit the workspace sizes")
    ws = _WS_COMPONENTS.get(need, dev)
    opt = lambda t, live: _ptr(t) if (t is not None and live) else None
    _lib.check(lib.sd3d_components(src, lp if L else None, L, width, cp if n else None, n, C if n else 0, int(min_nodes), int(min_links), min_extent32,
                                   int(keep_largest), opt(out["labels"], n), opt(out["n_nodes"], n), opt(out["n_links"], n), opt(out["box"], n),
                                   opt(out["keep"], n), opt(out["nodes"], n), opt(out["node_map"], n), opt(out["links"], L),
                                   opt(out["link_source"], L), opt(out["labels_out"], n), _ptr(out["info"]), ws.data_ptr(), ws.numel(), _stream()), who)
    return out
