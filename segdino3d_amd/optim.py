"""The parameter update of a training iteration on the device: `clip_grad_norm_` + `AdamW.step()` + `ModelEma.update()` of the
reference loop (`engine/train_engine_3d.py:99-120`) as three multi-tensor HIP kernels (csrc/optim.hip) instead of a few launches
per parameter tensor.

* `FusedAdamW` is a `torch.optim.AdamW`: same `param_groups`, same `state` (`step`, `exp_avg`, `exp_avg_sq`), so LR schedulers drive
  it and `state_dict()` / `load_state_dict()` interchange with torch's class.  Only `step()` differs: one table of every parameter
  that has a gradient, one launch for the gradient norm (when `max_norm > 0`), one for the update.
* `fuse(optimizer)` wraps an existing `torch.optim.AdamW` (groups and state shared).
* `ModelEma` has the surface of the reference's `utils/ema_utils.ModelEma`; `update()` is one launch, or no launch at all when it is
  attached to the optimizer (`FusedAdamW.attach_ema`), whose step then writes the average in the same pass.

The LR schedule, checkpoint I/O and DDP stay torch's.  There is no CPU fallback and no fallback to torch's kernels: what the kernels
do not cover raises.
"""
from __future__ import annotations

import math
import operator
import os
import shutil
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

__all__ = ["FusedAdamW", "ModelEma", "fuse"]

CHUNK = 4096                                            # SD3D_MT_CHUNK
# sd3d_mt_tensor (include/segdino3d_hip.h), 88 bytes
TENSOR_DTYPE = np.dtype([("p", "<u8"), ("m", "<u8"), ("v", "<u8"), ("ema", "<u8"), ("g", "<u8"), ("n", "<i8"),
                         ("decay", "<f4"), ("step_size", "<f4"), ("rsqrt_bc2", "<f4"),
                         ("one_minus_beta1", "<f4"), ("beta2", "<f4"), ("one_minus_beta2", "<f4"), ("eps", "<f4"),
                         ("ema_decay", "<f4"), ("one_minus_ema_decay", "<f4"), ("pad_", "<f4")])
assert TENSOR_DTYPE.itemsize == 88


# ------------------------------------------------------------------------------------------------------------ host tables (pure host code)
def build_chunks(sizes: Sequence[int], chunk: int = CHUNK) -> np.ndarray:
    """[n_chunks, 2] int32 rows (tensor, index): chunk `index` of tensor `tensor` covers its elements
    [index * chunk, min(size, (index + 1) * chunk)).  Tensors in order, chunks of a tensor in order; a chunk never crosses a tensor."""
    sizes = np.asarray(sizes, dtype=np.int64)
    if sizes.ndim != 1 or sizes.size == 0 or (sizes <= 0).any():
        raise ValueError("build_chunks: expected a non-empty list of positive tensor sizes")
    per = (sizes + chunk - 1) // chunk
    if int(per.max()) >= 2 ** 31:
        raise ValueError("build_chunks: tensor too large")
    first = np.cumsum(per) - per
    out = np.empty((int(per.sum()), 2), dtype=np.int32)
    out[:, 0] = np.repeat(np.arange(sizes.size), per)
    out[:, 1] = np.arange(out.shape[0]) - np.repeat(first, per)
    return out


def fold_scalars(lr: float, weight_decay: float, beta1: float, beta2: float, eps: float, step: int) -> Dict[str, float]:
    """The scalars of one tensor's AdamW update at its own step count `step` (after the increment), in double precision; storing them
    into the float32 fields of the table is the single rounding."""
    return {"decay": 1.0 - lr * weight_decay,
            "step_size": lr / (1.0 - beta1 ** step),
            "rsqrt_bc2": 1.0 / math.sqrt(1.0 - beta2 ** step),
            "one_minus_beta1": 1.0 - beta1, "beta2": beta2, "one_minus_beta2": 1.0 - beta2, "eps": eps}


_SCALAR_FIELDS = ("decay", "step_size", "rsqrt_bc2", "one_minus_beta1", "beta2", "one_minus_beta2", "eps")


def fill_scalars(table: np.ndarray, hyper: Sequence[Tuple[float, float, float, float, float]], group_of: Sequence[int],
                 steps: Sequence[int]) -> None:
    """table[i] gets fold_scalars(*hyper[group_of[i]], steps[i]); one evaluation per distinct (group, step) pair."""
    combo = np.asarray(group_of, dtype=np.int64) * (1 << 40) + np.asarray(steps, dtype=np.int64)
    uniq, inverse = np.unique(combo, return_inverse=True)
    rows = []
    for c in uniq.tolist():
        sc = fold_scalars(*hyper[c >> 40], c & ((1 << 40) - 1))
        rows.append([sc[k] for k in _SCALAR_FIELDS])
    vals = np.asarray(rows, dtype=np.float64)[inverse.reshape(-1)]
    for j, name in enumerate(_SCALAR_FIELDS):
        table[name] = vals[:, j]


def fill_ema_scalars(table: np.ndarray, decay: float) -> None:
    table["ema_decay"] = decay
    table["one_minus_ema_decay"] = 1.0 - decay


# ------------------------------------------------------------------------------------------------------------ launch plumbing
class _Launcher:
    """Device workspace plus pinned staging slots for the host tables of one object.  A slot is reused only once the stream has passed
    the copy that read it (event query, never a wait); while the device is behind, another slot is allocated instead of blocking."""

    def __init__(self):
        self.slots: List[list] = []                     # [pinned uint8 tensor, numpy view, event or None]
        self.ws: Optional[torch.Tensor] = None
        self.chunks: Dict[Tuple[int, ...], np.ndarray] = {}

    def chunks_of(self, sizes: Tuple[int, ...]) -> np.ndarray:
        c = self.chunks.get(sizes)
        if c is None:
            if len(self.chunks) > 8:
                self.chunks.clear()
            c = self.chunks[sizes] = build_chunks(sizes)
        return c

    def stage(self, n_tensors: int, chunks: np.ndarray):
        """-> (slot, table view [n_tensors], pointer of the table, pointer of the chunk list); the chunk list is already copied in."""
        t_bytes = (n_tensors * TENSOR_DTYPE.itemsize + 255) // 256 * 256
        need = t_bytes + chunks.nbytes
        slot = None
        for s in self.slots:
            if s[0].numel() >= need and (s[2] is None or s[2].query()):
                slot = s
                break
        if slot is None:
            buf = torch.empty(max(need, 1 << 16), dtype=torch.uint8, pin_memory=True)
            slot = [buf, buf.numpy(), None]
            self.slots.append(slot)
        raw = slot[1]
        table = raw[:n_tensors * TENSOR_DTYPE.itemsize].view(TENSOR_DTYPE)
        raw[t_bytes:t_bytes + chunks.nbytes].view(np.int32)[:] = chunks.reshape(-1)
        base = slot[0].data_ptr()
        return slot, table, base, base + t_bytes

    def workspace(self, lib, n_tensors: int, n_chunks: int, device) -> torch.Tensor:
        need = lib.sd3d_mt_ws_bytes(n_tensors, n_chunks)
        if self.ws is None or self.ws.numel() < need or self.ws.device != device:
            self.ws = torch.empty(need + need // 4, dtype=torch.uint8, device=device)
        return self.ws

    @staticmethod
    def done(slot, stream: "torch.cuda.Stream") -> None:
        if slot[2] is None:
            slot[2] = torch.cuda.Event()
        slot[2].record(stream)


def _require_device_fp32(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what}: expected a tensor on the HIP device, got {t.device} (no CPU fallback)")
    if t.dtype is not torch.float32:
        raise NotImplementedError(f"{what}: only float32 is implemented, got {t.dtype}")
    if t.layout is not torch.strided:
        raise NotImplementedError(f"{what}: only dense tensors are implemented, got {t.layout}")


_is = operator.is_
_data_ptr = torch.Tensor.data_ptr
_is_contiguous = torch.Tensor.is_contiguous
_numel = torch.Tensor.numel
_layout_of, _dtype_of = operator.attrgetter("layout"), operator.attrgetter("dtype")
_STRIDED, _FP32 = {torch.strided}, {torch.float32}


_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable", "fused")


def _refuse_options(options: dict) -> None:
    for k in _UNSUPPORTED:
        if options.get(k):
            raise NotImplementedError(f"FusedAdamW: {k}=True is not implemented by the multi-tensor HIP kernels (and there is no fallback to "
                                      "torch's)")
    if options.get("decoupled_weight_decay") is False:
        raise NotImplementedError("FusedAdamW: only decoupled weight decay (AdamW) is implemented")
    if isinstance(options.get("lr"), torch.Tensor):
        raise NotImplementedError("FusedAdamW: a tensor lr is not implemented (the scalars of the update are folded on the host)")


# ------------------------------------------------------------------------------------------------------------ optimizer
class _Plan:
    """What FusedAdamW.step keeps about one set of parameters between steps (FusedAdamW._plan)."""


class FusedAdamW(torch.optim.AdamW):
    """`torch.optim.AdamW` whose `step()` is `clip_grad_norm_(params, max_norm)` (when `max_norm > 0`) + the AdamW update, in the
    arithmetic order of torch's single-tensor AdamW, as two launches over all parameters.  `step()` only enqueues: it never reads
    the device.  `grad_norm` is the total gradient norm of the last step as a device scalar (None before the first clipped step)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm: float = 0.0, *, amsgrad=False,
                 maximize=False, capturable=False, differentiable=False, foreach=None, fused=None):
        _refuse_options({"amsgrad": amsgrad, "maximize": maximize, "capturable": capturable, "differentiable": differentiable, "fused": fused,
                         "lr": lr})
        if max_norm < 0:
            raise ValueError(f"Invalid max_norm: {max_norm}")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.max_norm = float(max_norm)
        self._mt_init()

    def _mt_init(self):
        self._mt = _Launcher()
        self._mt_leftover = _Launcher()
        self._norm: Optional[torch.Tensor] = None
        self._ema: Optional["ModelEma"] = None
        self._all = None                                # (group lengths, every parameter, its group)
        self._plans: Dict[Optional[tuple], "_Plan"] = {}

    def __setstate__(self, state):
        super().__setstate__(state)
        self._mt_init()
        self.__dict__.setdefault("max_norm", 0.0)

    @property
    def grad_norm(self) -> Optional[torch.Tensor]:
        return None if self._norm is None else self._norm[0]

    def attach_ema(self, ema: Optional["ModelEma"]) -> None:
        """Fold `ema.update()` into this optimizer's step: the update kernel writes the shadow of every parameter it steps in the same
        pass, and the shadows of this rank's parameters that got no gradient follow in one more launch.  The `ema.update()` call that
        follows such a step in the loop then does nothing.  `attach_ema(None)` detaches."""
        if ema is not None and not isinstance(ema, ModelEma):
            raise TypeError("attach_ema: expected a segdino3d_amd.optim.ModelEma")
        if self._ema is not None:
            self._ema._stepped = False
        self._ema = ema

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plans = {}

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._plans = {}

    def _plan(self, params: List[torch.Tensor], group_of: List[int]) -> "_Plan":
        """Everything about a set of parameters that does not change from one step to the next, checked once: the parameters and their
        state tensors (created like torch's on first use), sizes, chunk list, group of each.  The `step` counters of the set are re-homed
        as 0-d views of one flat CPU tensor, so that they advance and are read in one operation instead of one per parameter."""
        sts = []
        for p in params:
            _require_device_fp32(p, "FusedAdamW: parameter")
            if not p.is_contiguous():
                raise NotImplementedError("FusedAdamW: non-contiguous parameters are not implemented")
            if p.device != params[0].device:
                raise NotImplementedError("FusedAdamW: parameters on several devices are not implemented")
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            elif not (torch.is_tensor(st["step"]) and st["step"].device.type == "cpu"):
                raise NotImplementedError("FusedAdamW: `step` must be a CPU tensor (the state of a capturable / fused optimizer is not implemented)")
            for name in ("exp_avg", "exp_avg_sq"):
                _require_device_fp32(st[name], f"FusedAdamW: {name}")
                if not st[name].is_contiguous() or st[name].numel() != p.numel() or st[name].device != p.device:
                    raise RuntimeError(f"FusedAdamW: {name} does not match its parameter")
            sts.append(st)
        plan = _Plan()
        plan.params, plan.states, plan.group_of = params, sts, np.asarray(group_of, dtype=np.int64)
        plan.ms, plan.vs = [st["exp_avg"] for st in sts], [st["exp_avg_sq"] for st in sts]
        plan.sizes = tuple([p.numel() for p in params])
        plan.chunks = build_chunks(plan.sizes)
        plan.step_flat = torch.tensor([float(st["step"]) for st in sts], dtype=torch.float32)
        plan.step_np = plan.step_flat.numpy()
        plan.step_views = list(plan.step_flat.unbind(0))
        for st, view in zip(sts, plan.step_views):
            st["step"] = view
        plan.shadows, plan.shadow_ptrs, plan.shadow_of, plan.shadow_names = None, None, None, None
        return plan

    def _plan_is_current(self, plan: "_Plan") -> bool:
        sts = plan.states
        return (all(map(_is, [st.get("step") for st in sts], plan.step_views)) and all(map(_is, [st.get("exp_avg") for st in sts], plan.ms))
                and all(map(_is, [st.get("exp_avg_sq") for st in sts], plan.vs)))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        shape = tuple([len(g["params"]) for g in self.param_groups])
        if self._all is None or self._all[0] != shape:
            self._all = (shape, [p for g in self.param_groups for p in g["params"] if p.numel()],
                         [k for k, g in enumerate(self.param_groups) for p in g["params"] if p.numel()])
            self._plans = {}
        _, every, every_group = self._all
        for group in self.param_groups:
            _refuse_options(group)
        grads = [p.grad for p in every]
        missing = [g is None for g in grads]
        key = tuple(missing) if any(missing) else None
        ema = self._ema
        plan = self._plans.get(key)
        if key is not None:
            grads = [g for g in grads if g is not None]
        if grads and not (set(map(_layout_of, grads)) == _STRIDED and all(map(_is_contiguous, grads))):
            for i, g in enumerate(grads):
                if g.layout is not torch.strided:
                    raise NotImplementedError("FusedAdamW: sparse gradients are not implemented")
                if not g.is_contiguous():
                    grads[i] = g.contiguous()       # the kernels read flat memory; an unaligned but contiguous one is theirs to handle
        if grads:
            if plan is not None and not (self._plan_is_current(plan) and tuple(map(_numel, plan.params)) == plan.sizes):
                plan = None
            if plan is None:
                if len(self._plans) > 16:
                    self._plans = {}
                keep = [i for i, m in enumerate(missing) if not m]
                plan = self._plans[key] = self._plan([every[i] for i in keep], [every_group[i] for i in keep])
            ps, n, chunks = plan.params, len(plan.params), plan.chunks
            if set(map(_dtype_of, grads)) != _FP32:
                raise NotImplementedError("FusedAdamW: only float32 gradients are implemented")
            if tuple(map(_numel, grads)) != plan.sizes:
                raise RuntimeError("FusedAdamW: a gradient and its parameter differ in size")
            dev = ps[0].device
            lib = _lib.load()
            plan.step_np += 1.0
            hyper = [(float(g["lr"]), float(g["weight_decay"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]))
                     for g in self.param_groups]
            slot, table, t_ptr, c_ptr = self._mt.stage(n, chunks)
            table["p"] = list(map(_data_ptr, ps))
            table["g"] = list(map(_data_ptr, grads))
            table["m"] = list(map(_data_ptr, plan.ms))
            table["v"] = list(map(_data_ptr, plan.vs))
            table["n"] = plan.sizes
            table["pad_"] = 0.0
            fill_scalars(table, hyper, plan.group_of, plan.step_np)
            written = ps + plan.ms + plan.vs
            if ema is not None:
                shadows = ema._shadows_of(plan, dev)
                table["ema"] = plan.shadow_ptrs
                fill_ema_scalars(table, ema.decay)
                written = written + shadows
            else:
                table["ema"] = 0
                fill_ema_scalars(table, 0.0)
            ws = self._mt.workspace(lib, n, len(chunks), dev)
            stream = torch.cuda.current_stream(dev)
            coef = None
            if self.max_norm > 0:
                if self._norm is None or self._norm.device != dev:
                    self._norm = torch.zeros(2, dtype=torch.float32, device=dev)
                rc = lib.sd3d_mt_grad_norm(t_ptr, n, c_ptr, len(chunks), self.max_norm, self._norm.data_ptr(), ws.data_ptr(), ws.numel(),
                                           stream.cuda_stream)
                if rc:
                    _lib.check(rc, "mt_grad_norm")
                coef = self._norm.data_ptr() + 4
            rc = lib.sd3d_mt_adamw(t_ptr, n, c_ptr, len(chunks), coef, 1 if coef else 0, ws.data_ptr(), ws.numel(), stream.cuda_stream)
            self._mt.done(slot, stream)
            if rc:
                _lib.check(rc, "mt_adamw")
            # the kernels wrote behind torch's back: derived-weight caches (_cache.py) and autograd are keyed by the version counters
            torch.autograd.graph.increment_version(written)
        if ema is not None:
            covered = plan.shadow_of if grads else set()
            if len(covered) < len(ema.shadow):          # this rank's parameters that got no gradient: their average moves all the same
                ema._update(skip=covered, launcher=self._mt_leftover)
            ema._stepped = True
        return loss


def fuse(optimizer: torch.optim.Optimizer, max_norm: float = 0.0) -> FusedAdamW:
    """A `FusedAdamW` over the groups and the state of an existing `torch.optim.AdamW` (the very same group dicts and state tensors, so
    what the old object accumulated carries on).  Build LR schedulers on the returned object."""
    if isinstance(optimizer, FusedAdamW):
        optimizer.max_norm = float(max_norm) if max_norm else optimizer.max_norm
        return optimizer
    if not isinstance(optimizer, torch.optim.AdamW):
        raise TypeError(f"fuse: expected a torch.optim.AdamW, got {type(optimizer).__name__}")
    for group in optimizer.param_groups:
        _refuse_options(group)
    d = optimizer.defaults
    fused = FusedAdamW(optimizer.param_groups, lr=d["lr"], betas=d["betas"], eps=d["eps"], weight_decay=d["weight_decay"], max_norm=max_norm)
    fused.state = optimizer.state
    return fused


# ------------------------------------------------------------------------------------------------------------ EMA of the weights
def _dist():
    import torch.distributed as dist
    return dist if dist.is_available() and dist.is_initialized() else None


class ModelEma:
    """Exponential moving average of the model's parameters, sharded over the ranks, with the surface of the reference's
    `utils/ema_utils.ModelEma`.  The sorted names of all parameters and buffers are cut into `world_size` runs of
    `len(names) // world_size + 1`; rank r keeps `shadow[name]` for the PARAMETERS among its run (buffers take part in the cut only).
    `shadow` is what a checkpoint stores as `ema_model` (through `gather()` + `get_shadow()`, which exchange the shards as files
    `.ema_cache/.ema_cache_<seed>/ema_<rank>.pth`).  `update()` is shadow = (1 - decay) * param + decay * shadow in one launch, in
    place; it works without a process group (one rank that owns everything)."""

    def __init__(self, model: torch.nn.Module, decay: float = 0.9997, seed: str = ""):
        self.model = model
        self.decay = decay
        self.shadow: Dict[str, torch.Tensor] = {}
        self.backup: Dict[str, torch.Tensor] = {}
        dist = _dist()
        self.rank = dist.get_rank() if dist else 0
        self.world_size = dist.get_world_size() if dist else 1
        self.register()
        self.is_gathered = False
        self.seed = seed
        self._mt = _Launcher()
        self._stepped = False

    def register(self):
        names = sorted([n for n, _ in self.model.named_parameters()] + [n for n, _ in self.model.named_buffers()])
        per_rank = len(names) // self.world_size + 1
        self.names = names[self.rank * per_rank:(self.rank + 1) * per_rank]
        mine = set(self.names)
        for name, param in self.model.named_parameters():
            if name in mine:
                self.shadow[name] = param.data.clone()
        self._name_of = None
        self._checked: Dict[str, tuple] = {}

    def _pairs(self) -> List[Tuple[str, torch.Tensor]]:
        """(name, parameter) of every shadowed parameter, enumerated once per register()."""
        if self._name_of is None:
            self._name_of = [(n, p) for n, p in self.model.named_parameters() if n in self.shadow]
        return self._name_of

    def _check_pair(self, name: str, p: torch.Tensor, s: torch.Tensor) -> None:
        _require_device_fp32(p, f"ModelEma: {name}")
        _require_device_fp32(s, f"ModelEma: shadow of {name}")
        if not p.is_contiguous() or not s.is_contiguous() or s.numel() != p.numel() or s.device != p.device:
            raise RuntimeError(f"ModelEma: shadow of {name} does not match its parameter")

    def _shadows_of(self, plan, dev) -> List[torch.Tensor]:
        """Shadows of the plan's parameters that this rank averages (checked when they are first seen or replaced); leaves their
        pointers, 0 for the others, in plan.shadow_ptrs and the ids of the covered parameters in plan.shadow_of."""
        pairs = self._pairs()
        if plan.shadow_names is None or plan.shadow_names[0] is not pairs:
            name_of = {id(p): n for n, p in pairs}
            plan.shadow_names, plan.shadows = (pairs, [name_of.get(id(p)) for p in plan.params]), None
        names = plan.shadow_names[1]
        now = [self.shadow.get(n) if n is not None else None for n in names]
        if plan.shadows is None or not all(map(_is, now, plan.shadows)):
            for n, p, s in zip(names, plan.params, now):
                if s is not None:
                    self._check_pair(n, p, s)
            plan.shadows = now
            plan.shadow_of = {id(p) for p, s in zip(plan.params, now) if s is not None}
        plan.shadow_ptrs = [0 if s is None else s.data_ptr() for s in now]
        return [s for s in now if s is not None]

    def _cache_dir(self) -> str:
        return os.path.join(".ema_cache", f".ema_cache_{self.seed}")

    def _cache_file(self, rank: int) -> str:
        return os.path.join(self._cache_dir(), f"ema_{rank}.pth")

    @torch.no_grad()
    def _update(self, skip=(), launcher: Optional[_Launcher] = None) -> None:
        launcher = launcher or self._mt
        ps, ss = [], []
        for name, p in self._pairs():
            s = self.shadow[name]
            if id(p) in skip or p.numel() == 0:
                continue
            ok = self._checked.get(name)
            if ok is None or ok[0] is not p or ok[1] is not s:
                self._check_pair(name, p, s)
                self._checked[name] = (p, s)
            ps.append(p); ss.append(s)
        if not ps:
            return
        dev = ps[0].device
        if any(p.device != dev for p in ps):
            raise NotImplementedError("ModelEma: parameters on several devices are not implemented")
        lib = _lib.load()
        sizes = tuple([p.numel() for p in ps])
        chunks = launcher.chunks_of(sizes)
        slot, table, t_ptr, c_ptr = launcher.stage(len(ps), chunks)
        table[:] = 0
        table["p"] = [p.data_ptr() for p in ps]
        table["ema"] = [s.data_ptr() for s in ss]
        table["n"] = sizes
        fill_ema_scalars(table, self.decay)
        ws = launcher.workspace(lib, len(ps), len(chunks), dev)
        stream = torch.cuda.current_stream(dev)
        rc = lib.sd3d_mt_ema(t_ptr, len(ps), c_ptr, len(chunks), 0, ws.data_ptr(), ws.numel(), stream.cuda_stream)
        launcher.done(slot, stream)
        if rc:
            _lib.check(rc, "mt_ema")
        torch.autograd.graph.increment_version(ss)

    def update(self):
        if self._stepped:                               # the attached optimizer's step of this iteration already wrote the average
            self._stepped = False
            return
        self._update()

    def gather(self):
        dist = _dist()
        if self.rank == 0:
            os.makedirs(self._cache_dir(), exist_ok=True)
        if dist:
            dist.barrier()
        torch.save(self.shadow, self._cache_file(self.rank))
        if dist:
            dist.barrier()
        self.is_gathered = True

    def get_shadow(self) -> Dict[str, torch.Tensor]:
        assert self.is_gathered
        ckpt: Dict[str, torch.Tensor] = {}
        for r in range(self.world_size):
            ckpt.update(torch.load(self._cache_file(r), map_location="cpu"))
        return ckpt

    def apply_shadow(self):
        ckpt = self.get_shadow()
        for name, param in self.model.named_parameters():
            self.backup[name] = param.data
            param.data = ckpt[name].to(device=param.data.device)

    def restore(self):
        for name, param in self.model.named_parameters():
            if name in self.backup:
                param.data = self.backup[name]
        self.backup = {}
        self.is_gathered = False
        if self.rank == 0:
            shutil.rmtree(self._cache_dir(), ignore_errors=True)
        dist = _dist()
        if dist:
            dist.barrier()
