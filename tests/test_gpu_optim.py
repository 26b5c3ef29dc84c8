"""segdino3d_amd.optim on the device.  The yardstick is torch itself in float64 on the CPU: torch.optim.AdamW +
torch.nn.utils.clip_grad_norm_ + PolynomialLR(power=0.9), and for the EMA the reference's update formula
shadow = (1 - decay) * param + decay * shadow.  The same torch code in float32 on the CPU gives the error an fp32 chain of this length
has; the fused kernels must stay within 4 x that error plus one float32 ulp of the tensor's largest value (both results are rounded to
float32, so even an exact computation is half an ulp away, and on a 3-element tensor torch's float32 run can happen to be exact).
The factor 4: both sides are chains of the same dozen roundings per element and iteration that differ in operation order, in fused
multiply-adds and in a division replaced by a multiplication with the reciprocal; a wrong formula (a missing bias correction, eps
inside the square root) is off by orders of magnitude.  Run with -s to see the measured ratios."""
import copy

import numpy as np
import pytest
import torch

import segdino3d_amd as seg
from segdino3d_amd.optim import FusedAdamW, ModelEma, fuse

pytestmark = pytest.mark.gpu
d = torch.device("cuda:0")

SHAPES = [(3,), (32,), (257,), (27, 32, 64), (1000, 33), (1001,), (40, 50), (513,), (4097,)]
UNALIGNED, NONCONTIG, SKIPPED = 5, 6, 7                  # roles of three of the tensors; SKIPPED gets no gradient on iterations 5-9
GROUPS = [([0, 1, 3], 1e-3), ([2, 4, 5, 7], 3e-4), ([6, 8], 2e-3)]
ITERS, TOTAL_ITERS, DECAY, WD = 20, 40, 0.9, 0.05


class _Bag(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        self.w = torch.nn.ParameterList(params)


def _init_values(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(1.0 + 3.0 * torch.rand(s, generator=g)) * (1 - 2 * (torch.rand(s, generator=g) < 0.5).float()) for s in SHAPES]


def _grad_values(seed=1, iters=ITERS):
    g = torch.Generator().manual_seed(seed)
    return [[None if (i == SKIPPED and 5 <= it <= 9) else 3.0 * torch.randn(s, generator=g) for i, s in enumerate(SHAPES)] for it in range(iters)]


def _make(values, dtype, device, cls, max_norm, lrs=None):
    ps = [torch.nn.Parameter(v.to(dtype=dtype, device=device).clone()) for v in values]
    groups = [{"params": [ps[i] for i in idx], "lr": lr} for idx, lr in GROUPS]
    kw = {"max_norm": max_norm} if cls is FusedAdamW else {}
    opt = cls(groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=WD, **kw)
    return ps, opt


def _set_grads(ps, grads, on_device):
    for i, (p, g) in enumerate(zip(ps, grads)):
        if g is None:
            p.grad = None
        elif not on_device:
            p.grad = g.to(p.dtype)
        elif i == UNALIGNED:                                  # a slice of a flat buffer, 4 bytes off the 16-byte grid
            flat = torch.zeros(g.numel() + 4, device=d)
            flat[1:1 + g.numel()] = g.to(d).reshape(-1)
            p.grad = flat[1:1 + g.numel()].view(p.shape)
            assert p.grad.data_ptr() % 16 == 4 and p.grad.is_contiguous()
        elif i == NONCONTIG:
            p.grad = g.to(d).t().contiguous().t()
            assert not p.grad.is_contiguous()
        else:
            p.grad = g.to(d)


def _run_torch(dtype, max_norm, iters=ITERS, ema=True, start=None, grads=None):
    """The yardstick: -> params, exp_avg, exp_avg_sq, shadows, norms per iteration."""
    ps, opt = _make(start or _init_values(), dtype, "cpu", torch.optim.AdamW, max_norm)
    sched = torch.optim.lr_scheduler.PolynomialLR(opt, total_iters=TOTAL_ITERS, power=0.9)
    shadow = [p.detach().clone() for p in ps]
    norms = []
    for grads_it in (grads or _grad_values())[:iters]:
        _set_grads(ps, grads_it, False)
        if max_norm > 0:
            norms.append(torch.nn.utils.clip_grad_norm_(ps, max_norm).clone())
        opt.step()
        opt.zero_grad()
        sched.step()
        if ema:
            with torch.no_grad():
                shadow = [(1.0 - DECAY) * p.detach() + DECAY * s for p, s in zip(ps, shadow)]
    return dict(p=[p.detach() for p in ps], exp_avg=[opt.state[p]["exp_avg"] for p in ps], exp_avg_sq=[opt.state[p]["exp_avg_sq"] for p in ps],
                ema=shadow, norms=norms, opt=opt, params=ps)


def _run_fused(max_norm, iters=ITERS, route="attach"):
    ps, opt = _make(_init_values(), torch.float32, d, FusedAdamW, max_norm)
    sched = torch.optim.lr_scheduler.PolynomialLR(opt, total_iters=TOTAL_ITERS, power=0.9)
    bag = _Bag(ps)
    ema = ModelEma(bag, decay=DECAY) if route else None
    if route == "attach":
        opt.attach_ema(ema)
    norms = []
    for grads_it in _grad_values()[:iters]:
        _set_grads(ps, grads_it, True)
        opt.step()
        if max_norm > 0:
            norms.append(opt.grad_norm.clone())
        else:
            assert opt.grad_norm is None
        opt.zero_grad()
        sched.step()
        if ema is not None:
            ema.update()
    shadow = [ema.shadow[f"w.{i}"] for i in range(len(ps))] if ema is not None else None
    return dict(p=[p.detach() for p in ps], exp_avg=[opt.state[p]["exp_avg"] for p in ps], exp_avg_sq=[opt.state[p]["exp_avg_sq"] for p in ps],
                ema=shadow, norms=norms, opt=opt, params=ps)


def _check_bound(fused, r32, r64, keys=("p", "exp_avg", "exp_avg_sq", "ema"), label=""):
    worst = {}
    fails = []
    for key in keys:
        for i, (xf, x32, x64) in enumerate(zip(fused[key], r32[key], r64[key])):
            x64 = x64.double()
            err_f = (xf.detach().cpu().double() - x64).abs().max().item()
            err_32 = (x32.double() - x64).abs().max().item()
            ulp = float(np.spacing(np.float32(x64.abs().max().item())))
            ratio = err_f / max(err_32, 1e-300)
            worst[key] = max(worst.get(key, (0.0,)), (ratio, i, err_f, err_32))
            if not err_f <= 4 * err_32 + ulp:
                fails.append((key, i, SHAPES[i], err_f, err_32, ulp))
    print(f"\n[{label}] worst fused/torch32 error ratio per quantity (ratio, tensor, |fused-f64|, |torch32-f64|):")
    for key, w in worst.items():
        print(f"    {key:11s} {w[0]:8.3f}  tensor {w[1]} {SHAPES[w[1]]}  {w[2]:.3e}  {w[3]:.3e}")
    assert not fails, fails


@pytest.mark.parametrize("max_norm", [10.0, 1e9, 0.0])
def test_parity_of_20_iterations_with_float64_torch(max_norm):
    r64, r32 = _run_torch(torch.float64, max_norm), _run_torch(torch.float32, max_norm)
    fused = _run_fused(max_norm)
    _check_bound(fused, r32, r64, label=f"max_norm={max_norm:g}")
    for i, p in enumerate(fused["params"]):                    # `step` is torch's: per parameter, a float32 scalar on the CPU
        st = fused["opt"].state[p]["step"]
        assert st.device.type == "cpu" and st.dtype == torch.float32 and float(st) == (15.0 if i == SKIPPED else 20.0)
    if max_norm > 0:
        assert len(fused["norms"]) == ITERS
        worst = 0.0
        for nf, n32, n64 in zip(fused["norms"], r32["norms"], r64["norms"]):
            assert nf.is_cuda and nf.dtype == torch.float32 and nf.dim() == 0
            rel_f, rel_32 = abs(nf.item() - n64.item()) / n64.item(), abs(n32.item() - n64.item()) / n64.item()
            worst = max(worst, rel_f / max(rel_32, 2.0 ** -30))
            assert rel_f <= 4 * rel_32 + 2.0 ** -23, (nf.item(), n32.item(), n64.item())
        print(f"    grad norm: worst relative-error ratio fused/torch32 {worst:.3f} (norm {r64['norms'][0].item():.1f}, max_norm {max_norm:g})")
        if max_norm == 10.0:
            assert r64["norms"][0].item() > 50 * max_norm       # clipping is active in this case


def test_two_ema_routes_give_the_same_bits():
    a, b = _run_fused(10.0, iters=12, route="attach"), _run_fused(10.0, iters=12, route="separate")
    for key in ("ema", "p", "exp_avg", "exp_avg_sq"):
        for i, (x, y) in enumerate(zip(a[key], b[key])):
            assert torch.equal(x, y), (key, i)
    start = _init_values()
    assert all(not torch.equal(s.cpu(), v) for s, v in zip(a["ema"], start))                # and the average did move


def test_step_and_ema_update_do_not_block_the_host():
    ps, opt = _make(_init_values(), torch.float32, d, FusedAdamW, 10.0)
    ema = ModelEma(_Bag(ps), decay=DECAY)
    grads = _grad_values(iters=6)
    for it in range(2):                                         # first use allocates staging and workspace
        _set_grads(ps, grads[it], True)
        opt.step()
        ema.update()
    torch.cuda.synchronize()
    for attach in (False, True):
        opt.attach_ema(ema if attach else None)
        for it in range(2, 4):
            _set_grads(ps, grads[it + 2 * attach], True)
            torch.cuda.set_sync_debug_mode("error")
            try:
                opt.step()
                ema.update()
                norm = opt.grad_norm
            finally:
                torch.cuda.set_sync_debug_mode("default")
            assert norm.is_cuda
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in ps)


def test_fuse_mid_training_continues_within_the_bound():
    half = 10
    r64, r32 = _run_torch(torch.float64, 10.0, ema=False), _run_torch(torch.float32, 10.0, ema=False)
    grads = _grad_values()
    ps, opt = _make(_init_values(), torch.float32, d, torch.optim.AdamW, 10.0)              # torch's own optimizer on the device ...
    sched = torch.optim.lr_scheduler.PolynomialLR(opt, total_iters=TOTAL_ITERS, power=0.9)
    for it in range(half):
        _set_grads(ps, grads[it], True)
        torch.nn.utils.clip_grad_norm_(ps, 10.0)
        opt.step()
        opt.zero_grad()
        sched.step()
    fused = fuse(opt, max_norm=10.0)                                                         # ... handed over mid-training
    sched.optimizer = fused                                                                  # the schedule is re-pointed (the groups are shared)
    assert [g["lr"] for g in fused.param_groups] == [g["lr"] for g in opt.param_groups]
    for it in range(half, ITERS):
        _set_grads(ps, grads[it], True)
        fused.step()
        fused.zero_grad()
        sched.step()
    got = dict(p=[p.detach() for p in ps], exp_avg=[fused.state[p]["exp_avg"] for p in ps], exp_avg_sq=[fused.state[p]["exp_avg_sq"] for p in ps])
    _check_bound(got, r32, r64, keys=("p", "exp_avg", "exp_avg_sq"), label="fuse() after 10 of 20 iterations")
    # and the state goes back into torch's class
    back = torch.optim.AdamW([{"params": g["params"]} for g in fused.param_groups], lr=1e-3)
    back.load_state_dict(fused.state_dict())
    assert float(back.state[ps[0]]["step"]) == 20.0 and torch.equal(back.state[ps[3]]["exp_avg"], fused.state[ps[3]]["exp_avg"])


def test_grad_scaler_step_updates_the_parameters():
    ps, opt = _make(_init_values(), torch.float32, d, FusedAdamW, 10.0)
    r64, r32 = _run_torch(torch.float64, 10.0, iters=1, ema=False), _run_torch(torch.float32, 10.0, iters=1, ema=False)
    scaler = torch.amp.GradScaler("cuda", enabled=True, init_scale=1024.0)
    before = [p.detach().clone() for p in ps]
    assert scaler.scale(torch.ones((), device=d)).item() == 1024.0
    _set_grads(ps, [None if g is None else g * 1024.0 for g in _grad_values()[0]], True)    # what scaler.scale(loss).backward() leaves
    scaler.step(opt)                                                                         # unscales, finds no inf, calls opt.step()
    scaler.update()
    assert all(not torch.equal(a, b) for a, b in zip(before, ps))
    got = dict(p=[p.detach() for p in ps], exp_avg=[opt.state[p]["exp_avg"] for p in ps], exp_avg_sq=[opt.state[p]["exp_avg_sq"] for p in ps])
    _check_bound(got, r32, r64, keys=("p", "exp_avg", "exp_avg_sq"), label="GradScaler.step")
    _set_grads(ps, [None if g is None else g * float("inf") for g in _grad_values()[0]], True)
    kept = [p.detach().clone() for p in ps]
    scaler.step(opt)                                                                         # overflow: the step is skipped
    assert all(torch.equal(a, b) for a, b in zip(kept, ps))


# ---------------------------------------------------------------------------------------------------------------- whole model
def _train_once(seed=0, n_pts=150000):
    from segdino3d_amd.configs import scannet200_model_cfg
    from segdino3d_amd.synth import add_training_targets, make_scene
    torch.manual_seed(seed)
    model = seg.build_architecture(scannet200_model_cfg(query_num=-1)).to(d).train()
    pts, tgt = make_scene(5, n_pts, 3000, 300)
    tgt = add_training_targets(pts, tgt, n_instances=40, seed=2)
    pts, tgt = pts.to(d), tgt.to(d)
    backbone = [p for n, p in model.named_parameters() if n.startswith("backbone.")]
    rest = [p for n, p in model.named_parameters() if not n.startswith("backbone.")]
    opt = FusedAdamW([{"params": rest}, {"params": backbone, "lr": 1e-4}, {"params": []}], lr=1e-4, weight_decay=0.05, max_norm=10.0)
    losses = model([pts], [tgt])
    (losses["seg_loss"] + losses["inst_loss"]).backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    opt.step()
    norm = opt.grad_norm.clone()
    opt.zero_grad()
    return model, opt, norm, grads, (pts, tgt)


def test_whole_model_update_is_reproducible_and_seen_by_the_next_forward():
    model_a, opt_a, norm_a, grads_a, (pts, tgt) = _train_once()
    model_b, opt_b, norm_b, grads_b, _ = _train_once()
    n_params = sum(1 for _ in model_a.parameters())
    print(f"\n    whole model: {n_params} parameter tensors, {len(grads_a)} with a gradient, {sum(g.numel() for g in grads_a.values())} values")
    assert n_params >= 528 and len(grads_a) >= n_params // 2 and grads_a.keys() == grads_b.keys()
    assert all(torch.equal(grads_a[k], grads_b[k]) for k in grads_a), "the backward pass itself differs between two runs from one seed"
    assert torch.isfinite(norm_a) and norm_a.item() > 0
    ref_norm = torch.linalg.vector_norm(torch.stack([g.double().norm() for g in grads_a.values()])).item()
    assert abs(norm_a.item() - ref_norm) <= 1e-6 * ref_norm, (norm_a.item(), ref_norm)
    assert torch.equal(norm_a, norm_b)
    moved = 0
    for (name, pa), pb in zip(model_a.named_parameters(), model_b.parameters()):
        assert torch.equal(pa, pb), name
        if name in grads_a:
            sa, sb = opt_a.state[pa], opt_b.state[pb]
            assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), name
            assert float(sa["step"]) == 1.0
            moved += 1
    assert moved == len(grads_a)
    # the next forward must run on the UPDATED weights: model_a made its derived (packed / folded) copies before the update; a model that
    # loads the updated state_dict makes them afresh
    from segdino3d_amd.configs import scannet200_model_cfg
    fresh = seg.build_architecture(scannet200_model_cfg(query_num=-1)).to(d)
    fresh.load_state_dict(copy.deepcopy(model_a.state_dict()))
    model_a.eval(), fresh.eval()
    for k in ("query_inst_sem_masks", "instance_centers", "instance_sizes"):                # what the training forward cached on the target
        tgt.__dict__.pop(k, None)
    with torch.no_grad(), seg.capture() as cap_a:
        model_a([pts], [tgt])
    with torch.no_grad(), seg.capture() as cap_f:
        fresh([pts], [tgt])
    assert torch.equal(cap_a.outputs["masks"][0], cap_f.outputs["masks"][0])


def test_stale_derived_weights_without_mode_switch():
    """The same check where no .train() / .eval() call comes between update and forward (those calls drop the derived copies by
    themselves): an eval-mode model whose parameters are stepped must run its next forward on the stepped weights."""
    from segdino3d_amd.configs import scannet200_model_cfg
    from segdino3d_amd.synth import make_scene
    torch.manual_seed(0)
    cfg = scannet200_model_cfg(query_num=-1)
    model = seg.build_architecture(cfg).to(d).eval()
    pts, tgt = make_scene(1, n_points=8000, n_superpoints=64, n_query2d=8)
    pts, tgt = pts.to(d), tgt.to(d)
    with torch.no_grad(), seg.capture() as cap0:
        model([pts], [tgt])                                     # builds the derived copies
    params = [p for p in model.parameters()]
    opt = FusedAdamW(params, lr=1e-2, weight_decay=0.05, max_norm=10.0)
    g = torch.Generator(device=d).manual_seed(3)
    for p in params:
        p.grad = torch.randn(p.shape, device=d, generator=g)
    opt.step()
    with torch.no_grad(), seg.capture() as cap1:
        model([pts], [tgt])
    fresh = seg.build_architecture(cfg).to(d).eval()
    fresh.load_state_dict(copy.deepcopy(model.state_dict()))
    with torch.no_grad(), seg.capture() as cap2:
        fresh([pts], [tgt])
    assert not torch.equal(cap0.outputs["masks"][0], cap1.outputs["masks"][0])
    assert torch.equal(cap1.outputs["masks"][0], cap2.outputs["masks"][0])
