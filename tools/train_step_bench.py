"""One-scene training step (forward + loss + backward) at the benchmark shape, for profiling, and the parameter update that follows it:
python tools/train_step_bench.py [points] [steps] [update]
update = all (default) | none | torch | fused | torch_ema | fused_ema: which variants of the third phase run (one of them alone for a kernel trace).
The update phase keeps the gradients of a real backward and times clip_grad_norm_(10) + AdamW.step() + zero_grad() [+ the EMA of the weights]
on all parameter tensors of the model, with torch's own path (torch.optim.AdamW, foreach on the device; the EMA as the reference's loop
over the parameters) and with segdino3d_amd.optim (FusedAdamW(max_norm=10), ModelEma attached): HIP events around 20 updates, five times
over, and the host time of the step() call alone.  Prints one JSON line."""
import json, os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import segdino3d_amd as seg
from segdino3d_amd.configs import scannet200_model_cfg
from segdino3d_amd.synth import add_training_targets, make_scene
n_pts = int(sys.argv[1]) if len(sys.argv) > 1 else 150000
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
update = sys.argv[3] if len(sys.argv) > 3 else "all"
d = torch.device("cuda:0")
torch.manual_seed(0)
model = seg.build_architecture(scannet200_model_cfg(query_num=-1)).to(d).train()
pts, tgt = make_scene(5, n_pts, 3000 if n_pts > 50000 else 400, 300 if n_pts > 50000 else 50)
tgt = add_training_targets(pts, tgt, n_instances=40 if n_pts > 50000 else 10, seed=2)
pts, tgt = pts.to(d), tgt.to(d)


def step():
    for p in model.parameters():
        p.grad = None
    for k in ("query_inst_sem_masks", "instance_centers", "instance_sizes"):
        tgt.__dict__.pop(k, None)
    t0 = time.perf_counter()
    losses = model([pts], [tgt])
    torch.cuda.synchronize(); t1 = time.perf_counter()
    (losses["seg_loss"] + losses["inst_loss"]).backward()
    torch.cuda.synchronize(); t2 = time.perf_counter()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t1)

for _ in range(2):
    step()
ts = [step() for _ in range(steps)]
print("forward+loss ms", round(sum(t[0] for t in ts) / steps, 2), "backward ms", round(sum(t[1] for t in ts) / steps, 2))

if update != "none":
    from segdino3d_amd.optim import FusedAdamW, ModelEma
    REPS, ROUNDS, DECAY = 20, 5, 0.9997
    params = [p for p in model.parameters() if p.grad is not None]
    saved = [p.grad.detach().clone() for p in params]
    n_values = sum(p.numel() for p in params)
    names = [n for n, p in model.named_parameters() if p.grad is not None]
    backbone = [p for n, p in zip(names, params) if n.startswith("backbone.")]
    rest = [p for n, p in zip(names, params) if not n.startswith("backbone.")]

    def groups():                                               # the reference's three groups: the rest, the backbone, an empty third
        return [{"params": rest}, {"params": backbone, "lr": 1e-4}, {"params": []}]

    def give_grads():
        for p, g in zip(params, saved):
            p.grad = g

    def variant(kind, ema):
        if kind == "torch":
            opt = torch.optim.AdamW(groups(), lr=1e-4, weight_decay=0.05)
            shadow = {n: p.data.clone() for n, p in zip(names, params)} if ema else None

            def run():
                torch.nn.utils.clip_grad_norm_(params, 10.0)
                opt.step()
                opt.zero_grad()
                if ema:                                         # utils/ema_utils.py:34-38 restated: three kernels and a fresh tensor per parameter
                    for n, p in zip(names, params):
                        shadow[n] = ((1.0 - DECAY) * p.data + DECAY * shadow[n]).clone()
            step_only = opt.step
        else:
            opt = FusedAdamW(groups(), lr=1e-4, weight_decay=0.05, max_norm=10.0)
            if ema:
                avg = ModelEma(model, decay=DECAY)
                opt.attach_ema(avg)

            def run():
                opt.step()
                opt.zero_grad()
                if ema:
                    avg.update()                                # attached: the step above already wrote the average
            step_only = opt.step
        for _ in range(3):
            give_grads(); run()
        torch.cuda.synchronize()
        rounds = []
        for _ in range(ROUNDS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                give_grads(); run()
            e1.record()
            torch.cuda.synchronize()
            rounds.append(e0.elapsed_time(e1) / REPS)
        host = []
        for _ in range(REPS):
            give_grads()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step_only()
            host.append(1e3 * (time.perf_counter() - t0))
            opt.zero_grad()
        torch.cuda.synchronize()
        bytes_alg = n_values * (44 if ema else 32)
        ms = sum(rounds) / ROUNDS
        return dict(ms_per_update=round(ms, 4), ms_rounds=[round(r, 4) for r in rounds], spread_ms=round(max(rounds) - min(rounds), 4),
                    host_ms_step_call=round(sorted(host)[len(host) // 2], 4), algorithmic_TBps=round(bytes_alg / ms / 1e9, 3))

    out = dict(points=n_pts, tensors=len(params), values=n_values, reps=REPS, rounds=ROUNDS)
    for kind, ema in (("torch", False), ("fused", False), ("torch", True), ("fused", True)):
        key = kind + ("_ema" if ema else "")
        if update in ("all", key):
            out[key] = variant(kind, ema)
    print(json.dumps(out))
