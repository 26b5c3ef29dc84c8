"""Host side of segdino3d_amd.optim (no GPU): optimizer state interchange with torch.optim.AdamW, fuse(), the multi-tensor table
builder (chunk cover and the per-tensor scalars against the double-precision formulas), ModelEma's sharding against a fixture
recorded from the reference's class, its file round trip without a process group, and the refusals."""
import math
import os

import numpy as np
import pytest
import torch

from segdino3d_amd import optim
from segdino3d_amd.optim import FusedAdamW, ModelEma, fuse

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((3,), (4, 5), (2, 3, 4), (7,))]


def _groups(ps):
    return [{"params": ps[:2], "lr": 1e-4}, {"params": ps[2:], "lr": 1e-3, "weight_decay": 0.01}, {"params": [], "lr": 5e-4}]


def _torch_steps(opt, ps, n, seed=1):
    g = torch.Generator().manual_seed(seed)
    for _ in range(n):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()


def _assert_same_state_dict(a, b):
    assert a.keys() == b.keys()
    assert len(a["param_groups"]) == len(b["param_groups"])
    for ga, gb in zip(a["param_groups"], b["param_groups"]):
        assert ga.keys() == gb.keys()
        for k in ga:
            assert ga[k] == gb[k], k
    assert a["state"].keys() == b["state"].keys()
    for i in a["state"]:
        assert a["state"][i].keys() == b["state"][i].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for k, v in a["state"][i].items():
            w = b["state"][i][k]
            assert v.dtype == w.dtype and v.device == w.device and v.shape == w.shape and torch.equal(v, w), (i, k)


def test_state_dict_interchanges_with_torch_adamw_both_ways():
    ps = _params()
    ref = torch.optim.AdamW(_groups(ps), lr=2e-4, betas=(0.9, 0.98), eps=1e-7, weight_decay=0.05)
    _torch_steps(ref, ps, 3)
    sd = ref.state_dict()
    assert len(sd["state"]) == 4 and float(sd["state"][0]["step"]) == 3.0
    fused = FusedAdamW(_groups(_params(5)), lr=1.0, betas=(0.5, 0.5), eps=1.0, weight_decay=0.0, max_norm=10.0)
    fused.load_state_dict(sd)
    _assert_same_state_dict(fused.state_dict(), sd)
    st = fused.state[fused.param_groups[0]["params"][0]]
    assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32            # host arithmetic for the bias corrections
    back = torch.optim.AdamW(_groups(_params(6)), lr=3.0)
    back.load_state_dict(fused.state_dict())
    _assert_same_state_dict(back.state_dict(), sd)
    ps2 = [p for g in back.param_groups for p in g["params"]]
    _torch_steps(back, ps2, 1)                                                             # and torch carries on from it
    assert float(back.state[ps2[0]]["step"]) == 4.0


def test_fresh_state_dict_has_torch_layout():
    a = torch.optim.AdamW(_groups(_params()), lr=2e-4, weight_decay=0.05).state_dict()
    b = FusedAdamW(_groups(_params()), lr=2e-4, weight_decay=0.05, max_norm=10.0).state_dict()
    _assert_same_state_dict(a, b)


def test_fuse_keeps_groups_hyperparameters_and_state_objects():
    ps = _params()
    ref = torch.optim.AdamW(_groups(ps), lr=2e-4, betas=(0.9, 0.98), eps=1e-7, weight_decay=0.05)
    _torch_steps(ref, ps, 2)
    fused = fuse(ref, max_norm=10.0)
    assert isinstance(fused, FusedAdamW) and isinstance(fused, torch.optim.AdamW) and fused.max_norm == 10.0
    assert len(fused.param_groups) == 3 and fused.param_groups[2]["params"] == [] and fused.param_groups[2]["lr"] == 5e-4
    for gf, gr in zip(fused.param_groups, ref.param_groups):
        assert gf is gr
        assert all(a is b for a, b in zip(gf["params"], gr["params"]))
    assert fused.param_groups[1]["weight_decay"] == 0.01 and fused.param_groups[0]["betas"] == (0.9, 0.98)
    for p in ps:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert fused.state[p][k] is ref.state[p][k]
    assert fuse(fused) is fused
    sched = torch.optim.lr_scheduler.PolynomialLR(fused, total_iters=10, power=0.9)          # the reference's schedule drives it unchanged
    assert fused.param_groups[2]["initial_lr"] == 5e-4 and sched.get_last_lr()[1] == 1e-3
    with pytest.raises(TypeError):
        fuse(torch.optim.SGD(_params(), lr=0.1))


SIZES = [3, 32, 257, 4096, 4097, 2654208, 1, 8191, 8192]


def test_chunks_cover_every_element_once_and_stay_inside_their_tensor():
    chunks = optim.build_chunks(SIZES)
    assert chunks.dtype == np.int32 and chunks.shape[1] == 2 and optim.CHUNK == 4096
    for t, n in enumerate(SIZES):
        mine = chunks[chunks[:, 0] == t, 1].astype(np.int64)
        assert len(mine) == math.ceil(n / optim.CHUNK)
        hits = np.zeros(n, dtype=np.int32)
        for idx in mine:
            lo, hi = idx * optim.CHUNK, min(n, (idx + 1) * optim.CHUNK)
            assert 0 <= lo < hi <= n                                                      # the chunk lies inside tensor t
            hits[lo:hi] += 1
        assert (hits == 1).all(), t
    assert len(chunks) == sum(math.ceil(n / optim.CHUNK) for n in SIZES)
    assert (np.diff(chunks[:, 0]) >= 0).all()
    with pytest.raises(ValueError):
        optim.build_chunks([4, 0])


def test_table_layout_matches_the_header():
    text = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "segdino3d_hip.h")).read()
    body = text[text.index("typedef struct sd3d_mt_tensor {"):text.index("} sd3d_mt_tensor;")]
    body = "".join(line.split("/*")[0] for line in body.splitlines()[1:])
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.replace("const float", "").replace("float", "")
             .replace("int64_t", "").split(",")]
    assert names == list(optim.TENSOR_DTYPE.names)
    assert optim.TENSOR_DTYPE.itemsize == 88 and optim.TENSOR_DTYPE.fields["n"][1] == 40 and optim.TENSOR_DTYPE.fields["decay"][1] == 48
    assert "#define SD3D_MT_CHUNK 4096" in text


@pytest.mark.parametrize("t", [1, 2, 1000])
def test_per_tensor_scalars_equal_the_double_precision_formulas(t):
    hyper = [(1e-4, 0.05, 0.9, 0.999, 1e-8), (1e-3, 0.05, 0.9, 0.999, 1e-8), (2e-4, 0.0, 0.8, 0.98, 1e-6)]
    group_of = [0, 1, 2, 1, 0]
    lag = max(t - 3, 1) if t > 1 else 1
    steps = [t, t, t, lag, t]                                                              # tensor 3 had no gradient in three iterations
    table = np.zeros(5, dtype=optim.TENSOR_DTYPE)
    optim.fill_scalars(table, hyper, group_of, steps)
    optim.fill_ema_scalars(table, 0.9997)
    f32 = np.float32
    for i, (gi, s) in enumerate(zip(group_of, steps)):
        lr, wd, b1, b2, eps = hyper[gi]
        assert table["decay"][i] == f32(1.0 - lr * wd)
        assert table["step_size"][i] == f32(lr / (1.0 - b1 ** s))
        assert table["rsqrt_bc2"][i] == f32(1.0 / math.sqrt(1.0 - b2 ** s))
        assert table["one_minus_beta1"][i] == f32(1.0 - b1) and table["beta2"][i] == f32(b2) and table["one_minus_beta2"][i] == f32(1.0 - b2)
        assert table["eps"][i] == f32(eps)
        assert table["ema_decay"][i] == f32(0.9997) and table["one_minus_ema_decay"][i] == f32(1.0 - 0.9997)
    if t == 1000:
        assert table["step_size"][3] != table["step_size"][1] or table["rsqrt_bc2"][3] != table["rsqrt_bc2"][1]   # the lagging tensor has its own
    # rounded once: float32(1 - beta2) is not 1 - float32(beta2)
    assert f32(1.0 - 0.999) != f32(1.0) - f32(0.999)


def _shard(model, rank, world):
    ema = ModelEma.__new__(ModelEma)
    ema.model, ema.decay, ema.shadow, ema.backup, ema.rank, ema.world_size = model, 0.9997, {}, {}, rank, world
    ema.register()
    return ema


@pytest.mark.parametrize("world", [1, 2, 8])
def test_ema_shards_equal_the_reference_fixture(world):
    from make_golden_optim_ema import small_module
    gold = np.load(os.path.join(GOLDEN, "optim_ema.npz"))
    seen = []
    for rank in range(world):
        ema = _shard(small_module(), rank, world)
        assert list(ema.names) == list(gold[f"names_w{world}_r{rank}"])
        assert list(ema.shadow.keys()) == list(gold[f"shadow_keys_w{world}_r{rank}"])
        seen += list(ema.shadow.keys())
    params = dict(small_module().named_parameters())
    assert sorted(seen) == sorted(params)                                                  # every parameter on exactly one rank
    if world == 1:
        for k, v in _shard(small_module(), 0, 1).shadow.items():
            assert v is not params[k] and np.array_equal(v.numpy(), gold[f"shadow_value/{k}"])


def test_ema_constructor_without_process_group_owns_everything():
    from make_golden_optim_ema import small_module
    model = small_module()
    ema = ModelEma(model, decay=0.99, seed="abc")
    assert (ema.rank, ema.world_size, ema.decay, ema.seed, ema.is_gathered, ema.backup) == (0, 1, 0.99, "abc", False, {})
    assert set(ema.shadow) == {n for n, _ in model.named_parameters()}
    assert set(ema.names) == set(ema.shadow) | {n for n, _ in model.named_buffers()}


def test_ema_gather_apply_restore_round_trip(tmp_path, monkeypatch):
    from make_golden_optim_ema import small_module
    monkeypatch.chdir(tmp_path)
    model = small_module()
    ema = ModelEma(model, seed="s1")
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    with torch.no_grad():
        for s in ema.shadow.values():
            s.add_(1.0)                                                                    # the average differs from the live weights
    with pytest.raises(AssertionError):
        ema.get_shadow()
    ema.gather()
    assert ema.is_gathered and os.path.isfile(tmp_path / ".ema_cache" / ".ema_cache_s1" / "ema_0.pth")
    ckpt = ema.get_shadow()
    assert set(ckpt) == set(before) and all(v.device.type == "cpu" and torch.equal(v, before[k] + 1.0) for k, v in ckpt.items())
    ema.apply_shadow()
    assert all(torch.equal(p, before[k] + 1.0) for k, p in model.named_parameters()) and set(ema.backup) == set(before)
    ema.restore()
    assert all(torch.equal(p, before[k]) for k, p in model.named_parameters())
    assert ema.backup == {} and not ema.is_gathered and not os.path.exists(tmp_path / ".ema_cache" / ".ema_cache_s1")


def test_cpu_parameters_and_unsupported_options_raise():
    ps = _params()
    opt = FusedAdamW(ps, lr=1e-3, max_norm=10.0)
    opt.step()                                                                             # no gradients: nothing to do, like torch
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert all(len(opt.state[p]) == 0 for p in ps)                                         # and nothing was touched
    for kw in ("amsgrad", "maximize", "capturable", "differentiable", "fused"):
        with pytest.raises(NotImplementedError, match=kw):
            FusedAdamW(_params(), lr=1e-3, **{kw: True})
        with pytest.raises(NotImplementedError, match=kw):
            fuse(torch.optim.AdamW(_params(), lr=1e-3, **({kw: True} if kw in ("amsgrad", "maximize") else {})) if kw in ("amsgrad", "maximize")
                 else _with_option(kw))
    with pytest.raises(NotImplementedError, match="tensor lr"):
        FusedAdamW(_params(), lr=torch.tensor(1e-3))
    with pytest.raises(ValueError):
        FusedAdamW(_params(), lr=1e-3, max_norm=-1.0)
    ema = ModelEma(torch.nn.Linear(3, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ema.update()
    with pytest.raises(TypeError):
        opt.attach_ema(object())


def _with_option(kw):
    opt = torch.optim.AdamW(_params(), lr=1e-3)
    for g in opt.param_groups:
        g[kw] = True
    return opt
