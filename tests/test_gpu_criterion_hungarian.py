"""HungarianMatcher configs of the device criterion with the assignment solved on the device (SD3D_HUNGARIAN=device, the
default: csrc/assign.hip) against the host route (SD3D_HUNGARIAN=host: scipy) and the float64 oracle.  The same matches go
into the same kernels, so the two routes must agree bit for bit; against the oracle the tolerances are those of
test_gpu_criterion.test_training_size_against_float64_oracle (fp32 sums of ~S terms: 2e-5 relative on the losses, 2e-5 of the
largest gradient entry on the gradients) and the matches (integer decisions) must be identical."""
import pytest
import torch

from tests.loss_cases import KEYS, as_pred, load_case
from tests.test_gpu_criterion import _tiny_case, _training_size_case, build

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _run(monkeypatch, route, cfg, targets, layers):
    """-> (criterion, losses, gradients in (layer, key, scene) order) of one evaluation on fresh leaves."""
    monkeypatch.setenv("SD3D_HUNGARIAN", route)
    leaves = [{k: [None if v is None else v.detach().clone().requires_grad_(True) for v in lst] for k, lst in layer.items()} for layer in layers]
    crit = build(cfg)
    out = crit(as_pred(leaves), targets)
    (out["seg_loss"] + out["inst_loss"]).backward()
    grads = [v.grad for layer in leaves for k in KEYS for v in layer[k] if v is not None]
    return crit, out, grads


def _assert_routes_agree(a, b):
    (crit_a, out_a, grads_a), (crit_b, out_b, grads_b) = a, b
    assert len(crit_a.last_matches) == len(crit_b.last_matches)
    for la, lb in zip(crit_a.last_matches, crit_b.last_matches):
        assert len(la) == len(lb)
        for ma, mb in zip(la, lb):
            assert torch.equal(ma, mb)
    assert torch.equal(out_a["seg_loss"].detach(), out_b["seg_loss"].detach())
    assert torch.equal(out_a["inst_loss"].detach(), out_b["inst_loss"].detach()) or \
        (bool(torch.isnan(out_a["inst_loss"])) and bool(torch.isnan(out_b["inst_loss"])))
    assert len(grads_a) == len(grads_b)
    for ga, gb in zip(grads_a, grads_b):
        assert (ga is None) == (gb is None)
        if ga is not None:
            assert torch.equal(ga.isnan(), gb.isnan()) and torch.equal(ga.nan_to_num(), gb.nan_to_num())


def test_golden_case_device_route_equals_host_route(monkeypatch):
    d = dev()
    cfg, targets, layers, _ = load_case("hung", torch.float32, d)
    a = _run(monkeypatch, "device", cfg, targets, layers)
    b = _run(monkeypatch, "host", cfg, targets, layers)
    assert len(a[0].last_matches) == len(layers)
    assert torch.isfinite(a[1]["inst_loss"]).item() and all(m.sum().item() > 0 for m in a[0].last_matches[0])
    assert sum(g is not None for g in a[2]) >= 3 * len(layers)
    _assert_routes_agree(a, b)


def test_golden_case_shares_matches_when_iter_matcher_is_off(monkeypatch):
    d = dev()
    cfg, targets, layers, _ = load_case("hung", torch.float32, d)
    cfg = dict(cfg, iter_matcher=False)
    a = _run(monkeypatch, "device", cfg, targets, layers)
    b = _run(monkeypatch, "host", cfg, targets, layers)
    _assert_routes_agree(a, b)
    crit = a[0]
    assert len(crit.last_matches) == len(layers) > 1
    for layer_matches in crit.last_matches[1:]:
        for m, m_last in zip(layer_matches, crit.last_matches[0]):
            assert m is m_last


def test_unknown_route_is_refused(monkeypatch):
    d = dev()
    cfg, targets, layers, _ = load_case("hung", torch.float32, d)
    monkeypatch.setenv("SD3D_HUNGARIAN", "scipy")
    with pytest.raises(ValueError, match="SD3D_HUNGARIAN"):
        build(cfg)(as_pred(layers), targets)


def test_default_route_never_imports_scipy(monkeypatch):
    """With scipy made unimportable the default route still runs: no scipy import is reached on the training path."""
    import sys
    d = dev()
    cfg, targets, layers, _ = load_case("hung", torch.float32, d)
    monkeypatch.delenv("SD3D_HUNGARIAN", raising=False)
    for name in [n for n in sys.modules if n == "scipy" or n.startswith("scipy.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "scipy", None)                 # `import scipy...` now raises ImportError
    crit = build(cfg)
    out = crit(as_pred(layers), targets)
    assert torch.isfinite(out["inst_loss"]).item() and int(crit.last_matches[0][0].sum()) > 0
    monkeypatch.setenv("SD3D_HUNGARIAN", "host")
    with pytest.raises(ImportError):
        crit(as_pred(layers), targets)


def test_training_size_against_float64_oracle(monkeypatch):
    """ScanNet200 training shape with the HungarianMatcher: 2250 queries, 3000 superpoints, 120 objects, two prediction sets."""
    from oracle import loss_ref
    d = dev()
    monkeypatch.delenv("SD3D_HUNGARIAN", raising=False)
    Q, S, G, n_cls, n_sem = 2250, 3000, 120, 198, 200
    t, layers = _training_size_case(5, Q, S, G, n_cls, n_sem)
    cfg = dict(matcher="hungarian", topk=0, cost_weights=[0.5, 1.0, 1.0, 0.5, 0.5], loss_weight=[0.5, 1.0, 1.0, 0.5, 0.5, 0.5], num_classes=n_cls,
               num_semantic_classes=n_sem, sem_ignore_index=n_sem, sem_loss_weight=0.5, non_object_weight=0.1, fix_dice_loss_weight=True,
               iter_matcher=True, fix_mean_loss=True)
    crit = build(cfg)
    t_d = {k: v.to(d) for k, v in t.items()}
    l_d = [{k: [None if v is None else v.to(d).requires_grad_(True) for v in lst] for k, lst in layer.items()} for layer in layers]
    out = crit(as_pred(l_d), [t_d])
    (out["seg_loss"] + out["inst_loss"]).backward()
    t64 = {k: (v.double() if v.is_floating_point() else v) for k, v in t.items()}
    l64 = [{k: [None if v is None else v.double().requires_grad_(True) for v in lst] for k, lst in layer.items()} for layer in layers]
    ref = loss_ref.unified_criterion(as_pred(l64), [t64], cfg)
    (ref["seg_loss"] + ref["inst_loss"]).backward()
    for b, (iq, ig) in enumerate(ref["_indices"]):
        m = crit.last_matches[0][b].cpu()
        exp = torch.zeros_like(m)
        exp[iq, ig] = 1
        assert torch.equal(m, exp), b
    assert abs(float(out["seg_loss"].detach()) - float(ref["seg_loss"].detach())) < 2e-5 * abs(float(ref["seg_loss"].detach()))
    assert abs(float(out["inst_loss"].detach()) - float(ref["inst_loss"].detach())) < 2e-5 * abs(float(ref["inst_loss"].detach()))
    for a, b in zip(l_d, l64):
        for k in KEYS:
            if a[k][0] is None:
                continue
            gr = b[k][0].grad if b[k][0].grad is not None else torch.zeros_like(b[k][0])
            ga = a[k][0].grad.cpu().double() if a[k][0].grad is not None else torch.zeros_like(gr)
            assert (ga - gr).abs().max().item() <= 2e-5 * max(gr.abs().max().item(), 1e-6), k


def test_batch_with_a_scene_without_objects_behaves_like_the_host_route(monkeypatch):
    """Two scenes with different G, one of them G = 0: whatever the host route returns (NaN mask terms for the empty scene,
    loss_3d.py:479-481 on empty tensors), the device route returns the same bits."""
    d = dev()
    t0, layer0, cfg = _tiny_case(G=4, seed=1)
    t1, layer1, _ = _tiny_case(G=0, seed=2)
    cfg = dict(cfg, matcher="hungarian", topk=0)
    targets = [{k: v.to(d) for k, v in t.items()} for t in (t0, t1)]
    layers = [{k: [None if v is None else v.to(d) for v in (layer0[k][0], layer1[k][0])] for k in layer0}]
    a = _run(monkeypatch, "device", cfg, targets, layers)
    b = _run(monkeypatch, "host", cfg, targets, layers)
    _assert_routes_agree(a, b)
    m0, m1 = a[0].last_matches[0]
    assert tuple(m0.shape) == (24, 4) and int(m0.sum()) == 4
    assert tuple(m1.shape) == (24, 0)
