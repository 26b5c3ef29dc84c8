"""The query decoder with 64-channel attention heads (num_heads=4 at d_model=256) on the device: evaluation against the golden vector
captured from the imported reference (tests/golden/decoder_h4_s96_q16.npz, generator make_golden_heads.py), a batch of scenes against
the scenes' own forwards, the non-positional variant against the oracle, and one training step against float64 autograd of the oracle
(pinned to the same golden in test_decoder_heads.py)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from decoder_grad_case import objective  # noqa: E402
from test_gpu_decoder import DEC_KW, _build_decoder, dev  # noqa: E402
from test_oracle_golden import decoder_state_dict, load  # noqa: E402

H4 = dict(num_heads=4)


def _args(g, d, S=None):
    """Decoder arguments of the fixture's scene on device `d` (S: keep the first S superpoints and the query ids below S)."""
    ids = g["query_ids"].long()
    S = g["x"].shape[0] if S is None else S
    ids = ids[ids < S]
    t = lambda a: a.to(d)  # noqa: E731
    return (t(g["x"][:S]), t(g["pos"][:S]), t(g["pos_wo"][:S]), t(g["x"][ids]), t(g["pos"][ids]), t(g["q2d_feat"]), t(g["q2d_pos"]),
            (t(g["lo"]), t(g["hi"])))


def test_evaluation_matches_the_reference_golden():
    d = dev()
    g = load("decoder_h4_s96_q16")
    dec, _ = _build_decoder(H4)
    dec.to(d)
    assert dec._fusable(16) == 0
    out = dec(*[[a] for a in _args(g, d)])
    tol = 3e-4                                                  # test_gpu_decoder.py's bound for decoder_s96_q16 with 8 heads
    report = []

    def rows_ok(got, ref, what):
        err = (got.cpu() - ref).abs()
        bad = (err > tol + tol * ref.abs()).any(dim=1).float().mean().item()
        report.append(f"{what}: {bad:.1%} rows / max err {err.max().item():.1e}")
        assert bad == 0.0, f"{what}: {bad:.1%} of query rows outside tolerance (max err {err.max().item():.3e})"
    for li in range(6):
        aux = out["aux_outputs"][li]
        rows_ok(aux["cls_preds"][0], g[f"aux{li}_cls"], f"aux{li} cls")
        rows_ok(aux["masks"][0], g[f"aux{li}_masks"], f"aux{li} masks")
        if li > 0:
            rows_ok(aux["centers"][0], g[f"aux{li}_centers"], f"aux{li} centers")
            rows_ok(aux["sizes"][0], g[f"aux{li}_sizes"], f"aux{li} sizes")
    for k in ("cls_preds", "sem_preds", "masks", "centers", "sizes", "hidden_states"):
        rows_ok(out[k][0], g[k], k)
    print("4 heads, rows outside 3e-4 (abs + rel) / max abs error per tensor:\n  " + "\n  ".join(report))
    assert torch.equal(torch.sigmoid(out["masks"][0].cpu()) < 0.5, torch.sigmoid(g["masks"]) < 0.5)      # final mask bits


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_batched_evaluation_is_bitwise_the_single_scene_forward(mode):
    d = dev()
    g = load("decoder_h4_s96_q16")
    dec, _ = _build_decoder(H4)
    dec.to(d)
    dec.compute_dtype = mode
    scenes = [_args(g, d), _args(g, d, S=60)]
    assert 0 < scenes[1][3].shape[0] < scenes[0][3].shape[0]
    single = [dec(*[[a] for a in s]) for s in scenes]
    both = dec(*[[s[i] for s in scenes] for i in range(8)])
    for b in range(2):
        for k in ("cls_preds", "sem_preds", "masks", "centers", "sizes", "hidden_states"):
            assert torch.equal(both[k][b], single[b][k][0]), (b, k)
        for li in range(6):
            for k in ("cls_preds", "masks"):
                assert torch.equal(both["aux_outputs"][li][k][b], single[b]["aux_outputs"][li][k][0]), (b, li, k)


def test_plain_decoder_with_four_heads_matches_the_oracle():
    from oracle import decoder_ref as D
    from segdino3d_amd.decoder import ScanNetQueryDecoder
    from test_oracle_golden import plain_decoder_state_dict
    d = dev()
    x = load("decoder_plain_s40")["x"]
    kw = {k: v for k, v in DEC_KW.items() if k not in ("add_box_size_pred", "add_positional_embedding", "pos_type",
                                                         "temperature", "box_modulate_ca", "normalize_box_prediction")}
    kw.update(add_dinox_query_ca=False, num_heads=4)
    dec = ScanNetQueryDecoder(**kw).eval()
    sd = plain_decoder_state_dict()
    dec.load_state_dict({k[len("decoder."):]: v for k, v in sd.items()})
    dec.to(d)
    cfg = D.DecoderCfg(num_heads=4, add_positional_embedding=False, add_dinox_query_ca=False, add_box_size_pred=False,
                       box_modulate_ca=False, normalize_box_prediction=False)
    ref = D.decoder_forward(sd, cfg, x, None, None, x, None, None, None, None, None)
    out = dec([x.to(d)], None, None, [x.to(d)], None, None, None, None)
    assert len(out["aux_outputs"]) == 5

    def rows_ok(got, want, what):                             # the bound of test_plain_decoder_matches_reference_golden
        err = (got.cpu() - want).abs()
        bad = (err > 3e-4 + 3e-4 * want.abs()).any(dim=1).float().mean().item()
        print(f"plain decoder, 4 heads, {what}: {bad:.1%} rows outside 3e-4, max err {err.max().item():.1e}")
        assert bad == 0.0, f"{what}: {bad:.1%} rows outside tolerance (max err {err.max().item():.3e})"
    for li in range(5):
        rows_ok(out["aux_outputs"][li]["cls_preds"][0], ref["aux"][li]["cls_preds"], f"aux{li} cls")
        rows_ok(out["aux_outputs"][li]["masks"][0], ref["aux"][li]["masks"], f"aux{li} masks")
    for k in ("cls_preds", "sem_preds", "masks", "hidden_states"):
        rows_ok(out[k][0], ref[k], k)


def _pick(o):
    """cls / mask / box / semantic outputs of one layer of a single-scene decoder call (None where the decoder gives none)."""
    return {k: (None if o.get(k) is None or o[k][0] is None else o[k][0]) for k in ("cls_preds", "masks", "centers", "sizes", "sem_preds")}


@functools.lru_cache(maxsize=None)
def oracle_step64():
    """One training step of the oracle with four heads in float64 on the inputs of decoder_s96_q16 -> (mask signs, parameter gradients,
    dx, dq).  Computed once; the results are not modified."""
    from oracle import decoder_ref as D
    g = load("decoder_h4_s96_q16")
    sd = {k: (v.double().requires_grad_(True) if v.is_floating_point() else v) for k, v in decoder_state_dict().items()}
    ids = g["query_ids"].long()
    x = g["x"].detach().clone().double().requires_grad_(True)
    q = g["x"].detach()[ids].clone().double().requires_grad_(True)
    t = lambda a: a.double()  # noqa: E731
    out = D.decoder_forward(sd, D.DecoderCfg(num_heads=4), x, t(g["pos"]), t(g["pos_wo"]), q, t(g["pos"][ids]), t(g["q2d_feat"]),
                            t(g["q2d_pos"]), t(g["lo"]), t(g["hi"]))
    sets = [dict(a) for a in out["aux"]] + [dict(cls_preds=out["cls_preds"], masks=out["masks"], centers=out["centers"], sizes=out["sizes"],
                                                 sem_preds=out["sem_preds"])]
    objective(sets).backward()
    grads = {k[len("decoder."):]: v.grad for k, v in sd.items() if v.is_floating_point() and v.grad is not None}
    return out["masks"].detach() > 0, grads, x.grad, q.grad


def _device_step(mode, d):
    g = load("decoder_h4_s96_q16")
    dec, _ = _build_decoder(H4)
    dec.to(d).train()
    dec.return_hidden_states = False
    dec.compute_dtype = mode
    a = _args(g, d)
    x, q = a[0].clone().requires_grad_(True), a[3].clone().requires_grad_(True)
    out = dec([x], [a[1]], [a[2]], [q], [a[4]], [a[5]], [a[6]], [a[7]])
    objective([_pick(o) for o in out["aux_outputs"]] + [_pick(out)]).backward()
    return out["masks"][0].detach().cpu(), {n: p.grad.detach().cpu().double() for n, p in dec.named_parameters() if p.grad is not None}, x.grad, q.grad


def _param_errors(grads, ref):
    """Per parameter ||g - ref|| / max(||ref||, 1e-2 of the median norm) - the floor of decoder_grad_case.compare (key biases have a
    true gradient of zero and rounding noise in any implementation)."""
    norms = sorted(float(v.norm()) for v in ref.values())
    floor = 1e-2 * norms[len(norms) // 2]
    return sorted(((float((grads[n] - ref[n]).norm()) / max(float(ref[n].norm()), floor), n) for n in ref), reverse=True)


def test_training_step_matches_float64_oracle():
    """fp32: mask signs equal, every parameter gradient, d/d(superpoint features) and d/d(query features) within 2e-3 - the bound of
    test_gpu_train_dec.py::test_decoder_training_gradients_match_reference for 8 heads."""
    d = dev()
    signs, ref, dx64, dq64 = oracle_step64()
    masks, grads, dx, dq = _device_step("fp32", d)
    assert torch.equal(masks > 0, signs), "mask signs differ: gradients are not comparable"
    assert set(ref) <= set(grads)
    worst = _param_errors(grads, ref)
    print("4 heads, fp32 training step, worst parameter gradients vs float64 autograd:", worst[:3])
    assert worst[0][0] <= 2e-3, worst[:6]
    for got, want, what in ((dx, dx64, "dx"), (dq, dq64, "dq")):
        err = float((got.cpu().double() - want).abs().max())
        assert err <= 2e-3 * float(want.abs().max()), (what, err)


def test_bf16_training_step_stays_close_to_float64_oracle():
    """compute_dtype="bf16" (bf16 forward operands, fp32 attention backward): the bounds test_gpu_bf16_decoder.py::
    test_bf16_training_step_stays_close_to_fp32 applies to the 8-head decoder - mask signs > 95 % equal, gradient cosine > 0.97,
    median per-parameter relative L2 < 0.1, d/d(superpoint features) within 0.3 - here against float64 autograd."""
    d = dev()
    signs, ref, dx64, _ = oracle_step64()
    masks, grads, dx, _ = _device_step("bf16", d)
    assert not torch.equal(masks, _device_step("fp32", d)[0])                     # the bf16 forward really ran
    agree = ((masks > 0) == signs).float().mean().item()
    rel = _param_errors(grads, ref)
    names = sorted(ref)
    a64, a16 = torch.cat([ref[n].reshape(-1) for n in names]), torch.cat([grads[n].reshape(-1) for n in names])
    cos = float(torch.nn.functional.cosine_similarity(a64, a16, dim=0))
    dxe = float((dx.cpu().double() - dx64).norm() / dx64.norm())
    print(f"4 heads, bf16 training step vs float64: mask signs equal {agree:.4f}, gradient cosine {cos:.4f}, per-parameter relative L2 "
          f"median {rel[len(rel) // 2][0]:.3f} max {rel[0][0]:.3f}, dx {dxe:.3f}")
    assert agree > 0.95 and cos > 0.97 and rel[len(rel) // 2][0] < 0.1 and dxe < 0.3
