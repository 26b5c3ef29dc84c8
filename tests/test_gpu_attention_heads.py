"""Attention with 64-channel heads (the W = 2 instantiations of csrc/attention.hip attention_body and of csrc/attention_bwd.hip
attn_bwd_q_kernel / attn_bwd_kv_kernel) against float64 masked softmax attention (tests/attention_heads_case.py, pinned to the oracle in
test_decoder_heads.py): forward fp32 / bf16, one and two score sources, bit-packed masks, key split and merge, the batched launch, the
backward pass; and the kernels of both widths against device outputs recorded before the width became a template parameter of one body
per pass.  Bounds are those of test_gpu_train_dec.py / test_gpu_bf16_decoder.py for 32-channel heads (relative to the output scale; the
contraction only doubles)."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from attention_heads_case import attention64, case, views  # noqa: E402

D = 64
# (Lq, Lk, H, nsrc, masked): smallest call; partial query tile + partial single key tile + odd head count; two sources, one key past a
# tile; full tiles, no mask; the decoder's 2D-query shape; 4 workgroups x 33 key tiles: keys split four ways and merged
FWD = [(1, 1, 1, 1, False), (33, 31, 3, 1, True), (70, 65, 2, 2, True), (64, 64, 4, 1, False), (200, 301, 4, 2, True), (40, 1030, 2, 2, True)]
SPLIT = (40, 1030, 2, 2, True)
GRAD = [(16, 8, 1, 1, True), (33, 311, 3, 1, True), (70, 65, 2, 2, True), (200, 301, 4, 2, True), (40, 1030, 2, 2, False)]


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def bf(x):
    return x.to(torch.bfloat16).to(torch.float64)


def close(got, ref, what, tol):
    err = (got.detach().cpu().double() - ref.detach().cpu()).abs().max().item()
    scale = max(ref.abs().max().item(), 1e-3)
    print(f"{what}: max err {err:.3e} = {err / scale:.2e} of the scale {scale:.3e} (bound {tol:g})")
    assert err <= tol * scale, (what, err, scale)


@functools.lru_cache(maxsize=None)
def reference(shape):
    """(case, float64 attention) of one shape - computed once, shared, never modified."""
    Lq, Lk, H, nsrc, masked = shape
    c = case(Lq, Lk, H, D, nsrc, masked)
    q, k, v, q2, k2 = views(c["pack_q"], c["pack_k"], c["C"], nsrc)
    return c, attention64(q, k, v, H, c["scale"], c["blocked"], q2=q2, k2=k2)


def run(shape, d, bf16=False):
    from segdino3d_amd import ops
    Lq, Lk, H, nsrc, masked = shape
    c, _ = reference(shape)
    q, k, v, q2, k2 = views(c["pack_q"].to(d), c["pack_k"].to(d), c["C"], nsrc)          # strided column views of the packed projections
    bits = None if c["bits"] is None else c["bits"].to(d)
    if bf16:
        with ops.bf16_decoder_scope():
            return ops.attention(q, k, v, H, c["scale"], mask_bits=bits, q2=q2, k2=k2)
    return ops.attention(q, k, v, H, c["scale"], mask_bits=bits, q2=q2, k2=k2)


@pytest.mark.parametrize("shape", FWD)
def test_fp32_forward(shape):
    from segdino3d_amd import ops
    d = dev()
    _, ref = reference(shape)
    out = run(shape, d)
    assert out.shape == (shape[0], shape[2] * D)
    close(out, ref, f"fp32 forward {shape}", 2e-5)
    if shape == SPLIT:
        assert ops.attention_launch_config(shape[0], shape[1], shape[2], D) == (4, 4)         # four waves, keys split four ways


@pytest.mark.parametrize("shape", [s for s in FWD if s[1] >= 65])
def test_bf16_forward(shape):
    d = dev()
    Lq, Lk, H, nsrc, masked = shape
    c, exact = reference(shape)
    q, k, v, q2, k2 = views(c["pack_q"], c["pack_k"], c["C"], nsrc)
    rounded = attention64(q, k, v, H, c["scale"], c["blocked"], q2=q2, k2=k2, rnd=bf)            # bf16 Q (pre-scaled), K, V
    fp32 = run(shape, d)
    out = run(shape, d, bf16=True).cpu().double()
    vmax = v.abs().max().item()
    e_model, e_exact = (out - rounded).abs().max().item(), (out - exact).abs().max().item()
    print(f"bf16 forward {shape}: {e_model / vmax:.2e} |v|max from the rounded-operand model, {e_exact / vmax:.2e} from exact attention")
    assert e_model <= 4e-3 * vmax
    assert e_exact <= 3e-2 * vmax
    assert not torch.equal(out.float(), fp32.cpu())                                            # the bf16 kernel really ran
    assert torch.equal(run(shape, d), fp32)                                                    # outside the scope: the fp32 bits


# same waves per workgroup for all three (ONE launch; the first splits its keys four ways, the others do not) / different workgroup
# shapes (launched one by one inside the call)
JOBS = {"one_launch": ([(40, 1030, True), (70, 301, False), (33, 200, True)], 2, 2),
        "mixed_shapes": ([(40, 1030, False), (70, 65, True), (33, 31, True)], 3, 1)}


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("jobs", list(JOBS))
def test_batch_equals_single(jobs, bf16):
    import contextlib
    from segdino3d_amd import ops
    d = dev()
    shapes, H, nsrc = JOBS[jobs]
    cfgs = [ops.attention_launch_config(Lq, Lk, H, D) for Lq, Lk, _ in shapes]
    assert cfgs[0][1] > 1 and cfgs[1][1] == 1 and (len({c[0] for c in cfgs}) == 1) == (jobs == "one_launch"), cfgs
    scope = ops.bf16_decoder_scope if bf16 else contextlib.nullcontext
    single, table = [], []
    with scope():
        for Lq, Lk, masked in shapes:
            c, _ = reference((Lq, Lk, H, nsrc, masked))
            q, k, v, q2, k2 = views(c["pack_q"].to(d), c["pack_k"].to(d), c["C"], nsrc)
            bits = None if c["bits"] is None else c["bits"].to(d)
            single.append(ops.attention(q, k, v, H, c["scale"], mask_bits=bits, q2=q2, k2=k2))
            table.append((q, k, v, bits, q2, k2))
        scale = (D * nsrc) ** -0.5
        outs = []
        for _ in range(2):
            out = [torch.full_like(s, float("nan")) for s in single]
            ops.attention_batch([t + (o,) for t, o in zip(table, out)], H, scale)
            outs.append(out)
    for i, s in enumerate(single):
        assert torch.equal(outs[0][i], s), f"job {i}: batched rows differ from the job's own launch"
        assert torch.equal(outs[1][i], outs[0][i]), f"job {i}: second launch differs"


def _grads(shape, d, bf16=False):
    """(out, pq.grad, pk.grad) of train_dec.attention on strided views of the packed projections."""
    import contextlib
    from segdino3d_amd import ops, train_dec as T
    Lq, Lk, H, nsrc, masked = shape
    c, _ = reference(shape)
    pq, pk = c["pack_q"].to(d).requires_grad_(True), c["pack_k"].to(d).requires_grad_(True)
    q, k, v, q2, k2 = views(pq, pk, c["C"], nsrc)
    bits = None if c["bits"] is None else c["bits"].to(d)
    with (ops.bf16_decoder_scope if bf16 else contextlib.nullcontext)():
        out = T.attention(q, k, v, H, c["scale"], mask_bits=bits, q2=q2, k2=k2)
    out.backward(c["dy"].to(d))
    return out.detach(), pq.grad, pk.grad


@functools.lru_cache(maxsize=None)
def reference_grads(shape):
    Lq, Lk, H, nsrc, masked = shape
    c, _ = reference(shape)
    q64, k64 = c["pack_q"].double().requires_grad_(True), c["pack_k"].double().requires_grad_(True)
    q, k, v, q2, k2 = views(q64, k64, c["C"], nsrc)
    ref = attention64(q, k, v, H, c["scale"], c["blocked"], q2=q2, k2=k2)
    ref.backward(c["dy"].double())
    return ref.detach(), q64.grad, k64.grad


def _blocks(gq, gk, C, nsrc):
    names = [("dq", gq[:, :C]), ("dk", gk[:, :C]), ("dv", gk[:, 2 * C:])]
    return names + ([("dq1", gq[:, C:]), ("dk1", gk[:, C:2 * C])] if nsrc == 2 else [])


@pytest.mark.parametrize("shape", GRAD)
def test_gradients(shape):
    d = dev()
    C, nsrc = shape[2] * D, shape[3]
    ref, rq, rk = reference_grads(shape)
    out, gq, gk = _grads(shape, d)
    close(out, ref, f"output {shape}", 2e-5)
    for (name, got), (_, want) in zip(_blocks(gq, gk, C, nsrc), _blocks(rq, rk, C, nsrc)):
        close(got, want, f"{name} {shape}", 3e-5)
    if nsrc == 1:                                              # the unused second-source columns
        assert float(gq[:, C:].abs().max()) == 0.0 and float(gk[:, C:2 * C].abs().max()) == 0.0
    out2, gq2, gk2 = _grads(shape, d)
    assert torch.equal(out2, out) and torch.equal(gq2, gq) and torch.equal(gk2, gk)          # fixed summation order


def test_bf16_forward_with_fp32_backward():
    shape = (70, 65, 2, 2, True)
    d = dev()
    C = shape[2] * D
    _, rq, rk = reference_grads(shape)
    out, gq, gk = _grads(shape, d, bf16=True)
    assert not torch.equal(out, _grads(shape, d)[0])                                         # the bf16 forward really ran
    for (name, got), (_, want) in zip(_blocks(gq, gk, C, 2), _blocks(rq, rk, C, 2)):
        rel = float((got.cpu().double() - want).norm() / want.norm())
        print(f"bf16 forward + fp32 backward, {name}: relative L2 {rel:.2e}")
        assert rel < 1e-2, (name, rel)


@pytest.mark.parametrize("shape", [(64, 77, 2, 1, False), (70, 65, 2, 2, True)])
def test_dropout_path_equals_the_fused_attention_at_rate_zero(shape):
    from segdino3d_amd import train_dec as T
    d = dev()
    Lq, Lk, H, nsrc, masked = shape
    c, _ = reference(shape)
    q, k, v, q2, k2 = views(c["pack_q"].to(d), c["pack_k"].to(d), c["C"], nsrc)
    bits = None if c["bits"] is None else c["bits"].to(d)
    fused = T.attention(q, k, v, H, c["scale"], mask_bits=bits, q2=q2, k2=k2)
    drop = T.attention_dropout(q, k, v, H, c["scale"], mask_bits=bits, q2=q2, k2=k2, p=0.0)
    close(drop, fused.double(), f"dropout path {shape}", 2e-5)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("Lq,Lk,H,nsrc", [(33, 311, 8, 1), (200, 3000, 8, 2)])
def test_narrow_heads_are_bitwise_unchanged(Lq, Lk, H, nsrc, bf16):
    """32-channel heads: `ops.attention` against the output the same call gave on the commit before the head width became a kernel
    parameter (tests/golden/attention32.npz, written there by tests/golden/make_golden_attention32.py)."""
    import sys
    dev()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_attention32 as G
    recorded = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention32.npz"))[G.name(Lq, Lk, nsrc, bf16)]
    got = G.run(Lq, Lk, H, nsrc, bf16).numpy()
    assert got.shape == recorded.shape and np.array_equal(got.view(np.uint32), recorded.view(np.uint32))


def test_attention_bits_are_unchanged():
    """Forward with 64-channel heads (fp32, bf16) and the fp32 backward at both widths against what the same calls gave on the commit
    before the two widths shared one kernel body per pass (tests/golden/attention_bits.npz, written there on the device by
    tests/golden/make_golden_attention_bits.py; the two largest gradients are pinned by their SHA-256)."""
    import sys
    dev()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_attention_bits as G
    recorded = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_bits.npz"))
    got = G.outputs()
    assert sorted(got) == sorted(recorded.files)
    for name, a in got.items():
        want = recorded[name]
        assert a.shape == want.shape and a.dtype == want.dtype and np.array_equal(a.view(np.uint32), want.view(np.uint32)), name


def test_unsupported_widths_are_refused():
    from segdino3d_amd import ops
    d = dev()
    for H, C in ((2, 256), (16, 256), (3, 256)):              # 128- and 16-channel heads, a head count that does not divide
        q = torch.zeros(8, C, device=d)
        with pytest.raises(ValueError, match="32 or 64"):
            ops.attention(q, q, q, H, 1.0)
    q = torch.zeros(8, 256, device=d)
    with pytest.raises(ValueError, match="32 channels"):        # the row-chain consumer stays 32-wide
        ops.attention_parts([(q, q, q, None, None, None, torch.empty(8, 256, device=d))], 4, 1.0)
