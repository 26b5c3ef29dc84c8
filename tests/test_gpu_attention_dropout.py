"""Attention dropout inside the fused kernels (csrc/attention.h; the DROP instantiations of csrc/attention.hip attention_body and of
csrc/attention_bwd.hip attn_bwd_q_kernel / attn_bwd_kv_kernel) on the device: the mask kernel against the numpy restatement bit for
bit, forward (fp32, bf16) and gradients against float64 attention with that mask on its probabilities, independence of the key split,
rate 0, determinism, fully dropped rows, peak memory, and the decoder against its explicit-probability cross-check on the same bits.
Bounds are those of tests/test_gpu_attention_heads.py (2e-5 of the output scale forward, 3e-5 gradients, its bf16 bounds)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from attention_dropout_case import KEY, attention64_dropout, keep_mask, key_tensor  # noqa: E402
from attention_heads_case import case, views  # noqa: E402

H = 2
CALL = 3
# (Lq, Lk, nsrc, masked): partial tiles, one source; two sources, one key past a tile, mask; 33 key tiles split four ways
FWD = [(33, 31, 1, False), (70, 65, 2, True), (40, 1030, 2, True)]
SPLIT = (40, 1030, 2, True)
# one source, 10 key tiles; two sources + mask; 33 query tiles: the kv kernel's eight waves and 96 KiB of LDS at 32-channel heads
GRAD = [(33, 311, 1, False), (70, 65, 2, True), (1030, 40, 2, False)]
MASKED = (70, 65, 2, True)


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
def inputs(shape, D):
    Lq, Lk, nsrc, masked = shape
    return case(Lq, Lk, H, D, nsrc, masked, tag="ad")


@functools.lru_cache(maxsize=None)
def mask(Lq, Lk, p, call=CALL, key=KEY):
    return torch.from_numpy(keep_mask(key, call, H, Lq, Lk, p))


@functools.lru_cache(maxsize=None)
def reference(shape, D, p, rounded=False, call=CALL):
    """float64 attention with the restated keep mask on its probabilities - computed once, shared, never modified"""
    Lq, Lk, nsrc, masked = shape
    c = inputs(shape, D)
    q, k, v, q2, k2 = views(c["pack_q"], c["pack_k"], c["C"], nsrc)
    return attention64_dropout(q, k, v, H, c["scale"], mask(Lq, Lk, p, call), p, c["blocked"], q2=q2, k2=k2, rnd=bf if rounded else None)


def run(shape, D, p, d, bf16=False, call=CALL, key=KEY):
    import contextlib
    from segdino3d_amd import ops, train_dec as T
    Lq, Lk, nsrc, masked = shape
    c = inputs(shape, D)
    q, k, v, q2, k2 = views(c["pack_q"].to(d), c["pack_k"].to(d), c["C"], nsrc)
    bits = None if c["bits"] is None else c["bits"].to(d)
    with (ops.bf16_decoder_scope if bf16 else contextlib.nullcontext)():
        return T.attention(q, k, v, H, c["scale"], mask_bits=bits, q2=q2, k2=k2, dropout_p=p, key=key_tensor(key, d), call=call)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("Lq,Lk", [(33, 31), (70, 1030)])
def test_mask_kernel_equals_the_restatement(Lq, Lk, p):
    from segdino3d_amd import ops
    d = dev()
    got = ops.attention_dropout_keep(key_tensor(KEY, d), CALL, H, Lq, Lk, p)
    assert got.dtype == torch.bool and got.shape == (H, Lq, Lk)
    assert torch.equal(got.cpu(), mask(Lq, Lk, p))


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("shape", FWD)
def test_fp32_forward(shape, D, p):
    from segdino3d_amd import ops
    d = dev()
    out = run(shape, D, p, d)
    assert out.shape == (shape[0], H * D)
    close(out, reference(shape, D, p), f"fp32 forward {shape} x {D} channels, p = {p}", 2e-5)
    if shape == SPLIT:
        assert ops.attention_launch_config(shape[0], shape[1], H, D) == (4, 4)                # four waves, keys split four ways


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("shape", [s for s in FWD if s[1] >= 65])
def test_bf16_forward(shape, D, p):
    d = dev()
    nsrc = shape[2]
    c = inputs(shape, D)
    v = views(c["pack_q"], c["pack_k"], c["C"], nsrc)[2]
    rounded, exact = reference(shape, D, p, rounded=True), reference(shape, D, p)            # bf16 Q (pre-scaled), K, V
    fp32 = run(shape, D, p, d)
    out = run(shape, D, p, d, bf16=True).cpu().double()
    vmax = v.abs().max().item()
    e_model, e_exact = (out - rounded).abs().max().item(), (out - exact).abs().max().item()
    print(f"bf16 forward {shape} x {D}, p = {p}: {e_model / vmax:.2e} |v|max from the rounded-operand model, {e_exact / vmax:.2e} from exact attention")
    assert e_model <= 4e-3 * vmax
    assert e_exact <= 3e-2 * vmax
    assert not torch.equal(out.float(), fp32.cpu())                                            # the bf16 kernel really ran


@pytest.mark.parametrize("D", [32, 64])
def test_key_split_does_not_change_the_mask(D):
    """the same attention with the workspace that splits the keys four ways and with none (one pass): both within the forward bound
    of ONE reference mask"""
    from segdino3d_amd import _lib, ops
    d = dev()
    lib = _lib.load()
    Lq, Lk, nsrc, _ = SPLIT
    p = 0.5
    c = inputs(SPLIT, D)
    q, k, v, q2, k2 = (t.contiguous() for t in views(c["pack_q"].to(d), c["pack_k"].to(d), c["C"], nsrc))
    bits, key = c["bits"].to(d), key_tensor(KEY, d)
    full = lib.sd3d_attention_ws_bytes(Lq, H, D)
    ws = torch.empty(full, dtype=torch.uint8, device=d)
    outs = []
    for nbytes, want in ((full, 4), (0, 1)):
        nw, ks = C.c_int(0), C.c_int(0)
        _lib.check(lib.sd3d_attention_config(Lq, Lk, H, D, nbytes, C.byref(nw), C.byref(ks)), "config")
        assert ks.value == want
        out = torch.full((Lq, H * D), float("nan"), device=d)
        _lib.check(lib.sd3d_attention(q.data_ptr(), H * D, q2.data_ptr(), H * D, k.data_ptr(), H * D, k2.data_ptr(), H * D, v.data_ptr(), H * D,
                                      bits.data_ptr(), Lq, Lk, H, D, c["scale"], out.data_ptr(), H * D, None, 0,
                                      ws.data_ptr() if nbytes else None, nbytes, key.data_ptr(), CALL, p, ops._stream()), "attention")
        close(out, reference(SPLIT, D, p), f"key split {want}, {D} channels", 2e-5)
        outs.append(out)
    assert not torch.equal(outs[0], outs[1])                                                   # two different summation orders did run


def _grads(shape, D, p, d, call=CALL, key=KEY, **kw):
    """(out, pq.grad, pk.grad) of train_dec.attention on strided views of the packed projections"""
    from segdino3d_amd import train_dec as T
    Lq, Lk, nsrc, masked = shape
    c = inputs(shape, D)
    pq, pk = c["pack_q"].to(d).requires_grad_(True), c["pack_k"].to(d).requires_grad_(True)
    q, k, v, q2, k2 = views(pq, pk, c["C"], nsrc)
    bits = None if c["bits"] is None else c["bits"].to(d)
    if p is not None:
        kw = dict(dropout_p=p, key=key_tensor(key, d), call=call)
    out = T.attention(q, k, v, H, c["scale"], mask_bits=bits, q2=q2, k2=k2, **kw)
    out.backward(c["dy"].to(d))
    return out.detach(), pq.grad, pk.grad


@functools.lru_cache(maxsize=None)
def reference_grads(shape, D, p, call=CALL):
    Lq, Lk, nsrc, masked = shape
    c = inputs(shape, D)
    q64, k64 = c["pack_q"].double().requires_grad_(True), c["pack_k"].double().requires_grad_(True)
    q, k, v, q2, k2 = views(q64, k64, c["C"], nsrc)
    ref = attention64_dropout(q, k, v, H, c["scale"], mask(Lq, Lk, p, call), p, c["blocked"], q2=q2, k2=k2)
    ref.backward(c["dy"].double())
    return ref.detach(), q64.grad, k64.grad


def _blocks(gq, gk, Cw, nsrc):
    names = [("dq", gq[:, :Cw]), ("dk", gk[:, :Cw]), ("dv", gk[:, 2 * Cw:])]
    return names + ([("dq1", gq[:, Cw:]), ("dk1", gk[:, Cw:2 * Cw])] if nsrc == 2 else [])


@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("shape", GRAD)
def test_gradients(shape, D):
    d = dev()
    p = 0.1
    Cw, nsrc = H * D, shape[2]
    ref, rq, rk = reference_grads(shape, D, p)
    out, gq, gk = _grads(shape, D, p, d)
    close(out, ref, f"output {shape} x {D}", 2e-5)
    for (name, got), (_, want) in zip(_blocks(gq, gk, Cw, nsrc), _blocks(rq, rk, Cw, nsrc)):
        close(got, want, f"{name} {shape} x {D}", 3e-5)
    if nsrc == 1:                                              # the unused second-source columns
        assert float(gq[:, Cw:].abs().max()) == 0.0 and float(gk[:, Cw:2 * Cw].abs().max()) == 0.0


@pytest.mark.parametrize("D", [32, 64])
def test_rate_zero_is_the_plain_node(D):
    d = dev()
    plain = _grads(MASKED, D, None, d)
    zero = _grads(MASKED, D, None, d, dropout_p=0.0)
    keyed = _grads(MASKED, D, 0.0, d)
    for a, b, c in zip(plain, zero, keyed):
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("D", [32, 64])
def test_same_key_and_call_give_the_same_bits(D):
    d = dev()
    first = _grads(MASKED, D, 0.5, d)
    again = _grads(MASKED, D, 0.5, d)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    other_call = run(MASKED, D, 0.5, d, call=CALL + 1)
    other_key = run(MASKED, D, 0.5, d, key=(KEY[0] ^ 1, KEY[1]))
    assert not torch.equal(other_call, first[0]) and not torch.equal(other_key, first[0]) and not torch.equal(other_call, other_key)


@pytest.mark.parametrize("D", [32, 64])
def test_fully_dropped_rows_give_zeros_and_finite_gradients(D):
    """query 0 of the masked case is open to the last key and, by the case's open diagonal, to key 0 only: with p = 0.5 and a call for
    which both heads drop both, the row's output is zero (not NaN: l and lse are those of the attention without dropout) and every
    gradient is finite and within the bound"""
    d = dev()
    Lq, Lk, nsrc, _ = MASKED
    p = 0.5
    open_keys = (~inputs(MASKED, D)["blocked"][0]).nonzero().flatten().numpy()
    assert list(open_keys) == [0, Lk - 1]
    call = next(c for c in range(512) if not keep_mask(KEY, c, H, 1, Lk, p)[:, 0, open_keys].any())
    out, gq, gk = _grads(MASKED, D, p, d, call=call)
    assert float(out[0].abs().max()) == 0.0
    assert torch.isfinite(out).all() and torch.isfinite(gq).all() and torch.isfinite(gk).all()
    assert float(gq[0].abs().max()) == 0.0                         # dS = P o (0 - D) with D = dO . O = 0
    ref, rq, rk = reference_grads(MASKED, D, p, call)
    close(out, ref, f"output, call {call}", 2e-5)
    for (name, got), (_, want) in zip(_blocks(gq, gk, H * D, nsrc), _blocks(rq, rk, H * D, nsrc)):
        close(got, want, f"{name}, call {call}", 3e-5)


def test_nothing_of_the_size_of_the_probabilities_is_allocated():
    from segdino3d_amd import train_dec as T
    d = dev()
    Lq, Lk, heads, D = 512, 2048, 8, 32
    gen = torch.Generator().manual_seed(0)
    q = torch.randn(Lq, heads * D, generator=gen).to(d).requires_grad_(True)
    k = torch.randn(Lk, heads * D, generator=gen).to(d).requires_grad_(True)
    v = torch.randn(Lk, heads * D, generator=gen).to(d).requires_grad_(True)
    dy = torch.randn(Lq, heads * D, generator=gen).to(d)
    key = key_tensor(KEY, d)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    T.attention(q, k, v, heads, D ** -0.5, dropout_p=0.1, key=key, call=0).backward(dy)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"forward + backward at {Lq} x {Lk} x {heads} heads: peak rises by {rise / 2 ** 20:.2f} MiB (one probability tensor: {heads * Lq * Lk * 4 / 2 ** 20:.0f} MiB)")
    assert rise < heads * Lq * Lk * 4
    assert all(torch.isfinite(t.grad).all() for t in (q, k, v))


@pytest.mark.parametrize("heads", [8, 4])
def test_decoder_equals_its_explicit_cross_check(heads, monkeypatch):
    """dropout=0.1 in training: the fused path against SD3D_ATTN_DROPOUT=explicit (probabilities formed explicitly, the SAME keep mask
    from the mask kernel, torch's autograd) under the same seed: outputs within the decoder goldens' 3e-4 abs + rel, parameter
    gradients within 2e-3 relative L2"""
    from decoder_grad_case import objective
    from test_gpu_decoder import _build_decoder
    from test_oracle_golden import load
    d = dev()
    g = load("decoder_s96_q16")
    dec, _ = _build_decoder(dict(dropout=0.1, num_heads=heads))
    dec.to(d).train()
    ids = g["query_ids"].long()
    t = lambda a: a.to(d)  # noqa: E731
    pick = lambda o: {k: (None if o.get(k) is None or o[k][0] is None else o[k][0]) for k in ("cls_preds", "masks", "centers", "sizes", "sem_preds")}  # noqa: E731

    def step(route):
        if route == "explicit":
            monkeypatch.setenv("SD3D_ATTN_DROPOUT", "explicit")
        else:
            monkeypatch.delenv("SD3D_ATTN_DROPOUT", raising=False)
        dec.zero_grad(set_to_none=True)
        torch.manual_seed(5)
        out = dec([t(g["x"].detach())], [t(g["pos"])], [t(g["pos_wo"])], [t(g["x"].detach()[ids])], [t(g["pos"][ids])], [t(g["q2d_feat"])],
                  [t(g["q2d_pos"])], [(t(g["lo"]), t(g["hi"]))])
        objective([pick(z) for z in out["aux_outputs"]] + [pick(out)]).backward()
        return out, {n: p.grad.detach().double() for n, p in dec.named_parameters() if p.grad is not None}
    fused, gf = step("fused")
    twin, gt = step("explicit")
    for name in ("cls_preds", "masks"):
        a, b = fused[name][0].detach(), twin[name][0].detach()
        bad = ((a - b).abs() > 3e-4 + 3e-4 * b.abs()).any(dim=1).float().mean().item()
        print(f"{heads} heads, {name}: max difference {float((a - b).abs().max()):.3e}, rows outside 3e-4: {bad:.1%}")
        assert bad == 0.0, name
    assert set(gf) == set(gt) and len(gf) > 150
    norms = sorted(float(v.norm()) for v in gt.values())
    floor = 1e-2 * norms[len(norms) // 2]                          # key biases have a true gradient of zero (decoder_grad_case.compare)
    worst = sorted(((float((gf[n] - gt[n]).norm()) / max(float(gt[n].norm()), floor), n) for n in gt), reverse=True)
    print(f"{heads} heads, worst parameter gradients, fused vs explicit:", worst[:3])
    assert worst[0][0] <= 2e-3, worst[:6]
