"""Attention dropout without a GPU: the numpy restatement of the keep mask (tests/attention_dropout_case.py) reproduces the
Random123 known answers of Philox4x32-10 and has the statistics the scaling by 1 / (1 - p) assumes; `train_dec.attention` takes
the dropout arguments and refuses a rate outside [0, 1) before it touches the library; the decoder's training namespace sends
p > 0 to the fused node."""
import numpy as np
import pytest
import torch

from attention_dropout_case import KEY, keep_mask, philox4x32_10, threshold

KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
H, LQ, LK = 2, 200, 301
N = H * LQ * LK


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    assert " ".join(f"{int(w):08x}" for w in philox4x32_10(counter, key)) == want


def test_philox_is_elementwise():
    """arrays of counters give what the scalar calls give"""
    c = [np.array([0, 0xFFFFFFFF, KAT[2][0][i]]) for i in range(4)]
    for j, (counter, _, _) in enumerate(KAT):
        got = philox4x32_10(c, KAT[2][1])
        assert [int(w[j]) for w in got] == [int(w) for w in philox4x32_10(counter, KAT[2][1])]


def test_threshold_is_the_rate():
    assert threshold(0.5) == 2 ** 31 and threshold(0.0) == 0
    assert threshold(0.1) == int(np.float32(0.1).astype(np.float64) * 2 ** 32) < 2 ** 32
    assert abs(threshold(0.1) / 2 ** 32 - float(np.float32(0.1))) == 0.0          # realised rate = the fp32 p exactly


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate(p):
    rate = keep_mask(KEY, 0, H, LQ, LK, p).mean()
    print(f"p = {p}: keep rate {rate:.6f}")
    assert abs(rate - (1 - p)) <= 4 * np.sqrt(p * (1 - p) / N)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_calls_and_heads_are_independent(p):
    a = (1 - p) ** 2 + p ** 2                                      # share on which two independent masks agree
    bound = 4 * np.sqrt(a * (1 - a) / N)
    m0, m1 = keep_mask(KEY, 0, H, LQ, LK, p), keep_mask(KEY, 1, H, LQ, LK, p)
    calls, heads = (m0 == m1).mean(), (m0[0] == m0[1]).mean()
    print(f"p = {p}: calls 0 / 1 agree on {calls:.6f}, heads 0 / 1 on {heads:.6f} (independent: {a:.6f} +- {bound:.6f})")
    assert abs(calls - a) <= bound
    assert abs(heads - a) <= bound


def test_mask_depends_on_nothing_but_its_coordinates():
    """a sub-block of a larger mask is the mask of the smaller problem: Lq and Lk do not enter"""
    big, small = keep_mask(KEY, 3, 2, 40, 70, 0.5), keep_mask(KEY, 3, 1, 33, 31, 0.5)
    assert np.array_equal(big[:1, :33, :31], small)


def test_attention_takes_dropout_arguments_and_refuses_bad_rates(monkeypatch):
    from segdino3d_amd import _lib, train_dec as T

    def no_library():
        raise AssertionError("the library must not be touched")
    monkeypatch.setattr(_lib, "load", no_library)
    q = torch.zeros(4, 64)
    key = torch.zeros(2, dtype=torch.int32)
    for p in (1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            T.attention(q, q, q, 2, 1.0, dropout_p=p, key=key, call=0)
    with pytest.raises(ValueError, match="key"):
        T.attention(q, q, q, 2, 1.0, dropout_p=0.1)
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        from segdino3d_amd import ops
        ops.attention_dropout_keep(key, 0, 2, 4, 4, 1.0)


def test_training_namespace_routes_dropout_to_the_fused_node(monkeypatch):
    from segdino3d_amd import decoder, train_dec as T
    calls = []

    def explicit(*a, **kw):
        raise AssertionError("the explicit-probability route must not run")

    def fused(q, k, v, num_heads, scale, mask_bits=None, q2=None, k2=None, dropout_p=0.0, key=None, call=0):
        calls.append((dropout_p, key, call))
        return q
    monkeypatch.setattr(T, "attention_dropout", explicit)
    monkeypatch.setattr(T, "attention", fused)
    monkeypatch.delenv("SD3D_ATTN_DROPOUT", raising=False)
    tls = decoder._F_TLS
    key = torch.zeros(2, dtype=torch.int32)
    q = torch.zeros(4, 64)
    monkeypatch.setattr(tls, "p", 0.25, raising=False)
    monkeypatch.setattr(tls, "key", key, raising=False)
    monkeypatch.setattr(tls, "call", 0, raising=False)
    decoder._TrainF.attention(q, q, q, 2, 1.0)
    decoder._TrainF.attention(q, q, q, 2, 1.0, keys="q")
    assert [(p, c) for p, _, c in calls] == [(0.25, 0), (0.25, 1)] and all(k is key for _, k, _ in calls)
    assert tls.call == 2
    monkeypatch.setattr(tls, "p", 0.0, raising=False)
    decoder._TrainF.attention(q, q, q, 2, 1.0)
    assert calls[-1] == (0.0, None, 0)                             # rate 0: today's call, no key


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """p outside [0, 1), p > 0 with a NULL key or an unsupported head width: SD3D_ERR_ARG from the three C entry points, nothing launched (no GPU here)"""
    import ctypes as C
    from segdino3d_amd import _lib
    lib = _lib.load()
    words = (C.c_uint32 * 2)(1, 2)
    key = C.addressof(words)
    fwd = lambda D, k, p: lib.sd3d_attention(*([None, 0] * 5 + [None, 8, 8, 2, D, 1.0, None, 0, None, 0, None, 0, k, 0, p, None]))  # noqa: E731
    bwd = lambda D, k, p: lib.sd3d_attention_backward(*([None, 0] * 5 + [None, 8, 8, 2, D, 1.0, None, 0, None, None, 0] + [None, 0] * 5  # noqa: E731
                                                        + [None, 0, k, 0, p, None]))
    for f in (fwd, bwd):
        for D, k, p in ((32, key, 1.0), (32, key, -0.5), (64, key, float("nan")), (32, None, 0.1), (48, key, 0.1), (128, key, 0.0)):
            assert f(D, k, p) != 0, (D, k, p)
    for k, p in ((key, 1.0), (key, -0.1), (None, 0.5)):
        assert lib.sd3d_attention_dropout_keep(k, 0, 2, 8, 8, p, key, None) != 0
    assert lib.sd3d_attention_dropout_keep(key, 0, 2, 8, 8, 0.5, None, None) != 0
