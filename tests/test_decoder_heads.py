"""64-channel attention heads (num_heads=4 at d_model=256), CPU side: the constructor gate, the oracle pinned to the golden vector
captured from the imported reference (tests/golden/make_golden_heads.py), and the float64 restatement of attention that the GPU
tests compare against (tests/attention_heads_case.py) pinned to the oracle's attention_core."""
import pytest
import torch

from attention_heads_case import attention64, case, views
from test_oracle_golden import decoder_state_dict, load

DEC_KW = dict(add_dinox_query_ca=True, add_dinox_query_ca_mask=True, dinox_query_ca_mask_threshold=0.2, num_layers=6,
              num_instance_queries=0, num_semantic_queries=0, num_instance_classes=198, num_semantic_classes=200,
              num_semantic_linears=1, in_channels=96, d_model=256, num_heads=8, hidden_dim=1024, dropout=0.0,
              activation_fn="gelu", iter_pred=True, attn_mask=True, fix_attention=True, objectness_flag=False,
              add_box_size_pred=True, add_positional_embedding=True, pos_type="sine", temperature=20,
              box_modulate_ca=True, normalize_box_prediction=True)            # the ScanNet200 decoder (test_gpu_decoder.DEC_KW)


def test_constructor_accepts_32_and_64_channel_heads_only():
    from segdino3d_amd.decoder import ScanNetQueryDecoder
    dec = ScanNetQueryDecoder(**dict(DEC_KW, num_heads=4))
    assert dec.num_heads == 4 and dec.d_model == 256
    assert dec.eval()._fusable() == 0                         # wide heads never take the row-chain path
    assert ScanNetQueryDecoder(**DEC_KW).num_heads == 8
    for heads in (16, 2):                                     # 16- and 128-channel heads
        with pytest.raises(NotImplementedError) as e:
            ScanNetQueryDecoder(**dict(DEC_KW, num_heads=heads))
        assert "32" in str(e.value) and "64" in str(e.value)


def test_oracle_reproduces_the_reference_with_four_heads():
    from oracle import decoder_ref as D
    g = load("decoder_h4_s96_q16")
    sd = decoder_state_dict()
    ids = g["query_ids"].long()
    out = D.decoder_forward(sd, D.DecoderCfg(num_heads=4), g["x"], g["pos"], g["pos_wo"], g["x"][ids], g["pos"][ids],
                            g["q2d_feat"], g["q2d_pos"], g["lo"], g["hi"])
    tol = dict(rtol=2e-4, atol=2e-4)
    for li in range(6):
        torch.testing.assert_close(out["aux"][li]["cls_preds"], g[f"aux{li}_cls"], **tol)
        torch.testing.assert_close(out["aux"][li]["masks"], g[f"aux{li}_masks"], **tol)
        if li > 0:
            torch.testing.assert_close(out["aux"][li]["centers"], g[f"aux{li}_centers"], **tol)
            torch.testing.assert_close(out["aux"][li]["sizes"], g[f"aux{li}_sizes"], **tol)
    for k in ("cls_preds", "sem_preds", "masks", "centers", "sizes", "hidden_states"):
        torch.testing.assert_close(out[k], g[k], **tol)
    # the 8-head fixture on the same inputs differs: the head count really entered the reference's run
    assert not torch.allclose(g["masks"], load("decoder_s96_q16")["masks"], atol=1e-2)


def test_float64_attention_equals_the_oracle_attention_core():
    from oracle.decoder_ref import attention_core
    Lq, Lk, H, D = 37, 70, 3, 64
    c = case(Lq, Lk, H, D, 1, True)
    q, k, v, _, _ = views(c["pack_q"], c["pack_k"], c["C"], 1)
    ref = attention_core(q.double(), k.double(), v.double(), H, c["blocked"])
    got = attention64(q, k, v, H, D ** -0.5, c["blocked"])
    assert (got - ref).abs().max().item() <= 1e-6
    # two sources are the per-head concatenation [q | q2] . [k | k2]
    c = case(Lq, Lk, H, D, 2, True)
    q, k, v, q2, k2 = views(c["pack_q"], c["pack_k"], c["C"], 2)
    cat = lambda a, b, L: torch.cat([a.reshape(L, H, D), b.reshape(L, H, D)], 2).reshape(L, 2 * H * D).double()  # noqa: E731
    ref = attention_core(cat(q, q2, Lq), cat(k, k2, Lk), v.double(), H, c["blocked"])
    got = attention64(q, k, v, H, c["scale"], c["blocked"], q2=q2, k2=k2)
    assert (got - ref).abs().max().item() <= 1e-6


def test_c_entry_points_refuse_other_widths_and_report_the_split():
    """Host-side contract of the attention entry points (no launch): 16 / 128 channels -> SD3D_ERR_ARG and a zero workspace size;
    the partial-state layout (64 + 32 * head_dim floats, at most 8 splits) in the workspace size; the launcher's choice at the
    key-split shape of the GPU tests."""
    import ctypes as C
    from segdino3d_amd import _lib, ops
    lib = _lib.load()
    for bad in (16, 128, 0, 48):
        assert lib.sd3d_attention_ws_bytes(40, 2, bad) == 0 and lib.sd3d_attention_backward_ws_bytes(40, 2, bad) == 0
        assert lib.sd3d_attention(None, 0, None, 0, None, 0, None, 0, None, 0, None, 8, 8, 2, bad, 1.0, None, 0, None, 0, None, 0, None, 0, 0.0, None) != 0
        assert b"32 or 64" in lib.sd3d_last_error()
        assert lib.sd3d_attention_batch(1, None, 2, bad, 1.0, 0, None, 0, None) != 0
        assert lib.sd3d_attention_backward(*([None, 0] * 5 + [None, 8, 8, 2, bad, 1.0, None, 0, None, None, 0] + [None, 0] * 5 + [None, 0, None, 0, 0.0, None])) != 0
        nw, ks = C.c_int(), C.c_int()
        assert lib.sd3d_attention_config(40, 1030, 2, bad, 1 << 20, C.byref(nw), C.byref(ks)) != 0
    assert lib.sd3d_attention_ws_bytes(40, 2, 64) == 2 * 2 * 8 * (64 + 2048) * 4
    assert lib.sd3d_attention_ws_bytes(40, 2, 32) == 2 * 2 * 8 * (64 + 1024) * 4
    assert ops.attention_launch_config(40, 1030, 2, 64) == (4, 4)
    assert ops.attention_launch_config(200, 3000, 8, 32) == (4, 8) and ops.attention_launch_config(3000, 3000, 8, 32) == (8, 1)
    assert ops.attention_launch_config(3000, 3000, 4, 64) == (4, 1)
    for H, C_ in ((2, 256), (16, 256), (3, 256)):
        with pytest.raises(ValueError, match="32 or 64"):
            ops.head_width(torch.zeros(1, C_), torch.zeros(1, C_), H, "attention")
