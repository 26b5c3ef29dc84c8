"""tests/decoder_kernel_cases.py on the CPU: every float64 reference equals an independent formulation (torch's own LayerNorm / GELU /
sigmoid under float64 autograd, `oracle/decoder_ref.py` for the encodings and `inverse_sigmoid`), the planted situations are present,
the fp32 evaluation of each reference passes the tolerance rule by itself, and the wrappers refuse wrong shapes before they touch a
device."""
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from oracle import decoder_ref as D
from tests import decoder_kernel_cases as K

F64, F32 = torch.float64, torch.float32


def d64(t):
    return None if t is None else t.double()


def close(a, b, tol=1e-12):
    scale = max(1.0, float(b.abs().max())) if b.numel() else 1.0
    assert a.shape == b.shape and float((a - b).abs().max() if b.numel() else 0.0) <= tol * scale, float((a - b).abs().max())


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D_", K.LN_D)
@pytest.mark.parametrize("with_res", [False, True])
def test_layernorm_references_equal_torch(D_, with_res):
    for M in (1, 5):
        c = K.ln_case(M, D_, planted=False)
        for relu in (False, True):
            x, w, b = (d64(c[k]).clone().requires_grad_(True) for k in ("x", "w", "b"))
            res = d64(c["res"]).clone().requires_grad_(True) if with_res else None
            y = F.layer_norm(x if res is None else x + res, (D_,), w, b, K.EPS)
            y = torch.relu(y) if relu else y
            close(K.layernorm_ref(d64(c["x"]), d64(c["res"]) if with_res else None, d64(c["w"]), d64(c["b"]), relu=relu), y.detach())
            dy = d64(c["dy"])
            y.backward(dy)
            dxin, dw, db, g, gxh = K.layernorm_bwd_ref(dy, y.detach() if relu else None, d64(c["x"]), d64(c["res"]) if with_res else None, d64(c["w"]))
            close(dxin, x.grad)
            close(dw, w.grad)
            close(db, b.grad)
            if with_res:
                close(dxin, res.grad)


def test_layernorm_planted_rows():
    one_pass_errors = []
    for M in K.LN_M:
        for D_ in K.LN_D:
            c = K.ln_case(M, D_)
            for res in (None, c["res"]):
                v = d64(c["x"]) if res is None else d64(c["x"]) + d64(res)
                big = v[c["big"]]
                assert float(big.mean()) == 1000.0 and (D_ < 96 or 0.6 < float(big.std()) < 1.5)
                r32 = (c["x"] if res is None else c["x"] + res)[c["big"]]
                assert torch.equal(r32.double(), big) and float(r32.sum()) == 1000.0 * D_ and float(r32.flip(0).cumsum(0)[-1]) == 1000.0 * D_
                y64 = K.layernorm_ref(d64(c["x"]), d64(res), d64(c["w"]), d64(c["b"]))
                y32 = K.layernorm_ref(c["x"], res, c["w"], c["b"])
                if c["const"] is not None:
                    assert float(v[c["const"]].var(unbiased=False)) == 0.0
                    assert torch.equal(y64[c["const"]], d64(c["b"])) and torch.equal(y32[c["const"]], c["b"])
                # the one-pass variance E[x^2] - mean^2 in fp32 is what the big row is for: it is off by more than the row's spread allows
                r = (c["x"] if res is None else c["x"] + res)[c["big"]]
                one_pass = float((r * r).mean() - r.mean() ** 2)
                one_pass_errors.append(abs(one_pass - float(big.var(unbiased=False))))
    print(f"[decoder-case] one-pass fp32 variance of the big rows: off by {min(one_pass_errors):.1e} .. {max(one_pass_errors):.1e}")
    assert max(one_pass_errors) > 1e-2 and sum(e > 1e-4 for e in one_pass_errors) > len(one_pass_errors) // 2


def test_relu_mask_plant():
    y, spots = K.plant_relu_mask(torch.ones(2, 4))
    assert spots == dict(zero=0, minus_zero=1, denormal=2)
    f = y.view(-1)
    assert float(f[0]) == 0.0 and math.copysign(1.0, float(f[1])) == -1.0 and 0.0 < float(f[2]) < 1.5e-45
    assert (f > 0).tolist()[:4] == [False, False, True, True]
    dy = torch.full((2, 4), 2.0)
    _, _, _, g, _ = K.layernorm_bwd_ref(dy, y, torch.randn(2, 4), None, torch.ones(4))
    assert g.view(-1).tolist()[:4] == [0.0, 0.0, 2.0, 2.0]


# ---- activations ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", K.ACTS)
def test_activation_derivatives_equal_autograd(act):
    fwd = {None: lambda z: z, "relu": torch.relu, "gelu": lambda z: F.gelu(z), "sigmoid": torch.sigmoid}[act]
    g = K.gen(1, 2, 3)
    z = torch.cat([2.0 * torch.randn(500, generator=g, dtype=F64), torch.tensor(K.GELU_Z, dtype=F64)]).requires_grad_(True)
    dy = torch.randn(z.numel(), generator=g, dtype=F64)
    y = fwd(z)
    y.backward(dy)
    ref = z.detach() if act in (None, "gelu") else y.detach()
    close(K.act_backward_ref(dy, ref, act), z.grad, 1e-13)
    assert bool(torch.isfinite(K.act_backward_ref(dy, ref, act)).all())


def test_activation_plants():
    c = K.act_case("gelu", 5, 3)
    assert c["ref"].view(-1)[:11].tolist() == [float(torch.tensor(v, dtype=F32)) for v in K.GELU_Z] and c["planted"] == 11
    c = K.act_case("sigmoid", 5, 3)
    assert c["ref"].view(-1)[:4].tolist() == [0.0, 1.0, float(torch.tensor(1e-7)), 1.0 - 2.0 ** -24]
    c = K.act_case("relu", 5, 3)
    f = c["ref"].view(-1)
    assert float(f[0]) == 0.0 and math.copysign(1.0, float(f[1])) == -1.0 and float(f[2]) == K.DENORM
    assert K.act_backward_ref(c["dy"], c["ref"], "relu").view(-1)[:3].tolist() == [0.0, 0.0, float(c["dy"].view(-1)[2])]
    assert K.act_case("gelu", 1, 1)["planted"] == 1


# ---- column sums ------------------------------------------------------------------------------------------------------------------------
def test_col_sum_chain_and_data():
    assert [K.col_sum_chain(M) for M in (1, 16, 17, 8192, 8193, 8257)] == [1, 1, 2, 512, 16, 16]
    x = K.csum_case(17, 65)
    assert x.dtype == F32 and abs(float(x.mean()) - 1000) < 1
    # dropping one addend is far outside the bound
    assert float((x[0].double().abs() / K.col_sum_bound(x)).min()) > 1e3
    for M, factor in ((8191, 3), (8192, 3), (8193, 50), (8192 + 65, 50)):       # the 512-addend chains of the one-launch path: still 4 x the bound
        x = K.csum_case(M, 1)
        assert float((x[-1].double().abs() / K.col_sum_bound(x)).min()) > factor


# ---- positional encodings ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d_pos", K.SINE_D)
def test_pe_tables_equal_the_decoder_s(d_pos):
    from segdino3d_amd.decoder import ScanNetQueryDecoder
    dim_t, axis = K.pe_tables(d_pos)
    stand_in = SimpleNamespace(d_model=d_pos, temperature=K.TEMPERATURE, _pe_tables={})
    dt, ax = ScanNetQueryDecoder.pe_tables(stand_in, torch.device("cpu"))
    assert torch.equal(dim_t, dt) and torch.equal(axis, ax) and dim_t.dtype == F32 and axis.dtype == torch.int8
    assert dim_t.numel() == d_pos and [int((axis == a).sum()) for a in range(3)] == D.pe_channel_plan(d_pos, 3)


@pytest.mark.parametrize("d_pos", K.SINE_D)
def test_sine_pe_reference_equals_the_oracle(d_pos):
    dim_t, axis = K.pe_tables(d_pos)
    for n in K.PE_N:
        p = K.pe_case(n)
        for s in (0, 2):
            rows = p["row_scene"] == s
            if not bool(rows.any()):
                continue
            lo, hi = K.SCENE_RANGES[s, :3].double(), K.SCENE_RANGES[s, 3:].double()
            xyz = p["xyz"][rows].double()
            ours = K.sine_pe_ref(xyz, p["rng_rows"][rows].double(), dim_t, axis)
            close(ours, D.sine_pe(xyz, lo, hi, K.TEMPERATURE, d_pos), 1e-12)
            mod = (p["mod_num"] / p["den2"])[rows].double()
            ours = K.sine_pe_ref(xyz, p["rng_rows"][rows].double(), dim_t, axis, p["mod_num"][rows].double(), p["den2"][rows].double())
            close(ours, D.sine_pe(xyz, lo, hi, K.TEMPERATURE, d_pos, modulated=p["mod_num"][rows].double() / p["den2"][rows].double()), 1e-12)
            assert mod.shape == (int(rows.sum()), 3)


@pytest.mark.parametrize("d_pos", K.FOURIER_D)
def test_fourier_pe_reference_equals_the_oracle(d_pos):
    gb = K.gauss_b(d_pos)
    assert gb.shape == (3, d_pos // 2 + 5)
    for n in K.PE_N:
        p = K.pe_case(n)
        for s in (0, 2):
            rows = p["row_scene"] == s
            if not bool(rows.any()):
                continue
            xyz = p["xyz"][rows].double()
            ours = K.fourier_pe_ref(xyz, p["rng_rows"][rows].double(), gb.double(), d_pos)
            close(ours, D.fourier_pe(xyz, K.SCENE_RANGES[s, :3].double(), K.SCENE_RANGES[s, 3:].double(), gb.double(), d_pos), 1e-12)


def test_pe_case_plants():
    assert bool((K.SCENE_RANGES[:, 3:] > K.SCENE_RANGES[:, :3]).all())
    for n in K.PE_N:
        p = K.pe_case(n)
        rs = p["row_scene"]
        assert rs.dtype == torch.int32 and not bool((rs == 1).any())                   # scene 1 owns no row
        u = ((p["xyz"] - p["rng_rows"][:, :3]) / (p["rng_rows"][:, 3:] - p["rng_rows"][:, :3])).double()
        assert float(u.min()) >= -0.5 - 1e-6 and float(u.max()) <= 1.5 + 1e-6 and float(u.max()) > 1.4
        assert p["xyz"].stride(0) == 6 and p["pts"].shape == (n, 6)
        if n > 1:
            assert float(u.min()) < -0.4 and rs.tolist() != sorted(rs.tolist()) and {0, 2} == set(rs.tolist())
    assert any((n * d) % 256 for n in K.PE_N for d in K.SINE_D)
    for n in (1, 3, 5, 200):
        p, q = K.pe_case(n), K.pe_case_one_scene(n)
        assert q["pts"].shape == (n, 6) and q["xyz"].stride(0) == 6 and bool((q["rng_rows"] == K.SCENE_RANGES[2]).all())
        u = lambda c: ((c["xyz"] - c["rng_rows"][:, :3]) / (c["rng_rows"][:, 3:] - c["rng_rows"][:, :3])).double()  # noqa: E731
        assert float((u(p) - u(q)).abs().max()) < 1e-5 and torch.equal(p["mod_num"], q["mod_num"])


@pytest.mark.parametrize("d_pos", K.SINE_D)
def test_sine_pe_mod_backward_reference_equals_autograd(d_pos):
    dim_t, axis = K.pe_tables(d_pos)
    for n in (1, 5):
        p = K.pe_case_one_scene(n)
        rng = p["rng_rows"].double()
        for den in (p["den1"], p["den2"]):
            num = p["mod_num"].double().clone().requires_grad_(True)
            out = K.sine_pe_ref(p["xyz"].double(), rng, dim_t, axis, num, den.double())
            d_out = torch.randn(n, d_pos, generator=K.gen(5, n, d_pos), dtype=F64)
            out.backward(d_out)
            close(K.sine_pe_mod_bwd_ref(d_out, p["xyz"].double(), rng, dim_t, axis, den.double()), num.grad, 1e-12)


# ---- box refinement ---------------------------------------------------------------------------------------------------------------------
def test_inverse_sigmoid_equals_the_oracle():
    x = torch.tensor(K.SIZE_PREV + [0.3, 0.999], dtype=F32)
    for dt in (F64, F32):
        assert torch.equal(K.inverse_sigmoid(x.to(dt)), D.inverse_sigmoid(x.to(dt), eps=1e-5))
    z = K.inverse_sigmoid(x.double())
    assert bool(torch.isfinite(z).all()) and float(z[0]) == float(z[6]) == math.log(1e-5 / 1.0) and float(z[5]) == float(z[7]) == math.log(1.0 / 1e-5)
    assert abs(float(z[1]) - math.log(1e-5 / (1 - 1e-6))) < 1e-9                       # 1e-6 sits below eps: the eps branch of x
    assert abs(float(z[4]) - math.log(1e5)) < 2e-6                                     # 1 - 1e-6: the eps branch of 1 - x


@pytest.mark.parametrize("Q", K.BOX_Q)
@pytest.mark.parametrize("normalize", [0, 1])
def test_box_refine_reference_equals_autograd(Q, normalize):
    c = K.box_case(Q)
    ext = (c["rng_rows"][:, 3:] - c["rng_rows"][:, :3]).double()
    for sp in (c["sp1"], c["sp2"]):
        dc, ds = c["dc"].double().clone().requires_grad_(True), c["ds"].double().clone().requires_grad_(True)
        center = c["ref"].double() + dc
        if normalize:
            size = torch.sigmoid(D.inverse_sigmoid(sp.double().expand(Q, 3), eps=1e-5) + ds)
            metric = size * ext
        else:
            size = sp.double() + ds
            metric = size
        r_center, r_size, r_metric = K.box_refine_ref(c["ref"].double(), c["dc"].double(), sp.double(), c["ds"].double(), c["rng_rows"].double(), normalize)
        close(r_center, center.detach(), 0) and close(r_size, size.detach(), 1e-15) and close(r_metric, metric.detach(), 1e-15)
        assert bool(torch.isfinite(r_size).all()) and bool(torch.isfinite(r_metric).all())
        ((center * c["g_center"].double()).sum() + (metric * c["g_metric"].double()).sum()).backward()
        d_dc, d_ds = K.box_refine_bwd_ref(c["g_center"].double(), c["g_metric"].double(), r_size, c["rng_rows"].double(), normalize)
        close(d_dc, dc.grad, 0)
        close(d_ds, ds.grad, 1e-14)
        d_dc, d_ds = K.box_refine_bwd_ref(None, c["g_metric"].double(), r_size, c["rng_rows"].double(), normalize)
        assert not bool(d_dc.any()) and torch.equal(d_ds, K.box_refine_bwd_ref(c["g_center"].double(), c["g_metric"].double(), r_size, c["rng_rows"].double(), normalize)[1])
        d_dc, d_ds = K.box_refine_bwd_ref(c["g_center"].double(), None, r_size, c["rng_rows"].double(), normalize)
        assert not bool(d_ds.any())
    assert K.box_refine_ref(c["ref"], c["dc"], c["sp1"], None, c["rng_rows"], normalize)[1:] == (None, None)


def test_box_case_plants():
    grid = [(s, d) for s in K.SIZE_PREV for d in K.D_SIZE]
    for Q in K.BOX_Q:
        c = K.box_case(Q)
        n = c["planted"]
        assert n == min(56, 3 * Q)
        if Q > 1:
            assert c["sp2"].view(-1)[:n].tolist() == [float(torch.tensor(s, dtype=F32)) for s, _ in grid[:n]]
            assert c["ds"].view(-1)[:n].tolist() == [d for _, d in grid[:n]]
    c = K.box_case(85)
    size = K.box_refine_ref(c["ref"].double(), c["dc"].double(), c["sp2"].double(), c["ds"].double(), c["rng_rows"].double(), 1)[1]
    assert int((size == 1.0).sum()) >= 8 and float(size.min()) > 0.0 and float(size.min()) < 1e-40        # +100 rounds to 1 in float64; -100 does not reach 0
    assert 85 * 3 < 256 < 86 * 3


# ---- transpose --------------------------------------------------------------------------------------------------------------------------
def test_transpose_reference_and_jobs():
    src = K.transpose_src(3, 5, 2, 0)
    ref = K.transpose_ref(src, 8)
    assert ref.shape == (2, 5, 8) and torch.equal(ref[1, :, :3], src[1].T) and not bool(ref[:, :, 3:].any())
    for n in (113, 225):
        jobs = K.small_jobs(n)
        assert len(jobs) == n > (n // K.TB_MAX) * K.TB_MAX and all(ld >= r for r, _, ld, _ in jobs)
        assert len({j[:2] for j in jobs}) > 20 and any(ld == r for r, _, ld, _ in jobs) and any(b == 2 for *_, b in jobs)


# ---- the fp32 evaluation of every reference passes the rule by itself ---------------------------------------------------------------------
def test_fp32_references_pass_the_rule():
    worst = {}

    def note(name, r):
        worst[name] = max(worst.get(name, 0.0), r[0])

    for M in (5, 201):
        for D_ in K.LN_D:
            c = K.ln_case(M, D_)
            for res in (None, c["res"]):
                for relu in (False, True):
                    note("layernorm", K.reference_passes(K.layernorm_ref(d64(c["x"]), d64(res), d64(c["w"]), d64(c["b"]), relu=relu),
                                                         K.layernorm_ref(c["x"], res, c["w"], c["b"], relu=relu), K.layernorm_scale(c["x"], res, c["w"], c["b"])))
            c = K.ln_case(M, D_, planted=False)
            y, _ = K.plant_relu_mask(torch.relu(c["res"]))
            r64 = K.layernorm_bwd_ref(d64(c["dy"]), d64(y), d64(c["x"]), d64(c["res"]), d64(c["w"]))
            r32 = K.layernorm_bwd_ref(c["dy"], y, c["x"], c["res"], c["w"])
            note("layernorm_backward dxin", K.reference_passes(r64[0], r32[0], K.layernorm_bwd_scale(c["dy"], y, c["x"], c["res"], c["w"])))
            bw, bb = K.layernorm_sums_bound(c["dy"], y, c["x"], c["res"], c["w"])       # derived from the kernel's summation order, not torch's:
            assert bool((bw <= 1e-4 * (r64[4].abs().sum(0) + r64[3].abs().sum(0)) + K.FLOOR).all()) and bool((bb <= 1e-4 * r64[3].abs().sum(0) + K.FLOOR).all())
    for act in ("gelu", "sigmoid"):
        for M, C, _ in K.ACT_SHAPES:
            c = K.act_case(act, M, C)
            note("act_backward " + act, K.reference_passes(K.act_backward_ref(d64(c["dy"]), d64(c["ref"]), act), K.act_backward_ref(c["dy"], c["ref"], act),
                                                           K.act_backward_scale(c["dy"], c["ref"], act)))
    for n in K.PE_N:
        p = K.pe_case(n)
        for d_pos in K.SINE_D:
            dim_t, axis = K.pe_tables(d_pos)
            for num, den in ((None, None), (p["mod_num"], p["den1"]), (p["mod_num"], p["den2"])):
                note("sine_pe", K.reference_passes(K.sine_pe_ref(d64(p["xyz"]), d64(p["rng_rows"]), dim_t, axis, d64(num), d64(den)),
                                                   K.sine_pe_ref(p["xyz"], p["rng_rows"], dim_t, axis, num, den),
                                                   K.sine_pe_scale(p["xyz"], p["rng_rows"], dim_t, axis, num, den)))
            d_out = torch.randn(n, d_pos, generator=K.gen(7, n, d_pos))
            q = K.pe_case_one_scene(n)
            for den in (q["den1"], q["den2"]):
                note("sine_pe_mod_backward", K.reference_passes(K.sine_pe_mod_bwd_ref(d64(d_out), d64(q["xyz"]), d64(q["rng_rows"]), dim_t, axis, d64(den)),
                                                                K.sine_pe_mod_bwd_ref(d_out, q["xyz"], q["rng_rows"], dim_t, axis, den),
                                                                K.sine_pe_mod_bwd_scale(d_out, q["xyz"], q["rng_rows"], dim_t, axis, den)))
        for d_pos in K.FOURIER_D:
            gb = K.gauss_b(d_pos)
            note("fourier_pe", K.reference_passes(K.fourier_pe_ref(d64(p["xyz"]), d64(p["rng_rows"]), gb, d_pos), K.fourier_pe_ref(p["xyz"], p["rng_rows"], gb, d_pos),
                                                  K.fourier_pe_scale(p["xyz"], p["rng_rows"], gb, d_pos)))
    for Q in K.BOX_Q:
        c = K.box_case(Q)
        for sp in (c["sp1"], c["sp2"]):
            r64 = K.box_refine_ref(d64(c["ref"]), d64(c["dc"]), d64(sp), d64(c["ds"]), d64(c["rng_rows"]), 1)
            r32 = K.box_refine_ref(c["ref"], c["dc"], sp, c["ds"], c["rng_rows"], 1)
            s_size, s_metric = K.box_size_scale(sp, c["ds"], c["rng_rows"])
            note("box_refine size", K.reference_passes(r64[1], r32[1], s_size))
            note("box_refine size_metric", K.reference_passes(r64[2], r32[2], s_metric))
            size32 = r64[1].float()
            note("box_refine_backward chained", K.reference_passes(K.box_refine_bwd_ref(d64(c["g_center"]), d64(c["g_metric"]), r64[1], d64(c["rng_rows"]), 1)[1],
                                                                   K.box_refine_bwd_ref(c["g_center"], c["g_metric"], r32[1], c["rng_rows"], 1)[1],
                                                                   K.box_refine_chain_scale(c["g_metric"], sp, c["ds"], c["rng_rows"])))
            note("box_refine_backward", K.reference_passes(K.box_refine_bwd_ref(d64(c["g_center"]), d64(c["g_metric"]), r64[1], d64(c["rng_rows"]), 1)[1],
                                                           K.box_refine_bwd_ref(c["g_center"], c["g_metric"], size32, c["rng_rows"], 1)[1],
                                                           K.box_refine_bwd_scale(c["g_metric"], r64[1], c["rng_rows"])))
    for k, v in worst.items():
        print(f"[decoder-reference-e32] {k}: {v:.3e}")


# ---- the wrappers refuse wrong shapes before they touch a device ----------------------------------------------------------------------------
def test_wrappers_refuse_wrong_shapes():
    from segdino3d_amd import ops, train_dec
    Q = 5
    ok3, okq = torch.zeros(3), torch.zeros(Q, 3)
    rng, rngs, rs = torch.zeros(6), torch.zeros(2, 6), torch.zeros(Q, dtype=torch.int32)
    dim_t, axis = K.pe_tables(6)
    bad_boxes = [
        dict(size_prev=torch.zeros(1, 3)), dict(size_prev=torch.zeros(Q - 1, 3)), dict(size_prev=torch.zeros(Q, 4)), dict(size_prev=torch.zeros(4)),
        dict(d_center=torch.zeros(Q - 1, 3)), dict(d_center=torch.zeros(Q * 3)), dict(d_size=torch.zeros(Q + 1, 3)), dict(d_size=torch.zeros(Q, 2)),
        dict(ref_points=torch.zeros(Q, 6)), dict(rng=rngs), dict(rng=torch.zeros(3)), dict(rng=rng, row_scene=rs), dict(rng=torch.zeros(2, 3), row_scene=rs),
        dict(rng=rngs, row_scene=rs[:-1]), dict(rng=rngs, row_scene=torch.zeros(Q, 1, dtype=torch.int32)),
    ]
    for bad in bad_boxes:
        kw = dict(ref_points=okq, d_center=okq, size_prev=ok3, d_size=okq, rng=rng, normalize=True)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.box_refine(**kw)
        if "row_scene" not in kw:
            with pytest.raises(ValueError):
                train_dec.box_refine(**kw)
    xyz = torch.zeros(Q, 3)
    bad_pe = [dict(rng=rngs), dict(rng=torch.zeros(5)), dict(rng=rng, row_scene=rs), dict(rng=rngs, row_scene=rs[:-1]), dict(rng=torch.zeros(6, 2), row_scene=rs),
              dict(mod_num=torch.zeros(Q, 2), mod_den=ok3), dict(mod_num=torch.zeros(Q - 1, 3), mod_den=ok3), dict(mod_num=okq, mod_den=torch.zeros(1, 3)),
              dict(mod_num=okq, mod_den=torch.zeros(Q - 1, 3)), dict(mod_num=okq, mod_den=torch.zeros(4)), dict(mod_num=okq)]
    for bad in bad_pe:
        kw = dict(rng=rng)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.sine_pe(xyz, kw.pop("rng"), dim_t, axis, **kw)
        if "mod_num" not in bad:
            with pytest.raises(ValueError):
                ops.fourier_pe(xyz, bad["rng"], torch.zeros(3, 3), 6, row_scene=bad.get("row_scene"))
    for num, den in ((torch.zeros(Q, 2), ok3), (okq, torch.zeros(1, 3)), (okq, None), (None, ok3), (okq, torch.zeros(Q + 1, 3))):
        with pytest.raises(ValueError):
            train_dec.sine_pe_modulated(xyz, rng, dim_t, axis, num, den)
    with pytest.raises(ValueError):
        train_dec.sine_pe_modulated(xyz, rngs, dim_t, axis, okq, ok3)
    # right shapes pass the shape checks: what stops a CPU tensor is the device check behind them
    for call in (lambda: ops.box_refine(okq, okq, ok3, okq, rng, True), lambda: ops.box_refine(okq, okq, okq, okq, rngs, True, row_scene=rs),
                 lambda: ops.sine_pe(xyz, rng, dim_t, axis, mod_num=okq, mod_den=okq), lambda: ops.fourier_pe(xyz, rngs, torch.zeros(3, 3), 6, row_scene=rs)):
        with pytest.raises(RuntimeError):
            call()
