"""The decoder's small kernels in `segdino3d_amd/csrc/dense.hip` and `csrc/train_dec.hip` - sd3d_layernorm, sd3d_layernorm_backward,
sd3d_act_backward, sd3d_col_sums, sd3d_sine_pe, sd3d_fourier_pe, sd3d_sine_pe_mod_backward, sd3d_box_refine (each with and without row_scene),
sd3d_box_refine_backward, sd3d_transpose_batch, sd3d_linear_layernorm - called directly through ctypes (so that every leading dimension
can differ from its width), each against the float64 reference of the same operation in tests/decoder_kernel_cases.py, at the sizes the
launch geometry cares about: one wave per row and 4 x 64 lanes x float4 in LayerNorm, 256 threads over the elements of the elementwise
kernels, 16 row lanes / 64-row chunks and the switch at 8192 rows in the column sums, 32 x 32 tiles and 112 jobs per launch in the
transpose.

Exact outputs (masks, copies, single fp32 operations, the transpose, zeroed padding) are compared bit for bit.  Float outputs:
`check_float`, whose bound comes from the fp32 evaluation of the reference on the CPU; column sums: the derived bound of
`col_sum_bound`.  Every output buffer carries 64 sentinel elements behind its end and its padded columns are pre-filled - both must come
back untouched; padded input columns hold NaN, so a read behind a row shows.  Every case prints a `[decoder-kernel-error]` line;
profiles/decoder_kernel_errors.md holds the table."""
import numpy as np
import pytest
import torch

from tests import decoder_kernel_cases as K
from tests.decoder_kernel_cases import check_bound, check_float
from tests.helpers import Out, wide

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_WS = -1, -2
ACT = {None: 0, "relu": 1, "gelu": 2, "sigmoid": 3}


def _dev():
    return torch.device("cuda:0")


def _lib():
    from segdino3d_amd import _lib as L
    return L, L.load()


def _stream():
    from segdino3d_amd import ops
    return ops._stream()


def up(t):
    return None if t is None else t.contiguous().to(_dev())


def ptr(t):
    return None if t is None else t.data_ptr()


def d64(t):
    return None if t is None else t.double()


def rows_of(out, n_rows, ld, width):
    """[n_rows, width] of an Out of n_rows x ld elements whose columns width.. must still hold the fill."""
    full = out.get(n_rows, ld)
    assert bool((full[:, width:] == out.fill).all()), "columns behind the row's width were written"
    return full[:, :width].contiguous()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- sd3d_layernorm -----------------------------------------------------------------------------------------------------------------------
def device_layernorm(c, with_res, relu, D=None, pad_x=4, pad_res=8, pad_out=12, M=None):
    L, lib = _lib()
    M, D = c["M"] if M is None else M, D or c["D"]
    x, ld_x = wide(c["x"], pad_x)
    res, ld_res = wide(c["res"], pad_res) if with_res else (None, 0)
    w, b = up(c["w"]), up(c["b"])
    ld_out = c["D"] + pad_out
    out = Out(max(c["M"], 1) * ld_out)
    rc = lib.sd3d_layernorm(x.data_ptr(), ld_x, ptr(res), ld_res, w.data_ptr(), b.data_ptr(), K.EPS, M, D, out.ptr, ld_out, int(relu), _stream())
    torch.cuda.synchronize()
    return rc, out, ld_out


@pytest.mark.parametrize("D", K.LN_D)
def test_layernorm(D):
    L, lib = _lib()
    for M in K.LN_M:
        c = K.ln_case(M, D)
        for with_res in (False, True):
            res = c["res"] if with_res else None
            scale = K.layernorm_scale(c["x"], res, c["w"], c["b"])
            for relu in (False, True):
                rc, out, ld_out = device_layernorm(c, with_res, relu)
                L.check(rc, "layernorm")
                got = rows_of(out, M, ld_out, D)
                r64 = K.layernorm_ref(d64(c["x"]), d64(res), d64(c["w"]), d64(c["b"]), relu=relu)
                r32 = K.layernorm_ref(c["x"], res, c["w"], c["b"], relu=relu)
                check_float("layernorm", f"M{M} D{D} res={int(with_res)} relu={int(relu)}", got, r64, r32, scale)
                if c["const"] is not None:                      # the constant row: variance 0, the output is b (ReLU: max(b, 0))
                    assert torch.equal(got[c["const"]], torch.relu(c["b"]) if relu else c["b"])
                if relu:
                    assert float(got.min()) >= 0.0


def test_layernorm_refusals_and_no_rows():
    c = K.ln_case(5, 256)
    for kw in (dict(D=6), dict(D=1028), dict(pad_x=2)):          # D no multiple of 4, D > 1024, ld_x = D + 2
        rc, out, _ = device_layernorm(c, True, False, **kw)
        assert rc == ERR_ARG and out.untouched(), kw
    rc, out, _ = device_layernorm(c, True, True, M=0)           # no rows: nothing happens
    assert rc == 0 and out.untouched()


# ---- sd3d_layernorm_backward ----------------------------------------------------------------------------------------------------------------
def device_layernorm_backward(c, y, with_res, pads=(4, 8, 12, 16, 20), ws_short=0):
    """-> (rc, dxin Out, ld_dx, dw Out, db Out, ws Out); y None: no fused ReLU."""
    L, lib = _lib()
    M, D = c["M"], c["D"]
    dy, ld_dy = wide(c["dy"], pads[0])
    yy, ld_y = wide(y, pads[1]) if y is not None else (None, 0)
    x, ld_x = wide(c["x"], pads[2])
    res, ld_res = wide(c["res"], pads[3]) if with_res else (None, 0)
    w = up(c["w"])
    ld_dx = D + pads[4]
    dxin, dw, db = Out(M * ld_dx), Out(D), Out(D)
    ws_bytes = lib.sd3d_layernorm_backward_ws_bytes(M, D)
    ws = Out(ws_bytes, torch.uint8)
    rc = lib.sd3d_layernorm_backward(dy.data_ptr(), ld_dy, ptr(yy), ld_y, x.data_ptr(), ld_x, ptr(res), ld_res, w.data_ptr(), K.EPS, M, D,
                                     0 if y is None else 1, dxin.ptr, ld_dx, dw.ptr, db.ptr, ws.ptr, ws_bytes - ws_short, _stream())
    torch.cuda.synchronize()
    return rc, dxin, ld_dx, dw, db, ws


def check_layernorm_backward(c, relu, with_res, twice=False):
    L, lib = _lib()
    M, D = c["M"], c["D"]
    res = c["res"] if with_res else None
    y = None
    if relu:                                                    # the mask is an input: any forward output will do, with the planted zeros
        y, spots = K.plant_relu_mask(torch.relu(K.layernorm_ref(c["x"], res, c["w"], c["b"])))
    rc, dxin, ld_dx, dw, db, ws = device_layernorm_backward(c, y, with_res)
    L.check(rc, "layernorm_backward")
    ws.get(ws.n)                                                # the workspace was not overrun
    got = rows_of(dxin, M, ld_dx, D)
    r64 = K.layernorm_bwd_ref(d64(c["dy"]), d64(y), d64(c["x"]), d64(res), d64(c["w"]))
    r32 = K.layernorm_bwd_ref(c["dy"], y, c["x"], res, c["w"])
    name = f"M{M} D{D} res={int(with_res)} relu={int(relu)}"
    check_float("layernorm_backward dxin", name, got, r64[0], r32[0], K.layernorm_bwd_scale(c["dy"], y, c["x"], res, c["w"]))
    bw, bb = K.layernorm_sums_bound(c["dy"], y, c["x"], res, c["w"])
    check_bound("layernorm_backward dw", name, dw.get(D), r64[1], bw)
    check_bound("layernorm_backward db", name, db.get(D), r64[2], bb)
    if twice:
        rc, dxin2, _, dw2, db2, _ = device_layernorm_backward(c, y, with_res)
        L.check(rc, "layernorm_backward")
        for a, b in ((dxin, dxin2), (dw, dw2), (db, db2)):
            assert same_bits(a.buf, b.buf), "second call differs"


@pytest.mark.parametrize("D", K.LN_D)
def test_layernorm_backward(D):
    for M in K.LN_M:
        c = K.ln_case(M, D, planted=False)
        for with_res in (False, True):
            for relu in (False, True):
                check_layernorm_backward(c, relu, with_res, twice=relu and with_res)


@pytest.mark.parametrize("M", K.LN_M_SUMS)
def test_layernorm_backward_many_rows(M):
    """D = 8 around 8192 rows, where the column sums behind dw / db change from one launch to partial sums per 64-row chunk."""
    c = K.ln_case(M, 8, planted=False)
    check_layernorm_backward(c, True, True, twice=True)
    check_layernorm_backward(c, False, False)


def test_layernorm_backward_refusals():
    c = K.ln_case(5, 256, planted=False)
    y = torch.relu(c["res"])
    rc, dxin, _, dw, db, ws = device_layernorm_backward(c, y, True, ws_short=1)      # workspace one byte short
    assert rc == ERR_WS and dxin.untouched() and dw.untouched() and db.untouched() and ws.untouched()
    rc, dxin, _, dw, db, ws = device_layernorm_backward(c, y, True, pads=(4, 8, 2, 16, 20))       # ld_x = D + 2
    assert rc == ERR_ARG and dxin.untouched() and dw.untouched() and db.untouched() and ws.untouched()


# ---- sd3d_act_backward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", K.ACTS, ids=[str(a) for a in K.ACTS])
def test_act_backward(act):
    L, lib = _lib()
    for M, C, C_pad in K.ACT_SHAPES:
        c = K.act_case(act, M, C)
        dy, ld_dy = wide(c["dy"], 3)
        ref, ld_ref = wide(c["ref"], 7)
        ld_g = C_pad + 5
        g = Out(M * ld_g)
        rc = lib.sd3d_act_backward(dy.data_ptr(), ld_dy, None if act is None else ref.data_ptr(), ld_ref, ACT[act], M, C, C_pad, g.ptr, ld_g, _stream())
        torch.cuda.synchronize()
        L.check(rc, "act_backward")
        got = rows_of(g, M, ld_g, C_pad)                        # everything behind C_pad: untouched
        assert same_bits(got[:, C:], torch.zeros(M, C_pad - C)), "columns [C, C_pad) must be +0"
        got = got[:, :C]
        assert bool(torch.isfinite(got).all())
        r64 = K.act_backward_ref(d64(c["dy"]), d64(c["ref"]), act)
        r32 = K.act_backward_ref(c["dy"], c["ref"], act)
        if act in (None, "relu"):                               # a copy / a mask: exact (+0, -0 and the smallest denormal included)
            assert torch.equal(got, r32), (act, M, C)
            print(f"[decoder-kernel-error] act_backward {act} | M{M} C{C} C_pad{C_pad} | exact")
        else:
            check_float(f"act_backward {act}", f"M{M} C{C} C_pad{C_pad}", got, r64, r32, K.act_backward_scale(c["dy"], c["ref"], act))
    g = Out(64)
    rc = lib.sd3d_act_backward(dy.data_ptr(), ld_dy, ref.data_ptr(), ld_ref, ACT[act], 2, 8, 4, g.ptr, 8, _stream())       # C_pad < C
    assert rc == ERR_ARG and g.untouched()


# ---- sd3d_col_sums --------------------------------------------------------------------------------------------------------------------------
def device_col_sums(x, pad, M=None, ws_short=0):
    L, lib = _lib()
    Mx, C = x.shape
    M = Mx if M is None else M
    xd, ld = wide(x, pad)
    out = Out(C)
    ws_bytes = lib.sd3d_col_sums_ws_bytes(max(M, 1), C)
    ws = Out(ws_bytes, torch.uint8)
    rc = lib.sd3d_col_sums(xd.data_ptr(), ld, M, C, out.ptr, ws.ptr, ws_bytes - ws_short, _stream())
    torch.cuda.synchronize()
    return rc, out, ws


@pytest.mark.parametrize("C", K.CSUM_C)
def test_col_sums(C):
    L, lib = _lib()
    for M in K.CSUM_M:
        x = K.csum_case(M, C)
        rc, out, ws = device_col_sums(x, 3)
        L.check(rc, "col_sums")
        ws.get(ws.n)
        check_bound("col_sums", f"M{M} C{C}", out.get(C), x.double().sum(0), K.col_sum_bound(x))
        rc, out2, _ = device_col_sums(x, 3)
        assert rc == 0 and same_bits(out.buf, out2.buf), "second call differs"
    rc, out, ws = device_col_sums(x, 3, M=0)                    # no rows: refused
    assert rc == ERR_ARG and out.untouched()
    rc, out, ws = device_col_sums(x, 3, ws_short=1)
    assert rc == ERR_WS and out.untouched() and ws.untouched()


# ---- sd3d_sine_pe (one range / row_scene) ---------------------------------------------------------------------------------------------------------
def device_sine_pe(p, rows, dim_t, axis, rng, row_scene, mod):
    """Rows `rows` (bool mask) of case p; rng [6] with row_scene None, else [n_scenes, 6].  mod: None | 'den1' | 'den2'."""
    L, lib = _lib()
    pts = up(p["pts"][rows])                                    # xyz = columns 0-2 of [n, 6]: ld 6
    n, d = int(pts.shape[0]), int(dim_t.numel())
    ld_out = d + 3
    out = Out(n * ld_out)
    num, ld_num, den, ld_den = None, 0, None, 0
    if mod:
        num, ld_num = wide(p["mod_num"][rows], 2)
        den, ld_den = (up(p["den1"]), 0) if mod == "den1" else wide(p["den2"][rows], 1)
    dt, ax, rg = up(dim_t), up(axis), up(rng)
    rs = None if row_scene is None else up(row_scene[rows])
    rc = lib.sd3d_sine_pe(pts.data_ptr(), 6, n, rg.data_ptr(), ptr(rs), dt.data_ptr(), ax.data_ptr(), d, ptr(num), ld_num, ptr(den), ld_den, out.ptr, ld_out,
                          _stream())
    torch.cuda.synchronize()
    L.check(rc, "sine_pe")
    return rows_of(out, n, ld_out, d)


@pytest.mark.parametrize("d_pos", K.SINE_D)
def test_sine_pe(d_pos):
    dim_t, axis = K.pe_tables(d_pos)
    for n in K.PE_N:
        p = K.pe_case(n)
        every = torch.ones(n, dtype=torch.bool)
        for mod in (None, "den1", "den2"):
            num, den = (p["mod_num"], p[mod]) if mod else (None, None)
            got = device_sine_pe(p, every, dim_t, axis, K.SCENE_RANGES, p["row_scene"], mod)
            r64 = K.sine_pe_ref(d64(p["xyz"]), d64(p["rng_rows"]), dim_t, axis, d64(num), d64(den))
            r32 = K.sine_pe_ref(p["xyz"], p["rng_rows"], dim_t, axis, num, den)
            check_float("sine_pe_rows", f"n{n} d{d_pos} mod={mod}", got, r64, r32, K.sine_pe_scale(p["xyz"], p["rng_rows"], dim_t, axis, num, den))
            for s in (0, 2):                                    # one range (no row_scene) on that scene's rows: the same bits
                rows = p["row_scene"] == s
                if bool(rows.any()):
                    one = device_sine_pe(p, rows, dim_t, axis, K.SCENE_RANGES[s], None, mod)
                    assert same_bits(one, got[rows]), (n, d_pos, mod, s)
                    check_float("sine_pe", f"n{int(rows.sum())} d{d_pos} mod={mod} scene{s}", one, r64[rows], r32[rows],
                                K.sine_pe_scale(p["xyz"], p["rng_rows"], dim_t, axis, num, den)[rows])
            q = K.pe_case_one_scene(n)                          # ... and on all n rows
            one = device_sine_pe(q, every, dim_t, axis, K.SCENE_RANGES[q["scene"]], None, mod)
            check_float("sine_pe", f"n{n} d{d_pos} mod={mod} one scene", one, K.sine_pe_ref(d64(q["xyz"]), d64(q["rng_rows"]), dim_t, axis, d64(num), d64(den)),
                        K.sine_pe_ref(q["xyz"], q["rng_rows"], dim_t, axis, num, den), K.sine_pe_scale(q["xyz"], q["rng_rows"], dim_t, axis, num, den))


def test_sine_pe_refusals():
    L, lib = _lib()
    p = K.pe_case(17)
    dim_t, axis = K.pe_tables(6)
    pts, dt, ax, rg, num = up(p["pts"]), up(dim_t), up(axis), up(K.SCENE_RANGES), up(p["mod_num"])
    out = Out(17 * 6)
    rc = lib.sd3d_sine_pe(pts.data_ptr(), 6, 17, rg.data_ptr(), None, dt.data_ptr(), ax.data_ptr(), 6, num.data_ptr(), 3, None, 0, out.ptr, 6, _stream())
    assert rc == ERR_ARG and out.untouched()                   # numerator without denominator
    rc = lib.sd3d_sine_pe(pts.data_ptr(), 6, 0, rg.data_ptr(), None, dt.data_ptr(), ax.data_ptr(), 6, None, 0, None, 0, out.ptr, 6, _stream())
    assert rc == 0 and out.untouched()                         # no rows


# ---- sd3d_fourier_pe (one range / row_scene) -----------------------------------------------------------------------------------------------------
def device_fourier_pe(p, rows, gb, d_pos, rng, row_scene):
    L, lib = _lib()
    pts = up(p["pts"][rows])
    n = int(pts.shape[0])
    ld_out = d_pos + 3
    out = Out(n * ld_out)
    b, rg = up(gb), up(rng)
    rs = None if row_scene is None else up(row_scene[rows])
    rc = lib.sd3d_fourier_pe(pts.data_ptr(), 6, n, rg.data_ptr(), ptr(rs), b.data_ptr(), gb.shape[1], d_pos, out.ptr, ld_out, _stream())
    torch.cuda.synchronize()
    return rc, out, n, ld_out


@pytest.mark.parametrize("d_pos", K.FOURIER_D)
def test_fourier_pe(d_pos):
    L, lib = _lib()
    gb = K.gauss_b(d_pos)                                       # [3, d_pos / 2 + 5]: ld_b != d_pos / 2
    for n in K.PE_N:
        p = K.pe_case(n)
        rc, out, _, ld_out = device_fourier_pe(p, torch.ones(n, dtype=torch.bool), gb, d_pos, K.SCENE_RANGES, p["row_scene"])
        L.check(rc, "fourier_pe_rows")
        got = rows_of(out, n, ld_out, d_pos)
        r64 = K.fourier_pe_ref(d64(p["xyz"]), d64(p["rng_rows"]), gb, d_pos)
        r32 = K.fourier_pe_ref(p["xyz"], p["rng_rows"], gb, d_pos)
        scale = K.fourier_pe_scale(p["xyz"], p["rng_rows"], gb, d_pos)
        check_float("fourier_pe_rows", f"n{n} d{d_pos}", got, r64, r32, scale)
        for s in (0, 2):
            rows = p["row_scene"] == s
            if bool(rows.any()):
                rc, out, m, _ = device_fourier_pe(p, rows, gb, d_pos, K.SCENE_RANGES[s], None)
                L.check(rc, "fourier_pe")
                one = rows_of(out, m, ld_out, d_pos)
                assert same_bits(one, got[rows]), (n, d_pos, s)
                check_float("fourier_pe", f"n{m} d{d_pos} scene{s}", one, r64[rows], r32[rows], scale[rows])
        q = K.pe_case_one_scene(n)                              # ... and on all n rows
        rc, out, _, _ = device_fourier_pe(q, torch.ones(n, dtype=torch.bool), gb, d_pos, K.SCENE_RANGES[q["scene"]], None)
        L.check(rc, "fourier_pe")
        check_float("fourier_pe", f"n{n} d{d_pos} one scene", rows_of(out, n, ld_out, d_pos), K.fourier_pe_ref(d64(q["xyz"]), d64(q["rng_rows"]), gb, d_pos),
                    K.fourier_pe_ref(q["xyz"], q["rng_rows"], gb, d_pos), K.fourier_pe_scale(q["xyz"], q["rng_rows"], gb, d_pos))
    for odd in (d_pos + 1, 1):                                  # odd d_pos: refused, with and without row_scene
        rc, out, _, _ = device_fourier_pe(p, torch.ones(n, dtype=torch.bool), K.gauss_b(d_pos + 2), odd, K.SCENE_RANGES, p["row_scene"])
        assert rc == ERR_ARG and out.untouched()
        rc, out, _, _ = device_fourier_pe(p, torch.ones(n, dtype=torch.bool), K.gauss_b(d_pos + 2), odd, K.SCENE_RANGES[0], None)
        assert rc == ERR_ARG and out.untouched()


# ---- sd3d_sine_pe_mod_backward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d_pos", K.SINE_D)
def test_sine_pe_mod_backward(d_pos):
    L, lib = _lib()
    dim_t, axis = K.pe_tables(d_pos)
    dt, ax = up(dim_t), up(axis)
    for n in (1, 3, 5, 200):                                    # one wave per row, 4 rows per workgroup
        p = K.pe_case_one_scene(n)
        s, rows, m = p["scene"], torch.ones(n, dtype=torch.bool), n
        xyz, rng_rows = p["xyz"], p["rng_rows"]
        d_out = torch.randn(m, d_pos, generator=K.gen(71, n, d_pos))
        pts, rg = up(p["pts"][rows]), up(K.SCENE_RANGES[s])
        do, ld_do = wide(d_out, 5)
        for ld_den in (0, 3):
            den = p["den1"] if ld_den == 0 else p["den2"][rows]
            dd = up(den)
            d_num = Out(m * 3)
            rc = lib.sd3d_sine_pe_mod_backward(do.data_ptr(), ld_do, pts.data_ptr(), 6, m, rg.data_ptr(), dt.data_ptr(), ax.data_ptr(), d_pos, dd.data_ptr(),
                                               ld_den, d_num.ptr, _stream())
            torch.cuda.synchronize()
            L.check(rc, "sine_pe_mod_backward")
            r64 = K.sine_pe_mod_bwd_ref(d64(d_out), d64(xyz), d64(rng_rows), dim_t, axis, d64(den))
            r32 = K.sine_pe_mod_bwd_ref(d_out, xyz, rng_rows, dim_t, axis, den)
            check_float("sine_pe_mod_backward", f"n{m} d{d_pos} ld_den={ld_den}", d_num.get(m, 3), r64, r32,
                        K.sine_pe_mod_bwd_scale(d_out, xyz, rng_rows, dim_t, axis, den))
    d_num = Out(m * 3)
    rc = lib.sd3d_sine_pe_mod_backward(do.data_ptr(), ld_do, pts.data_ptr(), 6, m, rg.data_ptr(), dt.data_ptr(), ax.data_ptr(), d_pos, None, 0, d_num.ptr, _stream())
    assert rc == ERR_ARG and d_num.untouched()                 # no denominator


# ---- sd3d_box_refine (one range / row_scene) / sd3d_box_refine_backward ----------------------------------------------------------------------------
def device_box_refine(c, rows, sp, normalize, with_size, rng, row_scene):
    """sp: 'sp1' ([3], stride 0) or 'sp2' ([Q, 3], passed with leading dimension 5 and NaN behind every row)."""
    L, lib = _lib()
    Q = int(rows.sum())
    ref, dc, ds = up(c["ref"][rows]), up(c["dc"][rows]), up(c["ds"][rows])
    prev, ld_prev = (up(c["sp1"]), 0) if sp == "sp1" else wide(c["sp2"][rows], 2)
    center, size, metric = Out(Q * 3), Out(Q * 3), Out(Q * 3)
    rg = up(rng)
    rs = None if row_scene is None else up(row_scene[rows])
    rc = lib.sd3d_box_refine(ref.data_ptr(), dc.data_ptr(), prev.data_ptr(), ld_prev, ds.data_ptr() if with_size else None, rg.data_ptr(), ptr(rs),
                             normalize, Q, center.ptr, size.ptr, metric.ptr, _stream())
    torch.cuda.synchronize()
    L.check(rc, "box_refine")
    return center, size, metric


def check_box_outputs(name, c, rows, sp, normalize, outs):
    center, size, metric = outs
    Q = int(rows.sum())
    prev = c[sp] if sp == "sp1" else c[sp][rows]
    args = (c["ref"][rows], c["dc"][rows], prev, c["ds"][rows], c["rng_rows"][rows])
    r64 = K.box_refine_ref(*(d64(a) for a in args), normalize)
    r32 = K.box_refine_ref(*args, normalize)
    assert torch.equal(center.get(Q, 3), r32[0])                # one fp32 addition: the same bits as torch's
    got_size, got_metric = size.get(Q, 3), metric.get(Q, 3)
    assert bool(torch.isfinite(got_size).all()) and bool(torch.isfinite(got_metric).all())
    if not normalize:
        assert torch.equal(got_size, r32[1]) and torch.equal(got_metric, r32[1])
        return
    s_size, s_metric = K.box_size_scale(prev, c["ds"][rows], c["rng_rows"][rows])
    check_float("box_refine size", name, got_size, r64[1], r32[1], s_size)
    check_float("box_refine size_metric", name, got_metric, r64[2], r32[2], s_metric)
    for v in (0.0, 1.0):                                        # saturated where float64 saturates
        assert bool((got_size[r64[1] == v] == v).all())
    assert float(got_size.min()) >= 0.0 and float(got_size.max()) <= 1.0


@pytest.mark.parametrize("Q", K.BOX_Q)
def test_box_refine(Q):
    c = K.box_case(Q)
    every = torch.ones(Q, dtype=torch.bool)
    for normalize in (0, 1):
        for sp in ("sp1", "sp2"):
            name = f"Q{Q} normalize={normalize} size_prev={'[3]' if sp == 'sp1' else '[Q, 3]'}"
            outs = device_box_refine(c, every, sp, normalize, True, K.SCENE_RANGES, c["row_scene"])
            check_box_outputs(name + " rows", c, every, sp, normalize, outs)
            for s in (0, 2):                                    # one range (no row_scene) on that scene's rows: the same bits
                rows = c["row_scene"] == s
                if bool(rows.any()):
                    one = device_box_refine(c, rows, sp, normalize, True, K.SCENE_RANGES[s], None)
                    check_box_outputs(name + f" scene{s}", c, rows, sp, normalize, one)
                    for a, b in zip(one, outs):
                        assert same_bits(a.get(int(rows.sum()), 3), b.get(Q, 3)[rows])
            one = K.box_case_one_scene(Q)                      # ... and on all Q rows
            check_box_outputs(name + " one scene", one, every, sp, normalize, device_box_refine(one, every, sp, normalize, True, K.SCENE_RANGES[one["scene"]], None))
        for row_scene in (None, c["row_scene"]):                # no size head: the centre alone, the size outputs untouched
            rows = every if row_scene is not None else c["row_scene"] == int(c["row_scene"][0])
            rng = K.SCENE_RANGES if row_scene is not None else K.SCENE_RANGES[int(c["row_scene"][0])]
            center, size, metric = device_box_refine(c, rows, "sp2", normalize, False, rng, row_scene)
            assert torch.equal(center.get(int(rows.sum()), 3), (c["ref"] + c["dc"])[rows]) and size.untouched() and metric.untouched()


@pytest.mark.parametrize("Q", K.BOX_Q)
def test_box_refine_backward(Q):
    L, lib = _lib()
    c = K.box_case_one_scene(Q)                                 # the backward is one scene's
    s, rows, m = c["scene"], torch.ones(Q, dtype=torch.bool), Q
    rng_rows, rg = c["rng_rows"], up(K.SCENE_RANGES[s])
    gc, gm = c["g_center"][rows], c["g_metric"][rows]
    gcd, gmd = up(gc), up(gm)
    for normalize in (0, 1):
        size64 = K.box_refine_ref(d64(c["ref"][rows]), d64(c["dc"][rows]), d64(c["sp2"][rows]), d64(c["ds"][rows]), d64(rng_rows), normalize)[1]
        size32 = size64.float()                                 # the forward's size output, an input here
        szd = up(size32)
        for has_c, has_m, has_size in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
            d_dc, d_ds = Out(m * 3), Out(m * 3)
            rc = lib.sd3d_box_refine_backward(gcd.data_ptr() if has_c else None, gmd.data_ptr() if has_m else None, szd.data_ptr(), rg.data_ptr(), normalize, m,
                                              d_dc.ptr, d_ds.ptr if has_size else None, _stream())
            torch.cuda.synchronize()
            L.check(rc, "box_refine_backward")
            name = f"Q{m} normalize={normalize} d_center={has_c} d_metric={has_m} size={has_size}"
            r64 = K.box_refine_bwd_ref(d64(gc) if has_c else None, d64(gm) if has_m else None, size64, d64(rng_rows), normalize, bool(has_size))
            r32 = K.box_refine_bwd_ref(gc if has_c else None, gm if has_m else None, size32, rng_rows, normalize, bool(has_size))
            assert torch.equal(d_dc.get(m, 3), r32[0])          # a copy (zeros without a gradient)
            if not has_size:
                assert d_ds.untouched()
            elif not normalize or not has_m:
                assert torch.equal(d_ds.get(m, 3), r32[1])
            else:
                check_float("box_refine_backward d_ds", name, d_ds.get(m, 3), r64[1], r32[1], K.box_refine_bwd_scale(gm, size64, rng_rows))
    d_dc, d_ds = Out(m * 3), Out(m * 3)
    rc = lib.sd3d_box_refine_backward(None, gmd.data_ptr(), None, rg.data_ptr(), 1, m, d_dc.ptr, d_ds.ptr, _stream())          # normalised without the sizes
    assert rc == ERR_ARG and d_dc.untouched() and d_ds.untouched()


@pytest.mark.parametrize("normalize", [False, True])
def test_box_refine_autograd_ignores_the_size_output(normalize):
    """train_dec.box_refine: gradients reach d_center / d_size through center and size_metric; `size` feeds the next layer detached, a
    loss on it adds nothing."""
    from segdino3d_amd import train_dec
    c = K.box_case_one_scene(86)
    s, rows, m = c["scene"], torch.ones(86, dtype=torch.bool), 86
    rng_rows = c["rng_rows"]
    gc, gm = c["g_center"][rows], c["g_metric"][rows]
    for sp in (c["sp1"], c["sp2"][rows]):
        dc, ds = up(c["dc"][rows]).requires_grad_(True), up(c["ds"][rows]).requires_grad_(True)
        center, size, metric = train_dec.box_refine(up(c["ref"][rows]), dc, up(sp), ds, up(K.SCENE_RANGES[s]), normalize)
        assert not size.requires_grad
        ((center * up(gc)).sum() + (metric * up(gm)).sum() + (size * 1e3).sum()).backward()
        size64 = K.box_refine_ref(d64(c["ref"][rows]), d64(c["dc"][rows]), d64(sp), d64(c["ds"][rows]), d64(rng_rows), normalize)[1]
        r64 = K.box_refine_bwd_ref(d64(gc), d64(gm), size64, d64(rng_rows), normalize)
        size32 = K.box_refine_ref(c["ref"][rows], c["dc"][rows], sp, c["ds"][rows], rng_rows, normalize)[1]       # fp32 forward AND backward
        r32 = K.box_refine_bwd_ref(gc, gm, size32, rng_rows, normalize)
        assert torch.equal(dc.grad.cpu(), gc)
        name = f"Q{m} normalize={int(normalize)} size_prev={list(sp.shape)} autograd"
        if normalize:
            check_float("box_refine_backward d_ds", name, ds.grad.cpu(), r64[1], r32[1], K.box_refine_chain_scale(gm, sp, c["ds"][rows], rng_rows))
        else:
            assert torch.equal(ds.grad.cpu(), gm)
        dc2 = up(c["dc"][rows]).requires_grad_(True)           # no size head
        center, size, metric = train_dec.box_refine(up(c["ref"][rows]), dc2, up(sp), None, up(K.SCENE_RANGES[s]), normalize)
        assert size is None and metric is None
        (center * up(gc)).sum().backward()
        assert torch.equal(dc2.grad.cpu(), gc)


def test_wrappers_refuse_wrong_shapes_on_the_device():
    """The refusals of tests/test_decoder_kernel_cases.py with device tensors, where the kernels would read behind the tensors' ends."""
    from segdino3d_amd import ops, train_dec
    d = _dev()
    Q = 86
    okq, ok3 = torch.rand(Q, 3, device=d), torch.rand(3, device=d)
    rng, rngs, rs = torch.tensor([0.0, 0, 0, 1, 1, 1], device=d), torch.tensor([[0.0, 0, 0, 1, 1, 1]] * 2, device=d), torch.zeros(Q, dtype=torch.int32, device=d)
    dim_t, axis = (t.to(d) for t in K.pe_tables(6))
    for kw in (dict(size_prev=torch.rand(1, 3, device=d)), dict(d_size=torch.rand(Q - 1, 3, device=d)), dict(d_center=torch.rand(Q - 1, 3, device=d)),
               dict(rng=rngs), dict(rng=rng, row_scene=rs), dict(rng=rngs, row_scene=rs[:-1])):
        args = dict(ref_points=okq, d_center=okq, size_prev=ok3, d_size=okq, rng=rng, normalize=True)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.box_refine(**args)
    with pytest.raises(ValueError):
        train_dec.box_refine(okq, okq.clone().requires_grad_(True), torch.rand(1, 3, device=d), okq, rng, True)
    for kw in (dict(rng=rngs), dict(rng=rng, row_scene=rs), dict(rng=rngs, row_scene=rs[:-1]), dict(rng=rng, mod_num=okq[:-1], mod_den=ok3),
               dict(rng=rng, mod_num=okq, mod_den=torch.rand(1, 3, device=d)), dict(rng=rng, mod_num=okq)):
        kw = dict(kw)
        with pytest.raises(ValueError):
            ops.sine_pe(okq, kw.pop("rng"), dim_t, axis, **kw)
    with pytest.raises(ValueError):
        ops.fourier_pe(okq, rngs, torch.rand(3, 3, device=d), 6)
    with pytest.raises(ValueError):
        train_dec.sine_pe_modulated(okq, rng, dim_t, axis, okq.clone().requires_grad_(True), torch.rand(1, 3, device=d))
    # and the right shapes run: [3] and [Q, 3] previous sizes give the same rows when the [Q, 3] repeats the [3]
    a = ops.box_refine(okq, okq, ok3, okq, rng, True)
    b = ops.box_refine(okq, okq, ok3.expand(Q, 3).contiguous(), okq, rngs, True, row_scene=rs)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(ops.sine_pe(okq, rng, dim_t, axis, mod_num=okq, mod_den=ok3), ops.sine_pe(okq, rngs, dim_t, axis, mod_num=okq, mod_den=ok3.expand(Q, 3).contiguous(), row_scene=rs))


# ---- sd3d_transpose_batch -------------------------------------------------------------------------------------------------------------------
def device_transpose(jobs, seed=0):
    """jobs: [(rows, cols, ld_dst, batch)] -> (rc, [(src CPU, dst Out)])."""
    from segdino3d_amd import train_dec
    L, lib = _lib()
    arr = np.zeros(len(jobs), dtype=train_dec._TJOB_DT)
    keep = []
    for i, (rows, cols, ld, batch) in enumerate(jobs):
        src = K.transpose_src(rows, cols, batch, seed + i)
        sd, dst = up(src), Out(batch * cols * ld)
        arr[i] = (sd.data_ptr(), dst.ptr, rows, cols, ld, batch if i % 2 or batch > 1 else 0)       # batch 0 and 1 both mean one matrix
        keep.append((src, sd, dst))
    rc = lib.sd3d_transpose_batch(len(jobs), arr.ctypes.data, _stream())
    torch.cuda.synchronize()
    return rc, keep


@pytest.mark.parametrize("job", K.TRANSPOSE_JOBS, ids=lambda j: "-".join(map(str, j)))
def test_transpose_batch_one_job(job):
    L, lib = _lib()
    rows, cols, ld, batch = job
    rc, keep = device_transpose([job])
    L.check(rc, "transpose_batch")
    src, _, dst = keep[0]
    assert torch.equal(dst.get(batch, cols, ld), K.transpose_ref(src, ld))        # columns rows.. of the destination: zero


@pytest.mark.parametrize("n", [113, 225])
def test_transpose_batch_many_jobs(n):
    """More jobs than one launch takes (112): every destination exact, whichever launch made it."""
    L, lib = _lib()
    jobs = K.small_jobs(n)
    rc, keep = device_transpose(jobs, seed=n)
    L.check(rc, "transpose_batch")
    for (rows, cols, ld, batch), (src, _, dst) in zip(jobs, keep):
        assert torch.equal(dst.get(batch, cols, ld), K.transpose_ref(src, ld)), (rows, cols, ld, batch)


def test_transpose_batch_refusals():
    from segdino3d_amd import train_dec
    L, lib = _lib()
    src, dst = up(K.transpose_src(33, 5, 1, 0)), Out(5 * 32)
    arr = np.zeros(1, dtype=train_dec._TJOB_DT)
    arr[0] = (src.data_ptr(), dst.ptr, 33, 5, 32, 1)            # ld_dst < rows
    assert lib.sd3d_transpose_batch(1, arr.ctypes.data, _stream()) == ERR_ARG and dst.untouched()
    assert lib.sd3d_transpose_batch(0, arr.ctypes.data, _stream()) == 0 and dst.untouched()


# ---- sd3d_linear_layernorm: the shapes tests/test_gpu_decoder.py::test_fused_projection_residual_layernorm leaves out --------------------------------
@pytest.mark.parametrize("M,Cin,with_res,act", [(15, 16, True, None), (17, 512, True, "relu"), (17, 16, False, None), (15, 512, True, None)])
def test_linear_layernorm_gaps(M, Cin, with_res, act):
    """Rows on both sides of the 16-row workgroup, the shortest contraction and the longest the wrapper sends here, a residual whose
    leading dimension is not 256; the bound of the existing test (2e-6 of the row scale, x 4)."""
    L, lib = _lib()
    g = K.gen(83, M, Cin)
    x, w, b = torch.randn(M, Cin, generator=g), torch.randn(256, Cin, generator=g) * Cin ** -0.5, 0.1 * torch.randn(256, generator=g)
    res = torch.randn(M, 256, generator=g) if with_res else None
    gam, beta = 1 + 0.1 * torch.randn(256, generator=g), 0.1 * torch.randn(256, generator=g)
    xd, ld_x = wide(x, 4)
    rd, ld_res = wide(res, 5) if with_res else (None, 0)
    ld_out = 256 + 3
    out = Out(M * ld_out)
    wd, bd, gd, betad = up(w), up(b), up(gam), up(beta)
    rc = lib.sd3d_linear_layernorm(xd.data_ptr(), ld_x, M, Cin, wd.data_ptr(), 256, bd.data_ptr(), ptr(rd), ld_res, gd.data_ptr(), betad.data_ptr(),
                                   1e-5, ACT[act], out.ptr, ld_out, _stream())
    torch.cuda.synchronize()
    L.check(rc, "linear_layernorm")
    got = rows_of(out, M, ld_out, 256)
    pre = x.double() @ w.double().T + b.double() + (0 if res is None else res.double())
    ref = torch.nn.functional.layer_norm(pre, (256,), gam.double(), beta.double(), 1e-5)
    ref = torch.relu(ref) if act == "relu" else ref
    err = (got.double() - ref).abs().max().item()
    print(f"[decoder-kernel-error] linear_layernorm | M{M} Cin{Cin} res={int(with_res)} act={act} | abs {err:.3e} | bound {2e-6 * max(1.0, ref.abs().max().item()) * 4:.3e}")
    assert err <= 2e-6 * max(1.0, ref.abs().max().item()) * 4, err
