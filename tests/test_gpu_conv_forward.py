"""The forward convolution kernels - `ops.pair_conv` (csrc/pair_gemm.hip: weight-stationary, two-group, lock-step, chained and direct
pass 1, pass 2 over the row lists and over the position table), the dense pass-1 kernel behind a plain Linear on 16384 rows or more,
the output-stationary `ops.gather_gemm` with its split-bf16 twin and `ops.linear_group` - against the float64 reference of
tests/conv_forward_cases.py on planted tables.

Integer operands are compared bit for bit (every partial sum is an integer below 2^24: tests/test_conv_forward_cases.py), float
operands with `check_conv`.  Outputs that are column slices sit in buffers filled with a sentinel, and the buffer around the slice must
keep it; slices start at a multiple of 4 columns, since the kernels move 16 bytes at a time.  Every case prints a
`[conv-forward-error]` line; profiles/conv_forward_errors.md holds the table of one run."""
import numpy as np
import pytest
import torch

from tests import conv_forward_cases as C
from tests.conv_forward_cases import check_conv, record_exact

pytestmark = pytest.mark.gpu

SENT = -777.25
LEFT, RIGHT = 4, 8                  # columns around a slice: the row stride stays a multiple of 4 floats


def dev():
    return torch.device("cuda:0")


def up(t):
    return None if t is None else t.contiguous().to(dev())


def sliced(t, left=LEFT, right=RIGHT):
    """CPU [R, W] -> a device view of it inside a [R, left + W + right] tensor whose other columns hold NaN."""
    full = torch.full((t.shape[0], left + t.shape[1] + right), float("nan"))
    full[:, left:left + t.shape[1]] = t
    return full.to(dev())[:, left:left + t.shape[1]]


class Slice:
    """out= target: rows 1 .. M of columns LEFT .. LEFT + Cout of a sentinel-filled [M + 2, LEFT + Cout + right] buffer."""

    def __init__(self, M, Cout, right=RIGHT):
        self.buf = torch.full((M + 2, LEFT + Cout + right), SENT, device=dev())
        self.view = self.buf[1:M + 1, LEFT:LEFT + Cout]

    def get(self):
        """The slice on the CPU, after checking that every element around it still holds the sentinel, bit for bit."""
        rest = self.buf.clone()
        rest[1:-1, LEFT:LEFT + self.view.shape[1]] = SENT
        assert torch.equal(rest.view(torch.int32), torch.full_like(rest, SENT).view(torch.int32)), "written outside the output slice"
        return self.view.cpu()

    def untouched(self):
        return torch.equal(self.buf.view(torch.int32), torch.full_like(self.buf, SENT).view(torch.int32))


def _variant(pl, **kw):
    """A PairLists over the SAME device arrays with some products switched off or replaced (tests/test_gpu_pair_paths.py)."""
    from segdino3d_amd.ops import PairLists
    v = PairLists(pl.pos, pl.in_idx, pl.tile_k, pl.p_cap, pl.K, pl.M, rlist=pl.rlist, rl_stride=pl.rl_stride, center=pl.center,
                  out_idx=pl.out_idx, direct=pl.direct)
    for k, val in kw.items():
        setattr(v, k, val)
    return v


_LISTS, _NBR = {}, {}


def nbr_of(name):
    if name not in _NBR:
        _NBR[name] = up(C.table(name)["nbr"])
    return _NBR[name]


def lists_of(name, mode):
    """The table's PairLists, built once: plain lists, chained lists or the one-pair-per-row form."""
    from segdino3d_amd import ops
    if (name, mode) not in _LISTS:
        t = C.table(name)
        _LISTS[name, mode] = ops.pair_lists(nbr_of(name), t["n_pairs"], center=ops.PAIR_CHAINED if mode == "chained" else -1,
                                            direct=mode == "direct")
    return _LISTS[name, mode]


def sources(o, c):
    """(x, x2) on the device for a case: one source, or the two halves of a split."""
    if c.split:
        return up(o["x"][:, :c.split]), up(o["x"][:, c.split:])
    return up(o["x"]), None


def labels_of(c):
    t = C.table(c.table)
    return [C.pass1_variant(c.cin, c.cout, c.mode == "chained", c.mode == "direct", crowded, C.capacity_tiles(t)) for crowded in (False, True)]


def exact(family, case, label, got, ref):
    same = got.shape == ref.shape and torch.equal(got.cpu(), ref)
    record_exact(family, case, label, same)
    assert same, (family, case, label, "max |difference|", float((got.cpu().double() - ref.double()).abs().max()) if got.shape == ref.shape else got.shape)


# ---- pair_conv --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.PAIR_CASES, ids=C.case_id)
def test_pair_conv_integer(c):
    """Bit equality with the float64 reference: alone and with several scenes in flight (another pass-1 kernel, non-temporal partial
    stores), pass 2 over the row lists and over the position table, the one-pair-per-row table in two passes, mirrored weights."""
    from segdino3d_amd import ops
    t = C.table(c.table)
    o, ref, _mag = C.pair_int_case(c)
    pl = lists_of(c.table, c.mode)
    x, x2 = sources(o, c)
    w = up(o["w"])
    kw = dict(x2=x2, scale=up(o["scale"]), shift=up(o["shift"]), res=up(o["res"]), act=c.act)
    alone, crowded = labels_of(c)
    name = C.case_id(c)
    got = ops.pair_conv(x, w, pl, **kw)
    exact("pair_conv", name, alone, got, ref)
    if t["dead"] is not None:                                    # a row without any pair: act(shift + res)
        assert torch.equal(got[t["dead"]].cpu(), C.act_ref(o["shift"] + o["res"][t["dead"]], c.act))
    with ops.scenes_in_flight(4):
        exact("pair_conv", name + " in flight", crowded, ops.pair_conv(x, w, pl, **kw), ref)
    if c.mode == "plain":
        assert pl.rlist is not None and pl.pos is not None
        exact("pair_conv", name + " pass 2 over pos", alone, ops.pair_conv(x, w, _variant(pl, rlist=None), **kw), ref)
    elif c.mode == "direct":
        assert pl.direct and pl.rlist is None and pl.pos is not None
        two_pass = C.pass1_variant(c.cin, c.cout, False, False, False, C.capacity_tiles(t))
        exact("pair_conv", name + " two passes", two_pass, ops.pair_conv(x, w, _variant(pl, direct=False), **kw), ref)
    else:
        assert pl.center == ops.PAIR_CHAINED and pl.rlist is not None
    mirrored = ops.pair_conv(x, w, pl, mirror_w=True, **kw)
    explicit = ops.pair_conv(x, w.flip(0).contiguous(), pl, **kw)
    assert torch.equal(mirrored, explicit), "mirror_w must equal the call with the offsets' weights mirrored by hand"
    want, _ = C.conv_ref(o["x"], o["w"].flip(0), t["nbr"], o["scale"], o["shift"], o["res"], c.act, want_mag=False)
    exact("pair_conv", name + " mirror_w", alone, mirrored, want.float())


def test_pair_conv_range_longer_than_the_index_buffer():
    """3213 real tiles on the two-group kernel at Cin = 288: with 256 CUs the launch has 128 workgroups per column group, 25 tiles each -
    more than the 24 whose gather rows fit LDS, so every workgroup walks its range in two pieces."""
    from segdino3d_amd import ops
    c = C.RANGE_CASE
    t = C.table(c.table)
    o, ref, _mag = C.pair_int_case(c)
    pl = lists_of(c.table, c.mode)
    x, x2 = sources(o, c)
    real, cap = C.tile_counts(t["counts"])
    assert pl.p_cap // 128 == cap and int(pl.tile_k[cap]) == real
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    per_wg = real / C.ws_grid(c.cin, c.cout, cap, n_cu)
    got = ops.pair_conv(x, up(o["w"]), pl, x2=x2, scale=up(o["scale"]), shift=up(o["shift"]), res=up(o["res"]), act=c.act)
    exact("pair_conv", C.case_id(c) + f" ({n_cu} CUs: {per_wg:.1f} tiles per workgroup)", labels_of(c)[0], got, ref)


@pytest.mark.parametrize("c", C.PAIR_FLOAT_CASES, ids=C.case_id)
def test_pair_conv_float(c):
    from segdino3d_amd import ops
    o, r64, r32, mag = C.pair_float_case(c)
    pl = lists_of(c.table, c.mode)
    x, x2 = sources(o, c)
    w = up(o["w"])
    kw = dict(x2=x2, scale=up(o["scale"]), shift=up(o["shift"]), res=up(o["res"]), act=c.act)
    alone, crowded = labels_of(c)
    a = ops.pair_conv(x, w, pl, **kw)
    check_conv("pair_conv", C.case_id(c), alone, a, r64, r32, mag)
    with ops.scenes_in_flight(4):
        b = ops.pair_conv(x, w, pl, **kw)
    check_conv("pair_conv", C.case_id(c) + " in flight", crowded, b, r64, r32, mag)
    if c.mode == "plain":
        assert torch.equal(a, ops.pair_conv(x, w, _variant(pl, rlist=None), **kw)), "pass 2 over pos: the same offsets in the same order"
    if alone == crowded or c.mode == "direct":
        assert torch.equal(a, b), "the header promises the same bits from both pass-1 variants"


# ---- epilogue and layout ----------------------------------------------------------------------------------------------------------------------
EPILOGUES = [("scale",), ("shift",), ("res",), ()]
LAYOUT_PAIR = [C.PairCase("k27_m600", "plain", 96, 0, 96, "relu"), C.PairCase("up_planted", "direct", 96, 32, 100, "relu"),
               C.PairCase("sym27_planted", "chained", 64, 32, 36, None)]


def _epilogue(o, on, M=None):
    rows = slice(None) if M is None else slice(0, M)
    return dict(scale=o["scale"] if "scale" in on else None, shift=o["shift"] if "shift" in on else None,
                res=o["res"][rows] if "res" in on else None)


@pytest.mark.parametrize("c", LAYOUT_PAIR, ids=C.case_id)
def test_pair_conv_epilogue_and_layout(c):
    from segdino3d_amd import ops
    t = C.table(c.table)
    o = C.int_operands(t["V_in"], t["M"], t["K"], c.cin, c.cout, seed=1)
    pl = lists_of(c.table, c.mode)
    w = up(o["w"])
    label = labels_of(c)[0]
    for on in EPILOGUES + [("scale", "shift", "res")]:
        e = _epilogue(o, on)
        ref, _ = C.conv_ref(o["x"], o["w"], t["nbr"], act=c.act, want_mag=False, **e)
        x, x2 = (sliced(o["x"][:, :c.split]), sliced(o["x"][:, c.split:], left=8, right=4)) if c.split else (sliced(o["x"]), None)
        out = Slice(t["M"], c.cout)
        back = ops.pair_conv(x, w, pl, x2=x2, scale=up(e["scale"]), shift=up(e["shift"]), res=None if e["res"] is None else sliced(e["res"]),
                             act=c.act, out=out.view)
        assert back is out.view
        exact("pair_conv", f"{C.case_id(c)} strided, epilogue {'+'.join(on) or 'none'}", label, out.get(), ref.float())


LAYOUT_GG = [("k27_m600", 96, 32, 68, 0), ("k27_m600", 64, 0, 199, -12), ("k3_m150", 32, 0, 3, 2)]


@pytest.mark.parametrize("name,cin,split,cout,nt", LAYOUT_GG)
def test_gather_gemm_epilogue_and_layout(name, cin, split, cout, nt):
    from segdino3d_amd import ops
    t = C.table(name)
    o = C.int_operands(t["V_in"], t["M"], t["K"], cin, cout, seed=2)
    w, nbr = up(o["w"]), nbr_of(name)
    for on in EPILOGUES + [("scale", "shift", "res")]:
        e = _epilogue(o, on)
        ref, _ = C.conv_ref(o["x"], o["w"], t["nbr"], act="relu", want_mag=False, **e)
        x, x2 = (sliced(o["x"][:, :split]), sliced(o["x"][:, split:], left=8, right=4)) if split else (sliced(o["x"]), None)
        out = Slice(t["M"], cout, right=7)                       # a row stride that is no multiple of 4: these kernels store single floats
        ops.gather_gemm(x, w, nbr=nbr, x2=x2, scale=up(e["scale"]), shift=up(e["shift"]), res=None if e["res"] is None else sliced(e["res"], right=5),
                        act="relu", out=out.view, nt=nt)
        exact("gather_gemm", f"{name} {cin}->{cout} nt {nt} strided, epilogue {'+'.join(on) or 'none'}", ("gather_gemm", nt), out.get(), ref.float())


@pytest.mark.parametrize("M,cin,split,cout", [(16385, 32, 0, 64), (16511, 96, 64, 260)])
def test_dense_epilogue_and_layout(M, cin, split, cout):
    from segdino3d_amd import ops
    o = C.linear_operands(cin, cout)
    w = up(o["w"])
    assert C.takes_dense(M, cout, ld_out=LEFT + cout + RIGHT, ld_res=LEFT + cout + RIGHT)
    for on in EPILOGUES + [("scale", "shift", "res")]:
        e = _epilogue(o, on, M)
        ref, _ = C.conv_ref(o["x"][:M], o["w"], None, act="relu", want_mag=False, **e)
        xs = o["x"][:M]
        x, x2 = (sliced(xs[:, :split]), sliced(xs[:, split:], left=8, right=4)) if split else (sliced(xs), None)
        out = Slice(M, cout)
        ops.gather_gemm(x, w, x2=x2, scale=up(e["scale"]), shift=up(e["shift"]), res=None if e["res"] is None else sliced(e["res"]),
                        act="relu", out=out.view)
        exact("dense", f"{M} x {cin}->{cout} strided, epilogue {'+'.join(on) or 'none'}", C.dense_variant(cout), out.get(), ref.float())


def test_one_row_and_no_rows_and_no_columns():
    """M = 1 on every family; M == 0 and Cout == 0 return without an error and write nothing."""
    from segdino3d_amd import ops
    t = C.table("k1_m1")
    o = C.int_operands(1, 1, 1, 32, 36, seed=4)
    ref, _ = C.conv_ref(o["x"], o["w"], t["nbr"], o["scale"], o["shift"], o["res"], "relu", want_mag=False)
    kw = dict(scale=up(o["scale"]), shift=up(o["shift"]), res=up(o["res"]), act="relu")
    pl = lists_of("k1_m1", "plain")
    exact("pair_conv", "M = 1", C.pass1_variant(32, 36, False, False, False, 1), ops.pair_conv(up(o["x"]), up(o["w"]), pl, **kw), ref.float())
    for nt in (0, 2, -1, -12):
        exact("gather_gemm", f"M = 1 nt {nt}", ("gather_gemm", nt), ops.gather_gemm(up(o["x"]), up(o["w"]), nbr=nbr_of("k1_m1"), nt=nt, **kw), ref.float())
    exact("gather_gemm", "M = 1 identity", ("gather_gemm", 0), ops.gather_gemm(up(o["x"]), up(o["w"][0]), **kw), ref.float())

    t = C.table("k3_m150")
    o = C.int_operands(t["V_in"], t["M"], 3, 32, 36, seed=5)
    x, w, nbr = up(o["x"]), up(o["w"]), nbr_of("k3_m150")
    pl = lists_of("k3_m150", "plain")
    out = Slice(t["M"], 36)
    # no rows
    ops.pair_conv(x, w, _variant(pl, M=0), scale=up(o["scale"]), out=out.view[:0])
    ops.gather_gemm(x, w, nbr=nbr[:, :0].contiguous(), out=out.view[:0])
    ops.gather_gemm(x[:0], w[0], out=out.view[:0])
    assert ops.linear(x[:0], w[0]).shape == (0, 36)
    # no columns
    ops.pair_conv(x, w[:, :0].contiguous(), pl, out=out.view[:, :0])
    ops.gather_gemm(x, w[:, :0].contiguous(), nbr=nbr, out=out.view[:, :0])
    ops.gather_gemm(x, w[0, :0].contiguous(), out=out.buf[:t["V_in"], :0])
    assert ops.linear(x, w[0, :0].contiguous()).shape == (t["V_in"], 0)
    empty, full = ops.linear_group([(x, w[0, :0].contiguous(), None, None, None, None), (x, w[0], None, "relu", None, None)])
    assert empty.shape == (t["V_in"], 0) and torch.equal(full, ops.linear(x, w[0], act="relu"))
    torch.cuda.synchronize()
    assert out.untouched()


# ---- the dense product --------------------------------------------------------------------------------------------------------------------------
_DEV_LINEAR = {}


def dev_linear(cin, cout, rows=C.DENSE_ROWS[-1], kind="int"):
    if (cin, cout, rows, kind) not in _DEV_LINEAR:
        o = C.linear_operands(cin, cout, rows=rows, kind=kind)
        _DEV_LINEAR[cin, cout, rows, kind] = {k: up(v) for k, v in o.items()}
    return _DEV_LINEAR[cin, cout, rows, kind]


@pytest.mark.parametrize("c", C.DENSE_CASES, ids=C.case_id)
def test_dense_integer(c):
    """`ops.linear` and `ops.gather_gemm` around the 16384-row threshold: the ragged last 128-row tile, ragged column tiles, column groups,
    two sources; widths the dense kernel refuses go to the other kernels and must give the same exact answer."""
    from segdino3d_amd import ops
    o, d = C.linear_operands(c.cin, c.cout), dev_linear(c.cin, c.cout)
    M = c.M
    x, x2 = (d["x"][:M, :c.split], d["x"][:M, c.split:]) if c.split else (d["x"][:M], None)
    label = C.dense_variant(c.cout) if C.takes_dense(M, c.cout) else ("gather_gemm", 0)
    ref, _ = C.linear_ref(o, M, act=c.act, want_mag=False)
    if c.split:
        got = ops.gather_gemm(x, d["w"][0], x2=x2, shift=d["shift"], res=d["res"][:M], act=c.act)
    else:
        got = ops.linear(x, d["w"][0], bias=d["shift"], act=c.act, res=d["res"][:M])
    exact("dense", C.case_id(c) + " linear", label, got, ref.float())
    ref, _ = C.linear_ref(o, M, scale=True, res=False, act=c.act, want_mag=False)
    out = Slice(M, c.cout, right=RIGHT if c.cout % 4 == 0 else 7)
    ops.gather_gemm(x, d["w"], x2=x2, scale=d["scale"], shift=d["shift"], act=c.act, out=out.view)
    exact("dense", C.case_id(c) + " scale, out slice", label, out.get(), ref.float())


def test_dense_falls_through_on_an_odd_output_stride():
    """16384 rows, Cout = 100, a row stride of 111 floats (and a residual of 109): not the dense kernel, the same exact answer."""
    from segdino3d_amd import ops
    o, d = C.linear_operands(96, 100), dev_linear(96, 100)
    M = 16384
    ref, _ = C.linear_ref(o, M, scale=True, act="relu", want_mag=False)
    for right, res_right in ((7, RIGHT), (RIGHT, 5)):
        assert not C.takes_dense(M, 100, ld_out=LEFT + 100 + right, ld_res=LEFT + 100 + res_right)
        out = Slice(M, 100, right=right)
        ops.gather_gemm(d["x"][:M], d["w"], scale=d["scale"], shift=d["shift"], res=sliced(o["res"][:M], right=res_right), act="relu", out=out.view)
        exact("dense", f"16384 x 96->100 ld_out {LEFT + 100 + right} ld_res {LEFT + 100 + res_right}", ("gather_gemm", 0), out.get(), ref.float())


@pytest.mark.parametrize("rows,cin,cout", C.LINEAR_SHAPES)
def test_linear_below_the_dense_threshold(rows, cin, cout):
    """The 63 / 64 row-tile switch to the lock-step kernel, the contraction split over the four waves, ragged widths: exact on integers;
    on floats the rule, and `nt=dense_code(...)` reproduces the heuristic's launch bit for bit."""
    from segdino3d_amd import ops
    o, d = C.linear_operands(cin, cout, rows=C.LINEAR_ROWS), dev_linear(cin, cout, C.LINEAR_ROWS)
    code = ops.dense_code(rows, cin, cout)
    assert code == C.dense_plan_code(rows, cin, cout)
    ref, _ = C.linear_ref(o, rows, act="relu", want_mag=False)
    exact("linear", f"{rows} x {cin}->{cout}", ("gather_gemm", code), ops.linear(d["x"][:rows], d["w"][0], bias=d["shift"], act="relu", res=d["res"][:rows]), ref.float())
    f, fd = C.linear_operands(cin, cout, rows=C.LINEAR_ROWS, kind="float"), dev_linear(cin, cout, C.LINEAR_ROWS, "float")
    got = ops.linear(fd["x"][:rows], fd["w"][0], bias=fd["shift"], act="gelu", res=fd["res"][:rows])
    r64, mag = C.linear_ref(f, rows, act="gelu")
    r32, _ = C.linear_ref(f, rows, act="gelu", dtype=torch.float32, want_mag=False)
    check_conv("linear", f"{rows} x {cin}->{cout} float", ("gather_gemm", code), got, r64, r32, mag)
    if code != 0:
        forced = ops.gather_gemm(fd["x"][:rows], fd["w"][0], shift=fd["shift"], act="gelu", res=fd["res"][:rows], nt=code, exact=True)
        assert torch.equal(forced, got), "nt = dense_code must launch the kernel the heuristic picks"


# ---- the output-stationary gather-GEMM on tables ------------------------------------------------------------------------------------------------
GG_TABLES = list(C.TABLE_NAMES)
GG_CHANNELS = [(32, 0, 68), (96, 32, 199), (64, 0, 3), (160, 0, 96), (32, 0, 160), (96, 0, 36)]


@pytest.mark.parametrize("i,name", list(enumerate(GG_TABLES)), ids=GG_TABLES)
def test_gather_gemm_on_tables(i, name):
    """Every tiling code on every table, the fp32 kernels and the split-bf16 ones (integers in -2 .. 2 are exact in bf16)."""
    from segdino3d_amd import ops
    t = C.table(name)
    cin, split, cout = GG_CHANNELS[i % len(GG_CHANNELS)]
    c = C.PairCase(name, "plain", cin, split, cout, "relu" if i % 2 else None)
    o = C.int_operands(t["V_in"], t["M"], t["K"], cin, cout, seed=6)
    ref, mag = C.conv_ref(o["x"], o["w"], t["nbr"], o["scale"], o["shift"], o["res"], c.act)
    assert float(mag.max()) < C.EXACT_LIMIT
    ref = ref.float()
    x, x2 = sources(o, c)
    w, nbr = up(o["w"]), nbr_of(name)
    kw = dict(nbr=nbr, x2=x2, scale=up(o["scale"]), shift=up(o["shift"]), res=up(o["res"]), act=c.act)
    for nt in C.GG_NT:
        exact("gather_gemm", f"{name} {cin}->{cout}", ("gather_gemm", nt), ops.gather_gemm(x, w, nt=nt, **kw), ref)
    for terms in (1, 3, 6):
        for nt in (0, 1 + i % 4):
            got = ops.gather_gemm(x, w, nt=nt, wt_split=ops.split_weights(w, terms), **kw)
            exact("gather_gemm_split", f"{name} {cin}->{cout} bf16x{terms}", ("gather_gemm_split", nt), got, ref)


def _c_gather_gemm(x, nbr, w, M, out, nt, ws, ws_bytes):
    from segdino3d_amd import _lib, ops
    K, Cout, Cin = w.shape
    return _lib.load().sd3d_gather_gemm(x.data_ptr(), x.stride(0), Cin, None, 0, nbr.data_ptr(), w.data_ptr(), K, Cin, Cout, M, None, None, None, 0,
                                        out.data_ptr(), out.stride(0), 0, nt, None if ws is None else ws.data_ptr(), ws_bytes, ops._stream())


@pytest.mark.parametrize("name,nt", [("k27_m600", -13), ("big27_m6000", 0)])
def test_gather_gemm_offset_split_and_a_short_workspace(name, nt):
    """Few workgroups and K >= 8: the offsets are sliced over gridDim.z and `splitk_epilogue_kernel` adds the slices; with a workspace
    too short for the slices (or none) the launcher keeps the unsplit launch.  All exact; the slices' partial sums in the workspace
    show that the split ran, an untouched workspace that it did not."""
    from segdino3d_amd import _lib
    t = C.table(name)
    M, cin, cout = t["M"], 64, 96
    o = C.int_operands(t["V_in"], M, t["K"], cin, cout, seed=7)
    ref, _ = C.conv_ref(o["x"], o["w"], t["nbr"], want_mag=False)
    x, w, nbr = up(o["x"]), up(o["w"]), nbr_of(name)
    col_tiles = -nt - 10 if nt else C.lds_column_tiles((cout + 31) // 32, -(-M // 32), True)
    need = 8 * M * cout * 4
    ksp = C.lds_ksplit(M, cout, t["K"], col_tiles, need)
    assert ksp == (8 if nt else 4)
    used = ksp * M * cout * 4                                     # the slices' partial sums: [ksp][M][Cout] floats
    assert C.lds_ksplit(M, cout, t["K"], col_tiles, used - 1) == 1
    for ws_bytes, what in ((need, "offsets split over z"), (used - 1, "workspace one byte short"), (0, "no workspace")):
        ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=dev())
        out = Slice(M, cout)
        rc = _c_gather_gemm(x, nbr, w, M, out.view, nt, ws if ws_bytes else None, ws_bytes)
        torch.cuda.synchronize()
        _lib.check(rc, "gather_gemm")
        exact("gather_gemm", f"{name} {cin}->{cout} nt {nt}, {what}", ("gather_gemm", nt), out.get(), ref.float())
        if ws_bytes == need:                                     # every partial sum is a small integer: no float keeps the byte pattern
            parts = ws[:used].view(torch.float32).view(ksp, M, cout)
            assert not bool((ws[:used].view(torch.int32) == -1515870811).any()), "the split launch left part of its slices unwritten"
            assert torch.equal(parts.sum(0).cpu(), ref.float()), "the slices do not add up to the product"
            assert bool((ws[used:] == 0xA5).all()), "written behind the slices"
        else:
            assert bool((ws == 0xA5).all()), "the workspace was written although it is too short for the split"


# ---- linear_group -------------------------------------------------------------------------------------------------------------------------------
def _jobs(shapes, seed):
    """[(rows, Cin, split, Cout, act)] -> (jobs for ops.linear_group, float32 references)."""
    jobs, refs = [], []
    for i, (rows, cin, split, cout, act) in enumerate(shapes):
        o = C.int_operands(rows, rows, 1, cin, cout, seed=seed + i)
        bias, res = (o["shift"] if i % 3 != 2 else None), (o["res"] if i % 2 == 0 else None)
        ref, mag = C.conv_ref(o["x"], o["w"], None, None, bias, res, act)
        assert float(mag.max()) < C.EXACT_LIMIT
        x, x2 = (up(o["x"][:, :split]), up(o["x"][:, split:])) if split else (up(o["x"]), None)
        jobs.append((x, up(o["w"][0]), up(bias), act, up(res), x2))
        refs.append(ref.float())
    return jobs, refs


GROUPS = {
    "small": [(1, 32, 0, 3, None), (33, 96, 32, 199, "relu"), (200, 256, 0, 64, "relu")],
    "lock-step": [(2017, 64, 0, 199, "relu"), (3000, 96, 32, 64, None), (2100, 256, 0, 3, None), (2017, 64, 0, 256, "relu")],
    "nine": [(1 + 29 * i, 32 * (1 + i % 3), 0, (3, 36, 199)[i % 3], "relu" if i % 2 else None) for i in range(9)],
}


@pytest.mark.parametrize("which", list(GROUPS))
def test_linear_group(which):
    """Jobs of unequal size in one launch: each output equals its own single launch bit for bit and the integer reference."""
    from segdino3d_amd import ops
    jobs, refs = _jobs(GROUPS[which], seed=len(which))
    if which == "lock-step":
        assert all(ops.dense_code(j[0].shape[0], j[1].shape[1], j[1].shape[0]) == 0 for j in jobs)
    outs = ops.linear_group(jobs)
    assert len(outs) == len(jobs)
    for i, ((x, w, b, act, res, x2), got, ref) in enumerate(zip(jobs, outs, refs)):
        single = ops.gather_gemm(x, w, x2=x2, shift=b, act=act, res=res)
        assert torch.equal(got, single), (which, i)
        exact("linear_group", f"{which} job {i}: {x.shape[0]} x {w.shape[1]}->{w.shape[0]}", ("group", which), got, ref)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def _c_pair_conv(pl, x, w, out, **over):
    """`sd3d_pair_conv_ex` with every argument spelled out; `over` replaces some."""
    from segdino3d_amd import _lib, ops
    K, Cout, Cin = w.shape
    part = ops._WS3.get(pl.p_cap * Cout * 4, x.device)
    a = dict(in0=x.data_ptr(), ld0=x.stride(0), C0=Cin, in1=None, ld1=0, in_idx=pl.in_idx.data_ptr(), tile_k=pl.tile_k.data_ptr(), p_cap=pl.p_cap,
             pos=pl.pos.data_ptr(), rlist=pl.rlist.data_ptr(), rl_stride=pl.rl_stride, center=-1, out_idx=None, wt=w.data_ptr(), K=K, Cin=Cin,
             Cout=Cout, M=pl.M, scale=None, shift=None, res=None, ld_res=0, out=out.data_ptr(), ld_out=out.stride(0), act=0,
             part=part.data_ptr(), part_bytes=part.numel(), stream=ops._stream())
    assert set(over) <= set(a)
    a.update(over)
    return _lib.load().sd3d_pair_conv_ex(*a.values())


def _refused(rc, text):
    from segdino3d_amd import _lib
    assert rc == -1, rc                                          # SD3D_ERR_ARG
    msg = _lib.load().sd3d_last_error().decode()
    assert text in msg, msg


def test_pair_conv_refusals():
    """Every SD3D_ERR_ARG branch of `launch_pair_conv`, each checked before anything is launched; the output keeps its sentinel."""
    from segdino3d_amd import ops
    t = C.table("k3_m150")
    M, V = t["M"], t["V_in"]
    pl = lists_of("k3_m150", "plain")
    x, w = torch.zeros(V, 64, device=dev()), torch.zeros(3, 36, 64, device=dev())
    out = Slice(M, 36)
    odd = torch.zeros(V, 70, device=dev())[:, :64]                # a row stride of 70 floats
    res_odd = torch.zeros(M, 38, device=dev())[:, :36]
    assert _c_pair_conv(pl, x, w, out.view, M=0) == 0 and _c_pair_conv(pl, x, w, out.view, Cout=0) == 0
    _refused(_c_pair_conv(pl, x, w, out.view, Cin=48), "Cin must be a positive multiple of 32")
    _refused(_c_pair_conv(pl, x, w, out.view, Cin=0), "Cin must be a positive multiple of 32")
    _refused(_c_pair_conv(pl, x, w, out.view, Cout=34), "Cout must be a multiple of 4")
    _refused(_c_pair_conv(pl, x, w, out.view, in1=x.data_ptr(), ld1=64, C0=16), "concat split must be a multiple of 32")
    _refused(_c_pair_conv(pl, x, w, out.view, in1=x.data_ptr(), ld1=64, C0=96), "concat split must be a multiple of 32")
    _refused(_c_pair_conv(pl, odd, w, out.view), "row strides must be multiples of 4 floats")
    _refused(_c_pair_conv(pl, x, w, out.view, in1=odd.data_ptr(), ld1=70, C0=32), "row strides must be multiples of 4 floats")
    _refused(_c_pair_conv(pl, x, w, out.view, ld_out=out.view.stride(0) + 2), "row strides must be multiples of 4 floats")
    _refused(_c_pair_conv(pl, x, w, out.view, p_cap=pl.p_cap - 64), "p_cap must be a positive multiple of 128")
    _refused(_c_pair_conv(pl, x, w, out.view, p_cap=0), "p_cap must be a positive multiple of 128")
    _refused(_c_pair_conv(pl, x, w, out.view, part_bytes=pl.p_cap * 36 * 4 - 1), "partial-product buffer too small")
    _refused(_c_pair_conv(pl, x, w, out.view, res=res_odd.data_ptr(), ld_res=38), "residual row stride must be a multiple of 4 floats")
    for center in (0, 1, 13, -5, -6):
        _refused(_c_pair_conv(pl, x, w, out.view, center=center), "center must be -1 or SD3D_PAIR_CHAINED")
    _refused(_c_pair_conv(pl, x, w, out.view, rlist=None, pos=None), "pass 2 needs rlist, or pos, or out_idx")
    # ... and through the Python wrapper
    with pytest.raises(RuntimeError, match="Cout must be a multiple of 4"):
        ops.pair_conv(x, torch.zeros(3, 34, 64, device=dev()), pl, out=out.buf[1:-1, LEFT:LEFT + 34])
    with pytest.raises(RuntimeError, match="row strides must be multiples of 4 floats"):
        ops.pair_conv(odd, w, pl, out=out.view)
    with pytest.raises(RuntimeError, match="pass 2 needs"):
        ops.pair_conv(x, w, _variant(pl, rlist=None, pos=None), out=out.view)
    with pytest.raises(ValueError, match="weights have 5 offsets"):
        ops.pair_conv(x, torch.zeros(5, 36, 64, device=dev()), pl, out=out.view)
    with pytest.raises(ValueError, match="chained lists need an odd symmetric kernel"):
        ops.pair_lists(nbr_of("down_c40"), C.table("down_c40")["n_pairs"], center=ops.PAIR_CHAINED)
    torch.cuda.synchronize()
    assert out.untouched()


def test_gather_gemm_refusals():
    from segdino3d_amd import ops
    t = C.table("k3_m150")
    M, V = t["M"], t["V_in"]
    nbr = nbr_of("k3_m150")
    x, w = torch.zeros(V, 64, device=dev()), torch.zeros(3, 36, 64, device=dev())
    out = Slice(M, 36)
    odd = torch.zeros(V, 70, device=dev())[:, :64]
    for fn, who in ((lambda **kw: ops.gather_gemm(out=out.view, **kw), "gather_gemm"),
                    (lambda **kw: ops.gather_gemm(out=out.view, wt_split=ops.split_weights(kw["wt"], 3), **kw), "gather_gemm_split")):
        with pytest.raises(RuntimeError, match=f"{who}: Cin must be a positive multiple of 32"):
            fn(x=x[:, :48], wt=torch.zeros(3, 36, 48, device=dev()), nbr=nbr)
        with pytest.raises(RuntimeError, match=f"{who}: concat split must be a multiple of 32"):
            fn(x=x[:, :16], wt=w, nbr=nbr, x2=x[:, :48])
        with pytest.raises(RuntimeError, match=f"{who}: input row stride must be a multiple of 4 floats"):
            fn(x=odd, wt=w, nbr=nbr)
        with pytest.raises(RuntimeError, match=f"{who}: input row stride must be a multiple of 4 floats"):
            fn(x=x[:, :32], wt=w, nbr=nbr, x2=odd[:, :32])
        with pytest.raises(RuntimeError, match=f"{who}: at most 128 kernel offsets"):
            fn(x=x, wt=torch.zeros(129, 36, 64, device=dev()), nbr=torch.full((129, M), -1, dtype=torch.int32, device=dev()))
        with pytest.raises(RuntimeError, match=f"{who}: identity gather needs K == 1"):
            fn(x=x[:M], wt=w)
        with pytest.raises(RuntimeError, match=f"{who}: nt must be 1..4"):
            fn(x=x, wt=w, nbr=nbr, nt=5)
    with pytest.raises(ValueError, match="nbr shape"):
        ops.gather_gemm(x, w, nbr=nbr[:2], out=out.view)
    with pytest.raises(ValueError, match="wt_split must be contiguous bf16"):
        ops.gather_gemm(x, w, nbr=nbr, wt_split=ops.split_weights(w, 3).float(), out=out.view)
    with pytest.raises(ValueError, match="expected a 2-D fp32 tensor with contiguous rows"):
        ops.gather_gemm(x.double(), w, nbr=nbr, out=out.view)
    torch.cuda.synchronize()
    assert out.untouched()


def test_linear_group_refusals():
    """`sd3d_linear_group` through its C entry: the job table of `ops.linear_group` with one bad field."""
    from segdino3d_amd import _lib, ops
    lib = _lib.load()
    out = Slice(2100, 64)

    def table(n, rows, **bad):
        x, w = torch.zeros(rows, 96, device=dev()), torch.zeros(64, 64, device=dev())
        keep.extend([x, w])
        tab = np.zeros(n, dtype=ops._LINEAR_JOB_DT)
        for i in range(n):
            tab[i] = (x.data_ptr(), 0, w.data_ptr(), 0, 0, out.view.data_ptr(), rows, 96, 64, 0, 64, 64, 0, out.view.stride(0), 0)
        for k, v in bad.items():
            tab[n - 1][k] = v
        return tab

    keep = []
    for rows in (200, 2100):                                     # the small group kernel; the grouped lock-step kernel
        assert lib.sd3d_linear_group(0, table(1, rows).ctypes.data, ops._stream()) == 0
        _refused(lib.sd3d_linear_group(9, table(9, rows).ctypes.data, ops._stream()), "at most 8 jobs per launch")
        x2 = torch.zeros(rows, 96, device=dev())
        keep.append(x2)
        _refused(lib.sd3d_linear_group(2, table(2, rows, in1=x2.data_ptr(), ld1=96, C0=16).ctypes.data, ops._stream()), "concat split must be a multiple of 32")
        _refused(lib.sd3d_linear_group(2, table(2, rows, in1=x2.data_ptr(), ld1=96, C0=96).ctypes.data, ops._stream()), "concat split must be a multiple of 32")
        _refused(lib.sd3d_linear_group(2, table(2, rows, ld0=98).ctypes.data, ops._stream()), "input row stride must be a multiple of 4 floats")
        _refused(lib.sd3d_linear_group(2, table(2, rows, in1=x2.data_ptr(), ld1=98, C0=32).ctypes.data, ops._stream()), "input row stride must be a multiple of 4 floats")
    for bad in (dict(Cin=48), dict(Cin=0), dict(M=0), dict(Cout=0)):
        _refused(lib.sd3d_linear_group(2, table(2, 200, **bad).ctypes.data, ops._stream()), "Cin must be a positive multiple of 32")
    # every job on 2017 rows or more (the grouped lock-step kernel), one of them without columns
    _refused(lib.sd3d_linear_group(2, table(2, 2100, Cout=0).ctypes.data, ops._stream()), "linear_group: empty job")
    x, w = torch.zeros(33, 64, device=dev()), torch.zeros(8, 64, device=dev())
    with pytest.raises(ValueError, match="linear_group: input channels do not match"):
        ops.linear_group([(x, w, None, None, None, None), (x, w, None, None, None, x)])
    with pytest.raises(ValueError, match="linear_group: residual must be"):
        ops.linear_group([(x, w, None, None, None, None), (x, w, None, None, torch.zeros(33, 9, device=dev()), None)])
    with pytest.raises(ValueError, match="linear_group: bias must be"):
        ops.linear_group([(x, w, None, None, None, None), (x, w, torch.zeros(9, device=dev()), None, None, None)])
    torch.cuda.synchronize()
    assert out.untouched()
