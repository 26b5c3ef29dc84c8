"""Row-chain executor (`segdino3d_amd/csrc/rowchain.hip`, `csrc/rowchain_narrow.hip`, `csrc/rowchain_ops.h`; `sd3d_row_chain`): every op on
both tile shapes against the float64 reference of the same operation in tests/rowchain_cases.py (LN, PE, BOX: the references and planted
rows of tests/decoder_kernel_cases.py), at the shapes the CPU test tests/test_rowchain_cases.py proves sufficient - all 13 instantiations of
the 16-row LINEAR dispatch with every block count mod 3 of the generic loops, the K parts and round sizes of the 4-row split, both paths
of BITS2D, the 16- and 64-key tile edges of ATTN, key splits of MERGE with a blocked split and a scene that starts inside a 32-row block.

Integer LINEAR cases, LOAD / STORE, the centres and plain sizes of BOX, the decoded bits of BITS2D and the constant LayerNorm row are
compared bit for bit; float outputs by `check_float`, whose bound comes from the fp32 evaluation of the reference on the CPU.  Every
output buffer carries 64 sentinel elements behind its end and pre-filled padding columns - both must come back untouched; the padding
columns of every input row hold NaN, so a read behind a row's width shows.  Every float case prints a `[rowchain-error]` line;
profiles/rowchain_errors.md holds the table."""
import ctypes as C

import pytest
import torch

from tests import decoder_kernel_cases as K
from tests import rowchain_cases as R
from tests.helpers import Out, wide
from tests.rowchain_cases import check_float

pytestmark = pytest.mark.gpu
ERR_ARG = -1
NAN = float("nan")


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(params=[16, 4], ids=["rows16", "rows4"])
def tile(request):
    return request.param


def up(t):
    return None if t is None else t.contiguous().to(_dev())


def d64(t):
    return None if t is None else t.double()


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def inp(t, pad=4):
    """[R, W] CPU tensor -> its device copy as a [R, W] view of rows W + pad apart whose padding holds NaN."""
    full, _ = wide(t, pad, poison=NAN)
    return full[:, :t.shape[1]]


def outp(n, width, pad=4):
    """-> (Out, its [n, width] view of rows width + pad apart)."""
    ld = width + pad
    o = Out(n * ld)
    return o, o.buf[:n * ld].view(n, ld)[:, :width]


def rows_of(o, view):
    """What the kernel wrote through `view`; the sentinels and the padding columns must still hold the fill."""
    n, width, ld = view.shape[0], view.shape[1], view.stride(0)
    full = o.get(n, ld)
    assert bool((full[:, width:] == o.fill).all()), "columns behind the row's width were written"
    return full[:, :width].contiguous()


def two_scenes(rows):
    return [dict(q0=0, nq=rows[0]), dict(q0=rows[0], nq=rows[1])]


def op_flag(P, i=-1):
    from segdino3d_amd import rowchain as RC
    i = P.n_ops + i if i < 0 else i
    return P.buf.raw[RC._OFF_OPS + 64 * i + 6]


# ---- LINEAR ---------------------------------------------------------------------------------------------------------------------------------
def add_linear(P, dst, src0, w, b, act, res, src1, k1, gout):
    """`Program.linear`; two sources of different widths (k0 != k1), which the wrapper cannot say, through `Program._op`."""
    from segdino3d_amd import ops
    from segdino3d_amd import rowchain as RC
    cout, Kt = w.shape
    if src1 is None or k1 == Kt // 2:
        P.linear(dst, src0, w, b, act=act, res=res, src1=src1, gout=gout)
        return
    wp = RC.pack_weight(w, P.rows)
    P._op(keep=(wp, b, gout), type=RC.LINEAR, act=ops.ACT[act], src0=src0, src1=src1, dst=RC.NONE if dst is None else dst,
          res=RC.NONE if res is None else res, flag=RC.F_NO_LDS_DST if dst is None else 0, k0=Kt - k1, k1=k1, cout=cout,
          ld=0 if gout is None else gout.stride(0), p0=wp.data_ptr(), p1=b.data_ptr(), p2=0 if gout is None else gout.data_ptr())


def run_linear(c, exact, tile):
    """-> (global copy, LDS copy or None, second program's global copy or None) of the case's Linear over its two scenes."""
    from segdino3d_amd import rowchain as RC
    p = R.linear_case(c, exact)
    plan = R.linear_slots(c)
    k0, k1, cout, n, opt = p["k0"], p["k1"], p["cout"], p["n"], p["opt"]
    x0 = inp(p["x"][:, :k0], 4)
    x1 = inp(p["x"][:, k0:], 8) if k1 else None
    res = None
    if p["res"] is not None:                                    # LOAD moves multiples of 4 columns: the columns past cout hold NaN too
        wpad = -cout % 4
        res = inp(torch.cat([p["res"], torch.full((n, wpad), NAN)], 1), 4)
    w, b = up(p["w"]), up(p["b"])
    P = RC.Program(plan["n_slots"], rows=tile)
    outs = []

    def body():
        P.load(plan["src0"], x0)
        if k1:
            P.load(plan["src1"], x1)
        if res is not None:
            P.load(plan["res"], res)
        o, v = outp(n, cout, 12)
        add_linear(P, plan["dst"], plan["src0"], w, b, p["act"], plan["res"], plan["src1"], k1, v)
        if opt == "inplace":
            assert op_flag(P) & RC.F_INPLACE                    # a destination over its source: Program.linear must say so
        elif k1 in (0, (k0 + k1) // 2):
            assert not op_flag(P) & RC.F_INPLACE
        outs.append((o, v))
        if plan["dst"] is not None:
            o2, v2 = outp(n, cout, 8)
            P.store(plan["dst"], v2)
            outs.append((o2, v2))
    body()
    if opt == "prog4":                                          # the same op in program 0 and in program 3; two loads between them
        P.begin(); P.load(plan["src0"], x0)
        P.begin(); P.load(plan["src0"], x0)
        P.begin(); body()
    P.launch(two_scenes(p["rows"]))
    torch.cuda.synchronize()
    return p, [rows_of(o, v) for o, v in outs]


@pytest.mark.parametrize("c", R.LINEAR_EXACT, ids=R.linear_id)
def test_linear_exact(c, tile):
    p, got = run_linear(c, True, tile)
    ref = R.linear_ref(p["x"].double(), p["w"].double(), p["b"].double(), d64(p["res"]), p["act"]).float()
    for i, g in enumerate(got):                                 # the global copy, the LDS copy, program 3's two
        assert same_bits(g, ref), (R.linear_id(c), i, float((g.double() - ref.double()).abs().max()))


@pytest.mark.parametrize("c", R.LINEAR_FLOAT, ids=R.linear_id)
def test_linear_float(c, tile):
    p, got = run_linear(c, False, tile)
    r64 = R.linear_ref(p["x"].double(), p["w"].double(), p["b"].double(), d64(p["res"]), p["act"])
    r32 = R.linear_ref(p["x"], p["w"], p["b"], p["res"], p["act"])
    check_float("linear", f"rows{tile} {R.linear_id(c)}", got[0], r64, r32, R.linear_scale(p["x"], p["w"], p["b"], p["res"], p["act"]))
    for g in got[1:]:
        assert same_bits(g, got[0])


# ---- ATTN -------------------------------------------------------------------------------------------------------------------------------------
def attn_launch(cases, masked, tile):
    """The scenes' attention in one launch -> per scene (output rows, the stand-alone kernel's rows)."""
    from segdino3d_amd import ops
    from segdino3d_amd import rowchain as RC
    q = inp(torch.cat([c["q"] for c in cases]), 4)
    kv = inp(torch.cat([torch.cat([c["k"], c["v"]], 1) for c in cases]), 4)
    k, v = kv[:, :R.D], kv[:, R.D:]
    n = q.shape[0]
    P = RC.Program(4, rows=tile)
    P.load(0, q)
    scenes, q0, m0, boff, noff = [], 0, 0, 0, 0
    nw_max = nw2_max = 0
    if masked:
        # the mask through BITS2D: superpoint s is near key s alone, so a query's open superpoints are its open keys
        blk, near = [], []
        for c in cases:
            Mq = c["Lk"] - 1
            nw = max(1, (Mq + 31) // 32)
            blk.append(R.pack_bits(~c["open"][:, :Mq], nw, True).reshape(-1))
            near.append(R.pack_bits(torch.eye(Mq, dtype=torch.bool), nw, False).reshape(-1))
            scenes.append(dict(q0=q0, nq=c["nq"], m0=m0, nm=c["Lk"], bits_off=boff, nw=nw, near_off=noff))
            q0, m0, boff, noff = q0 + c["nq"], m0 + c["Lk"], boff + blk[-1].numel(), noff + near[-1].numel()
            nw_max, nw2_max = max(nw_max, nw), max(nw2_max, (c["Lk"] + 31) // 32)
        blk_all = up(torch.cat(blk + [torch.full((4,), -1, dtype=torch.int32)]))
        near_all = up(torch.cat(near + [torch.zeros(4, dtype=torch.int32)]))
        P.bits2d(blk_all, near_all)
        P.attn(1, 0, k, v, R.ATTN_SCALE, aux=2, keys_2d=True, masked=True)
    else:
        for c in cases:
            scenes.append(dict(q0=q0, nq=c["nq"]))
            q0 += c["nq"]
        P.attn(1, 0, k, v, R.ATTN_SCALE, aux=2)
    o, view = outp(n, R.D, 4)
    P.store(1, view)
    P.launch(scenes, nw_max=nw_max, nw2_max=nw2_max)
    torch.cuda.synchronize()
    got = rows_of(o, view)
    res, k0 = [], 0
    for c, sc in zip(cases, scenes):
        bits = up(R.pack_bits(~c["open"], (c["Lk"] + 31) // 32, True)) if masked else None
        alone = ops.attention(up(c["q"]), k[k0:k0 + c["Lk"]], v[k0:k0 + c["Lk"]], R.H, R.ATTN_SCALE, mask_bits=bits)
        res.append((got[sc["q0"]:sc["q0"] + c["nq"]], alone.cpu()))
        k0 += c["Lk"]
    return res


def check_attn(tag, c, got, alone):
    q, k, v = c["q"], c["k"], c["v"]
    r64 = R.attn_ref(q.double(), k.double(), v.double(), R.ATTN_SCALE, c["open"])
    r32 = R.attn_ref(q, k, v, R.ATTN_SCALE, c["open"])
    check_float("attn", f"{tag} nq{c['nq']} Lk{c['Lk']} spread{R.ATTN_SPREAD}", got, r64, r32, R.attn_scale(v, c["open"], c["nq"]))
    rel = float((got.double() - alone.double()).abs().max() / (alone.double().abs().max() + 1e-30))
    assert rel < 2e-5, (tag, rel)                               # the stand-alone attention kernel (tests/test_gpu_rowchain.py)


@pytest.mark.parametrize("pair", R.ATTN_2D, ids=lambda p: f"{p[0][0]}x{p[0][1]}+{p[1][0]}x{p[1][1]}")
def test_attention_masked_2d(pair, tile):
    cases = [R.attn_case(nq, Lk, True, R.ATTN_SPREAD) for nq, Lk in pair]
    for c, (got, alone) in zip(cases, attn_launch(cases, True, tile)):
        check_attn(f"rows{tile} 2d", c, got, alone)


@pytest.mark.parametrize("pair", R.ATTN_SELF, ids=lambda p: f"{p[0]}+{p[1]}")
def test_attention_self(pair, tile):
    cases = [R.attn_case(n, n, False, R.ATTN_SPREAD) for n in pair]
    for c, (got, alone) in zip(cases, attn_launch(cases, False, tile)):
        check_attn(f"rows{tile} self", c, got, alone)


# ---- BITS2D -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("launch", R.BITS_LAUNCHES, ids=lambda l: "+".join(f"q{a}w{b}m{c}" for a, b, c in l))
def test_bits2d_decoded_through_attention(launch, tile):
    """Equal logits (q = 0) and the key table as V: a query's output is 1 / (its open keys) at its open keys' columns, 0 elsewhere -
    the open set of BITS2D, decoded exactly.  Twice: the table as it is and shifted by one column."""
    from segdino3d_amd import rowchain as RC
    cases = [R.bits_case(nq, nw, nm, si == 0) for si, (nq, nw, nm) in enumerate(launch)]
    n, nm_all = sum(c["nq"] for c in cases), sum(c["nm"] for c in cases)
    q = inp(torch.zeros(n, R.D), 4)
    blk = up(torch.cat([R.pack_bits(~c["open"], c["nw"], True).reshape(-1) for c in cases] + [torch.full((4,), -1, dtype=torch.int32)]))
    near = up(torch.cat([R.pack_bits(c["near"], c["nw"], False).reshape(-1) for c in cases] + [torch.zeros(4, dtype=torch.int32)]))
    scenes, q0, m0, boff, noff = [], 0, 0, 0, 0
    for c in cases:
        scenes.append(dict(q0=q0, nq=c["nq"], m0=m0, nm=c["nm"], bits_off=boff, nw=c["nw"], near_off=noff))
        q0, m0, boff, noff = q0 + c["nq"], m0 + c["nm"], boff + c["nq"] * c["nw"], noff + (c["nm"] - 1) * c["nw"]
    assert scenes[1]["bits_off"] > 0 and (scenes[1]["near_off"] > 0 or cases[0]["nm"] == 1)
    for shift in (0, 1):
        kv = inp(torch.cat([torch.cat([torch.zeros(c["nm"], R.D), R.key_table(c["nm"], shift)], 1) for c in cases]), 4)
        P = RC.Program(4, rows=tile)
        P.load(0, q)
        P.bits2d(blk, near)
        P.attn(1, 0, kv[:, :R.D], kv[:, R.D:], R.ATTN_SCALE, aux=2, keys_2d=True, masked=True)
        o, view = outp(n, R.D, 4)
        P.store(1, view)
        P.launch(scenes, nw_max=max(c["nw"] for c in cases), nw2_max=max((c["nm"] + 31) // 32 for c in cases))
        torch.cuda.synchronize()
        got = rows_of(o, view)
        for c, sc in zip(cases, scenes):
            g = got[sc["q0"]:sc["q0"] + c["nq"]]
            open_ref = ~R.bits2d_ref(c["open"], c["near"])                                 # [nq, nm]
            cols = (torch.arange(c["nm"]) + shift) % R.D
            decoded = g[:, cols] > 0
            assert torch.equal(decoded, open_ref), (launch, shift, (decoded != open_ref).nonzero()[:8].tolist())
            want = torch.zeros(c["nq"], R.D)
            want[:, cols] = open_ref.float() / open_ref.sum(1, keepdim=True).float()
            assert torch.allclose(g, want, rtol=1e-6, atol=0), (launch, shift)
            for qi, mi, _ in c["planted"]:
                assert bool(decoded[qi, mi])
            assert int(decoded[0].sum()) == 1 and bool(decoded[0, c["nm"] - 1])            # nothing open: the dummy key alone


# ---- MERGE ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes", [((7, 40, 2), (45, 97, 3)), ((33, 64, 1), (40, 333, 8)), ((5, 20, 1), (37, 50, 2))],
                         ids=lambda s: "+".join(f"q{a}k{b}z{c}" for a, b, c in s))
def test_merge_against_float64(shapes, tile):
    """Partial softmax states laid out as attention.hip leaves them; the second scene starts inside a 32-row block of the launch's rows
    (its own blocks count from its first row); split 0 of row 0 has every key blocked; a scene with one split copies its finished rows."""
    from segdino3d_amd import rowchain as RC
    cases = [R.merge_case(*s) for s in shapes]
    n = sum(c["nq"] for c in cases)
    parts, scenes, q0, off = [], [], 0, 0
    for c in cases:
        ws = R.merge_pack(c)
        scenes.append(dict(q0=q0, nq=c["nq"], ksplit=c["ksplit"], part_off=off))
        parts.append(ws)
        q0, off = q0 + c["nq"], off + ws.numel()
    assert scenes[1]["q0"] % 32 != 0 and scenes[1]["part_off"] > 0
    ws = up(torch.cat(parts))
    done = torch.randn(n, R.D, generator=R.gen(103, n))
    for c, sc in zip(cases, scenes):                            # rows of a split scene are not final in `out`: poison
        if c["ksplit"] > 1:
            done[sc["q0"]:sc["q0"] + c["nq"]] = NAN
    P = RC.Program(2, rows=tile)
    P.merge(1, ws, inp(done, 4))
    o, view = outp(n, R.D, 4)
    P.store(1, view)
    P.launch(scenes)
    torch.cuda.synchronize()
    got = rows_of(o, view)
    for c, sc in zip(cases, scenes):
        g = got[sc["q0"]:sc["q0"] + c["nq"]]
        if c["ksplit"] == 1:
            assert same_bits(g, done[sc["q0"]:sc["q0"] + c["nq"]])
            continue
        r64 = R.merge_ref(c["m"].double(), c["l"].double(), c["o"].double())
        check_float("merge", f"rows{tile} nq{c['nq']} ksplit{c['ksplit']} q0={sc['q0']}", g, r64, R.merge_ref(c["m"], c["l"], c["o"]),
                    R.attn_scale(c["v"], c["open"], c["nq"]))


def test_merge_equals_the_attention_kernels_own_merge_in_two_scenes(tile):
    """Bit for bit the stand-alone attention's result, the second scene starting at row 45 of the launch."""
    from segdino3d_amd import ops
    from segdino3d_amd import rowchain as RC
    d, g = _dev(), torch.Generator().manual_seed(7)
    sizes = [(45, 700), (70, 3000)]
    total = sum(s[0] for s in sizes)
    a = torch.full((total, R.D), NAN, device=d)
    jobs, refs, q0 = [], [], 0
    for Lq, Lk in sizes:
        q, q2 = torch.randn(Lq, R.D, generator=g).to(d), torch.randn(Lq, R.D, generator=g).to(d)
        k, k2, v = (torch.randn(Lk, R.D, generator=g).to(d) for _ in range(3))
        bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (Lq, (Lk + 31) // 32), generator=g, dtype=torch.int64).to(torch.int32).to(d)
        refs.append(ops.attention(q, k, v, R.H, 0.125, mask_bits=bits, q2=q2, k2=k2))
        jobs.append((q, k, v, bits, q2, k2, a[q0:q0 + Lq]))
        q0 += Lq
    ws, ca = ops.attention_parts(jobs, R.H, 0.125)
    P = RC.Program(2, rows=tile)
    P.merge(0, ws, a)
    o, view = outp(total, R.D, 4)
    P.store(0, view)
    scenes, q0 = [], 0
    for (Lq, _), (ks, off) in zip(sizes, ca):
        scenes.append(dict(q0=q0, nq=Lq, ksplit=ks, part_off=off))
        q0 += Lq
    P.launch(scenes)
    torch.cuda.synchronize()
    got = rows_of(o, view)
    assert ca[1][0] > 1                                         # the long scene's keys were split
    assert same_bits(got[:45], refs[0].cpu()) and same_bits(got[45:], refs[1].cpu())


# ---- LN, PE, BOX --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", R.SMALL_ROWS)
def test_layernorm_and_pe(rows, tile):
    from segdino3d_amd import rowchain as RC
    n, rng_rows, ranges = R.scene_rows(rows)
    scenes = two_scenes((rows, R.SECOND_SCENE_ROWS))
    c = K.ln_case(n, R.D)
    p = R.pe_rows(rows)
    dim_t, axis = K.pe_tables(R.D)
    w, b = up(c["w"]), up(c["b"])
    xyz, den, tdim, tax = up(p["xyz"]), up(p["den2"]), up(dim_t), up(axis)
    num4 = inp(torch.cat([p["mod_num"], torch.full((n, 1), NAN)], 1), 4)
    P = RC.Program(6, up(ranges), rows=tile)
    P.load(0, inp(c["x"], 4))
    P.load(1, inp(c["res"], 8))
    outs = {}
    for name, kw in (("ln res", dict(res=1)), ("ln res relu", dict(res=1, act="relu")), ("ln", dict()), ("ln relu", dict(act="relu"))):
        o, v = outp(n, R.D, 12)
        o2, v2 = outp(n, R.D, 4)
        P.ln(2, 0, w, b, gout=v, **kw)
        P.store(2, v2)
        outs[name] = (o, v, o2, v2)
    po, pv = outp(n, R.D, 4)
    P.pe(3, xyz, tdim, tax)
    P.store(3, pv)
    P.load(4, num4)
    mo, mv = outp(n, R.D, 8)
    P.pe(3, xyz, tdim, tax, num_slot=4, den=den)
    P.store(3, mv)
    P.launch(scenes)
    torch.cuda.synchronize()
    for name, (o, v, o2, v2) in outs.items():
        res, relu = (c["res"] if "res" in name else None), "relu" in name
        got = rows_of(o, v)
        r64 = K.layernorm_ref(c["x"].double(), d64(res), c["w"].double(), c["b"].double(), relu=relu)
        check_float("layernorm", f"rows{tile} M{rows}+{R.SECOND_SCENE_ROWS} {name}", got, r64, K.layernorm_ref(c["x"], res, c["w"], c["b"], relu=relu),
                    K.layernorm_scale(c["x"], res, c["w"], c["b"]))
        assert same_bits(rows_of(o2, v2), got)                  # the LDS copy
        if c["const"] is not None:                              # variance 0: the output is b, bit for bit
            assert same_bits(got[c["const"]], torch.relu(c["b"]) if relu else c["b"])
    for name, o, v, num, dn in (("plain", po, pv, None, None), ("modulated", mo, mv, p["mod_num"], p["den2"])):
        r64 = K.sine_pe_ref(p["xyz"].double(), rng_rows.double(), dim_t.double(), axis, d64(num), d64(dn))
        r32 = K.sine_pe_ref(p["xyz"], rng_rows, dim_t, axis, num, dn)
        check_float("sine_pe", f"rows{tile} n{rows}+{R.SECOND_SCENE_ROWS} {name}", rows_of(o, v), r64, r32, K.sine_pe_scale(p["xyz"], rng_rows, dim_t, axis, num, dn))


@pytest.mark.parametrize("rows", R.SMALL_ROWS)
def test_box(rows, tile):
    from segdino3d_amd import rowchain as RC
    n, rng_rows, ranges = R.scene_rows(rows)
    c = R.box_rows(rows)
    pad4 = lambda t: inp(torch.cat([t, torch.full((n, 1), NAN)], 1), 4)  # noqa: E731
    ref, sp = up(c["ref"]), up(c["sp2"])
    P = RC.Program(2, up(ranges), rows=tile)
    P.load(0, pad4(c["dc"]))
    P.load(1, pad4(c["ds"]))
    o = {name: Out(3 * n) for name in ("c_norm", "s_norm", "m_norm", "c_plain", "s_plain", "m_plain", "c_only")}
    t = {name: b.buf[:3 * n].view(n, 3) for name, b in o.items()}
    P.box(ref, 0, t["c_norm"], size_prev=sp, ds_slot=1, size=t["s_norm"], size_metric=t["m_norm"], normalize=True)
    P.box(ref, 0, t["c_plain"], size_prev=sp, ds_slot=1, size=t["s_plain"], size_metric=t["m_plain"], normalize=False)
    P.box(ref, 0, t["c_only"])
    P.launch(two_scenes((rows, R.SECOND_SCENE_ROWS)))
    torch.cuda.synchronize()
    got = {name: b.get(n, 3) for name, b in o.items()}
    centre = c["ref"] + c["dc"]
    for name in ("c_norm", "c_plain", "c_only"):
        assert same_bits(got[name], centre), name
    plain = c["sp2"] + c["ds"]
    assert same_bits(got["s_plain"], plain) and same_bits(got["m_plain"], plain)
    _, s64, m64 = K.box_refine_ref(c["ref"].double(), c["dc"].double(), c["sp2"].double(), c["ds"].double(), rng_rows.double(), True)
    _, s32, m32 = K.box_refine_ref(c["ref"], c["dc"], c["sp2"], c["ds"], rng_rows, True)
    ss, sm = K.box_size_scale(c["sp2"], c["ds"], rng_rows)
    check_float("box size", f"rows{tile} Q{rows}+{R.SECOND_SCENE_ROWS}", got["s_norm"], s64, s32, ss)
    check_float("box size_metric", f"rows{tile} Q{rows}+{R.SECOND_SCENE_ROWS}", got["m_norm"], m64, m32, sm)


# ---- LOAD, STORE ------------------------------------------------------------------------------------------------------------------------------
def test_load_store_bit_exact(tile):
    from segdino3d_amd import rowchain as RC
    rows = (17, 5)
    n = sum(rows)
    g = R.gen(107)
    for width, store_widths in ((4, (4, 1, 3)), (8, (8,)), (256, (256, 199)), (260, (260,)), (1024, (1024,))):
        x = torch.randn(n, width, generator=g)
        P = RC.Program(R.nslots(width), rows=tile)
        P.load(0, inp(x, 12))                                   # leading dimension width + 12
        outs = []
        for sw in store_widths:
            o, v = outp(n, sw, 5 if sw & 3 else 8)
            P.store(0, v)
            outs.append((sw, o, v))
        P.launch(two_scenes(rows))
        torch.cuda.synchronize()
        for sw, o, v in outs:
            assert same_bits(rows_of(o, v), x[:, :sw]), (width, sw)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def raw_launch(P, scenes, nw_max=0, nw2_max=0, **over):
    """`Program.launch` with any header field overridden -> (status, message); nothing is raised."""
    from segdino3d_amd import _lib, ops
    from segdino3d_amd import rowchain as RC
    lib = _lib.load()
    tile0, tiles = [0] * (RC.MAX_BATCH + 1), 0
    for i, sc in enumerate(scenes):
        tile0[i] = tiles
        tiles += (sc["nq"] + P.rows - 1) // P.rows
        g = sc.get
        RC._SCENE.pack_into(P.buf, RC._OFF_SCENES + 40 * i, sc["q0"], sc["nq"], g("m0", 0), g("nm", 0), g("bits_off", 0), g("nw", 0),
                            g("near_off", 0), g("ksplit", 0), g("part_off", 0))
    tile0[len(scenes)] = tiles
    tile0 = over.get("tile0", tile0)
    pb = P.prog_begin + [P.n_ops]
    pb += [P.n_ops] * (RC.MAX_PROGRAMS + 1 - len(pb))
    RC._HEAD.pack_into(P.buf, 0, over.get("n_scenes", len(scenes)), over.get("n_programs", len(P.prog_begin)), over.get("n_slots", P.n_slots),
                       nw_max, nw2_max, over.get("tile_rows", P.rows), P.rng, *tile0, *pb)
    rc = lib.sd3d_row_chain(C.addressof(P.buf), ops._stream())
    torch.cuda.synchronize()
    return rc, lib.sd3d_last_error().decode(errors="replace")


def test_refusals_come_back_before_any_launch(tile):
    from segdino3d_amd import rowchain as RC
    d = _dev()
    n = 20
    x = inp(torch.randn(n, 256, generator=R.gen(109)), 4)
    w = torch.zeros(4096, device=d)
    xyz, i8 = torch.zeros(n, 3, device=d), torch.zeros(256, dtype=torch.int8, device=d)
    bits = torch.zeros(n * 8, dtype=torch.int32, device=d)
    one = [dict(q0=0, nq=n)]
    tiles = (n + tile - 1) // tile
    o, view = outp(n, 256, 4)

    def prog(n_slots=2, rng=None):
        P = RC.Program(n_slots, rng, rows=tile)
        P.load(0, x)
        return P

    def lin(**kw):
        P = prog()
        f = dict(type=RC.LINEAR, src0=0, dst=1, k0=256, cout=256, p0=w.data_ptr())
        f.update(kw)
        P._op(keep=(w,), **f)
        return P

    def with_op(n_slots=2, rng=None, **kw):
        P = prog(n_slots, rng)
        P._op(**kw)
        return P
    cases = [
        ("1..16 scenes", prog(), dict(scenes=[])),
        ("1..16 scenes", prog(), dict(scenes=one, n_scenes=17)),
        ("1..4 programs", prog(), dict(scenes=one, n_programs=5)),
        ("1..9 LDS slots", prog(), dict(scenes=one, n_slots=10)),
        ("tile0 must be the prefix sums", prog(), dict(scenes=[dict(q0=0, nq=8), dict(q0=8, nq=12)], tile0=[0, 7] + [0] * 15)),
        ("tile0[n_scenes] != number of tiles", prog(), dict(scenes=one, tile0=[0, tiles + 1] + [0] * 15)),
        ("a scene without query rows", prog(), dict(scenes=[dict(q0=0, nq=0)])),
        ("bad LINEAR", lin(k0=8), dict(scenes=one)),
        ("bad LINEAR", lin(cout=1025), dict(scenes=one)),
        ("bad LINEAR", lin(dst=RC.NONE, flag=RC.F_NO_LDS_DST), dict(scenes=one)),                      # no LDS destination and no global one
        ("bad LOAD", with_op(type=RC.LOAD, dst=1, cout=6, ld=8, p0=x.data_ptr()), dict(scenes=one)),
        ("bad STORE", with_op(type=RC.STORE, src0=2, cout=256, ld=256, p0=view.data_ptr()), dict(scenes=one)),   # a slot past the last
        ("PE / BOX need the scene ranges", with_op(type=RC.PE, dst=1, p0=xyz.data_ptr(), p1=w.data_ptr(), p2=i8.data_ptr()), dict(scenes=one)),
        ("MERGE without its source", with_op(type=RC.MERGE, dst=1, ld=256, p0=0, p1=x.data_ptr()), dict(scenes=[dict(q0=0, nq=n, ksplit=2)])),
        ("BITS2D sizes exceed the LDS areas", with_op(type=RC.BITS2D, p0=bits.data_ptr(), p1=bits.data_ptr()),
         dict(scenes=[dict(q0=0, nq=n, nm=3, nw=8)], nw_max=4, nw2_max=1)),
        ("BITS2D sizes exceed the LDS areas", with_op(type=RC.BITS2D, p0=bits.data_ptr(), p1=bits.data_ptr()),
         dict(scenes=[dict(q0=0, nq=n, nm=33, nw=4)], nw_max=4, nw2_max=1)),
        ("bad ATTN", with_op(type=RC.ATTN, dst=1, src0=0, aux=1, ld=514, p0=x.data_ptr(), p1=x.data_ptr()), dict(scenes=one)),
        ("tile_rows must be 16 (or 0) or 4", prog(), dict(scenes=one, tile_rows=8)),
        ("more than 160 KB of LDS", prog(9), dict(scenes=one, nw_max=300 if tile == 16 else 7000)),
        ("unknown op", with_op(type=17), dict(scenes=one)),
    ]
    if tile == 16:
        cases += [("bad LINEAR", lin(k0=24), dict(scenes=one)),                                       # 16-row tiles: multiples of 16 channels
                  ("bad ATTN", with_op(n_slots=9, type=RC.ATTN, dst=1, src0=0, aux=8, ld=256, p0=x.data_ptr(), p1=x.data_ptr()), dict(scenes=one))]
    for msg, P, kw in cases:
        P.store(0, view)                                        # what a launch would have written
        kw = dict(kw)
        rc, text = raw_launch(P, kw.pop("scenes"), **kw)
        assert rc == ERR_ARG and msg in text, (msg, rc, text)
        assert o.untouched(), msg
    for bad in (lambda: RC.Program(2, rows=8), lambda: prog().launch([dict(q0=0, nq=1)] * 17)):
        with pytest.raises(ValueError):
            bad()
    P = prog()
    for _ in range(3):
        P.begin()
    with pytest.raises(ValueError):
        P.begin()
    P = prog()                                                   # and the same program, admitted: the output is written
    P.store(0, view)
    rc, text = raw_launch(P, one)
    assert rc == 0, text
    assert same_bits(rows_of(o, view), x.cpu().contiguous())
