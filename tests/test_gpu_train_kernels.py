"""The sparse U-Net's training kernels - sd3d_pair_out_rows and sd3d_pair_wgrad (`segdino3d_amd/csrc/pair_wgrad.hip`), sd3d_bn_stats_running,
sd3d_bn_apply, sd3d_bn_backward and sd3d_pool_superpoints_backward (`csrc/train.hip`) - called directly through ctypes (so that every
leading dimension can differ from its width and workspaces can be short), and the autograd nodes `SparseConv` / `SparseConvNative`
over them, each against the float64 reference of the same operation in tests/train_kernel_cases.py at the sizes the launch geometry cares
about: offsets of 0 / 1 / 127 / 128 / 129 pairs, fewer tiles than tile ranges, all 16 (32-wide tiles per block) instantiations of the
weight-gradient kernel with ragged last tiles, 255 / 256 / 257 rows and 4 .. 1024 channels in the column reductions, 7 / 8 / 9 voxels
around the eight of a workgroup.

Integer-valued weight gradients, copies, masks and the constant BatchNorm column are compared bit for bit; float weight gradients
against the derived bound of `wgrad_bound`, everything else with `check_float`.  Every output buffer carries 64 sentinel elements
behind its end, padded input columns hold NaN, workspaces start out as garbage.  Every case prints a `[train-kernel-error]` line;
profiles/train_kernel_errors.md holds the table."""
import numpy as np
import pytest
import torch

from tests import train_kernel_cases as K
from tests.train_kernel_cases import check_bound, check_float
from tests.helpers import Out, wide

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_WS = -1, -2
ACCUMULATE, BF16, BIAS = 1, 2, 4


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
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- tables on the device -------------------------------------------------------------------------------------------------------------------
_LISTS = {}


def lists_of(name):
    """(case, PairLists) of a hand-built table, built once."""
    from segdino3d_amd import ops
    if name not in _LISTS:
        c = K.table_case(name)
        _LISTS[name] = (c, ops.pair_lists(up(c["nbr"]), c["n_pairs"]))
    return _LISTS[name]


@pytest.fixture(scope="module")
def tiny_scene():
    """The `same`, `down` and `up` tables of a scene of isolated points, a tight cluster and a line, as training prepares them."""
    from segdino3d_amd.sparse import SceneMaps
    maps = SceneMaps(K.tiny_scene_points().to(_dev()), 0.02, 2)
    maps.prepare(same=[(0, 3), (1, 3)], strides=[0])
    out = {}
    for key, nbr, v_in in ((("same", 0, 3), maps.same(0, 3), maps.n_vox[0]), (("same", 1, 3), maps.same(1, 3), maps.n_vox[1]),
                           (("down", 0), maps.down(0), maps.n_vox[0]), (("up", 0), maps.up(0), maps.n_vox[1])):
        nbr = nbr.cpu()
        out[key[0] + str(key[1])] = dict(name="scene " + " ".join(str(k) for k in key), nbr=nbr, K=nbr.shape[0], M=nbr.shape[1], V_in=int(v_in),
                                         counts=(nbr >= 0).sum(1).tolist(), n_pairs=int((nbr >= 0).sum()), pairs=maps.pairs[key])
    return out


def check_lists(c, pl):
    """The lists are the table: every pair sits in a tile of its offset, `in_idx` holds its input row, the padding is -1."""
    nbr = c["nbr"].numpy()
    pos, in_idx = pl.pos.cpu().numpy(), pl.in_idx.cpu().numpy()
    tile_k = pl.tile_k.cpu().numpy()
    n_tiles = pl.p_cap // 128
    n_real = int(tile_k[n_tiles])
    assert n_real == K.tile_counts(c["counts"])[0] and n_tiles >= n_real
    assert ((pos >= 0) == (nbr >= 0)).all()
    k, r = np.nonzero(nbr >= 0)
    p = pos[k, r]
    assert len(np.unique(p)) == len(p) and p.max(initial=-1) < n_real * 128
    assert (tile_k[p // 128] == k).all() and (in_idx[p] == nbr[k, r]).all()
    rest = np.ones(n_real * 128, dtype=bool)
    rest[p] = False
    assert (in_idx[: n_real * 128][rest] < 0).all()


# ---- sd3d_pair_out_rows -------------------------------------------------------------------------------------------------------------------
def device_out_rows(pl):
    L, lib = _lib()
    out = Out(pl.p_cap, torch.int32)
    rc = lib.sd3d_pair_out_rows(pl.pos.data_ptr(), pl.K, pl.M, pl.p_cap, out.ptr, _stream())
    torch.cuda.synchronize()
    L.check(rc, "pair_out_rows")
    return out.get(pl.p_cap)


@pytest.mark.parametrize("name", list(K.TABLES))
def test_pair_out_rows(name):
    from segdino3d_amd import train_ops
    c, pl = lists_of(name)
    check_lists(c, pl)
    got = device_out_rows(pl)
    want = K.out_rows_ref(pl.pos.cpu().numpy(), pl.p_cap)
    assert np.array_equal(got.numpy(), want)                     # out_idx[pos[k][r]] = r, -1 everywhere else, the capacity tail included
    assert int((want >= 0).sum()) == c["n_pairs"]
    assert c["dead"] is None or not (want == c["dead"]).any()
    assert np.array_equal(train_ops.pair_out_rows(pl).cpu().numpy(), want)
    assert np.array_equal(device_out_rows(pl).numpy(), want)    # a second call: the same list


def test_pair_out_rows_of_scene_tables(tiny_scene):
    from segdino3d_amd import train_ops
    for key, c in tiny_scene.items():
        pl = c["pairs"]
        check_lists(c, pl)
        want = K.out_rows_ref(pl.pos.cpu().numpy(), pl.p_cap)
        n_real = int(pl.tile_k[pl.p_cap // 128])
        if pl.out_idx is not None:                              # a one-pair-per-row table comes with its list: the same one over the real tiles
            assert np.array_equal(pl.out_idx.cpu().numpy()[: n_real * 128], want[: n_real * 128]), key
        assert np.array_equal(device_out_rows(pl).numpy(), want), key
        assert np.array_equal(train_ops.pair_out_rows(pl).cpu().numpy()[: n_real * 128], want[: n_real * 128]), key


# ---- sd3d_pair_wgrad ----------------------------------------------------------------------------------------------------------------------
def out_rows(pl):
    from segdino3d_amd import train_ops
    return train_ops.pair_out_rows(pl)


def device_wgrad(pl, dy, x, flags=0, old=None, pads=(4, 8), ws_short=0, Cin=None, p_cap=None, swap=False, stale=True):
    """-> (rc, dw Out [K * Cout * Cin (+ Cout with BIAS)], ws Out).  old: the buffer's content before the call (accumulate).
    swap: the operands and their index lists exchanged (what `pair_wgrad_native` launches).
    stale: the workspace starts out as the worst a previous launch can leave behind - every entry of the slot table (the launch's
    ranges + K int32 at its front, padded to 256 bytes) names a valid offset, every partial block behind it is NaN: a slot the kernel
    neither fills nor marks empty puts NaN into the gradient.  Otherwise it holds the fill of `Out`."""
    L, lib = _lib()
    Cout, Cin_ = dy.shape[1], x.shape[1] if Cin is None else Cin
    a, ld_a = wide(dy, pads[0])
    b, ld_b = wide(x, pads[1])
    n = pl.K * Cout * x.shape[1] + (Cout if flags & BIAS else 0)
    dw = Out(n)
    if old is not None:
        dw.buf[:n] = old.reshape(-1).to(_dev())
    ws_bytes = lib.sd3d_pair_wgrad_ws_bytes(pl.K, Cout, Cin_) if swap else lib.sd3d_pair_wgrad_ws_bytes(pl.K, Cin_, Cout)
    ws = Out(ws_bytes, torch.uint8)
    if stale:
        table = (K.wgrad_ranges(pl.K, Cin_, Cout, pl.p_cap) + pl.K + 63) // 64 * 64
        words = ws.buf[:ws_bytes].view(torch.int32)
        words[:table] = torch.arange(table, dtype=torch.int32, device=_dev()) % pl.K
        words[table:] = 0x7FC00000
    oi, ii = out_rows(pl), pl.in_idx
    if swap:
        rc = lib.sd3d_pair_wgrad(b.data_ptr(), ld_b, a.data_ptr(), ld_a, oi.data_ptr(), ii.data_ptr(), pl.tile_k.data_ptr(), pl.p_cap, pl.K, Cout, Cin_,
                                 dw.ptr, flags, ws.ptr, ws_bytes - ws_short, _stream())
    else:
        rc = lib.sd3d_pair_wgrad(a.data_ptr(), ld_a, b.data_ptr(), ld_b, ii.data_ptr(), oi.data_ptr(), pl.tile_k.data_ptr(),
                                 pl.p_cap if p_cap is None else p_cap, pl.K, Cin_, Cout, dw.ptr, flags, ws.ptr, ws_bytes - ws_short, _stream())
    torch.cuda.synchronize()
    return rc, dw, ws


def run_wgrad(c, pl, Cout, Cin, kind, flags=0, seed=0):
    """One case, twice: kind "int" / "ones" (bit-exact against float64) or "float" (the derived bound); -> dw [K, Cout, Cin] (CPU)."""
    L, lib = _lib()
    Kk = c["K"]
    dy, x = (K.float_operands if kind == "float" else K.int_operands)(c["M"], c["V_in"], Cout, Cin, seed, **(dict(ones=True) if kind == "ones" else {}))
    old = None
    if flags & ACCUMULATE:
        g = K.gen(107, Kk, Cout, Cin)
        old = torch.randint(-50, 51, (Kk, Cout, Cin), generator=g).float() if kind != "float" else torch.randn(Kk, Cout, Cin, generator=g)
    got = []
    for _ in range(2):
        rc, dw, ws = device_wgrad(pl, dy, x, flags, old)
        L.check(rc, "pair_wgrad")
        ws.get(ws.n)                                            # the workspace was not overrun
        got.append(dw.get(Kk, Cout, Cin))
    assert same_bits(got[0], got[1]), "second call differs"
    r64, mag = K.wgrad_ref(d64(dy), d64(x), c["nbr"], bf16=bool(flags & BF16))
    want = r64 if old is None else r64 + d64(old)
    name = f"{c['name']} Cout{Cout} Cin{Cin} {kind} flags={flags}"
    empty = [k for k, n in enumerate(c["counts"]) if n == 0]
    for k in empty:                                             # no pairs: exact zeros, or the old block as it was
        assert same_bits(got[0][k], torch.zeros(Cout, Cin) if old is None else old[k]), (name, k)
    if kind == "float":
        n_slots = K.wgrad_ranges(Kk, Cin, Cout, pl.p_cap) + Kk
        check_bound("pair_wgrad", name, got[0], want, K.wgrad_bound(mag, c["counts"], n_slots, old))
    else:
        if kind == "ones":
            assert torch.equal(r64[:, 0, 0], torch.tensor(c["counts"], dtype=torch.float64))
        assert float(mag.max()) + 50 < 2 ** 24
        bad = int((got[0].double() != want).sum())
        K.record(f"pair_wgrad | {name} | exact | entries off {bad} of {want.numel()}")
        assert torch.equal(got[0].double(), want), (name, bad)
    return got[0]


@pytest.mark.parametrize("Cout,Cin", K.CHANNEL_PAIRS, ids=[f"{a}x{b}" for a, b in K.CHANNEL_PAIRS])
def test_wgrad_every_instantiation(Cout, Cin):
    """Every channel pair on the table with the planted small offsets and on one more (in turn)."""
    names = list(K.TABLES)
    other = names[(K.CHANNEL_PAIRS.index((Cout, Cin))) % len(names)]
    for name in dict.fromkeys(["k27_m40", other]):
        c, pl = lists_of(name)
        for kind in ("int", "ones", "float"):
            run_wgrad(c, pl, Cout, Cin, kind)


TABLE_CHANNELS = {"k1_m1": [(4, 4), (100, 36), (260, 160)], "k1_m5": [(36, 4), (68, 100)], "k1_m130": [(4, 68), (128, 128), (36, 36)],
                  "k3_m150": [(68, 36), (160, 260), (4, 100)], "k27_m40": [(96, 128)], "k27_m600": [(36, 68), (100, 100), (260, 160), (4, 4)],
                  "k125_m20": [(68, 68), (4, 36), (128, 96)]}


@pytest.mark.parametrize("name", list(K.TABLES))
def test_wgrad_every_table(name):
    """Every table with a few channel pairs, plain and with each flag."""
    c, pl = lists_of(name)
    for i, (Cout, Cin) in enumerate(TABLE_CHANNELS[name]):
        assert (Cout, Cin) in K.CHANNEL_PAIRS
        for kind in ("int", "ones", "float"):
            run_wgrad(c, pl, Cout, Cin, kind, seed=1)
        for kind in ("int", "float"):
            run_wgrad(c, pl, Cout, Cin, kind, flags=ACCUMULATE, seed=2)
            run_wgrad(c, pl, Cout, Cin, kind, flags=BF16, seed=3)
        if i == 0:
            run_wgrad(c, pl, Cout, Cin, "float", flags=ACCUMULATE | BF16, seed=4)


def test_wgrad_scene_tables(tiny_scene):
    for key, c in tiny_scene.items():
        for Cout, Cin in ((36, 68), (128, 96)):
            for kind in ("int", "ones", "float"):
                run_wgrad(c, c["pairs"], Cout, Cin, kind)
            run_wgrad(c, c["pairs"], Cout, Cin, "float", flags=BF16)


def test_wgrad_bf16_rounds_the_operands():
    """Operands that are bf16 values already: the flag changes nothing; operands that are not: it rounds them (carry into the exponent
    included) - the result is the exact gradient of the rounded operands."""
    c, pl = lists_of("k1_m5")
    dy, x = K.float_operands(c["M"], c["V_in"], 4, 4)
    dyr, xr = K.round_bf16(dy), K.round_bf16(x)
    assert float(dyr.view(-1)[0]) == 2.0 and float(xr.view(-1)[0]) == -1.0 and not torch.equal(dyr, dy)
    res = [device_wgrad(pl, a, b, f)[1].get(1, 4, 4) for a, b, f in ((dy, x, BF16), (dyr, xr, BF16), (dyr, xr, 0))]
    assert same_bits(res[0], res[1]) and same_bits(res[1], res[2])


@pytest.mark.parametrize("name", ["k1_m1", "k1_m5", "k1_m130"])
def test_wgrad_bias(name):
    """K = 1 with SD3D_WGRAD_BIAS: (dw, db) out of one launch, db = the column sums of dy as staged (rounded to bf16 with that flag)."""
    from segdino3d_amd import train_ops
    L, lib = _lib()
    c, pl = lists_of(name)
    for Cout, Cin in ((4, 4), (100, 36), (160, 68), (128, 128)):
        for kind, flags in (("int", BIAS), ("float", BIAS), ("float", BIAS | BF16)):
            dy, x = (K.float_operands if kind == "float" else K.int_operands)(c["M"], c["V_in"], Cout, Cin, 5)
            rc, out, ws = device_wgrad(pl, dy, x, flags)
            L.check(rc, "pair_wgrad")
            ws.get(ws.n)
            flat = out.get(Cout * Cin + Cout)
            dw, db = flat[: Cout * Cin].view(1, Cout, Cin), flat[Cout * Cin:]
            r64, mag = K.wgrad_ref(d64(dy), d64(x), c["nbr"], bf16=bool(flags & BF16))
            staged = d64(K.round_bf16(dy) if flags & BF16 else dy)
            rows = (c["nbr"][0] >= 0)
            db64, dbmag = staged[rows].sum(0), staged[rows].abs().sum(0)
            label = f"{name} Cout{Cout} Cin{Cin} {kind} flags={flags}"
            if kind == "int":
                assert torch.equal(dw.double(), r64) and torch.equal(db.double(), db64), label
            else:
                n_slots = K.wgrad_ranges(1, Cin, Cout, pl.p_cap) + 1
                check_bound("pair_wgrad bias dw", label, dw, r64, K.wgrad_bound(mag, c["counts"], n_slots))
                # db: the same chain - the rows of a slot one after the other, then the slots
                check_bound("pair_wgrad bias db", label, db, db64, (c["counts"][0] + n_slots) * K.U * dbmag + K.FLOOR)
            w_dw, w_db = train_ops.pair_wgrad(up(dy), up(x), pl, bias=True, bf16_operands=bool(flags & BF16))
            assert same_bits(w_dw.cpu(), dw) and same_bits(w_db.cpu(), db), label


def test_wgrad_wrappers_and_native_layout():
    """`pair_wgrad` (fresh, accumulate, bf16) gives the bits of the direct call; `pair_wgrad_native` the transposed ones."""
    from segdino3d_amd import train_ops
    L, lib = _lib()
    for name, (Cout, Cin) in (("k27_m600", (36, 100)), ("k3_m150", (160, 68)), ("k125_m20", (4, 36)), ("k1_m130", (128, 96)), ("k27_m40", (68, 4))):
        c, pl = lists_of(name)
        dy, x = K.float_operands(c["M"], c["V_in"], Cout, Cin, 6)
        direct = device_wgrad(pl, dy, x)[1].get(c["K"], Cout, Cin)
        dyd, xd = wide(dy, 12)[0][:, :Cout], wide(x, 4)[0][:, :Cin]     # strided rows through the wrappers too
        assert same_bits(train_ops.pair_wgrad(dyd, xd, pl).cpu(), direct)
        native = train_ops.pair_wgrad_native(dyd, xd, pl)
        assert tuple(native.shape) == (c["K"], Cin, Cout) and native.is_contiguous()
        assert same_bits(native.cpu(), direct.transpose(1, 2).contiguous()), name
        rc, sw, _ = device_wgrad(pl, dy, x, swap=True)
        L.check(rc, "pair_wgrad")
        assert same_bits(sw.get(c["K"], Cin, Cout), native.cpu())
        r64, mag = K.wgrad_ref(d64(dy), d64(x), c["nbr"])
        n_slots = K.wgrad_ranges(c["K"], Cin, Cout, pl.p_cap) + c["K"]
        check_bound("pair_wgrad_native", f"{name} Cout{Cout} Cin{Cin}", native.cpu().transpose(1, 2), r64, K.wgrad_bound(mag, c["counts"], n_slots))
        old = torch.randn(c["K"], Cout, Cin, generator=K.gen(7))
        acc = up(old.clone())
        assert train_ops.pair_wgrad(dyd, xd, pl, dw=acc, accumulate=True) is acc
        assert same_bits(acc.cpu(), device_wgrad(pl, dy, x, ACCUMULATE, old)[1].get(c["K"], Cout, Cin))
        assert same_bits(train_ops.pair_wgrad(dyd, xd, pl, bf16_operands=True).cpu(), device_wgrad(pl, dy, x, BF16)[1].get(c["K"], Cout, Cin))
    with pytest.raises(ValueError):                              # bias is for K = 1
        c, pl = lists_of("k3_m150")
        train_ops.pair_wgrad(up(torch.zeros(c["M"], 4)), up(torch.zeros(c["V_in"], 4)), pl, bias=True)


def test_wgrad_refusals():
    L, lib = _lib()
    c, pl = lists_of("k3_m150")
    dy, x = K.int_operands(c["M"], c["V_in"], 36, 68)
    for kw, want in ((dict(Cin=6), ERR_ARG), (dict(pads=(2, 8)), ERR_ARG), (dict(pads=(4, 6)), ERR_ARG), (dict(p_cap=pl.p_cap - 1), ERR_ARG),
                     (dict(flags=BIAS), ERR_ARG), (dict(ws_short=1), ERR_WS)):
        rc, dw, ws = device_wgrad(pl, dy, x, stale=False, **kw)
        assert rc == want and dw.untouched() and ws.untouched(), kw
    rc, dw, ws = device_wgrad(pl, dy[:, :6].contiguous(), x, stale=False)      # Cout = 6
    assert rc == ERR_ARG and dw.untouched() and ws.untouched()


# ---- the autograd nodes: input gradient, native layout ------------------------------------------------------------------------------------------
def conv_case(c, pairs, pairs_t, mirrored, Cin, Cout, seed=0):
    """SparseConv and SparseConvNative, forward and backward, against float64 autograd of the gather + matmul model."""
    from segdino3d_amd import ops, train_ops
    g = K.gen(109, c["K"], c["M"], Cin, Cout, seed)
    Kk, M, V = c["K"], c["M"], c["V_in"]
    x, w = torch.randn(V, Cin, generator=g), 0.1 * torch.randn(Kk, Cout, Cin, generator=g)
    res, dy = torch.randn(M, Cout, generator=g), torch.randn(M, Cout, generator=g)
    y64, dx64, dw64, dres64 = K.conv_grads(x, w, c["nbr"], dy, res)
    name = f"{c['name']} Cin{Cin} Cout{Cout}"

    xa, wa, ra = (up(t).requires_grad_(True) for t in (x, w, res))
    ya = train_ops.SparseConv.apply(xa, wa, pairs, pairs_t, mirrored, ra)
    ya.backward(up(dy))
    kernel = up(w.transpose(1, 2)).requires_grad_(True)         # the parameter as it lies: [K, Cin, Cout]
    tw = train_ops.transpose_all({"w": kernel})["w"]
    assert same_bits(tw.fwd.cpu(), w)
    xb, rb = (up(t).requires_grad_(True) for t in (x, res))
    yb = train_ops.SparseConvNative.apply(xb, kernel, tw.fwd, pairs, pairs_t, mirrored, rb)
    yb.backward(up(dy))
    errs = []
    for label, got, ref in (("y", ya.detach(), y64), ("dx", xa.grad, dx64)):
        e = K.row_error(got.cpu(), ref)
        errs.append(e)
        K.record(f"sparse_conv {label} | {name} | row error {e:.3e} | bound {K.ROW_TOL:.1e}")
    assert max(errs) < K.ROW_TOL, (name, errs)
    _, mag = K.wgrad_ref(d64(dy), d64(x), c["nbr"])
    n_slots = K.wgrad_ranges(Kk, Cin, Cout, pairs.p_cap) + Kk
    check_bound("sparse_conv dw", name, wa.grad.cpu(), dw64, K.wgrad_bound(mag, c["counts"], n_slots))
    assert same_bits(ra.grad.cpu(), dy) and same_bits(rb.grad.cpu(), dy) and torch.equal(dres64, d64(dy))      # the residual's gradient passes through
    # the native-layout node: the same bits on permuted copies
    assert same_bits(yb.detach().cpu(), ya.detach().cpu()) and same_bits(xb.grad.cpu(), xa.grad.cpu()), name
    assert tuple(kernel.grad.shape) == (Kk, Cin, Cout) and same_bits(kernel.grad.cpu(), wa.grad.cpu().transpose(1, 2).contiguous()), name
    if mirrored:                                                # the input gradient on the parameter as it lies
        dyd = up(dy)
        assert same_bits(ops.pair_conv(dyd, kernel.detach(), pairs_t, mirror_w=True).cpu(),
                         ops.pair_conv(dyd, train_ops.transposed_weights(up(w), True), pairs_t).cpu()), name
        assert same_bits(ops.pair_conv(dyd, kernel.detach(), pairs_t, mirror_w=True).cpu(), xb.grad.cpu()), name


def conv_case_padded(c, pairs, pairs_t, mirrored, cin, pad, Cout):
    """The stem's case: cin input channels zero-padded to `pad` in x and in the forward copy, no input gradient; the parameter keeps cin."""
    from segdino3d_amd import train_ops
    g = K.gen(113, c["K"], c["M"], cin, Cout)
    Kk, M, V = c["K"], c["M"], c["V_in"]
    x, w, dy = torch.randn(V, cin, generator=g), 0.1 * torch.randn(Kk, Cout, cin, generator=g), torch.randn(M, Cout, generator=g)
    xp, wp = torch.zeros(V, pad), torch.zeros(Kk, Cout, pad)
    xp[:, :cin], wp[:, :, :cin] = x, w
    y64, _, dw64, _ = K.conv_grads(x, w, c["nbr"], dy)
    wa = up(wp).requires_grad_(True)
    ya = train_ops.SparseConv.apply(up(xp), wa, pairs, pairs_t, mirrored)
    ya.backward(up(dy))
    kernel = up(w.transpose(1, 2)).requires_grad_(True)
    tw = train_ops.transpose_all({"w": kernel}, pad_cin={"w": pad})["w"]
    assert tw.pad_cin == pad and same_bits(tw.fwd.cpu(), wp)    # zero-padded forward copy
    yb = train_ops.SparseConvNative.apply(up(xp), kernel, tw.fwd, pairs, pairs_t, mirrored, None)
    yb.backward(up(dy))
    name = f"{c['name']} cin{cin} pad{pad} Cout{Cout}"
    e = K.row_error(ya.detach().cpu(), y64)
    K.record(f"sparse_conv y | {name} | row error {e:.3e} | bound {K.ROW_TOL:.1e}")
    assert e < K.ROW_TOL
    assert same_bits(yb.detach().cpu(), ya.detach().cpu())
    assert tuple(kernel.grad.shape) == (Kk, cin, Cout)
    assert same_bits(kernel.grad.cpu(), wa.grad.cpu()[:, :, :cin].transpose(1, 2).contiguous()), name
    assert same_bits(wa.grad.cpu()[:, :, cin:], torch.zeros(Kk, Cout, pad - cin))
    _, mag = K.wgrad_ref(d64(dy), d64(x), c["nbr"])
    n_slots = K.wgrad_ranges(Kk, pad, Cout, pairs.p_cap) + Kk
    check_bound("sparse_conv_native dk", name, kernel.grad.cpu().transpose(1, 2), dw64, K.wgrad_bound(mag, c["counts"], n_slots))


def _as_case(name, nbr, V_in):
    return dict(name=name, nbr=nbr, K=nbr.shape[0], M=nbr.shape[1], V_in=V_in, counts=(nbr >= 0).sum(1).tolist(), n_pairs=int((nbr >= 0).sum()))


@pytest.mark.parametrize("Kk,M", [(3, 7), (27, 61), (27, 300)])
def test_conv_nodes_on_symmetric_tables(Kk, M):
    from segdino3d_amd import ops
    c = _as_case(f"symmetric K{Kk} M{M}", K.symmetric_table(Kk, M), M)
    pl = ops.pair_lists(up(c["nbr"]), c["n_pairs"])
    conv_case(c, pl, pl, True, 32, 64)
    conv_case(c, pl, pl, True, 96, 32, seed=1)
    conv_case_padded(c, pl, pl, True, 36, 64, 32)


def test_conv_nodes_on_a_stride_pair():
    from segdino3d_amd import ops
    down, up_, Mf = K.stride_tables(37)
    cd, cu = _as_case("down Mc37", down, Mf), _as_case("up Mc37", up_, 37)
    pd, pu = ops.pair_lists(up(down), Mf), ops.pair_lists(up(up_), Mf, direct=True)
    conv_case(cd, pd, pu, False, 32, 64)
    conv_case(cu, pu, pd, False, 64, 32)
    conv_case_padded(cd, pd, pu, False, 4, 32, 36)


def test_conv_nodes_on_the_scene(tiny_scene):
    from segdino3d_amd import train_ops
    s, d, u = tiny_scene["same0"], tiny_scene["down0"], tiny_scene["up0"]
    conv_case(s, s["pairs"], s["pairs"], True, 32, 32)
    conv_case(tiny_scene["same1"], tiny_scene["same1"]["pairs"], tiny_scene["same1"]["pairs"], True, 64, 32)
    conv_case(d, d["pairs"], u["pairs"], False, 32, 64)
    conv_case(u, u["pairs"], d["pairs"], False, 64, 32)


# ---- BatchNorm --------------------------------------------------------------------------------------------------------------------------------
def device_bn_stats(c, running=True, momentum=K.MOMENTA[0], pad=4, C=None, ws_short=0, tracked=41, ws_off=0):
    """-> (rc, mean, var, rstd Outs, (running mean, running var, num_batches_tracked) device tensors or None, ws Out)."""
    L, lib = _lib()
    M, C = c["M"], c["C"] if C is None else C
    x, ld = wide(c["x"], pad)
    mean, var, rstd = Out(c["C"]), Out(c["C"]), Out(c["C"])
    ws_bytes = lib.sd3d_bn_ws_bytes(M, C)
    ws = Out(ws_bytes, torch.uint8)
    run = (up(c["run_mean"]).clone(), up(c["run_var"]).clone(), torch.tensor([tracked], dtype=torch.int64, device=_dev())) if running else None
    rc = lib.sd3d_bn_stats_running(x.data_ptr(), ld, M, C, K.EPS, mean.ptr, var.ptr, rstd.ptr, *([ptr(t) for t in run] if running else [None] * 3),
                                   momentum, ws.ptr + ws_off, ws_bytes - ws_short, _stream())
    torch.cuda.synchronize()
    return rc, mean, var, rstd, run, ws


@pytest.mark.parametrize("C", K.BN_C)
def test_bn_stats(C):
    """Batch and running statistics.  With fp32 partial sums (the kernels before these tests) the column whose first row is an outlier
    missed the rule at 255 - 513 rows: var 4.3e-5 off at M255 C4 (cap 2.3e-5), rstd 6.1e-6 of its value at M255 C12 and 3.9e-6 at
    M256 C256 (bound 9.5e-7) - the variance is E[d^2] - E[d]^2 around row 0, 65 times the variance there.  The sums are doubles now."""
    L, lib = _lib()
    for M in K.BN_M:
        c = K.bn_case(M, C)
        r64, r32 = K.bn_stats_ref(d64(c["x"])), K.bn_stats_ref(c["x"])
        scales = K.bn_stats_scale(c["x"])
        name = f"M{M} C{C}"
        outs = {}
        for mom in K.MOMENTA:
            rc, mean, var, rstd, run, ws = device_bn_stats(c, True, mom)
            L.check(rc, "bn_stats")
            ws.get(ws.n)
            got = [o.get(C) for o in (mean, var, rstd)]
            outs[mom] = got
            if mom == K.MOMENTA[0]:
                for label, g_, a, b, sc in zip(("mean", "var", "rstd"), got, r64, r32, scales):
                    check_float(f"bn_stats {label}", name, g_, a, b, sc)
                # the constant column: variance exactly 0, rstd = 1 / sqrt(eps); the big column's mean is exact
                assert float(got[0][K.COL_CONST]) == 1.75 and float(got[1][K.COL_CONST]) == 0.0
                assert float(got[2][K.COL_CONST]) == float(np.float32(1.0 / np.sqrt(np.float64(K.EPS))))
                if M >= 2:
                    assert float(got[0][K.COL_BIG]) == 1000.0
                if M == 1:
                    assert torch.equal(got[0], c["x"][0]) and bool((got[1] == 0).all())
            # running statistics from the batch statistics the kernel made (their own error is checked above)
            m_, v_ = got[0], got[1]
            a = K.bn_running_ref(d64(c["run_mean"]), d64(c["run_var"]), d64(m_), d64(v_), M, mom)
            b = K.bn_running_ref(c["run_mean"], c["run_var"], m_, v_, M, mom)
            unb = M / max(M - 1, 1)
            check_float("bn_stats running_mean", f"{name} momentum {mom:.2f}", run[0].cpu(), a[0], b[0], torch.maximum(c["run_mean"].abs(), m_.abs()))
            check_float("bn_stats running_var", f"{name} momentum {mom:.2f}", run[1].cpu(), a[1], b[1], torch.maximum(c["run_var"].abs(), v_ * unb))
            if mom == 1.0:                                      # the batch statistics themselves (the variance unbiased)
                assert same_bits(run[0].cpu(), m_)
                if M == 1:
                    assert same_bits(run[1].cpu(), v_)
            assert run[2].tolist() == [42]                      # num_batches_tracked: + 1 per call
        assert all(same_bits(a, b) for a, b in zip(outs[K.MOMENTA[0]], outs[1.0]))
        rc, mean, var, rstd, _, ws = device_bn_stats(c, False)   # without the running statistics: the same batch statistics
        L.check(rc, "bn_stats")
        assert all(same_bits(o.get(C), b) for o, b in zip((mean, var, rstd), outs[1.0]))


def test_bn_stats_wide_counter_and_refusals():
    L, lib = _lib()
    c = K.bn_case(257, 12)
    rc, mean, var, rstd, run, ws = device_bn_stats(c, True, tracked=2 ** 40)
    assert rc == 0 and run[2].tolist() == [2 ** 40 + 1]
    for kw, want in ((dict(C=6), ERR_ARG), (dict(C=1028), ERR_ARG), (dict(pad=2), ERR_ARG), (dict(ws_short=1), ERR_WS),
                     (dict(ws_off=4), ERR_ARG)):                # (the partial sums are doubles: a workspace at an odd multiple of 4 bytes)
        rc, mean, var, rstd, run, ws = device_bn_stats(c, True, **kw)
        assert rc == want and mean.untouched() and var.untouched() and rstd.untouched() and ws.untouched(), kw
        assert same_bits(run[0].cpu(), c["run_mean"]) and same_bits(run[1].cpu(), c["run_var"]) and run[2].tolist() == [41], kw


def fp32_stats(c):
    """(mean, rstd) the apply / backward kernels are handed: the float64 statistics rounded to fp32."""
    mean, _, rstd = K.bn_stats_ref(d64(c["x"]))
    return mean.float(), rstd.float()


def device_bn_apply(c, mean, rstd, with_res, act, pads=(4, 8, 12), C=None, M=None):
    L, lib = _lib()
    M, C = c["M"] if M is None else M, c["C"] if C is None else C
    x, ld_x = wide(c["x"], pads[0])
    res, ld_res = wide(c["res"], pads[1]) if with_res else (None, 0)
    ld_y = c["C"] + pads[2]
    y = Out(c["M"] * ld_y)
    mu, rs, ga, be = up(mean), up(rstd), up(c["gamma"]), up(c["beta"])
    rc = lib.sd3d_bn_apply(x.data_ptr(), ld_x, mu.data_ptr(), rs.data_ptr(), ga.data_ptr(), be.data_ptr(), ptr(res), ld_res, M, C, act, y.ptr, ld_y,
                           _stream())
    torch.cuda.synchronize()
    return rc, y, ld_y


@pytest.mark.parametrize("C", K.BN_C)
def test_bn_apply(C):
    L, lib = _lib()
    for M in K.BN_M:
        c = K.bn_case(M, C)
        mean, rstd = fp32_stats(c)
        for with_res in (False, True):
            res = c["res"] if with_res else None
            scale = K.bn_apply_scale(c["x"], mean, rstd, c["gamma"], c["beta"], res)
            for relu in (False, True):
                rc, y, ld_y = device_bn_apply(c, mean, rstd, with_res, int(relu))
                L.check(rc, "bn_apply")
                got = rows_of(y, M, ld_y, C)
                r64, z64 = K.bn_apply_ref(d64(c["x"]), d64(mean), d64(rstd), d64(c["gamma"]), d64(c["beta"]), d64(res), relu)
                r32, _ = K.bn_apply_ref(c["x"], mean, rstd, c["gamma"], c["beta"], res, relu)
                _, _, bound = check_float("bn_apply", f"M{M} C{C} res={int(with_res)} relu={int(relu)}", got, r64, r32, scale)
                want = c["beta"][K.COL_CONST] + (res[:, K.COL_CONST] if with_res else torch.zeros(M))      # the constant column: beta (+ res), exactly
                assert same_bits(got[:, K.COL_CONST], torch.relu(want) if relu else want)
                if relu:                                        # the mask differs from the float64 one only where the pre-activation is inside the bound
                    assert float(got.min()) >= 0.0
                    flipped = (got > 0) != (z64 > 0)
                    assert bool((z64.abs()[flipped] <= bound * scale[flipped] + K.FLOOR).all())


def test_bn_apply_refusals_and_no_rows():
    c = K.bn_case(257, 12)
    mean, rstd = fp32_stats(c)
    for kw in (dict(C=6), dict(pads=(2, 8, 12)), dict(pads=(4, 6, 12)), dict(pads=(4, 8, 2)), dict(act=2)):
        rc, y, _ = device_bn_apply(c, mean, rstd, True, kw.pop("act", 1), **kw)
        assert rc == ERR_ARG and y.untouched(), kw
    rc, y, _ = device_bn_apply(c, mean, rstd, True, 1, M=0)      # no rows: nothing happens
    assert rc == 0 and y.untouched()


def device_bn_backward(c, y, mean, rstd, with_res, act=None, pads=(4, 8, 12, 16, 20), C=None, ws_short=0, null_y=False, ws_off=0):
    """-> (rc, dx Out, ld_dx, dres Out or None, ld_dres, dgamma Out, dbeta Out, ws Out); y None: no ReLU."""
    L, lib = _lib()
    M, C = c["M"], c["C"] if C is None else C
    dy, ld_dy = wide(c["dy"], pads[0])
    yy, ld_y = wide(y, pads[1]) if (y is not None and not null_y) else (None, 0)
    x, ld_x = wide(c["x"], pads[2])
    ld_dx, ld_dres = c["C"] + pads[3], c["C"] + pads[4]
    dx, dres = Out(M * ld_dx), Out(M * ld_dres) if with_res else None
    dgamma, dbeta = Out(c["C"]), Out(c["C"])
    ws_bytes = lib.sd3d_bn_ws_bytes(M, C)
    ws = Out(ws_bytes, torch.uint8)
    act = (0 if y is None else 1) if act is None else act
    mu, rs, ga = up(mean), up(rstd), up(c["gamma"])
    rc = lib.sd3d_bn_backward(dy.data_ptr(), ld_dy, ptr(yy), ld_y, x.data_ptr(), ld_x, mu.data_ptr(), rs.data_ptr(), ga.data_ptr(), M, C, act, dx.ptr, ld_dx, None if dres is None else dres.ptr, ld_dres, dgamma.ptr, dbeta.ptr, ws.ptr + ws_off,
                              ws_bytes - ws_short, _stream())
    torch.cuda.synchronize()
    return rc, dx, ld_dx, dres, ld_dres, dgamma, dbeta, ws


@pytest.mark.parametrize("C", K.BN_C)
def test_bn_backward(C):
    L, lib = _lib()
    for M in K.BN_M:
        c = K.bn_case(M, C)
        mean, rstd = fp32_stats(c)
        for relu, with_res in ((False, False), (True, True), (True, False), (False, True)):
            y = None
            if relu:                                            # the mask comes from the device's own forward output
                rc, yo, ld_y = device_bn_apply(c, mean, rstd, with_res, 1)
                L.check(rc, "bn_apply")
                y = rows_of(yo, M, ld_y, C)
            outs = []
            for _ in range(2 if relu and with_res else 1):
                rc, dx, ld_dx, dres, ld_dres, dgamma, dbeta, ws = device_bn_backward(c, y, mean, rstd, with_res)
                L.check(rc, "bn_backward")
                ws.get(ws.n)
                outs.append((dx.buf.clone(), dgamma.buf.clone(), dbeta.buf.clone()))
            assert all(same_bits(a, b) for a, b in zip(outs[0], outs[-1])), "second call differs"
            r64 = K.bn_backward_ref(d64(c["dy"]), d64(y), d64(c["x"]), d64(mean), d64(rstd), d64(c["gamma"]))
            r32 = K.bn_backward_ref(c["dy"], y, c["x"], mean, rstd, c["gamma"])
            sdx, sdg, sdb = K.bn_backward_scale(c["dy"], y, c["x"], mean, rstd, c["gamma"])
            name = f"M{M} C{C} res={int(with_res)} relu={int(relu)}"
            check_float("bn_backward dx", name, rows_of(dx, M, ld_dx, C), r64[0], r32[0], sdx)
            check_float("bn_backward dgamma", name, dgamma.get(C), r64[2], r32[2], sdg)
            check_float("bn_backward dbeta", name, dbeta.get(C), r64[3], r32[3], sdb)
            if with_res:                                        # dres = the masked dy, a copy
                assert same_bits(rows_of(dres, M, ld_dres, C), r32[1])


def test_bn_backward_refusals():
    c = K.bn_case(257, 12)
    mean, rstd = fp32_stats(c)
    y = torch.relu(c["res"])
    for kw, want in ((dict(C=6), ERR_ARG), (dict(C=1028), ERR_ARG), (dict(pads=(2, 8, 12, 16, 20)), ERR_ARG), (dict(pads=(4, 8, 2, 16, 20)), ERR_ARG),
                     (dict(pads=(4, 8, 12, 2, 20)), ERR_ARG), (dict(pads=(4, 8, 12, 16, 2)), ERR_ARG), (dict(pads=(4, 2, 12, 16, 20)), ERR_ARG),
                     (dict(act=2), ERR_ARG), (dict(null_y=True), ERR_ARG), (dict(ws_short=1), ERR_WS), (dict(ws_off=4), ERR_ARG)):
        rc, dx, _, dres, _, dgamma, dbeta, ws = device_bn_backward(c, y, mean, rstd, True, **kw)
        assert rc == want and all(o.untouched() for o in (dx, dres, dgamma, dbeta, ws)), kw


# ---- sd3d_pool_superpoints_backward -----------------------------------------------------------------------------------------------------------
def device_pool_backward(c, dout, C=None, pad=4, V=None):
    L, lib = _lib()
    V, C = c["V"] if V is None else V, dout.shape[1] if C is None else C
    ld = dout.shape[1] + pad
    dfeat = Out(c["V"] * ld)
    sp, sidx = up(c["superpoints"]), up(c["sidx"].to(torch.int32))          # (uint32 on the device: the ids are below 2^31)
    seg, sps = up(c["seg_start"]), up(c["sp_start"])
    do = up(dout)
    rc = lib.sd3d_pool_superpoints_backward(do.data_ptr(), C, sp.data_ptr(), sidx.data_ptr(), seg.data_ptr(), sps.data_ptr(), V, dfeat.ptr, ld,
                                            _stream())
    torch.cuda.synchronize()
    return rc, dfeat, ld


@pytest.mark.parametrize("V", K.POOL_V)
def test_pool_superpoints_backward(V):
    L, lib = _lib()
    for C in K.POOL_C:
        for pow2 in (False, True):
            c = K.pool_case(V, pow2)
            dout = K.pool_dout(c["S"], C, seed=V)
            rc, dfeat, ld = device_pool_backward(c, dout)
            L.check(rc, "pool_superpoints_backward")
            got = rows_of(dfeat, V, ld, C)
            r64, top = K.pool_backward_ref(d64(dout), c)
            r32, _ = K.pool_backward_ref(dout, c)
            check_float("pool_backward", f"V{V} C{C} pow2={int(pow2)}", got, r64, r32, top)
            rc, again, _ = device_pool_backward(c, dout)
            assert same_bits(again.buf, dfeat.buf), "second call differs"
            if pow2:                                            # integer gradients over power-of-two superpoints: exact
                di = K.pool_dout(c["S"], C, seed=V, integer=True)
                rc, dfeat, ld = device_pool_backward(c, di)
                L.check(rc, "pool_superpoints_backward")
                assert torch.equal(rows_of(dfeat, V, ld, C).double(), K.pool_backward_ref(d64(di), c)[0]), (V, C)


def test_pool_superpoints_backward_refusals_and_no_voxels():
    c = K.pool_case(9)
    for kw in (dict(C=132), dict(C=6), dict(pad=2)):
        rc, dfeat, _ = device_pool_backward(c, K.pool_dout(c["S"], 136), **kw)
        assert rc == ERR_ARG and dfeat.untouched(), kw
    rc, dfeat, _ = device_pool_backward(c, K.pool_dout(c["S"], 32), V=0)
    assert rc == 0 and dfeat.untouched()


# ---- chained and lean lists are refused by the host wrappers -------------------------------------------------------------------------------------
def test_wrappers_refuse_chained_and_lean_lists_on_the_device():
    from segdino3d_amd import ops, train_ops
    nbr = up(K.symmetric_table(27, 61))
    P = int((nbr >= 0).sum())
    chained = ops.pair_lists(nbr, P, center=ops.PAIR_CHAINED)
    lean = ops.pair_lists_batch([(nbr, P, -1, False, True)])[0]
    assert chained.pos.numel() == 0 and lean.pos is None and chained.out_idx is None and lean.out_idx is None
    dy, x = up(torch.ones(61, 4)), up(torch.ones(61, 4))
    for pairs in (chained, lean):
        for call in (lambda: train_ops.pair_out_rows(pairs), lambda: train_ops.pair_wgrad(dy, x, pairs), lambda: train_ops.pair_wgrad_native(dy, x, pairs)):
            with pytest.raises(ValueError):
                call()
        assert pairs.out_idx is None
    torch.cuda.synchronize()
