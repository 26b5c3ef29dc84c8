"""tests/train_kernel_cases.py on the CPU: every float64 reference equals float64 autograd of an independent formulation (an explicit
loop over the pairs, torch's own batch_norm, the pooled mean), the planted situations are present, the channel list reaches all 16
instantiations of the weight-gradient kernel, the fp32 evaluation of each reference passes its tolerance rule by itself, and the host
wrappers refuse lists they cannot serve before they touch a device."""
import pytest
import torch
import torch.nn.functional as F

from tests import train_kernel_cases as K

F64 = torch.float64


def d64(t):
    return None if t is None else t.double()


def close(a, b, tol=1e-12):
    scale = max(1.0, float(b.abs().max())) if b.numel() else 1.0
    assert a.shape == b.shape and float((a - b).abs().max() if b.numel() else 0.0) <= tol * scale, float((a - b).abs().max())


# ---- tables -------------------------------------------------------------------------------------------------------------------------------
def test_tables_hold_the_planted_counts():
    seen = set()
    for name in K.TABLES:
        c = K.table_case(name)
        nbr = c["nbr"]
        assert nbr.dtype == torch.int32 and tuple(nbr.shape) == (c["K"], c["M"])
        assert (nbr >= 0).sum(1).tolist() == c["counts"] and c["n_pairs"] == int((nbr >= 0).sum())
        assert int(nbr.max()) < c["V_in"] and int(nbr.min()) >= -1
        seen |= set(c["counts"])
        real, cap = K.tile_counts(c["counts"])
        assert real <= cap and (real < cap or c["K"] == 1), (name, real, cap)      # K >= 3: fewer real tiles than the capacity has - empty ranges
        if c["dead"] is not None:
            assert bool((nbr[:, c["dead"]] < 0).all())          # an output row no pair writes
        if c["n_pairs"] >= 20 and c["V_in"] > 1:
            assert int((nbr == K.HOT).sum()) >= c["n_pairs"] // 5   # an input row many pairs read
    assert {0, 1, 127, 128, 129} <= seen
    assert sorted({K.TABLES[n][0] for n in K.TABLES}) == [1, 3, 27, 125]
    assert [K.TABLES[n][1] for n in K.TABLES if K.TABLES[n][0] == 1] == [1, 5, 130]
    assert K.tile_counts(K.table_case("k1_m1")["counts"]) == (1, 1)


def test_symmetric_and_stride_tables():
    for Kk, M in ((3, 7), (27, 61)):
        nbr = K.symmetric_table(Kk, M)
        assert torch.equal(nbr[Kk // 2], torch.arange(M, dtype=torch.int32))
        for k in range(Kk):
            r = (nbr[k] >= 0).nonzero(as_tuple=True)[0]
            assert r.numel() >= 1 and torch.equal(nbr[Kk - 1 - k][nbr[k][r].long()].long(), r)
        assert int((nbr >= 0).sum()) > M
    down, up, Mf = K.stride_tables(37)
    assert tuple(up.shape) == (8, Mf) and bool(((up >= 0).sum(0) == 1).all()) and bool(((down >= 0).sum(0) >= 1).all())
    for k in range(8):
        p = (down[k] >= 0).nonzero(as_tuple=True)[0]
        assert torch.equal(up[k][down[k][p].long()].long(), p)
    assert int((down >= 0).sum()) == Mf == int((up >= 0).sum())


def test_channel_pairs_reach_all_sixteen_instantiations():
    assert set(c for pair in K.CHANNEL_PAIRS for c in pair) <= set(K.CHANNELS)
    assert {c: K.sub_tiles(c) for c in K.CHANNELS} == {4: 1, 36: 2, 68: 3, 96: 3, 100: 4, 128: 4, 160: 3, 260: 3}
    hit = {(K.sub_tiles(co), K.sub_tiles(ci)) for co, ci in K.CHANNEL_PAIRS}
    assert hit == {(a, b) for a in range(1, 5) for b in range(1, 5)}
    # the instantiations whose waves multiply into accumulators they never flush (tiles no multiple of the waves)
    idle = {(a, b) for a, b in hit if (a * b) % K.wgrad_waves(a, b)}
    assert idle == {(1, 1), (1, 2), (1, 3), (2, 1), (2, 3), (3, 1), (3, 2)}
    assert any(c % 32 for pair in K.CHANNEL_PAIRS for c in pair) and (160, 260) in K.CHANNEL_PAIRS      # ragged last tiles, several blocks
    # a channel count of several blocks: the last block is ragged (160 = 96 + 64, 260 = 96 + 96 + 68)
    assert 160 - 32 * K.sub_tiles(160) == 64 and 260 - 2 * 32 * K.sub_tiles(260) == 68


# ---- weight gradient ----------------------------------------------------------------------------------------------------------------------
def _loop_model(dy, x, w, nbr):
    y = torch.zeros(nbr.shape[1], w.shape[1], dtype=F64)
    rows = []
    for k in range(nbr.shape[0]):
        for r in range(nbr.shape[1]):
            if int(nbr[k, r]) >= 0:
                rows.append((r, w[k] @ x[int(nbr[k, r])]))
    for r, v in rows:
        y = y + F.one_hot(torch.tensor(r), nbr.shape[1]).double()[:, None] * v[None, :]
    return (y * dy).sum()


def test_wgrad_reference_equals_autograd():
    c = K.table_case("k27_m40")
    dy, x = K.float_operands(c["M"], c["V_in"], 8, 12)
    w = torch.zeros(c["K"], 8, 12, dtype=F64, requires_grad=True)
    _loop_model(d64(dy), d64(x), w, c["nbr"]).backward()
    dw, mag = K.wgrad_ref(d64(dy), d64(x), c["nbr"])
    close(dw, w.grad)
    assert bool((mag >= dw.abs() - 1e-12).all())
    assert bool((dw[0] == 0).all()) and bool((mag[0] == 0).all())      # the offset without pairs
    # the gather + matmul model gives the same gradients, and its input gradient is the model on the transposed table
    y, dx, dw2, dres = K.conv_grads(x, torch.randn(c["K"], 8, 12, generator=K.gen(1)), c["nbr"], dy, res=torch.zeros(c["M"], 8))
    close(dw2, dw)
    close(dres, d64(dy))


def test_integer_gradients_are_exact_in_fp32():
    for name in ("k27_m600", "k1_m130"):
        c = K.table_case(name)
        for ones in (False, True):
            dy, x = K.int_operands(c["M"], c["V_in"], 36, 68, ones=ones)
            r64, mag = K.wgrad_ref(d64(dy), d64(x), c["nbr"])
            r32, _ = K.wgrad_ref(dy, x, c["nbr"])
            assert float(mag.max()) < 2 ** 24 and torch.equal(r32.double(), r64)
            if ones:
                assert torch.equal(r64[:, 0, 0], torch.tensor(c["counts"], dtype=F64))


def test_bf16_rounding_and_carry():
    t = torch.cat([torch.randn(4096, generator=K.gen(3)), torch.tensor([K.CARRY, K.CARRY2, 0.0, -0.0, 1.0, 2.0 ** -130, 3.0e38])])
    assert torch.equal(K.round_bf16(t), t.bfloat16().float())
    assert float(K.round_bf16(torch.tensor([K.CARRY]))) == 2.0 and float(K.round_bf16(torch.tensor([K.CARRY2]))) == -1.0
    dy, x = K.float_operands(5, 4, 8, 4)
    assert float(dy.view(-1)[0]) == K.CARRY and float(x.view(-1)[0]) == K.CARRY2
    # products of two bf16 values are exact in fp32
    a, b = K.round_bf16(dy.view(-1)[:16]), K.round_bf16(x.view(-1)[:16])
    assert torch.equal((a * b).double(), a.double() * b.double())


@pytest.mark.parametrize("bf16", [False, True])
def test_wgrad_fp32_reference_stays_inside_the_bound(bf16):
    for name, (co, ci) in (("k27_m600", (36, 100)), ("k3_m150", (160, 68)), ("k1_m1", (4, 4)), ("k125_m20", (68, 4))):
        c = K.table_case(name)
        dy, x = K.float_operands(c["M"], c["V_in"], co, ci)
        r64, mag = K.wgrad_ref(d64(dy), d64(x), c["nbr"], bf16=bf16)
        r32, _ = K.wgrad_ref(dy, x, c["nbr"], bf16=bf16)
        real, cap = K.tile_counts(c["counts"])
        n_slots = K.wgrad_ranges(c["K"], ci, co, cap * K.PT) + c["K"]
        bound = K.wgrad_bound(mag, c["counts"], n_slots)
        assert bool(((r32.double() - r64).abs() <= bound).all())
        empty = [k for k, n in enumerate(c["counts"]) if n == 0]
        assert all(float(bound[k].max()) <= K.FLOOR for k in empty)     # an empty offset: exact zeros
        old = torch.randn(r64.shape, generator=K.gen(5))
        assert bool((((old + r32).double() - (old.double() + r64)).abs() <= K.wgrad_bound(mag, c["counts"], n_slots, old)).all())


def test_out_rows_reference():
    pos = torch.tensor([[0, -1, 1], [-1, 128, -1]]).numpy()
    assert K.out_rows_ref(pos, 256).tolist() == [0, 2] + [-1] * 126 + [1] + [-1] * 127


def test_wgrad_ranges_never_exceed_the_tiles():
    assert K.wgrad_ranges(1, 4, 4, 128) == 1 and K.wgrad_ranges(27, 64, 64, 128 * 1000) == 768
    assert K.wgrad_ranges(27, 260, 160, 128 * 1000) == 42 and K.wgrad_ranges(125, 32, 32, 128 * 1000) == 512


# ---- BatchNorm ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 257])
@pytest.mark.parametrize("relu", [False, True])
def test_batchnorm_references_equal_torch(M, relu):
    c = K.bn_case(M, 12)
    x, gamma, beta, res = (d64(c[k]).clone().requires_grad_(True) for k in ("x", "gamma", "beta", "res"))
    rm, rv = d64(c["run_mean"]).clone(), d64(c["run_var"]).clone()
    mom = K.MOMENTA[0]
    y = F.batch_norm(x, rm, rv, gamma, beta, True, mom, K.EPS) + res
    y = torch.relu(y) if relu else y
    mean, var, rstd = K.bn_stats_ref(d64(c["x"]))
    close(mean, x.detach().mean(0))
    close(var, x.detach().var(0, unbiased=False))
    got, _ = K.bn_apply_ref(d64(c["x"]), mean, rstd, d64(c["gamma"]), d64(c["beta"]), d64(c["res"]), relu)
    close(got, y.detach(), 1e-9)                                 # the big column: torch's variance differs in the last bits of a double
    ref_rm, ref_rv = K.bn_running_ref(d64(c["run_mean"]), d64(c["run_var"]), mean, var, M, mom)
    close(ref_rm, rm)
    close(ref_rv, rv, 1e-9)
    y.backward(d64(c["dy"]))
    dx, dres, dgamma, dbeta = K.bn_backward_ref(d64(c["dy"]), y.detach() if relu else None, d64(c["x"]), mean, rstd, d64(c["gamma"]))
    keep = [j for j in range(12) if j != K.COL_CONST]            # (the constant column: rstd = 316, torch's x - mean is not exactly 0)
    close(dx[:, keep], x.grad[:, keep], 1e-8)
    close(dres, res.grad)
    close(dgamma[keep], gamma.grad[keep], 1e-8)
    close(dbeta, beta.grad)


def test_batchnorm_unbiased_factor_is_one_for_one_row():
    c = K.bn_case(1, 4)
    mean, var, _ = K.bn_stats_ref(d64(c["x"]))
    assert bool((var == 0).all())
    rm, rv = K.bn_running_ref(d64(c["run_mean"]), d64(c["run_var"]), mean, var, 1, 1.0)
    assert torch.equal(rm, mean) and bool((rv == 0).all())


def test_batchnorm_planted_columns():
    one_pass = []
    for M in K.BN_M:
        for C in K.BN_C:
            c = K.bn_case(M, C)
            x = d64(c["x"])
            mean, var, rstd = K.bn_stats_ref(x)
            m32, v32, r32 = K.bn_stats_ref(c["x"])
            assert float(var[K.COL_CONST]) == 0.0 and float(v32[K.COL_CONST]) == 0.0 and float(mean[K.COL_CONST]) == 1.75
            assert float(rstd[K.COL_CONST]) == 1.0 / K.EPS ** 0.5
            for res in (None, c["res"]):                         # y = beta (+ res) exactly, in fp32 too
                y64, _ = K.bn_apply_ref(x, mean, rstd, d64(c["gamma"]), d64(c["beta"]), d64(res))
                y32, _ = K.bn_apply_ref(c["x"], m32, r32, c["gamma"], c["beta"], res)
                want = d64(c["beta"])[K.COL_CONST] + (0 if res is None else d64(res)[:, K.COL_CONST])
                assert torch.equal(y64[:, K.COL_CONST], want.expand(M))
                assert torch.equal(y32[:, K.COL_CONST], (c["beta"][K.COL_CONST] + (0 if res is None else res[:, K.COL_CONST])).expand(M))
            if M < 2:
                continue
            big = x[:, K.COL_BIG]
            assert float(big.mean()) == 1000.0 and float(c["x"][:, K.COL_BIG].sum()) == 1000.0 * M
            assert float(c["x"][:, K.COL_BIG].flip(0).cumsum(0)[-1]) == 1000.0 * M          # any order of the partial sums is exact
            assert bool(((big - 1000.0) * 8 == torch.round((big - 1000.0) * 8)).all())
            if M >= 255:
                assert 0.6 < float(big.std()) < 1.5
                b32 = c["x"][:, K.COL_BIG]
                one_pass.append(abs(float((b32 * b32).mean() - b32.mean() ** 2) - float(var[K.COL_BIG])))
            out = x[:, K.COL_OUT]
            rest = out[1:]
            if M >= 255:
                assert int((out - out.mean()).abs().argmax()) == 0
                assert 7.0 < float((out[0] - rest.mean()) / rest.std()) < 9.5
    assert max(one_pass) > 1e-2 and sum(e > 1e-4 for e in one_pass) == len(one_pass)       # a one-pass fp32 variance loses the big column


@pytest.mark.parametrize("C", K.BN_C)
def test_batchnorm_fp32_references_pass_the_rule(C):
    for M in K.BN_M:
        c = K.bn_case(M, C)
        x = d64(c["x"])
        s64, s32 = K.bn_stats_ref(x), K.bn_stats_ref(c["x"])
        for name, a, b, sc in zip(("mean", "var", "rstd"), s64, s32, K.bn_stats_scale(c["x"])):
            K.reference_passes(f"bn_stats {name}", a, b, sc)
        mean32, rstd32 = s64[0].float(), s64[2].float()          # what the device tests hand to apply / backward: the fp32 statistics
        for res in (None, c["res"]):
            for relu in (False, True):
                y64, _ = K.bn_apply_ref(x, d64(mean32), d64(rstd32), d64(c["gamma"]), d64(c["beta"]), d64(res), relu)
                y32, _ = K.bn_apply_ref(c["x"], mean32, rstd32, c["gamma"], c["beta"], res, relu)
                K.reference_passes("bn_apply", y64, y32, K.bn_apply_scale(c["x"], mean32, rstd32, c["gamma"], c["beta"], res))
        for y in (None, torch.relu(c["res"])):
            r64 = K.bn_backward_ref(d64(c["dy"]), d64(y), x, d64(mean32), d64(rstd32), d64(c["gamma"]))
            r32 = K.bn_backward_ref(c["dy"], y, c["x"], mean32, rstd32, c["gamma"])
            sdx, sdg, sdb = K.bn_backward_scale(c["dy"], y, c["x"], mean32, rstd32, c["gamma"])
            K.reference_passes("bn_backward dx", r64[0], r32[0], sdx)
            assert torch.equal(r32[1].double(), r64[1])
            K.reference_passes("bn_backward dgamma", r64[2], r32[2], sdg)
            K.reference_passes("bn_backward dbeta", r64[3], r32[3], sdb)
        for mom in K.MOMENTA:
            a = K.bn_running_ref(d64(c["run_mean"]), d64(c["run_var"]), d64(mean32), d64(s64[1].float()), M, mom)
            b = K.bn_running_ref(c["run_mean"], c["run_var"], mean32, s64[1].float(), M, mom)
            K.reference_passes("bn_stats running_mean", a[0], b[0], torch.maximum(c["run_mean"].abs(), mean32.abs()))
            K.reference_passes("bn_stats running_var", a[1], b[1], torch.maximum(c["run_var"].abs(), s64[1].float() * (M / max(M - 1, 1))))


# ---- backward of the superpoint mean ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", K.POOL_V)
def test_pool_case_and_reference(V):
    for pow2 in (False, True):
        c = K.pool_case(V, pow2)
        N, S = c["N"], c["S"]
        assert sorted(c["sidx"].tolist()) == list(range(N)) and c["seg_start"].tolist()[0] == 0 and c["seg_start"].tolist()[-1] == N
        assert c["superpoints"].dtype == torch.int64 and c["seg_start"].dtype == torch.int32 and c["sp_start"].dtype == torch.int32
        sizes = torch.bincount(c["superpoints"], minlength=S)
        assert sizes.tolist() == c["sp_sizes"] == (c["sp_start"][1:] - c["sp_start"][:-1]).tolist()
        assert sizes[0] == 1 and sizes[-1] == 0                  # a superpoint of one point, an id no point carries
        if pow2:
            assert all(s in (0, 1, 2, 4, 8) for s in c["sp_sizes"])
        per_voxel = torch.bincount(c["voxel_of"], minlength=V).tolist()
        assert per_voxel == c["sizes"] and 50 in per_voxel and (V == 1 or per_voxel[0] == 1)
        for v in range(V):                                      # sidx lists a voxel's points
            assert bool((c["voxel_of"][c["sidx"][c["seg_start"][v]:c["seg_start"][v + 1]]] == v).all())
        big = per_voxel.index(50)
        assert len(set(c["superpoints"][c["voxel_of"] == big].tolist())) > 5      # one voxel, many superpoints
        dout = pool_dout = K.pool_dout(S, 12)
        feat = torch.randn(V, 12, dtype=F64, requires_grad=True)
        (K.pool_forward_model(feat, c) * d64(dout)).sum().backward()
        r64, top = K.pool_backward_ref(d64(pool_dout), c)
        close(r64, feat.grad)
        r32, _ = K.pool_backward_ref(dout, c)
        K.reference_passes("pool_backward", r64, r32, top)
        assert bool((top >= 0).all()) and bool((r64.abs() <= top * 50 + 1e-12).all())
        if pow2:
            di = K.pool_dout(S, 12, integer=True)
            assert torch.equal(K.pool_backward_ref(di, c)[0].double(), K.pool_backward_ref(d64(di), c)[0])


# ---- the host wrappers refuse before they touch a device ------------------------------------------------------------------------------------
def test_wrappers_refuse_chained_and_lean_lists(monkeypatch):
    from segdino3d_amd import _lib, ops, train_ops

    def no_library():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(_lib, "load", no_library)
    dy, x = torch.zeros(5, 4), torch.zeros(5, 4)
    bad = [K.StubPairs(center=ops.PAIR_CHAINED, pos=torch.empty(0, dtype=torch.int32)),
           K.StubPairs(center=ops.PAIR_CHAINED, pos=torch.zeros(3, 5, dtype=torch.int32)),
           K.StubPairs(pos=None), K.StubPairs(pos=torch.empty(0, dtype=torch.int32))]
    for pairs in bad:
        with pytest.raises(ValueError):
            train_ops.pair_out_rows(pairs)
        with pytest.raises(ValueError):
            train_ops.pair_wgrad(dy, x, pairs)
        with pytest.raises(ValueError):
            train_ops.pair_wgrad_native(dy, x, pairs)
        assert pairs.out_idx is None
    # lists that carry their output rows are served without a position table: nothing to refuse, the cached list comes back
    rows = torch.arange(4, dtype=torch.int32)
    assert train_ops.pair_out_rows(K.StubPairs(pos=None, out_idx=rows)) is rows


def test_wrappers_refuse_wrong_shapes_before_the_device():
    from segdino3d_amd import train_ops
    pairs = K.StubPairs(pos=torch.zeros(3, 5, dtype=torch.int32))
    with pytest.raises(RuntimeError):                            # CPU tensors: no fallback
        train_ops.pair_wgrad(torch.zeros(5, 4), torch.zeros(5, 4), pairs)
