"""The inputs, the float64 reference and the kernel-selection twins of tests/conv_forward_cases.py, checked on the CPU: the reference
against an independent formulation, the 2^24 condition that makes the integer cases bit-exact, the planted situations of the table
set, the pass-1 / dense variants the GPU case lists reach, `sd3d_dense_plan_code` at its boundaries, and the refusals the host wrappers
make before anything reaches a device."""
import pytest
import torch

from tests import conv_forward_cases as C
from tests.train_kernel_cases import StubPairs

F64 = torch.float64
ALL_PAIR_CASES = C.PAIR_CASES + [C.RANGE_CASE]


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.TABLE_NAMES)
def test_reference_equals_the_loop_over_pairs(name):
    t = C.table(name)
    for kind, act in ((C.int_operands, "relu"), (C.float_operands, None)):
        o = kind(t["V_in"], t["M"], t["K"], 32, 8, seed=3)
        a, mag = C.conv_ref(o["x"], o["w"], t["nbr"], o["scale"], o["shift"], o["res"], act)
        b = C.conv_pairs_ref(o["x"], o["w"], t["nbr"], o["scale"], o["shift"], o["res"], act)
        assert a.dtype == F64 and torch.allclose(a, b, rtol=1e-13, atol=1e-13 * float(mag.max()))
        if kind is C.int_operands:
            assert torch.equal(a, b)
        pre, _ = C.conv_ref(o["x"], o["w"], t["nbr"], o["scale"], o["shift"], o["res"])
        assert bool((mag >= pre.abs() - 1e-12 * mag).all())          # the magnitude bounds the sum before the activation
        if t["dead"] is not None:                                # a row without any pair: act(shift + res)
            assert torch.equal(a[t["dead"]], C.act_ref(o["shift"].double() + o["res"][t["dead"]].double(), act))


def test_reference_of_a_linear_and_the_activations():
    o = C.int_operands(7, 7, 1, 32, 5)
    y, mag = C.conv_ref(o["x"], o["w"], None, o["scale"], o["shift"], o["res"])
    want = (o["x"].double() @ o["w"][0].double().t()) * o["scale"].double() + o["shift"].double() + o["res"].double()
    assert torch.equal(y, want)
    assert torch.equal(mag, (o["x"].abs().double() @ o["w"][0].abs().double().t()) * o["scale"].double() + o["shift"].abs().double()
                       + o["res"].abs().double())
    v = torch.linspace(-4, 4, 33, dtype=F64)
    assert torch.allclose(C.act_ref(v, "gelu"), torch.nn.functional.gelu(v), rtol=0, atol=1e-15)
    assert torch.allclose(C.act_ref(v, "sigmoid"), torch.sigmoid(v), rtol=0, atol=1e-15)
    assert torch.equal(C.act_ref(v, "relu"), v.clamp_min(0)) and C.act_ref(v, None) is v


@pytest.mark.parametrize("c", ALL_PAIR_CASES, ids=C.case_id)
def test_integer_pair_cases_are_exact_in_fp32(c):
    """Every term is an integer and the magnitude - a bound on every partial sum of every order - stays below 2^24: fp32 cannot round."""
    t = C.table(c.table)
    o, ref32, mag = C.pair_int_case(c)
    for v in o.values():
        assert torch.equal(v, v.round())
    assert float(mag.max()) < C.EXACT_LIMIT
    r32, _ = C.conv_ref(o["x"], o["w"], t["nbr"], o["scale"], o["shift"], o["res"], c.act, dtype=torch.float32, want_mag=False)
    assert r32.dtype == torch.float32 and torch.equal(r32, ref32)
    if t["dead"] is not None:
        assert torch.equal(ref32[t["dead"]], C.act_ref(o["shift"] + o["res"][t["dead"]], c.act))


def test_integer_linear_cases_are_exact_in_fp32():
    for cin, cout in sorted({(c.cin, c.cout) for c in C.DENSE_CASES} | {(ci, co) for _m, ci, co in C.LINEAR_SHAPES}):
        o = C.linear_operands(cin, cout, rows=257)
        M = 257                                                  # the rows are independent: a slice shows the condition for all of them
        r64, mag = C.linear_ref(o, M, scale=True, act="relu")
        bound = (4 * cin) * 3 + 3 + 3                            # the same bound for every row, from the operand ranges alone
        assert float(mag.max()) <= bound < C.EXACT_LIMIT
        r32, _ = C.linear_ref(o, M, scale=True, act="relu", dtype=torch.float32, want_mag=False)
        assert torch.equal(r32, r64.float())


@pytest.mark.parametrize("c", C.PAIR_FLOAT_CASES, ids=C.case_id)
def test_float_reference_passes_its_own_rule(c):
    _o, r64, r32, mag = C.pair_float_case(c)
    e32 = C.reference_passes("pair_conv", r64, r32, mag)
    assert 0 < e32 < 1e-6


# ---- the planted situations -----------------------------------------------------------------------------------------------------------------
def test_planted_situations_are_in_the_table_set():
    tabs = {n: C.table(n) for n in C.TABLE_NAMES}
    assert {t["K"] for t in tabs.values()} >= {1, 3, 8, 27, 125}
    for name in C.BOTH_PLANTED:
        assert set(C.PLANTED) <= set(tabs[name]["counts"]), name
    for t in tabs.values():
        nbr = t["nbr"]
        assert nbr.dtype == torch.int32 and int(nbr.max()) < t["V_in"] and int(nbr.min()) >= -1
        assert t["counts"] == (nbr >= 0).sum(1).tolist() and t["n_pairs"] == sum(t["counts"])
        if t["dead"] is not None:
            assert int((nbr[:, t["dead"]] >= 0).sum()) == 0
        if t["kind"] == "direct":
            assert bool(((nbr >= 0).sum(0) == 1).all())
        if t["kind"] == "sym":
            K, M = nbr.shape
            assert torch.equal(nbr[K // 2], torch.arange(M, dtype=torch.int32))
            for k in range(K // 2):
                r = (nbr[k] >= 0).nonzero(as_tuple=True)[0]
                assert torch.equal(nbr[K - 1 - k][nbr[k][r].long()].long(), r)
    assert sum(t["dead"] is not None for t in tabs.values()) >= 6
    hot = tabs["k27_m600"]["nbr"]
    assert float((hot == C.HOT).sum()) > 0.25 * tabs["k27_m600"]["n_pairs"]
    assert C.capacity_tiles(tabs["big27_m6000"]) >= 1024
    # a run of one offset longer than WS_RANGE_TILES tiles, short offsets behind it
    lr = tabs["long_run"]["counts"]
    assert -(-lr[0] // C.PT) > C.WS_RANGE_TILES and lr[1:] == [1, 127, 128, 129]
    # ... and a launch in which one workgroup's range is longer than WS_RANGE_TILES
    r = C.RANGE_CASE
    real, cap = C.tile_counts(tabs[r.table]["counts"])
    assert C.pass1_variant(r.cin, r.cout, False, False, False, cap) == ("ws2",)
    assert real // C.ws_grid(r.cin, r.cout, cap) > C.WS_RANGE_TILES


def test_every_table_has_a_pair_case():
    assert {c.table for c in ALL_PAIR_CASES} == set(C.TABLE_NAMES)
    for c in ALL_PAIR_CASES + C.PAIR_FLOAT_CASES:
        kind = C.table(c.table)["kind"]
        assert (c.mode == "direct") == (kind == "direct") and (c.mode != "chained" or kind == "sym")
        assert c.cin % 32 == 0 and c.split % 32 == 0 and c.split < c.cin and c.cout % 4 == 0
    assert {c.cout for c in C.PAIR_CASES} >= set(C.COUT_PAIR)
    assert {(c.cin, c.split) for c in C.PAIR_CASES} >= set(C.CIN + C.CIN_SPLITS)
    assert {c.act for c in C.PAIR_FLOAT_CASES} == {None, "relu", "gelu", "sigmoid"}


# ---- the kernel selection -------------------------------------------------------------------------------------------------------------------
def test_column_tiles():
    want = {4: (1, 1), 32: (1, 1), 36: (2, 1), 64: (2, 1), 68: (3, 1), 96: (3, 1), 100: (4, 1), 128: (4, 1), 160: (1, 5), 192: (3, 2),
            256: (4, 2), 260: (3, 3), 224: (1, 7), 512: (4, 4)}
    for cout, v in want.items():
        assert C.pg_col_tiles(cout) == v, cout


def test_pass1_variants_by_hand():
    P = C.pass1_variant
    assert P(32, 32, False, False, False, 10) == ("ws", 1, False) and P(512, 32, False, True, True, 10) == ("ws", 1, True)
    assert P(544, 32, False, False, False, 10) == ("lockstep", 1, False)                                 # 32 x 548 x 4 bytes > 68 KB
    assert P(256, 64, False, False, True, 10) == ("ws", 2, False) and P(288, 64, False, False, False, 10) == ("lockstep", 2, False)
    assert P(160, 96, False, False, False, 10) == ("ws", 3, False) and P(192, 96, False, False, False, 10) == ("lockstep", 3, False)
    assert P(128, 128, False, True, False, 10) == ("ws", 4, True) and P(160, 128, False, False, False, 10) == ("lockstep", 4, False)
    assert P(96, 96, False, False, True, 10) == ("lockstep", 3, False) and P(96, 128, False, False, True, 10) == ("lockstep", 4, False)
    assert P(32, 32, True, False, False, 10) == ("chained", 1) and P(96, 260, True, False, False, 5000) == ("chained", 3)
    assert P(32, 36, False, False, False, 10) == ("lockstep", 2, False)                                   # Cout != 32 nt
    assert P(32, 256, False, False, False, 1023) == ("lockstep", 4, False) and P(32, 256, False, False, False, 1024) == ("ws2",)
    assert P(288, 256, False, False, False, 1024) == ("ws2",) and P(320, 256, False, False, False, 1024) == ("lockstep", 4, False)
    assert P(32, 256, False, False, True, 1024) == ("lockstep", 4, False)


def test_case_lists_reach_every_variant():
    want = {("ws2",)} | {("ws", nt, d) for nt in (1, 2, 3, 4) for d in (False, True)} \
        | {("lockstep", nt, d) for nt in (1, 2, 3, 4) for d in (False, True)} | {("chained", nt) for nt in (1, 2, 3, 4)}
    reached = {}
    for c in C.PAIR_CASES:
        for label in C.pair_variants(c):
            reached.setdefault(label, set()).add(c.table)
    assert set(reached) == want, sorted(want - set(reached), key=str)
    for label, tables in reached.items():                        # ... each on a table with an empty offset and the 127 / 128 / 129 boundary
        assert tables & set(C.BOTH_PLANTED), label
    several = set()                                              # ... and each where a workgroup has more than one tile
    for c in C.PAIR_CASES:
        t = C.table(c.table)
        for crowded in (False, True):
            if C.tiles_per_workgroup(c, crowded) > 1:
                several.add(C.pass1_variant(c.cin, c.cout, c.mode == "chained", c.mode == "direct", crowded, C.capacity_tiles(t)))
    assert several == want, sorted(want - several, key=str)
    dense = {C.dense_variant(c.cout) for c in C.DENSE_CASES if C.takes_dense(c.M, c.cout)}
    assert dense == {("dense", nt) for nt in (1, 2, 3, 4)}
    groups = {C.pg_col_tiles(c.cout) for c in C.DENSE_CASES if C.takes_dense(c.M, c.cout)}
    assert groups >= {(1, 5), (3, 2), (3, 3), (4, 2)}
    assert not C.takes_dense(16383, 64) and C.takes_dense(16384, 64) and not C.takes_dense(16384, 199)
    assert not C.takes_dense(16384, 100, ld_out=102) and not C.takes_dense(16384, 100, ld_res=102) and not C.takes_dense(16384, 64, nt=1)
    assert {c.M for c in C.DENSE_CASES} == set(C.DENSE_ROWS)


def test_dense_plan_code_at_its_boundaries():
    from segdino3d_amd import ops
    pinned = {(2016, 32, 64): 1, (2017, 32, 64): 1, (2016, 64, 64): 1, (2017, 64, 64): 0,       # 63 / 64 row tiles, one / two steps
              (200, 224, 256): 1, (200, 256, 256): -1,                                              # steps >= 8: the four waves split them
              (100000, 32, 160): 1, (100000, 32, 199): 1, (100000, 32, 192): 3, (100000, 32, 128): 4, (100000, 32, 260): 3,
              (8192, 32, 64): 1, (65536, 32, 64): 2, (1, 32, 4): 1, (1, 256, 3): -1}
    for (rows, cin, cout), code in pinned.items():
        assert ops.dense_code(rows, cin, cout) == code, (rows, cin, cout)
    for rows in (1, 31, 32, 33, 200, 2016, 2017, 2048, 4096, 16383, 16384, 65536, 100000):
        for cin in (32, 64, 224, 256, 288):
            for cout in (3, 4, 32, 36, 64, 96, 128, 160, 192, 199, 256, 260, 1024):
                assert ops.dense_code(rows, cin, cout) == C.dense_plan_code(rows, cin, cout), (rows, cin, cout)
    assert ops.small_rows_code(224) == 1 and ops.small_rows_code(256) == -1
    for rows, cin, cout in C.LINEAR_SHAPES:
        assert rows <= C.LINEAR_ROWS < C.DENSE_MIN_ROWS
    # an empty product has a code too: the C function itself (it divided by its zero column tiles below 64 row tiles)
    from segdino3d_amd import _lib
    plan = _lib.load().sd3d_dense_plan_code
    for rows, cin, cout, code in ((200, 64, 0, 1), (200, 256, 0, 1), (2016, 64, 0, 1), (2100, 64, 0, 0), (2100, 32, 0, 1), (0, 64, 64, 1), (0, 64, 0, 1)):
        assert plan(rows, cin, cout) == code == ops.dense_code(rows, cin, cout) == C.dense_plan_code(rows, cin, cout), (rows, cin, cout)


def test_ksplit_twin():
    assert C.lds_ksplit(600, 96, 27, 3, 1 << 30) == 8 and C.lds_ksplit(600, 96, 27, 3, 8 * 600 * 96 * 4 - 1) == 1
    assert C.lds_ksplit(600, 96, 3, 3, 1 << 30) == 1 and C.lds_ksplit(128 * 96, 32, 27, 1, 1 << 30) == 4


# ---- refusals of the host wrappers ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Host tensors stand in for device ones: the wrappers' pointer helpers hand out a fake address, and any call into the library
    fails the test."""
    from segdino3d_amd import _lib, ops

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the wrapper called {name} before it refused")

    monkeypatch.setattr(ops, "_rows", lambda t, name="tensor": (64, t.stride(0)))
    monkeypatch.setattr(ops, "_ptr", lambda t, dtype=None, name="tensor": None if t is None else 64)
    monkeypatch.setattr(_lib, "load", lambda: Untouchable())
    return ops


def test_host_wrappers_refuse_before_touching_a_device(no_device):
    ops = no_device
    x, x2 = torch.zeros(5, 32), torch.zeros(5, 64)
    w = torch.zeros(3, 8, 96)
    with pytest.raises(ValueError, match="weights have 3 offsets, the pair lists 5"):
        ops.pair_conv(x, w, StubPairs(K=5), x2=x2)
    with pytest.raises(ValueError, match=r"concat channels 32\+32 != Cin 96"):
        ops.pair_conv(x, w, StubPairs(K=3), x2=x)
    with pytest.raises(ValueError, match="input channels 32 != Cin 96"):
        ops.pair_conv(x, w, StubPairs(K=3))
    nbr = torch.zeros(3, 5, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"concat channels 32\+32 != Cin 96"):
        ops.gather_gemm(x, w, nbr=nbr, x2=x)
    with pytest.raises(ValueError, match="input channels 64 != Cin 96"):
        ops.gather_gemm(x2, w, nbr=nbr)
    for bad in (torch.zeros(2, 5, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int32)):
        with pytest.raises(ValueError, match="nbr shape"):
            ops.gather_gemm(x, w, nbr=bad, x2=x2, M=5)
    good = ops.split_weights(w, 3)
    assert good.dtype == torch.bfloat16 and tuple(good.shape) == (2, 3, 8, 96)
    for bad in (good.float(), good[:, :2].contiguous(), good[:, :, :, :64].contiguous(), good.transpose(2, 3)):
        with pytest.raises(ValueError, match="wt_split must be contiguous bf16"):
            ops.gather_gemm(x, w, nbr=nbr, x2=x2, wt_split=bad)
