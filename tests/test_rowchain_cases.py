"""CPU checks of tests/rowchain_cases.py: every reference against a float64 torch restatement, the fp32 evaluation of every float
reference against the tolerance rule (cap included), and the reach of the case lists - all 13 instantiations of the 16-row LINEAR
dispatch, the block counts of the generic loops, the K parts and round sizes of the 4-row split, both paths of BITS2D.  No case is
skipped or filtered: a shape that cannot be expressed fails here."""
import math

import pytest
import torch

from tests import decoder_kernel_cases as K
from tests import rowchain_cases as R


def d64(t):
    return None if t is None else t.double()


ALL_LINEAR = [(c, True) for c in R.LINEAR_EXACT] + [(c, False) for c in R.LINEAR_FLOAT]


# ---- references ---------------------------------------------------------------------------------------------------------------------------
def test_linear_reference_is_torch_linear():
    for c, exact in ALL_LINEAR[::5]:
        p = R.linear_case(c, exact)
        want = torch.nn.functional.linear(p["x"].double(), p["w"].double(), p["b"].double())
        if p["res"] is not None:
            want = want + p["res"].double()
        want = {None: lambda t: t, "relu": torch.relu, "gelu": torch.nn.functional.gelu, "sigmoid": torch.sigmoid}[p["act"]](want)
        got = R.linear_ref(p["x"].double(), p["w"].double(), p["b"].double(), d64(p["res"]), p["act"])
        assert torch.allclose(got, want, rtol=1e-13, atol=1e-13), R.linear_id(c)


def test_attention_reference_is_scaled_dot_product_attention():
    for nq, Lk, masked in [(5, 33, True), (17, 17, False), (3, 65, True)]:
        c = R.attn_case(nq, Lk, masked, 8)
        q, k, v = (c[n].double().view(-1, R.H, R.DH).transpose(0, 1) for n in "qkv")
        want = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=None if c["open"] is None else c["open"][None], scale=R.ATTN_SCALE)
        got = R.attn_ref(c["q"].double(), c["k"].double(), c["v"].double(), R.ATTN_SCALE, c["open"])
        assert torch.allclose(got, want.transpose(0, 1).reshape(nq, R.D), rtol=1e-12, atol=1e-12)


def test_attention_planted_rows():
    c = R.attn_case(17, 129, True, 16)
    o = c["open"]
    assert int(o[0].sum()) >= 1 and bool(o[0, 128]) and not bool(o[1, 16:32].any()) and not bool(o[1, 64:128].any())
    assert bool(o[1, :16].all()) and bool(o[1, 128])
    mid = ((9 + 1) // 2) * 16
    assert not bool(o[2, mid:128].any()) and not bool(o[3, :mid].any())
    s = R.logits(c["q"], c["k"], R.ATTN_SCALE).masked_fill(~o[None], float("-inf"))
    top2 = s[:, 16].topk(2, -1)
    assert int(top2.indices[0, 0]) == 0 and int(top2.indices[1, 0]) == 128                 # first tile / last tile of the second half
    assert float(top2.values[0, 0] - top2.values[0, 1]) > 3.0 and float(top2.values[1, 0] - top2.values[1, 1]) > 3.0
    for nq, Lk, masked in R.attn_shapes():                      # no open logit of any row further than the spread from the row's largest
        cc = R.attn_case(nq, Lk, masked, R.ATTN_SPREAD)
        ss = R.logits(cc["q"], cc["k"], R.ATTN_SCALE)
        hi = ss if cc["open"] is None else ss.masked_fill(~cc["open"][None], float("-inf"))
        lo = ss if cc["open"] is None else ss.masked_fill(~cc["open"][None], float("inf"))
        assert float((hi.amax(-1) - lo.amin(-1)).max()) <= R.ATTN_SPREAD * (1 + 1e-5)
        assert cc["open"] is None or bool(cc["open"][:, Lk - 1].all())                     # BITS2D always opens the dummy key
    only_dummy = R.attn_case(4, 33, True, 16)["open"][0]
    assert int(only_dummy.sum()) == 1 and bool(only_dummy[32])


def test_merge_reference_recombines_the_whole_softmax():
    for nq, Lk, ks in [(45, 97, 3), (7, 40, 2), (33, 64, 1), (40, 333, 8)]:
        c = R.merge_case(nq, Lk, ks)
        got = R.merge_ref(c["m"].double(), c["l"].double(), c["o"].double())
        g = R.gen(101, nq, Lk, ks, 0)
        q, k = torch.randn(nq, R.D, generator=g), torch.randn(Lk, R.D, generator=g)
        want = R.attn_ref(q.double(), k.double(), c["v"].double(), R.ATTN_SCALE, c["open"])
        assert torch.allclose(got, want, rtol=2e-6, atol=2e-5)                             # the parts were rounded to fp32
        if ks > 1:
            assert bool(torch.isinf(c["m"][0, 0]).all()) and bool((c["l"][0, 0] == 0).all())   # row 0: split 0 has every key blocked
        ws = R.merge_pack(c).view(-1, R.H, ks, R.PART)
        assert float(ws[1 if nq > 32 else 0, 3, ks - 1, 64 + 5 * 32]) == float(c["o"][ks - 1, 32 if nq > 32 else 0, 3, 5])


def test_bits2d_reference_and_planted_bits():
    for launch in R.BITS_LAUNCHES:
        for si, (nq, nw, nm) in enumerate(launch):
            c = R.bits_case(nq, nw, nm, si == 0)
            ref = R.bits2d_ref(c["open"], c["near"])
            loop = torch.ones(nq, nm, dtype=torch.bool)
            for qi in range(nq):
                for m in range(nm - 1):
                    loop[qi, m] = not bool((c["open"][qi] & c["near"][m]).any())
            loop[:, nm - 1] = False
            assert torch.equal(ref, loop)
            assert bool(ref[0, :nm - 1].all())                                             # nothing open: only the dummy key
            for qi, mi, s in c["planted"]:
                assert not bool(ref[qi, mi]) and int((~ref[:, mi]).sum()) == 1             # the one hit of that key, carried by one bit
                assert int((c["open"][qi] & c["near"][mi]).sum()) == 1 and bool(c["open"][qi, s])
            words = R.pack_bits(~c["open"], nw, True)
            assert words.shape == (nq, nw)
            if si == 0 and c["planted"]:
                assert int(words[1, nw - 1]) == 0x7FFFFFFF and (nw == 1 or int(words[1, 0]) == -1)     # only bit 31 of the last word open


def test_bits2d_cases_reach_both_paths_and_every_size():
    shapes = [s for launch in R.BITS_LAUNCHES for s in launch]
    assert {nw for _, nw, _ in shapes} == set(R.BITS_NW) and {nm for _, _, nm in shapes} == set(R.BITS_NM)
    assert {nw for _, nw, _ in shapes if nw > 128} == {129, 130, 200}
    planted = {(s > 64 * 32, s >= 128 * 32) for launch in R.BITS_LAUNCHES for si, (nq, nw, nm) in enumerate(launch)
               for _, _, s in R.bits_case(nq, nw, nm, si == 0)["planted"]}
    words = {s // 32 for launch in R.BITS_LAUNCHES for si, (nq, nw, nm) in enumerate(launch) for _, _, s in R.bits_case(nq, nw, nm, si == 0)["planted"]}
    assert 64 in words and 128 in words and planted
    last_bit = [c for launch in R.BITS_LAUNCHES for c in [R.bits_case(*launch[0], True)] if any(s == 32 * c["nw"] - 1 for _, _, s in c["planted"])]
    assert {c["nw"] <= 128 for c in last_bit} == {True, False}                             # the last bit of the last word on both paths
    for a, b in R.BITS_LAUNCHES:
        assert a[1:] != b[1:]                                                              # two scenes with different nw and nm


# ---- reach of the LINEAR lists ------------------------------------------------------------------------------------------------------------------
def test_linear_twin_matches_the_dispatch_table():
    """The decoder's shapes named in the dispatch's comments."""
    assert R.linear_dispatch16(256, 256) == ((1, 4, 4), 4) and R.linear_dispatch16(512, 256) == ((1, 4, 8), 8)
    assert R.linear_dispatch16(1024, 256) == ((1, 4, 16), 16) and R.linear_dispatch16(96, 256) == ((1, 2, 3), 3)
    assert R.linear_dispatch16(512, 768) == ((3, 1, 32), 32) and R.linear_dispatch16(256, 1024) == ((4, 1, 16), 16)
    assert R.linear_dispatch16(48, 32) == ((1, 1, 0), 3) and R.linear_dispatch16(256, 199) == ((1, 4, 4), 4)


def test_linear_cases_reach_every_instantiation_and_block_count():
    reach = {}
    for c, _ in ALL_LINEAR:
        inst, nb = R.linear_dispatch16(c[0] + c[1], c[2])
        reach.setdefault(inst, set()).add(nb)
    assert set(reach) == set(R.INSTANTIATIONS) and len(R.INSTANTIATIONS) == 13
    for inst in R.GENERIC:
        can = R.possible_nb(inst)
        assert {nb % 3 for nb in reach[inst]} == {0, 1, 2}, (inst, reach[inst])
        for nb in (1, 2):                                      # where the dispatch admits it (an even count of <1,2,0> / <2,1,0> blocks goes elsewhere)
            assert (nb in reach[inst]) == (nb in can), (inst, nb)
        assert 1 in reach[inst]
    assert not (2 in R.possible_nb((1, 2, 0)) or 2 in R.possible_nb((2, 1, 0)) or 2 in R.possible_nb((1, 1, 0)))
    for line in sorted(f"rc_linear<{i[0]},{i[1]},{i[2]}>: nb {sorted(v)}" for i, v in reach.items()):
        print("[rowchain-reach]", line)


def test_linear_cases_reach_the_narrow_split():
    kps, rounds = set(), set()
    for c, _ in ALL_LINEAR:
        s = R.narrow_split(c[0] + c[1], c[2])
        assert s["scratch"] <= 4096 and s["kp"] * s["pq"] * 4 == c[0] + c[1] and sum(s["rounds"]) == s["pq"]
        kps.add(s["kp"])
        rounds |= set(s["rounds"])
    assert kps == {1, 2, 4, 8} and rounds == {32, 16, 8, 4, 1}
    print("[rowchain-reach] rcn_linear: K parts", sorted(kps), "round sizes", sorted(rounds))


def test_linear_lists_hold_the_sizes_and_options():
    ks = {c[0] + c[1] for c in R.LINEAR_EXACT}
    assert set(R.LINEAR_K) <= ks and set(R.LINEAR_COUT) <= {c[2] for c in R.LINEAR_EXACT}
    assert {r for c in R.LINEAR_EXACT for r in c[3]} == set(R.LINEAR_ROWS)
    assert {c[6] for c in R.LINEAR_EXACT} == {None, "nodst", "inplace", "prog4"}
    assert any(c[1] and c[0] == c[1] for c in R.LINEAR_EXACT) and any(c[1] and c[0] != c[1] for c in R.LINEAR_EXACT)
    assert any(c[4] for c in R.LINEAR_EXACT) and {c[5] for c in R.LINEAR_FLOAT} == set(R.ACTS)
    assert len(set(ALL_LINEAR)) == len(ALL_LINEAR)
    for c, _ in ALL_LINEAR:
        plan = R.linear_slots(c)                                # fails when the shape does not fit the workgroup's slots
        assert plan["n_slots"] <= R.MAX_SLOTS
        assert c[0] % 16 == 0 and c[1] % 16 == 0 and 1 <= c[2] <= 1024
        assert not c[4] or c[2] <= 256 or c[2] % 4 == 0      # the residual's LOAD and the output share their row stride


def test_exact_linear_cases_are_exact_in_fp32():
    for c in R.LINEAR_EXACT:
        p = R.linear_case(c, True)
        assert R.exact_magnitude(p) < R.EXACT_LIMIT
        ref = R.linear_ref(p["x"].double(), p["w"].double(), p["b"].double(), d64(p["res"]), p["act"])
        assert torch.equal(ref, ref.round()) and torch.equal(ref.float().double(), ref)
        assert torch.equal(R.linear_ref(p["x"], p["w"], p["b"], p["res"], p["act"]).double(), ref)


# ---- the fp32 reference alone passes the rule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.LINEAR_FLOAT, ids=R.linear_id)
def test_fp32_linear_reference_passes(c):
    p = R.linear_case(c, False)
    r64 = R.linear_ref(p["x"].double(), p["w"].double(), p["b"].double(), d64(p["res"]), p["act"])
    r32 = R.linear_ref(p["x"], p["w"], p["b"], p["res"], p["act"])
    R.reference_passes(r64, r32, R.linear_scale(p["x"], p["w"], p["b"], p["res"], p["act"]))
    assert float(p["x"][1].abs().max()) > 500 and float(p["x"][0].abs().max()) < 10


def test_attention_spread_is_the_largest_the_fp32_reference_passes():
    shapes = R.attn_shapes()
    assert {Lk for _, Lk, m in shapes if m} >= set(R.ATTN_LK) | {R.ATTN_LK_MAX} and {Lk for _, Lk, m in shapes if not m} >= set(R.ATTN_LK)
    assert {nq for nq, _, m in shapes if m} == set(R.ATTN_NQ)
    passing = [s for s in R.SPREADS if R.spread_passes(s, shapes)]
    print("[rowchain-reach] attention logit spreads at which the fp32 reference passes the rule:", passing)
    assert passing and max(passing) == R.ATTN_SPREAD


def test_fp32_merge_reference_passes():
    for nq, Lk, ks in [(45, 97, 3), (7, 40, 2), (40, 333, 8)]:
        c = R.merge_case(nq, Lk, ks)
        r64 = R.merge_ref(c["m"].double(), c["l"].double(), c["o"].double())
        R.reference_passes(r64, R.merge_ref(c["m"], c["l"], c["o"]), R.attn_scale(c["v"], c["open"], nq))


@pytest.mark.parametrize("rows", R.SMALL_ROWS)
def test_fp32_ln_pe_box_references_pass_on_two_scenes(rows):
    n, rng_rows, ranges = R.scene_rows(rows)
    assert n == rows + R.SECOND_SCENE_ROWS and torch.equal(rng_rows[0], ranges[0]) and torch.equal(rng_rows[-1], ranges[1])
    c = K.ln_case(n, 256)
    for res in (None, c["res"]):
        r64 = K.layernorm_ref(c["x"].double(), d64(res), c["w"].double(), c["b"].double())
        R.reference_passes(r64, K.layernorm_ref(c["x"], res, c["w"], c["b"]), K.layernorm_scale(c["x"], res, c["w"], c["b"]))
    dim_t, axis = K.pe_tables(256)
    p = R.pe_rows(rows)
    for num, den in ((None, None), (p["mod_num"], p["den2"])):
        r64 = K.sine_pe_ref(p["xyz"].double(), p["rng_rows"].double(), dim_t.double(), axis, d64(num), d64(den))
        R.reference_passes(r64, K.sine_pe_ref(p["xyz"], p["rng_rows"], dim_t, axis, num, den), K.sine_pe_scale(p["xyz"], p["rng_rows"], dim_t, axis, num, den))
    b = R.box_rows(rows)
    _, s64, m64 = K.box_refine_ref(b["ref"].double(), b["dc"].double(), b["sp2"].double(), b["ds"].double(), b["rng_rows"].double(), True)
    _, s32, m32 = K.box_refine_ref(b["ref"], b["dc"], b["sp2"], b["ds"], b["rng_rows"], True)
    ss, sm = K.box_size_scale(b["sp2"], b["ds"], b["rng_rows"])
    R.reference_passes(s64, s32, ss)
    R.reference_passes(m64, m32, sm)
    assert math.isfinite(float(m64.abs().max()))
