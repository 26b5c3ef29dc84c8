"""tests/merge_queries_ref.py, the restatement the merging kernels are pinned against, held to expectations written out by hand
(tests/merge_queries_case.py HAND_CASES and the arithmetic in the docstrings below), so that it is not its own judge; and the room, on
which the restatement alone must find every object."""
import numpy as np

import merge_queries_case as K
import merge_queries_ref as R


def _run(case, **kw):
    return R.merge(case["feats"], case["centre"], case["scores"], case["count"], case["Q"], **{**case["rule"], **kw})


def test_hand_cases():
    cases = K.hand_cases()
    assert len({c["name"] for c in cases}) == len(cases) >= 25
    for case in cases:
        got, want = _run(case), case["expect"]
        assert got["labels"].tolist() == want["labels"], case["name"]
        assert got["seeds"].tolist() == want["seeds"], case["name"]
        k = len(want["seeds"])
        assert got["feats"].shape == (k, K.C_HAND) and got["pos"].shape == (k, 3) and got["scores"].shape == (k,) and got["views"].shape == (k,)
        assert got["scores"].tolist() == case["scores"][want["seeds"]].tolist(), case["name"]          # the seed's score
        for key in ("views", "scores", "pos", "feats"):
            if key in want:
                assert np.array_equal(got[key], np.array(want[key], got[key].dtype).reshape(got[key].shape)), (case["name"], key)
        if case["name"] == "signed zeros":
            assert not np.signbit(got["scores"][0])


def test_chain_is_not_a_transitive_closure():
    """A = 0, B = 0.25, C = 0.5 m on a line, radius 0.3: p = 0, 256, 512 and r_q = 307, so 256^2 <= 307^2 < 512^2: A~B, B~C, A!~C.  With A
    on top A takes B and C stays alone; with B on top B takes both; with C on top C takes B and A stays alone."""
    assert R.rule(radius=0.3)["radius_q"] == 307
    by_name = {c["name"]: c for c in K.hand_cases()}
    assert [m.tolist() for m in _run(by_name["chain, A on top"])["members"]] == [[0, 1], [2]]
    assert [m.tolist() for m in _run(by_name["chain, B on top"])["members"]] == [[0, 1, 2]]
    assert [m.tolist() for m in _run(by_name["chain, C on top"])["members"]] == [[0], [1, 2]]


def test_rank_order_is_the_one_of_the_sort_keys():
    s = np.array([0.5, -0.0, 0.0, 0.5, np.nan, -1.0, np.inf], np.float32)
    keys = R.score_keys(s)
    assert keys[0] == keys[3] and keys[2] < keys[1] and keys[6] < keys[0] < keys[2] and keys[1] < keys[5]
    rows = R.ranked_rows(np.zeros((7, 3)), s, np.full(7, 16), -2.0, 1)
    assert rows.tolist() == [6, 0, 3, 2, 1, 5]                                        # the NaN fails the threshold


def test_quantised_feature():
    """s = 1 lies in [2^0, 2^1): e = 1, scale 2^6, so 1 -> 64, 1/64 -> 1, 1/256 -> rint(0.25) = 0, -1 -> -64.  s = 0.99 lies in [2^-1, 2^0):
    e = 0, scale 2^7, 0.99 -> rint(126.72) = 127.  s = 2^-100 is coded (64 at its place), 2^-101 is not.  Ties go to even: with s = 1,
    f = 2.5 / 64 -> rint(2.5) = 2 and f = 3.5 / 64 -> 4.  s = 65504 lies in [2^15, 2^16): e = 16, scale 2^-9, 65504 -> rint(127.94) = 128,
    clamped to 127."""
    f = np.zeros((6, 8), np.float32)
    f[0, :4] = (1.0, 1 / 64, 1 / 256, -1.0)
    f[1, 0] = 0.99
    f[2, 0], f[3, 0] = 2.0 ** -100, 2.0 ** -101
    f[4, :3] = (1.0, 2.5 / 64, 3.5 / 64)
    f[5, :2] = (np.float32(65504.0), -1.0)                                            # the largest float16: e = 16, scale 2^-9
    q, nrm = R.quantise(f)
    assert q[0, :4].tolist() == [64, 1, 0, -64] and nrm[0] == 2 * 4096 + 1
    assert q[1, 0] == 127 and q[2, 0] == 64 and not q[3].any() and nrm[3] == 0
    assert q[4, :3].tolist() == [64, 2, 4]
    assert q[5, :2].tolist() == [127, 0] and np.array_equal(R.quantise(f.astype(np.float16))[0][5], q[5])
    assert R.fixed_point(np.array([[0.25, -1.5 / 1024, 2.5 / 1024]], np.float32)).tolist() == [[256, -2, 2]]     # rint: ties to even


def test_cosine_at_equality_and_beside_it():
    """One-hot a = (1, 0, ..): code 64, nrm_a = 4096.
    * b = (0.5, 0, ..): s = 0.5, e = 0, code 64, nrm_b = 4096, d = 4096.  sim = 1: s7 = 128; d d 16384 = 2^24 2^14 = 2^38 and
      s7 s7 nrm_a nrm_b = 2^14 2^12 2^12 = 2^38: equality, adjacent.
    * b = (1, 1/64, 0, ..): code (64, 1), nrm_b = 4097, d = 4096: 2^38 < 2^14 * 4096 * 4097: not adjacent at sim = 1.
    * b = (0.75, 1, 0, ..): code (48, 64), nrm_b = 6400, d = 3072, cosine 0.6.  d d 16384 = 154 618 822 656.  s7 = 76 (sim 0.59375):
      76^2 * 4096 * 6400 = 151 414 374 400 <= that: adjacent.  s7 = 77 (sim 0.6 -> round(76.8)): 155 425 177 600 > that: not adjacent."""
    a = K.E0[None]
    for b, sim, want, d_want, nrm_want in (([0.5, 0], 1.0, True, 4096, 4096), ([1.0, 1 / 64], 1.0, False, 4096, 4097),
                                           ([0.75, 1.0], 0.59375, True, 3072, 6400), ([0.75, 1.0], 0.6, False, 3072, 6400)):
        f = np.concatenate([a, np.array([b + [0] * 6], np.float32)])
        q, nrm = R.quantise(f)
        assert int(q[0].astype(np.int64) @ q[1].astype(np.int64)) == d_want and nrm.tolist() == [4096, nrm_want]
        r = R.rule(sim=sim)
        adj = R.adjacency_bits(np.zeros((2, 3), np.int32), q, nrm, r["radius_q"], r["sim_q"])
        assert adj.tolist() == [[False, want], [False, False]], (b, sim)
    assert 3072 * 3072 * 16384 == 154618822656 and 76 * 76 * 4096 * 6400 == 151414374400 and 77 * 77 * 4096 * 6400 == 155425177600
    assert R.rule(sim=0.6)["sim_q"] == 77 and R.rule(sim=0.59375)["sim_q"] == 76 and R.rule(sim=None)["sim_q"] == 0


def test_pre_cap_keeps_the_best_rows():
    n = R.MAX_ROWS + 10
    scores = np.full(n, 0.5, np.float32)
    scores[5], scores[n - 1] = 0.4, 0.9
    rows = R.ranked_rows(np.zeros((n, 3)), scores, np.full(n, 16), 0.3, 16)
    assert len(rows) == R.MAX_ROWS and rows[0] == n - 1 and rows[1] == 0 and 5 not in rows and rows[-1] == R.MAX_ROWS - 1


def test_room_finds_every_object():
    """On the room the restatement alone returns exactly K clusters, each holding the valid rows of one object: the chair next to the table
    (0.15 m, unlike features) and the two like chairs 3 m apart stay apart.  The GPU test relies on this."""
    for dtype in (np.float16, np.float32):
        case = K.room(dtype)
        got = _run(case)
        obj, labels = case["obj"], got["labels"]
        assert len(got["seeds"]) == K.ROOM_K
        assert np.array_equal(labels >= 0, obj >= 0)
        for k in range(K.ROOM_K):
            rows = np.nonzero(labels == k)[0]
            assert len(set(obj[rows].tolist())) == 1 and len(rows) == int((obj == obj[rows[0]]).sum()) >= 5
            assert got["views"][k] == len(rows)                                       # one slot per object and frame
        # distance alone chains the chair into the table; the cosine alone joins the two like chairs
        assert len(_run(case, sim=None)["seeds"]) == K.ROOM_K - 1
        assert len(_run(case, radius=5.0)["seeds"]) == K.ROOM_K - 1
        more = int(got["views"].min()) + 1
        assert len(_run(case, min_views=more)["seeds"]) == int((got["views"] >= more).sum()) < K.ROOM_K
        capped = _run(case, max_queries=5)
        best = sorted(range(K.ROOM_K), key=lambda i: (-got["scores"][i], got["seeds"][i]))[:5]
        assert capped["seeds"].tolist() == sorted(got["seeds"][best].tolist())


def test_recorded_dev32_is_current():
    assert abs(K.dev32() - K.DEV32) <= 0.001 * K.DEV32, f"DEV32 is {K.dev32():.3e}: update tests/merge_queries_case.py and profiles/merge_queries.md"
