"""Test cases of the query merging (segdino3d_amd/lift_queries.py `merge_queries`), built on the CPU and shared by the CPU and the GPU
tests (read-only).

Hand cases: eight channels, expectations written out by hand in HAND_CASES (tests/test_merge_queries_ref.py holds the restatement to
them, the GPU test holds the kernels to the restatement).  Room: K objects seen from V frames, one query slot per object and frame,
with centre noise, feature noise, unseen slots, weak scores, two objects 0.15 m apart with unlike features and two objects with the
same feature 3 m apart.  Rows: `n` rows that are all valid, drawn from K objects on a 1 m grid, for the sweeps over M and C.

`python tests/merge_queries_case.py` prints DEV32, the largest deviation of the restatement's feature mean evaluated sequentially in
float32 from the same mean in float64 over all these cases."""
import functools

import numpy as np

import merge_queries_ref as R

DEV32 = 4.519e-06      # `python tests/merge_queries_case.py`; profiles/merge_queries.md, "tolerance"
HAND_RULE = dict(score_thr=0.0, min_pixels=1)
C_HAND = 8


def _f(*pairs):
    """A feature row of eight channels from (channel, value) pairs."""
    f = np.zeros(C_HAND, np.float32)
    for ch, v in pairs:
        f[ch] = v
    return f


def _case(name, xs, feats, scores, rule, expect, count=None, Q=1):
    centre = np.array([x if isinstance(x, tuple) else (x, 0.0, 0.0) for x in xs], np.float32).reshape(-1, 3)
    n = len(centre)
    feats = np.stack(feats).astype(np.float32) if n else np.zeros((0, C_HAND), np.float32)
    count = np.full(n, 16, np.int32) if count is None else np.array(count, np.int32)
    return dict(name=name, feats=feats, centre=centre, scores=np.array(scores, np.float32), count=count, Q=Q, rule={**HAND_RULE, **rule},
                expect=expect)


E0 = _f((0, 1.0))
CHAIN_X = [0.0, 0.25, 0.5]                                       # p = 0, 256, 512; r_q = round(0.3 * 1024) = 307: A~B, B~C, A!~C
CHAIN = dict(radius=0.3, sim=None)
NAN, INF = float("nan"), float("inf")


def hand_cases():
    """-> the list of cases; `expect` holds labels (and seeds, views, scores, pos, feats where given)."""
    cases = [
        # leader clustering is not a transitive closure
        _case("chain, A on top", CHAIN_X, [E0] * 3, [0.9, 0.8, 0.7], CHAIN, dict(labels=[0, 0, 1], seeds=[0, 2], views=[2, 1])),
        _case("chain, B on top", CHAIN_X, [E0] * 3, [0.8, 0.9, 0.7], CHAIN, dict(labels=[0, 0, 0], seeds=[1], views=[3], scores=[0.9])),
        _case("chain, C on top", CHAIN_X, [E0] * 3, [0.7, 0.8, 0.9], CHAIN, dict(labels=[0, 1, 1], seeds=[0, 2], views=[1, 2])),
        _case("equal scores: ties to the lower row", CHAIN_X, [E0] * 3, [0.5, 0.5, 0.5], CHAIN, dict(labels=[0, 0, 1], seeds=[0, 2])),
        # +0 sorts before -0: B is the seed
        _case("signed zeros", CHAIN_X, [E0] * 3, [-0.0, 0.0, -0.0], dict(CHAIN, score_thr=-1.0), dict(labels=[0, 0, 0], seeds=[1], scores=[0.0])),
        # r_q = 256: 256^2 <= 256^2 merges, 257^2 > 256^2 does not
        _case("distance exactly r_q", [0.0, 0.25], [E0] * 2, [0.9, 0.8], dict(radius=0.25, sim=None), dict(labels=[0, 0], seeds=[0])),
        _case("distance r_q + 1", [0.0, 257 / 1024], [E0] * 2, [0.9, 0.8], dict(radius=0.25, sim=None), dict(labels=[0, 1], seeds=[0, 1])),
        # p = (192, 144, 0) against the origin: 192^2 + 144^2 = 57600 = 240^2
        _case("diagonal distance exactly r_q", [0.0, (0.1875, 0.140625, 0.0)], [E0] * 2, [0.9, 0.8], dict(radius=240 / 1024, sim=None),
              dict(labels=[0, 0], seeds=[0])),
        _case("diagonal distance, r_q one less", [0.0, (0.1875, 0.140625, 0.0)], [E0] * 2, [0.9, 0.8], dict(radius=239 / 1024, sim=None),
              dict(labels=[0, 1], seeds=[0, 1])),
        # cosine, see test_cosine_at_equality_and_beside_it for the arithmetic
        _case("cosine at equality", [0.0, 0.0], [E0, _f((0, 0.5))], [0.9, 0.8], dict(sim=1.0), dict(labels=[0, 0], seeds=[0])),
        _case("cosine one unit off", [0.0, 0.0], [E0, _f((0, 1.0), (1, 1 / 64))], [0.9, 0.8], dict(sim=1.0), dict(labels=[0, 1], seeds=[0, 1])),
        _case("cosine 0.6 against s7 = 76", [0.0, 0.0], [E0, _f((0, 0.75), (1, 1.0))], [0.9, 0.8], dict(sim=0.59375), dict(labels=[0, 0], seeds=[0])),
        _case("cosine 0.6 against s7 = 77", [0.0, 0.0], [E0, _f((0, 0.75), (1, 1.0))], [0.9, 0.8], dict(sim=0.6), dict(labels=[0, 1], seeds=[0, 1])),
        _case("opposite features", [0.0, 0.0], [E0, _f((0, -1.0))], [0.9, 0.8], dict(sim=0.01), dict(labels=[0, 1], seeds=[0, 1])),       # d < 0
    ]
    bad = [E0, _f((0, 1.0), (3, NAN)), _f((0, 1.0), (5, INF)), _f(), E0]
    for sim in (0.75, None):                                     # a zero code is adjacent to nothing, with or without the cosine test
        cases.append(_case(f"NaN, Inf and all-zero features, sim {sim}", [0.0] * 5, bad, [0.9, 0.8, 0.7, 0.6, 0.5], dict(sim=sim),
                           dict(labels=[0, 1, 2, 3, 0], seeds=[0, 1, 2, 3], views=[2, 1, 1, 1])))
    cases.append(_case("non-finite and out-of-world centres", [0.0, NAN, (0.0, INF, 0.0), (0.0, 0.0, 16384.0), 0.0, (0.0, 0.0, -16383.0)], [E0] * 6,
                       [0.9, 0.8, 0.7, 0.6, 0.5, 0.4], dict(), dict(labels=[0, -1, -1, -1, 0, 1], seeds=[0, 5])))
    # two frames' worth of two slots each, and a fifth row: X = rows 0, 1 (both frame 0), Y = rows 2 (frame 1), 4 (frame 2), Z = row 3
    frames = dict(xs=[0.0, 0.0, 1.0, 5.0, 1.125], feats=[E0, E0, E0, E0, _f((0, 2.0))], scores=[0.9, 0.5, 0.8, 0.7, 0.6], count=[16, 16, 16, 16, 48], Q=2)
    # Y: sum w p = 16 * 1024 + 48 * 1152 = 71680, sum w = 64 -> 1120 / 1024 = 1.09375; feature (16 * 1 + 48 * 2) / 64 = 1.75
    y_pos, y_feat = (1.09375, 0.0, 0.0), _f((0, 1.75))
    cases += [
        _case("two members in one frame", rule=dict(), expect=dict(labels=[0, 0, 1, 2, 1], seeds=[0, 2, 3], views=[1, 2, 1], scores=[0.9, 0.8, 0.7],
                                                                    pos=[(0, 0, 0), y_pos, (5, 0, 0)], feats=[E0, y_feat, E0]), **frames),
        _case("min_views = 2", rule=dict(min_views=2), expect=dict(labels=[-1, -1, 0, -1, 0], seeds=[2], views=[2], pos=[y_pos], feats=[y_feat]), **frames),
        _case("max_queries = 2", rule=dict(max_queries=2), expect=dict(labels=[0, 0, 1, -1, 1], seeds=[0, 2], views=[1, 2]), **frames),
        _case("max_queries = 1", rule=dict(max_queries=1), expect=dict(labels=[0, 0, -1, -1, -1], seeds=[0], views=[1]), **frames),
        _case("max_queries = 0", rule=dict(max_queries=0), expect=dict(labels=[-1] * 5, seeds=[]), **frames),
        _case("reduce = best", rule=dict(reduce="best"), expect=dict(labels=[0, 0, 1, 2, 1], seeds=[0, 2, 3], feats=[E0, E0, E0]), **frames),
        _case("score threshold", rule=dict(score_thr=0.65), expect=dict(labels=[0, -1, 1, 2, -1], seeds=[0, 2, 3], views=[1, 1, 1]), **frames),
        _case("min_pixels", rule=dict(min_pixels=17), expect=dict(labels=[-1, -1, -1, -1, 0], seeds=[4], views=[1]), **frames),
        _case("n = 0", [], [], [], dict(), dict(labels=[], seeds=[])),
    ]
    # the weight of a member is capped at 2^20: (2^20 * 0 + 2^20 * 256) / 2^21 = 128 -> 0.125
    cases.append(_case("weight cap", [0.0, 0.25], [E0, E0], [0.9, 0.8], dict(radius=0.3, sim=None), dict(labels=[0, 0], seeds=[0], pos=[(0.125, 0, 0)]),
                       count=[2 ** 20, 2 ** 30]))
    return cases


# ---------------------------------------------------------------------------------------------- the room and the row sweeps
ROOM_K, ROOM_V, ROOM_C = 12, 20, 64
ROOM_RULE = dict()                                               # the defaults: radius 0.3, sim 0.75, score_thr 0.3, min_pixels 16


def _freeze(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _objects(rng, K, C):
    k = np.arange(K)
    centre = np.stack([k % 8, (k // 8) % 8, k // 64], axis=1).astype(np.float64)       # a 1 m grid
    return centre, rng.standard_normal((K, C))


@functools.lru_cache(maxsize=None)
def room(dtype=np.float16, seed=11):
    """-> dict(feats [V K, C], centre, scores, count, Q = K, obj int [V K]: the object behind each row, -1 where the row is not valid)."""
    rng = np.random.default_rng(seed)
    K, V, C = ROOM_K, ROOM_V, ROOM_C
    oc, of = _objects(rng, K, C)
    oc[1] = oc[0] + (0.15, 0.0, 0.0)                                                   # a chair next to a table: unlike features
    oc[3], of[3] = oc[2] + (0.0, 3.0, 0.0), of[2]                                      # the same chair twice, 3 m apart
    obj = np.tile(np.arange(K), V)
    centre = (oc[obj] + rng.uniform(-0.04, 0.04, (V * K, 3))).astype(np.float32)
    feats = (of[obj] + 0.1 * rng.standard_normal((V * K, C))).astype(dtype)
    scores = (rng.integers(20, 64, V * K) / 64).astype(np.float32)                     # 0.3125 .. 0.984 in steps of 1 / 64: ties abound
    count = rng.integers(16, 3000, V * K).astype(np.int32)
    unseen, weak = rng.random(V * K) < 0.3, rng.random(V * K) < 0.1
    count[unseen] = rng.integers(0, 16, int(unseen.sum()))
    scores[weak] = np.float32(0.25)
    obj = np.where(unseen | weak, -1, obj)
    return _freeze(dict(name=f"room {np.dtype(dtype).name}", feats=feats, centre=centre, scores=scores, count=count, Q=K, rule=dict(ROOM_RULE), obj=obj))


@functools.lru_cache(maxsize=None)
def rows_case(n, C, dtype=np.float16, K=20, Q=5, seed=7, tile=1, spread=0.04):
    """`n` valid rows drawn from K objects (K = None: every row an object of its own, no two adjacent), tiled `tile` times."""
    rng = np.random.default_rng(seed + 1000 * n + C)
    oc, of = _objects(rng, n if K is None else K, C)
    obj = np.arange(n) if K is None else rng.integers(0, K, n)
    centre = (oc[obj] + rng.uniform(-spread, spread, (n, 3))).astype(np.float32)
    feats = (of[obj] + 0.1 * rng.standard_normal((n, C))).astype(dtype)
    scores = (rng.integers(20, 64, n) / 64).astype(np.float32)
    count = rng.integers(16, 3000, n).astype(np.int32)
    if n:
        count[rng.integers(0, n)] = 2 ** 21                                            # one weight beyond the cap
    t = lambda a: np.tile(a, (tile,) + (1,) * (a.ndim - 1))
    return _freeze(dict(name=f"rows n={n * tile} C={C} {np.dtype(dtype).name} K={K}", feats=t(feats), centre=t(centre), scores=t(scores),
                        count=t(count), Q=Q, rule=dict(ROOM_RULE)))


M_SWEEP = [1, 2, 63, 64, 65, 129, 1000]
C_SWEEP = [8, 64, 72, 256, 1024]
BIG_TILE = (1100, 16)                                            # 17600 valid rows: the 16384 best enter


def sweep_cases():
    """(id, case) of the GPU test's sweeps; the restatement of each is computed once (`reference`)."""
    out = [(f"M{m}", rows_case(m, 64)) for m in M_SWEEP]
    out += [(f"C{c}-{np.dtype(dt).name}", rows_case(200, c, dt)) for c in C_SWEEP for dt in (np.float16, np.float32)]
    out += [("one-cluster", rows_case(200, 64, K=1)), ("none-adjacent", rows_case(129, 64, K=None)),
            ("pre-cap", rows_case(BIG_TILE[0], 8, np.float32, tile=BIG_TILE[1])), ("room-f16", room(np.float16)), ("room-f32", room(np.float32))]
    return out


_REF = {}


def reference(case, feat_dtype=np.float64, **kw):
    """The restatement of a shared case (with rule overrides `kw`), computed once."""
    key = (case["name"], np.dtype(feat_dtype).name, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = R.merge(case["feats"], case["centre"], case["scores"], case["count"], case["Q"], feat_dtype=feat_dtype, **{**case["rule"], **kw})
    return _REF[key]


def dev32():
    """The largest deviation of the sequential float32 feature mean from the float64 one over the hand cases, the room and the sweeps."""
    worst = 0.0
    for case in hand_cases() + [c for _, c in sweep_cases()]:
        a, b = reference(case), reference(case, np.float32)
        assert np.array_equal(a["labels"], b["labels"])
        both = np.isfinite(a["feats"]) & np.isfinite(b["feats"])
        if both.any():
            worst = max(worst, float(np.abs(a["feats"][both] - b["feats"][both].astype(np.float64)).max()))
    return worst


if __name__ == "__main__":                     # the figure of profiles/merge_queries.md, "tolerance"
    for name, case in sweep_cases():
        ref = reference(case)
        print(f"{name}: {len(case['scores'])} rows -> {len(ref['seeds'])} clusters, largest {max((len(m) for m in ref['members']), default=0)} members")
    d = dev32()
    print(f"DEV32 = {d:.3e}; bound of the merged features = 4 x that = {4 * d:.3e}")
