"""Every kernel of `segdino3d_amd/csrc/post.hip` on the evaluation path against its plain restatement in tests/post_ref.py (pinned to
the oracle by tests/test_post_ref_oracle.py), through the `ops.*` wrappers, at the smallest shapes that cross the kernels' own
structure: 64-lane waves, 4 rows per workgroup, 16 NMS row lanes, 32-row words, 4 words per block, 4 points per thread, 1024 points
per workgroup.

Float outputs: within max(8 ulp of fp32, 4 x e32) relative of the float64 restatement, where e32 is the error of the SAME expression
evaluated in fp32 by torch on the CPU (the factor 4 pays for another summation order - 64-lane strided sum plus butterfly - and
another expf), plus 1e-37 absolute for values that underflow; the bound itself must not exceed 1e-5.  Discrete outputs: exact.
Measured errors: every case prints a `[post-kernel-error]` line; profiles/post_kernel_errors.md holds the table."""
import numpy as np
import pytest
import torch

import post_ref as R

pytestmark = pytest.mark.gpu

FLOOR = 1e-37
BOUND_CAP = 1e-5


def _dev():
    return torch.device("cuda:0")


def _rel(a, ref):
    """Largest (|a - ref| - FLOOR)+ / |ref| over the finite non-zero entries of ref."""
    a, ref = a.double().reshape(-1), ref.double().reshape(-1)
    ok = torch.isfinite(ref) & (ref != 0)
    if not bool(ok.any()):
        return 0.0
    return float((((a[ok] - ref[ok]).abs() - FLOOR).clamp(min=0) / ref[ok].abs()).max())


def check_float(family, case, got, ref64, ref32):
    """The tolerance rule of the module docstring; non-finite entries (and exact zeros) must be the reference's."""
    got, ref64, ref32 = got.detach().cpu().double().reshape(-1), ref64.double().reshape(-1), ref32.double().reshape(-1)
    assert got.shape == ref64.shape
    e32 = _rel(ref32, ref64)
    bound = max(8 * R.ULP32, 4 * e32)
    kerr = _rel(got, ref64)
    print(f"[post-kernel-error] {family} | {case} | kernel {kerr:.3e} | e32 {e32:.3e} | bound {bound:.3e}")
    assert bound <= BOUND_CAP, (family, case, bound)
    fin = torch.isfinite(ref64)
    assert torch.equal(torch.isnan(got), torch.isnan(ref64)), (family, case, "NaN set")
    inf = torch.isinf(ref64)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], ref64[inf]), (family, case, "infinities")
    assert bool(((got[fin] - ref64[fin]).abs() <= bound * ref64[fin].abs() + FLOOR).all()), (family, case, kerr, bound)
    return kerr, e32, bound


# ---- class_scores -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 18, 63, 64, 65, 198])
def test_class_scores(C):
    from segdino3d_amd import ops
    d = _dev()
    for Q in (1, 3, 4, 5, 200):
        for pad in (0, 3):
            g = torch.Generator().manual_seed(1000 * C + 10 * Q + pad)
            full = 4.0 * torch.randn(Q, C + 1 + pad, generator=g)
            if pad:
                full[:, C + 1:] = 1e4                                      # columns behind the row: must not be read
            cls = full[:, :C + 1]
            rows = torch.randperm(Q, generator=g).tolist()
            if C >= 2:
                r = rows[0]
                cls[r, :] = torch.where(torch.rand(C + 1, generator=g) < 0.5, 80.0, -80.0)      # +-80 in one row
                cls[r, 0], cls[r, 1] = 80.0, -80.0
            if len(rows) > 1:
                cls[rows[1], :] = 1.25                                     # a constant row
            if len(rows) > 2:
                cls[rows[2], -1] = 50.0                                    # the no-object column is the largest: rowmax ignores it
            if len(rows) > 3 and C >= 2:
                cls[rows[3], 1::2] = float("-inf")                         # -inf entries (column 0 stays finite)
            p64, m64 = R.class_scores_ref(cls, C)
            p32, m32 = R.class_scores_ref(cls, C, torch.float32)
            dev_cls = full.to(d)[:, :C + 1]
            assert dev_cls.stride(0) == C + 1 + pad
            case = f"Q={Q} C={C} ld={C + 1 + pad}"
            s, m = ops.class_scores(dev_cls, C, want_scores=True, want_rowmax=True)
            check_float("class_scores", case + " scores", s, p64, p32)
            check_float("class_scores", case + " rowmax", m, m64, m32)
            assert torch.equal(m, s.view(Q, C).max(1)[0])                  # the row maximum is one of the scores
            s1, none = ops.class_scores(dev_cls, C, want_scores=True, want_rowmax=False)
            assert none is None and torch.equal(s1, s)
            none, m1 = ops.class_scores(dev_cls, C, want_scores=False, want_rowmax=True)
            assert none is None and torch.equal(m1, m)


# ---- mask_scores --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 63, 64, 65, 96, 500])
def test_mask_scores(S):
    from segdino3d_amd import ops
    d = _dev()
    Q = 7
    for C in (1, 198):
        for n in (1, 4, 5, 600):
            for pad in (0, 5):
                g = torch.Generator().manual_seed(100 * S + 10 * n + C + pad)
                full = 3.0 * torch.randn(Q, S + pad, generator=g)
                if pad:
                    full[:, S:] = 50.0                                     # behind the row: must not be read
                masks = full[:, :S]
                masks[0] = -masks[0].abs() - 0.1                           # no positive logit: score exactly 0
                masks[1] = torch.where(torch.rand(S, generator=g) < 0.5, 0.0, -0.0)          # +-0.0 are not positive
                if S > 1:
                    masks[2, ::2] = 0.0                                    # zeros among positives and negatives
                    masks[2, 1::4] = -0.0
                flat_idx = torch.randint(0, Q * C, (n,), generator=g, dtype=torch.int32)      # several entries per query
                for i in range(min(n, 3)):
                    flat_idx[(7 * i) % n] = i * C + int(torch.randint(0, C, (1,), generator=g))
                score_in = torch.rand(n, generator=g)
                lab, q, s64 = R.mask_scores_ref(masks, flat_idx, score_in, C, True)
                _, _, s32 = R.mask_scores_ref(masks, flat_idx, score_in, C, True, torch.float32)
                dm = full.to(d)[:, :S]
                glab, gq, gs = ops.mask_scores(dm, S, flat_idx.to(d), score_in.to(d), C, True)
                assert torch.equal(glab.cpu().long(), lab) and torch.equal(gq.cpu().long(), q)
                check_float("mask_scores", f"S={S} n={n} C={C} ld={S + pad}", gs, s64, s32)
                # rows without a positive logit: exactly 0 (they also carry the check of the 1e-6 in the denominator: without it 0 / 0)
                zero = s64 == 0
                assert bool(zero.any()) and bool((gs.cpu()[zero] == 0).all())
                glab, gq, gs = ops.mask_scores(dm, S, flat_idx.to(d), score_in.to(d), C, False)
                assert torch.equal(glab.cpu().long(), lab) and torch.equal(gq.cpu().long(), q)
                assert torch.equal(gs.cpu(), score_in)                     # normalize=False: bit for bit


# ---- gather_sigmoid -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 33, 96, 500])
def test_gather_sigmoid(S):
    from segdino3d_amd import ops
    d = _dev()
    Q, ld_out = 9, (S + 31) // 32 * 32
    for n in (1, 5, 130):
        for pad in (0, 7):
            g = torch.Generator().manual_seed(100 * S + n + pad)
            full = 3.0 * torch.randn(Q, S + pad, generator=g)
            if pad:
                full[:, S:] = 5.0                                          # behind the row: the pad of the output must still be 0
            masks = full[:, :S]
            masks[0, 0], masks[1, -1] = 100.0, -100.0
            if S > 2:
                masks[2, ::3], masks[2, 1::3] = 100.0, -100.0
            qidx = torch.randint(0, Q, (n,), generator=g, dtype=torch.int32)                  # repeats
            qidx[: min(n, 3)] = torch.arange(min(n, 3), dtype=torch.int32)
            order = torch.randperm(n, generator=g).to(torch.int32)
            s64, a64 = R.gather_sigmoid_ref(masks, S, qidx, order, ld_out)
            s32, a32 = R.gather_sigmoid_ref(masks, S, qidx, order, ld_out, torch.float32)
            sig, area = ops.gather_sigmoid(full.to(d)[:, :S], S, qidx.to(d), order.to(d), ld_out)
            assert sig.shape == (n, ld_out)
            assert bool((sig[:, S:] == 0).all())                           # pad columns exactly 0
            case = f"S={S} n={n} ld={S + pad}"
            check_float("gather_sigmoid", case + " sig", sig, s64, s32)
            check_float("gather_sigmoid", case + " area", area, a64, a32)


# ---- nms_decay ----------------------------------------------------------------------------------------------------------------------------
def _nms_case(n, S, pattern, plant, seed):
    """inter / area in float64 from U(0,1) rows, rounded to fp32 (kernel and reference read the same values); scores descending.
    plant: None | "iou1" | ("nan", t) | "lanes"."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.rand(n, S, generator=g, dtype=torch.float64)
    inter, area = (rows @ rows.t()).float(), rows.sum(1).float()
    scores = torch.sort(torch.rand(n, generator=g), descending=True)[0]
    labels = {"distinct": torch.randperm(n, generator=g), "equal": torch.full((n,), 3),
              "five": torch.randint(0, 5, (n,), generator=g)}[pattern].to(torch.int32)
    a, b = (0, n - 1) if n < 20 else (n // 3, n // 3 + 17)                # 17 apart: two different row lanes of the 16-way split
    if plant == "iou1":                                                    # IoU exactly 1: the linear kernel divides by 1 - 1
        labels[b] = labels[a]
        for r in (a, b):                                                   # two small masks: their other intersections shrink with them
            inter[r, :] *= 8.0 / area[r]
            inter[:, r] = inter[r, :]
        inter[a, b] = inter[b, a] = area[a] = area[b] = 8.0
    if isinstance(plant, tuple):                                           # IoU 0 / 0 between rows a and b
        if n >= 48:                                                        # ... which sit in row lanes t and (t + 5) % 16
            a, b = plant[1], 16 + (plant[1] + 5) % 16
        labels[b] = labels[a]
        inter[a, :] = inter[:, a] = inter[b, :] = inter[:, b] = 0.0
        area[a] = area[b] = 0.0
    if plant == "lanes":
        # every row lane decides something: for t = 0 .. 15 the rows i = t < j = 16 + (t + 5) % 16 < k = 32 + t carry one label;
        # IoU(i, j) = 0.7 makes comp[j] (found by row lane t alone: the other IoUs are about 1/3), IoU(j, k) = 0.9 makes row j (row
        # lane (t + 5) % 16) the minimum of column k: coef[k] = decay(0.9) / decay(0.7), below every other ratio of the column
        assert n >= 48 and pattern == "equal"
        for t in range(16):
            i, j, k = t, 16 + (t + 5) % 16, 32 + t
            for (p, q, iou) in ((i, j, 0.7), (j, k, 0.9)):
                inter[p, q] = inter[q, p] = iou * (area[p] + area[q]) / (1.0 + iou)
    return inter, area, labels, scores


def _plants(n, pattern):
    if n < 2 or pattern == "distinct":
        return [None]
    plants = [None, "iou1", ("nan", 0)]
    if n >= 48 and pattern == "equal":
        plants += [("nan", t) for t in range(1, 16)] + ["lanes"]
    return plants


@pytest.mark.parametrize("kernel,sigma", [("linear", 2.0), ("gaussian", 2.0), ("gaussian", 0.5)])
@pytest.mark.parametrize("n", [1, 2, 16, 17, 63, 64, 65, 130, 600])
def test_nms_decay(kernel, sigma, n):
    from segdino3d_amd import ops
    d = _dev()
    S = 500 if n == 600 else 96
    for pattern in ("distinct", "equal", "five"):
        for plant in _plants(n, pattern):
            for pad in (0, 5):
                inter, area, labels, scores = _nms_case(n, S, pattern, plant, 10 * n + pad)
                ref64 = R.nms_decay_ref(inter, area, labels, scores, kernel, sigma)
                ref32 = R.nms_decay_ref(inter, area, labels, scores, kernel, sigma, torch.float32)
                wide = torch.full((n, n + pad), 1e9)                       # behind the row: must not be read
                wide[:, :n] = inter
                got = ops.nms_decay(wide.to(d)[:, :n] if pad else inter.to(d), area.to(d), labels.to(d), scores.to(d), kernel, sigma)
                tag = f"nan lane {plant[1]}" if isinstance(plant, tuple) else plant
                case = f"{kernel} sigma={sigma} n={n} ld={n + pad} labels={pattern} plant={tag}"
                check_float("nms_decay", case, got, ref64, ref32)
                if pattern == "distinct":
                    assert torch.equal(got.cpu(), scores)                  # coefficient exactly 1: bit for bit
                elif plant is None and n >= 16 and pattern == "equal":
                    assert float((ref64 / scores.double()).min()) < 0.97   # something is decayed
                if isinstance(plant, tuple):
                    assert bool(torch.isnan(ref64).any())
                if plant == "iou1" and kernel == "linear":
                    assert bool((ref64 == 0).any()) and bool((got.cpu()[ref64 == 0] == 0).all())
                if plant == "lanes":                                       # the planted rows decide their columns, as designed
                    decay = (lambda x: 1 - x) if kernel == "linear" else (lambda x: float(np.exp(-sigma * x * x)))
                    coef = (ref64 / scores.double())[32:48]
                    assert bool(((coef - decay(0.9) / decay(0.7)).abs() < 1e-3).all()), coef


# ---- row_argmax, gather_i64 -----------------------------------------------------------------------------------------------------------------
def _plant_argmax_rows(x, ncols, g):
    """Special rows over the first ncols columns of x (as many as x has rows), most important first."""
    nan, inf = float("nan"), float("inf")
    c0 = int(torch.randint(0, ncols, (1,), generator=g))

    def all_nan(r): x[r, :ncols] = nan

    def one_nan(r): x[r, c0] = nan

    def some_nan(r): x[r, c0:ncols:3] = nan

    def all_ninf(r): x[r, :ncols] = -inf

    def tie_lanes(r): x[r, max(c0 - 1, 0)], x[r, c0] = 100.0, 100.0      # neighbouring lanes: decided in the butterfly

    def tie_stride(r): x[r, c0 % 64::64] = 100.0                           # columns c, c + 64, ...: one lane's loop

    def nan_and_inf(r): x[r, ncols - 1], x[r, 0] = nan, inf                # +inf before a NaN: the NaN wins

    def nan_stride(r): x[r, c0 % 64::64] = nan                             # NaNs in one lane: the lowest column

    def constant(r): x[r, :ncols] = -2.5
    for r, f in enumerate((all_nan, one_nan, some_nan, all_ninf, tie_lanes, tie_stride, nan_and_inf, nan_stride, constant)):
        if r < x.shape[0]:
            f(r)
            x[r, ncols:] = 1e9


@pytest.mark.parametrize("ncols", [1, 2, 63, 64, 65, 200])
def test_row_argmax_first_columns(ncols):
    from segdino3d_amd import ops
    d = _dev()
    for Q in (1, 4, 5, 3000):
        for rot in range(3 if Q < 3000 else 1):                           # small Q: rotate through the special rows
            g = torch.Generator().manual_seed(ncols * 7 + Q + rot)
            x = torch.randn(Q + 3 * rot, ncols + 1, generator=g)
            x[:, ncols] = 1e9                                              # the column behind the list: must be ignored
            _plant_argmax_rows(x, ncols, g)
            x = x[3 * rot:].contiguous()
            ref = R.row_argmax_ref(x, ncols=ncols)
            got = ops.row_argmax(x.to(d), ncols=ncols)
            assert got.dtype == torch.int64 and torch.equal(got.cpu(), ref), (ncols, Q, rot)
            assert int(got.min()) >= 0 and int(got.max()) < ncols


@pytest.mark.parametrize("cols", [[0, 1], [5, 2, 9], [70, 3, 3, 199, 64] + list(range(100, 170))])
def test_row_argmax_column_list(cols):
    """The result is the position in the list, ties and NaNs go to the lowest position."""
    from segdino3d_amd import ops
    d = _dev()
    g = torch.Generator().manual_seed(len(cols))
    Q, width = 300, 201
    x = torch.randn(Q, width, generator=g)
    x[:, [c for c in range(width) if c not in cols]] = 1e9                # unlisted columns: must be ignored
    sub = x[:, cols].clone()
    _plant_argmax_rows(sub, len(cols), g)
    for pos in reversed(range(len(cols))):                                 # a repeated column keeps the value of its first position
        x[:, cols[pos]] = sub[:, pos]
    ref = R.row_argmax_ref(x, cols=cols)
    got = ops.row_argmax(x.to(d), cols=torch.tensor(cols, dtype=torch.int32, device=d))
    assert torch.equal(got.cpu(), ref)
    assert len(set(ref.tolist())) > 1 and int(got.max()) < len(cols)


@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_gather_i64(N):
    from segdino3d_amd import ops
    d = _dev()
    g = torch.Generator().manual_seed(N)
    table = torch.randint(-2 ** 40, 2 ** 40, (37,), generator=g)
    idx = torch.randint(0, 37, (N,), generator=g)
    assert torch.equal(ops.gather_i64(table.to(d), idx.to(d), True).cpu(), table[idx])
    assert torch.equal(ops.gather_i64(table.to(d), idx.to(d), False).cpu(), table[torch.zeros_like(idx)])


# ---- MaskBits, MaskBits.rows ----------------------------------------------------------------------------------------------------------------
def _expand_case(N, n, with_boxes):
    g = torch.Generator().manual_seed(1000 * N + n)
    W, S_real, thr = 96, 90, np.float32(0.4)
    sig = torch.rand(n, W, generator=g)
    sig[:, S_real:] = 0.0
    sig[torch.rand(n, W, generator=g) < 0.05] = float(thr)                 # exactly the fp32 threshold: not set
    src = torch.randperm(n, generator=g).to(torch.int32)
    sp = torch.randint(0, S_real - 2, (N,), generator=g)                   # ids 88 and 89 never occur
    for i, v in enumerate((-1, W, W - 1, 2 ** 33 + 5, -2 ** 40)):          # out of range -> 0; W - 1 is a pad column of zeros
        if N > 16 or i < N - 2:
            sp[(3 * i + 1) % N] = v
    pts = torch.rand(N, 6, generator=g) * 4.1 + 0.013                      # non-dyadic coordinates
    boxes = None
    if with_boxes:
        boxes = torch.cat([torch.rand(n, 3, generator=g) * 4.1, torch.rand(n, 3, generator=g) * 1.7], 1)
        # final row 0: a box of size zero around point N // 2 (and its copy, if there is room); its sig row is on everywhere
        sig[src[0], :S_real] = 0.9
        boxes[0, :3], boxes[0, 3:] = pts[N // 2, :3], 0.0
        if N > 8:
            pts[N // 2 + 3, :3] = pts[N // 2, :3]
        if n > 1 and N > 2:
            # final row 1: centre 2, size 1 -> faces at 2 -+ 1.25 exactly; points on the faces are inside, the next fp32 outside is not
            sig[src[1], :S_real] = 0.9
            boxes[1] = torch.tensor([2.0, 2.0, 2.0, 1.0, 1.0, 1.0])
            lo, hi = np.float32(0.75), np.float32(3.25)
            faces = [(0, hi), (0, lo), (1, hi), (2, lo), (0, np.nextafter(hi, np.float32(9))), (0, np.nextafter(lo, np.float32(-9))),
                     (1, np.nextafter(hi, np.float32(9))), (2, np.nextafter(lo, np.float32(-9)))]
            for i, (axis, v) in enumerate(faces):
                p = (5 * i + 2) % N
                if p == N // 2 or (N > 8 and p == N // 2 + 3):
                    continue
                pts[p, :3] = 2.0
                pts[p, axis] = float(v)
    return sig, src, sp, pts, boxes, float(thr)


@pytest.mark.parametrize("with_boxes", [False, True])
@pytest.mark.parametrize("N", [1, 3, 4, 5, 1023, 1024, 1025, 4099])
def test_mask_bits_rows_and_counts(N, with_boxes):
    """`MaskBits(...).count` and `MaskBits(...).rows` (the whole table among the lists) against `expand_masks_ref`: bytes and counts exact."""
    from segdino3d_amd import ops
    d = _dev()
    for n in (1, 31, 32, 33, 127, 128, 129):
        sig, src, sp, pts, boxes, thr = _expand_case(N, n, with_boxes)
        ref, ref_count = R.expand_masks_ref(sig.numpy(), src.numpy(), sp.numpy(), pts.numpy(), thr, None if boxes is None else boxes.numpy())
        if with_boxes and N >= 1023:
            plain, _ = R.expand_masks_ref(sig.numpy(), src.numpy(), sp.numpy(), pts.numpy(), thr)
            assert 0 < ref.sum() < plain.sum() and ref[0].sum() >= 1       # the filter cuts, the zero-size box keeps its centre
        dsig, dsrc, dsp, dpts = sig.to(d), src.to(d), sp.to(d), pts.to(d)
        dbox = None if boxes is None else boxes.to(d)
        mb = ops.MaskBits(dsig, dsrc, dsp, dpts, thr, dbox)
        assert np.array_equal(mb.count.cpu().numpy().astype(np.int64), ref_count), (N, n, "MaskBits count")
        lists = ([], [0], [n - 1, 0, 0, n // 2], list(range(n)), list(range(n))[::-1], [n // 2, n // 3, n - 1, 31 % n, 32 % n, 33 % n, 96 % n])
        for rows in lists:
            got = mb.rows(torch.tensor(rows, dtype=torch.int32, device=d))
            assert got.shape == (len(rows), N)
            assert np.array_equal(got.cpu().numpy(), ref[rows].reshape(len(rows), N)), (N, n, rows[:8])


# ---- panoptic -----------------------------------------------------------------------------------------------------------------------------
def _panoptic_case(N, n, n_stuff):
    g = torch.Generator().manual_seed(100 * N + 10 * n + n_stuff)
    M = n + 7                                                              # the candidates are a subset of a larger table
    density = 0.02 + 0.3 * torch.rand(M, 1, generator=g)
    masks = (torch.rand(M, N, generator=g) < density).to(torch.uint8)      # overlapping: the best-scoring instance wins
    rows_desc = torch.randperm(M, generator=g)[:n].to(torch.int32)         # unordered
    if N > 3:                                                              # some points are covered by nothing: they keep sem_stuff
        masks[:, torch.randperm(N, generator=g)[: max(N // 10, 1)]] = 0
    thr = 0
    if N >= 200:
        # the two best candidates on point sets of their own: exactly npoint_thr painted points (dropped) and npoint_thr + 1 (kept)
        thr = 100 if N > 1000 else 10
        perm = torch.randperm(N, generator=g)
        masks[rows_desc[0].long()] = 0
        masks[rows_desc[0].long(), perm[:thr]] = 1
        if n > 1:
            masks[rows_desc[1].long()] = 0
            masks[rows_desc[1].long(), perm[thr:2 * thr + 1]] = 1
    if n >= 4:                                                             # the last candidate lies inside a better one
        masks[rows_desc[n - 1].long()] = masks[rows_desc[2].long()] * (torch.rand(N, generator=g) < 0.5).to(torch.uint8)
    labels = torch.randint(0, 198, (n,), generator=g, dtype=torch.int32)
    sem_stuff = torch.randint(0, max(n_stuff, 1), (N,), generator=g)
    return masks, rows_desc, labels, thr, sem_stuff


@pytest.mark.parametrize("n_stuff", [0, 2])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 10_003])
def test_panoptic(N, n_stuff):
    from segdino3d_amd import ops
    d = _dev()
    for n in (1, 2, 33, 250):
        masks, rows_desc, labels, thr, sem_stuff = _panoptic_case(N, n, n_stuff)
        ref_sem, ref_inst = R.panoptic_ref(masks.numpy(), rows_desc.numpy(), labels.numpy(), n_stuff, thr, sem_stuff.numpy())
        if N >= 200 and n > 1 and (n_stuff > 0 or n > 2):                  # (with n_stuff = 0 the lowest candidate has id 0 and vanishes)
            best, second = n_stuff + n - 1, n_stuff + n - 2                # ids of the two planted candidates
            assert (ref_inst == best).sum() == 0 and (ref_inst == second).sum() == thr + 1
        sem, inst = ops.panoptic(masks.to(d), rows_desc.to(d), labels.to(d), n_stuff, thr, sem_stuff.to(d))
        assert sem.dtype == torch.int64 and inst.dtype == torch.int64
        assert np.array_equal(inst.cpu().numpy(), ref_inst), (N, n, n_stuff, "instance map")
        assert np.array_equal(sem.cpu().numpy(), ref_sem), (N, n, n_stuff, "semantic map")


# ---- the chain on constructed decoder outputs -----------------------------------------------------------------------------------------------
CHAIN = R.CHAIN                                                          # tests/test_post_ref_oracle.py checks its conditions on the CPU


@pytest.fixture(scope="module")
def chain_model():
    import bench
    return bench.build_model(200, _dev())


@pytest.fixture(scope="module")
def chain_inputs():
    return R.chain_scene(**CHAIN)


def _keyed(labels, masks, scores, cut=1e-3):
    out = {}
    for lab, m, s in zip(labels, masks, scores):
        if float(s) > cut:
            key = (int(lab), np.packbits(np.asarray(m).astype(bool)).tobytes())
            assert key not in out
            out[key] = float(s)
    return out


@pytest.mark.parametrize("kernel,query_num", [("linear", -1), ("gaussian", -1), ("linear", 200)])
def test_chain_on_constructed_decoder_outputs(chain_model, chain_inputs, monkeypatch, kernel, query_num):
    """`Baseline3D.predict_by_feat` on hand-made decoder outputs that fill the panoptic path (>= 10 candidates above pan_score_thr,
    >= 3 demoted by matrix-NMS: asserted on the oracle's output) == `oracle.postprocess_ref.predict_by_feat`: both panoptic maps and the
    semantic map exactly, the instances above 1e-3 as a set of (label, mask bytes), their scores within the module's tolerance rule."""
    from oracle import postprocess_ref as P
    d = _dev()
    model, s, C = chain_model, chain_inputs, CHAIN["C"]
    assert model.num_classes == C and model.filter_outofbox_points_eval
    cfg = P.TestCfg(matrix_nms_kernel=kernel)
    for key in ("topk_insts", "inst_score_thr", "pan_score_thr", "npoint_thr", "obj_normalization", "sp_score_thr", "nms", "stuff_classes"):
        assert model.test_cfg[key] == getattr(cfg, key), key
    ref, measured = R.chain_conditions(P, s, C, cfg, True, query_num)
    print(f"[chain conditions, {kernel}] {measured}")
    monkeypatch.setitem(model.test_cfg, "matrix_nms_kernel", kernel)
    monkeypatch.setattr(model, "query_num", query_num)
    out = {k: [s[k].to(d)] for k in ("cls_preds", "masks", "centers", "sizes", "sem_preds")}
    with torch.no_grad():
        pd = model.predict_by_feat([s["points"].to(d)], out, s["superpoints"].to(d), 0)[0]
    assert torch.equal(pd.pts_semantic_mask[0].cpu(), ref["pts_semantic_mask"][0])
    assert torch.equal(pd.pts_semantic_mask[1].cpu(), ref["pts_semantic_mask"][1])
    assert torch.equal(pd.pts_instance_mask[1].cpu(), ref["pts_instance_mask"][1])
    assert len(torch.unique(ref["pts_instance_mask"][1])) > 8              # the panoptic kernels ran with content
    got = _keyed(pd.instance_labels.cpu().numpy(), pd.pts_instance_mask[0].cpu().numpy(), pd.instance_scores.cpu().numpy())
    ref32 = _keyed(ref["instance_labels"].numpy(), ref["pts_instance_mask"][0].numpy(), ref["instance_scores"].numpy())
    assert len(ref32) >= 30 and set(got) == set(ref32)
    r64 = R.predict_instance_ref(s["cls_preds"], s["masks"], s["superpoints"], s["points"][:, :3], s["centers"], s["sizes"], C, cfg,
                                 cfg.inst_score_thr, True)
    ref64 = _keyed(r64["labels"].numpy(), r64["masks"], r64["scores"].numpy())
    assert set(ref64) == set(ref32)
    keys = sorted(ref32)
    as_t = lambda dct: torch.tensor([dct[k] for k in keys], dtype=torch.float64)  # noqa: E731
    check_float("chain", f"{kernel} query_num={query_num} instance scores", as_t(got), as_t(ref64), as_t(ref32))
