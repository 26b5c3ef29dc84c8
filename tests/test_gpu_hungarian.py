"""Device linear-sum-assignment solver (segdino3d_amd/csrc/assign.hip through ops.hungarian_match) against
scipy.optimize.linear_sum_assignment on the same fp32 matrix.  The outcome is integer decisions: where the optimum is
unique the match matrix must be identical to scipy's pairs (a float64 restatement of the algorithm with lowest-index
tie-breaking reproduced scipy on every such input here, so the optimum of these inputs is unique); where it is not, the
match must be one-to-one, complete, and of exactly scipy's total cost."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RANDOM_SHAPES = [(1, 1), (1, 7), (7, 1), (5, 5), (24, 4), (4, 24), (65, 64), (64, 65), (300, 120), (2250, 120)]
TRAINING_SHAPES = [(2250, 3000, 120), (200, 3000, 120), (96, 300, 130)]            # (Q, S, G)


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def scipy_match(cost: np.ndarray) -> np.ndarray:
    from scipy.optimize import linear_sum_assignment
    q, g = linear_sum_assignment(cost)
    m = np.zeros(cost.shape, dtype=np.uint8)
    m[q, g] = 1
    return m


@functools.lru_cache(maxsize=None)
def random_costs():
    """The ten normal matrices, drawn from ONE generator in the order of RANDOM_SHAPES, with scipy's matches."""
    rng = np.random.default_rng(0)
    costs = [rng.standard_normal(s).astype(np.float32) for s in RANDOM_SHAPES]
    return costs, [scipy_match(c) for c in costs]


@functools.lru_cache(maxsize=None)
def training_costs():
    """Training-shaped costs: the recipe of test_gpu_criterion._training_size_case through the oracle's match_costs (fp32)."""
    from oracle import loss_ref
    from tests.test_gpu_criterion import _training_size_case
    costs = []
    for Q, S, G in TRAINING_SHAPES:
        t, layers = _training_size_case(5, Q, S, G, 198, 200)
        layer = layers[-1]
        c = loss_ref.match_costs(layer["cls_preds"][0], layer["masks"][0], layer["centers"][0], layer["sizes"][0], t["labels"],
                                 t["sp_inst_sem_masks"][:G], t["instance_centers"], t["instance_sizes"], [0.5, 1.0, 1.0, 0.5, 0.5])
        costs.append(np.ascontiguousarray(c.numpy(), dtype=np.float32))
    return costs, [scipy_match(c) for c in costs]


def solve(costs, **kw):
    from segdino3d_amd import ops
    d = dev()
    return ops.hungarian_match([torch.from_numpy(c).to(d) for c in costs], **kw)


def assert_one_to_one(m: np.ndarray, n_ones: int):
    assert set(np.unique(m).tolist()) <= {0, 1}
    assert int(m.sum()) == n_ones
    if m.size:
        assert int(m.sum(0).max()) <= 1 and int(m.sum(1).max()) <= 1


@pytest.mark.parametrize("k", range(len(RANDOM_SHAPES)), ids=[f"{q}x{g}" for q, g in RANDOM_SHAPES])
def test_random_matrices_equal_scipy(k):
    costs, refs = random_costs()
    m = solve([costs[k]])[0].cpu().numpy()
    assert m.dtype == np.uint8 and m.shape == costs[k].shape
    assert np.array_equal(m, refs[k])


@pytest.mark.parametrize("k", range(len(TRAINING_SHAPES)), ids=[f"Q{q}-S{s}-G{g}" for q, s, g in TRAINING_SHAPES])
def test_training_shaped_costs_equal_scipy(k):
    costs, refs = training_costs()
    m = solve([costs[k]])[0].cpu().numpy()
    assert np.array_equal(m, refs[k])


def test_one_batched_call_equals_the_single_problem_calls():
    """All of the above plus twenty (40, 12) matrices in one call: more problems than one launch holds (SD3D_MAX_BATCH = 16),
    mixed shapes and orientations.  Bit for bit the single-problem results, and the same bytes on a second call."""
    rc, rr = random_costs()
    tc, tr = training_costs()
    rng = np.random.default_rng(1)
    small = [rng.standard_normal((40, 12)).astype(np.float32) for _ in range(20)]
    costs = list(rc) + list(tc) + small
    assert len(costs) > 16
    single = [solve([c])[0].cpu() for c in costs]
    for m, ref in zip(single, list(rr) + list(tr) + [scipy_match(c) for c in small]):
        assert np.array_equal(m.numpy(), ref)
    batched = [m.cpu() for m in solve(costs)]
    again = [m.cpu() for m in solve(costs)]
    for a, b, c in zip(single, batched, again):
        assert torch.equal(a, b) and torch.equal(b, c)


def test_ties_give_an_optimal_one_to_one_match():
    rng = np.random.default_rng(2)
    cost = rng.integers(0, 4, (40, 12)).astype(np.float32)
    m = solve([cost])[0].cpu().numpy()
    assert_one_to_one(m, 12)
    # small integers: both totals are exact
    assert float(cost[m.astype(bool)].astype(np.float64).sum()) == float(cost[scipy_match(cost).astype(bool)].astype(np.float64).sum())


def test_large_constants_are_ordinary_values():
    """Half the entries at 1e8, the value of a masked cost (loss_3d.py:326)."""
    rng = np.random.default_rng(3)
    cost = rng.standard_normal((40, 12)).astype(np.float32)
    cost[rng.random((40, 12)) < 0.5] = 1e8
    m = solve([cost])[0].cpu().numpy()
    assert np.array_equal(m, scipy_match(cost))


@pytest.mark.parametrize("shape", [(12000, 8), (8, 12000)], ids=["12000x8", "8x12000"])
def test_more_columns_than_the_lds_path_holds(shape):
    """m = 12000 > 4096: the solver state lives in the workspace.  Eight agents keep it cheap."""
    rng = np.random.default_rng(4)
    cost = rng.standard_normal(shape).astype(np.float32)
    m = solve([cost])[0].cpu().numpy()
    assert np.array_equal(m, scipy_match(cost))


@pytest.mark.parametrize("shape", [(0, 5), (5, 0), (0, 0)], ids=["Q0", "G0", "both0"])
def test_empty_problems_give_empty_matches(shape):
    rng = np.random.default_rng(5)
    other = rng.standard_normal((6, 3)).astype(np.float32)
    ms, status = solve([np.zeros(shape, np.float32), other], check=True, return_status=True)
    assert tuple(ms[0].shape) == shape and int(ms[0].sum()) == 0
    assert np.array_equal(ms[1].cpu().numpy(), scipy_match(other))
    assert status.cpu().tolist() == [0, 0]


def test_nan_entry_sets_the_status_word_and_the_match_stays_one_to_one():
    """scipy raises ValueError on NaN; the device call returns (every loop of the solver is bounded by a counter: n agents,
    at most m search steps each, at most n hops per flipped path), flags the problem and still matches one-to-one."""
    rng = np.random.default_rng(6)
    cost = rng.standard_normal((24, 4)).astype(np.float32)
    good = cost.copy()
    cost[7, 2] = np.nan
    ms, status = solve([cost, good], return_status=True)
    assert status.cpu().tolist() == [1, 0]
    assert_one_to_one(ms[0].cpu().numpy(), 4)
    assert np.array_equal(ms[1].cpu().numpy(), scipy_match(good))
    with pytest.raises(ValueError):
        solve([cost], check=True)


def test_no_finite_assignment_sets_the_status_word():
    """Every entry +inf (scipy: "cost matrix is infeasible"): the lowest-index unvisited column is still taken at every step, so
    the match is complete and one-to-one, and the problem is flagged.  A single +inf entry is an ordinary value."""
    rng = np.random.default_rng(7)
    cost = rng.standard_normal((9, 5)).astype(np.float32)
    cost[2, 3] = np.inf
    ms, status = solve([np.full((6, 3), np.inf, np.float32), cost], return_status=True)
    assert status.cpu().tolist() == [1, 0]
    assert_one_to_one(ms[0].cpu().numpy(), 3)
    assert np.array_equal(ms[1].cpu().numpy(), scipy_match(cost))


def test_cpu_tensors_are_refused():
    from segdino3d_amd import ops
    dev()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.hungarian_match([torch.zeros(4, 3)])
