"""tests/ordered_sum_witness.py itself (no GPU): exact where every order is, within the fp32 bound elsewhere, and sensitive to the
order — it is what pins the summation order of csrc/ordered_sum.hpp in the GPU tests."""
import math

import numpy as np
import pytest

import ordered_sum_witness as ow

# (rows, workgroups, strided): one lane; a ragged chunk; 258 chunks (a second partial for lane 0 of the last sum, three rows in the
# last chunk); a capped grid with a second row for five lanes and four partials per lane of the last sum
SHAPES = [(1, 1, False), (129, 1, False), (1500, 6, False), (65795, 258, False), (4096, 16, True), (262149, 1024, True), (700, 2, True)]


@pytest.mark.parametrize("n,groups,strided", SHAPES)
def test_small_integer_terms_sum_exactly(n, groups, strided):
    terms = np.random.default_rng(n).integers(-8, 9, n).astype(np.float32)
    got = ow.ordered_sum(terms, groups, strided=strided)
    assert got.dtype == np.float32 and float(got) == float(terms.astype(np.int64).sum())


@pytest.mark.parametrize("n,groups,strided", SHAPES)
def test_random_terms_stay_within_the_fp32_bound_of_the_exact_sum(n, groups, strided):
    terms = np.random.default_rng(n + 1).uniform(-1, 1, n).astype(np.float32)
    exact = math.fsum(float(t) for t in terms)
    bound = n * 2.0 ** -24 * math.fsum(abs(float(t)) for t in terms)
    assert abs(float(ow.ordered_sum(terms, groups, strided=strided)) - exact) <= bound


def test_the_witness_depends_on_the_order():
    terms = np.random.default_rng(7).uniform(0, 1, 1500).astype(np.float32)
    left_to_right = np.float32(0)
    for t in terms:
        left_to_right = np.float32(left_to_right + t)
    got = ow.ordered_sum(terms, 6, strided=False)
    assert got.view(np.uint32) != left_to_right.view(np.uint32)
    # ... and on the grid: the same rows over another number of workgroups are another order
    assert got.view(np.uint32) != ow.ordered_sum(terms, 2).view(np.uint32) or got.view(np.uint32) != ow.ordered_sum(terms, 3).view(np.uint32)


def test_one_row_per_lane_is_the_strided_plan_of_a_grid_that_covers_the_rows():
    terms = np.random.default_rng(3).uniform(-1, 1, 1500).astype(np.float32)
    assert ow.ordered_sum(terms, 6, strided=False).view(np.uint32) == ow.ordered_sum(terms, 6, strided=True).view(np.uint32)
    with pytest.raises(AssertionError):
        ow.ordered_sum(terms, 5, strided=False)
