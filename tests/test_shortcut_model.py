"""tests/shortcut_model.py: the dynamic programme against a brute force over every chain of hops (no GPU).  The costs are
multiples of 1/8 below 2^10, so every sum is exact and ties are real ties; +inf marks hops that are not admitted."""
import numpy as np
import pytest

import shortcut_model as XM


def matrix(rng, W, max_hop, p_inf, levels):
    c = rng.integers(1, levels, (W - 1, max_hop)).astype(np.float64) / 8.0
    c[rng.random(c.shape) < p_inf] = np.inf
    c[:, 0] = rng.integers(1, levels, W - 1) / 8.0  # the adjacent hop is always admitted
    return c


@pytest.mark.parametrize("W", [2, 3, 5, 8])
def test_dp_equals_brute_force(W):
    rng = np.random.default_rng(40 + W)
    for trial in range(60):
        max_hop = int(rng.integers(1, W + 1))
        c = matrix(rng, W, max_hop, 0.3 * (trial % 3), 4 if trial % 2 else 64)  # few levels: many exact ties
        status, keep, cost, chain = XM.dp(c, W, max_hop)
        want_keep, want_cost = XM.brute(c, W, max_hop)
        assert status == 0 and keep == want_keep, (W, trial, keep, want_keep)
        assert np.float64(cost).view(np.uint64) == np.float64(want_cost).view(np.uint64)
        assert keep[0] == 0 and keep[-1] == W - 1 and cost <= chain
        assert chain == sum(c[:, 0])
        if max_hop == 1:
            assert keep == list(range(W)) and cost == chain


def test_ties_go_to_the_smallest_predecessor():
    c = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, np.inf], [1.0, np.inf, np.inf]])  # 0-3 direct, 0-1-3, 0-2-3, 0-1-2-3: all 3
    assert XM.dp(c, 4, 3)[1] == [0, 3]
    c[0, 2] = np.inf
    assert XM.dp(c, 4, 3)[1] == [0, 1, 3]  # predecessors 1 and 2 tie: the smaller
    assert XM.brute(c, 4, 3)[0] == [0, 1, 3]


def test_statuses():
    c = np.ones((3, 2))
    assert XM.dp(c, 1, 2)[0] == XM.EMPTY and XM.dp(c, 0, 2)[0] == XM.EMPTY
    c[1, 0] = np.nan
    status, keep, cost, chain = XM.dp(c, 4, 2)
    assert status == XM.BAD_CHAIN and keep == [0, 1, 2, 3] and np.isnan(cost) and np.isnan(chain)
    assert XM.dp(c, 2, 2)[0] == 0  # the bad hop is past this chain's end
