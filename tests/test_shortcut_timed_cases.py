"""The batch of the timed shortcut (tests/shortcut_timed_cases.py) on the CPU: the conditions without which
tests/test_gpu_shortcut_timed_batch.py would compare little.  The reference alone -- shortcut_model.DensePairs, edge_costs,
reserve_poly_model.check, admit, chain_hit, shortcut_model.dp -- must meet them, for every configuration and both B.  No
GPU."""
import numpy as np
import pytest

import shortcut_model as XM
import shortcut_timed_cases as TC

CONFIGS = sorted(XM.CONFIGS)


@pytest.mark.parametrize("B", TC.BS)
@pytest.mark.parametrize("D,control", CONFIGS, ids=["%dd-%#04x" % c for c in CONFIGS])
def test_the_batch_is_not_vacuous(D, control, B):
    c = TC.counts(D, control, B)
    print("D=%d control=%#04x B=%d: %s" % (D, control, B, c))
    assert c["live"] == 48 and c["admitted"] >= 100
    # non-adjacent pairs the untimed costs admit that the table blocks: enough to change the programme, not all of them
    assert 0.15 * c["admitted"] <= c["blocked"] <= 0.70 * c["admitted"]
    assert c["blocked_horizon"] >= 2
    assert 5 * c["keep_changes"] >= c["live"]
    assert c["chain_hit"] >= 5 and c["chain_horizon"] >= 1 and c["chain_clear"] >= 5
    # the rule h >= 0 ? ... : (h == -2 && ch == -1) of the programme kernel: a chain with both kinds of hit on its own edges
    assert c["both_on_chain"] >= 1
    # per-query rows: what the pair hits would be if every query got query 0's t0 / radius / ignored group, if the t row
    # were read as [i * Q + k] from a buffer laid out with the raw ABI test's stride, if nobody ignored anybody
    assert 10 * c["query0_changes"] >= c["solved"]
    assert 10 * c["stride_changes"] >= c["solved"]
    assert c["ignore_changes"] >= 5
    if B > 256:
        assert c["partner_256"] >= 10


@pytest.mark.parametrize("D", [2, 3])
def test_the_inputs(D):
    """What the inputs are said to be: the grid, the excluded ninth, both kinds of ignored group, t0 off the step."""
    for B in TC.BS:
        r = TC.reservations(D, B)
        c, dts, n_segs = r["res"]
        assert c.shape == (1, D + 1, 6, B) and np.array_equal(c[0, :D, 5] * 8, np.round(c[0, :D, 5] * 8))
        assert (n_segs[8::9] == 0).all() and n_segs.sum() == B - len(n_segs[8::9]) and (c[0, :, :5] == 0).all()
        tab = TC.table(D, B)
        assert tab["pos"].shape == (TC.N_STEPS[D], D, B) and tab["active"][:, n_segs > 0].all() == r["park"]
        assert not tab["included"][8::9].any() and tab["included"].sum() == n_segs.sum()
        t0, radius, ignore = TC.query_rows(D, B)
        assert len(set(t0)) == 11 and len(set(radius)) == 3 and (ignore == -1).any() and len(set(ignore)) > 10
        assert (np.round(t0[:11] / TC.STEP) * TC.STEP != t0[:11]).sum() == 8  # (all but 0, 0.5 and 1)


def test_the_hop_1_and_hop_5_cases():
    """max_hop = 1 has nothing non-adjacent to mask (the programme keeps every chain) and still reports chain hits of all
    three kinds; max_hop = 5 admits and blocks hops of every length."""
    D, control, B = 2, 0x03, 65
    b = XM.batch(D, control)
    t0, radius, ignore = TC.query_rows(D, B)
    for hop in (1, 5):
        _, cost, _ = TC.dense(D, control, hop)
        hit = TC.hits(D, control, B, TC.pair_rows(b["states"][4 * D + 1], t0, radius, ignore, hop), hop)
        timed, untimed = TC.programme(cost, hit, b["n_wp"], hop), TC.programme(cost, None, b["n_wp"], hop)
        ch = np.array([t[4] for t in timed if t[0] == 0])
        print("max_hop %d: chain_hit >= 0: %d, -2: %d, -1: %d" % (hop, (ch >= 0).sum(), (ch == -2).sum(), (ch == -1).sum()))
        assert (ch >= 0).sum() >= 5 and (ch == -2).any() and (ch == -1).sum() >= 5
        if hop == 1:
            assert all(t[1] == u[1] for t, u in zip(timed, untimed))
        else:
            blocked = np.isfinite(cost) & (hit != -1)
            assert all(blocked[:, :, h].any() for h in range(1, 5))
            assert sum(t[1] != u[1] for t, u in zip(timed, untimed)) >= 5
