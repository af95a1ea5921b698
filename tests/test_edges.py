"""Batched edge re-validation: env_map::is_free(Primitive),
calculate_intrinsic_cost and the linked cells of MapPlanner::getLinkedNodes.
CPU: restatement against the reference's own env_map / Primitive::sample.
GPU: edge_kernel.hip through mplx_check_edges against the oracle."""
import os

import numpy as np
import pytest

from helpers import engine_env, oracle_env
from oracle import oracle as O

REF_SO = os.path.join(O.HERE, "_ref", "libmpl_ref.so")


def _edges(m, dim, control, seed, region=False, n=400, dims=None):
    from test_gpu_parity import _small_world
    wl = _small_world(m, dim, control, seed=seed, n_nodes=n, region=region, dims=dims)
    rng = np.random.default_rng(seed + 1)
    actions = rng.integers(0, wl.U.shape[0], size=n).astype(np.int32)
    wl.nodes[dim:4 * dim, :8] = 0.0  # a few parents at rest: with u = 0 the primitive does not move (n == 0)
    zero_u = int(np.nonzero(np.all(wl.U[:, :dim] == 0, axis=1))[0][0])
    actions[:4] = zero_u
    return wl, actions


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref not built")
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("control", [0x01, 0x03, 0x07, 0x0F])
@pytest.mark.parametrize("region", [False, True])
def test_restatement_matches_reference_is_free_and_linked_cells(dim, control, region):
    import motion_primitive_library_amd as m
    wl, actions = _edges(m, dim, control, 7000 + 16 * dim + control, region)
    a = O.check_edges(oracle_env(wl), wl.nodes, actions, cell_cap=64)
    b = O.check_edges(oracle_env(wl), wl.nodes, actions, cell_cap=64, ref=True)
    assert np.array_equal(a["free"], b["free"]) and 0 < a["free"].sum() < a["free"].size
    assert np.array_equal(a["cost"], b["cost"])
    assert np.array_equal(a["cell_count"], b["cell_count"]) and a["cell_count"].max() <= 64
    for k in range(actions.size):
        c = a["cell_count"][k]
        assert np.array_equal(a["cells"][k, :c], b["cells"][k, :c]), k


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("control", [0x01, 0x03, 0x07, 0x0F])
@pytest.mark.parametrize("region", [False, True])
def test_device_edges_match_the_oracle(engine, dim, control, region):
    wl, actions = _edges(engine, dim, control, 7000 + 16 * dim + control, region)
    env = engine_env(engine, wl)
    got = env.check_edges(wl.nodes, actions, cell_cap=64)
    small = env.check_edges(wl.nodes, actions, cell_cap=3)   # truncated rows still report the full count
    plain = env.check_edges(wl.nodes, actions)
    env.close()
    ref = O.check_edges(oracle_env(wl), wl.nodes, actions, cell_cap=64)
    assert np.array_equal(got["free"], ref["free"]) and np.array_equal(plain["free"], ref["free"])
    assert np.array_equal(got["cost"], ref["cost"]) and np.array_equal(plain["cost"], ref["cost"])
    assert np.array_equal(got["cell_count"], ref["cell_count"]) and np.array_equal(small["cell_count"], ref["cell_count"])
    for k in range(actions.size):
        c = ref["cell_count"][k]
        assert np.array_equal(got["cells"][k, :c], ref["cells"][k, :c]), k
        assert np.array_equal(small["cells"][k, :min(c, 3)], ref["cells"][k, :min(c, 3)]), k
    assert (ref["free"][:4] == 0).all() and np.isinf(ref["cost"][:4]).all()  # the edges that do not move


@pytest.mark.gpu
def test_check_edges_rejects_bad_actions(engine):
    wl, actions = _edges(engine, 2, 0x03, 1)
    env = engine_env(engine, wl)
    actions[5] = wl.U.shape[0]
    with pytest.raises(engine._abi.MplxError) as e:
        env.check_edges(wl.nodes, actions)
    assert e.value.code == engine._abi.ERR_ARG
    env.close()
