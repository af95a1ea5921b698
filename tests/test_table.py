"""CPU: the semantics of include/mplx_table.h as tests/table_model.py restates them -- the label-correcting sweep reaches
the fixed point a heap Dijkstra reaches, and on the corridor of the reference's test_planner_2d it finds the cost the
reference publishes -- plus the plumbing of the new header (declared in _abi.py, parses as C).  Successors come from the
CPU oracle; no GPU."""
import math
import os
import re
import subprocess

import numpy as np

from helpers import oracle_env
from oracle import oracle as O
from table_model import TableModel, dijkstra, oracle_provider, sweep
from test_gpu_parity import _small_world
from test_plan_known_answer import corridor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_start(wl):
    """A state at rest in a free cell near the middle of the workload's map."""
    md = wl.map_dim
    grid = np.asarray(wl.grid).reshape(md[::-1])
    free = np.argwhere(grid == 0)[:, ::-1]  # (x, y[, z])
    mid = np.array(md) / 2.0
    cell = free[np.argmin(np.abs(free - mid).sum(axis=1))]
    s = np.zeros(4 * wl.dim + 2)
    s[:wl.dim] = np.asarray(wl.origin) + (cell + 0.5) * wl.res
    return s


def test_sweep_reaches_the_fixed_point_of_dijkstra(engine):
    wl = _small_world(engine, 2, engine.ACC, seed=5, edge=32)
    oenv = oracle_env(wl)
    prov = oracle_provider(O, oenv)
    start = small_start(wl)
    h0 = O.lattice_hash(2, engine.ACC, start)
    model = TableModel(10)
    rounds, largest = sweep(model, prov, start, [h0])
    want = dijkstra(prov, start, h0)
    got = model.arrays()
    assert got["n_nodes"] > 200 and rounds > 3, (got["n_nodes"], rounds)  # a sweep worth the name
    reached = {int(h): float(g) for h, g in zip(got["hash"], got["g"]) if math.isfinite(g)}
    assert reached == want  # exact: both only add and compare doubles
    # nodes the sweep created but never reached: only blocked edges lead to them -- it has none (they do not count)
    assert len(reached) == got["n_nodes"]
    # every back-pointer is an edge of the final tree: g[v] = g[pred] + cost needs the lists, so check the order instead
    for i in range(1, got["n_nodes"]):
        assert got["pred"][i] >= 0 and got["g"][got["pred"][i]] < got["g"][i]
    assert got["pred"][0] == -1 and got["g"][0] == 0.0


def corridor_sweep_model(engine):
    c = corridor()
    U = engine.workloads.grid_controls([-0.5, 0.0, 0.5], 2)  # test_planner_2d.cpp:49-53
    oenv = O.Env(2, O.ACC, U, c["cells"], c["dim"], c["origin"], c["res"], v_max=1.0, a_max=1.0, dt=1.0)
    start = engine.Waypoint(2, engine.ACC, pos=c["start"]).to_row()
    model = TableModel(10)
    rounds, largest = sweep(model, oracle_provider(O, oenv), start, [O.lattice_hash(2, O.ACC, start)], g_max=351.5)
    return c, model, rounds, largest


def test_corridor_sweep_finds_the_published_cost(engine):
    """reference README.md:199-202: T = 35, J(ACC) = 1.5 -> g = 10 * 35 + 1.5 = 351.5 (tests/test_plan_known_answer.py).
    A sweep bounded by that cost reaches the goal region in exactly one node, at exactly that cost."""
    c, model, rounds, largest = corridor_sweep_model(engine)
    got = model.arrays()
    near = np.nonzero(np.abs(got["state"][:2] - np.asarray(c["goal"])[:, None]).max(axis=0) <= 0.5)[0]
    assert near.size == 1 and got["g"][near[0]] == 351.5
    assert rounds == 36 and got["n_nodes"] == 21677
    assert model.counting - 1 == 114107 and largest == 1047  # (the seed is a counting entry too)


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mplx_[a-z0-9_]+)\s*\(", text)))


def test_every_function_of_the_header_is_declared_in_abi(engine):
    syms = _declared("mplx_table.h")
    assert "mplx_table_relax_device" in syms and "mplx_table_seed" in syms and "mplx_table_path" in syms
    assert sorted(engine._abi.TABLE_SYMBOLS) == syms
    lib = engine._abi.lib()
    for s in syms:
        assert getattr(lib, s).argtypes is not None, s
    import ctypes as C
    assert C.sizeof(engine._abi.TableView) == 6 * 8 and C.sizeof(engine._abi.TableFrontier) == 6 * 8


def test_header_parses_as_c():
    r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "include", "mplx_table.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
