"""GPU: MapPlanner.setHeurIgnoreDynamics (include/mplx_heur.h) with the engine's own expansion: the REFERENCE mode
reproduces the reference's plan on the corridor (tests/golden/heur_golden.npz), the ROBUST mode finds the default plan's
cost on the exact-goal scenario with fewer expansions, LPA* replans with it, and REFERENCE on a JRK planner is refused."""
import os

import numpy as np
import pytest

import heur_model as HM
from test_plan_known_answer import corridor

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "heur_golden.npz")


def corridor_planner(m):
    c = corridor()
    planner = m.MapPlanner(2)
    mu = m.MapUtil(2)
    mu.setMap(c["origin"], c["dim"], c["cells"], c["res"])
    planner.setMapUtil(mu)
    planner.setVmax(1.0)
    planner.setAmax(1.0)
    planner.setDt(1.0)
    planner.setU(m.workloads.grid_controls([-0.5, 0.0, 0.5], 2))
    return planner, m.Waypoint(2, m.ACC, pos=c["start"]), m.Waypoint(2, m.ACC, pos=c["goal"])


def scene_planner(m, cells=None, lpa=False):
    planner = m.MapPlanner(2)
    mu = m.MapUtil(2)
    mu.setMap([0.0, 0.0], HM.SCENE_DIMS, HM.scene_cells() if cells is None else cells, HM.SCENE_RES)
    planner.setMapUtil(mu)
    planner.setVmax(HM.SCENE_VMAX)
    planner.setAmax(1.0)
    planner.setDt(1.0)
    planner.setW(HM.SCENE_W)
    planner.setTol(0.0, 0.0)
    planner.setU(m.workloads.grid_controls([-1.0, 0.0, 1.0], 2))
    if lpa:
        planner.setLPAstar(True)
    return planner, m.Waypoint(2, m.ACC, pos=HM.SCENE_START), m.Waypoint(2, m.ACC, pos=HM.SCENE_GOAL)


def test_reference_mode_reproduces_the_reference_plan(engine):
    m = engine
    z = np.load(GOLD)
    planner, start, goal = corridor_planner(m)
    planner.setHeurIgnoreDynamics(False)
    planner.useDeviceHeuristic(True)  # (the planner evaluates new nodes itself while the mode is on)
    assert planner.plan(start, goal)
    s = planner.summary()
    print("REFERENCE on the corridor:", s["cost"], s["expansions"], planner.getTraj().getTotalTime(), planner.timing()["heur_from_device"])
    assert s["cost"] == z["plan/cost"].view(np.float64)[0] == 352.0
    assert s["expansions"] == int(z["plan/expanded"][0])
    assert planner.getTraj().getTotalTime() == z["plan/duration"].view(np.float64)[0]
    assert planner.timing()["heur_from_device"] == 0
    planner.setHeurIgnoreDynamics(True)
    assert planner.plan(start, goal) and planner.summary()["cost"] == 351.5  # off again: the published plan
    planner.close()


def test_robust_mode_on_the_exact_goal_scenario(engine):
    m = engine
    planner, start, goal = scene_planner(m)
    assert planner.plan(start, goal)
    d = planner.summary()
    planner.setHeurIgnoreDynamics(False, robust=True)
    assert planner.plan(start, goal)
    r = planner.summary()
    print("exact goal: default", d["cost"], d["expansions"], "ROBUST", r["cost"], r["expansions"])
    assert r["cost"] == d["cost"] == 21.0 and r["expansions"] < d["expansions"]
    planner.close()


def test_lpastar_with_robust_replans_to_the_cost_of_a_fresh_plan(engine):
    m = engine
    planner, start, goal = scene_planner(m, lpa=True)
    planner.setHeurIgnoreDynamics(False, robust=True)
    assert planner.plan(start, goal) and planner.summary()["cost"] == 21.0
    new = HM.scene_cells(gap=True)
    changed = np.nonzero(new != HM.scene_cells())[0]
    planner.getLinkedNodes(want_points=False)
    planner.updateClearedNodes(np.array([[i % HM.SCENE_DIMS[0], i // HM.SCENE_DIMS[0]] for i in changed], np.int32))  # (edits the map too)
    assert planner.plan(start, goal)
    again = planner.summary()
    fresh, s2, g2 = scene_planner(m, cells=new)
    fresh.setHeurIgnoreDynamics(False, robust=True)
    assert fresh.plan(s2, g2)
    print("LPA* after the edit:", again["cost"], "fresh:", fresh.summary()["cost"])
    assert again["cost"] == fresh.summary()["cost"] < 21.0
    fresh.close()
    planner.close()


def test_reference_mode_on_a_jrk_planner_is_refused(engine):
    m = engine
    A = m._abi
    planner, start, goal = scene_planner(m)
    planner.setU(m.workloads.grid_controls([-1.0, 0.0, 1.0], 2))
    planner.setHeurIgnoreDynamics(False)
    with pytest.raises(A.MplxError) as e:
        planner.plan(m.Waypoint(2, m.JRK, pos=HM.SCENE_START), m.Waypoint(2, m.JRK, pos=HM.SCENE_GOAL))
    assert e.value.code == A.ERR_STATE
    planner.setHeurIgnoreDynamics(False, robust=True)  # ROBUST covers JRK
    planner.setMaxNum(200)
    planner.plan(m.Waypoint(2, m.JRK, pos=HM.SCENE_START), m.Waypoint(2, m.JRK, pos=HM.SCENE_GOAL))
    planner.close()
