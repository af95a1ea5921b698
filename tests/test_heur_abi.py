"""CPU: the symbols include/mplx_heur.h declares are exported, reachable through _abi.py, and leave the ABI version of
include/mplx.h alone; the entry points answer NULL handles without touching a device; the Python surface."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared():
    text = open(os.path.join(ROOT, "include", "mplx_heur.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mplx_[a-z0-9_]+)\s*\(", text)))


def test_heur_symbols_resolve(engine):
    A = engine._abi
    assert sorted(A.HEUR_SYMBOLS) == declared()
    raw = C.CDLL(A.LIB_PATH)
    L = A.lib()
    for s in A.HEUR_SYMBOLS:
        assert hasattr(raw, s), "libmplx.so does not export %s" % s
        assert getattr(L, s).argtypes is not None
    assert L.mplx_abi_version() == 9
    text = open(os.path.join(ROOT, "include", "mplx_heur.h")).read()
    assert (A.HEUR_DEFAULT, A.HEUR_REFERENCE, A.HEUR_ROBUST) == (0, 1, 2)
    assert "MPLX_HEUR_DEFAULT = 0, MPLX_HEUR_REFERENCE = 1, MPLX_HEUR_ROBUST = 2" in text
    assert "#define MPLX_HEUR_BISECT %d" % A.HEUR_BISECT in text
    import heur_model as HM
    assert HM.BISECT == A.HEUR_BISECT and (HM.DEFAULT, HM.REFERENCE, HM.ROBUST) == (0, 1, 2)
    math_h = open(os.path.join(ROOT, "motion_primitive_library_amd", "csrc", "mplx_heur_math.h")).read()
    assert "kBisect = %d" % A.HEUR_BISECT in math_h


def test_heur_entry_points_answer_null_handles(engine):
    A = engine._abi
    L = A.lib()
    assert L.mplx_heur_eval(None, None, 2, None, 0, 0, None) == A.ERR_ARG
    assert L.mplx_heur_eval_device(None, None, 2, None, 0, 0, None) == A.ERR_ARG
    assert L.mplx_open_set_heur(None, 2) == A.ERR_ARG
    assert L.mplx_planner_set_heur_dynamics(None, 2) == A.ERR_ARG


def test_python_surface(engine):
    import inspect
    m = engine
    A = m._abi
    assert hasattr(m.EnvMap, "heur_eval") and hasattr(m.EnvMap, "heur_eval_resident") and hasattr(m.OpenSet, "set_heur")
    for fn in (m.EnvMap.search, m.EnvMap.search_many):
        assert inspect.signature(fn).parameters["heur"].default is None
    p = inspect.signature(m.MapPlanner.setHeurIgnoreDynamics).parameters
    assert p["ignore"].default is True and p["robust"].default is False
    assert inspect.signature(m.EnvMap.heur_eval).parameters["mode"].default == "robust"
    assert [A.heur_mode(x) for x in (None, "default", "reference", "robust", 2)] == [0, 0, 1, 2, 2]
    with pytest.raises(ValueError):
        A.heur_mode("exact")
