"""CPU: the symbols include/mplx_field.h declares are exported, reachable through _abi.py, and leave the ABI version of
include/mplx.h alone; the entry points answer NULL handles without touching a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared():
    text = open(os.path.join(ROOT, "include", "mplx_field.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mplx_[a-z0-9_]+)\s*\(", text)))


def test_field_symbols_resolve(engine):
    A = engine._abi
    assert sorted(A.FIELD_SYMBOLS) == declared()
    raw = C.CDLL(A.LIB_PATH)
    L = A.lib()
    for s in A.FIELD_SYMBOLS:
        assert hasattr(raw, s), "libmplx.so does not export %s" % s
        assert getattr(L, s).argtypes is not None
    assert L.mplx_abi_version() == 9
    assert A.FIELD_MAX_BYTES == 1 << 30
    assert C.sizeof(A.FieldView) == 24


def test_field_entry_points_answer_null_handles(engine):
    A = engine._abi
    L = A.lib()
    out = C.c_void_p()
    n = C.c_int64()
    assert L.mplx_field_create(None, C.byref(out)) == A.ERR_ARG
    assert L.mplx_field_build(None, 0, None, None) == A.ERR_ARG
    assert L.mplx_field_shape(None, None, None) == A.ERR_ARG
    assert L.mplx_field_view_of(None, None) == A.ERR_ARG
    assert L.mplx_field_download(None, None) == A.ERR_ARG
    assert L.mplx_field_is_stale(None) == A.ERR_ARG
    assert L.mplx_field_passes(None, C.byref(n)) == A.ERR_ARG
    assert L.mplx_open_set_field(None, None, None) == A.ERR_ARG
    assert L.mplx_open_clear_field(None) == A.ERR_ARG
    L.mplx_field_destroy(None)


def test_python_surface(engine):
    import inspect
    m = engine
    assert hasattr(m.search, "GoalField") and hasattr(m.EnvMap, "alloc_field")
    for fn in (m.EnvMap.search, m.EnvMap.search_many):
        p = inspect.signature(fn).parameters
        assert p["field"].default is None and p["field_of_query"].default is None
    assert inspect.signature(m.search.plan_prioritised).parameters["field"].default is False
    assert m.search.float_to_int(0.26, 0.0, 0.25) == 1 and m.search.float_to_int(-0.01, 0.0, 0.25) == -1
