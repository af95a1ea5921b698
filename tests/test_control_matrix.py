"""No GPU: the control matrix of the device search layer stays closed.

The dispatch switches of wait_kernel.hip, reserve_kernel.hip, replan_kernel.hip and table_kernel.hip are read line by line
(`case 0x..:` and `case 1..4:`), the instantiations they launch are derived (times 2 for dim) and tests/control_matrix.py
has to name at least one GPU test case for every one of them -- a case that exists in the GPU test it names.  Only those
dispatch lines are read.  (What the added GPU cases rest on -- the models at every order, the numbers the SNP worlds pin,
the wait inputs -- is checked in tests/test_search_orders.py.)"""
import importlib
import os
import re

import numpy as np
import pytest

import control_matrix as CM

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "motion_primitive_library_amd", "csrc")
# (file, function holding the switch, what its cases are)
SWITCHES = [("wait_kernel.hip", "launch_dim", "flag"), ("reserve_kernel.hip", "check_dim", "order"),
            ("replan_kernel.hip", "edge_dim", "flag"), ("replan_kernel.hip", "reserve_dim", "order"),
            ("table_kernel.hip", "hash_dim", "flag")]


def switch_cases(file, function):
    """The case labels of the switch inside `function`, as the source spells them."""
    lines = open(os.path.join(CSRC, file)).read().split("\n")
    start = [i for i, ln in enumerate(lines) if re.match(r"\s*hipError_t %s\(" % function, ln)]
    assert len(start) == 1, (file, function, start)
    cases = []
    for ln in lines[start[0]:]:
        m = re.match(r"\s*case (0x[0-9a-fA-F]+|\d+):", ln)
        if m:
            cases.append(m.group(1))
        if re.match(r"\s*default:", ln):
            return cases
    raise AssertionError("%s: the switch of %s has no default" % (file, function))


def instantiations(file, function, kind):
    """{(dim, control name)} or {(dim, order)}: every case of the switch, in 2D and 3D (the function is a template on D and
    its caller dispatches dim 2 and 3: both spellings have to be in the file)."""
    text = open(os.path.join(CSRC, file)).read()
    for d in (2, 3):
        assert re.search(r"%s<%d[,>]" % (function, d), text), (file, function, d)
    cases = switch_cases(file, function)
    if kind == "flag":
        assert all(c.startswith("0x") for c in cases), cases
        return {(d, CM.NAMES[int(c, 16)]) for d in (2, 3) for c in cases}
    assert all(not c.startswith("0x") for c in cases), cases
    return {(d, int(c)) for d in (2, 3) for c in cases}


@pytest.mark.parametrize("file,function,kind", SWITCHES, ids=["%s-%s" % (f.split("_")[0], fn) for f, fn, _ in SWITCHES])
def test_every_instantiation_has_a_gpu_case(file, function, kind):
    inst = instantiations(file, function, kind)
    assert len(inst) == (16 if kind == "flag" else 8), sorted(inst)  # what the registry was written for
    if function == "edge_dim":
        # the switch is instantiated twice, TIMED and not: every pair runs in the timed form; the untimed form runs in the
        # pairs the registry names, and the ones that run in no untimed GPU case are listed by name, exactly
        timed, untimed = CM.COVERAGE[(file, function, "timed")], CM.COVERAGE[(file, function, "untimed")]
        missing = sorted(i for i in inst if not timed.get(i))
        assert not missing, "replan_edge_kernel<.., TIMED = true> without a GPU case: %s" % missing
        assert set(untimed) | set(CM.UNTIMED_EDGE_NOT_RUN) == inst and not set(untimed) & set(CM.UNTIMED_EDGE_NOT_RUN)
        assert all(untimed.values())
        assert all((d, "SNP") in untimed for d in (2, 3)) and (2, "JRKxYAW") in untimed  # the jerk row and K = 3 with yaw
        return
    cover = CM.COVERAGE[(file, function)]
    missing = sorted(i for i in inst if not cover.get(i))
    assert not missing, "%s %s: instantiations without a GPU case: %s" % (file, function, missing)
    assert set(cover) == inst, sorted(set(cover) - inst)  # nothing named that the switch does not launch


def test_the_pairs_are_the_switch_labels():
    assert len(CM.PAIRS) == 16 and {CM.FLAGS[c] for _, c in CM.PAIRS} == {0x01, 0x03, 0x07, 0x0F, 0x11, 0x13, 0x17, 0x1F}
    assert [CM.order_of(c) for c in ("VEL", "ACC", "JRK", "SNP", "VELxYAW", "SNPxYAW")] == [1, 2, 3, 4, 1, 4]
    for file, function, kind in SWITCHES:
        if kind == "flag":
            assert sorted(int(c, 16) for c in switch_cases(file, function)) == sorted(CM.FLAGS.values()), (file, function)
        else:
            assert [int(c) for c in switch_cases(file, function)] == [1, 2, 3, 4], (file, function)


def case_ids(test_id):
    """The ids the named GPU test is parametrised with (None: it is not parametrised)."""
    path, name = test_id.split("::")
    name, _, case = name.partition("[")
    mod = importlib.import_module(os.path.basename(path)[:-3])
    fn = getattr(mod, name)
    assert any(mk.name == "gpu" for mk in np.atleast_1d(getattr(mod, "pytestmark", []))), test_id
    marks = [mk for mk in getattr(fn, "pytestmark", []) if mk.name == "parametrize"]
    if not marks:
        return None, case
    assert len(marks) == 1, test_id
    values, ids = marks[0].args[1], marks[0].kwargs.get("ids")
    names = marks[0].args[0]
    out = []
    for k, v in enumerate(values):
        if hasattr(v, "id") and v.id is not None:
            out.append(v.id)
        elif ids is not None:
            out.append(ids[k])
        else:
            out.append("%s%d" % (names, k))  # pytest's own id of a value it cannot spell
    return out, case


def test_every_named_case_exists():
    named = sorted({t for cover in CM.COVERAGE.values() for tests in cover.values() for t in tests})
    assert len(named) > 60
    for t in named:
        ids, case = case_ids(t)
        if ids is None:
            assert case == "", t
        else:
            assert case.rstrip("]") in ids, (t, ids)
