"""csrc/mplx_stage.h needs no HIP: tests/stage_layout_check.cpp compiles it with the host compiler alone and checks the
offsets of StageRows against the raw StageLayout, the rows that were not asked for and the fixed capacity."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_the_row_layout_compiles_and_holds_without_hip(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "stage_layout_check")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", os.path.join(HERE, "stage_layout_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
