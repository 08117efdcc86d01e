"""The render launch planner on the host (raytrace2_amd/csrc/launch_plan.h, built into the stand-alone
tests/cpp/launch_plan_host.cpp): magic divisors, the chunk schedule's invariants and pinned tables, tile
shapes, frames per launch and item counts. No GPU."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "raytrace2_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True])
def test_launch_plan(tmp_path, sanitize):
    """Plain and with the host sanitizers (a stand-alone program)."""
    exe = str(tmp_path / ("launch_plan_host_san" if sanitize else "launch_plan_host"))
    extra = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g") if sanitize else ()
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "launch_plan_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "launch plan ok" in r.stdout
