"""The render launch planner on the host (raytrace2_amd/csrc/launch_plan.h, built into the stand-alone
tests/cpp/launch_plan_host.cpp): magic divisors, the chunk schedule's invariants and pinned tables, tile
shapes, frames per launch and item counts. No GPU."""
import subprocess

import pytest

import host_build as H


@pytest.mark.parametrize("sanitize", [False, True])
def test_launch_plan(sanitize):
    """Plain and with the host sanitizers (a stand-alone program)."""
    exe = H.program("launch_plan_host.cpp", [*H.PLAN, *(H.HOST_SAN if sanitize else ())])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "launch plan ok" in r.stdout
