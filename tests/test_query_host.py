"""The ray queries' host side (raytrace2_amd/csrc/query.h QueryRayValid, launch_plan.h PlanQuery, built into the
stand-alone tests/cpp/query_host.cpp): the validity rule at every edge of its domain and the launch plan at the
wave edges, with and without a threaded program, for every kernel variant. No GPU."""
import subprocess

import pytest

import host_build as H


@pytest.mark.parametrize("sanitize", [False, True])
def test_query_host(sanitize):
    """Plain and with the host sanitizers (a stand-alone program)."""
    exe = H.program("query_host.cpp", [*H.HOST, *(H.HOST_SAN if sanitize else ())])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "query host ok" in r.stdout
