"""The ray queries' host side (raytrace2_amd/csrc/query.h QueryRayValid, launch_plan.h PlanQuery, built into the
stand-alone tests/cpp/query_host.cpp): the validity rule at every edge of its domain and the launch plan at the
wave edges, with and without a threaded program, for every kernel variant. No GPU."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "raytrace2_amd", "csrc")


@pytest.mark.parametrize("sanitize", [False, True])
def test_query_host(tmp_path, sanitize):
    """Plain and with the host sanitizers (a stand-alone program)."""
    exe = str(tmp_path / ("query_host_san" if sanitize else "query_host"))
    extra = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g") if sanitize else ()
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC,
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "query_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "query host ok" in r.stdout
