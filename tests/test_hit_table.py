"""The hit table the scene compiler builds for the threaded program (rt2_layout.h HIT, compile.cpp
BuildHitTable), host only: tests/cpp/hit_table.cpp checks, for every committed scene, that each hit
record equals bit for bit the words the kernel's global-memory chain reads from lind, materials and
textures, that every quad step's record offset addresses its record in the table, and that
RT2_HIT_TABLE=0 builds none. The program is built stand-alone, plainly and with ASan + UBSan."""
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytrace2_amd", "csrc")
SAN = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def scenes():
    out = sorted(p for p in glob.glob(os.path.join(ROOT, "scenes", "*.json")) if not p.endswith("cam.json")
                 and not p.endswith("cam1.json"))
    return out + sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "scenes", "*.json")))


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_hit_records_are_bit_copies_of_what_the_chain_reads(tmp_path, flags):
    exe = str(tmp_path / "hit_table")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", *flags, "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "hit_table.cpp")]
                       + [os.path.join(CSRC, f) for f in ("json.cpp", "scene.cpp", "compile.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, *scenes()], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    got = {}
    for line in r.stdout.splitlines():
        f = line.split()
        got[os.path.basename(f[0])[:-5]] = {k: int(v) for k, v in (x.split("=") for x in f[1:])}
    assert len(got) == len(scenes())
    # the Cornell box: 18 quads under at most one transform each, two transforms, a table the kernel can stage
    c = got["cornell_box_original"]
    assert (c["quads"], c["xforms"], c["depth"]) == (18, 2, 1) and 0 < c["hit_bytes"] <= 6144, c
    # nested transforms get no table; neither do the books (no quads, or far too many records)
    assert got["cornell_box_scene_graph"]["depth"] > 1 and got["cornell_box_scene_graph"]["hit_bytes"] == 0
    assert got["final_render_book_1"]["hit_bytes"] == 0 and got["book2_final_scene_10000_samples"]["hit_bytes"] == 0
    assert sum(1 for v in got.values() if v["hit_bytes"] > 0) >= 2, got
