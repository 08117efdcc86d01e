"""The premise of the flat walk's scalar step index (render.hip trace_linear with kFlat; DESIGN.md §4 "The step
index as a scalar"), host only: tests/cpp/flat_program_shape.cpp compiles scenes with the product's compiler and
checks on every flat program that no step sends lanes to different places. Every entry is a kQuad, kXform,
kXformExit or kProgramEnd entry; a quad entry's successor at + run and every other entry's at + 1 land on an
entry start; and following the successors from 0 reaches kProgramEnd in at most flat_steps moves, through each
transform's entry and exit exactly once. The program is built stand-alone, plainly and with ASan + UBSan.

Cases: the committed scenes (those that qualify get a flat program, the others none) and generated scenes of 2
to 8 BVH leaves (the generator of tests/cpp/flat_cert.cpp)."""
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytrace2_amd", "csrc")
SAN = ["-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
QUALIFY = {"cornell_box_original", "cornell_box1", "cornell_box2", "quad_scene1", "cornell_original_10000_samples"}


def scenes():
    out = sorted(p for p in glob.glob(os.path.join(ROOT, "scenes", "*.json")) if not p.endswith("cam.json")
                 and not p.endswith("cam1.json"))
    return out + sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "scenes", "*.json")))


@pytest.mark.parametrize("flags,generated", [([], 112), (SAN, 56)], ids=["plain", "asan_ubsan"])
def test_no_flat_program_step_sends_lanes_to_different_places(tmp_path, flags, generated):
    exe = str(tmp_path / "flat_program_shape")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", *flags, "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I", CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "flat_program_shape.cpp")]
                       + [os.path.join(CSRC, f) for f in ("json.cpp", "scene.cpp", "compile.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("RT2_FLAT_BVH", None)
    r = subprocess.run([exe, str(tmp_path), "1", str(generated), *scenes()], capture_output=True, text=True, env=env,
                       timeout=600)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    got = {}
    for line in r.stdout.splitlines():
        f = line.split()
        got[f[0]] = {k: int(v) for k, v in (x.split("=") for x in f[1:])}
    # which committed scenes qualify: every one of them was checked
    flat = {k[len("scene:"):-len(".json")] for k, v in got.items() if k.startswith("scene:") and v["flat"]}
    assert flat == QUALIFY, flat
    assert len([k for k in got if k.startswith("scene:")]) == len(scenes())
    for k, v in got.items():
        if k.startswith("scene:") and v["flat"]:
            assert 0 < v["moves"] <= v["steps"] and v["quad_steps"] > 0, (k, v)
    # the Cornell box: 22 steps, its two boxes' transforms on the walk; quad_scene1: a flat program without one
    c = got["scene:cornell_box_original.json"]
    assert c["steps"] == 22 and c["xforms"] == 2 and c["moves"] < c["steps"], c  # (runs: fewer moves than steps)
    assert got["scene:quad_scene1.json"]["xforms"] == 0, got["scene:quad_scene1.json"]
    # the generated scenes are not vacuous: most get a flat program, of every leaf count, with transforms among them
    g = got["generated"]
    assert g["flat"] >= generated * 3 // 4 and g["xforms"] > 0 and 0 < g["moves"] <= g["steps"], g
    assert g["leaves_mask"] == sum(1 << n for n in range(2, 9)), g
