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

import pytest

import host_build as H
from host_build import ROOT, SAN

QUALIFY = {"cornell_box_original", "cornell_box1", "cornell_box2", "quad_scene1", "cornell_original_10000_samples"}


def scenes():
    out = sorted(p for p in glob.glob(os.path.join(ROOT, "scenes", "*.json")) if not p.endswith("cam.json")
                 and not p.endswith("cam1.json"))
    return out + sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "scenes", "*.json")))


@pytest.mark.parametrize("flags,generated", [([], 112), (SAN, 56)], ids=["plain", "asan_ubsan"])
def test_no_flat_program_step_sends_lanes_to_different_places(tmp_path, flags, generated):
    exe = H.program("flat_program_shape.cpp", [*H.COMPILER, *flags], H.COMPILER_SOURCES)
    got = H.parse(H.run(exe, [str(tmp_path), "1", str(generated), *scenes()], 600, drop=["RT2_FLAT_BVH"]))
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
