"""The flat walk's certificate (rt2_layout.h "Flat program", boxaa.h FlatCertRule; DESIGN.md §4 "Flat walk of
small BVHs"), host only: tests/cpp/flat_cert.cpp compiles scenes with the product's compiler and executes, per
ray, the BVH program's walk and the flat program's walk with its certificate as the kernel executes them for
one lane. A ray whose two walks disagree (in primitive, t or interval key) is a ray a slab test decides; every
such ray must be uncertified (the kernel then traces the BVH program for it), and no certified ray may
disagree. The program is built stand-alone, plainly and with ASan + UBSan.

Cases: the committed scenes (those that qualify get a flat program, the others none); generated scenes of 2 to
8 BVH leaves; the four-leaf scene in which a transformed box's model-space t makes the reference cull the
subtree that holds the true nearest hit, where the slab test decides every ray."""
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


@pytest.mark.parametrize("flags,rays,generated", [([], 60000, 56), (SAN, 6000, 28)], ids=["plain", "asan_ubsan"])
def test_no_certified_ray_disagrees_with_the_bvh_walk(tmp_path, flags, rays, generated):
    exe = str(tmp_path / "flat_cert")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", *flags, "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "flat_cert.cpp")]
                       + [os.path.join(CSRC, f) for f in ("json.cpp", "scene.cpp", "compile.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("RT2_FLAT_BVH", None)
    r = subprocess.run([exe, str(tmp_path), "1", str(rays), str(generated), *scenes()], capture_output=True, text=True,
                       env=env, timeout=900)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    got = {}
    for line in r.stdout.splitlines():
        f = line.split()
        got[f[0]] = {k: int(v) for k, v in (x.split("=") for x in f[1:])}
    for v in got.values():
        assert v["bad"] == 0 and v["decided"] == v["decided_uncertified"], got
    # which committed scenes qualify: those get a flat program shorter than their BVH program
    flat = {k[len("scene:"):-len(".json")] for k, v in got.items() if k.startswith("scene:") and v["flat"]}
    assert flat == QUALIFY, flat
    assert len([k for k in got if k.startswith("scene:")]) == len(scenes())
    # the rays are not vacuous: slab tests decide some, and the certificate covers most hits of interior rays
    c = got["scene:cornell_box_original.json"]
    assert c["steps"] == 22 and c["hits"] > 0 and c["decided"] > 0 and c["certified"] > c["uncertified"], c
    g = got["generated"]
    assert g["steps"] >= generated * 3 // 4, g  # (generated scenes that got a flat program)
    assert g["decided"] > 0 and g["certified"] > 0 and g["nonfinite"] > 0, g
    # the four-leaf scene: the slab test decides every ray, and the certificate leaves every one open
    four = got["four_leaf"]
    assert four["rays"] == 160000 and four["decided"] == four["rays"] == four["uncertified"] and four["certified"] == 0, four
