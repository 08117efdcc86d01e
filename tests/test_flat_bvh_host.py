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

import pytest

import host_build as H
from host_build import ROOT, SAN

QUALIFY = {"cornell_box_original", "cornell_box1", "cornell_box2", "quad_scene1", "cornell_original_10000_samples"}


def scenes():
    out = sorted(p for p in glob.glob(os.path.join(ROOT, "scenes", "*.json")) if not p.endswith("cam.json")
                 and not p.endswith("cam1.json"))
    return out + sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "scenes", "*.json")))


@pytest.mark.parametrize("flags,rays,generated", [([], 60000, 56), (SAN, 6000, 28)], ids=["plain", "asan_ubsan"])
def test_no_certified_ray_disagrees_with_the_bvh_walk(tmp_path, flags, rays, generated):
    exe = H.program("flat_cert.cpp", [*H.COMPILER, *flags], H.COMPILER_SOURCES)
    got = H.parse(H.run(exe, [str(tmp_path), "1", str(rays), str(generated), *scenes()], 900, drop=["RT2_FLAT_BVH"]))
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
