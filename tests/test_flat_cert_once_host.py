"""The flat walk's certificate evaluated once per trace (render.hip trace_linear with kFlat; DESIGN.md §4 "Flat
walk of small BVHs"), host only: tests/cpp/flat_cert_once.cpp compiles scenes with the product's compiler,
checks that the certificate table gives every quad under a transform that transform's certificate box bit for
bit, and walks the flat program twice per ray: with the entry rule evaluated at every transform entry and the
end rule at the end (the earlier evaluation, restated there), and with the one lazy rule that reads the box
from the table. The two must agree on the hit and on `uncertified` for every ray. The program is built
stand-alone, plainly and with ASan + UBSan.

Cases, drawn as tests/cpp/flat_cert.cpp draws them: the committed scenes that get a flat program at 60,000 rays
each, generated scenes of 2 to 8 BVH leaves, the four-leaf scene."""
import os

import pytest

import host_build as H
from host_build import ROOT, SAN

FLAT_SCENES = ["cornell_box_original", "cornell_box1", "cornell_box2", "quad_scene1"]


@pytest.mark.parametrize("flags,rays,generated", [([], 60000, 56), (SAN, 6000, 28)], ids=["plain", "asan_ubsan"])
def test_one_lazy_rule_decides_what_the_entry_and_end_rules_decided(tmp_path, flags, rays, generated):
    exe = H.program("flat_cert_once.cpp", [*H.COMPILER, *flags], H.COMPILER_SOURCES)
    scenes = [os.path.join(ROOT, "scenes", n + ".json") for n in FLAT_SCENES]
    got = H.parse(H.run(exe, [str(tmp_path), "1", str(rays), str(generated), *scenes], 900, drop=["RT2_FLAT_BVH"]))
    assert set(got) == {"scene:" + n + ".json" for n in FLAT_SCENES} | {"generated", "four_leaf"}, sorted(got)
    # 0 disagreements, every scene walked
    for k, v in got.items():
        assert v["bad"] == 0 and v["flat"] == 1 and v["rays"] > 0 and v["hits"] > 0, (k, v)
    for n in FLAT_SCENES:
        assert got["scene:" + n + ".json"]["rays"] >= rays, got
    # not vacuous: the rule leaves hits uncertified under a transform and in world space (rays with a finite
    # reciprocal, so the rule and not the reciprocal decided), and the table check saw transformed quads
    under = sum(v["rule_uncert_xform"] for v in got.values())
    world = sum(v["rule_uncert_world"] for v in got.values())
    assert under > 0 and world > 0, got
    c = got["scene:cornell_box_original.json"]
    assert c["steps"] == 22 and c["table_rows"] == 12 and c["rule_uncert_xform"] > 0 and c["rule_uncert_world"] > 0, c
    assert got["generated"]["table_rows"] > 0 and got["generated"]["nonfinite"] > 0, got["generated"]
    four = got["four_leaf"]
    assert four["rays"] == 160000 and four["table_rows"] == 12, four
