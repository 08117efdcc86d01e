"""The hit table the scene compiler builds for the threaded program (rt2_layout.h HIT, compile.cpp
BuildHitTable), host only: tests/cpp/hit_table.cpp checks, for every committed scene, that each hit
record equals bit for bit the words the kernel's global-memory chain reads from lind, materials and
textures, that every quad step's record offset addresses its record in the table, and that
RT2_HIT_TABLE=0 builds none. The program is built stand-alone, plainly and with ASan + UBSan."""
import glob
import os

import pytest

import host_build as H
from host_build import ROOT, SAN



def scenes():
    out = sorted(p for p in glob.glob(os.path.join(ROOT, "scenes", "*.json")) if not p.endswith("cam.json")
                 and not p.endswith("cam1.json"))
    return out + sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "scenes", "*.json")))


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_hit_records_are_bit_copies_of_what_the_chain_reads(tmp_path, flags):
    exe = H.program("hit_table.cpp", [*H.COMPILER, *flags], H.COMPILER_SOURCES)
    got = H.parse(H.run(exe, scenes(), 600), name=lambda path: os.path.basename(path)[:-5])
    assert len(got) == len(scenes())
    # the Cornell box: 18 quads under at most one transform each, two transforms, a table the kernel can stage
    c = got["cornell_box_original"]
    assert (c["quads"], c["xforms"], c["depth"]) == (18, 2, 1) and 0 < c["hit_bytes"] <= 6144, c
    # nested transforms get no table; neither do the books (no quads, or far too many records)
    assert got["cornell_box_scene_graph"]["depth"] > 1 and got["cornell_box_scene_graph"]["hit_bytes"] == 0
    assert got["final_render_book_1"]["hit_bytes"] == 0 and got["book2_final_scene_10000_samples"]["hit_bytes"] == 0
    assert sum(1 for v in got.values() if v["hit_bytes"] > 0) >= 2, got
