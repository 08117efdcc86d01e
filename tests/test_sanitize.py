"""ASan + UBSan build of the host code (SURVEY.md §5 "Race detection / sanitizers").

json.cpp, scene.cpp, compile.cpp, image.cpp (the product's loader, scene compiler and image writer) and
oracle/rt_oracle.cpp (the CPU restatement) are compiled with -fsanitize=address,undefined and
-fno-sanitize-recover=all, and tests/cpp/sanitize_host.cpp drives them over every committed scene (load,
compile in both list modes, again with the step limit at 1, at 10 and one below the program's length, where the
threaded program is given up part-way and must leave a stack-traversal scene, and once with every compile
option at its non-default value, camera at the BASELINE sizes, a small oracle render in both product orders),
every byte prefix and 400 single-byte corruptions of each scene document, the malformed documents of
tests/test_loader.py, the camera files' WriteCamera round trip and WriteImage in both formats. Any
sanitizer report aborts the run. CPU only; the GPU code is not built here (no device sanitizer on this
pool)."""
import glob
import os

import pytest

import host_build as H
from host_build import ROOT

BAD_DOCS = [
    '{"materials": [{"type": "plastic"}], "camera": {}}',
    '{"materials": [{"albedo": [1,1,1]}], "camera": {}}',
    '{"camera": {}, "materials": [{"type":"lambertian"}], "primitives": [{"type":"quad"}], "scene": [{"primitive": 3}]}',
    '{"camera": {}, "materials": [], "primitives": [], "scene": []}',
    '{"camera": {}, "materials": [{"type":"lambertian"}], "primitives": [{"type":"quad","material":5}], '
    '"scene": [{"primitive": 0}]}',
    '{"camera": {"fov": 40,',
    '{"camera": {"center": [0, 0, 1]}, "materials": [{"type": "lambertian"}], '
    '"primitives": {"triangles": [{"material_id": 0}]}}',
    '{"camera": {}, "materials": [{"type":"lambertian"}], "primitives": [{"type":"sphere","center":[0,0]}], '
    '"scene": [{"primitive": 0}]}',
    '{"camera": {}, "materials": [{"type":"lambertian"}], "primitives": [{"type":"quad"}], '
    '"scene": [{"children": [{"children": [{"primitive": -1}]}]}]}',
    '[1e999999, "\\ud800", "\\u00zz"]',
    '{"a": ' * 4000,
    '',
]


@pytest.fixture(scope="module")
def sanitized():
    return H.program("sanitize_host.cpp", H.SANITIZE, ("oracle/rt_oracle.cpp", *H.COMPILER_SOURCES, "image.cpp"))


def test_host_code_is_clean_under_asan_and_ubsan(sanitized, tmp_path):
    scenes = sorted(p for p in glob.glob(os.path.join(ROOT, "scenes", "*.json")) if not p.endswith("cam.json")
                    and not p.endswith("cam1.json"))
    scenes += sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "scenes", "*.json")))
    bad = []
    for i, doc in enumerate(BAD_DOCS):
        p = tmp_path / f"bad{i}.json"
        p.write_text(doc)
        bad.append(str(p))
    cams = [os.path.join(ROOT, "scenes", "cam1.json"), os.path.join(ROOT, "scenes", "scene2_cam.json")]
    out = H.run(sanitized, ["--out", str(tmp_path), "--good", *scenes, "--bad", *bad, "--camera", *cams], 1200,
                env=H.SANITIZE_ENV)
    assert out.startswith("documents=")
    assert int(out.split()[0].split("=")[1]) > 5000  # (every scene, its prefixes and corruptions)
