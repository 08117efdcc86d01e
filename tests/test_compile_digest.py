"""Everything the scene compiler produces, for every committed scene under every compile setting, against
digests recorded from the commit before the compiler was split into passes (host only).

tests/cpp/compile_digest.cpp prints, per scene and setting, every scalar of CompiledScene, an FNV-1a digest
of every array and one combined digest. tests/golden/compiled_scene_digests.json holds the combined digest
and the step counts that commit gave (recorded by the same program built with -DDIGEST_PARENT against its
sources: its CompileScene under the RT2_* variables, its CompileSceneWith(bool, int) for the slack row).
Both ways of asking, the environment through CompileScene and CompileOptions through CompileSceneWith, must
reproduce every row and agree with each other.

The step limit is not in the goldens (below the program's length that commit overflowed the heap, and it
read the limit once per process); it is held to its properties: under linear_max_steps = 10 every scene
compiles, a scene with a longer program is exactly a stack-traversal scene (no program array, no table, no
count of it) whose other arrays are those of its default row, and under linear_max_steps = the scene's own
step count the row is the default row."""
import glob
import json
import os
import subprocess

import pytest

import host_build as H
from host_build import ROOT

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "compiled_scene_digests.json")))
ROWS = ["default", "lists_plain", "flat_bvh=0", "flat_bvh=2", "box_aa=0", "bvh_pairs=0", "acc_octants=0", "acc_sah=0",
        "hit_table=0", "acc_depth_slack=0"]
PROGRAM_ARRAYS = ["lin", "lind", "lin_wide", "hit", "flat_wide", "flat_cert"]
PROGRAM_SCALARS = ["steps", "box_steps", "flat_steps", "flat_mode", "lin_xform_depth", "origins_bounded"]
# what a program that is not built leaves alone
SCENE_FIELDS = ["nodes", "materials", "textures", "perlin_vec", "perlin_perm", "root", "max_stack", "hot_records",
                "bvh_nodes", "quads", "spheres", "lists", "xforms", "media", "acc_lists", "acc_nodes", "bvh_depth"]
EMPTY = "a8c7f832281a39c5"  # FNV-1a of an empty array: its length, eight zero bytes


def scenes():
    out = sorted(p for p in glob.glob(os.path.join(ROOT, "scenes", "*.json")) if not p.endswith("cam.json")
                 and not p.endswith("cam1.json"))
    return out + sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "scenes", "*.json")))


@pytest.fixture(scope="module")
def digests():
    """{mode: {scene: {row: {field: text}}}} of both modes"""
    exe = H.program("compile_digest.cpp", H.COMPILER_O2, H.COMPILER_SOURCES)
    out = {}
    env = {k: v for k, v in os.environ.items() if not k.startswith("RT2_")}
    for mode in ("env", "options"):
        r = subprocess.run([exe, mode, *scenes()], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        got = {}
        for line in r.stdout.splitlines():
            f = line.split()
            got.setdefault(f[0], {})[f[1]] = dict(x.split("=", 1) for x in f[2:])
        out[mode] = got
    return out


def test_the_golden_file_covers_every_scene_and_row():
    assert sorted(GOLDEN) == sorted(os.path.basename(p) for p in scenes()) and len(GOLDEN) == 13
    for name, rows in GOLDEN.items():
        assert list(rows) == ROWS, name


@pytest.mark.parametrize("mode", ["env", "options"])
def test_every_row_is_what_the_parent_commit_compiled(digests, mode):
    got = digests[mode]
    assert sorted(got) == sorted(GOLDEN)
    bad = []
    for name, rows in GOLDEN.items():
        for row, want in rows.items():
            g = got[name][row]
            have = {"combined": g["combined"], "steps": int(g["steps"]), "flat_steps": int(g["flat_steps"]),
                    "box_steps": int(g["box_steps"])}
            if g["ok"] != "1" or have != want:
                # (the default row beside it: its arrays' digests name the array that differs)
                print(name, row, "got", g, "\n  want", want, "\n  this build's default row", got[name]["default"])
                bad.append((name, row))
    assert not bad, bad


def test_the_environment_and_the_options_agree(digests):
    for name in digests["env"]:
        assert list(digests["env"][name]) == ROWS + ["linear_max_steps=10", "linear_max_steps=own"]
        for row, e in digests["env"][name].items():
            o = digests["options"][name][row]
            assert e == o, (name, row, {k: (e[k], o.get(k)) for k in e if e[k] != o.get(k)})


@pytest.mark.parametrize("mode", ["env", "options"])
def test_a_program_past_the_step_limit_leaves_no_trace(digests, mode):
    longer = 0
    for name, rows in digests[mode].items():
        d, lim, own = rows["default"], rows["linear_max_steps=10"], rows["linear_max_steps=own"]
        assert own == d, (name, {k: (own[k], d[k]) for k in d if own[k] != d[k]})
        assert lim["ok"] == "1", name
        if int(d["steps"]) <= 10:
            assert lim == d, name
            continue
        longer += 1
        assert [lim[k] for k in PROGRAM_ARRAYS] == [EMPTY] * len(PROGRAM_ARRAYS), (name, lim)
        assert [lim[k] for k in PROGRAM_SCALARS] == ["0"] * len(PROGRAM_SCALARS), (name, lim)
        assert [lim[k] for k in SCENE_FIELDS] == [d[k] for k in SCENE_FIELDS], (name, lim, d)
        assert lim["stack_ok"] == "1" and lim["features"] == d["features"], (name, lim)
    assert longer >= 8  # (every Cornell box, both books)
