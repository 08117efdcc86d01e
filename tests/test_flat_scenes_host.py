"""The slab-decided scenes of tests/flat_scenes.py on the CPU: that they are what tests/test_gpu_flat_scenes.py
needs them to be. No GPU.

  the control     CTL_NO_SLAB (oracle/rt_oracle.cpp: BVHNode::Hit without its slab test) leaves the faithful oracle
                  alone, turns the far box into the near one on rays of the four-leaf class, and visits no fewer
                  BVH nodes.
  per scene       D, the number of pixels whose accumulation differs in any bit between the faithful oracle and
                  CTL_NO_SLAB at 70 x 37, 16 frames of spp 16: at least 50 (about 2 % of the image) for the
                  deciding scenes, 0 for `two` (no inner node). The product's loader gives each a flat program
                  (none to `nine`, one leaf past the limit) and the expected number of transforms.
  the harnesses   tests/cpp/flat_cert.cpp and flat_cert_once.cpp on the scene files: no certified ray disagrees
                  with the BVH walk, every decided ray is uncertified, and the eager and the lazy evaluation of
                  the certificate agree; flat_cert once more under ASan + UBSan.

D as measured here (the oracle is deterministic, so these are properties of the scene files):
mix 170, eight 254 (199 at max_depth 2), nine 253, nonuni 96, norot 95, side 191, metal 188, two 0."""
import numpy as np
import pytest

import flat_scenes as S
import host_build as H
import raytrace2_amd as R
from helpers import SEED
from host_build import SAN
from oracle import oracle as O

# flat_cert's `steps` per scene: what the product's compiler gives these files
STEPS = {"mix": 35, "eight": 43, "nine": 0, "nonuni": 27, "norot": 19, "side": 35, "metal": 35, "two": 16}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_control_leaves_the_faithful_oracle_alone():
    """Mask 0 before, between and after renders under the control: the same bits, rays and counters."""
    assert O.lib().oracle_get_controls() == 0
    path = S.scene_file("norot")
    acc0, rc0, cnt0 = O.OracleScene(path, SEED).render(S.W, S.H, S.SPP, 4, forward=True)
    with O.controls(O.CTL_NO_SLAB):
        assert O.lib().oracle_get_controls() == O.CTL_NO_SLAB == 16
        acc1, rc1, cnt1 = O.OracleScene(path, SEED).render(S.W, S.H, S.SPP, 4, forward=True)
    assert O.lib().oracle_get_controls() == 0
    acc2, rc2, cnt2 = O.OracleScene(path, SEED).render(S.W, S.H, S.SPP, 4, forward=True)
    assert np.array_equal(bits(acc0), bits(acc2)) and np.array_equal(rc0, rc2) and cnt0 == cnt2
    assert not np.array_equal(bits(acc0), bits(acc1)), "the control changed nothing"
    # a scene loaded under the control and rendered without it is the faithful one too: the bit acts at Hit
    with O.controls(O.CTL_NO_SLAB):
        o = O.OracleScene(path, SEED)
    acc3, rc3, cnt3 = o.render(S.W, S.H, S.SPP, 4, forward=True)
    assert np.array_equal(bits(acc0), bits(acc3)) and cnt0 == cnt3
    assert cnt1["bvh"] >= cnt0["bvh"] > 0, (cnt0, cnt1)


def test_without_the_slab_test_the_near_box_wins():
    """200 rays from x = 1000 down -x through B (near, scale 16) and A (far, scale 8) of `norot`: A is visited
    first and reports a model-space t of about 835 / 8; B's subtree enters at a world t of 2,350 or more and is
    culled. Without the slab test B is visited with that tmax and reports about 235 / 16."""
    o, d = S.four_leaf_rays(200)
    sc = O.OracleScene(S.scene_file("norot"), SEED)
    faithful = np.array([sc.hit(a, b) for a, b in zip(o, d)])
    with O.controls(O.CTL_NO_SLAB):
        open_ = np.array([sc.hit(a, b) for a, b in zip(o, d)])
    again = np.array([sc.hit(a, b) for a, b in zip(o, d)])
    assert np.array_equal(bits(faithful), bits(again))
    assert (faithful[:, 0] == 1).all() and (open_[:, 0] == 1).all()
    assert (faithful[:, 9] == S.MATERIAL_A).all(), faithful[:, 9]
    assert (open_[:, 9] == S.MATERIAL_B).all(), open_[:, 9]
    assert (open_[:, 1] < faithful[:, 1]).all()  # (model-space t: 235 / 16 against 835 / 8)


@pytest.mark.parametrize("name", list(S.SCENES))
def test_the_slab_tests_decide_enough_pixels(name):
    m = S.decided(name)
    _, c0 = S.oracle_render(name, 0)
    _, c1 = S.oracle_render(name, O.CTL_NO_SLAB)
    print(f"{name}: D = {int(m.sum())} of {m.size} pixels; rays {c0['rays']} (no slab test: {c1['rays']}), "
          f"bvh {c0['bvh']} (no slab test: {c1['bvh']})")
    assert m.shape == (S.H, S.W) and m.size % 64 != 0
    if name == "two":
        assert m.sum() == 0 and c0["rays"] == c1["rays"]
    else:
        assert m.sum() >= S.D_MIN, int(m.sum())
    assert c1["bvh"] >= c0["bvh"] > 0
    if name == "eight":  # the render at max_depth 2 that the GPU test uses
        m2 = S.decided(name, 2)
        print(f"{name} at max_depth 2: D = {int(m2.sum())}")
        assert m2.sum() >= S.D_MIN, int(m2.sum())


@pytest.mark.parametrize("name", list(S.SCENES))
def test_the_product_loader_gives_each_scene_its_program(name, monkeypatch):
    monkeypatch.delenv("RT2_FLAT_BVH", raising=False)
    i = R.Scene(S.scene_file(name), SEED).info()
    print(name, "leaves", S.leaves(name), "flat_steps", i.flat_steps, "linear_steps", i.linear_steps, "xforms", i.xforms)
    assert i.n_top_nodes == S.leaves(name) and i.xforms == S.xforms(name) and i.media == 0 and i.spheres == 0
    assert i.quads == 6 * S.xforms(name) + S.leaves(name) - S.xforms(name)
    assert i.flat_steps == STEPS[name]
    if name in S.COMPILED_FLAT:
        assert 0 < i.flat_steps < i.linear_steps
    monkeypatch.setenv("RT2_FLAT_BVH", "0")
    assert R.Scene(S.scene_file(name), SEED).info().flat_steps == 0


def _run(tmp_path, source, flags, rays, names):
    exe = H.program(source + ".cpp", [*H.COMPILER, *flags], H.COMPILER_SOURCES)
    return H.parse(H.run(exe, [str(tmp_path), "1", str(rays), "0", *[S.scene_file(n) for n in names]], 900,
                         drop=["RT2_FLAT_BVH"]))


@pytest.mark.parametrize("flags,rays", [([], 60000), (SAN, 6000)], ids=["plain", "asan_ubsan"])
def test_no_certified_ray_of_these_scenes_disagrees_with_the_bvh_walk(tmp_path, flags, rays):
    got = _run(tmp_path, "flat_cert", flags, rays, list(S.SCENES))
    for name in S.SCENES:
        v = got["scene:" + name + ".json"]
        assert v["bad"] == 0 and v["decided"] == v["decided_uncertified"], (name, v)
        assert v["flat"] == (name in S.COMPILED_FLAT) and v["steps"] == STEPS[name], (name, v)
        if name in S.DECIDING:
            assert v["rays"] >= rays and v["decided"] > 0 and v["certified"] > 0, (name, v)
        else:  # `two` has no slab test below the root's; `nine` has no flat program to walk
            assert v["decided"] == 0, (name, v)


def test_the_eager_and_the_lazy_certificate_agree_on_these_scenes(tmp_path):
    rays = 60000
    got = _run(tmp_path, "flat_cert_once", [], rays, list(S.COMPILED_FLAT))
    for name in S.COMPILED_FLAT:
        v = got["scene:" + name + ".json"]
        assert v["bad"] == 0 and v["flat"] == 1 and v["steps"] == STEPS[name], (name, v)
        assert v["rays"] >= rays and v["hits"] > 0 and v["table_rows"] == 6 * S.xforms(name), (name, v)
        if name in S.DECIDING:
            assert v["rule_uncert_xform"] > 0, (name, v)
