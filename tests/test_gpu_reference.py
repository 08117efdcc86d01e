"""The kernels against the reference itself, through the fixtures of tests/golden/ref (recorded from the
compiled reference by tests/golden/make_ref_golden.py; tests/test_reference_build.py keeps them honest): the
first-hit records of tr.features() against the reference's own Hit on the 32x18 pixel-centre rays, and depth-1
renders against the reference's own RayTracer::Update, bit for bit. Nothing here reads the reference or the
compiled reference library."""
import os

import numpy as np
import pytest

from bits import f32_bits
from conftest import ROOT, scene_path
from helpers import SEED, gpu_render
from test_gpu_parity import CASES, MODES

pytestmark = pytest.mark.gpu
REF = os.path.join(ROOT, "tests", "golden", "ref")
W, H = 32, 18
SPP = {c[0]: c[3] for c in CASES}
HIT_SCENES = sorted(f[:-len("_hits.npy")] for f in os.listdir(REF) if f.endswith("_hits.npy"))
DEPTH1_SCENES = sorted(f[:-len("_depth1.npy")] for f in os.listdir(REF) if f.endswith("_depth1.npy"))


def test_the_fixtures_cover_the_cases():
    media = {"cornell_box_volume", "book2_final_scene_10000_samples"}
    assert set(HIT_SCENES) == set(SPP) - media
    assert len(DEPTH1_SCENES) >= 4 and set(DEPTH1_SCENES) <= set(HIT_SCENES)
    assert "cornell_box_original" in DEPTH1_SCENES  # a transformed child, the flat walk
    assert "perlin_spheres" in DEPTH1_SCENES  # a background that is not black


@pytest.mark.parametrize("name", HIT_SCENES)
def test_first_hits_match_the_reference(have_gpu, name):
    """tr.features() slots 0-9 against the reference's Hit: the flag everywhere, the record where hit, and
    the camera words the rays are built from."""
    import raytrace2_amd as R
    fx = np.load(os.path.join(REF, name + "_hits.npy"))
    cam, ref = fx[:21], fx[21:].reshape(H, W, 10)
    sc = R.Scene(scene_path(name), SEED)
    tr = R.RayTracer(sc, 0)
    tr.set_seed(SEED)
    tr.SetSamplesPerPixel(SPP[name])
    tr.OnResize((W, H))
    assert np.array_equal(f32_bits(sc.camera_params(W, H, SPP[name])), f32_bits(cam))
    got = tr.features()
    tr.close()
    assert got.shape == (H, W, 16)
    assert np.array_equal(got[..., 0], ref[..., 0]), "hit flags differ"
    hit = ref[..., 0] == 1
    assert hit.any()
    words = f32_bits(got[hit][:, 1:10]) != f32_bits(ref[hit][:, 1:10])
    assert not words.any(), f"{np.count_nonzero(words)} words differ, first at pixel {np.argwhere(hit)[np.argwhere(words)[0][0]]}"


@pytest.mark.parametrize("mode", ["linear", "stack_global"])
@pytest.mark.parametrize("name", DEPTH1_SCENES)
def test_depth1_matches_the_reference(have_gpu, monkeypatch, name, mode):
    """max_depth 1, spp setting 4, 6 frames: emission or background of the first hit, summed in frame order,
    equals the reference's own Update bit for bit, with one ray per path."""
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    ref = np.load(os.path.join(REF, name + "_depth1.npy"))
    acc, _, st, _ = gpu_render(name, W, H, 4, 6, max_depth=1)
    assert np.array_equal(f32_bits(acc), f32_bits(ref)), f"{np.count_nonzero(f32_bits(acc) != f32_bits(ref))} words differ"
    assert st["rays"] == W * H * 6


def test_depth1_cornell_without_the_flat_walk(have_gpu, monkeypatch):
    monkeypatch.setenv("RT2_FLAT_BVH", "0")  # read at scene load
    ref = np.load(os.path.join(REF, "cornell_box_original_depth1.npy"))
    acc, _, st, _ = gpu_render("cornell_box_original", W, H, 4, 6, max_depth=1)
    assert np.array_equal(f32_bits(acc), f32_bits(ref))
    assert st["rays"] == W * H * 6
