"""Feature buffers and the variance-guided a-trous denoiser on the GPU (include/rt2.h "Feature buffers and
denoiser"): the feature records against oracle.hit on the pixel-centre rays built in numpy, the filter against
its numpy float32 statement (tests/denoise_ref.py) bit for bit, tracer.denoise() against the same statement on
the oracle's sums, the refusals and rt2_headless --denoise. Images are 70x37 (wider than the 64-pixel reach of
step 16, ragged against the 32x8 tile), spp 16, seed 0x5EED2024."""
import functools
import os
import subprocess

import numpy as np
import pytest

from bits import refused, same_bits
from conftest import ROOT, scene_path
from denoise_ref import denoise_ref, features_ref, synthetic_case, variance_of_sem
from helpers import SEED
from noise_ref import noise_ref

pytestmark = pytest.mark.gpu
W, H, SPP, FRAMES = 70, 37, 16, 16
F32 = np.float32
SCENES = ["cornell_box_original", "final_render_book_1", "cornell_box_volume"]
APP = os.path.join(ROOT, "raytrace2_amd", "lib", "rt2_headless")


def _tracer(name, *, moments=False, **kw):
    import raytrace2_amd as R
    sc = R.Scene(scene_path(name), SEED)
    tr = R.RayTracer(sc, 0, **kw)
    tr.set_seed(SEED)
    tr.SetSamplesPerPixel(SPP)
    tr.OnResize((W, H))
    if moments:
        tr.enable_moments()
    return sc, tr


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle.oracle import OracleScene
    return OracleScene(scene_path(name), SEED)


@functools.lru_cache(maxsize=None)
def _features_ref(name):
    """(records, flagged) from oracle.hit at the scene's own camera, frozen."""
    o = _oracle(name)
    f, flagged = features_ref(o, o.camera_params(W, H, SPP), W, H, SEED)
    f.setflags(write=False)
    return f, flagged


def _assert_features(got, ref, flagged, what):
    hit = ref[..., 0] == 1
    assert np.array_equal(got[..., 0], ref[..., 0]), f"hit flags differ {what}"
    assert hit.any()
    assert same_bits(got[hit][:, 0:10], ref[hit][:, 0:10]), f"hit records differ {what}"
    assert same_bits(got[..., 13], ref[..., 13]), f"dist differs {what}"
    assert same_bits(got[~flagged][:, 10:13], ref[~flagged][:, 10:13]), f"albedo differs {what}"
    assert (got[~hit][:, 1:10] == 0).all() and (got[..., 14:16] == 0).all()


@pytest.mark.parametrize("name", SCENES)
def test_features_match_the_oracle(have_gpu, name):
    """Slots 0-9 bit-equal to oracle.hit where hit, the hit flag everywhere, dist and the untextured albedo.
    Book 1 has a defocus camera: the ray still starts at the camera's centre."""
    ref, flagged = _features_ref(name)
    sc, tr = _tracer(name)
    ocp = _oracle(name).camera_params(W, H, SPP)
    assert same_bits(sc.camera_params(W, H, SPP), ocp)  # the rays are built from camera_params' words
    if name == "final_render_book_1":
        assert ocp[18] > 0  # defocus_angle
    got = tr.features()
    assert got.shape == (H, W, 16)
    _assert_features(got, ref, flagged, name)
    assert not flagged.any() and (ref[..., 0] == 0).any()
    assert same_bits(tr.features(), got)  # the cached buffer
    assert tr.denoise_times()["features_ms"] > 0
    # the tracer still renders what it rendered
    tr.Render(3)
    acc, _, _ = _oracle(name).render(W, H, SPP, 3, forward=True)
    assert same_bits(tr.Accumulation(), acc)
    tr.close()


def test_features_checker_albedo(have_gpu):
    """Every textured hit's albedo is one of the checker's two colours, bit for bit, and both occur."""
    name = "checker_test"
    ref, flagged = _features_ref(name)
    sc, tr = _tracer(name)
    got = tr.features()
    _assert_features(got, ref, flagged, name)
    assert flagged.any()
    alb = got[flagged][:, 10:13]
    even, odd = F32([0, 1, 1]), F32([1, 1, 0])
    is_even, is_odd = (alb == even).all(-1), (alb == odd).all(-1)
    assert (is_even | is_odd).all() and is_even.any() and is_odd.any()
    tr.close()


def test_features_under_a_partition(have_gpu):
    from raytrace2_amd import local_rows
    name = "cornell_box_volume"
    ref, flagged = _features_ref(name)
    rows = local_rows(H, 2, 1, 3)
    sc, tr = _tracer(name)
    full = tr.features()
    tr.set_partition(2, 1, 3)
    part = tr.features()
    assert part.shape == (len(rows), W, 16)
    assert same_bits(part, full[rows])
    _assert_features(part, ref[rows], flagged[rows], "partition")
    tr.close()


def test_features_follow_the_camera(have_gpu):
    name = "cornell_box_original"
    sc, tr = _tracer(name)
    before = tr.features()
    cam = tr.get_camera()
    cam.center = (cam.center[0] + 40.0, cam.center[1] + 25.0, cam.center[2])
    cam.vfov = cam.vfov + 5.0
    tr.set_camera(cam)
    after = tr.features()
    assert not same_bits(before, after)
    from oracle.oracle import OracleScene
    o = OracleScene(scene_path(name), SEED)
    o.set_camera(cam.center, cam.look_at, cam.view_up, cam.vfov, cam.defocus_angle, cam.focus_distance)
    ref, flagged = features_ref(o, o.camera_params(W, H, SPP), W, H, SEED)
    _assert_features(after, ref, flagged, "moved camera")
    # a new seed keys the medium's stream: the buffer is traced again (same records in a scene without media)
    tr.set_seed(SEED + 7)
    assert same_bits(tr.features(), after)
    tr.close()


# ---- denoise_buffers against the numpy statement ---------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (1, 9), (9, 1), (33, 9), (70, 37)])
def test_denoise_buffers_match_numpy_bit_for_bit(have_gpu, size):
    import raytrace2_amd as R
    w, h = size
    c, v, f = synthetic_case(w, h)
    for it in (1, 3, 5, 8):
        rc, rv = denoise_ref(c, v, f, iterations=it)
        gc, gv = R.denoise_buffers(c, v, f, iterations=it)
        assert same_bits(gc, rc), (size, it, "colour")
        assert same_bits(gv, rv), (size, it, "variance")
    gc2, gv2 = R.denoise_buffers(c, v, f, iterations=8)
    assert same_bits(gc2, gc) and same_bits(gv2, gv)  # the same call twice: the same bytes


def test_denoise_buffers_lds_and_direct_paths_agree(have_gpu, monkeypatch):
    """Steps 1 and 2 with their tiles staged in LDS and read from global memory: the same bytes, other
    parameters than the defaults."""
    import raytrace2_amd as R
    c, v, f = synthetic_case(70, 37, seed=5)
    kw = dict(iterations=3, normal_power_log2=2, sigma_l=0.5, sigma_p=0.25, sigma_a=2.0, eps_l=0.125)
    rc, rv = denoise_ref(c, v, f, **kw)
    for lds in ("1", "0"):
        monkeypatch.setenv("RT2_DENOISE_LDS", lds)
        gc, gv = R.denoise_buffers(c, v, f, **kw)
        assert same_bits(gc, rc) and same_bits(gv, rv), f"RT2_DENOISE_LDS={lds}"


# ---- tracer.denoise() ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sums(name):
    o = _oracle(name)
    a, q = np.zeros((H, W, 3), F32), np.zeros((H, W, 3), F32)
    for fr in range(FRAMES):
        s, _, _ = o.render(W, H, SPP, 1, frame_begin=fr, forward=True)
        a = a + s
        q = q + s * s
    a.setflags(write=False)
    q.setflags(write=False)
    return a, q


def test_tracer_denoise_matches_numpy_on_the_oracle_sums(have_gpu):
    import raytrace2_amd as R
    name = "cornell_box_original"
    a, q = _sums(name)
    feat, _ = _features_ref(name)
    sem, _, _ = noise_ref(a, q, FRAMES)
    rc, rv = denoise_ref(a / F32(FRAMES), variance_of_sem(sem), feat)
    sc, tr = _tracer(name, moments=True)
    tr.Render(FRAMES)
    state = (tr.Accumulation(), tr.moments(), tr.FrameIdx())
    gc, gv = tr.denoise(variance=True)
    assert same_bits(gc, rc) and same_bits(gv, rv)
    assert same_bits(tr.denoise(), rc)
    bc, bv = R.denoise_buffers(tr.NonConvertedPixels(), variance_of_sem(tr.standard_error()), tr.features())
    assert same_bits(bc, gc) and same_bits(bv, gv)
    assert tr.denoise_times()["denoise_ms"] > 0
    # other parameters reach the kernel
    kw = dict(iterations=2, sigma_l=3.0)
    assert same_bits(tr.denoise(**kw), denoise_ref(a / F32(FRAMES), variance_of_sem(sem), feat, **kw)[0])
    # the call changed nothing: the sums, the frame index, and what rendering on gives
    assert same_bits(tr.Accumulation(), state[0]) and same_bits(tr.moments(), state[1])
    assert tr.FrameIdx() == state[2] == FRAMES
    tr.Render(5)
    acc, _, _ = _oracle(name).render(W, H, SPP, FRAMES + 5, forward=True)
    assert same_bits(tr.Accumulation(), acc)
    tr.close()


def test_tracer_denoise_with_adaptive_sampling(have_gpu):
    """After render_adaptive the pixels' sample counts differ; the inputs rest on each pixel's own n_p, as the
    readbacks do (tests/test_gpu_adaptive.py pins those to the oracle)."""
    import raytrace2_amd as R
    name = "cornell_box_original"
    sc, tr = _tracer(name, moments=True)
    tr.enable_adaptive()
    out = tr.render_adaptive(float(F32(0.05)), 48, check_every=16)
    n = tr.sample_counts()
    assert len(np.unique(n)) > 1 and out["frames"] == 48
    state = (tr.Accumulation(), tr.moments(), n, tr.FrameIdx())
    c = tr.NonConvertedPixels()
    assert same_bits(c, state[0] / n[..., None].astype(F32))
    v = variance_of_sem(tr.standard_error())
    feat, _ = _features_ref(name)
    rc, rv = denoise_ref(c, v, feat)
    gc, gv = tr.denoise(variance=True)
    assert same_bits(gc, rc) and same_bits(gv, rv)
    bc, bv = R.denoise_buffers(c, v, tr.features())
    assert same_bits(bc, gc) and same_bits(bv, gv)
    assert same_bits(tr.Accumulation(), state[0]) and same_bits(tr.moments(), state[1])
    assert np.array_equal(tr.sample_counts(), state[2]) and tr.FrameIdx() == state[3]
    tr.close()


# ---- refusals -------------------------------------------------------------------------------------------------
def _renders(tr, frames, rows=None):
    """The tracer still renders: `frames` frames from a reset give the oracle's sums."""
    tr.Reset()
    tr.Render(frames)
    acc, _, _ = _oracle("cornell_box_original").render(W, H, SPP, frames, forward=True)
    assert same_bits(tr.Accumulation(), acc if rows is None else acc[rows])


def test_refusals(have_gpu):
    import ctypes
    import raytrace2_amd as R
    from raytrace2_amd import local_rows
    name = "cornell_box_original"
    # moments off
    sc, tr = _tracer(name)
    tr.Render(4)
    refused(tr.denoise)
    _renders(tr, 3)
    # fewer than 2 frames
    tr.enable_moments()
    refused(tr.denoise)
    tr.Render(1)
    refused(tr.denoise)
    # bad parameters, NULL outputs
    tr.Render(3)
    for kw in (dict(iterations=0), dict(iterations=9), dict(normal_power_log2=-1), dict(normal_power_log2=9),
               dict(sigma_l=0.0), dict(sigma_p=float("nan")), dict(sigma_a=float("inf")), dict(eps_l=-1.0)):
        refused(lambda: tr.denoise(**kw))
    assert R.lib.rt2_tracer_denoise(tr._h, None, None, None) == -1
    assert R.lib.rt2_tracer_features(tr._h, None) == -1
    buf = (ctypes.c_float * 16)()
    assert R.lib.rt2_denoise_buffers(0, 1, 1, buf, buf, buf, None, None, None) == -1
    assert tr.denoise().shape == (H, W, 3)
    _renders(tr, 3)
    # a partitioned tracer: features work, denoise does not
    tr.set_partition(2, 1, 3)
    tr.Render(4)
    refused(tr.denoise)
    rows = local_rows(H, 2, 1, 3)
    assert tr.features().shape == (len(rows), W, 16)
    _renders(tr, 3, rows)
    tr.close()
    # a multi tracer over one GPU twice
    sc, multi = _tracer(name, moments=True, devices=[0, 0], band_h=2)
    multi.Render(4)
    refused(multi.denoise)
    refused(multi.features)
    _renders(multi, 3)
    multi.close()
    # a joined world-1 tracer
    sc, tr = _tracer(name)
    tr.join(R.comm_unique_id(), 1, 0, 16)
    tr.enable_moments()
    tr.Render(4)
    refused(tr.denoise)
    refused(tr.features)
    _renders(tr, 3)
    tr.close()


def test_headless_denoise(have_gpu, tmp_path):
    import raytrace2_amd as R
    name = "cornell_box_original"
    png, ref_png = str(tmp_path / "denoised.png"), str(tmp_path / "py.png")
    plain = str(tmp_path / "plain.png")
    for out, extra in ((png, ["--denoise", "--denoise-iterations", "4"]), (plain, [])):
        r = subprocess.run([APP, scene_path(name), out, "--size", f"{W}x{H}", "--samples", str(FRAMES), *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
    sc = R.Scene(scene_path(name), R.DEFAULT_SEED)
    tr = R.RayTracer(sc, 0)
    tr.SetSamplesPerPixel(FRAMES)
    tr.OnResize((W, H))
    tr.enable_moments()
    tr.Render(FRAMES)
    R.WriteImage(tr.denoise(iterations=4), W, H, ref_png)
    tr.close()
    assert open(png, "rb").read() == open(ref_png, "rb").read()
    assert open(png, "rb").read() != open(plain, "rb").read()
