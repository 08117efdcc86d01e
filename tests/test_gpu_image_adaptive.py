"""Adaptive sampling of the gathered image on the GPU (include/rt2.h "Adaptive sampling of the gathered image"):
a create_multi or joined tracer retires converged pixels like a one-GPU tracer, its checks' scalars are summed over
the parts, and every pixel's sample count travels with the gather, so the gathered image, its estimate and its
reconstruction are those of the one-GPU adaptive tracer, bit for bit. The reference in every test is a plain
one-GPU tracer through the existing entry points (tests/test_gpu_adaptive.py pins those to the oracle), never the
calls under test. The shapes are that file's: 40x24 pixels, spp 16, seed 0x5EED2024, threshold float32(0.05),
window 1, steps of 16 frames up to 80."""
import dataclasses
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from bits import refused, same_bits
from conftest import ROOT, scene_path
from denoise_ref import variance_of_sem
from helpers import SEED

pytestmark = pytest.mark.gpu
W, H, SPP, MAXF, STEP = 40, 24, 16, 80, 16
THR = float(np.float32(0.05))
NPIX = W * H
NAME = "cornell_box_original"
F32 = np.float32
APP = os.path.join(ROOT, "raytrace2_amd", "lib", "rt2_headless")
FIELDS = ("pixels", "active", "retired", "samples", "nonfinite")


def _tracer(name=NAME, *, moments=True, **kw):
    import raytrace2_amd as R
    sc = R.Scene(scene_path(name), SEED)
    tr = R.RayTracer(sc, 0, **kw)
    tr.set_seed(SEED)
    tr.SetSamplesPerPixel(SPP)
    tr.OnResize((W, H))
    if moments:
        tr.enable_moments()
    return sc, tr


def _multi(name=NAME, n=3, band_h=2):
    sc, tr = _tracer(name, devices=[0] * n, band_h=band_h)
    tr.image_enable_adaptive()
    return sc, tr


def _state(tr):
    """What the comparisons take of a plain adaptive tracer."""
    s = dict(acc=tr.Accumulation(), n=tr.sample_counts(), nc=tr.NonConvertedPixels(), px=tr.Pixels(), mom=tr.moments(),
             sem=tr.standard_error())
    for a in s.values():
        a.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _plain(name=NAME, max_frames=MAXF):
    """The one-GPU reference after render_adaptive(THR, max_frames, check_every=STEP): its dict, the active pixels
    before the last step and its state. The run is made of two calls (the loop continues from FrameIdx()), so the
    check before the last step can be read."""
    sc, tr = _tracer(name)
    tr.enable_adaptive()
    before = tr.render_adaptive(THR, max_frames - STEP, check_every=STEP)
    out = tr.render_adaptive(THR, max_frames, check_every=STEP)
    ref = dict(out=out, before=before, **_state(tr))
    tr.close()
    # a divide by the frame index would not pass: pixels are still active before the last step, others have
    # retired, and the image mixes sample counts
    assert 0 < before["active"] < NPIX and before["frames"] == max_frames - STEP and out["frames"] == max_frames
    assert len(np.unique(ref["n"])) >= 3
    return ref


@functools.lru_cache(maxsize=None)
def _plain13():
    sc, tr = _tracer(moments=False)
    tr.Render(13)
    acc = tr.Accumulation()
    tr.close()
    acc.setflags(write=False)
    return acc


def _assert_gathered(tr, ref, what=""):
    """The gathered image's readbacks against the plain tracer's state."""
    assert same_bits(tr.image_accumulation(), ref["acc"]), f"image_accumulation {what}"
    assert np.array_equal(tr.image_sample_counts(), ref["n"]), f"image_sample_counts {what}"
    assert same_bits(tr.image_non_converted_pixels(), ref["nc"]), f"image_non_converted_pixels {what}"
    assert np.array_equal(tr.image_pixels(), ref["px"]), f"image_pixels {what}"


def _whole_run(name, n, band_h):
    ref = _plain(name)
    sc, tr = _multi(name, n, band_h)
    out = tr.image_render_adaptive(THR, MAXF, check_every=STEP)
    print(name, n, band_h, "product", out, "reference", ref["out"], "before the last step", ref["before"])
    assert out == ref["out"] and tr.FrameIdx() == MAXF
    tr.gather()
    _assert_gathered(tr, ref, (name, n, band_h))
    # the multi tracer's own readbacks
    assert same_bits(tr.Accumulation(), ref["acc"])
    assert same_bits(tr.NonConvertedPixels(), ref["nc"])
    assert np.array_equal(tr.Pixels(), ref["px"])
    assert same_bits(tr.moments(), ref["mom"])
    assert same_bits(tr.standard_error(), ref["sem"])
    tr.close()


# ---- 1, 2. the whole run, bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("n,band_h", [(1, 16), (2, 5), (3, 2), (5, 2)])
def test_whole_run_matches_one_gpu(have_gpu, n, band_h):
    """devices=[0] is the RCCL path (a communicator of size 1); (2, 5) has a ragged last band, 14 rows against 10;
    (5, 2) stacks of 4, 4, 6, 6, 4 rows: the counts' padding rows are sent."""
    _whole_run(NAME, n, band_h)


@pytest.mark.parametrize("name", ["final_render_book_1", "cornell_box_volume"])
def test_other_scenes(have_gpu, name):
    _whole_run(name, 3, 2)


# ---- 3. the sum over the parts --------------------------------------------------------------------------------------
def test_check_sums_the_parts_and_waits_once_per_part(have_gpu):
    n = 3
    sc, tr = _multi(NAME, n, 2)
    sc1, plain = _tracer()
    plain.enable_adaptive()
    for t in (tr, plain):
        t.Render(STEP)
    tr.flush()
    refused(lambda: tr.image_part_adaptive(0))  # no check yet
    w0 = tr.stats()["host_waits"]
    out = tr.image_adaptive_check(THR, 1)
    w1 = tr.stats()["host_waits"]
    assert out == plain.adaptive_check(THR, 1) and 0 < out["retired"] < NPIX
    assert w1 - w0 <= n, (w0, w1)
    parts = [tr.image_part_adaptive(p) for p in range(n)]
    print(out, parts)
    for f in FIELDS:
        assert sum(p[f] for p in parts) == out[f], f
    assert all(p["frames"] == STEP for p in parts) and [p["pixels"] for p in parts] == [W * 8] * n
    refused(lambda: tr.image_part_adaptive(n))
    refused(lambda: tr.image_part_adaptive(-1))
    tr.close()
    plain.close()


# ---- 4. estimate and reconstruction ---------------------------------------------------------------------------------
def _moved(cam):
    d = float(np.linalg.norm(np.subtract(cam.center, cam.look_at)))
    return dataclasses.replace(cam, center=(cam.center[0] + 0.15 * d, cam.center[1] + 0.07 * d, cam.center[2]))


def test_estimate_and_reconstruction(have_gpu):
    sc, multi = _multi(NAME, 3, 2)
    sc1, plain = _tracer()
    plain.enable_adaptive()
    cam = plain.get_camera()
    multi.set_camera(cam)
    plain.set_camera(cam)
    ref_out = plain.render_adaptive(THR, 48, check_every=STEP)
    assert multi.image_render_adaptive(THR, 48, check_every=STEP) == ref_out
    assert 0 < ref_out["active"] < NPIX and plain.noise()["nonfinite"] == 0
    multi.gather_estimate()
    assert same_bits(multi.image_variance(), variance_of_sem(plain.standard_error()))
    _assert_gathered(multi, _state(plain), "estimate")
    dn = plain.denoise(variance=True)
    got = multi.image_resolve(temporal=0, variance=True)
    assert same_bits(got[0], dn[0]) and same_bits(got[1], dn[1])
    assert np.array_equal(multi.image_present(temporal=0, denoise=0), plain.Pixels())
    # the blend's length is each pixel's own count
    c, v, ln = multi.image_resolve(temporal=1, denoise=0, variance=True, length=True)
    assert np.array_equal(ln, plain.sample_counts().astype(F32)) and len(np.unique(ln)) >= 3
    # the camera moves: the history is pushed under the old camera, every pixel is active again
    plain.move_camera(_moved(cam))
    multi.image_move_camera(_moved(cam))
    assert multi.FrameIdx() == 0
    ref_out = plain.render_adaptive(THR, 32, check_every=STEP)
    assert multi.image_render_adaptive(THR, 32, check_every=STEP) == ref_out and 0 < ref_out["active"] < NPIX
    assert np.array_equal(multi.image_present(), plain.present())
    assert not np.array_equal(multi.image_present(), multi.image_present(temporal=0)), "a history is held"
    multi.close()
    plain.close()


# ---- 5. a joined tracer (one rank) ----------------------------------------------------------------------------------
def test_joined_world_1(have_gpu):
    import raytrace2_amd as R
    ref = _plain()
    sc, tr = _tracer(moments=False)
    tr.join(R.comm_unique_id(), 1, 0, 16)  # bands of 16 rows at height 24: the stacks carry padding rows
    tr.enable_moments()
    tr.image_enable_adaptive()
    out = tr.image_render_adaptive(THR, MAXF, check_every=STEP)
    assert out == ref["out"] and tr.image_part_adaptive(0) == out
    tr.gather_estimate()
    _assert_gathered(tr, ref, "joined")
    assert same_bits(tr.image_variance(), variance_of_sem(ref["sem"]))
    assert same_bits(tr.Accumulation(), ref["acc"]) and same_bits(tr.NonConvertedPixels(), ref["nc"])
    assert np.array_equal(tr.image_present(temporal=0, denoise=0), ref["px"])
    # the section above keeps its refusals on a joined tracer
    refused(tr.sample_counts)
    refused(lambda: tr.adaptive_check(THR))
    refused(lambda: tr.render_adaptive(THR, MAXF))
    tr.close()


# ---- 6. everything retired ------------------------------------------------------------------------------------------
def test_everything_retired(have_gpu):
    sc1, plain = _tracer(moments=False)
    plain.Render(STEP)
    nc16 = plain.NonConvertedPixels()
    plain.close()
    sc, tr = _multi(NAME, 3, 2)
    out = tr.image_render_adaptive(1e9, MAXF, check_every=STEP)  # a threshold no pixel exceeds
    assert tr.FrameIdx() == STEP and (out["active"], out["retired"], out["samples"]) == (0, NPIX, NPIX * STEP)
    launches = tr.stats()["launches"]
    tr.Render(16)  # nothing to trace: the frame index advances
    assert tr.FrameIdx() == 2 * STEP and tr.stats()["launches"] == launches
    tr.gather()  # a new gather, at frame index 32: the means are still sums / 16
    assert same_bits(tr.image_non_converted_pixels(), nc16) and (tr.image_sample_counts() == STEP).all()
    assert same_bits(tr.NonConvertedPixels(), nc16)
    tr.close()


# ---- 7. reset ---------------------------------------------------------------------------------------------------------
def test_reset_reactivates_and_reproduces(have_gpu):
    ref = _plain()
    sc, tr = _multi(NAME, 3, 2)
    first = tr.image_render_adaptive(THR, MAXF, check_every=STEP)
    tr.gather()
    _assert_gathered(tr, ref, "first run")
    tr.Reset()
    assert tr.FrameIdx() == 0
    refused(tr.image_sample_counts)  # the reset dropped the gathered image
    tr.Render(2)
    assert tr.image_adaptive_check(0.0, 64)["pixels"] == NPIX
    tr.gather()
    assert (tr.image_sample_counts() == 2).all(), "every pixel of every part active again"
    tr.Reset()
    second = tr.image_render_adaptive(THR, MAXF, check_every=STEP)
    assert first == second == ref["out"]
    tr.gather()
    _assert_gathered(tr, ref, "second run")
    assert same_bits(tr.moments(), ref["mom"])
    tr.close()


# ---- 8. switching it off ---------------------------------------------------------------------------------------------
def test_switching_it_off(have_gpu):
    acc = _plain13()
    sc, tr = _multi(NAME, 3, 2)
    tr.Render(3)
    tr.image_enable_adaptive(False)
    assert tr.FrameIdx() == 0
    tr.Render(13)
    tr.gather()
    assert same_bits(tr.image_accumulation(), acc)
    assert same_bits(tr.image_non_converted_pixels(), acc / F32(13)) and same_bits(tr.NonConvertedPixels(), acc / F32(13))
    refused(tr.image_sample_counts)
    refused(lambda: tr.image_adaptive_check(THR))
    tr.close()


# ---- 9. refusals -------------------------------------------------------------------------------------------------------
def test_refusals(have_gpu):
    import ctypes
    import raytrace2_amd as R
    from raytrace2_amd._native import Adaptive
    lib = R.lib
    sc, tr = _tracer(moments=False, devices=[0, 0, 0], band_h=2)
    refused(tr.image_enable_adaptive)  # moments off
    tr.enable_moments()
    tr.Render(2)
    for call in (lambda: tr.image_adaptive_check(THR), lambda: tr.image_render_adaptive(THR, 16), tr.image_sample_counts,
                 lambda: tr.image_part_adaptive(0)):
        refused(call)  # not switched on
    assert tr.FrameIdx() == 2
    tr.image_enable_adaptive()
    refused(tr.image_sample_counts)  # before a gather
    tr.Render(1)
    refused(lambda: tr.image_adaptive_check(THR))  # one frame
    assert tr.FrameIdx() == 1
    tr.Render(1)
    for window in (-1, 65):
        refused(lambda: tr.image_adaptive_check(THR, window))
        refused(lambda: tr.image_render_adaptive(THR, 16, window=window))
    for thr in (-1.0, float("nan")):
        refused(lambda: tr.image_adaptive_check(thr))
        refused(lambda: tr.image_render_adaptive(thr, 16))
    a = Adaptive()
    assert lib.rt2_tracer_image_adaptive_check(tr._h, THR, 1, None) == -1
    assert lib.rt2_tracer_image_render_adaptive(tr._h, THR, 1, 0, 16, 0, None) == -1
    assert lib.rt2_tracer_image_part_adaptive(tr._h, 0, None) == -1
    assert lib.rt2_tracer_image_sample_counts(tr._h, None) == -1
    assert lib.rt2_tracer_image_adaptive_check(None, THR, 1, ctypes.byref(a)) == -1
    # nothing has changed: two frames so far, every pixel active; eleven more give the plain tracer's sums
    assert tr.FrameIdx() == 2
    tr.Render(11)
    tr.gather()
    assert same_bits(tr.image_accumulation(), _plain13()) and (tr.image_sample_counts() == 13).all()
    tr.close()
    # a partition that is not joined has no communicator to gather over
    sc, tr = _tracer()
    tr.set_partition(2, 1, 3)
    refused(tr.image_enable_adaptive)
    refused(lambda: tr.image_adaptive_check(THR))
    tr.Render(13)
    assert same_bits(tr.Accumulation(), _plain13()[R.local_rows(H, 2, 1, 3)])
    tr.close()


# ---- 10. the refusals other files pin, restated ----------------------------------------------------------------------
def test_the_old_calls_keep_their_refusals(have_gpu):
    sc, multi = _tracer(devices=[0, 0], band_h=2)
    refused(multi.enable_adaptive)
    multi.image_enable_adaptive()
    refused(multi.enable_adaptive)
    refused(multi.sample_counts)
    refused(lambda: multi.adaptive_check(THR))
    refused(lambda: multi.render_adaptive(THR, 16))
    multi.close()
    sc, tr = _tracer()
    tr.enable_adaptive()  # the old call: no counts in the gather
    tr.Render(4)
    refused(tr.gather_estimate)
    refused(tr.image_resolve)
    refused(tr.image_present)
    refused(lambda: tr.image_move_camera(tr.get_camera()))
    refused(lambda: tr.image_adaptive_check(THR))
    assert tr.FrameIdx() == 4 and (tr.sample_counts() == 4).all()
    # the new call on the same plain tracer: its gathers carry the counts, and the old family still works
    tr.image_enable_adaptive()
    ref = _plain()
    assert tr.image_render_adaptive(THR, MAXF, check_every=STEP) == ref["out"]
    tr.gather_estimate()
    _assert_gathered(tr, ref, "plain")
    assert np.array_equal(tr.sample_counts(), ref["n"])
    # and the old call again takes the counts out of the gather
    tr.enable_adaptive()
    tr.Render(4)
    refused(tr.gather_estimate)
    tr.close()


# ---- 11. rt2_headless --gpus N --adaptive ------------------------------------------------------------------------------
def test_headless_adaptive_on_the_gathered_image(have_gpu, tmp_path):
    outs, lines = {}, {}
    for key, extra in (("multi", ["--gpus", "1"]), ("one", [])):
        png = str(tmp_path / f"{key}.png")
        r = subprocess.run([APP, scene_path(NAME), png, "--size", f"{W}x{H}", *extra, "--adaptive", repr(THR), "--window", "1",
                            "--max-samples", str(2 * SPP)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        m = re.search(r"^frames (\d+) active (\d+) samples (\d+)$", r.stderr, re.M)
        assert m, r.stderr
        outs[key], lines[key] = open(png, "rb").read(), m.group(0)
    assert lines["multi"] == lines["one"]
    assert 0 < int(lines["one"].split()[3]) < NPIX
    assert outs["multi"] == outs["one"]
