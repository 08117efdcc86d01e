"""Reconstructing the gathered image on the GPU (include/rt2.h "Reconstructing the gathered image"): what a
create_multi or joined tracer gathers on rank 0 gets the variance of the mean, the feature records, the filter, the
temporal blend and the RGBA8 present of a one-GPU tracer, bit for bit. The reference in every test is a plain
one-GPU tracer at the same seed, size, camera and frame count (existing entry points, not the ones under test).
Cornell at 70x37 (ragged against the 32x8 tile and the row bands), spp 16, 16 frames, seed 0x5EED2024; the gather's
kernel also at 50x45 and 33x10 over the band layouts of the host test."""
import ctypes
import dataclasses
import functools
import os
import subprocess

import numpy as np
import pytest

from bits import refused, same_bits
from conftest import ROOT, scene_path
from denoise_ref import variance_of_sem
from helpers import SEED

pytestmark = pytest.mark.gpu
W, H, SPP, FRAMES = 70, 37, 16, 16
NAME = "cornell_box_original"
F32 = np.float32
APP = os.path.join(ROOT, "raytrace2_amd", "lib", "rt2_headless")
DN3 = dict(iterations=3, sigma_l=2.0)  # a filter off its defaults


def _all_same(got, ref):
    return len(got) == len(ref) and all(same_bits(g, r) for g, r in zip(got, ref))


def _tracer(name=NAME, size=(W, H), *, moments=True, **kw):
    import raytrace2_amd as R
    sc = R.Scene(scene_path(name), SEED)
    tr = R.RayTracer(sc, 0, **kw)
    tr.set_seed(SEED)
    tr.SetSamplesPerPixel(SPP)
    tr.OnResize(size)
    if moments:
        tr.enable_moments()
    return sc, tr


def _moved(cam, step):
    """The camera `step` moves on: the centre shifts sideways and up by a fraction of the viewing distance."""
    d = float(np.linalg.norm(np.subtract(cam.center, cam.look_at)))
    return dataclasses.replace(cam, center=(cam.center[0] + 0.15 * d * step, cam.center[1] + 0.07 * d * step, cam.center[2]))


@functools.lru_cache(maxsize=None)
def _plain(size=(W, H)):
    """The one-GPU reference after FRAMES frames of Cornell at `size`: sums, means, pixels, the variance of the
    mean from standard_error(), and (at the tests' main size) the filter at its defaults and off them."""
    sc, tr = _tracer(size=size)
    tr.Render(FRAMES)
    assert tr.noise()["nonfinite"] == 0  # every comparison is over defined values
    ref = dict(acc=tr.Accumulation(), nc=tr.NonConvertedPixels(), px=tr.Pixels(), var=variance_of_sem(tr.standard_error()))
    if size == (W, H):
        ref["dn"] = tr.denoise(variance=True)
        ref["dn3"] = tr.denoise(variance=True, **DN3)
        ref["present"] = {(t, d): tr.present(temporal=t, denoise=d) for t in (0, 1) for d in (0, 1)}
    tr.close()
    for v in ref.values():
        for a in (v if isinstance(v, tuple) else v.values() if isinstance(v, dict) else (v,)):
            a.setflags(write=False)
    return ref


def _renders(tr, frames, ref_rows=None):
    """The tracer still renders: `frames` frames from a reset give the plain tracer's sums."""
    sc, plain = _tracer(moments=False)
    plain.Render(frames)
    acc = plain.Accumulation()
    plain.close()
    tr.Reset()
    tr.Render(frames)
    assert same_bits(tr.Accumulation(), acc if ref_rows is None else acc[ref_rows])


# ---- 3. the gather's kernel: image, means, pixels and variance over the band layouts ------------------------------
@pytest.mark.parametrize("n,band_h,size", [(1, 16, (50, 45)), (2, 8, (50, 45)), (3, 5, (50, 45)), (4, 1, (50, 45)),
                                           (4, 8, (33, 10))])
def test_gather_estimate_matches_one_gpu(have_gpu, n, band_h, size):
    """devices=[0] is the RCCL path (a communicator of size 1), the others copy on the one GPU. 33x10 over 4 ranks
    in bands of 8: two ranks own no row, and the stacks carry padding rows."""
    ref = _plain(size)
    sc, tr = _tracer(size=size, devices=[0] * n, band_h=band_h)
    tr.Render(FRAMES)
    tr.gather_estimate()
    assert same_bits(tr.image_accumulation(), ref["acc"])
    assert same_bits(tr.image_non_converted_pixels(), ref["nc"])
    assert np.array_equal(tr.image_pixels(), ref["px"])
    var = tr.image_variance()
    assert var.shape == (size[1], size[0]) and same_bits(var, ref["var"])
    assert (var > 0).any()
    # a plain gather afterwards leaves the same image, and the estimate stays readable
    tr.gather()
    assert same_bits(tr.image_non_converted_pixels(), ref["nc"]) and same_bits(tr.image_variance(), ref["var"])
    tr.close()


def test_gather_estimate_on_a_plain_tracer(have_gpu):
    ref = _plain()
    sc, tr = _tracer()
    tr.Render(FRAMES)
    tr.gather_estimate()
    assert same_bits(tr.image_accumulation(), ref["acc"]) and same_bits(tr.image_variance(), ref["var"])
    assert np.array_equal(tr.image_pixels(), ref["px"])
    tr.close()


# ---- 4. features ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell_box_original", "cornell_box_volume", "final_render_book_1"])
def test_image_features_match_one_gpu(have_gpu, name):
    """Word for word, the volume scene's fixed medium stream included; needs no gather and no moments; a moved
    camera traces again."""
    (_, plain), (_, multi) = _tracer(name, moments=False), _tracer(name, moments=False, devices=[0, 0, 0], band_h=2)
    cam = plain.get_camera()
    for step in (0, 1):
        for t in (plain, multi):
            t.set_camera(_moved(cam, step))
        got, ref = multi.image_features(), plain.features()
        assert got.shape == (H, W, 16) and same_bits(got, ref), (name, step)
        assert (ref[..., 0] == 1).any()
        if step == 0:
            first = ref
            assert same_bits(multi.image_features(), ref)  # the cached records
    assert not same_bits(first, ref), "the move changes the records"
    plain.close()
    multi.close()


# ---- 5. the filter -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3])
def test_image_resolve_is_denoise(have_gpu, n):
    ref = _plain()
    sc, tr = _tracer(devices=[0] * n, band_h=2)
    tr.Render(FRAMES)
    # no gather_estimate before: all ranks are in this process, the call gathers
    assert _all_same(tr.image_resolve(temporal=0, denoise=1, variance=True), ref["dn"])
    assert _all_same(tr.image_resolve(temporal=0, denoise=1, variance=True, dp=DN3), ref["dn3"])
    assert not same_bits(ref["dn"][0], ref["dn3"][0])
    assert _all_same(tr.image_resolve(temporal=0, denoise=0, variance=True), (ref["nc"], ref["var"]))
    # length is left untouched with temporal off; with it on and no history the current estimate comes back
    c, v, ln = tr.image_resolve(temporal=0, denoise=0, variance=True, length=True)
    assert (ln == 0).all()
    c, v, ln = tr.image_resolve(temporal=1, denoise=0, variance=True, length=True)
    assert same_bits(c, ref["nc"]) and same_bits(v, ref["var"]) and (ln == FRAMES).all()
    assert _all_same(tr.image_resolve(variance=True), ref["dn"])  # the defaults: both on, no history held
    assert tr.FrameIdx() == FRAMES and same_bits(tr.Accumulation(), ref["acc"])
    tr.close()


# ---- 6. temporal ---------------------------------------------------------------------------------------------------
def test_image_move_camera_carries_the_history(have_gpu):
    (_, plain), (_, multi) = _tracer(), _tracer(devices=[0, 0], band_h=2)
    cam = plain.get_camera()
    for t in (plain, multi):
        t.set_camera(cam)
        t.Render(FRAMES)

    def same_after(frames, history):
        for t in (plain, multi):
            t.Render(frames)
        assert plain.noise()["nonfinite"] == 0
        ref = plain.temporal_resolve(denoise=True, variance=True, length=True)
        got = multi.image_resolve(temporal=1, denoise=1, variance=True, length=True)
        assert _all_same(got, ref)
        assert _all_same(multi.image_resolve(temporal=1, denoise=0, variance=True, length=True),
                         plain.temporal_resolve(variance=True, length=True))
        assert bool((got[2] > frames).any()) == history
        return got

    plain.move_camera(_moved(cam, 1))
    multi.image_move_camera(_moved(cam, 1))
    assert multi.FrameIdx() == 0
    same_after(8, True)
    # a second move: the history pushed is itself a blend with the first one
    plain.move_camera(_moved(cam, -0.6), max_history=64.0)
    multi.image_move_camera(_moved(cam, -0.6), max_history=64.0)
    got = same_after(8, True)
    assert (got[2] > 8 + 8).any(), "lengths past both renders since the first move: the first history is carried"
    # invalid temporal parameters: refused, nothing moves
    refused(lambda: multi.image_move_camera(cam, max_history=0.0))
    assert multi.FrameIdx() == 8
    # a resize drops the history
    multi.OnResize((W, H))
    multi.Render(8)
    blended = multi.image_resolve(temporal=1, denoise=1, variance=True, length=True)
    assert _all_same(blended[:2], multi.image_resolve(temporal=0, denoise=1, variance=True))
    assert (blended[2] == 8).all()
    plain.close()
    multi.close()
    # moments off, or one frame: set_camera + reset
    (_, plain), (_, multi) = _tracer(moments=False), _tracer(moments=False, devices=[0, 0], band_h=2)
    for t in (plain, multi):
        t.set_camera(cam)
        t.Render(4)
    multi.image_move_camera(_moved(cam, 1))
    plain.set_camera(_moved(cam, 1))
    plain.Reset()
    for t in (plain, multi):
        t.Render(3)
    assert multi.FrameIdx() == 3 and same_bits(multi.Accumulation(), plain.Accumulation())
    plain.close()
    multi.close()


# ---- 7. present ----------------------------------------------------------------------------------------------------
def _after_a_move(**kw):
    """A plain tracer and a gathered one with 13 frames' history from the scene's camera and 5 frames at a moved one."""
    (_, plain), (_, multi) = _tracer(), _tracer(**kw)
    cam = plain.get_camera()
    for t in (plain, multi):
        t.set_camera(cam)
        t.Render(13)
    plain.move_camera(_moved(cam, 1))
    multi.image_move_camera(_moved(cam, 1))
    for t in (plain, multi):
        t.Render(5)
    assert plain.noise()["nonfinite"] == 0
    return plain, multi, cam


def test_image_present_is_present(have_gpu):
    from raytrace2_amd.progressive import PinnedBuffer
    plain, multi, cam = _after_a_move(devices=[0, 0, 0], band_h=2)
    assert multi.image_present_time() == -1
    shown = {}
    for temporal in (0, 1):
        for denoise in (0, 1):
            got = multi.image_present(temporal=temporal, denoise=denoise)
            assert got.shape == (H, W, 4) and got.dtype == np.uint8
            assert np.array_equal(got, plain.present(temporal=temporal, denoise=denoise)), (temporal, denoise)
            shown[temporal, denoise] = got
    assert len({a.tobytes() for a in shown.values()}) == 4, "each stage changes the picture"
    assert np.array_equal(shown[0, 0], multi.image_pixels())
    assert np.array_equal(multi.image_present(), shown[1, 1])  # the defaults: both on
    # the timer: read by polling once the present has finished
    multi.synchronize()
    ms = multi.image_present_time()
    assert np.isfinite(ms) and ms >= 0
    assert multi.image_present_time() == ms
    # two presents in flight into two buffers, one synchronize
    a, b = PinnedBuffer((H, W, 4)), PinnedBuffer((H, W, 4))
    multi.image_present_async(a.array)
    multi.image_present_async(b.array, denoise=0, tp=dict(max_history=8.0))
    multi.synchronize()
    assert np.array_equal(a.array, shown[1, 1])
    assert np.array_equal(b.array, plain.present(denoise=0, tp=dict(max_history=8.0)))
    assert not np.array_equal(a.array, b.array)
    with pytest.raises(ValueError):
        multi.image_present_async(np.zeros((H, W, 3), np.uint8))
    # neither call blocks the host: host_waits stands still across them (stats() does not count its own wait),
    # also when the call has to gather first
    a.array[:] = 0
    w0 = multi.stats()["host_waits"]
    multi.image_present_async(a.array)
    assert multi.stats()["host_waits"] == w0
    assert np.array_equal(a.array, shown[1, 1])
    multi.Render(2)
    plain.Render(2)
    w0 = multi.stats()["host_waits"]
    multi.image_present_async(a.array)  # queued frames, a stale estimate: flushes and gathers, still no wait
    multi.image_move_camera(cam)
    assert multi.stats()["host_waits"] == w0
    assert np.array_equal(a.array, plain.present())
    assert multi.FrameIdx() == 0
    # the history just pushed is the plain tracer's
    plain.move_camera(cam)
    for t in (plain, multi):
        t.Render(3)
    assert np.array_equal(multi.image_present(), plain.present())
    a.close()
    b.close()
    plain.close()
    multi.close()


# ---- 8. a joined tracer (one rank) ---------------------------------------------------------------------------------
def test_joined_tracer_needs_its_gather_estimate(have_gpu):
    import raytrace2_amd as R
    ref = _plain()
    sc, tr = _tracer(moments=False)
    tr.join(R.comm_unique_id(), 1, 0, 16)  # bands of 16 rows at height 37: the stacks carry padding rows
    tr.enable_moments()
    tr.Render(FRAMES)
    refused(tr.image_resolve)  # no estimate yet
    refused(tr.image_present)
    refused(tr.image_variance)
    tr.gather_estimate()
    assert same_bits(tr.image_variance(), ref["var"])
    assert _all_same(tr.image_resolve(temporal=0, denoise=1, variance=True), ref["dn"])
    assert _all_same(tr.image_resolve(variance=True), ref["dn"])
    for key, px in ref["present"].items():
        assert np.array_equal(tr.image_present(temporal=key[0], denoise=key[1]), px), key
    tr.Render(4)
    refused(tr.image_resolve)  # stale: frames since the gather
    refused(tr.image_present)
    assert tr.FrameIdx() == FRAMES + 4
    tr.gather_estimate()
    assert tr.image_resolve().shape == (H, W, 3)
    # image_move_camera is collective: this rank gathers when it is behind
    cam = tr.get_camera()
    sc2, plain = _tracer()
    plain.set_camera(cam)
    plain.Render(FRAMES + 4)
    for t, move in ((tr, tr.image_move_camera), (plain, plain.move_camera)):
        t.Render(2)
        move(_moved(cam, 1))
        t.Render(5)
    tr.gather_estimate()
    assert _all_same(tr.image_resolve(temporal=1, denoise=1, variance=True, length=True),
                     plain.temporal_resolve(denoise=True, variance=True, length=True))
    plain.close()
    tr.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------
def test_refusals(have_gpu):
    import raytrace2_amd as R
    from raytrace2_amd import local_rows
    from raytrace2_amd.progressive import PinnedBuffer
    buf = PinnedBuffer((H, W, 4))
    u8 = ctypes.POINTER(ctypes.c_uint8)

    def estimate_refused(tr):
        refused(tr.gather_estimate)
        refused(tr.image_resolve)
        refused(tr.image_present)
        refused(lambda: tr.image_present_async(buf.array))

    # moments off
    sc, multi = _tracer(moments=False, devices=[0, 0], band_h=2)
    cam = multi.get_camera()
    multi.Render(4)
    estimate_refused(multi)
    refused(multi.image_variance)
    assert multi.image_features().shape == (H, W, 16)  # needs neither moments nor a gather
    _renders(multi, 3)
    # fewer than 2 frames
    multi.enable_moments()
    estimate_refused(multi)
    multi.Render(1)
    estimate_refused(multi)
    assert multi.FrameIdx() == 1
    # NULL outputs; invalid parameters of a stage that is on; the same values with the stage off are accepted
    multi.Render(3)
    acc = multi.Accumulation()
    lib = R.lib
    assert lib.rt2_tracer_image_variance(multi._h, None) == -1
    assert lib.rt2_tracer_image_features(multi._h, None) == -1
    assert lib.rt2_tracer_image_resolve(multi._h, None, None, None, None) == -1
    assert lib.rt2_tracer_image_present(multi._h, None, None) == -1
    assert lib.rt2_tracer_image_present_async(multi._h, None, None) == -1
    assert lib.rt2_tracer_image_move_camera(multi._h, None, None) == -1
    for kw in (dict(dp=dict(iterations=0)), dict(dp=dict(sigma_l=0.0)), dict(tp=dict(max_history=0.0)),
               dict(tp=dict(min_normal_dot=float("nan")))):
        refused(lambda: multi.image_resolve(**kw))
        refused(lambda: multi.image_present(**kw))
        refused(lambda: multi.image_present_async(buf.array, **kw))
    refused(lambda: multi.image_move_camera(cam, sigma_p=-1.0))
    assert multi.FrameIdx() == 4 and same_bits(multi.Accumulation(), acc)
    assert np.array_equal(multi.image_present(denoise=0, dp=dict(iterations=0)), multi.image_present(denoise=0))
    assert same_bits(multi.image_resolve(temporal=0, tp=dict(max_history=0.0)), multi.image_resolve(temporal=0))
    with pytest.raises(TypeError):
        multi.image_resolve(iterations=3)
    # the existing calls keep their refusals on the same tracer
    refused(multi.denoise)
    refused(multi.features)
    refused(multi.temporal_resolve)
    refused(multi.temporal_push)
    refused(multi.present)
    refused(multi.present_time)
    refused(lambda: multi.move_camera(cam))
    refused(multi.enable_adaptive)
    _renders(multi, 3)
    multi.close()
    # a joined tracer keeps them too
    sc, tr = _tracer(moments=False)
    tr.join(R.comm_unique_id(), 1, 0, 16)
    tr.enable_moments()
    tr.Render(4)
    refused(tr.denoise)
    refused(tr.present)
    refused(lambda: tr.move_camera(cam))
    refused(tr.enable_adaptive)
    _renders(tr, 3)
    tr.close()
    # a plain tracer with adaptive sampling on
    sc, tr = _tracer()
    tr.enable_adaptive()
    tr.Render(4)
    estimate_refused(tr)
    refused(lambda: tr.image_move_camera(cam))
    assert tr.FrameIdx() == 4
    assert tr.present().shape == (H, W, 4)  # its own chain works as before
    tr.enable_adaptive(False)
    _renders(tr, 3)
    # a partition that is not joined: as gather refuses it; rank 1 holds no image either
    tr.set_partition(2, 1, 3)
    tr.Render(4)
    refused(tr.gather)
    estimate_refused(tr)
    refused(tr.image_features)
    refused(tr.image_present_time)
    refused(lambda: tr.image_move_camera(cam))
    assert lib.rt2_tracer_image_present_async(tr._h, None, buf.array.ctypes.data_as(u8)) == -1
    assert tr.FrameIdx() == 4
    _renders(tr, 3, local_rows(H, 2, 1, 3))
    tr.set_partition(2, 0, 3)  # rank 0 of an unjoined partition: still no communicator to gather over
    tr.Render(4)
    estimate_refused(tr)
    _renders(tr, 3, local_rows(H, 2, 0, 3))
    tr.close()
    buf.close()


# ---- 10. rt2_headless --gpus N --denoise ----------------------------------------------------------------------------
def test_headless_denoises_the_gathered_image(have_gpu, tmp_path):
    outs = {}
    for key, extra in (("multi", ["--gpus", "1", "--denoise"]), ("one", ["--denoise"]), ("plain", ["--gpus", "1"])):
        out = str(tmp_path / f"{key}.png")
        r = subprocess.run([APP, scene_path(NAME), out, "--samples", "16", "--size", "80x72", *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[key] = open(out, "rb").read()
    assert outs["multi"] == outs["one"]
    assert outs["multi"] != outs["plain"]
