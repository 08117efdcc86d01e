"""Temporal reuse on the GPU (include/rt2.h "Temporal reuse"): temporal_buffers against the numpy float32 statement
(tests/temporal_ref.py) bit for bit, and the tracer's push / move / resolve chain against the same statement applied
to the GPU's own readbacks, with the filter, under adaptive sampling, the history's lifetime and the refusals.
Images are 70x37 (ragged against the 32x8 tile, more than one workgroup each way), spp 16, seed 0x5EED2024."""
import ctypes

import numpy as np
import pytest

from bits import refused, same_bits
from conftest import scene_path
from denoise_ref import denoise_ref, variance_of_sem
from helpers import SEED
from temporal_ref import case_args, synthetic_case, temporal_ref

pytestmark = pytest.mark.gpu
W, H, SPP = 70, 37, 16
F32 = np.float32
SCENES = ["cornell_box_original", "final_render_book_1", "cornell_box_volume"]
OTHER = dict(max_history=48.0, max_history_specular=6.0, min_normal_dot=0.5, sigma_p=0.25, sigma_a=2.0)


def _same3(got, ref):
    return all(same_bits(g, r) for g, r in zip(got, ref))


# ---- temporal_buffers against the numpy statement --------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (1, 9), (9, 1), (33, 9), (70, 37)])
def test_temporal_buffers_match_numpy_bit_for_bit(have_gpu, size):
    import raytrace2_amd as R
    w, h = size
    case = synthetic_case(w, h)
    args = case_args(case)
    for mats in (case["materials"], None):
        for kw in ({}, OTHER):
            ref = temporal_ref(*args, materials=mats, **kw)
            got = R.temporal_buffers(*args, materials=mats, **kw)
            for g, r, what in zip(got, ref, ("colour", "variance", "length")):
                assert same_bits(g, r), (size, mats is None, kw, what)
    again = R.temporal_buffers(*args, materials=mats, **kw)
    assert _same3(again, got)  # the same call twice: the same bytes


# ---- the tracer ------------------------------------------------------------------------------------------------
def _tracer(name, *, moments=True, **kw):
    import raytrace2_amd as R
    sc = R.Scene(scene_path(name), SEED)
    tr = R.RayTracer(sc, 0, **kw)
    tr.set_seed(SEED)
    tr.SetSamplesPerPixel(SPP)
    tr.OnResize((W, H))
    if moments:
        tr.enable_moments()
    return sc, tr


def _moved(cam, step):
    """The camera `step` moves on: the centre shifts sideways and up by a fraction of the viewing distance."""
    import dataclasses
    d = float(np.linalg.norm(np.subtract(cam.center, cam.look_at)))
    return dataclasses.replace(cam, center=(cam.center[0] + 0.15 * d * step, cam.center[1] + 0.07 * d * step, cam.center[2]))


def _words(sc, cam):
    sc.cam = cam
    return sc.camera_params(W, H, SPP)


def _current(tr, adaptive=False):
    """The GPU's own readbacks: colour, variance of the mean, length, features."""
    c = tr.NonConvertedPixels()
    v = variance_of_sem(tr.standard_error())
    n = tr.sample_counts().astype(F32) if adaptive else np.full((H, W), tr.FrameIdx(), F32)
    return c, v, n, tr.features()


def _no_history(cur):
    c, v, n, f = cur
    fin = np.isfinite(c).all(-1) & np.isfinite(v)
    return c, v, np.where(fin, n, F32(0)).astype(F32), f


def _untouched(tr, state):
    return same_bits(tr.Accumulation(), state[0]) and same_bits(tr.moments(), state[1]) and tr.FrameIdx() == state[2]


@pytest.mark.parametrize("name", SCENES)
def test_tracer_chain_matches_numpy_on_its_own_readbacks(have_gpu, name):
    """16 frames at A, push, move, reset, 4 frames at B, resolve; push, move, reset, 4 frames at C, resolve with a
    cap the history reaches and a positive specular cap. Every result is the numpy statement applied to the
    tracer's own readbacks, bit for bit; resolve and push change nothing the tracer renders from."""
    sc, tr = _tracer(name)
    mats = sc.materials()
    camA = tr.get_camera()
    tr.set_camera(camA)
    tr.Render(16)
    curA = _current(tr)
    state = (tr.Accumulation(), tr.moments(), tr.FrameIdx())
    assert tr.temporal_time() == -1
    first = tr.temporal_resolve(variance=True, length=True)  # no history yet: the current estimate
    assert _same3(first, _no_history(curA)[:3]) and (first[2] == 16).any()
    tr.temporal_push()
    assert _untouched(tr, state)
    hist = _no_history(curA) + (_words(sc, camA),)
    # B
    camB = _moved(camA, 1)
    tr.set_camera(camB)
    tr.Reset()
    tr.Render(4)
    curB = _current(tr)
    state = (tr.Accumulation(), tr.moments(), tr.FrameIdx())
    trace = {}
    refB = temporal_ref(*curB, *hist, materials=mats, trace=trace)
    assert trace["has"].mean() > 0.2 and (refB[2] == 20).any(), "the move leaves history to find"
    gotB = tr.temporal_resolve(variance=True, length=True)
    for g, r, what in zip(gotB, refB, ("colour", "variance", "length")):
        assert same_bits(g, r), (name, "B", what)
    assert tr.temporal_time() > 0
    assert _same3(tr.temporal_resolve(variance=True, length=True), gotB)  # twice: the same bytes
    assert same_bits(tr.temporal_resolve(), gotB[0])
    assert _untouched(tr, state)
    if name == "final_render_book_1":
        types = mats[curB[3][..., 9].astype(int), 0][curB[3][..., 0] != 0]
        assert (types == 0).any() and (types == 2).any(), "metal and dielectric first hits"
        assert trace["cap_zero"].any() and not trace["has"][trace["specular"]].any()
    # the second push chains: the history is now the blend at B, taken with B's features and camera
    kw = dict(max_history=18.0, max_history_specular=6.0)
    tr.temporal_push(**kw)
    assert _untouched(tr, state)
    histB = temporal_ref(*curB, *hist, materials=mats, **kw) + (curB[3], _words(sc, camB))
    camC = _moved(camB, -0.6)
    tr.set_camera(camC)
    tr.Reset()
    tr.Render(4)
    curC = _current(tr)
    trace = {}
    refC = temporal_ref(*curC, *histB, materials=mats, trace=trace, **kw)
    assert trace["capped"].any() and (refC[2] == 22).any(), "the cap of 18 is reached"
    if name == "final_render_book_1":
        assert trace["has"][trace["specular"]].any(), "a positive specular cap lets metal and glass reuse"
    gotC = tr.temporal_resolve(variance=True, length=True, **kw)
    for g, r, what in zip(gotC, refC, ("colour", "variance", "length")):
        assert same_bits(g, r), (name, "C", what)
    # the tracer still renders what it rendered
    tr.Render(3)
    from oracle.oracle import OracleScene
    o = OracleScene(scene_path(name), SEED)
    o.set_camera(camC.center, camC.look_at, camC.view_up, camC.vfov, camC.defocus_angle, camC.focus_distance)
    acc, _, _ = o.render(W, H, SPP, 7, forward=True)
    assert same_bits(tr.Accumulation(), acc)
    tr.close()


def test_resolve_with_the_filter(have_gpu):
    """denoise=True: the existing filter over the blended colour and variance with the features at B; the length
    is the blend's. The history stays the unfiltered blend."""
    name = "cornell_box_original"
    sc, tr = _tracer(name)
    mats = sc.materials()
    camA = tr.get_camera()
    tr.set_camera(camA)
    tr.Render(16)
    hist = _no_history(_current(tr)) + (_words(sc, camA),)
    tr.temporal_push()
    tr.set_camera(_moved(camA, 1))
    tr.Reset()
    tr.Render(4)
    cur = _current(tr)
    bc, bv, bn = temporal_ref(*cur, *hist, materials=mats)
    for dn, kw in ((True, {}), (dict(iterations=2, sigma_l=3.0), dict(iterations=2, sigma_l=3.0))):
        rc, rv = denoise_ref(bc, bv, cur[3], **kw)
        gc, gv, gn = tr.temporal_resolve(denoise=dn, variance=True, length=True)
        assert same_bits(gc, rc) and same_bits(gv, rv) and same_bits(gn, bn), kw
    assert _same3(tr.temporal_resolve(variance=True, length=True), (bc, bv, bn))  # the filter left no trace
    tr.close()


def test_resolve_with_adaptive_sampling(have_gpu):
    """After render_adaptive the pixels' sample counts differ: n is each pixel's own n_p, in the history too."""
    name = "cornell_box_original"
    sc, tr = _tracer(name)
    tr.enable_adaptive()
    mats = sc.materials()
    camA = tr.get_camera()
    tr.set_camera(camA)
    tr.render_adaptive(float(F32(0.05)), 48, check_every=16)
    curA = _current(tr, adaptive=True)
    assert len(np.unique(curA[2])) > 1
    tr.temporal_push()
    hist = _no_history(curA) + (_words(sc, camA),)
    tr.set_camera(_moved(camA, 1))
    tr.Reset()
    tr.render_adaptive(float(F32(0.05)), 32, check_every=16)
    cur = _current(tr, adaptive=True)
    counts = tr.sample_counts()
    assert len(np.unique(cur[2])) > 1
    ref = temporal_ref(*cur, *hist, materials=mats)
    got = tr.temporal_resolve(variance=True, length=True)
    assert _same3(got, ref)
    assert np.array_equal(tr.sample_counts(), counts)
    tr.close()


def test_history_lifetime(have_gpu):
    name = "cornell_box_original"
    sc, tr = _tracer(name)
    cam = tr.get_camera()
    tr.set_camera(cam)

    def fresh():
        """Whether a resolve returns the current estimate with length == n."""
        tr.Render(4)
        c, v, n = tr.temporal_resolve(variance=True, length=True)
        fresh_c, fresh_n = same_bits(c, tr.NonConvertedPixels()), bool((n == tr.FrameIdx()).all())
        assert fresh_c == fresh_n
        return fresh_n

    assert fresh()
    tr.temporal_push()
    tr.Reset()
    assert not fresh(), "Reset keeps the history"
    _, _, n = tr.temporal_resolve(variance=True, length=True)
    assert (n == 8).any() and set(np.unique(n)) <= {4.0, 8.0}  # 4 frames of history, 4 current; the misses
    tr.temporal_clear()
    tr.Reset()
    assert fresh(), "temporal_clear drops it"
    tr.temporal_push()
    tr.OnResize((W + 3, H + 2))
    tr.enable_moments()
    tr.Render(4)
    c, n = tr.temporal_resolve(length=True)
    assert c.shape == (H + 2, W + 3, 3) and same_bits(c, tr.NonConvertedPixels()) and (n == 4).all(), "a resize drops it"
    tr.OnResize((W, H))
    tr.Reset()
    assert fresh()
    tr.temporal_push()
    tr.enable_moments(False)
    tr.enable_moments(True)
    assert fresh(), "enable_moments reallocates and drops it"
    tr.temporal_push()
    tr.set_partition(0, 0, 1)
    assert fresh(), "set_partition drops it"
    tr.close()


def test_history_counts_as_device_bytes(have_gpu):
    """At a size above the scene's own (where the tracer was created, its high-water mark until then) the first
    temporal call adds the packed history (64 bytes per pixel), the length plane (4) and the blend's colour and
    variance (16) to device_bytes_peak; a tracer that never calls it holds none of them."""
    sc, tr = _tracer("cornell_box_original")
    w = h = 672
    tr.OnResize((w, h))
    tr.enable_moments()
    tr.Render(2)
    tr.Render(2)  # both launch slots hold their sample buffers now
    tr.features()  # and the feature records are allocated
    before = tr.stats()["device_bytes_peak"]
    n = tr.temporal_resolve(length=True)[1]
    assert (n == 4).all()
    assert tr.stats()["device_bytes_peak"] == before + w * h * (64 + 4 + 16)
    tr.temporal_push()
    assert tr.stats()["device_bytes_peak"] == before + w * h * (64 + 4 + 16)
    tr.close()


# ---- refusals ---------------------------------------------------------------------------------------------------
def _renders(tr, frames, rows=None):
    """The tracer still renders: `frames` frames from a reset give the oracle's sums."""
    from oracle.oracle import OracleScene
    tr.Reset()
    tr.Render(frames)
    acc, _, _ = OracleScene(scene_path("cornell_box_original"), SEED).render(W, H, SPP, frames, forward=True)
    assert same_bits(tr.Accumulation(), acc if rows is None else acc[rows])


def test_refusals(have_gpu):
    import raytrace2_amd as R
    from raytrace2_amd import local_rows
    name = "cornell_box_original"
    # moments off
    sc, tr = _tracer(name, moments=False)
    tr.Render(4)
    refused(tr.temporal_resolve)
    refused(tr.temporal_push)
    _renders(tr, 3)
    # fewer than 2 frames
    tr.enable_moments()
    refused(tr.temporal_resolve)
    tr.Render(1)
    refused(tr.temporal_resolve)
    refused(tr.temporal_push)
    # each invalid parameter, a NULL output, invalid filter parameters
    tr.Render(3)
    for kw in (dict(max_history=0.0), dict(max_history=float("inf")), dict(max_history_specular=-1.0),
               dict(max_history_specular=float("nan")), dict(min_normal_dot=float("nan")), dict(sigma_p=0.0),
               dict(sigma_p=float("inf")), dict(sigma_a=-1.0), dict(sigma_a=float("nan"))):
        refused(lambda: tr.temporal_resolve(**kw))
        refused(lambda: tr.temporal_push(**kw))
    refused(lambda: tr.temporal_resolve(denoise=dict(iterations=0)))
    assert R.lib.rt2_tracer_temporal_resolve(tr._h, None, 0, None, None, None, None) == -1
    buf = (ctypes.c_float * 32)()
    assert R.lib.rt2_temporal_buffers(0, 1, 1, *([buf] * 9), None, 0, None, None, None, None) == -1
    assert tr.temporal_resolve().shape == (H, W, 3)
    _renders(tr, 3)
    # a partitioned tracer
    tr.set_partition(2, 1, 3)
    tr.Render(4)
    refused(tr.temporal_resolve)
    refused(tr.temporal_push)
    refused(tr.temporal_clear)
    _renders(tr, 3, local_rows(H, 2, 1, 3))
    tr.close()
    # a multi tracer over one GPU twice
    sc, multi = _tracer(name, devices=[0, 0], band_h=2)
    multi.Render(4)
    refused(multi.temporal_resolve)
    refused(multi.temporal_push)
    refused(multi.temporal_clear)
    refused(multi.temporal_time)
    _renders(multi, 3)
    multi.close()
    # a joined world-1 tracer
    sc, tr = _tracer(name, moments=False)
    tr.join(R.comm_unique_id(), 1, 0, 16)
    tr.enable_moments()
    tr.Render(4)
    refused(tr.temporal_resolve)
    refused(tr.temporal_push)
    refused(tr.temporal_clear)
    _renders(tr, 3)
    tr.close()
