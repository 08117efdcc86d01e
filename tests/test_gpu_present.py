"""Presenting reconstructed frames on the GPU (include/rt2.h "Presenting reconstructed frames"): present() against
the numpy tone map (tests/present_ref.py) of the blocking readbacks it chains, byte for byte; present_async and
move_camera without a host wait; present_buffers, present_time, the refusals and ProgressiveLoop(reconstruct=...).
Cornell at 70x37 (ragged against the 32x8 tile, wider than step 16's reach), spp 16, seed 0x5EED2024, 13 frames
before the camera move and 5 after."""
import ctypes
import dataclasses

import numpy as np
import pytest

from bits import refused, same_bits
from conftest import scene_path
from helpers import SEED
from present_ref import EDGE_BYTES, edge_cases, edge_image, present

pytestmark = pytest.mark.gpu
W, H, SPP = 70, 37, 16
BEFORE, AFTER = 13, 5
NAME = "cornell_box_original"
F32 = np.float32
# adaptive sampling's threshold in the tests: loose enough that a check after a few frames retires pixels
ADAPTIVE_THRESHOLD = 0.5


def _tracer(*, moments=True, adaptive=False, **kw):
    import raytrace2_amd as R
    sc = R.Scene(scene_path(NAME), SEED)
    tr = R.RayTracer(sc, 0, **kw)
    tr.set_seed(SEED)
    tr.SetSamplesPerPixel(SPP)
    tr.OnResize((W, H))
    if moments:
        tr.enable_moments()
    if adaptive:
        tr.enable_adaptive()
    return sc, tr


def _moved(cam, step):
    """The camera `step` moves on: the centre shifts sideways and up by a fraction of the viewing distance."""
    d = float(np.linalg.norm(np.subtract(cam.center, cam.look_at)))
    return dataclasses.replace(cam, center=(cam.center[0] + 0.15 * d * step, cam.center[1] + 0.07 * d * step, cam.center[2]))


def _same_camera(a, b):
    """Equal as the tracer holds them (float32)."""
    return all(np.array_equal(F32(x), F32(y)) for x, y in zip(dataclasses.astuple(a), dataclasses.astuple(b)))


def _after_a_move(adaptive=False):
    """A tracer with 13 frames' history pushed from the scene's camera and 5 frames at a moved one. Adaptive: a
    check retires pixels before the move, and again after 3 of the 5 frames, so the counts n_p differ."""
    sc, tr = _tracer(adaptive=adaptive)
    cam = tr.get_camera()
    tr.set_camera(cam)
    tr.Render(BEFORE)
    if adaptive:
        assert tr.adaptive_check(ADAPTIVE_THRESHOLD)["retired"] > 0
    tr.temporal_push()
    tr.set_camera(_moved(cam, 1))
    tr.Reset()
    if adaptive:
        tr.Render(3)
        assert tr.adaptive_check(ADAPTIVE_THRESHOLD)["retired"] > 0
        tr.Render(AFTER - 3)
        assert len(np.unique(tr.sample_counts())) > 1
    else:
        tr.Render(AFTER)
    assert tr.FrameIdx() == AFTER
    assert tr.noise()["nonfinite"] == 0  # every comparison below is over defined bytes
    return sc, tr


def _waits_across(tr, fn=None):
    """host_waits added between two stats() calls around fn() and a synchronize(). stats() reports the count from
    before its own synchronisation, so the figure holds the first stats' and the synchronize's own waits: compare
    it with the figure of a control (fn None, or the documented no-wait launch path), never with 0."""
    w0 = tr.stats()["host_waits"]
    if fn is not None:
        fn()
    tr.synchronize()
    return tr.stats()["host_waits"] - w0


def _state(tr):
    return tr.Accumulation(), tr.moments(), tr.FrameIdx()


def _untouched(tr, state):
    return same_bits(tr.Accumulation(), state[0]) and same_bits(tr.moments(), state[1]) and tr.FrameIdx() == state[2]


def _blocking(tr, temporal, denoise):
    """What present(temporal, denoise) must show, from the blocking readbacks."""
    if temporal:
        return present(tr.temporal_resolve(denoise=bool(denoise)))
    if denoise:
        return present(tr.denoise())
    return tr.Pixels()


# ---- 1. present() against the blocking readbacks ---------------------------------------------------------------
@pytest.mark.parametrize("adaptive", [False, True])
def test_present_is_the_tone_map_of_the_blocking_readbacks(have_gpu, adaptive):
    sc, tr = _after_a_move(adaptive)
    length = tr.temporal_resolve(length=True)[1]
    assert (length > AFTER).any(), "the move leaves history to blend with"
    state = _state(tr)
    shown = {}
    for temporal in (0, 1):
        for denoise in (0, 1):
            got = tr.present(temporal=temporal, denoise=denoise)
            assert got.shape == (H, W, 4) and got.dtype == np.uint8
            assert np.array_equal(got, _blocking(tr, temporal, denoise)), (adaptive, temporal, denoise)
            shown[temporal, denoise] = got
    # both stages off: also the numpy tone map of NonConvertedPixels (each pixel's own n_p under adaptive sampling)
    assert np.array_equal(shown[0, 0], present(tr.NonConvertedPixels()))
    assert np.array_equal(tr.present(), shown[1, 1])  # the defaults: both on
    assert len({a.tobytes() for a in shown.values()}) == 4, "each stage changes the picture"
    assert _untouched(tr, state)
    if adaptive:
        assert len(np.unique(tr.sample_counts())) > 1
    tr.close()


# ---- 2. present_async --------------------------------------------------------------------------------------------
def test_present_async_does_not_wait_and_changes_nothing(have_gpu):
    from raytrace2_amd.progressive import PinnedBuffer
    sc, tr = _after_a_move()
    buf = PinnedBuffer((H, W, 4))
    tr.present_async(buf.array)  # warm-up: the first call allocates
    tr.synchronize()
    state = _state(tr)
    buf.array[:] = 0
    control = _waits_across(tr)
    assert _waits_across(tr, lambda: tr.present_async(buf.array)) == control
    first = buf.array.copy()
    assert np.array_equal(first, tr.present())
    buf.array[:] = 0
    tr.present_async(buf.array)
    tr.synchronize()
    assert np.array_equal(buf.array, first)  # a second call: the same bytes
    assert _untouched(tr, state)
    with pytest.raises(ValueError):
        tr.present_async(np.zeros((H, W, 3), np.uint8))
    buf.close()
    tr.close()


# ---- 3. queued frames are included ---------------------------------------------------------------------------------
def test_present_async_launches_the_queued_frames(have_gpu):
    from raytrace2_amd.progressive import PinnedBuffer
    (_, tr), (_, twin) = _after_a_move(), _after_a_move()
    buf = PinnedBuffer((H, W, 4))
    for t in (tr, twin):  # warm-up
        t.present_async(buf.array)
        t.synchronize()

    def queued_then_present():
        tr.Render(3)  # under the default lazy queue: queued, not launched
        tr.present_async(buf.array)

    def queued_then_flush():  # the control: the launch path that is documented not to wait
        twin.Render(3)
        twin.flush()

    waits = _waits_across(tr, queued_then_present)
    assert waits == _waits_across(twin, queued_then_flush)
    assert tr.FrameIdx() == twin.FrameIdx() == AFTER + 3
    assert np.array_equal(buf.array, twin.present())
    assert same_bits(tr.Accumulation(), twin.Accumulation())
    buf.close()
    tr.close()
    twin.close()


# ---- 4. two presents in flight ---------------------------------------------------------------------------------------
def test_two_presents_back_to_back_into_two_buffers(have_gpu):
    from raytrace2_amd.progressive import PinnedBuffer
    sc, tr = _after_a_move()
    a, b = PinnedBuffer((H, W, 4)), PinnedBuffer((H, W, 4))
    tr.present_async(a.array)  # filter on
    tr.present_async(b.array, denoise=0)  # filter off: the same scratch, reused in stream order
    tr.synchronize()
    assert np.array_equal(a.array, tr.present())
    assert np.array_equal(b.array, tr.present(denoise=0))
    assert not np.array_equal(a.array, b.array)
    a.close()
    b.close()
    tr.close()


# ---- 5. move_camera ------------------------------------------------------------------------------------------------------
def test_move_camera_is_push_set_camera_reset_without_a_wait(have_gpu):
    (_, tr), (_, twin) = _tracer(), _tracer()
    cam = tr.get_camera()
    cam_b, cam_c = _moved(cam, 1), _moved(cam, -0.6)
    for t in (tr, twin):
        t.set_camera(cam)
        t.Render(BEFORE)
        t.synchronize()
    control = _waits_across(tr)
    assert _waits_across(tr, lambda: tr.move_camera(cam_b)) == control
    twin.temporal_push()
    twin.set_camera(cam_b)
    twin.Reset()
    assert tr.FrameIdx() == 0 and _same_camera(tr.get_camera(), cam_b)

    def same_after(frames, history):
        for t in (tr, twin):
            t.Render(frames)
        assert tr.noise()["nonfinite"] == 0
        for dn in (False, True):
            got = tr.temporal_resolve(denoise=dn, variance=True, length=True)
            ref = twin.temporal_resolve(denoise=dn, variance=True, length=True)
            assert all(same_bits(g, r) for g, r in zip(got, ref)), dn
        assert same_bits(tr.Accumulation(), twin.Accumulation()) and same_bits(tr.moments(), twin.moments())
        assert bool((got[2] > tr.FrameIdx()).any()) == history
        assert np.array_equal(tr.present(), twin.present())

    same_after(AFTER, True)
    # one frame rendered: set_camera + reset, and the history pushed at the first camera is kept
    for t in (tr, twin):
        t.Reset()
        t.Render(1)
    tr.move_camera(cam_c)
    twin.set_camera(cam_c)
    twin.Reset()
    same_after(4, True)
    # invalid temporal parameters: refused, nothing moves
    from raytrace2_amd import Rt2Error
    with pytest.raises(Rt2Error):
        tr.move_camera(cam, max_history=0.0)
    assert tr.FrameIdx() == 4 and _same_camera(tr.get_camera(), cam_c)
    # temporal_clear still drops the history
    tr.temporal_clear()
    twin.temporal_clear()
    same_after(1, False)
    tr.close()
    twin.close()
    # moments off: set_camera + reset
    (_, tr), (_, twin) = _tracer(moments=False), _tracer(moments=False)
    for t in (tr, twin):
        t.set_camera(cam)
        t.Render(4)
    tr.move_camera(cam_b)
    twin.set_camera(cam_b)
    twin.Reset()
    for t in (tr, twin):
        t.Render(3)
    assert tr.FrameIdx() == 3 and same_bits(tr.Accumulation(), twin.Accumulation())
    tr.close()
    twin.close()


# ---- 6. present_buffers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(33, 9), (70, 37)])
def test_present_buffers_match_numpy_byte_for_byte(have_gpu, size):
    import raytrace2_amd as R
    c = edge_image(*size)
    assert np.isnan(c).any() and np.isinf(c).any()
    assert np.array_equal(R.present_buffers(c), present(c))
    got = R.present_buffers(edge_cases())
    for k in range(3):
        assert np.array_equal(got[k, :, k], EDGE_BYTES), k


# ---- 7. present_time ----------------------------------------------------------------------------------------------------
def test_present_time_polls_and_never_waits(have_gpu):
    sc, tr = _after_a_move()
    assert tr.present_time() == -1
    tr.present()
    tr.synchronize()
    ms = tr.present_time()
    assert np.isfinite(ms) and ms > 0
    control = _waits_across(tr)
    assert _waits_across(tr, tr.present_time) == control
    assert tr.present_time() == ms  # read once, kept until the next present
    tr.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------
def _renders(tr, frames, rows=None):
    """The tracer still renders: `frames` frames from a reset give the oracle's sums."""
    from oracle.oracle import OracleScene
    tr.Reset()
    tr.Render(frames)
    acc, _, _ = OracleScene(scene_path(NAME), SEED).render(W, H, SPP, frames, forward=True)
    assert same_bits(tr.Accumulation(), acc if rows is None else acc[rows])


def test_refusals(have_gpu):
    import raytrace2_amd as R
    from raytrace2_amd import local_rows
    from raytrace2_amd.progressive import PinnedBuffer
    buf = PinnedBuffer((H, W, 4))

    def both_refused(tr):
        refused(tr.present)
        refused(lambda: tr.present_async(buf.array))

    # moments off
    sc, tr = _tracer(moments=False)
    cam = tr.get_camera()
    tr.Render(4)
    both_refused(tr)
    _renders(tr, 3)
    # one frame
    tr.enable_moments()
    both_refused(tr)
    tr.Render(1)
    both_refused(tr)
    assert tr.FrameIdx() == 1
    # a NULL output, invalid parameters of a stage that is on; the same values with the stage off are accepted
    tr.Render(3)
    state = _state(tr)
    assert R.lib.rt2_tracer_present(tr._h, None, None) == -1
    assert R.lib.rt2_tracer_present_async(tr._h, None, None) == -1
    assert R.lib.rt2_tracer_move_camera(tr._h, None, None) == -1
    refused(lambda: tr.present(dp=dict(iterations=0)))
    refused(lambda: tr.present_async(buf.array, dp=dict(iterations=0)))
    refused(lambda: tr.present(tp=dict(max_history=0.0)))
    assert _untouched(tr, state)
    assert np.array_equal(tr.present(denoise=0, dp=dict(iterations=0)), tr.present(denoise=0))
    assert np.array_equal(tr.present(temporal=0, tp=dict(max_history=0.0)), tr.present(temporal=0))
    with pytest.raises(TypeError):
        tr.present(iterations=3)
    _renders(tr, 3)
    # a partitioned tracer: move_camera is set_camera + reset there
    tr.set_partition(2, 1, 3)
    tr.Render(4)
    refused(tr.present)
    assert R.lib.rt2_tracer_present_async(tr._h, None, buf.array.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))) == -1
    refused(tr.present_time)
    tr.move_camera(_moved(cam, 1))
    assert tr.FrameIdx() == 0
    tr.move_camera(cam)
    _renders(tr, 3, local_rows(H, 2, 1, 3))
    tr.close()
    # a multi tracer over one GPU twice
    sc, multi = _tracer(devices=[0, 0], band_h=2)
    multi.Render(4)
    both_refused(multi)
    refused(multi.present_time)
    refused(lambda: multi.move_camera(cam))
    _renders(multi, 3)
    multi.close()
    # a joined world-1 tracer
    sc, tr = _tracer(moments=False)
    tr.join(R.comm_unique_id(), 1, 0, 16)
    tr.enable_moments()
    tr.Render(4)
    both_refused(tr)
    refused(tr.present_time)
    refused(lambda: tr.move_camera(cam))
    _renders(tr, 3)
    tr.close()
    buf.close()


# ---- 9. ProgressiveLoop ----------------------------------------------------------------------------------------------------
def test_progressive_loop_shows_the_reconstruction(have_gpu):
    from raytrace2_amd.progressive import ProgressiveLoop
    sc, tr = _tracer()
    cam = tr.get_camera()
    tr.set_camera(cam)
    loop = ProgressiveLoop(tr, 24, first_frames=1, reconstruct={})
    frames = []
    while not loop.done():
        px = loop.tick().copy()
        f = tr.FrameIdx()
        frames.append(f)
        assert tr.noise()["nonfinite"] == 0 if f >= 2 else True
        assert np.array_equal(px, tr.Pixels() if f < 2 else tr.present()), f
    assert frames[0] == 1 and frames[-1] == 24 and loop.tick() is None
    _, twin = _tracer()
    twin.set_camera(cam)
    twin.Render(24)
    assert same_bits(tr.Accumulation(), twin.Accumulation()) and same_bits(tr.moments(), twin.moments())
    # a move restarts the count; the ticks after it blend with the history
    loop.move(_moved(cam, 1))
    assert loop.frames_done == 0 and not loop.done() and not loop.converged and loop.n == 1 and tr.FrameIdx() == 0
    px = loop.tick().copy()
    assert tr.FrameIdx() == 1 and np.array_equal(px, tr.Pixels())
    px = loop.tick().copy()
    f = tr.FrameIdx()
    assert f >= 2 and np.array_equal(px, tr.present())
    assert (tr.temporal_resolve(length=True)[1] > f).any()
    assert not np.array_equal(px, tr.present(temporal=0))
    loop.close()
    # other keyword arguments reach present()
    tr.Reset()
    loop = ProgressiveLoop(tr, 4, first_frames=4, reconstruct=dict(denoise=0))
    assert np.array_equal(loop.tick(), tr.present(denoise=0))
    loop.close()
    tr.close()
    twin.close()
    # reconstruct needs moments; reconstruct=None is the loop as it was: Pixels() every tick
    _, tr = _tracer(moments=False)
    with pytest.raises(ValueError):
        ProgressiveLoop(tr, 4, reconstruct={})
    loop = ProgressiveLoop(tr, 7, first_frames=1)
    assert loop.reconstruct is None
    while not loop.done():
        assert np.array_equal(loop.tick(), tr.Pixels())
    assert tr.FrameIdx() == 7
    loop.close()
    tr.close()
