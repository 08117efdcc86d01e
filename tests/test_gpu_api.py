"""C-ABI error behaviour and host-side bookkeeping of a live tracer (needs the GPU): invalid
arguments return RT2_ERR_INVALID with a message and leave the tracer usable; FrameIdx counts queued
frames; Reset drops them."""
import numpy as np
import pytest

import raytrace2_amd as R
from conftest import scene_path
from raytrace2_amd._native import Rt2Error

pytestmark = pytest.mark.gpu


@pytest.fixture
def tracer(have_gpu):
    sc = R.Scene(scene_path("cornell_box_original"), R.DEFAULT_SEED)
    tr = R.RayTracer(sc, 0)
    tr.SetSamplesPerPixel(16)
    tr.OnResize((24, 16))
    yield tr
    tr.close()


@pytest.mark.parametrize("call", [
    lambda tr: setattr(tr, "max_depth", 70000),
    lambda tr: tr.OnResize((0, 5)),
    lambda tr: tr.OnResize((70000, 5)),
    lambda tr: tr.Render(-1),
    lambda tr: tr.SetSamplesPerPixel(0),
    lambda tr: tr.set_work_split(-1),
    lambda tr: tr.set_batch_max(0),
    lambda tr: tr.set_lazy_frames(-1),
    lambda tr: tr.set_partition(8, 3, 2),
])
def test_invalid_arguments_fail_loudly_and_keep_the_tracer(tracer, call):
    with pytest.raises(Rt2Error) as e:
        call(tracer)
    assert e.value.args and "rt2 error -1" in str(e.value)
    tracer.Render(2)
    assert tracer.FrameIdx() == 2 and np.isfinite(tracer.NonConvertedPixels()).all()


def test_camera_beyond_the_exact_range_fails_loudly(tracer):
    """The rectangle test is exact for ray origins within +-2^100 (compile.cpp RectAAWords): a camera
    whose rays would start beyond +-2^64 (capi.cpp CameraOriginsBounded) is refused at Render with
    RT2_ERR_INVALID, and the tracer renders again once the camera is back in range."""
    import dataclasses
    good = tracer.get_camera()
    tracer.set_camera(dataclasses.replace(good, center=(1e30, 278.0, -800.0)))
    with pytest.raises(Rt2Error) as e:
        tracer.Render(1)
    assert "2^64" in str(e.value)
    tracer.set_camera(good)
    tracer.Render(2)
    assert tracer.FrameIdx() == 2 and np.isfinite(tracer.NonConvertedPixels()).all()


def test_far_camera_renders_sphere_scenes_like_the_oracle():
    """the +-2^64 camera bound belongs to the tests that need it (QUADAA rectangles, box
    boundaries, transforms about y: CompiledScene::origins_bounded). A sphere-only scene renders a camera
    beyond it as the reference would (here every ray misses: the sphere test's squares overflow), bit for
    bit like the oracle."""
    from oracle.oracle import OracleScene
    name, w, h, spp, frames = "perlin_spheres", 24, 16, 4, 3
    sc = R.Scene(scene_path(name), R.DEFAULT_SEED)
    far = R.Camera((3e20, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, 0.0, 10.0)
    tr = R.RayTracer(sc, 0)
    tr.set_seed(R.DEFAULT_SEED)
    tr.SetSamplesPerPixel(spp)
    tr.OnResize((w, h))
    tr.camera = far
    tr.Render(frames)
    acc = tr.Accumulation()
    tr.close()
    o = OracleScene(scene_path(name), R.DEFAULT_SEED)
    o.set_camera(far.center, far.look_at, far.view_up, far.vfov, far.defocus_angle, far.focus_distance)
    o_acc, _, _ = o.render(w, h, spp, frames, forward=True)
    assert np.array_equal(acc.view(np.uint32), o_acc.view(np.uint32))


def test_queued_frames_and_reset(tracer):
    for _ in range(5):
        tracer.Update()
    assert tracer.FrameIdx() == 5 and tracer.stats()["launches"] == 1  # stats() launched the queue
    tracer.Update()
    tracer.Reset()  # drops the queued frame: nothing is launched for it
    assert tracer.FrameIdx() == 0 and tracer.stats()["launches"] == 1
    assert not tracer.Accumulation().any()
    tracer.Render(3)
    a = tracer.Accumulation()
    assert tracer.FrameIdx() == 3 and a.any()


def test_kernel_time_is_gpu_busy_time_not_queue_time(have_gpu):
    """with two launch slots, step i + 1's render is queued while step i's still
    holds the CUs; kernel_ms must count the time the GPU ran render launches (each launch timed by its
    own first-wave / last-wave clock, overlaps once), not the time a launch waited in its queue. Back
    to back renders (the bench's step shape, no host wait between them): kernel time <= wall time,
    the sum of the launches' own times >= their union, and the host never waited inside the loop."""
    import time
    sc = R.Scene(scene_path("cornell_box_original"), R.DEFAULT_SEED)
    tr = R.RayTracer(sc, 0)
    tr.SetSamplesPerPixel(1000)
    tr.OnResize((256, 256))
    tr.Render(100)
    tr.synchronize()
    tr.reset_stats()
    steps = 6
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.Reset()
        tr.Render(1000)
        tr.flush()
    # (stats() synchronizes, and reports the host waits from before its own synchronization)
    waits_in_loop = tr.stats()["host_waits"]
    tr.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    st = tr.stats()
    tr.close()
    assert st["launches"] == steps
    assert 0.0 < st["kernel_ms"] <= wall_ms * 1.001, (st["kernel_ms"], wall_ms)
    assert st["launch_ms_sum"] >= st["kernel_ms"] * 0.9999, (st["launch_ms_sum"], st["kernel_ms"])
    # consecutive launches overlap only in a launch's tail (about a millisecond)
    assert st["launch_ms_sum"] <= st["kernel_ms"] + 3.0 * steps, (st["launch_ms_sum"], st["kernel_ms"])
    # structural (no wall-clock ratio): the launch path blocked the host nowhere
    assert waits_in_loop == 0, waits_in_loop
    print(f"kernel {st['kernel_ms']:.1f} ms of {wall_ms:.1f} ms wall (informational)")
    # the two launch slots' sample buffers stay within the (total) sample budget (rt2.h)
    assert 0 < st["sample_buffer_bytes"] <= (24 << 30)
    assert st["sample_buffer_bytes"] == 2 * 1000 * 256 * 256 * 12
    assert st["device_bytes_peak"] >= st["sample_buffer_bytes"] + 256 * 256 * 16


@pytest.mark.parametrize("name,w,h,spp,frames", [("cornell_box_original", 64, 64, 1000, 6),
                                                 ("cornell_box_volume", 64, 64, 1000, 6),
                                                 ("book2_final_scene_10000_samples", 48, 48, 10000, 4)])
def test_box_level_test_certifies_and_changes_no_bit(have_gpu, monkeypatch, name, w, h, spp, frames):
    """The box-level test (boxaa.h; DESIGN.md §4 "Box-level test"): the compiler gives the scene's MakeBox
    runs and MakeBox medium boundaries a box record, the counting kernel reports that it certifies
    nearly every lane there (the rest run the six faces), and the accumulation equals, bit for bit, the
    render with the test switched off (RT2_BOX_AA=0 at scene load: plain six-face runs)."""
    def render(env):
        if env is None:
            monkeypatch.delenv("RT2_BOX_AA", raising=False)
        else:
            monkeypatch.setenv("RT2_BOX_AA", env)
        sc = R.Scene(scene_path(name), R.DEFAULT_SEED)
        tr = R.RayTracer(sc, 0)
        tr.set_seed(R.DEFAULT_SEED)
        tr.SetSamplesPerPixel(spp)
        tr.OnResize((w, h))
        tr.enable_stats(True)
        tr.Render(frames)
        acc = tr.Accumulation().copy()
        st = tr.stats()
        tr.close()
        return sc.info().box_steps, acc, st
    steps, acc, st = render(None)
    steps0, acc0, st0 = render("0")
    assert steps > 0 and steps0 == 0
    assert st["box_tests"] > 0 and st0["box_tests"] == 0
    assert st["box_certified"] >= 0.99 * st["box_tests"], (st["box_certified"], st["box_tests"])
    assert st["box_wave_runs"] <= 0.01 * st["box_wave_visits"], (st["box_wave_runs"], st["box_wave_visits"])
    assert st["rays"] == st0["rays"] and st["quad_tests"] == st0["quad_tests"]  # the reference's counts
    assert np.array_equal(acc.view(np.uint32), acc0.view(np.uint32))


def test_scene_past_the_step_limit_renders_on_the_stack_like_the_oracle(have_gpu, monkeypatch):
    """A threaded program given up part-way (RT2_LINEAR_MAX_STEPS=10 at scene load, below the Cornell box's 29
    steps and after its first MakeBox was recorded) leaves a stack-traversal scene: no threaded steps, no box
    steps, and an accumulation bit-identical to the scene loaded without the variable and to the oracle."""
    from oracle.oracle import OracleScene
    name, w, h, spp, frames = "cornell_box_original", 32, 32, 4, 4

    def render(env):
        if env is None:
            monkeypatch.delenv("RT2_LINEAR_MAX_STEPS", raising=False)
        else:
            monkeypatch.setenv("RT2_LINEAR_MAX_STEPS", env)
        sc = R.Scene(scene_path(name), R.DEFAULT_SEED)
        tr = R.RayTracer(sc, 0)
        tr.set_seed(R.DEFAULT_SEED)
        tr.SetSamplesPerPixel(spp)
        tr.OnResize((w, h))
        tr.Render(frames)
        acc = tr.Accumulation().copy()
        tr.close()
        return sc.info(), acc
    info10, acc10 = render("10")
    info, acc = render(None)
    assert info.linear_steps > 10 and info.box_steps > 0
    assert info10.linear_steps == 0 and info10.box_steps == 0
    o_acc, _, _ = OracleScene(scene_path(name), R.DEFAULT_SEED).render(w, h, spp, frames, forward=True)
    assert np.array_equal(acc10.view(np.uint32), acc.view(np.uint32))
    assert np.array_equal(acc10.view(np.uint32), o_acc.view(np.uint32))


def test_medium_box_far_away_matches_the_oracle(have_gpu):
    """The medium's box-boundary test (boxaa.h BoxAAPair) at distances where the second boundary query
    starts on the first hit itself: for t1 above 2^11, fl(t1 + 0.0001) = t1 (ConstantMedium.cpp:26-30), so
    the entry face answers both queries and the medium has zero thickness there. The Cornell volume seen
    from 6000 units away, bit-identical to the oracle (whose two queries run on the six faces)."""
    from oracle.oracle import OracleScene
    name, w, h, spp, frames = "cornell_box_volume", 24, 24, 4, 3
    sc = R.Scene(scene_path(name), R.DEFAULT_SEED)
    assert sc.info().box_steps == 2
    cam = R.Camera((278.0, 278.0, -6000.0), (278.0, 278.0, 0.0), (0.0, 1.0, 0.0), 6.0, 0.0, 10.0)
    tr = R.RayTracer(sc, 0)
    tr.set_seed(R.DEFAULT_SEED)
    tr.SetSamplesPerPixel(spp)
    tr.OnResize((w, h))
    tr.camera = cam
    tr.enable_stats(True)
    tr.Render(frames)
    acc = tr.Accumulation()
    st = tr.stats()
    tr.close()
    o = OracleScene(scene_path(name), R.DEFAULT_SEED)
    o.set_camera(cam.center, cam.look_at, cam.view_up, cam.vfov, cam.defocus_angle, cam.focus_distance)
    o_acc, _, _ = o.render(w, h, spp, frames, forward=True)
    assert st["box_certified"] > 0
    assert np.array_equal(acc.view(np.uint32), o_acc.view(np.uint32))


# ---- device-byte accounting ---------------------------------------------------------------------------------
# Scene program, tables and small per-tracer buffers (work counters, clock ring, counters) of the two scenes, in
# bytes: what a fresh tracer reported beyond its frame buffers before the flat program's tables were counted.
CORNELL_SCENE_BYTES = 17140
BOOK1_SCENE_BYTES = 167476
# The Cornell box's flat program: its wide steps, 64 * (flat_steps + 1) = 1472 bytes, and the certificate table,
# 1984 bytes (one float per float of the threaded program's records).
CORNELL_FLAT_BYTES = 1472 + 1984


@pytest.mark.parametrize("w,h", [(64, 48), (672, 672)])
def test_device_bytes_peak_is_the_sum_of_the_buffers(have_gpu, w, h):
    """rt2_stats.device_bytes_peak is the high-water mark of everything the tracer holds: it equals, state by
    state, the running maximum of the documented buffer list (a tracer is created at the scene's own dims, which
    is the mark until a larger state; 672 x 672 is above the Cornell box's 600 x 600, so there every Cornell state
    shows, while book 1's 1600 x 900 mark checks its scene bytes alone)."""
    from raytrace2_amd.dist import band_rows_max
    n = w * h
    sc = R.Scene(scene_path("cornell_box_original"), R.DEFAULT_SEED)
    assert 64 * (sc.info().flat_steps + 1) == 1472
    scene = CORNELL_SCENE_BYTES + CORNELL_FLAT_BYTES
    tr = R.RayTracer(sc, 0)
    peak = scene + 600 * 600 * 16  # accumulation float3 + RGBA8 at the scene's 600 x 600

    def check(t, now, what):
        nonlocal peak
        peak = max(peak, now)
        got = t.stats()["device_bytes_peak"]
        print(f"{w}x{h} {what}: held {now}, peak {got}")
        assert got == peak, (what, got, peak)

    tr.SetSamplesPerPixel(16)
    tr.OnResize((w, h))
    check(tr, scene + n * 16, "fresh")
    tr.enable_moments()  # + the float3 sums of squares
    check(tr, scene + n * 28, "moments")
    tr.enable_adaptive()  # + counts, active, over, list (padded by 64), slot_of, and the check's scratch
    tiles, blocks = -(-w // 32) * -(-h // 8), -(-n // 256)
    frame = n * 28 + n * 14 + 256 + tiles * 12 + 4 + blocks * 16 + 32 + 16
    check(tr, scene + frame, "adaptive")
    tr.Render(2)
    tr.denoise()
    assert tr.last_launch()["chunk_frames"] == 1
    # one launch slot: an octet of frames of float3 samples, and the table of two one-frame chunks and the
    # sentinel; the feature records (16 floats); the filter's scratch (DenoiseScratchBytes: 100 bytes per pixel)
    held = scene + frame + 8 * n * 12 + 24 + n * 64 + n * 100
    check(tr, held, "denoise")
    tr.temporal_resolve()  # + the packed history (64 bytes per pixel) and the length plane
    check(tr, held + n * 68, "temporal")
    tr.close()

    # two parts on one GPU: each holds its band stack (the largest rank's rows); the root, after a gather, also
    # the gathered stacks and the image (float3 sum, float3 mean, RGBA8)
    tr = R.RayTracer(sc, devices=[0, 0])
    peak = scene + 600 * 600 * 16
    tr.OnResize((w, h))
    rows = band_rows_max(h, 2, 2)
    tr.gather()
    check(tr, scene + w * rows * 16 + 2 * rows * w * 12 + n * 28, "gathered")
    tr.close()

    sc = R.Scene(scene_path("final_render_book_1"), R.DEFAULT_SEED)
    assert sc.info().flat_steps == 0
    tr = R.RayTracer(sc, 0)
    peak = BOOK1_SCENE_BYTES + 1600 * 900 * 16  # no dims in the scene file: the window default
    tr.OnResize((w, h))
    check(tr, BOOK1_SCENE_BYTES + n * 16, "book 1, fresh")
    tr.close()


@pytest.mark.parametrize("size,resized", [((64, 48), (96, 80)), ((290, 201), (500, 365))])
def test_device_bytes_peak_counts_the_gathered_image_and_its_reconstruction(have_gpu, size, resized):
    """The root of two parts on one GPU (stats() of a multi tracer is the largest part's, the root's): state by
    state, device_bytes_peak is the running maximum of the documented list, the gathered image's six
    reconstruction buffers included; and a resize drops every one of them. As above, the parts are created at the
    scene's 600 x 600, which is the mark until a larger state: at 64 x 48 nothing rises above it (the mark itself
    is what is checked), at 290 x 201 every state does, and its resize to 500 x 365 is large enough that the new
    size's list without any reconstruction buffer is above everything the old size held, so a buffer that
    survived the resize at its old size would show as an excess."""
    from raytrace2_amd import local_rows
    from raytrace2_amd.dist import band_rows_max
    sc = R.Scene(scene_path("cornell_box_original"), R.DEFAULT_SEED)
    scene = CORNELL_SCENE_BYTES + CORNELL_FLAT_BYTES
    peak = scene + 600 * 600 * 16

    def rendered(w, h):
        """What the root holds after 2 frames with moments on: its band's sums, pixels and sums of squares (as
        tall as the largest rank's band), and one launch slot: an octet of frames of float3 samples of its own
        rows, and the table of two one-frame chunks and the sentinel."""
        rows, own = band_rows_max(h, 2, 2), len(local_rows(h, 2, 0, 2))
        return scene + w * rows * 28 + 8 * w * own * 12 + 24

    def gathered(w, h):
        """+ the two gathered stacks (sums, sums of squares: capi_multi.cpp EnsureImage, EnsureEstimate), the image
        (float3 sum, float3 mean, RGBA8) and the variance plane."""
        return rendered(w, h) + 2 * (2 * band_rows_max(h, 2, 2) * w * 12) + w * h * 28 + w * h * 4

    def check(now, what):
        nonlocal peak
        peak = max(peak, now)
        got = tr.stats()["device_bytes_peak"]
        print(f"{w}x{h} {what}: held {now}, peak {got}")
        assert got == peak, (what, got, peak)

    tr = R.RayTracer(sc, devices=[0, 0])
    tr.SetSamplesPerPixel(16)
    (w, h), n = size, size[0] * size[1]
    tr.OnResize((w, h))
    tr.enable_moments()
    tr.Render(2)
    tr.gather_estimate()
    assert tr.last_launch()["chunk_frames"] == 1
    check(gathered(w, h), "gather_estimate")
    # + the whole-image feature records (16 floats), the filter's scratch (denoise.hip DenoiseScratchBytes: 100 bytes
    # per pixel), the packed history (temporal.hip TemporalHistoryBytes: 64) and the length plane
    full = gathered(w, h) + n * 64 + n * 100 + n * 68
    tr.image_resolve(temporal=1, denoise=1)
    check(full, "image_resolve")
    tr.image_present()  # the RGBA8 words live in the scratch
    check(full, "image_present")
    # the resize frees the frame buffers, the sample buffer and the gathered image; the next launch takes the other
    # launch slot (launches alternate), and the first slot keeps its 24-byte chunk table until the tracer goes
    (w, h), n = resized, resized[0] * resized[1]
    again = gathered(w, h) + 24
    if size != (64, 48):
        assert again > full, "the resized list alone is above the old peak"
    tr.OnResize((w, h))
    tr.Render(2)
    tr.gather_estimate()
    assert tr.last_launch()["chunk_frames"] == 1
    check(again, "resized, gather_estimate")
    tr.image_resolve(temporal=1, denoise=1)
    check(again + n * 232, "resized, image_resolve")
    tr.close()
