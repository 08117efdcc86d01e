"""Ambient occlusion on the GPU (include/rt2.h "Ambient occlusion"): the counts of
RayTracer.ambient_counts and ambient_points word for word against both the sum of RayTracer.occluded over the rays
tests/ambient_ref.py builds (from the tracer's own features(), or from the caller's points) and the oracle's counts,
in the threaded program and in the stack walk; the edges of the launch (waves that straddle points, sample counts
about 64, a 1x1 image, chunks), miss pixels and invalid points, the device entries' exact words, a partition, no
disturbance of a render or of the feature cache, repeatability, the refusals and rt2_headless --ao. Every test goes
through an ambient entry, which the library did not have before."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ambient_ref as A
import edge_rays as E
from conftest import ROOT
from helpers import SEED
from test_gpu_parity import MODES
from test_gpu_query import _tracer, _valid

pytestmark = pytest.mark.gpu
F32 = np.float32
FLT_MAX = np.finfo(F32).max
KERNELS = ["linear", "stack_global"]
CORNELL = "cornell_box_original"
APP = os.path.join(ROOT, "raytrace2_amd", "lib", "rt2_headless")
SIZE = (A.W, A.H)
FILL = 0x55555555


def _set(monkeypatch, mode):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)


def _occluded_flags(tr, rays, seed=SEED):
    """tr.occluded over rays (n, k, 8) as (n, k) 0 / 1: a ray that is not traced (-1) counts as clear."""
    f = tr.occluded(np.ascontiguousarray(rays.reshape(-1, 8)), seed=seed).reshape(rays.shape[0], rays.shape[1])
    return (f == 1).astype(np.uint32)


def _counts(flags, traced):
    return np.where(traced, flags.sum(-1).astype(np.uint32), A.INVALID).astype(np.uint32)


def _check(what, got, want, rays, traced, flags, width=None):
    """got == want word for word; a failure names the point (pixel), one of its samples, that ray and both answers."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.dtype == np.uint32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if not bad.size:
        return
    i = int(bad[0])
    where = f"pixel ({i % width}, {i // width})" if width else f"point {i}"
    lines = [f"{what}: {bad.size} of {got.size} counts differ; first: {where}: kernel {int(got[i])}, expected {int(want[i])}"]
    if traced[i]:
        s = int(np.flatnonzero(flags[i])[0]) if flags[i].any() else 0
        lines.append(f"  its sample {s}: ray {rays[i, s].tolist()} answers {int(flags[i, s])} in the expected count "
                     f"(the expected flags of its samples: {flags[i].tolist()})")
    pytest.fail("\n".join(lines))


def _image_case(tr, name, radius, samples, seed, what, oracle=None):
    """One image call against the occluded sum over the rays of the tracer's own features, and the oracle's counts."""
    feats = tr.features()
    rays, traced = A.image_rays(feats, radius, samples, seed)
    flags = _occluded_flags(tr, rays, seed)
    got = tr.ambient_counts(samples, radius, seed)
    w = feats.shape[1]
    assert got.shape == feats.shape[:2]
    _check(f"{what} against occluded", got, _counts(flags, traced), rays, traced, flags, w)
    miss = (feats[..., 0] == 0).reshape(-1)
    assert (got.reshape(-1)[miss] == A.INVALID).all() and (got.reshape(-1)[~miss] <= samples).all()
    if oracle is not None:
        o_counts, o_rays, o_traced = oracle
        assert np.array_equal(o_traced, traced) and np.array_equal(E.bits(o_rays[traced]), E.bits(rays[traced])), what
        _check(f"{what} against the oracle", got, o_counts, rays, traced, flags, w)
    return got


@pytest.mark.parametrize("mode", KERNELS)
@pytest.mark.parametrize("name,radius", A.IMAGE_CASES)
def test_image_against_occluded_and_the_oracle(have_gpu, monkeypatch, name, radius, mode):
    """32x18 with 24 samples (waves straddle points): every count equals the occluded sum and the oracle's; miss
    pixels answer 0xFFFFFFFF; Cornell volume again under a second seed, given to the call and not to the tracer, after
    which features() is still the tracer's own."""
    _set(monkeypatch, mode)
    sc, tr = _tracer(name, SIZE)
    got = _image_case(tr, name, radius, A.SAMPLES, SEED, f"{name} {float(radius)} {mode}", A.oracle_image(name, radius))
    assert (got == A.INVALID).any() and ((got > 0) & (got < A.SAMPLES)).sum() >= 100
    assert tr.ambient_time() >= 0
    if name == "cornell_box_volume":
        own = tr.features()
        seed2 = SEED + 7
        got2 = tr.ambient_counts(A.SAMPLES, radius, seed2)
        o_counts, o_rays, o_traced = A.oracle_image(name, radius, seed2)
        _check(f"{name} seed 2 against the oracle", got2, o_counts, o_rays, o_traced,
               np.zeros(o_rays.shape[:2], np.uint32), A.W)
        assert not np.array_equal(got2, got)
        assert np.array_equal(E.bits(tr.features()), E.bits(own))  # (the cache is keyed by the seed)
        tr.set_seed(seed2)
        _image_case(tr, name, radius, A.SAMPLES, seed2, f"{name} seed 2 {mode}", A.oracle_image(name, radius, seed2))
    assert tr.stats()["overflow"] == 0
    tr.close()


@pytest.mark.parametrize("mode", KERNELS)
def test_sample_counts_about_a_wave(have_gpu, monkeypatch, mode):
    """37x5 with 1, 63, 64, 65 and 130 samples (neither product is a multiple of 64): sample s does not depend on the
    count, so one batch of 130 rays per pixel serves every count by its prefix, on the GPU and on the oracle."""
    _set(monkeypatch, mode)
    sc, tr = _tracer(CORNELL, (37, 5))
    feats = tr.features()
    rays, traced = A.image_rays(feats, FLT_MAX, 130, SEED)
    flags = _occluded_flags(tr, rays)
    o_flags = np.zeros(flags.shape, np.uint32)
    for i in np.flatnonzero(traced):
        o_flags[i] = A.flags(E.scene_file(CORNELL), rays[i])
    # (the wide image sees the room in its middle columns only: hit and miss pixels share waves)
    part = o_flags.sum(-1)[traced]
    assert 20 <= traced.sum() < 37 * 5 and ((part > 0) & (part < 130)).sum() >= 20
    for k in (1, 63, 64, 65, 130):
        got = tr.ambient_counts(k)
        _check(f"{k} samples {mode} against occluded", got, _counts(flags[:, :k], traced), rays, traced, flags[:, :k], 37)
        _check(f"{k} samples {mode} against the oracle", got, _counts(o_flags[:, :k], traced), rays, traced,
               o_flags[:, :k], 37)
    tr.close()


def test_one_pixel(have_gpu):
    sc, tr = _tracer(CORNELL, (1, 1))
    feats = tr.features()
    assert feats[0, 0, 0] == 1
    rays, traced = A.image_rays(feats, FLT_MAX, 24, SEED)
    got = tr.ambient_counts(24)
    assert got.shape == (1, 1)
    flags = _occluded_flags(tr, rays)
    _check("1x1 against occluded", got, _counts(flags, traced), rays, traced, flags, 1)
    _check("1x1 against the oracle", got, A.counts(E.scene_file(CORNELL), rays, traced), rays, traced, flags, 1)
    vis = tr.ambient(24)
    assert vis.dtype == np.float32 and vis[0, 0] == F32(1) - F32(got[0, 0]) / F32(24)
    tr.close()


@pytest.mark.parametrize("mode", KERNELS)
@pytest.mark.parametrize("name", A.POINT_SCENES)
def test_points_against_occluded_and_the_oracle(have_gpu, monkeypatch, name, mode):
    """Point records from the hit rays of the scene's edge batch, before on_resize: the oracle's counts and the
    occluded sum; again in chunks of 64 and 128 points; book 2 (below its mist's free-flight distance) again without
    the list acceleration."""
    _set(monkeypatch, mode)
    pts = np.array(A.edge_points(name))
    o_counts, rays, traced = A.oracle_points(name)
    sc, tr = _tracer(name)
    flags = _occluded_flags(tr, rays)
    got = tr.ambient_points(pts, A.POINT_SAMPLES)
    _check(f"{name} {mode} against occluded", got, _counts(flags, traced), rays, traced, flags)
    _check(f"{name} {mode} against the oracle", got, o_counts, rays, traced, flags)
    assert tr.ambient_time() >= 0
    for chunk in ("64", "128"):
        monkeypatch.setenv("RT2_QUERY_CHUNK", chunk)
        assert np.array_equal(tr.ambient_points(pts, A.POINT_SAMPLES), got), chunk  # (the index is the record's)
    monkeypatch.delenv("RT2_QUERY_CHUNK")
    assert tr.stats()["overflow"] == 0
    tr.close()
    if name == A.BOOK2:
        monkeypatch.setenv("RT2_NO_LIST_ACCEL", "1")  # read at scene load
        sc, tr = _tracer(name)
        _check(f"{name} {mode} without the list tree", tr.ambient_points(pts, A.POINT_SAMPLES), o_counts, rays, traced, flags)
        tr.close()


def _bad_records(good):
    """One invalid record per valid one given: NaN, a zero normal, tmax <= 0.001, time 2, an origin at 2^65."""
    bad = np.array(good, F32)
    for k in range(len(bad)):
        c = k % 5
        if c == 0:
            bad[k, k % 8] = np.nan
        elif c == 1:
            bad[k, 4:7] = 0
        elif c == 2:
            bad[k, 3] = F32(0.001) if k % 2 else F32(0.0)
        elif c == 3:
            bad[k, 7] = 2
        else:
            bad[k, k % 3] = F32(2.0 ** 65)
    return bad


@pytest.mark.parametrize("mode", KERNELS)
@pytest.mark.parametrize("name", [CORNELL, "final_render_book_1"])
def test_invalid_points_stay_out(have_gpu, monkeypatch, name, mode):
    """Invalid records at every fourth place of a batch answer 0xFFFFFFFF and their neighbours answer the oracle's
    counts at their own indices; a batch of only invalid records answers 0xFFFFFFFF throughout."""
    import raytrace2_amd as R
    _set(monkeypatch, mode)
    good = np.array(A.edge_points(name)[:120])
    bad = _bad_records(good[:40])
    assert not _valid(bad).any() and not R.ray_valid(bad).any()
    mixed = np.zeros((160, 8), F32)
    is_bad = np.arange(160) % 4 == 3
    mixed[~is_bad], mixed[is_bad] = good, bad
    rays, traced = A.sample_rays(mixed, np.arange(160), A.POINT_SAMPLES)
    assert np.array_equal(traced, ~is_bad)
    want = A.counts(E.scene_file(name), rays, traced)
    sc, tr = _tracer(name)
    flags = _occluded_flags(tr, rays)
    got = tr.ambient_points(mixed, A.POINT_SAMPLES)
    _check(f"{name} {mode} mixed against the oracle", got, want, rays, traced, flags)
    _check(f"{name} {mode} mixed against occluded", got, _counts(flags, traced), rays, traced, flags)
    assert (got[is_bad] == A.INVALID).all() and (got[~is_bad] <= A.POINT_SAMPLES).all()
    assert (tr.ambient_points(bad, A.POINT_SAMPLES) == A.INVALID).all()
    assert (tr.ambient_points(np.tile(bad, (2, 1))[:64], 64) == A.INVALID).all()
    empty = tr.ambient_points(np.zeros((0, 8), F32), 4)
    assert empty.shape == (0,) and empty.dtype == np.uint32
    tr.close()


def test_device_entries_write_exactly_their_words(have_gpu):
    """Both device entries into n + 64 words of 0x55555555: the counts in the first n, the last 64 untouched; the
    tensor form of ambient_points."""
    import torch
    from raytrace2_amd._native import lib
    pts = np.array(A.edge_points(CORNELL))
    o_counts = A.oracle_points(CORNELL)[0]
    sc, tr = _tracer(CORNELL, SIZE)
    d_pts = torch.from_numpy(pts).cuda()
    d_got = tr.ambient_points(d_pts, A.POINT_SAMPLES)
    assert d_got.is_cuda and d_got.dtype == torch.int32
    assert np.array_equal(d_got.cpu().numpy().view(np.uint32), o_counts)
    assert tr.ambient_time() >= 0
    for n in (1, 65, 257):
        out = torch.full((n + 64,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert lib.rt2_tracer_ambient_points_device(tr._h, n, ctypes.c_void_p(d_pts.data_ptr()), A.POINT_SAMPLES, SEED,
                                                    ctypes.c_void_p(out.data_ptr())) == 0
        tr.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:n], o_counts[:n]) and (got[n:] == FILL).all(), n
    want = tr.ambient_counts(A.SAMPLES, F32(100)).reshape(-1)
    assert np.array_equal(want, A.oracle_image(CORNELL, F32(100))[0])
    n = want.size
    waits = tr.stats()["host_waits"]
    out = torch.full((n + 64,), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.rt2_tracer_ambient_device(tr._h, A.SAMPLES, 100.0, SEED, ctypes.c_void_p(out.data_ptr())) == 0
    assert tr.stats()["host_waits"] == waits  # (it only enqueues)
    tr.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:n], want) and (got[n:] == FILL).all()
    assert tr.ambient_time() >= 0
    tr.close()


def test_a_partition_answers_the_image_s_rows(have_gpu):
    from raytrace2_amd import local_rows
    sc, tr = _tracer("cornell_box_volume", SIZE)
    full = tr.ambient_counts(A.SAMPLES, F32(100))
    assert np.array_equal(full.reshape(-1), A.oracle_image("cornell_box_volume", F32(100))[0])
    rows = local_rows(A.H, 2, 1, 3)
    tr.set_partition(2, 1, 3)
    part = tr.ambient_counts(A.SAMPLES, F32(100))
    assert part.shape == (len(rows), A.W) and 0 < len(rows) < A.H
    assert np.array_equal(part, full[rows])
    pts = np.array(A.edge_points("cornell_box_volume")[:70])  # point mode needs no image and knows no partition
    assert np.array_equal(tr.ambient_points(pts, A.POINT_SAMPLES), A.oracle_points("cornell_box_volume")[0][:70])
    tr.close()


def test_no_disturbance_and_repeatable(have_gpu):
    """4 Updates, an ambient call by each entry, 4 Updates equal 8 Updates bit for bit: accumulation, FrameIdx() and
    the ray counts; features() returns the same bytes before and after; a second call returns the same bytes."""
    import torch
    from raytrace2_amd._native import lib
    pts = np.array(A.edge_points(CORNELL))

    def tracer():
        sc, tr = _tracer(CORNELL)
        tr.enable_ray_counts(True)
        tr.OnResize((48, 48))
        return sc, tr
    sc, tr = tracer()
    for _ in range(8):
        tr.Update(sc)
    ref, ref_idx, ref_rc, ref_rays = tr.Accumulation(), tr.FrameIdx(), tr.ray_counts(), tr.stats()["rays"]
    tr.close()
    sc, tr = tracer()
    for _ in range(4):
        tr.Update(sc)
    feats = tr.features()
    image = tr.ambient_counts(A.SAMPLES, F32(100))
    assert np.array_equal(tr.ambient_counts(A.SAMPLES, F32(100)), image)
    points = tr.ambient_points(pts, A.POINT_SAMPLES)
    assert np.array_equal(tr.ambient_points(pts, A.POINT_SAMPLES), points)
    assert np.array_equal(points, A.oracle_points(CORNELL)[0])
    d_points = tr.ambient_points(torch.from_numpy(pts).cuda(), A.POINT_SAMPLES)
    assert np.array_equal(d_points.cpu().numpy().view(np.uint32), points)
    d_image = torch.empty((image.size,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.rt2_tracer_ambient_device(tr._h, A.SAMPLES, 100.0, SEED, ctypes.c_void_p(d_image.data_ptr())) == 0
    tr.synchronize()
    assert np.array_equal(d_image.cpu().numpy().view(np.uint32), image.reshape(-1))
    assert np.array_equal(E.bits(tr.features()), E.bits(feats))
    assert tr.FrameIdx() == 4
    for _ in range(4):
        tr.Update(sc)
    assert tr.FrameIdx() == ref_idx == 8
    assert np.array_equal(tr.Accumulation().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(tr.ray_counts(), ref_rc) and tr.stats()["rays"] == ref_rays
    tr.close()


def test_refusals_on_a_live_tracer(have_gpu):
    """The arguments on a tracer handle; point mode needs no on_resize (a created tracer holds the scene's default
    image, so image mode's refusal of a tracer without one cannot be met here); a create_multi tracer refuses; a
    refused call leaves the output alone."""
    import raytrace2_amd as R
    from raytrace2_amd._native import lib
    INVALID = R._native.RT2_ERR_INVALID
    pts = np.array(A.edge_points(CORNELL)[:10])
    sc, tr = _tracer(CORNELL)
    assert np.array_equal(tr.ambient_points(pts, A.POINT_SAMPLES), A.oracle_points(CORNELL)[0][:10])
    tr.OnResize((2, 2))
    assert tr.Dims() == (2, 2) and tr.local_rows() == 2
    out = np.full(8, FILL, np.uint32)  # (room for the 2x2 image's four words and four more)
    po = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    fp = ctypes.POINTER(ctypes.c_float)
    for samples, radius in ((0, 100.0), (65536, 100.0), (4, 0.001), (4, float("nan")), (4, float("inf")), (4, -1.0)):
        assert lib.rt2_tracer_ambient(tr._h, samples, radius, SEED, po) == INVALID, (samples, radius)
        assert lib.rt2_last_error().startswith(b"ambient: need ")
    assert lib.rt2_tracer_ambient(tr._h, 4, 100.0, SEED, None) == INVALID
    for n in (-1, 1 << 31):
        assert lib.rt2_tracer_ambient_points(tr._h, n, pts.ctypes.data_as(fp), 4, SEED, po) == INVALID
        assert lib.rt2_last_error().startswith(b"ambient_points: need 0 <= n < 2^31")
    assert lib.rt2_tracer_ambient_points(tr._h, 0, pts.ctypes.data_as(fp), 4, SEED, po) == 0
    assert (out == FILL).all()
    assert lib.rt2_tracer_ambient(tr._h, 4, float(FLT_MAX), SEED, po) == 0 and (out[:4] != FILL).all() and (out[4:] == FILL).all()
    with pytest.raises(R.Rt2Error):
        tr.ambient_counts(0)
    tr.close()
    multi = R.RayTracer(sc, devices=[0, 0], band_h=8)
    multi.OnResize((16, 16))
    for call, what in ((lambda: multi.ambient_counts(4), "ambient"), (lambda: multi.ambient_points(pts, 4), "ambient_points")):
        with pytest.raises(R.Rt2Error) as e:
            call()
        assert e.value.code == INVALID and f"{what}: not on a create_multi tracer" in str(e.value)
    multi.close()


def test_headless_ao(have_gpu, tmp_path):
    """rt2_headless --ao writes the image WriteImage makes of ambient()'s visibility as a grey."""
    import raytrace2_amd as R
    got_png, want_png = str(tmp_path / "ao.png"), str(tmp_path / "want.png")
    r = subprocess.run([APP, E.scene_file(CORNELL), got_png, "--ao", "8", "--ao-radius", "100", "--size", "32x18"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sc, tr = _tracer(CORNELL, SIZE)
    vis = tr.ambient(8, F32(100))
    counts = tr.ambient_counts(8, F32(100))
    tr.close()
    assert vis.dtype == np.float32 and vis.shape == (A.H, A.W)
    assert (vis[counts == A.INVALID] == 1).all() and (counts == A.INVALID).any()
    hit = counts != A.INVALID
    assert np.array_equal(vis[hit], F32(1) - counts[hit].astype(F32) / F32(8)) and (vis[hit] < 1).any()
    R.WriteImage(np.repeat(vis[..., None], 3, axis=-1), A.W, A.H, want_png)
    assert open(got_png, "rb").read() == open(want_png, "rb").read()
