"""The query families' timers on the GPU (tracer.h KernelTimer, capi_query.cpp ChunkedHostCall): intersect's and
occluded's, ambient occlusion's, the radiance queries' and the present's are four timers, each moved by its own calls
alone; a device entry's time is readable after a synchronise and is read once and kept; a host entry's time is the sum
over its chunks and readable at once, and chunks change no answer. Cornell at 32x32, the first 192 of the camera's own
rays of frame 0 (three waves, the last of which is a chunk of its own under RT2_QUERY_CHUNK=64), samples 2. stats() has
no count of the events created, so that the borrowed events go back to the pool is not checked here."""
import ctypes
import functools

import numpy as np
import pytest

import radiance_ref as Rr
from bits import same_bits
from helpers import SEED
from test_gpu_query import _tracer

pytestmark = pytest.mark.gpu
NAME = "cornell_box_original"
SIZE = (32, 32)
N, SAMPLES = 192, 2


@functools.lru_cache(maxsize=None)
def _rays():
    """(rays (N, 8) float32, streams (N, 2) uint32, first_draw), read-only."""
    rays, streams, fd = Rr.camera_rays(NAME, *SIZE, [0])
    rays, streams = np.array(rays[0, :N]), np.array(streams[0, :N])
    rays.setflags(write=False)
    streams.setflags(write=False)
    return rays, streams, fd


def _times(tr):
    return tr.intersect_time(), tr.ambient_time(), tr.radiance_time()


def _host_calls(tr):
    """The three families' host entries over the rays: (records, counts, sums) and each call's time read at once."""
    rays, streams, fd = _rays()
    rec = tr.intersect(rays)
    t_i = tr.intersect_time()
    cnt = tr.ambient_points(rays, SAMPLES)
    t_a = tr.ambient_time()
    rad = tr.radiance(rays, samples=SAMPLES, streams=streams, first_draw=fd)
    t_r = tr.radiance_time()
    return (rec, cnt, rad), (t_i, t_a, t_r)


def test_four_timers_each_moved_by_its_own_calls(have_gpu):
    rays, streams, fd = _rays()
    sc, tr = _tracer(NAME, SIZE)
    tr.enable_moments()
    tr.Render(2)
    assert _times(tr) == (-1, -1, -1) and tr.present_time() == -1
    tr.intersect(rays)
    t_i = tr.intersect_time()
    assert t_i >= 0 and _times(tr) == (t_i, -1, -1)
    tr.ambient_points(rays, SAMPLES)
    t_a = tr.ambient_time()
    assert t_a >= 0 and _times(tr) == (t_i, t_a, -1)
    tr.radiance(rays, samples=SAMPLES, streams=streams, first_draw=fd)
    t_r = tr.radiance_time()
    assert t_r >= 0 and _times(tr) == (t_i, t_a, t_r)
    tr.occluded(rays)  # (the other kind of the first family)
    t_o = tr.intersect_time()
    assert t_o >= 0 and _times(tr) == (t_o, t_a, t_r)
    assert tr.present_time() == -1
    tr.present(temporal=False)
    tr.synchronize()
    assert _times(tr) == (t_o, t_a, t_r)
    assert tr.present_time() >= 0
    tr.close()


def test_device_entries_time_after_a_synchronise_read_once(have_gpu):
    """The raw device entries (RayTracer's methods synchronise): after the synchronise the family's time is there, a
    second read returns the same value, and the words are the host entry's."""
    import torch
    from raytrace2_amd._native import RadianceParams, lib
    rays, streams, fd = _rays()
    sc, tr = _tracer(NAME, SIZE)
    (rec, cnt, rad), _ = _host_calls(tr)
    occ = tr.occluded(rays)
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    d_streams = torch.from_numpy(np.array(streams).view(np.int32)).cuda()
    prm = RadianceParams(SAMPLES, 0, fd)

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr())

    cases = [
        ("intersect", tr.intersect_time, rec, torch.float32,
         lambda out: lib.rt2_tracer_intersect_device(tr._h, N, ptr(d_rays), SEED, ptr(out))),
        ("occluded", tr.intersect_time, occ, torch.int8,
         lambda out: lib.rt2_tracer_occluded_device(tr._h, N, ptr(d_rays), SEED, ptr(out))),
        ("ambient_points", tr.ambient_time, cnt, torch.int32,
         lambda out: lib.rt2_tracer_ambient_points_device(tr._h, N, ptr(d_rays), SAMPLES, SEED, ptr(out))),
        ("radiance", tr.radiance_time, rad, torch.float32,
         lambda out: lib.rt2_tracer_radiance_device(tr._h, N, ptr(d_rays), ptr(d_streams), ctypes.byref(prm), SEED,
                                                    ptr(out), None)),
    ]
    for what, time, want, dtype, call in cases:
        out = torch.zeros(want.shape, dtype=dtype, device="cuda")
        torch.cuda.synchronize()
        waits = tr.stats()["host_waits"]
        assert call(out) == 0, what
        assert tr.stats()["host_waits"] == waits, what  # (it only enqueues)
        tr.synchronize()
        ms = time()
        assert np.isfinite(ms) and ms >= 0, what
        assert time() == ms, what
        assert same_bits(out.cpu().numpy().view(want.dtype), want), what
    tr.close()


def test_host_entries_sum_their_chunks(have_gpu, monkeypatch):
    """Three chunks of 64: each time is there as the call returns, with no synchronise, and the answers are the
    unchunked call's bit for bit."""
    sc, tr = _tracer(NAME, SIZE)
    whole, _ = _host_calls(tr)
    monkeypatch.setenv("RT2_QUERY_CHUNK", "64")
    chunked, (t_i, t_a, t_r) = _host_calls(tr)
    assert t_i > 0 and t_a >= 0 and t_r >= 0
    for a, b, what in zip(chunked, whole, ("intersect", "ambient_points", "radiance")):
        assert same_bits(a, b), what
    tr.close()
