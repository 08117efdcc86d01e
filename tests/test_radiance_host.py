"""Radiance queries without a GPU (include/rt2.h "Radiance queries", raytrace2_amd/csrc/radiance.h): the stand-alone
tests/cpp/radiance_host.cpp (the plan's coverage under both kinds of split, the ordered sum over split sample ranges,
validity) plain and under the host sanitizers, the C ABI's symbols and the refusals that need no device, the C++
mirror's members, and the premise of the GPU test: the numpy camera rays of tests/radiance_ref.py, sent through
oracle.hit, reproduce the oracle's depth-1 render, and every case is as informative as DESIGN.md §6m records."""
import ctypes
import subprocess

import numpy as np
import pytest

import host_build as H
import radiance_ref as Rr
from test_gpu_query import _valid

F32 = np.float32
SYMBOLS = ["rt2_tracer_radiance", "rt2_tracer_radiance_device", "rt2_tracer_radiance_time"]
BOOK2 = "book2_final_scene_10000_samples"


@pytest.mark.parametrize("flags", ["HOST", "PLAN"])
@pytest.mark.parametrize("sanitize", [False, True])
def test_radiance_host_self_checks(flags, sanitize):
    """PlanRadiance's ranges, the ordered sum and validity; under the HOST and the PLAN flags, plain and with the host
    sanitizers (a stand-alone program with its own main)."""
    exe = H.program("radiance_host.cpp", [*getattr(H, flags), *(H.HOST_SAN if sanitize else ())])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "radiance host ok" in r.stdout


def test_cpp_mirror_radiance_members_compile():
    """include/rt2/RayTracer.hpp: RadianceDefaults, Radiance, RadianceDevice, RadianceTime."""
    H.syntax_only("mirror_radiance.cpp")


def test_symbols_are_exported_and_declared():
    import raytrace2_amd as R
    from raytrace2_amd._native import RadianceParams
    declared = R.declared_symbols()
    for s in SYMBOLS:
        assert s in declared and hasattr(R.lib, s), s
        assert getattr(R.lib, s).argtypes is not None and getattr(R.lib, s).restype is ctypes.c_int32, s
    assert "rt2_radiance_defaults" in declared and R.lib.rt2_radiance_defaults.restype is None
    assert len(R.lib.rt2_tracer_radiance.argtypes) == 8 and len(R.lib.rt2_tracer_radiance_device.argtypes) == 8
    assert [f for f, _ in RadianceParams._fields_] == ["samples", "max_depth", "first_draw"]
    assert ctypes.sizeof(RadianceParams) == 12
    p = RadianceParams(7, 7, 7)
    R.lib.rt2_radiance_defaults(ctypes.byref(p))
    assert (p.samples, p.max_depth, p.first_draw) == (1, 0, 0)
    R.lib.rt2_radiance_defaults(None)
    for m in ("radiance", "radiance_time"):
        assert callable(getattr(R.RayTracer, m)), m


def test_refusals_through_the_c_abi():
    """What needs no device, in CheckCall's order: the parameters, n, NULL pointers, a wrapping frame word (host
    entry), a NULL tracer; a refused call leaves the output alone."""
    import raytrace2_amd as R
    from raytrace2_amd._native import RadianceParams
    L = R.lib
    fp, up = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    INVALID = R._native.RT2_ERR_INVALID
    rays, out, cnt = np.zeros((2, 8), F32), np.full((2, 3), 0x55555555, np.uint32), np.full(2, 0x55555555, np.uint32)
    st = np.array([[0, 0], [1, 0xFFFFFFFF]], np.uint32)
    pr, po, pc, ps = rays.ctypes.data_as(fp), out.ctypes.data_as(fp), cnt.ctypes.data_as(up), st.ctypes.data_as(up)
    dev = ctypes.c_void_p(8)

    def host(n=2, r=pr, s=None, p=None, o=po):
        return L.rt2_tracer_radiance(None, n, r, s, ctypes.byref(p) if p else None, 1, o, pc)

    def device(n=2, r=dev, p=None, o=dev):
        return L.rt2_tracer_radiance_device(None, n, r, None, ctypes.byref(p) if p else None, 1, o, None)
    for call, what in ((host, b"radiance"), (device, b"radiance_device")):
        for prm in (RadianceParams(0, 0, 0), RadianceParams(-1, 0, 0), RadianceParams(65536, 0, 0), RadianceParams(1, -1, 0),
                    RadianceParams(1, 65536, 0), RadianceParams(1, 0, 9), RadianceParams(1, 0, 0xFFFFFFFF)):
            assert call(n=-1, p=prm) == INVALID  # (the parameters come before n)
            assert L.rt2_last_error().startswith(what + b": need 1 <= samples <= 65535"), what
        for n in (-1, -(1 << 40), 1 << 31, 1 << 40):
            assert call(n=n, r=None) == INVALID and (what + b": need 0 <= n < 2^31") in L.rt2_last_error(), n
        assert call(r=None) == INVALID and (what + b": null pointer") in L.rt2_last_error()
        assert call(o=None) == INVALID and (what + b": null pointer") in L.rt2_last_error()
        assert call() == INVALID and (what + b": null tracer") in L.rt2_last_error()
        assert call(n=0) == INVALID and (what + b": null tracer") in L.rt2_last_error()  # n == 0 excuses no null tracer
    assert host(s=ps, p=RadianceParams(2, 0, 0)) == INVALID and b"radiance: frame word + samples passes 2^32 at ray 1" in L.rt2_last_error()
    assert host(s=ps, p=RadianceParams(1, 0, 0)) == INVALID and b"radiance: null tracer" in L.rt2_last_error()
    ms = ctypes.c_double(0)
    assert L.rt2_tracer_radiance_time(None, ctypes.byref(ms)) == INVALID
    assert (out == 0x55555555).all() and (cnt == 0x55555555).all()


@pytest.mark.parametrize("case", Rr.CASES, ids=Rr.NAMES)
def test_the_premise_of_the_gpu_test(case):
    """The numpy rays through oracle.hit reproduce the oracle's depth-1 render (the light's emission, the background or
    0 at every pixel) at frames 0 and 7, and the case is as informative as recorded: at least 50 non-zero pixels, the
    distinct ray counts and the pixels that change at max_depth 5. Book 2 is wrapped in a mist whose free flight
    oracle.hit draws from its own probe stream and a render from the path's: there the pixels where the two depth-1
    images differ must be pixels that see a light or the background through the mist in one of them."""
    name, w, h, first_draw, nonzero, distinct, depth5 = case
    rays, streams, fd = Rr.case_rays(name)
    assert fd == first_draw and rays.shape == (Rr.FRAMES, w * h, 8) and _valid(rays.reshape(-1, 8)).all()
    assert Rr.FRAMES * w * h <= 5376  # (4,096 for the 16x16 cases; book 1's 24x14 is the largest)
    assert np.array_equal(streams[:, :, 0], np.tile(np.arange(w * h, dtype=np.uint32), (Rr.FRAMES, 1)))
    assert np.array_equal(streams[:, 0, 1], np.arange(Rr.FRAME0, Rr.FRAME0 + Rr.FRAMES, dtype=np.uint32))
    d = rays[..., 4:7].astype(np.float64)
    assert np.abs((d * d).sum(-1) - 1).max() < 1e-6
    for f in (0, 7):
        r, _, _ = Rr.camera_rays(name, w, h, [f])
        want = Rr.oracle(name).render(w, h, Rr.SPP, 1, frame_begin=f, max_depth=1, forward=True)[0].reshape(-1, 3)
        got = Rr.depth1_from_hits(name, r[0])
        bad = (got.view(np.uint32) != want.view(np.uint32)).any(-1)
        if name == BOOK2:
            assert ((got[bad] != 0).any(-1) | (want[bad] != 0).any(-1)).all() and bad.sum() <= 0.1 * w * h
        else:
            assert not bad.any(), (name, f, int(bad.sum()), np.flatnonzero(bad)[:5])
    acc, rc = Rr.case_render(name)
    assert int((acc.reshape(-1, 3) != 0).any(-1).sum()) == nonzero >= Rr.MIN_INFORMATIVE
    assert len(np.unique(rc)) == distinct
    if depth5 is not None:
        acc5 = Rr.case_render(name, 5)[0]
        assert int((acc5.view(np.uint32) != acc.view(np.uint32)).any(-1).sum()) == depth5
    one = Rr.case_render(name, 1)
    assert (one[1] == Rr.FRAMES).all()
