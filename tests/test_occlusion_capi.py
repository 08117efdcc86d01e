"""The occlusion queries' C ABI without a GPU (include/rt2.h "Ray queries"): the symbols, the refusals that need no
device, and the C++ mirror's members."""
import ctypes
import os
import subprocess

import numpy as np

import host_build as H
from conftest import ROOT

F32 = np.float32
SYMBOLS = ["rt2_tracer_occluded", "rt2_tracer_occluded_device"]


def test_symbols_are_exported_and_declared():
    import raytrace2_amd as R
    declared = R.declared_symbols()
    for s in SYMBOLS:
        assert s in declared and hasattr(R.lib, s), s
    assert callable(R.RayTracer.occluded) and callable(R.RayTracer.visible)


def test_refusals_through_the_c_abi():
    import raytrace2_amd as R
    L = R.lib
    fp, bp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int8)
    rays, out = np.zeros((2, 8), F32), np.full(2, 0x55, np.int8)
    pr, po = rays.ctypes.data_as(fp), out.ctypes.data_as(bp)
    INVALID = R._native.RT2_ERR_INVALID
    assert L.rt2_tracer_occluded(None, 2, pr, 1, po) == INVALID
    assert b"occluded: null tracer" in L.rt2_last_error()
    assert L.rt2_tracer_occluded_device(None, 2, ctypes.c_void_p(8), 1, ctypes.c_void_p(8)) == INVALID
    assert b"occluded_device: null tracer" in L.rt2_last_error()
    assert L.rt2_tracer_occluded(None, 0, pr, 1, po) == INVALID  # n == 0 excuses no null tracer
    assert b"occluded: null tracer" in L.rt2_last_error()
    assert L.rt2_tracer_occluded_device(None, 0, ctypes.c_void_p(8), 1, ctypes.c_void_p(8)) == INVALID
    assert b"occluded_device: null tracer" in L.rt2_last_error()
    for fn, what in ((L.rt2_tracer_occluded, b"occluded"), (L.rt2_tracer_occluded_device, b"occluded_device")):
        hand = (lambda p: p) if fn is L.rt2_tracer_occluded else (lambda p: ctypes.cast(p, ctypes.c_void_p))
        for n in (-1, -(1 << 40), 1 << 31, 1 << 40):
            assert fn(None, n, hand(pr), 1, hand(po)) == INVALID
            assert what + b": need 0 <= n < 2^31" in L.rt2_last_error(), n
        for a, b in ((None, hand(po)), (hand(pr), None), (None, None)):
            assert fn(None, 2, a, 1, b) == INVALID
            assert what + b": null pointer" in L.rt2_last_error()
    assert (out == 0x55).all()


def test_refusals_on_a_tracer_handle_need_no_launch():
    """A NULL pointer, n < 0 and n >= 2^31 are refused before anything touches the device, and n == 0 is RT2_OK:
    checked on a tracer where a device is present, and skipped over (nothing to create) where it is not."""
    import raytrace2_amd as R
    L = R.lib
    fp, bp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int8)
    sc = R.Scene(os.path.join(ROOT, "scenes", "cornell_box_original.json"), R.DEFAULT_SEED)
    h = ctypes.c_void_p()
    if L.rt2_tracer_create(sc._h, 0, ctypes.byref(h)) != 0:
        return  # no device on this machine: tests/test_gpu_occlusion.py covers the handle's refusals
    rays, out = np.zeros((2, 8), F32), np.full(2, 0x55, np.int8)
    pr, po = rays.ctypes.data_as(fp), out.ctypes.data_as(bp)
    for n, a, b in ((2, None, po), (2, pr, None), (-1, pr, po), (1 << 31, pr, po)):
        assert L.rt2_tracer_occluded(h, n, a, 1, b) == R._native.RT2_ERR_INVALID, n
        assert L.rt2_last_error().startswith(b"occluded: ")
    assert L.rt2_tracer_occluded(h, 0, pr, 1, po) == 0
    assert L.rt2_tracer_occluded_device(h, 0, ctypes.c_void_p(8), 1, ctypes.c_void_p(8)) == 0
    ms = ctypes.c_double(0)
    assert L.rt2_tracer_intersect_time(h, ctypes.byref(ms)) == 0 and ms.value == -1.0
    assert (out == 0x55).all()
    L.rt2_tracer_destroy(h)


def test_cpp_mirror_occlusion_members_compile_and_link():
    """include/rt2/RayTracer.hpp: Occluded, OccludedDevice, against the built library."""
    exe = H.program("mirror_occlusion.cpp", H.MIRROR, link=H.LIBRT2)
    r = subprocess.run([exe], capture_output=True, text=True)  # no arguments: it touches no device
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
