"""The ray queries' C ABI without a GPU (include/rt2.h "Ray queries"): the symbols, the refusals that need no
device, rt2_query_ray_valid against a numpy restatement of the rule, and the C++ mirror's members."""
import ctypes
import os
import subprocess

import numpy as np

import host_build as H
from conftest import ROOT

F32 = np.float32
SYMBOLS = ["rt2_query_ray_valid", "rt2_tracer_intersect", "rt2_tracer_intersect_device", "rt2_tracer_intersect_time"]


def _valid(r):
    """query.h QueryRayValid in numpy: all words finite; the largest |d| component within [2^-20, 2^20]; every origin
    coordinate within +-2^64; 0.001 < tmax; 0 <= time <= 1."""
    r = np.asarray(r, F32).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        m = np.abs(r[:, 4:7]).max(-1)
        return (np.isfinite(r).all(-1) & (m >= F32(2.0 ** -20)) & (m <= F32(2.0 ** 20))
                & (np.abs(r[:, 0:3]) <= F32(2.0 ** 64)).all(-1) & (r[:, 3] > F32(0.001)) & (r[:, 7] >= 0) & (r[:, 7] <= 1))


def test_symbols_are_exported_and_declared():
    import raytrace2_amd as R
    declared = R.declared_symbols()
    for s in SYMBOLS:
        assert s in declared and hasattr(R.lib, s), s
    assert callable(R.RayTracer.intersect) and callable(R.RayTracer.intersect_time) and callable(R.ray_valid)


def test_refusals_through_the_c_abi():
    import raytrace2_amd as R
    L = R.lib
    fp = ctypes.POINTER(ctypes.c_float)
    rays, out = np.zeros((2, 8), F32), np.zeros((2, 16), F32)
    pr, po = rays.ctypes.data_as(fp), out.ctypes.data_as(fp)
    ms = ctypes.c_double(0)
    INVALID = R._native.RT2_ERR_INVALID
    assert L.rt2_tracer_intersect(None, 2, pr, 1, po) == INVALID
    assert b"intersect: null tracer" in L.rt2_last_error()
    assert L.rt2_tracer_intersect_device(None, 2, ctypes.c_void_p(8), 1, ctypes.c_void_p(8)) == INVALID
    assert b"intersect_device: null tracer" in L.rt2_last_error()
    assert L.rt2_tracer_intersect(None, 0, pr, 1, po) == INVALID  # n == 0 excuses no null tracer
    assert b"null tracer" in L.rt2_last_error()
    for fn, what in ((L.rt2_tracer_intersect, b"intersect"), (L.rt2_tracer_intersect_device, b"intersect_device")):
        hand = (lambda p: p) if fn is L.rt2_tracer_intersect else (lambda p: ctypes.cast(p, ctypes.c_void_p))
        for n in (-1, -(1 << 40), 1 << 31, 1 << 40):
            assert fn(None, n, hand(pr), 1, hand(po)) == INVALID
            assert what + b": need 0 <= n < 2^31" in L.rt2_last_error(), n
        for a, b in ((None, hand(po)), (hand(pr), None), (None, None)):
            assert fn(None, 2, a, 1, b) == INVALID
            assert what + b": null pointer" in L.rt2_last_error()
    assert L.rt2_tracer_intersect_time(None, ctypes.byref(ms)) == R._native.RT2_ERR_INVALID
    assert b"null" in L.rt2_last_error()
    assert L.rt2_query_ray_valid(None) == 0
    assert not out.any()


def test_refusals_on_a_tracer_handle_need_no_launch():
    """A NULL pointer, n < 0 and n >= 2^31 are refused before anything touches the device: checked on a tracer where
    a device is present, and skipped over (nothing to create) where it is not."""
    import raytrace2_amd as R
    L = R.lib
    fp = ctypes.POINTER(ctypes.c_float)
    sc = R.Scene(os.path.join(ROOT, "scenes", "cornell_box_original.json"), R.DEFAULT_SEED)
    h = ctypes.c_void_p()
    if L.rt2_tracer_create(sc._h, 0, ctypes.byref(h)) != 0:
        return  # no device on this machine: tests/test_gpu_query.py covers the handle's refusals
    rays, out = np.zeros((2, 8), F32), np.zeros((2, 16), F32)
    pr, po = rays.ctypes.data_as(fp), out.ctypes.data_as(fp)
    for n, a, b in ((2, None, po), (2, pr, None), (-1, pr, po), (1 << 31, pr, po)):
        assert L.rt2_tracer_intersect(h, n, a, 1, b) == R._native.RT2_ERR_INVALID, n
        assert L.rt2_last_error()
    assert L.rt2_tracer_intersect(h, 0, pr, 1, po) == 0
    ms = ctypes.c_double(0)
    assert L.rt2_tracer_intersect_time(h, ctypes.byref(ms)) == 0 and ms.value == -1.0
    L.rt2_tracer_destroy(h)


def test_ray_valid_agrees_with_numpy():
    import raytrace2_amd as R
    rng = np.random.default_rng(5)
    rnd = rng.integers(0, 1 << 32, (10000, 8), dtype=np.uint64).astype(np.uint32).view(F32)
    # random bit patterns are almost never valid: half of them get plausible words in a random subset of slots
    base = np.array([1, 2, 3, 1e30, 0.6, 0, -0.8, 0.5], F32)
    keep = rng.random((10000, 8)) < 0.85
    keep[5000:] = False
    mixed = np.where(keep, base, rnd).astype(F32)
    nxt = lambda x, d: np.nextafter(F32(x), F32(d))
    inf, nan = np.inf, np.nan
    edges = []
    for k in range(8):
        for v in (nan, inf, -inf, 0.0, -0.0):
            e = base.copy()
            e[k] = v
            edges.append(e)
    for v in (0.001, nxt(0.001, 1), np.finfo(F32).max):
        e = base.copy()
        e[3] = v
        edges.append(e)
    for v in (-0.0, 0.0, 1.0, nxt(1, 2), nxt(-0.0, -1)):
        e = base.copy()
        e[7] = v
        edges.append(e)
    for k in range(3):
        for s in (1, -1):
            for v in (2.0 ** 64, nxt(2.0 ** 64, inf)):
                e = base.copy()
                e[k] = s * v
                edges.append(e)
            for v in (2.0 ** 20, nxt(2.0 ** 20, inf), 2.0 ** -20, nxt(2.0 ** -20, 0)):
                e = base.copy()
                e[4:7] = 0
                e[4 + k] = s * v
                edges.append(e)
    e = base.copy()
    e[4:7] = 0
    edges.append(e)
    allr = np.concatenate([mixed, np.array(edges, F32)])
    want = _valid(allr)
    got = R.ray_valid(allr)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert want.sum() > 1000 and (~want).sum() > 1000
    assert got[len(mixed):].any() and not got[len(mixed):].all()


def test_cpp_mirror_intersect_members_compile_and_link():
    """include/rt2/RayTracer.hpp: Intersect, IntersectDevice, IntersectTime, RayValid, against the built library."""
    exe = H.program("mirror_intersect.cpp", H.MIRROR, link=H.LIBRT2)
    r = subprocess.run([exe], capture_output=True, text=True)  # no arguments: it touches no device
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
