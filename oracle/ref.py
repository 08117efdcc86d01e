"""ctypes front-end of the compiled reference (oracle/_ref/librt2_ref.so: the reference's own
src/cpu_raytrace behind oracle/refshim/ref_driver.cpp). TEST INFRASTRUCTURE ONLY.

The library exists only where the reference checkout does (oracle/Makefile, target ref): the CPU tests of
tests/test_reference_build.py and the fixture generator tests/golden/make_ref_golden.py load it; nothing that
runs on a GPU machine may.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "librt2_ref.so")
REFERENCE_DIR = os.environ.get("RT2_REFERENCE_DIR", "/root/reference")
FLT_MAX = 3.4028234663852886e38
_lib = None


def available() -> bool:
    return os.path.exists(LIB_PATH)


def checkout_present() -> bool:
    return os.path.isdir(os.path.join(REFERENCE_DIR, "src", "cpu_raytrace"))


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(LIB_PATH)
        vp, fp, u64, i32, u32 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32
        ip = ctypes.POINTER(ctypes.c_int)
        L.ref_last_error.restype = ctypes.c_char_p
        L.ref_scene_load.restype = vp
        L.ref_scene_load.argtypes = [ctypes.c_char_p, u64]
        L.ref_scene_free.argtypes = [vp]
        L.ref_scene_free.restype = None
        L.ref_scene_info.argtypes = [vp, ip, ip, i32]
        L.ref_uniforms.argtypes = [u64, u32, u32, i32, fp]
        L.ref_uniforms.restype = None
        L.ref_hit.argtypes = [vp, fp, fp, ctypes.c_float, ctypes.c_float, ctypes.c_float, u64, fp]
        L.ref_set_camera.argtypes = [vp, fp]
        L.ref_set_camera.restype = None
        L.ref_camera.argtypes = [vp, i32, i32, i32, fp]
        L.ref_render.argtypes = [vp, i32, i32, i32, i32, u64, i32, i32, fp, ctypes.POINTER(u64)]
        L.ref_perlin_probe.argtypes = [vp, i32, fp, i32, fp]
        _lib = L
    return _lib


def _f(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def uniforms(seed, pixel, frame, n):
    """The first n uniforms RandReal() returns on the path stream of (seed, pixel, frame)."""
    out = np.zeros(n, np.float32)
    lib().ref_uniforms(seed, pixel, frame, n, _f(out))
    return out


class RefScene:
    """A reference Scene built by ref_driver.cpp's loader from the reference's own constructors."""

    def __init__(self, path: str, seed: int = 0x5EED2024):
        self.path = path
        self.seed = seed
        self._h = lib().ref_scene_load(path.encode(), seed)
        if not self._h:
            raise RuntimeError(lib().ref_last_error().decode())

    def __del__(self):
        if getattr(self, "_h", None):
            lib().ref_scene_free(self._h)
            self._h = None

    def info(self):
        """(number of materials, list of texture kinds: 0 solid, 1 checker, 2 noise)."""
        nm = ctypes.c_int(0)
        kinds = (ctypes.c_int * 4096)()
        nt = lib().ref_scene_info(self._h, ctypes.byref(nm), kinds, 4096)
        return nm.value, list(kinds[:nt])

    def hit(self, o, d, time=0.0, tmin=0.001, tmax=FLT_MAX, seed=1):
        """hit, t, point(3), normal(3), front_face, material index, uv(2)."""
        o = np.asarray(o, np.float32)
        d = np.asarray(d, np.float32)
        out = np.zeros(12, np.float32)
        lib().ref_hit(self._h, _f(o), _f(d), time, tmin, tmax, seed, _f(out))
        return out

    def set_camera(self, center, look_at, view_up, vfov, defocus_angle, focus_distance) -> None:
        v = np.array(list(center) + list(look_at) + list(view_up) + [vfov, defocus_angle, focus_distance], np.float32)
        lib().ref_set_camera(self._h, _f(v))

    def camera_params(self, w: int, h: int, spp: int) -> np.ndarray:
        out = np.zeros(21, np.float32)
        lib().ref_camera(self._h, w, h, spp, _f(out))
        return out

    def render(self, w, h, spp_setting, frames, *, frame_begin=0, max_depth=50, seed=None, accum=None):
        """Frames [frame_begin, frame_begin + frames) of the reference's RayTracer::Update. Returns the
        accumulation (h, w, 3) and the number of uniforms consumed."""
        seed = self.seed if seed is None else seed
        if accum is None:
            accum = np.zeros((h, w, 3), np.float32)
        draws = ctypes.c_uint64(0)
        lib().ref_render(self._h, w, h, spp_setting, max_depth, seed, frame_begin, frames, _f(accum), ctypes.byref(draws))
        return accum, int(draws.value)

    def perlin_probe(self, tex: int, points) -> np.ndarray:
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        out = np.zeros_like(p)
        if lib().ref_perlin_probe(self._h, tex, _f(p), len(p), _f(out)) != 0:
            raise ValueError("not a noise texture")
        return out
