"""Adaptive sampling of the gathered image on the host (include/rt2.h "Adaptive sampling of the gathered image"):
rt2_deinterleave_adaptive_host, the CPU statement of the gather's kernel when the sample counts travel with it,
against a numpy restatement (assemble_bands, the noise estimate per sample count, the float32 divide), its argument
checks, the ctypes signatures of the new entry points and the C++ mirror's new members. No GPU."""
import ctypes

import numpy as np
import pytest

import host_build as H
import raytrace2_amd as R
from adaptive_ref import pixel_noise
from denoise_ref import variance_of_sem
from raytrace2_amd._native import Adaptive
from raytrace2_amd.dist import band_rows_max, deinterleave_adaptive

F32 = np.float32
# (width, height, world, band_h): 33x10 in single rows over 4 ranks gives stacks of 3, 3, 2, 2 rows; 40x24 over
# (5, 2) stacks of 4, 4, 6, 6, 4 rows and over (2, 5) 14 rows against 10: every layout sends padding rows
LAYOUTS = [(33, 10, 4, 1), (40, 24, 5, 2), (40, 24, 2, 5)]


def _same_or_both_nan(got, ref):
    """Bit for bit, but for the payload of a NaN (0 / 0 at a pixel without a sample): NaN where the other is."""
    got, ref = np.ascontiguousarray(got, F32), np.ascontiguousarray(ref, F32)
    return got.shape == ref.shape and bool(np.all((got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))))


def _stacks(w, h, world, band_h, seed):
    """Padded band stacks (world, max_rows, w[, 3]): per pixel a count in [0, 80] and the frame-order float32 sums
    of that many samples in [0, 4) and of their squares; the padding rows hold other values, which must not show."""
    rng = np.random.default_rng(seed)
    rows = band_rows_max(h, band_h, world)
    n = rng.integers(0, 81, (world, rows, w)).astype(np.uint32)
    acc, sq = np.zeros((world, rows, w, 3), F32), np.zeros((world, rows, w, 3), F32)
    for f in range(80):
        s = (rng.random(acc.shape, F32) * F32(4.0)).astype(F32)
        live = (f < n)[..., None]
        acc = np.where(live, acc + s, acc)
        sq = np.where(live, sq + s * s, sq)
    for r in range(world):
        own = len(R.local_rows(h, band_h, r, world))
        acc[r, own:], sq[r, own:], n[r, own:] = F32(-7.0), F32(-3.0), 12345
    return acc, sq, n


def _reference(acc, sq, n, h, band_h):
    a = R.assemble_bands(list(acc), h, band_h)
    q = R.assemble_bands(list(sq), h, band_h)
    cnt = R.assemble_bands(list(n[..., None]), h, band_h)[..., 0]
    with np.errstate(all="ignore"):
        mean = a / cnt.astype(F32)[..., None]
        sem, _, _ = pixel_noise(a, q, cnt)
        var = variance_of_sem(sem)
    return a, mean, var, cnt


@pytest.mark.parametrize("squares", [True, False])
@pytest.mark.parametrize("w,h,world,band_h", LAYOUTS)
def test_deinterleave_adaptive_host_matches_numpy(w, h, world, band_h, squares):
    acc, sq, n = _stacks(w, h, world, band_h, seed=w * 100 + world)
    ref_a, ref_mean, ref_var, ref_n = _reference(acc, sq, n, h, band_h)
    assert {0, 1}.issubset(set(np.unique(ref_n))) and ref_n.max() <= 80 and len(np.unique(ref_n)) > 40
    image, mean, var, cnt = deinterleave_adaptive(acc, sq if squares else None, n, h, band_h)
    assert np.array_equal(cnt, ref_n) and cnt.dtype == np.uint32
    assert np.array_equal(image.view(np.uint32), ref_a.view(np.uint32))
    assert _same_or_both_nan(mean, ref_mean)
    assert np.isfinite(mean[ref_n > 0]).all(), "no padding value came through"
    if squares:
        assert var.shape == (h, w) and _same_or_both_nan(var, ref_var)
        ok = ref_n >= 2
        assert np.isfinite(var[ok]).all() and (var[ok] > 0).any()
    else:
        assert var is None


def test_deinterleave_adaptive_host_argument_checks():
    fp, u32 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    buf, cnt = (ctypes.c_float * 64)(), (ctypes.c_uint32 * 64)()
    call = R.lib.rt2_deinterleave_adaptive_host
    null_f, null_u = ctypes.cast(None, fp), ctypes.cast(None, u32)
    assert call(buf, buf, cnt, buf, buf, buf, cnt, 2, 2, 1, 2) == 0
    assert call(buf, null_f, cnt, buf, buf, null_f, cnt, 2, 2, 1, 2) == 0  # without squares
    assert call(null_f, buf, cnt, buf, buf, buf, cnt, 2, 2, 1, 2) == -1
    assert call(buf, buf, null_u, buf, buf, buf, cnt, 2, 2, 1, 2) == -1
    assert call(buf, buf, cnt, null_f, buf, buf, cnt, 2, 2, 1, 2) == -1
    assert call(buf, buf, cnt, buf, null_f, buf, cnt, 2, 2, 1, 2) == -1
    assert call(buf, buf, cnt, buf, buf, buf, null_u, 2, 2, 1, 2) == -1
    assert call(buf, null_f, cnt, buf, buf, buf, cnt, 2, 2, 1, 2) == -1, "squares and variance come together"
    assert call(buf, buf, cnt, buf, buf, null_f, cnt, 2, 2, 1, 2) == -1
    assert call(buf, buf, cnt, buf, buf, buf, cnt, -1, 2, 1, 2) == -1
    assert call(buf, buf, cnt, buf, buf, buf, cnt, 2, -1, 1, 2) == -1
    assert call(buf, buf, cnt, buf, buf, buf, cnt, 2, 2, -1, 2) == -1
    assert call(buf, buf, cnt, buf, buf, buf, cnt, 2, 2, 1, 0) == -1
    with pytest.raises(ValueError):  # max_rows is 2
        deinterleave_adaptive(np.zeros((2, 3, 4, 3), F32), None, np.zeros((2, 3, 4), np.uint32), 4, 1)


def test_new_entry_points_refuse_null_tracers():
    lib = R.lib
    a = Adaptive()
    buf = (ctypes.c_uint32 * 4)()
    assert lib.rt2_tracer_image_enable_adaptive(None, 1) == -1
    assert lib.rt2_tracer_image_adaptive_check(None, 0.1, 1, ctypes.byref(a)) == -1
    assert lib.rt2_tracer_image_render_adaptive(None, 0.1, 1, 0, 16, 0, ctypes.byref(a)) == -1
    assert lib.rt2_tracer_image_part_adaptive(None, 0, ctypes.byref(a)) == -1
    assert lib.rt2_tracer_image_sample_counts(None, buf) == -1
    assert b"null" in lib.rt2_last_error()


def test_python_bindings_argument_types():
    lib = R.lib
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    fp, u32, ad = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(Adaptive)
    expect = {"rt2_tracer_image_enable_adaptive": [vp, i32],
              "rt2_tracer_image_adaptive_check": [vp, f32, i32, ad],
              "rt2_tracer_image_render_adaptive": [vp, f32, i32, i32, i32, i32, ad],
              "rt2_tracer_image_part_adaptive": [vp, i32, ad],
              "rt2_tracer_image_sample_counts": [vp, u32],
              "rt2_deinterleave_adaptive_host": [fp, fp, u32, fp, fp, fp, u32, i32, i32, i32, i32]}
    declared = R.declared_symbols()
    for name, args in expect.items():
        fn = getattr(lib, name)
        assert name in declared and fn.restype is i32 and list(fn.argtypes) == args, name
    # the same argument order as adaptive_check / render_adaptive
    assert list(lib.rt2_tracer_image_adaptive_check.argtypes) == list(lib.rt2_tracer_adaptive_check.argtypes)
    assert list(lib.rt2_tracer_image_render_adaptive.argtypes) == list(lib.rt2_tracer_render_adaptive.argtypes)
    for method in ("image_enable_adaptive", "image_adaptive_check", "image_render_adaptive", "image_sample_counts",
                   "image_part_adaptive"):
        assert callable(getattr(R.RayTracer, method))


def test_cpp_mirror_image_adaptive_members_compile():
    """include/rt2/RayTracer.hpp: ImageEnableAdaptive, ImageAdaptiveCheck, ImageRenderAdaptive, ImageSampleCounts."""
    H.syntax_only("mirror_image_adaptive.cpp")
