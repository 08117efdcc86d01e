"""Reconstructing the gathered image on the host (include/rt2.h "Reconstructing the gathered image"):
rt2_deinterleave_estimate_host, the CPU statement of gather_estimate()'s kernel, against rt2_deinterleave_host and
the noise estimate's numpy formulas bit for bit, its argument checks, and the C++ mirror's new members. No GPU."""
import ctypes

import numpy as np
import pytest

import host_build as H
import raytrace2_amd as R
from bits import f32_bits
from denoise_ref import variance_of_sem
from noise_ref import noise_ref
from raytrace2_amd.dist import band_rows_max, deinterleave, deinterleave_estimate, source_rows

F32 = np.float32
FRAMES = 16
# (width, height, world, band_h): 33x10 over 4 ranks in bands of 8 leaves ranks 2 and 3 without a row and rank 1
# with padding rows; 1x45 is one pixel per row
LAYOUTS = [(50, 45, 2, 8), (50, 45, 3, 5), (50, 45, 4, 1), (50, 45, 8, 16), (33, 10, 4, 8), (1, 45, 3, 5)]


def _stacks(w, h, world, band_h, seed):
    """Band stacks of sums and sums of squares over FRAMES frames, (world, max_rows, w, 3) float32: random sums
    of samples in [0, 4) in frame order like the kernel's, then whole image rows of NaN, +-inf and zeros (a row of
    the image is a row of the stacks; the padding rows are never read)."""
    rng = np.random.default_rng(seed)
    rows = band_rows_max(h, band_h, world)
    shape = (world, rows, w, 3)
    acc, sq = np.zeros(shape, F32), np.zeros(shape, F32)
    for _ in range(FRAMES):
        s = (rng.random(shape, F32) * F32(4.0)).astype(F32)
        acc = acc + s
        sq = sq + s * s
    flat_a, flat_q = acc.reshape(world * rows, w, 3), sq.reshape(world * rows, w, 3)
    picks = source_rows(h, band_h, world)[rng.permutation(h)[:5]]  # stack rows of five image rows
    flat_a[picks[0]] = np.nan
    flat_q[picks[1]] = np.inf
    flat_a[picks[2]] = -np.inf
    flat_a[picks[3]] = 0
    flat_q[picks[3]] = 0
    flat_q[picks[4]] = 0  # squares below a^2 / n: the clamp
    return acc, sq


@pytest.mark.parametrize("w,h,world,band_h", LAYOUTS)
def test_deinterleave_estimate_host_matches_numpy(w, h, world, band_h):
    acc, sq = _stacks(w, h, world, band_h, seed=w * 1000 + world)
    image, mean, var = deinterleave_estimate(acc, sq, h, band_h, FRAMES)
    assert image.shape == mean.shape == (h, w, 3) and var.shape == (h, w)
    ref_a, ref_q = deinterleave(acc, h, band_h), deinterleave(sq, h, band_h)
    assert np.array_equal(f32_bits(image), f32_bits(ref_a))
    with np.errstate(all="ignore"):
        assert np.array_equal(f32_bits(mean), f32_bits(ref_a / F32(FRAMES)))
    sem, _, finite = noise_ref(ref_a, ref_q, FRAMES)
    assert np.array_equal(f32_bits(var), f32_bits(variance_of_sem(sem)))
    # the data reaches the cases it is meant to: non-finite pixels (variance +inf), clamped and ordinary ones
    if w * h >= 330:
        assert (~finite).any() and np.isinf(var[~finite]).all() and np.isfinite(var[finite]).all()
        assert (var[finite] == 0).any() and (var[finite] > 0).any()


def test_deinterleave_estimate_host_argument_checks():
    fp = ctypes.POINTER(ctypes.c_float)
    buf = (ctypes.c_float * 64)()
    call = R.lib.rt2_deinterleave_estimate_host
    assert call(buf, buf, buf, buf, buf, 2, 2, 1, 2, 16) == 0
    assert call(None, buf, buf, buf, buf, 2, 2, 1, 2, 16) == -1
    assert call(buf, None, buf, buf, buf, 2, 2, 1, 2, 16) == -1
    assert call(buf, buf, buf, buf, ctypes.cast(None, fp), 2, 2, 1, 2, 16) == -1
    assert call(buf, buf, buf, buf, buf, -1, 2, 1, 2, 16) == -1
    assert call(buf, buf, buf, buf, buf, 2, 2, -1, 2, 16) == -1
    assert call(buf, buf, buf, buf, buf, 2, 2, 1, 0, 16) == -1
    assert call(buf, buf, buf, buf, buf, 2, 2, 1, 2, 1) == -1, "an estimate needs two frames"
    assert call(buf, buf, buf, buf, buf, 2, 2, 1, 2, 1 << 31) == -1
    with pytest.raises(ValueError):
        deinterleave_estimate(np.zeros((2, 3, 4, 3), F32), np.zeros((2, 3, 4, 3), F32), 4, 1, 16)  # max_rows is 2


def test_new_entry_points_refuse_null_tracers():
    lib = R.lib
    assert lib.rt2_tracer_gather_estimate(None) == -1
    assert lib.rt2_tracer_image_variance(None, None) == -1
    assert lib.rt2_tracer_image_features(None, None) == -1
    assert lib.rt2_tracer_image_resolve(None, None, None, None, None) == -1
    assert lib.rt2_tracer_image_present_async(None, None, None) == -1
    assert lib.rt2_tracer_image_present(None, None, None) == -1
    assert lib.rt2_tracer_image_move_camera(None, None, None) == -1
    assert lib.rt2_tracer_image_present_time(None, None) == -1


def test_cpp_mirror_image_reconstruct_members_compile():
    """include/rt2/RayTracer.hpp: GatherEstimate, ImageVariance, ImageFeatures, ImageResolve, ImagePresentAsync,
    ImagePresent, ImageMoveCamera, ImagePresentTime."""
    H.syntax_only("mirror_image_reconstruct.cpp")
