"""The noise estimate on the GPU (include/rt2.h "Noise estimate and render-until-converged") against a
reference built from the oracle's per-frame samples: a += s and q += s * s in float32 and frame order,
then the formulas in numpy float64 (tests/noise_ref.py). Every case is 40x24 pixels (960: not a multiple
of the kernels' 256-pixel workgroups), seed 0x5EED2024."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from bits import f32_bits
from conftest import ROOT, scene_path
from helpers import SEED
from noise_ref import noise_ref, scalars_ref, ss_unclamped

pytestmark = pytest.mark.gpu
W, H, SPP, FRAMES = 40, 24, 16, 13  # 13 frames: one whole octet and a partial one
SCENES = ["cornell_box_original", "cornell_box_volume", "final_render_book_1"]
NPIX = W * H
# Any two summation orders of N non-negative doubles differ by at most N * 2^-53 relative each from the
# exact sum, so by at most N * 2^-52 from one another.
SUM_TOL = NPIX * 2.0 ** -52
APP = os.path.join(ROOT, "raytrace2_amd", "lib", "rt2_headless")


ORACLE_FRAMES = {"cornell_box_original": 80}  # frames the cases need of each scene (others: FRAMES)


@functools.lru_cache(maxsize=None)
def _samples(name):
    """The oracle's per-frame samples (frames, H, W, 3) float32: each frame rendered into a zero accumulation."""
    from oracle.oracle import OracleScene
    o = OracleScene(scene_path(name), SEED)
    frames = ORACLE_FRAMES.get(name, FRAMES)
    out = np.zeros((frames, H, W, 3), np.float32)
    for f in range(frames):
        out[f], _, _ = o.render(W, H, SPP, 1, frame_begin=f, forward=True)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _sums(name, frames):
    """(a, q) float32 (H, W, 3) after `frames` frames, summed in frame order."""
    s = _samples(name)
    assert frames <= len(s)
    a, q = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
    for f in range(frames):
        a = a + s[f]
        q = q + s[f] * s[f]
    a.setflags(write=False)
    q.setflags(write=False)
    return a, q


def _tracer(name, *, moments=True, devices=None, band_h=0):
    import raytrace2_amd as R
    sc = R.Scene(scene_path(name), SEED)
    tr = R.RayTracer(sc, 0) if devices is None else R.RayTracer(sc, devices=devices, band_h=band_h)
    tr.set_seed(SEED)
    tr.SetSamplesPerPixel(SPP)
    tr.OnResize((W, H))
    if moments:
        tr.enable_moments()
    return sc, tr


def _within(value, ref, tol=SUM_TOL):
    return abs(value - ref) <= tol * abs(ref)


def _rms_ok(rms, ref_sum_sq, finite):
    """The float32 rms lies between the float32 roundings of the reference rms at the ends of the sum's
    tolerance (rounding is monotonic)."""
    lo = np.float32(np.sqrt(np.float64(ref_sum_sq) * (1 - SUM_TOL) / finite))
    hi = np.float32(np.sqrt(np.float64(ref_sum_sq) * (1 + SUM_TOL) / finite))
    return lo <= np.float32(rms) <= hi


def _safe_threshold(err, finite):
    """A float32 strictly between two adjacent distinct err values near the median of the distinct ones, so
    no last-bit difference can move a pixel across it."""
    u = np.unique(err[finite])
    mid = len(u) // 2
    for k in sorted(range(1, len(u)), key=lambda k: abs(k - mid)):
        t = np.float32((u[k - 1] + u[k]) / 2)
        if u[k - 1] < np.float64(t) < u[k]:
            return float(t)
    raise AssertionError("no float32 between adjacent err values")


def _render(tr, sc, pattern):
    if pattern == "launch8":
        tr.set_launch_frames(8)  # two launches (8 + 5 frames), one per launch slot
    if pattern == "updates":
        for _ in range(FRAMES):
            tr.Update(sc)
    else:
        tr.Render(FRAMES)


@pytest.mark.parametrize("pattern", ["render", "launch8", "updates", "partition"])
@pytest.mark.parametrize("name", SCENES)
def test_moments_are_bit_exact(have_gpu, name, pattern):
    from raytrace2_amd import local_rows
    a, q = _sums(name, FRAMES)
    rows = local_rows(H, 2, 1, 3) if pattern == "partition" else list(range(H))
    out = []
    for moments in (True, False):
        sc, tr = _tracer(name, moments=moments)
        if pattern == "partition":
            tr.set_partition(2, 1, 3)
        _render(tr, sc, pattern)
        assert tr.FrameIdx() == FRAMES
        out.append((tr.Accumulation(), tr.moments() if moments else None))
        tr.close()
    (acc_on, mom), (acc_off, _) = out
    assert acc_on.shape == (len(rows), W, 3)
    assert np.array_equal(f32_bits(mom), f32_bits(q[rows])), "moment2 differs from the oracle's frame-order sum"
    assert np.array_equal(f32_bits(acc_on), f32_bits(a[rows]))
    assert np.array_equal(f32_bits(acc_on), f32_bits(acc_off)), "moments changed the accumulation"


@pytest.mark.parametrize("name", SCENES)
def test_standard_error_is_bit_exact(have_gpu, name):
    a, q = _sums(name, FRAMES)
    sem, _, finite = noise_ref(a, q, FRAMES)
    assert finite.all()
    if name == "final_render_book_1":  # the clamp is exercised: channels whose ss rounds below zero
        neg = int((ss_unclamped(a, q, FRAMES) < 0).sum())
        print("book 1 channels with ss < 0:", neg)
        assert neg >= 1
    sc, tr = _tracer(name)
    tr.Render(FRAMES)
    got = tr.standard_error()
    again = tr.standard_error()
    tr.close()
    assert np.array_equal(f32_bits(got), f32_bits(sem))
    assert np.array_equal(f32_bits(got), f32_bits(again))


@pytest.mark.parametrize("name", SCENES)
def test_noise_scalars(have_gpu, name):
    import raytrace2_amd as R
    from raytrace2_amd._native import Noise
    a, q = _sums(name, FRAMES)
    _, err, finite = noise_ref(a, q, FRAMES)
    thr = _safe_threshold(err, finite)
    ref = scalars_ref(err, finite, thr)
    sc, tr = _tracer(name)
    tr.Render(FRAMES)
    n1, n2 = Noise(), Noise()
    R._native.check(R.lib.rt2_tracer_noise(tr._h, thr, ctypes.byref(n1)))
    R._native.check(R.lib.rt2_tracer_noise(tr._h, thr, ctypes.byref(n2)))
    got = tr.noise(thr)
    zero = tr.noise()
    tr.close()
    print(name, "threshold", thr, "product", got, "reference", ref)
    assert bytes(n1) == bytes(n2) and n1.as_dict() == got, "two calls in a row differ"
    assert got["frames"] == FRAMES
    assert (got["pixels"], got["below"], got["nonfinite"]) == (ref["pixels"], ref["below"], ref["nonfinite"])
    assert 0 < got["below"] < NPIX
    assert np.float32(got["max_err"]) == np.float32(ref["max_err"])
    assert _within(got["sum_sq"], ref["sum_sq"])
    assert _rms_ok(got["rms"], ref["sum_sq"], ref["pixels"] - ref["nonfinite"])
    # the default threshold 0 counts the pixels whose estimate is exactly 0
    assert zero["below"] == int((err[finite] == 0).sum()) and zero["sum_sq"] == got["sum_sq"]


def test_noise_errors(have_gpu):
    from raytrace2_amd import Rt2Error
    a, _ = _sums("cornell_box_original", FRAMES)
    sc, tr = _tracer("cornell_box_original", moments=False)
    tr.Render(3)
    for call in (tr.moments, tr.standard_error, tr.noise, lambda: tr.render_until(0.1, 16)):
        with pytest.raises(Rt2Error) as e:  # moments off
            call()
        assert e.value.code == -1
    assert tr.FrameIdx() == 3
    tr.enable_moments()
    assert tr.FrameIdx() == 0, "enable_moments resets the frame"
    tr.Update(sc)
    for call in (tr.standard_error, tr.noise):
        with pytest.raises(Rt2Error) as e:  # one frame: no variance estimate
            call()
        assert e.value.code == -1
    assert tr.moments().shape == (H, W, 3)
    tr.Render(FRAMES - 1)  # the tracer still renders
    assert tr.FrameIdx() == FRAMES
    assert np.array_equal(f32_bits(tr.Accumulation()), f32_bits(a))
    assert tr.noise()["frames"] == FRAMES
    tr.enable_moments(False)
    assert tr.FrameIdx() == 0
    with pytest.raises(Rt2Error):
        tr.moments()
    tr.close()


@functools.lru_cache(maxsize=None)
def _until_reference():
    """The oracle's rms after 16, 32 and 48 frames of the Cornell box and the target between the last two."""
    rms = {}
    for n in (16, 32, 48, 64):
        a, q = _sums("cornell_box_original", n)
        _, err, finite = noise_ref(a, q, n)
        rms[n] = scalars_ref(err, finite, 0.0)
    target = float(np.float32((rms[32]["rms"] + rms[48]["rms"]) / 2))
    print("oracle rms at 16, 32, 48 frames:", [rms[n]["rms"] for n in (16, 32, 48)], "target", target)
    assert rms[16]["rms"] > rms[32]["rms"] > 1.01 * target and rms[48]["rms"] < target / 1.01
    assert rms[64]["rms"] < target / 1.01
    return rms, target


def test_render_until_stops_at_the_target(have_gpu):
    rms, target = _until_reference()
    a48, _ = _sums("cornell_box_original", 48)
    sc, tr = _tracer("cornell_box_original")
    out = tr.render_until(target, 80)  # check_every 0: one sweep of the 4 x 4 strata = 16 frames
    print("render_until:", out)
    assert tr.FrameIdx() == 48 and out["frames"] == 48
    assert np.array_equal(f32_bits(tr.Accumulation()), f32_bits(a48))
    assert out["nonfinite"] == 0 and out["pixels"] == NPIX
    assert _within(out["sum_sq"], rms[48]["sum_sq"]) and _rms_ok(out["rms"], rms[48]["sum_sq"], NPIX)
    # an accumulation already begun is continued: the next sweep is checked at 64 frames, still converged
    again = tr.render_until(target, 80)
    assert tr.FrameIdx() == 64 and again["frames"] == 64 and again["rms"] <= target
    tr.close()


@pytest.mark.parametrize("max_frames", [80, 70])
def test_render_until_target_zero_runs_to_max_frames(have_gpu, max_frames):
    a, q = _sums("cornell_box_original", max_frames)
    _, err, finite = noise_ref(a, q, max_frames)
    ref = scalars_ref(err, finite, 0.0)
    sc, tr = _tracer("cornell_box_original")
    out = tr.render_until(0.0, max_frames)
    assert tr.FrameIdx() == max_frames and out["frames"] == max_frames  # 70: a shortened last step
    assert np.array_equal(f32_bits(tr.Accumulation()), f32_bits(a))
    assert np.array_equal(f32_bits(tr.moments()), f32_bits(q))
    assert _within(out["sum_sq"], ref["sum_sq"]) and out["rms"] > 0
    # min_frames above max_frames: no check on the way, the estimate of the final image
    tr.Reset()
    late = tr.render_until(1e9, 24, min_frames=100, check_every=5)
    assert tr.FrameIdx() == 24 and late["frames"] == 24
    # check_every: the first check at or after min_frames stops a target this loose
    tr.Reset()
    early = tr.render_until(1e9, 80, min_frames=7, check_every=3)
    assert tr.FrameIdx() == 9 and early["frames"] == 9
    tr.close()


def test_progressive_loop_stops_at_the_target(have_gpu):
    from raytrace2_amd.progressive import ProgressiveLoop
    _, target = _until_reference()
    sc, tr = _tracer("cornell_box_original", moments=False)
    with pytest.raises(ValueError):
        ProgressiveLoop(tr, 80, target_rms=target)
    tr.enable_moments()
    # a budget no tick reaches: the ticks double, 16 then 32 frames, and the check after 48 frames meets the target
    loop = ProgressiveLoop(tr, 80, budget_ms=1e9, first_frames=16, target_rms=target)
    loop.run()
    assert loop.done() and loop.converged and loop.frames_done == 48 and loop.ticks == 2
    assert loop.noise["frames"] == 48 and loop.noise["rms"] <= target
    loop.close()
    tr.close()


def test_multi_gpu_noise(have_gpu):
    from raytrace2_amd.dist import combine_noise
    name = "cornell_box_volume"
    a, q = _sums(name, FRAMES)
    sem, err, finite = noise_ref(a, q, FRAMES)
    thr = _safe_threshold(err, finite)
    ref = scalars_ref(err, finite, thr)
    sc, one = _tracer(name)
    one.Render(FRAMES)
    one_mom, one_sem, one_nz = one.moments(), one.standard_error(), one.noise(thr)
    one.close()
    sc, tr = _tracer(name, devices=[0, 0, 0], band_h=2)  # three partitions on one GPU
    tr.Render(FRAMES)
    mom, se, nz = tr.moments(), tr.standard_error(), tr.noise(thr)
    acc = tr.Accumulation()
    tr.close()
    assert mom.shape == (H, W, 3) and np.array_equal(f32_bits(mom), f32_bits(one_mom))
    assert np.array_equal(f32_bits(mom), f32_bits(q))
    assert np.array_equal(f32_bits(se), f32_bits(one_sem)) and np.array_equal(f32_bits(se), f32_bits(sem))
    assert np.array_equal(f32_bits(acc), f32_bits(a))
    for k in ("frames", "pixels", "below", "nonfinite", "max_err"):
        assert nz[k] == one_nz[k], k
    assert (nz["pixels"], nz["below"], nz["nonfinite"]) == (ref["pixels"], ref["below"], ref["nonfinite"])
    # the GPUs' partial sums are added in another order than one GPU's
    assert _within(nz["sum_sq"], one_nz["sum_sq"]) and _within(nz["sum_sq"], ref["sum_sq"])
    assert _rms_ok(nz["rms"], ref["sum_sq"], NPIX)
    # one tracer per partition, merged on the host: the multi-GPU tracer's own sums, in its order
    parts = []
    for r in range(3):
        sc, p = _tracer(name)
        p.set_partition(2, r, 3)
        p.Render(FRAMES)
        parts.append(p.noise(thr))
        assert parts[-1]["pixels"] == p.local_rows() * W
        p.close()
    assert combine_noise(parts) == nz


def test_headless_noise_target(have_gpu, tmp_path):
    import raytrace2_amd as R
    _, target = _until_reference()
    png, ref_png = str(tmp_path / "until.png"), str(tmp_path / "py.png")
    r = subprocess.run([APP, scene_path("cornell_box_original"), png, "--size", f"{W}x{H}", "--noise-target",
                        repr(target), "--max-samples", str(SPP)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"^frames (\d+) rms (\S+)$", r.stderr, re.M)
    assert m, r.stderr
    sc = R.Scene(scene_path("cornell_box_original"), R.DEFAULT_SEED)
    tr = R.RayTracer(sc, 0)
    tr.SetSamplesPerPixel(SPP)
    tr.OnResize((W, H))
    tr.enable_moments()
    out = tr.render_until(target, SPP)
    assert int(m.group(1)) == out["frames"] == tr.FrameIdx()
    assert np.float32(float(m.group(2))) == np.float32(out["rms"])
    R.WriteImage(tr.NonConvertedPixels(), W, H, ref_png)
    tr.close()
    assert open(png, "rb").read() == open(ref_png, "rb").read()
