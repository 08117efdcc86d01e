"""The noise estimate on the host: the per-pixel function the GPU kernel runs (raytrace2_amd/csrc/noise.h,
built into the stand-alone tests/cpp/noise_host.cpp) against the formulas in numpy float64, the new entry
points' argument checks, and the host merge of per-GPU noise scalars. No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import host_build as H
import raytrace2_amd as R
from conftest import ROOT
from noise_ref import noise_ref, ss_unclamped
from raytrace2_amd._native import Noise
from raytrace2_amd.dist import combine_noise



def _build(sanitize):
    return H.program("noise_host.cpp", [*H.HOST, *(H.HOST_SAN if sanitize else ())])


def _run(exe, tmp_path, a, q, n):
    """NoiseOfPixel over cases a, q (k, 3) float32 with frame counts n (k): sem bits, err bits, finite."""
    a, q = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(q, np.float32)
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for i in range(len(a)):
            f.write(f"{int(n[i])} " + " ".join(f"{w:08x}" for w in np.concatenate([a[i], q[i]]).view(np.uint32)) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [l.split() for l in r.stdout.splitlines()]
    assert len(rows) == len(a)
    sem = np.array([[int(x, 16) for x in row[:3]] for row in rows], np.uint32)
    err = np.array([int(row[3], 16) for row in rows], np.uint64)
    fin = np.array([row[4] == "1" for row in rows])
    return sem, err, fin


def _cases():
    rng = np.random.default_rng(7)
    below3 = np.nextafter(np.float32(3), np.float32(0))
    a = [[3, 3, 3],            # 0: q just below a^2 / n: ss rounds below zero -> sem 0
         [30, 30, 30],         # 1: mean 10 > 1: err is divided by it
         [0.3, 0.3, 0.3],      # 2: the same relative spread at mean 0.1: no division
         [np.nan, 1, 1],       # 3..6: non-finite sums
         [1, np.inf, 1], [1, 1, 1], [1, 1, 1],
         [0, 0, 0]]            # 7: a black pixel
    q = [[below3, below3, below3], [400, 400, 400], [0.04, 0.04, 0.04], [1, 1, 1], [1, 1, 1], [1, 1, np.nan],
         [-np.inf, 1, 1], [0, 0, 0]]
    n = [3, 3, 3, 5, 5, 5, 5, 13]
    # random sums of n samples in [0, 4) and of their squares, in float32 and frame order like the kernel's
    for _ in range(64):
        k = int(rng.integers(2, 200))
        s = (rng.random((k, 3), np.float32) * np.float32(4.0) * (rng.random(3) < 0.8)).astype(np.float32)
        acc, sq = np.zeros(3, np.float32), np.zeros(3, np.float32)
        for f in range(k):
            acc = acc + s[f]
            sq = sq + s[f] * s[f]
        a.append(acc)
        q.append(sq)
        n.append(k)
    # equal samples: ss is pure rounding noise, on either side of zero
    for v in (0.1, 0.7, 1.3, 0.73, 2.9):
        k = 13
        acc, sq = np.float32(0), np.float32(0)
        for f in range(k):
            acc = acc + np.float32(v)
            sq = sq + np.float32(v) * np.float32(v)
        a.append([acc] * 3)
        q.append([sq] * 3)
        n.append(k)
    return np.array(a, np.float32), np.array(q, np.float32), np.array(n)


@pytest.mark.parametrize("sanitize", [False, True])
def test_pixel_noise_matches_the_formulas_bit_for_bit(tmp_path, sanitize):
    """tests/cpp/noise_host.cpp over noise.h, plain and with the host sanitizers (a stand-alone program)."""
    exe = _build(sanitize)
    a, q, n = _cases()
    sem, err, fin = _run(exe, tmp_path, a, q, n)
    ref = [noise_ref(a[i], q[i], n[i]) for i in range(len(a))]
    r_sem = np.array([r[0] for r in ref], np.float32)
    r_err = np.array([r[1] for r in ref], np.float64)
    r_fin = np.array([r[2] for r in ref])
    assert np.array_equal(fin, r_fin)
    assert np.array_equal(sem, r_sem.view(np.uint32))
    assert np.array_equal(err, r_err.view(np.uint64))
    f32 = sem.view(np.float32)
    f64 = err.view(np.float64)
    # 0: ss below zero clamps to a standard error of exactly +0
    assert (ss_unclamped(a[0], q[0], n[0]) < 0).all() and (sem[0] == 0).all() and err[0] == 0
    # some equal-sample case lands below zero too (rounding noise), and all of them give sem 0 or tiny
    assert any((ss_unclamped(a[i], q[i], n[i]) < 0).any() for i in range(len(a) - 5, len(a)))
    # 1, 2: mean 10 divides by 10, mean 0.1 by 1
    s1 = np.float64(np.float32(np.sqrt(np.float64(100) / 6)))
    assert f64[1] == np.sqrt((s1 * s1 + s1 * s1 + s1 * s1) / 3.0) / np.float64(10.0)
    assert abs(f64[2] - float(f32[2, 0])) <= 1e-15 and f64[2] > 0
    # 3..6: NaN or inf in a or q: +inf, counted as non-finite
    assert not fin[3:7].any() and (sem[3:7] == 0x7F800000).all() and np.isposinf(f64[3:7]).all()
    # 7: black
    assert fin[7] and (sem[7] == 0).all() and err[7] == 0


def test_null_arguments_return_invalid():
    n = Noise()
    buf = (ctypes.c_float * 3)()
    L = R.lib
    assert L.rt2_tracer_enable_moments(None, 1) == R._native.RT2_ERR_INVALID
    assert L.rt2_tracer_moments(None, buf) == -1
    assert L.rt2_tracer_standard_error(None, buf) == -1
    assert L.rt2_tracer_noise(None, 0.0, ctypes.byref(n)) == -1
    assert L.rt2_tracer_render_until(None, 0.1, 0, 16, 0, ctypes.byref(n)) == -1
    assert b"null" in L.rt2_last_error()


def test_cpp_mirror_noise_members_compile():
    """include/rt2/RayTracer.hpp: EnableMoments, Moments, StandardError, Noise, RenderUntil."""
    H.syntax_only("mirror_noise.cpp")


def test_noise_struct_matches_the_header(tmp_path):
    """rt2_noise (include/rt2.h) and its ctypes mirror agree on size and offsets (gcc lays out the C one)."""
    fields = [f for f, _ in Noise._fields_]
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "rt2.h"\nint main(void) {\n'
           '  printf("%zu", sizeof(rt2_noise));\n'
           + "".join(f'  printf(" %zu", offsetof(rt2_noise, {f}));\n' for f in fields) + "  return 0;\n}\n")
    c, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(c, "w").write(src)
    b = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(Noise)] + [getattr(Noise, f).offset for f in fields]


def test_combine_noise_merges_like_the_multi_gpu_tracer():
    parts = [{"frames": 13, "pixels": 320, "below": 100, "nonfinite": 0, "sum_sq": 1.25, "max_err": 0.5, "rms": 0.0625},
             {"frames": 13, "pixels": 320, "below": 7, "nonfinite": 2, "sum_sq": 0.1, "max_err": 0.75, "rms": 0.1},
             {"frames": 13, "pixels": 320, "below": 0, "nonfinite": 0, "sum_sq": 0.2, "max_err": 0.25, "rms": 0.2}]
    c = combine_noise(parts)
    assert (c["frames"], c["pixels"], c["below"], c["nonfinite"]) == (13, 960, 107, 2)
    assert c["sum_sq"] == (1.25 + 0.1) + 0.2 and c["max_err"] == 0.75
    assert c["rms"] == float(np.float32(np.sqrt(np.float64(c["sum_sq"]) / 958)))
    assert combine_noise(parts[:1]) == {**parts[0], "rms": float(np.float32(np.sqrt(np.float64(1.25) / 320)))}
    # no finite pixel: rms 0
    z = combine_noise([{"frames": 2, "pixels": 4, "below": 0, "nonfinite": 4, "sum_sq": 0.0, "max_err": 0.0, "rms": 0.0}])
    assert z["rms"] == 0.0 and z["nonfinite"] == 4
    with pytest.raises(ValueError):
        combine_noise([parts[0], {**parts[1], "frames": 14}])
    with pytest.raises(ValueError):
        combine_noise([])
