"""The variance-guided a-trous filter on the host: the shared header the GPU kernels run
(raytrace2_amd/csrc/denoise.h, built into the stand-alone tests/cpp/denoise_host.cpp) against its numpy float32
statement (tests/denoise_ref.py) bit for bit, each degenerate case the header names, the quality check and the
mirrored control on the numpy statement with the oracle's images, and the new entry points' argument checks.
No GPU."""
import ctypes
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import host_build as H
import raytrace2_amd as R
from bits import same_bits
from conftest import ROOT, scene_path
from denoise_ref import DEFAULTS, FEATURE_FLOATS, denoise_ref, features_ref, params, synthetic_case, variance_of_sem
from helpers import SEED, rmse
from noise_ref import noise_ref
from raytrace2_amd._native import DenoiseParams

F32 = np.float32
SIZES = [(1, 1), (1, 9), (9, 1), (33, 9), (70, 37)]


def _exe(sanitize):
    return H.program("denoise_host.cpp", [*H.HOST, *(H.HOST_SAN if sanitize else ())])


def _run(exe, tmp_path, c, v, f, **kw):
    k = params(**kw)
    h, w = v.shape
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<4i4f", w, h, k["iterations"], k["normal_power_log2"], k["sigma_l"], k["sigma_p"],
                             k["sigma_a"], k["eps_l"]))
        for a in (c, v, f):
            fh.write(np.ascontiguousarray(a, F32).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = np.fromfile(dst, F32)
    assert out.size == 4 * w * h
    return out[:3 * w * h].reshape(h, w, 3), out[3 * w * h:].reshape(h, w)


@pytest.mark.parametrize("sanitize", [False, True])
def test_host_program_matches_numpy_bit_for_bit(tmp_path, sanitize):
    """Every size and iteration count of the GPU test; the sanitized build is its own program."""
    exe = _exe(sanitize)
    for (w, h) in SIZES:
        c, v, f = synthetic_case(w, h)
        for it in ((1, 3, 5, 8) if not sanitize else (5,)):
            rc, rv = denoise_ref(c, v, f, iterations=it)
            gc, gv = _run(exe, tmp_path, c, v, f, iterations=it)
            assert same_bits(gc, rc) and same_bits(gv, rv), (w, h, it)
    # other parameters than the defaults
    c, v, f = synthetic_case(33, 9, seed=5)
    kw = dict(iterations=2, normal_power_log2=0, sigma_l=0.5, sigma_p=0.25, sigma_a=2.0, eps_l=0.125)
    rc, rv = denoise_ref(c, v, f, **kw)
    gc, gv = _run(exe, tmp_path, c, v, f, **kw)
    assert same_bits(gc, rc) and same_bits(gv, rv)


def test_synthetic_case_reaches_the_branches():
    c, v, f = synthetic_case(70, 37)
    hit = f[..., 0]
    assert (hit == 0).any() and (hit == 1).any()
    assert np.isnan(c).any() and np.isinf(v).any() and (v < 0).any() and (v == 0).any()
    assert ((f[..., 13] == 0) & (hit == 1)).sum() == 1
    rc, rv = denoise_ref(c, v, f)
    fin = np.isfinite(c).all(-1) & np.isfinite(v)
    # no finite input gives a NaN or an inf; the others pass through bit for bit
    assert np.isfinite(rc[fin]).all() and np.isfinite(rv[fin]).all()
    assert same_bits(rc[~fin], c[~fin]) and same_bits(rv[~fin], v[~fin])
    # the filter does something, and the noisy region's variance shrinks
    assert (rc[fin] != c[fin]).any()
    noisy = fin & (v == F32(1.5))
    assert (rv[noisy] < v[noisy]).all()
    # the flat zero-variance region stays what it was where it has only its own kind within reach of step 1
    one, _ = denoise_ref(c, v, f, iterations=1)
    assert np.isfinite(one[fin]).all()


def _flat(w, h, value=0.5, var=0.01):
    c = np.full((h, w, 3), value, F32)
    v = np.full((h, w), var, F32)
    f = np.zeros((h, w, FEATURE_FLOATS), F32)
    f[..., 0] = 1
    f[..., 2:5] = [0, 0, 4]
    f[..., 5:8] = [0, 0, 1]
    f[..., 10:13] = 0.5
    f[..., 13] = 4
    return c, v, f


def test_degenerate_cases(tmp_path):
    exe = _exe(False)

    def both(c, v, f, **kw):
        rc, rv = denoise_ref(c, v, f, **kw)
        gc, gv = _run(exe, tmp_path, c, v, f, **kw)
        assert same_bits(gc, rc) and same_bits(gv, rv)
        return rc, rv

    # every neighbour rejected (perpendicular normals all round): the centre comes back bit for bit,
    # although (h * c) / h alone would not round back (0.1 * 9/64 / (9/64) != 0.1 in float32 is possible)
    c, v, f = _flat(5, 5)
    rng = np.random.default_rng(3)
    c[:] = rng.random((5, 5, 3), F32)
    v[:] = rng.random((5, 5), F32)
    f[..., 5:8] = [1, 0, 0]
    f[2, 2, 5:8] = [0, 0, 1]
    rc, rv = both(c, v, f, iterations=2)
    assert same_bits(rc[2, 2], c[2, 2]) and same_bits(rv[2, 2], v[2, 2])
    # ... and with every neighbour a miss or not finite
    c2, v2, f2 = c.copy(), v.copy(), f.copy()
    f2[..., 5:8] = [0, 0, 1]
    f2[..., 0] = 0
    f2[2, 2, 0] = 1
    c2[2, 3] = np.nan
    rc, rv = both(c2, v2, f2, iterations=3)
    assert same_bits(rc[2, 2], c2[2, 2]) and same_bits(rv[2, 2], v2[2, 2])
    # a 1x1 image: nothing to average
    rc, rv = both(c[:1, :1], v[:1, :1], f[:1, :1], iterations=8)
    assert same_bits(rc, c[:1, :1]) and same_bits(rv, v[:1, :1])
    # dist == 0: wp = 1, no 0 / 0; with equal colours everywhere the image stays finite and equal
    c, v, f = _flat(6, 4)
    f[..., 13] = 0
    rc, rv = both(c, v, f)
    assert np.isfinite(rc).all() and np.isfinite(rv).all() and (np.abs(rc - c) <= 1e-6).all()
    # variance 0 everywhere: the tolerance is eps_l; a step edge far above it is kept, to the bit at the edge
    c, v, f = _flat(8, 4, var=0.0)
    c[:, 4:] = 0.9
    rc, rv = both(c, v, f)
    assert np.isfinite(rc).all() and (rv == 0).all()
    assert (np.abs(rc - c) <= 1e-4).all()
    # a negative variance counts as 0 under the square root
    v[:] = -1.0
    rc, rv = both(c, v, f)
    assert np.isfinite(rc).all() and np.isfinite(rv).all()
    # non-finite pixels pass through in every pass and reach no neighbour
    c, v, f = _flat(7, 5)
    c[2, 3] = [np.inf, 0.5, 0.5]
    v[1, 1] = np.nan
    rc, rv = both(c, v, f, iterations=4)
    fin = np.isfinite(c).all(-1) & np.isfinite(v)
    assert np.isfinite(rc[fin]).all() and np.isfinite(rv[fin]).all()
    assert same_bits(rc[~fin], c[~fin]) and same_bits(rv[~fin], v[~fin])
    # huge finite colours whose luminances overflow: the luminance weight is 0, no NaN
    c, v, f = _flat(4, 3)
    c[1, 1] = 3e38
    c[1, 2] = 3e38
    rc, rv = both(c, v, f, iterations=1)
    assert not np.isnan(rc).any() and not np.isnan(rv).any()


# ---- quality on the oracle's images (numpy statement alone) -------------------------------------------------
QW, QH, QSPP, QFRAMES, QREF = 70, 37, 16, 16, 1024


@functools.lru_cache(maxsize=None)
def _quality_inputs(name):
    """(c, v, features, reference): the oracle's first 16 frames (samples and squares summed in frame order),
    the features from oracle.hit on the centre rays, and the oracle's 1024-frame mean at another seed."""
    from oracle.oracle import OracleScene
    o = OracleScene(scene_path(name), SEED)
    a, q = np.zeros((QH, QW, 3), F32), np.zeros((QH, QW, 3), F32)
    for fr in range(QFRAMES):
        s, _, _ = o.render(QW, QH, QSPP, 1, frame_begin=fr, forward=True)
        a = a + s
        q = q + s * s
    c = a / F32(QFRAMES)
    sem, _, _ = noise_ref(a, q, QFRAMES)
    feat, flagged = features_ref(o, o.camera_params(QW, QH, QSPP), QW, QH, SEED)
    assert not flagged.any()
    ref, _, _ = OracleScene(scene_path(name), SEED + 1).render(QW, QH, QSPP, QREF, forward=True)
    return c, variance_of_sem(sem), feat, ref / F32(QREF)


@pytest.mark.parametrize("name", ["cornell_box_original", "final_render_book_1", "cornell_box_volume"])
def test_denoised_image_is_closer_to_the_converged_one(name):
    """At the defaults the denoised 16-frame image has a lower RMSE against a 1024-frame render at another
    seed than the 16-frame image itself (measured ratios: DESIGN.md §6e)."""
    c, v, feat, ref = _quality_inputs(name)
    dc, dv = denoise_ref(c, v, feat)
    noisy, den = rmse(c, ref), rmse(dc, ref)
    print(f"{name}: rmse 16 frames {noisy:.5f}, denoised {den:.5f}, ratio {den / noisy:.4f}")
    assert np.isfinite(dc).all() and np.isfinite(dv).all()
    assert den < noisy


def test_mirrored_features_score_worse_on_cornell():
    """The control: the same filter guided by the feature image flipped left to right does worse."""
    c, v, feat, ref = _quality_inputs("cornell_box_original")
    good, _ = denoise_ref(c, v, feat)
    bad, _ = denoise_ref(c, v, np.ascontiguousarray(feat[:, ::-1]))
    g, b = rmse(good, ref), rmse(bad, ref)
    print(f"cornell_box_original: rmse with the features {g:.6f}, with them mirrored {b:.6f}")
    assert b > g


# ---- the public surface without a GPU ------------------------------------------------------------------------
def test_defaults_match_the_reference_statement():
    d = R.denoise_defaults()
    assert d["iterations"] == DEFAULTS["iterations"] and d["normal_power_log2"] == DEFAULTS["normal_power_log2"]
    for k in ("sigma_l", "sigma_p", "sigma_a", "eps_l"):
        assert d[k] == float(F32(DEFAULTS[k]))


def test_argument_checks_return_invalid():
    L = R.lib
    buf = (ctypes.c_float * 16)()
    assert L.rt2_tracer_features(None, buf) == -1
    assert L.rt2_tracer_denoise(None, None, buf, None) == -1
    assert L.rt2_tracer_denoise_times(None, None, None) == -1
    assert L.rt2_denoise_buffers(0, 1, 1, None, buf, buf, None, buf, buf) == -1
    assert L.rt2_denoise_buffers(0, 1, 1, buf, buf, buf, None, None, buf) == -1
    assert b"null" in L.rt2_last_error()
    assert L.rt2_denoise_buffers(0, 0, 1, buf, buf, buf, None, buf, buf) == -1
    for field, bad in [("iterations", 0), ("iterations", 9), ("normal_power_log2", -1), ("normal_power_log2", 9),
                       ("sigma_l", 0.0), ("sigma_p", float("nan")), ("sigma_a", float("inf")), ("eps_l", -1.0)]:
        p = DenoiseParams()
        L.rt2_denoise_defaults(ctypes.byref(p))
        setattr(p, field, bad)
        assert L.rt2_denoise_buffers(0, 1, 1, buf, buf, buf, ctypes.byref(p), buf, buf) == -1, (field, bad)
        assert b"denoise" in L.rt2_last_error()
    with pytest.raises(TypeError):
        R.denoise_buffers(np.zeros((1, 1, 3), F32), np.zeros((1, 1), F32), np.zeros((1, 1, 16), F32), sigma=1)
    with pytest.raises(ValueError):
        R.denoise_buffers(np.zeros((1, 2, 3), F32), np.zeros((1, 1), F32), np.zeros((1, 1, 16), F32))


def test_cpp_mirror_denoise_members_compile():
    """include/rt2/RayTracer.hpp: DenoiseDefaults, Features, Denoise."""
    H.syntax_only("mirror_denoise.cpp")


def test_params_struct_matches_the_header(tmp_path):
    """rt2_denoise_params (include/rt2.h) and its ctypes mirror agree on size and offsets."""
    fields = [f for f, _ in DenoiseParams._fields_]
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "rt2.h"\nint main(void) {\n'
           '  printf("%zu", sizeof(rt2_denoise_params));\n'
           + "".join(f'  printf(" %zu", offsetof(rt2_denoise_params, {f}));\n' for f in fields) + "  return 0;\n}\n")
    c, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(c, "w").write(src)
    b = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(DenoiseParams)] + [getattr(DenoiseParams, f).offset for f in fields]
