"""Temporal reuse on the host: the shared header the GPU kernels run (raytrace2_amd/csrc/temporal.h, built into the
stand-alone tests/cpp/temporal_host.cpp) against its numpy float32 statement (tests/temporal_ref.py) bit for bit,
plain and under sanitizers, each degenerate case the header names, the properties that follow from the statement,
the quality check and its control on the numpy statement with the oracle's images, and the new entry points'
argument checks. No GPU."""
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
from denoise_ref import features_ref, variance_of_sem
from helpers import SEED, rmse
from noise_ref import noise_ref
from raytrace2_amd._native import TemporalParams
from temporal_ref import DEFAULTS, FEATURE_FLOATS, case_args, params, project, synthetic_case, temporal_ref

F32 = np.float32
SIZES = [(1, 1), (1, 9), (9, 1), (33, 9), (70, 37)]
OTHER = dict(max_history=48.0, max_history_specular=6.0, min_normal_dot=0.5, sigma_p=0.25, sigma_a=2.0)


def _exe(sanitize):
    return H.program("temporal_host.cpp", [*H.HOST, *(H.HOST_SAN if sanitize else ())])


def _run(exe, tmp_path, args, materials=None, **kw):
    k = params(**kw)
    h, w = np.asarray(args[1]).shape
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<4i5f", w, h, -1 if materials is None else len(materials), 0, k["max_history"],
                             k["max_history_specular"], k["min_normal_dot"], k["sigma_p"], k["sigma_a"]))
        fh.write(np.ascontiguousarray(args[8], F32).tobytes())
        for a in args[:8]:
            fh.write(np.ascontiguousarray(a, F32).tobytes())
        if materials is not None:
            fh.write(np.ascontiguousarray(materials, F32).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = np.fromfile(dst, F32)
    n = w * h
    assert out.size == 5 * n
    return out[:3 * n].reshape(h, w, 3), out[3 * n:4 * n].reshape(h, w), out[4 * n:].reshape(h, w)


def _same3(got, ref):
    return all(same_bits(g, r) for g, r in zip(got, ref))


@pytest.mark.parametrize("sanitize", [False, True])
def test_host_program_matches_numpy_bit_for_bit(tmp_path, sanitize):
    """Every size of the GPU test, with and without the material table, at the defaults and at other parameters;
    the sanitized build is its own program."""
    exe = _exe(sanitize)
    for (w, h) in SIZES:
        case = synthetic_case(w, h)
        args = case_args(case)
        for mats in (case["materials"], None):
            for kw in ({}, OTHER):
                ref = temporal_ref(*args, materials=mats, **kw)
                got = _run(exe, tmp_path, args, materials=mats, **kw)
                assert _same3(got, ref), (w, h, mats is None, kw)
    case = synthetic_case(33, 9, seed=5)
    kw = dict(max_history=3.0, max_history_specular=1000.0, min_normal_dot=-1.0, sigma_p=1e-6, sigma_a=1e-3)
    assert _same3(_run(exe, tmp_path, case_args(case), materials=case["materials"], **kw),
                  temporal_ref(*case_args(case), materials=case["materials"], **kw))


def test_synthetic_case_reaches_the_branches():
    case = synthetic_case(70, 37)
    args = case_args(case)
    c, v, n, f = args[:4]
    for spec_cap in (0.0, 6.0):
        tr = {}
        oc, ov, on = temporal_ref(*args, materials=case["materials"], trace=tr, max_history_specular=spec_cap)
        assert (~tr["hit"]).any(), "a current miss"
        assert (~tr["finite"]).any() and np.isnan(c).any() and np.isinf(v).any(), "a non-finite current pixel"
        for edge in ("outside_l", "outside_r", "outside_b", "outside_t"):
            assert tr[edge].any(), edge
        for key in ("len_zero", "hist_nonfinite", "old_miss", "mat", "normal", "plane", "albedo", "accepted", "b_zero"):
            assert tr[key].any(), key
        assert np.isinf(case["hist_color"]).any() and np.isnan(case["hist_variance"]).any()
        P, K = f[..., 2:5], case["hist_camera"]
        dr = (P[..., 2] - K[11]) * (K[3] * K[7] - K[4] * K[6])
        assert (tr["hit"] & tr["finite"] & (dr < 0)).any(), "a point behind the old camera"
        assert (tr["hit"] & tr["finite"] & (dr == 0)).any(), "dr == 0"
        assert not tr["has"][tr["hit"] & (dr <= 0)].any()
        assert tr["tx_zero"].any() and (tr["tx_zero"] & tr["has"]).any(), "tx == 0"
        assert tr["capped"].any() and tr["uncapped"].any(), "the cap reached and not reached"
        assert ((f[..., 13] == 0) & tr["hit"]).any(), "dist == 0"
        mt = case["materials"][:, 0]
        metal = tr["specular"] & (mt[f[..., 9].astype(int) % len(mt)] == 0)
        glass = tr["specular"] & (mt[f[..., 9].astype(int) % len(mt)] == 2)
        assert metal.any() and glass.any(), "a metal and a dielectric current hit"
        if spec_cap == 0:
            assert tr["cap_zero"][metal].any() and tr["cap_zero"][glass].any() and not tr["has"][tr["specular"]].any()
            assert same_bits(on[tr["specular"]], n[tr["specular"]])
        else:
            assert tr["has"][metal].any() and tr["has"][glass].any()
            assert (on[tr["has"] & tr["specular"]] == F32(spec_cap) + F32(4)).all()
        fin = tr["finite"]
        # no finite input gives a NaN or an inf; the others pass through bit for bit with length 0
        assert np.isfinite(oc[fin]).all() and np.isfinite(ov[fin]).all() and np.isfinite(on).all()
        assert same_bits(oc[~fin], c[~fin]) and same_bits(ov[~fin], v[~fin]) and (on[~fin] == 0).all()
        # no history: the current pixel bit for bit
        no = fin & ~tr["has"]
        assert no.any() and same_bits(oc[no], c[no]) and same_bits(ov[no], v[no]) and same_bits(on[no], n[no])
        assert (oc[tr["has"]] != c[tr["has"]]).any()


def _flat(w, h):
    """A plane z = 4 seen by the same exact camera in both images, constant lengths."""
    case = synthetic_case(w, h, seed=3)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    K = case["hist_camera"].astype(np.float64)
    d = K[0:3] + x[..., None] * K[3:6] + y[..., None] * K[6:9] - K[9:12]
    P = K[9:12] + 4.0 * d
    f = np.zeros((h, w, FEATURE_FLOATS), F32)
    f[..., 0], f[..., 8] = 1, 1
    f[..., 2:5] = P
    f[..., 5:8] = [0, 0, -1]
    f[..., 10:13] = 0.5
    f[..., 13] = np.sqrt((P * P).sum(-1))
    rng = np.random.default_rng(9)
    c, hc = rng.random((h, w, 3), F32), rng.random((h, w, 3), F32)
    v, hv = rng.random((h, w), F32) * F32(0.01), rng.random((h, w), F32) * F32(0.001)
    return dict(color=c, variance=v, length=np.full((h, w), 4, F32), features=f, hist_color=hc, hist_variance=hv,
                hist_length=np.full((h, w), 64, F32), hist_features=f.copy(), hist_camera=case["hist_camera"].copy(),
                materials=None)


def test_degenerate_cases(tmp_path):
    exe = _exe(False)

    def both(case, **kw):
        ref = temporal_ref(*case_args(case), materials=case["materials"], **kw)
        got = _run(exe, tmp_path, case_args(case), materials=case["materials"], **kw)
        assert _same3(got, ref)
        return ref

    # the same camera, the same features: every pixel projects onto itself with tx == ty == 0; only tap (0, 0)
    # counts, the other three have weight 0 and are skipped although they hold NaN
    case = _flat(6, 5)
    ok, fx, fy = project(case["features"][..., 2:5], case["hist_camera"], 6, 5)
    yy, xx = np.mgrid[0:5, 0:6]
    assert ok.all() and (fx == xx).all() and (fy == yy).all()
    ref = both(case)
    a = F32(4) / (F32(64) + F32(4))
    assert same_bits(ref[2], np.full((5, 6), 68, F32))
    assert same_bits(ref[0], case["hist_color"] + a * (case["color"] - case["hist_color"]))
    poisoned = dict(case)
    poisoned["hist_color"] = case["hist_color"].copy()
    poisoned["hist_color"][2, 3] = np.nan
    ref2 = both(poisoned)
    changed = np.zeros((5, 6), bool)
    changed[2, 3] = True
    assert same_bits(ref2[0][~changed], ref[0][~changed]) and same_bits(ref2[0][2, 3], case["color"][2, 3])
    assert ref2[2][2, 3] == 4
    # a 1 x 1 image
    one = _flat(1, 1)
    r1 = both(one)
    assert r1[2][0, 0] == 68
    # dr == 0: every point in the old camera's plane through its centre; behind it
    for z in (0.0, -4.0):
        flat = _flat(6, 5)
        flat["features"][..., 4] = z
        r = both(flat)
        assert _same3(r, (flat["color"], flat["variance"], flat["length"]))
    # dist == 0: the tolerance is 0; the taps lie exactly in the plane and pass, one moved off it by an ulp fails
    flat = _flat(6, 5)
    flat["features"][..., 13] = 0
    r = both(flat)
    assert (r[2] == 68).all()
    flat["hist_features"][1, 1, 4] = np.nextafter(F32(4), F32(5))
    r = both(flat)
    assert r[2][1, 1] == 4 and (r[2] == 68).sum() == 29
    # a cap of 0 for everything specular, and the smallest positive cap
    flat = _flat(6, 5)
    flat["materials"] = np.zeros((1, 8), F32)  # material 0 is a metal
    r = both(flat)
    assert _same3(r, (flat["color"], flat["variance"], flat["length"]))
    r = both(flat, max_history_specular=0.5)
    assert (r[2] == F32(4.5)).all()
    # a degenerate history camera (du == 0): fx is not finite
    flat = _flat(6, 5)
    flat["hist_camera"][3:6] = 0
    r = both(flat)
    assert _same3(r, (flat["color"], flat["variance"], flat["length"]))
    # huge finite values: no NaN comes out
    flat = _flat(6, 5)
    flat["features"][0, 0, 2:5] = [1e30, -1e30, 1e30]
    flat["hist_features"][2, 2, 2:5] = 3e38
    flat["hist_color"][3, 3] = 3e38
    r = both(flat)
    assert not any(np.isnan(x).any() for x in r)


def test_derivable_properties():
    case = synthetic_case(70, 37)
    args = case_args(case)
    c, v, n = args[:3]
    fin = np.isfinite(c).all(-1) & np.isfinite(v)
    # every history length 0: the current image bit for bit, n_out == n
    a0 = list(args)
    a0[6] = np.zeros_like(args[6])
    oc, ov, on = temporal_ref(*a0, materials=case["materials"])
    assert same_bits(oc, c) and same_bits(ov, v) and same_bits(on[fin], n[fin]) and (on[~fin] == 0).all()
    # the history camera turned to face away: the same
    a1 = list(args)
    cam = args[8].copy()
    cam[0:3] = cam[9:12] - (cam[0:3] - cam[9:12])  # pixel00 mirrored through the centre
    a1[8] = cam
    tr = {}
    oc, ov, on = temporal_ref(*a1, materials=case["materials"], trace=tr)
    assert not tr["has"].any() and tr["hit"].any()
    assert same_bits(oc, c) and same_bits(ov, v) and same_bits(on[fin], n[fin])
    # identical camera and features, a constant history length: n_out within 8 ulp of min(nh, cap) + n (four
    # products, three sums and one division, each within half an ulp)
    for nh, cap in ((64.0, 1024.0), (2000.0, 1024.0), (37.3, 1024.0), (37.3, 18.0)):
        flat = _flat(33, 9)
        # a fractional shift, so that all four taps take part
        K = flat["hist_camera"].astype(np.float64)
        flat["features"][..., 2:5] = flat["features"][..., 2:5] + F32(4) * (0.3 * K[3:6] + 0.6 * K[6:9])
        flat["hist_features"][..., 2:5] = flat["features"][..., 2:5]  # one plane, one normal: every tap accepted
        flat["hist_length"][:] = nh
        tr = {}
        _, _, on = temporal_ref(*case_args(flat), trace=tr, max_history=cap)
        inner = tr["has"] & ~(tr["outside_l"] | tr["outside_r"] | tr["outside_b"] | tr["outside_t"])
        assert inner.sum() > 100 and not tr["tx_zero"][inner].any()
        want = F32(min(F32(nh), F32(cap))) + F32(4)
        assert (np.abs(on[inner].astype(np.float64) - float(want)) <= 8 * float(np.spacing(want))).all()


# ---- quality on the oracle's images (numpy statement alone) -------------------------------------------------
QW, QH, QSPP, QHIST, QCUR, QREF = 70, 37, 16, 64, 4, 1024
MOVE = (150.0, 70.0, 0.0)  # added to the camera's centre; look_at stays: the view turns and shifts
RATIO_BOUND = 0.37  # measured 0.3637, rounded up to two decimals


def _sums(o, frames):
    a, q = np.zeros((QH, QW, 3), F32), np.zeros((QH, QW, 3), F32)
    for fr in range(frames):
        s, _, _ = o.render(QW, QH, QSPP, 1, frame_begin=fr, forward=True)
        a = a + s
        q = q + s * s
    return a, q


@functools.lru_cache(maxsize=None)
def _quality_inputs():
    from oracle.oracle import OracleScene
    name = "cornell_box_original"
    o = OracleScene(scene_path(name), SEED)
    camA = o.camera_params(QW, QH, QSPP)
    a, q = _sums(o, QHIST)
    semA, _, _ = noise_ref(a, q, QHIST)
    featA, flagged = features_ref(o, camA, QW, QH, SEED)
    assert not flagged.any()
    hist = (a / F32(QHIST), variance_of_sem(semA), np.full((QH, QW), QHIST, F32), featA, camA)
    cam = _camera_desc(name)
    moved = dict(cam, center=tuple(c + m for c, m in zip(cam["center"], MOVE)))
    o.set_camera(moved["center"], moved["look_at"], moved["view_up"], moved["vfov"], moved["defocus_angle"],
                 moved["focus_distance"])
    camB = o.camera_params(QW, QH, QSPP)
    b, qb = _sums(o, QCUR)
    semB, _, _ = noise_ref(b, qb, QCUR)
    featB, flagged = features_ref(o, camB, QW, QH, SEED)
    assert not flagged.any()
    cur = (b / F32(QCUR), variance_of_sem(semB), np.full((QH, QW), QCUR, F32), featB)
    t = OracleScene(scene_path(name), SEED + 1)
    t.set_camera(moved["center"], moved["look_at"], moved["view_up"], moved["vfov"], moved["defocus_angle"],
                 moved["focus_distance"])
    ref, _, _ = t.render(QW, QH, QSPP, QREF, forward=True)
    return cur, hist, o.materials(), ref / F32(QREF)


def _camera_desc(name):
    from raytrace2_amd._native import CameraDesc
    sc = R.Scene(scene_path(name), SEED)
    c = CameraDesc()
    assert R.lib.rt2_scene_get_camera(sc._h, ctypes.byref(c)) == 0
    return dict(center=tuple(c.center), look_at=tuple(c.look_at), view_up=tuple(c.view_up), vfov=c.vfov,
                defocus_angle=c.defocus_angle, focus_distance=c.focus_distance)


def test_reprojected_history_is_closer_to_the_converged_image():
    """Cornell 70x37: 64 frames of history at camera A, 4 current frames at the moved camera B, against the
    oracle's 1024-frame mean at B with another seed. The resolved image beats the 4 frames alone, and the
    control (the history taken at the same pixel, no acceptance tests) does worse than the reprojected one.
    The computation is deterministic: the ratio is bounded by its measured value."""
    cur, hist, mats, ref = _quality_inputs()
    c, v, n, feat = cur
    hc, hv, hn, hfeat, camA = hist
    tr = {}
    oc, ov, on = temporal_ref(c, v, n, feat, hc, hv, hn, hfeat, camA, materials=mats, trace=tr)
    # the move, in pixels of the history image
    ok, fx, fy = project(feat[..., 2:5], camA, QW, QH)
    yy, xx = np.mgrid[0:QH, 0:QW]
    sel = ok & (feat[..., 0] != 0)
    dx, dy = (fx - xx)[sel], (fy - yy)[sel]
    print(f"move {MOVE}: dx {dx.min():.2f}..{dx.max():.2f} px, dy {dy.min():.2f}..{dy.max():.2f} px, "
          f"history found at {tr['has'].mean():.3f} of the pixels")
    assert dx.max() - dx.min() >= 3 and np.abs(dx).max() >= 3, "the parallax across the image is several pixels"
    # the control: no reprojection, no acceptance tests
    a = n / (np.minimum(hn, F32(DEFAULTS["max_history"])) + n)
    control = hc + a[..., None] * (c - hc)
    noisy, res, ctl = rmse(c, ref), rmse(oc, ref), rmse(control, ref)
    print(f"rmse: 4 frames {noisy:.5f}, resolved {res:.5f}, control {ctl:.5f}, ratio {res / noisy:.4f}")
    assert np.isfinite(oc).all() and np.isfinite(ov).all()
    assert res < noisy
    assert ctl > res
    assert res / noisy <= RATIO_BOUND


# ---- the public surface without a GPU ------------------------------------------------------------------------
def test_defaults_match_the_reference_statement():
    d = R.temporal_defaults()
    assert set(d) == set(DEFAULTS)
    for k in DEFAULTS:
        assert d[k] == float(F32(DEFAULTS[k]))


def test_argument_checks_return_invalid():
    L = R.lib
    buf = (ctypes.c_float * 32)()
    ins = [buf] * 9
    assert L.rt2_tracer_temporal_resolve(None, None, 0, None, buf, None, None) == -1
    assert L.rt2_tracer_temporal_push(None, None) == -1
    assert L.rt2_tracer_temporal_clear(None) == -1
    assert L.rt2_tracer_temporal_time(None, None) == -1
    for i in range(9):
        a = list(ins)
        a[i] = None
        assert L.rt2_temporal_buffers(0, 1, 1, *a, None, 0, None, buf, buf, buf) == -1, i
        assert b"null" in L.rt2_last_error()
    assert L.rt2_temporal_buffers(0, 1, 1, *ins, None, 0, None, None, buf, buf) == -1
    for w, h in ((0, 1), (1, 0), (-1, 1), (1 << 13, 1 << 13)):
        assert L.rt2_temporal_buffers(0, w, h, *ins, None, 0, None, buf, buf, buf) == -1, (w, h)
        assert b"2^26" in L.rt2_last_error()
    assert L.rt2_temporal_buffers(0, 1, 1, *ins, buf, -1, None, buf, buf, buf) == -1
    assert b"n_materials" in L.rt2_last_error()
    for field, bad in [("max_history", 0.0), ("max_history", float("inf")), ("max_history_specular", -1.0),
                       ("max_history_specular", float("nan")), ("min_normal_dot", float("nan")), ("sigma_p", 0.0),
                       ("sigma_p", float("inf")), ("sigma_a", -1.0), ("sigma_a", float("nan"))]:
        p = TemporalParams()
        L.rt2_temporal_defaults(ctypes.byref(p))
        setattr(p, field, bad)
        assert L.rt2_temporal_buffers(0, 1, 1, *ins, None, 0, ctypes.byref(p), buf, buf, buf) == -1, (field, bad)
        assert b"temporal" in L.rt2_last_error()
    z = lambda *s: np.zeros(s, F32)  # noqa: E731
    good = [z(1, 1, 3), z(1, 1), z(1, 1), z(1, 1, 16)] * 2 + [z(21)]
    with pytest.raises(TypeError):
        R.temporal_buffers(*good, sigma=1)
    with pytest.raises(ValueError):
        R.temporal_buffers(z(1, 2, 3), *good[1:])
    with pytest.raises(ValueError):
        R.temporal_buffers(*good[:8], z(20))
    with pytest.raises(ValueError):
        R.temporal_buffers(*good, materials=z(2, 7))


def test_cpp_mirror_temporal_members_compile():
    """include/rt2/RayTracer.hpp: TemporalDefaults, TemporalResolve, TemporalPush, TemporalClear."""
    H.syntax_only("mirror_temporal.cpp")


def test_params_struct_matches_the_header(tmp_path):
    """rt2_temporal_params (include/rt2.h) and its ctypes mirror agree on size and offsets."""
    fields = [f for f, _ in TemporalParams._fields_]
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "rt2.h"\nint main(void) {\n'
           '  printf("%zu", sizeof(rt2_temporal_params));\n'
           + "".join(f'  printf(" %zu", offsetof(rt2_temporal_params, {f}));\n' for f in fields) + "  return 0;\n}\n")
    c, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(c, "w").write(src)
    b = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(TemporalParams)] + [getattr(TemporalParams, f).offset for f in fields]
