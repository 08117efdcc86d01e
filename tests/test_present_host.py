"""The tone map of a present on the host: the shared header the GPU kernel runs (raytrace2_amd/csrc/present.h,
built into the stand-alone tests/cpp/present_host.cpp, also under the address and undefined-behaviour
sanitizers) against its numpy statement (tests/present_ref.py) byte for byte, the edge values the header names,
and the new entry points' argument checks, defaults and struct layout. No GPU."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import host_build as H
import raytrace2_amd as R
from conftest import ROOT
from present_ref import EDGE_BYTES, EDGE_VALUES, edge_cases, edge_image, present
from raytrace2_amd._native import CameraDesc, DenoiseParams, PresentParams, TemporalParams

F32 = np.float32
SIZES = [(1, 1), (1, 9), (33, 9), (70, 37)]


def _exe(sanitize):
    return H.program("present_host.cpp", [*H.HOST, *(H.HOST_SAN if sanitize else ())])


def _run(exe, tmp_path, c):
    h, w = c.shape[:2]
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(struct.pack("<2i", w, h))
        fh.write(np.ascontiguousarray(c, F32).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = np.fromfile(dst, np.uint8)
    assert out.size == 4 * w * h
    return out.reshape(h, w, 4)


def test_numpy_statement_on_the_edge_values():
    """What present.h states for each edge value, and the alpha byte."""
    c = edge_cases()
    px = present(c)
    for k in range(3):
        assert np.array_equal(px[k, :, k], EDGE_BYTES), k
    assert (px[..., 3] == 255).all()
    # the bytes of ToColor(clamp(c, 0, 1)) on finite values: floor(clip(c) * 255.999) in double
    fin = np.isfinite(c)
    want = np.floor(np.clip(np.where(fin, c, 0), 0, 1).astype(np.float64) * 255.999).astype(np.uint8)
    assert np.array_equal(px[..., :3][fin], want[fin])
    assert present(np.array([[0.5, 0.25, 1.0]], F32)).tolist() == [[127, 63, 255, 255]]


@pytest.mark.parametrize("sanitize", [False, True])
def test_host_program_matches_numpy_byte_for_byte(tmp_path, sanitize):
    """Every size of the issue on random values in [-0.5, 1.5] (the two larger ones with the edge values in), and
    each edge value in every channel; the sanitized build is its own program."""
    exe = _exe(sanitize)
    for (w, h) in SIZES:
        c = edge_image(w, h)
        assert c.shape == (h, w, 3)
        assert np.array_equal(_run(exe, tmp_path, c), present(c)), (w, h)
    big = edge_image(70, 37)
    for e in EDGE_VALUES:  # (NaN compares unequal to itself)
        same = np.isnan(big) if np.isnan(e) else (big.view(np.uint32) == np.array(e, F32).view(np.uint32))
        assert same.any(axis=(0, 1)).all(), e
    c = edge_cases()
    got = _run(exe, tmp_path, c)
    assert np.array_equal(got, present(c))
    for k in range(3):
        assert np.array_equal(got[k, :, k], EDGE_BYTES), k


def test_argument_checks_return_invalid():
    L = R.lib
    px = (ctypes.c_uint8 * 16)()
    col = (ctypes.c_float * 16)()
    ms = ctypes.c_double(0)
    cam = CameraDesc()
    assert L.rt2_tracer_present_async(None, None, px) == -1
    assert L.rt2_tracer_present(None, None, px) == -1
    assert L.rt2_tracer_move_camera(None, ctypes.byref(cam), None) == -1
    assert L.rt2_tracer_present_time(None, ctypes.byref(ms)) == -1
    assert b"null" in L.rt2_last_error()
    assert L.rt2_present_buffers(0, 1, 1, None, px) == -1
    assert L.rt2_present_buffers(0, 1, 1, col, None) == -1
    assert b"null" in L.rt2_last_error()
    for w, h in [(0, 1), (1, 0), (-1, 4), (4, -1), (1 << 13, 1 << 13), (65536, 65536)]:
        assert L.rt2_present_buffers(0, w, h, col, px) == -1, (w, h)
        assert b"present_buffers" in L.rt2_last_error()
    L.rt2_present_defaults(None)  # a no-op
    with pytest.raises(ValueError):
        R.present_buffers(np.zeros((2, 2), F32))
    with pytest.raises(ValueError):
        R.present_buffers(np.zeros((2, 2, 4), F32))


def test_defaults_are_the_two_existing_defaults_with_both_stages_on():
    p = PresentParams()
    p.temporal, p.denoise = 7, 7
    R.lib.rt2_present_defaults(ctypes.byref(p))
    assert (p.temporal, p.denoise) == (1, 1)
    tp, dp = TemporalParams(), DenoiseParams()
    R.lib.rt2_temporal_defaults(ctypes.byref(tp))
    R.lib.rt2_denoise_defaults(ctypes.byref(dp))
    assert bytes(p.tp) == bytes(tp) and bytes(p.dp) == bytes(dp)
    assert R.present_defaults() == {"temporal": 1, "denoise": 1, "tp": R.temporal_defaults(), "dp": R.denoise_defaults()}


def test_params_struct_matches_the_header(tmp_path):
    """rt2_present_params (include/rt2.h) and its ctypes mirror agree on size and offsets."""
    fields = [f for f, _ in PresentParams._fields_]
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "rt2.h"\nint main(void) {\n'
           '  printf("%zu", sizeof(rt2_present_params));\n'
           + "".join(f'  printf(" %zu", offsetof(rt2_present_params, {f}));\n' for f in fields) + "  return 0;\n}\n")
    c, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(c, "w").write(src)
    b = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(PresentParams)] + [getattr(PresentParams, f).offset for f in fields]


def test_cpp_mirror_present_members_compile():
    """include/rt2/RayTracer.hpp: PresentDefaults, Present, PresentAsync, MoveCamera, PresentTime, Query."""
    H.syntax_only("mirror_present.cpp")
