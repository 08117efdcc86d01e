"""Adaptive sampling on the host: the per-pixel rules the GPU's check runs (raytrace2_amd/csrc/adaptive.h,
built into the stand-alone tests/cpp/adaptive_host.cpp) against the numpy simulator (tests/adaptive_ref.py),
the new entry points' argument checks, the struct layout and the C++ mirror. No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import host_build as H
import raytrace2_amd as R
from adaptive_ref import AdaptiveSim, over_flags, window_or
from conftest import ROOT
from raytrace2_amd._native import Adaptive



def _build(sanitize):
    return H.program("adaptive_host.cpp", [*H.HOST, *(H.HOST_SAN if sanitize else ())])


def _sums(rng, width, kind):
    """One row: n (width) uint32, a and q (width, 3) float32 sums of n samples in frame order, as the kernel's."""
    n = rng.integers(2, 40, width).astype(np.uint32)
    a, q = np.zeros((width, 3), np.float32), np.zeros((width, 3), np.float32)
    for x in range(width):
        if kind == "none-over":
            s = np.full((n[x], 3), np.float32(0.5))  # equal samples: err 0 (or rounding noise far below any threshold)
        else:
            scale = np.float32(4.0 if kind == "all-over" else rng.choice([0.0, 0.02, 0.5, 4.0]))
            s = (rng.random((n[x], 3), np.float32) * scale).astype(np.float32)
        for f in range(n[x]):
            a[x] = a[x] + s[f]
            q[x] = q[x] + s[f] * s[f]
    if kind == "nonfinite":
        bad = rng.random(width) < 0.3
        bad[rng.integers(width)] = True
        a[bad, rng.integers(3)] = rng.choice([np.nan, np.inf, -np.inf])
    return n, a, q


def _rows():
    """(threshold, window, n, a, q, active) per row."""
    rng = np.random.default_rng(11)
    rows = []
    for width in (1, 2, 7, 40, 64, 65, 130, 200):
        for window in (0, 1, 64):
            for kind in ("random", "all-over", "none-over", "nonfinite"):
                n, a, q = _sums(rng, width, kind)
                thr = np.float32(0.05 if kind != "all-over" else 1e-6)
                active = rng.random(width) < 0.8
                rows.append((thr, window, n, a, q, active))
    rows.append((np.float32(0.0), 3, *_sums(rng, 50, "random"), np.ones(50, bool)))  # threshold 0: only err == 0 is below
    return rows


def _run(exe, tmp_path, rows):
    path = tmp_path / "rows.txt"
    with open(path, "w") as f:
        for thr, window, n, a, q, active in rows:
            f.write(f"{np.float32(thr).view(np.uint32):08x} {window} {len(n)}\n")
            for x in range(len(n)):
                words = " ".join(f"{w:08x}" for w in np.concatenate([a[x], q[x]]).view(np.uint32))
                f.write(f"{int(n[x])} {words} {int(active[x])}\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.array([[int(v) for v in l.split()] for l in r.stdout.splitlines()], bool)
    assert len(got) == sum(len(row[2]) for row in rows)
    return got


@pytest.mark.parametrize("sanitize", [False, True])
def test_retire_rule_matches_the_simulator(tmp_path, sanitize):
    """tests/cpp/adaptive_host.cpp over adaptive.h, plain and with the host sanitizers (a stand-alone program)."""
    exe = _build(sanitize)
    rows = _rows()
    got = _run(exe, tmp_path, rows)
    at = 0
    seen = {"all": 0, "none": 0, "nonfinite": 0, "mixed": 0, "retired": 0, "kept_by_window": 0}
    for thr, window, n, a, q, active in rows:
        over, finite = over_flags(a[None], q[None], n[None], thr)
        stays = active[None] & window_or(over, window)
        g = got[at:at + len(n)]
        at += len(n)
        assert np.array_equal(g[:, 0], over[0]), (thr, window, len(n))
        assert np.array_equal(g[:, 1], finite[0])
        assert np.array_equal(g[:, 2], stays[0]), (thr, window, len(n))
        assert over[0][~finite[0]].all(), "a non-finite pixel is always over"
        if window == 0:
            assert np.array_equal(stays[0], active & over[0])
        seen["all"] += over.all()
        seen["none"] += not over.any()
        seen["nonfinite"] += (~finite).any()
        seen["mixed"] += over.any() and not over.all()
        seen["retired"] += int((active & ~stays[0]).sum())
        seen["kept_by_window"] += int((stays[0] & ~over[0]).sum())
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


def test_simulator_steps():
    """The simulator itself on a hand-made 1 x 4 image: constant pixels retire at the first check unless a
    neighbour within the window is noisy; a retired pixel keeps its sums and count."""
    s = np.zeros((8, 1, 4, 3), np.float32)
    s[:, 0, 0] = 0.5                                   # constant: err 0
    s[:, 0, 1] = 0.25                                  # constant, next to the noisy pixel
    s[:, 0, 2] = (np.arange(8) % 2)[:, None] * 2.0     # alternating 0 / 2: noisy
    s[:, 0, 3] = np.nan                                # non-finite: never retires
    s[:, 0, 3, 1:] = 0.0
    sim = AdaptiveSim(s)
    sim.render(4)
    out = sim.check(0.05, 1)
    assert out == {"frames": 4, "pixels": 4, "active": 3, "retired": 1, "samples": 16, "nonfinite": 1}
    assert list(sim.active[0]) == [False, True, True, True]
    sim.render(4)
    assert list(sim.n[0]) == [4, 8, 8, 8] and sim.a[0, 0, 0] == 2.0 and sim.a[0, 1, 0] == 2.0
    out = sim.check(0.05, 0)  # window 0: the quiet neighbour goes, the NaN pixel and the noisy one stay
    assert (out["active"], out["retired"], out["samples"]) == (2, 1, 28)
    sim.reset()
    full = sim.render_adaptive(1e9, 8, window=1, check_every=4)
    # the finite pixels are below; the NaN pixel is over and keeps its neighbour within the window going
    assert full["frames"] == 8 and full["active"] == 2 and list(sim.n[0]) == [4, 4, 8, 8]


def test_null_arguments_return_invalid():
    a = Adaptive()
    buf = (ctypes.c_uint32 * 3)()
    L = R.lib
    assert L.rt2_tracer_enable_adaptive(None, 1) == R._native.RT2_ERR_INVALID
    assert L.rt2_tracer_sample_counts(None, buf) == -1
    assert L.rt2_tracer_adaptive_check(None, 0.1, 1, ctypes.byref(a)) == -1
    assert L.rt2_tracer_render_adaptive(None, 0.1, 1, 0, 16, 0, ctypes.byref(a)) == -1
    assert b"null" in L.rt2_last_error()


def test_cpp_mirror_adaptive_members_compile():
    """include/rt2/RayTracer.hpp: EnableAdaptive, SampleCounts, AdaptiveCheck, RenderAdaptive."""
    H.syntax_only("mirror_adaptive.cpp")


def test_adaptive_struct_matches_the_header(tmp_path):
    """rt2_adaptive (include/rt2.h) and its ctypes mirror agree on size and offsets (gcc lays out the C one)."""
    fields = [f for f, _ in Adaptive._fields_]
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "rt2.h"\nint main(void) {\n'
           '  printf("%zu", sizeof(rt2_adaptive));\n'
           + "".join(f'  printf(" %zu", offsetof(rt2_adaptive, {f}));\n' for f in fields) + "  return 0;\n}\n")
    c, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    open(c, "w").write(src)
    b = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(Adaptive)] + [getattr(Adaptive, f).offset for f in fields]
    assert fields == ["frames", "pixels", "active", "retired", "samples", "nonfinite"]


@pytest.mark.parametrize("window", ["65", "-1", "1x", ""])
def test_headless_refuses_a_bad_window_on_the_command_line(tmp_path, window):
    """rt2_headless --adaptive: --window is checked while the options are parsed, before any GPU work."""
    app = os.path.join(ROOT, "raytrace2_amd", "lib", "rt2_headless")
    r = subprocess.run([app, os.path.join(ROOT, "scenes", "cornell_box_original.json"), str(tmp_path / "x.png"),
                        "--adaptive", "0.05", "--window", window], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--window needs an integer in [0, 64]" in r.stderr
    assert not (tmp_path / "x.png").exists()
