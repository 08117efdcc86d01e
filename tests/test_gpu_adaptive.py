"""Adaptive sampling on the GPU (include/rt2.h "Adaptive sampling") against the numpy simulator
(tests/adaptive_ref.py) run over the oracle's per-frame samples: which pixel retires at which check, every
bit of its sums at its own sample count, the check's scalars and the readbacks. The cases are 40x24 pixels
(960: not a multiple of 256 or 64), spp 16, seed 0x5EED2024, steps of 16 frames up to 80, threshold
float32(0.05), window 1, unless the case says otherwise."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from adaptive_ref import AdaptiveSim, margin, pixel_noise
from bits import f32_bits, refused
from conftest import ROOT, scene_path
from helpers import SEED

pytestmark = pytest.mark.gpu
W, H, SPP, MAXF, STEP = 40, 24, 16, 80, 16
THR = float(np.float32(0.05))
NPIX = W * H
SCENES = ["cornell_box_original", "final_render_book_1", "cornell_box_volume"]
APP = os.path.join(ROOT, "raytrace2_amd", "lib", "rt2_headless")
# pixels the reference retires at the checks after 16, 32, 48 and 64 frames, and pixels still active
# before the last step (window 1; Cornell also windows 0 and 2)
TABLE = {("cornell_box_original", 1): ((687, 13, 27, 12), 221),
         ("final_render_book_1", 1): ((478, 342, 107, 27), 6),
         ("cornell_box_volume", 1): ((417, 12, 12, 12), 507),
         ("cornell_box_original", 0): ((835, 10, 20, 10), None),
         ("cornell_box_original", 2): ((591, 11, 31, 13), None)}


@functools.lru_cache(maxsize=None)
def _frames(name):
    """The oracle's per-frame samples (MAXF, H, W, 3) float32 and ray counts (MAXF, H, W): each frame
    rendered into a zero accumulation."""
    from oracle.oracle import OracleScene
    o = OracleScene(scene_path(name), SEED)
    s = np.zeros((MAXF, H, W, 3), np.float32)
    rc = np.zeros((MAXF, H, W), np.uint32)
    for f in range(MAXF):
        s[f], rc[f], _ = o.render(W, H, SPP, 1, frame_begin=f, forward=True)
    s.setflags(write=False)
    rc.setflags(write=False)
    return s, rc


@functools.lru_cache(maxsize=None)
def _reference(name, threshold=THR, window=1, rows=None):
    """The simulator after render_adaptive(threshold, MAXF, window, check_every=STEP), frozen, and its `out`."""
    s, _ = _frames(name)
    sim = AdaptiveSim(s if rows is None else s[:, list(rows)])
    out = sim.render_adaptive(threshold, MAXF, window=window, check_every=STEP)
    for x in (sim.a, sim.q, sim.n, sim.active):
        x.setflags(write=False)
    return sim, out


def _preconditions(name, window):
    """No pass can be empty: every one of the four checks retires a pixel, a pixel is still active before the
    last step, and no pixel is within 1e-9 (relative) of the threshold at any check."""
    sim, _ = _reference(name, THR, window)
    hist = sim.history
    print(name, "window", window, [(h["frames"], h["retired"], h["active"], h["margin"]) for h in hist])
    assert [h["frames"] for h in hist] == [16, 32, 48, 64, 80]
    retired, before_last = TABLE[(name, window)]
    assert tuple(h["retired"] for h in hist[:4]) == retired
    assert all(h["retired"] >= 1 for h in hist[:4]) and hist[3]["active"] >= 1
    if before_last is not None:
        assert hist[3]["active"] == before_last
    assert min(h["margin"] for h in hist) >= 1e-9


def _tracer(name, *, adaptive=True, ray_counts=False):
    import raytrace2_amd as R
    sc = R.Scene(scene_path(name), SEED)
    tr = R.RayTracer(sc, 0)
    tr.set_seed(SEED)
    tr.SetSamplesPerPixel(SPP)
    tr.OnResize((W, H))
    if ray_counts:
        tr.enable_ray_counts(True)
    tr.enable_moments()
    if adaptive:
        tr.enable_adaptive()
    return sc, tr


def _assert_state(tr, sim, what=""):
    assert np.array_equal(tr.sample_counts(), sim.n), f"sample counts differ {what}"
    assert np.array_equal(f32_bits(tr.Accumulation()), f32_bits(sim.a)), f"accumulation differs {what}"
    assert np.array_equal(f32_bits(tr.moments()), f32_bits(sim.q)), f"moments differ {what}"


@pytest.mark.parametrize("name", SCENES)
def test_render_adaptive_matches_the_reference(have_gpu, name):
    _preconditions(name, 1)
    sim, ref = _reference(name)
    sc, tr = _tracer(name)
    out = tr.render_adaptive(THR, MAXF, check_every=STEP)
    print(name, "product", out, "reference", ref)
    assert tr.FrameIdx() == MAXF
    _assert_state(tr, sim)
    assert out == ref
    assert out["samples"] == int(sim.n.sum()) and out["active"] + sum(h["retired"] for h in sim.history) == NPIX
    tr.close()


@pytest.mark.parametrize("window", [0, 2])
def test_windows(have_gpu, window):
    name = "cornell_box_original"
    _preconditions(name, window)
    sim, ref = _reference(name, THR, window)
    sc, tr = _tracer(name)
    out = tr.render_adaptive(THR, MAXF, window=window, check_every=STEP)
    _assert_state(tr, sim, f"window {window}")
    assert out == ref
    tr.close()


@pytest.mark.parametrize("pattern", ["launch8", "updates", "split0"])
def test_launch_patterns_change_no_bit(have_gpu, pattern):
    name = "cornell_box_original"
    sim, ref = _reference(name)
    sc, tr = _tracer(name)
    if pattern == "launch8":
        tr.set_launch_frames(8)  # two launches per step, one per launch slot
    if pattern == "split0":
        tr.set_work_split(0)  # one chunk per pixel
    if pattern == "updates":
        for _ in range(MAXF // STEP):
            for _ in range(STEP):
                tr.Update(sc)
            out = tr.adaptive_check(THR, 1)
    else:
        out = tr.render_adaptive(THR, MAXF, check_every=STEP)
    assert tr.FrameIdx() == MAXF
    _assert_state(tr, sim, pattern)
    assert out == ref
    tr.close()


def test_many_tiles_and_the_widest_window(have_gpu):
    """530x131 pixels: 17 x 17 = 289 retire workgroups and 272 classify workgroups, so each thread of the scan
    takes two of either (40x24 has six), ragged tiles on both edges, and a window of 64 columns that reaches
    over two neighbouring tiles on either side. Checks by hand after 2, 4 and 6 frames, windows 64, 3, 0."""
    import raytrace2_amd as R
    from oracle.oracle import OracleScene
    name, w, h, spp = "cornell_box_original", 530, 131, 4
    o = OracleScene(scene_path(name), SEED)
    s = np.zeros((6, h, w, 3), np.float32)
    for f in range(6):
        s[f], _, _ = o.render(w, h, spp, 1, frame_begin=f, forward=True)
    sim = AdaptiveSim(s)
    sc = R.Scene(scene_path(name), SEED)
    tr = R.RayTracer(sc, 0)
    tr.set_seed(SEED)
    tr.SetSamplesPerPixel(spp)
    tr.OnResize((w, h))
    tr.enable_moments()
    tr.enable_adaptive()
    for window in (64, 3, 0):
        sim.render(2)
        ref = sim.check(THR, window)
        assert ref["retired"] >= 1 and ref["active"] >= 1 and sim.history[-1]["margin"] >= 1e-9
        tr.Render(2)
        out = tr.adaptive_check(THR, window)
        print("window", window, out)
        assert out == ref
        _assert_state(tr, sim, f"window {window}")
    tr.close()


def test_partition(have_gpu):
    from raytrace2_amd import local_rows
    name = "cornell_box_original"
    rows = tuple(local_rows(H, 2, 1, 3))
    full, _ = _reference(name)
    sim, ref = _reference(name, THR, 1, rows)
    # the window runs along the row: a partition decides as the full image does
    assert np.array_equal(sim.n, full.n[list(rows)]) and np.array_equal(f32_bits(sim.a), f32_bits(full.a[list(rows)]))
    assert 0 < ref["active"] < len(rows) * W
    sc, tr = _tracer(name)
    tr.set_partition(2, 1, 3)
    out = tr.render_adaptive(THR, MAXF, check_every=STEP)
    assert tr.local_rows() == len(rows)
    _assert_state(tr, sim, "partition")
    assert out == ref
    tr.close()


def test_ray_counts_are_those_of_each_pixels_frames(have_gpu):
    name = "cornell_box_original"
    sim, ref = _reference(name)
    _, rc = _frames(name)
    expect = np.where(np.arange(MAXF)[:, None, None] < sim.n[None], rc, 0).astype(np.uint64).sum(0)
    sc, tr = _tracer(name, ray_counts=True)  # the counting instantiation of the list kernel
    out = tr.render_adaptive(THR, MAXF, check_every=STEP)
    _assert_state(tr, sim, "ray counts")
    assert out == ref
    assert np.array_equal(tr.ray_counts().astype(np.uint64), expect)
    assert tr.stats()["rays"] == int(expect.sum()) and tr.stats()["paths"] == ref["samples"]
    tr.close()


def test_readbacks_use_each_pixels_count(have_gpu):
    name = "final_render_book_1"
    sim, _ = _reference(name)
    sem, err, finite = pixel_noise(sim.a, sim.q, sim.n)
    sc, tr = _tracer(name)
    tr.render_adaptive(THR, MAXF, check_every=STEP)
    mean = sim.a / sim.n.astype(np.float32)[..., None]
    assert np.array_equal(f32_bits(tr.NonConvertedPixels()), f32_bits(mean))
    px = tr.Pixels()
    expect = np.floor(np.clip(mean, 0, 1).astype(np.float64) * 255.999).astype(np.uint8)
    assert np.array_equal(px[..., :3], expect) and np.all(px[..., 3] == 255)
    assert np.array_equal(f32_bits(tr.standard_error()), f32_bits(sem))
    # (every pixel of this scene has retired, so all are below THR: count against a lower threshold)
    thr = float(np.float32(0.02))
    below = int((err[finite] <= np.float64(np.float32(thr))).sum())
    assert 0 < below < NPIX and margin(sim.a, sim.q, sim.n, thr) >= 1e-9
    nz = tr.noise(thr)
    assert nz["frames"] == MAXF and nz["pixels"] == NPIX and nz["nonfinite"] == 0
    assert nz["below"] == below
    assert len(np.unique(sim.n)) >= 3, "the image mixes sample counts"
    tr.close()


def test_edges(have_gpu):
    name = "cornell_box_original"
    s, _ = _frames(name)
    sc, tr = _tracer(name)
    # a threshold no pixel exceeds: everything retires at the first check
    out = tr.render_adaptive(1e9, MAXF, check_every=STEP)
    assert tr.FrameIdx() == STEP and (out["active"], out["retired"], out["samples"]) == (0, NPIX, NPIX * STEP)
    acc, mom, cnt, launches = tr.Accumulation(), tr.moments(), tr.sample_counts(), tr.stats()["launches"]
    tr.Render(16)  # nothing to trace: the frame index advances, nothing else moves
    assert tr.FrameIdx() == 2 * STEP
    assert np.array_equal(f32_bits(tr.Accumulation()), f32_bits(acc))
    assert np.array_equal(f32_bits(tr.moments()), f32_bits(mom))
    assert np.array_equal(tr.sample_counts(), cnt) and (cnt == STEP).all()
    assert tr.stats()["launches"] == launches
    # threshold 0: only pixels whose estimate is exactly 0, with such neighbours, retire
    sim, ref = _reference(name, 0.0, 1)
    assert 0 < ref["active"] < NPIX
    tr.Reset()
    out = tr.render_adaptive(0.0, MAXF, check_every=STEP)
    _assert_state(tr, sim, "threshold 0")
    assert out == ref
    tr.close()


def test_reset_reactivates_and_reproduces(have_gpu):
    name = "cornell_box_volume"
    sim, ref = _reference(name)
    sc, tr = _tracer(name)
    first = tr.render_adaptive(THR, MAXF, check_every=STEP)
    state = (tr.Accumulation(), tr.moments(), tr.sample_counts())
    tr.Reset()
    assert tr.FrameIdx() == 0 and (tr.sample_counts() == 0).all() and (tr.Accumulation() == 0).all()
    tr.Render(2)
    assert tr.adaptive_check(0.0, 64)["pixels"] == NPIX and (tr.sample_counts() == 2).all(), "every pixel active again"
    tr.Reset()
    second = tr.render_adaptive(THR, MAXF, check_every=STEP)
    assert first == second == ref
    for got, was in zip((tr.Accumulation(), tr.moments(), tr.sample_counts()), state):
        assert np.array_equal(got.view(np.uint32), was.view(np.uint32))
    tr.close()


def test_off_path_is_untouched(have_gpu):
    from helpers import oracle_render
    name = "cornell_box_original"
    o_acc, _, _ = oracle_render(name, W, H, SPP, 13)
    sc, tr = _tracer(name)
    tr.Render(3)
    tr.enable_adaptive(False)
    assert tr.FrameIdx() == 0
    tr.Render(13)
    assert np.array_equal(f32_bits(tr.Accumulation()), f32_bits(o_acc))
    assert np.array_equal(f32_bits(tr.NonConvertedPixels()), f32_bits(o_acc / np.float32(13)))
    tr.close()


def test_refusals(have_gpu):
    import raytrace2_amd as R
    name = "cornell_box_original"
    s, _ = _frames(name)

    sc = R.Scene(scene_path(name), SEED)
    tr = R.RayTracer(sc, 0)
    tr.set_seed(SEED)
    tr.SetSamplesPerPixel(SPP)
    tr.OnResize((W, H))
    refused(tr.enable_adaptive)  # moments off
    for call in (tr.sample_counts, lambda: tr.adaptive_check(THR), lambda: tr.render_adaptive(THR, 16)):
        refused(call)  # adaptive off
    tr.enable_moments()
    tr.enable_adaptive()
    refused(lambda: tr.enable_moments(False))
    tr.Update(sc)
    refused(lambda: tr.adaptive_check(THR))  # one frame
    tr.Update(sc)
    for window in (-1, 65):
        refused(lambda: tr.adaptive_check(THR, window))
    for thr in (-1.0, float("nan")):
        refused(lambda: tr.adaptive_check(thr))
        refused(lambda: tr.render_adaptive(thr, 16))
    multi = R.RayTracer(sc, devices=[0, 0], band_h=2)
    multi.enable_moments()
    refused(multi.enable_adaptive)
    multi.close()
    # the tracer still renders: two frames so far, every pixel active
    assert tr.FrameIdx() == 2
    tr.Render(11)
    a = np.zeros((H, W, 3), np.float32)
    for f in range(13):
        a = a + s[f]
    assert np.array_equal(f32_bits(tr.Accumulation()), f32_bits(a)) and (tr.sample_counts() == 13).all()
    tr.close()


def _plain_tracer(name="cornell_box_original"):
    import raytrace2_amd as R
    sc = R.Scene(scene_path(name), SEED)
    tr = R.RayTracer(sc, 0)
    tr.set_seed(SEED)
    tr.SetSamplesPerPixel(SPP)
    tr.OnResize((W, H))
    return sc, tr


def _sum13(rows=None):
    s, _ = _frames("cornell_box_original")
    a = np.zeros((H, W, 3), np.float32)
    for f in range(13):
        a = a + s[f]
    return a if rows is None else a[rows]


def test_joined_tracer_is_refused_and_adaptive_tracer_cannot_join(have_gpu):
    """One process per GPU (rt2_tracer_join), world 1 on this GPU: a joined tracer refuses enable_adaptive, an
    adaptive tracer refuses join; both still render afterwards."""
    import raytrace2_amd as R
    from raytrace2_amd import local_rows
    sc, tr = _plain_tracer()
    tr.join(R.comm_unique_id(), 1, 0, 16)
    tr.enable_moments()
    refused(tr.enable_adaptive)
    refused(tr.sample_counts)  # adaptive stayed off
    tr.Render(13)
    assert tr.FrameIdx() == 13 and np.array_equal(f32_bits(tr.Accumulation()), f32_bits(_sum13(local_rows(H, 16, 0, 1))))
    tr.close()
    sc, tr = _plain_tracer()
    tr.enable_moments()
    tr.enable_adaptive()
    refused(lambda: tr.join(R.comm_unique_id(), 1, 0, 16))
    tr.Render(13)  # still adaptive, unpartitioned, every pixel active
    assert np.array_equal(f32_bits(tr.Accumulation()), f32_bits(_sum13())) and (tr.sample_counts() == 13).all()
    assert tr.adaptive_check(THR, 1)["pixels"] == NPIX
    tr.close()


def test_tracer_without_the_threaded_traversal_is_refused(have_gpu, monkeypatch):
    """The list kernels exist for the threaded traversal only: a tracer that renders with the stack traversal
    (RT2_NO_LINEAR=1 at creation) refuses enable_adaptive at once, and renders on without it."""
    monkeypatch.setenv("RT2_NO_LINEAR", "1")
    sc, tr = _plain_tracer()
    monkeypatch.delenv("RT2_NO_LINEAR")
    tr.enable_moments()
    refused(tr.enable_adaptive)
    tr.enable_adaptive(False)  # switching it off is always allowed
    tr.Render(13)
    assert np.array_equal(f32_bits(tr.Accumulation()), f32_bits(_sum13()))
    assert tr.noise()["frames"] == 13
    tr.close()


def test_headless_adaptive(have_gpu, tmp_path):
    import raytrace2_amd as R
    png, ref_png = str(tmp_path / "adaptive.png"), str(tmp_path / "py.png")
    r = subprocess.run([APP, scene_path("cornell_box_original"), png, "--size", f"{W}x{H}", "--adaptive", repr(THR),
                        "--window", "1", "--max-samples", str(2 * SPP)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"^frames (\d+) active (\d+) samples (\d+)$", r.stderr, re.M)
    assert m, r.stderr
    sc = R.Scene(scene_path("cornell_box_original"), R.DEFAULT_SEED)
    tr = R.RayTracer(sc, 0)
    tr.SetSamplesPerPixel(2 * SPP)
    tr.OnResize((W, H))
    tr.enable_moments()
    tr.enable_adaptive()
    out = tr.render_adaptive(THR, 2 * SPP)
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (tr.FrameIdx(), out["active"], out["samples"])
    assert 0 < out["active"] < NPIX
    R.WriteImage(tr.NonConvertedPixels(), W, H, ref_png)
    tr.close()
    assert open(png, "rb").read() == open(ref_png, "rb").read()
