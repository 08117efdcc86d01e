"""Occlusion queries on the GPU (include/rt2.h "Ray queries"): RayTracer.occluded against the
oracle's flag and against slot 0 of intersect's record on the boundary batches of tests/edge_rays.py, on the
flag-level batches of tests/occlusion_rays.py, on the compiled reference's recorded answers and on the random
batches of tests/test_gpu_query.py, in the threaded program and in the stack walk; the edges of the launch, the
device entry's exact n bytes, invalid rays, RayTracer.visible, no disturbance of a render, and the refusals. Every
test goes through occluded, which the library did not have before."""
import ctypes
import functools
import os

import numpy as np
import pytest

import edge_rays as E
import occlusion_rays as O
from conftest import ROOT
from helpers import SEED
from test_gpu_parity import MODES
from test_gpu_query import SCENES, _batch, _rays, _tracer, _valid

pytestmark = pytest.mark.gpu
F32 = np.float32
FLT_MAX = np.finfo(F32).max
REF = os.path.join(ROOT, "tests", "golden", "ref")
ALL = E.SCENES + list(E.TIES)
KERNELS = ["linear", "stack_global"]
EDGE_FILES = sorted(f[:-len("_edges.npy")] for f in os.listdir(REF) if f.endswith("_edges.npy"))
BOOK2 = "book2_final_scene_10000_samples"
CORNELL = "cornell_box_original"


def _set(monkeypatch, mode):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)


@functools.lru_cache(maxsize=None)
def _edge_flags(name, seed):
    """The oracle's flags on the scene's edge batch, once for every test and mode."""
    if seed == SEED:
        f = E.answers(name)[:, 0].astype(np.int8)
    else:
        f = np.array([E.hit(E.scene_file(name), r, seed)[0] for r in E.batch(name).rays], F32).astype(np.int8)
    f.setflags(write=False)
    return f


def _describe(name, what, rays, cls, pair, got, exp, bad):
    """A failure's message: the ray, its class, its pair partner and both answers."""
    i = int(bad[0])
    lines = [f"{name} {what}: {bad.size} of {len(got)} answers differ, by class "
             f"{ {str(c): int((cls[bad] == c).sum()) for c in np.unique(cls[bad])} }",
             f"first: ray {i} of class {cls[i]}: {rays[i].tolist()}", f"  kernel {int(got[i])}  expected {int(exp[i])}"]
    j = int(pair[i])
    if j >= 0:
        lines += [f"its pair partner, ray {j}: {rays[j].tolist()}", f"  kernel {int(got[j])}  expected {int(exp[j])}"]
    return "\n".join(lines)


def _check(name, what, rays, cls, pair, got, exp):
    assert got.dtype == np.int8 and got.shape == (len(rays),)
    bad = np.flatnonzero(got != exp)
    if bad.size:
        pytest.fail(_describe(name, what, rays, cls, pair, got, exp, bad))


@pytest.mark.parametrize("mode", KERNELS)
@pytest.mark.parametrize("name", ALL)
def test_edge_batches_against_the_oracle(have_gpu, monkeypatch, name, mode):
    """Every ray of the scene's edge batch: the byte equals the oracle's flag and slot 0 of intersect's record from
    the same tracer; the media scenes again under a second seed; book 2 again without the list acceleration."""
    _set(monkeypatch, mode)
    b = E.batch(name)
    sc, tr = _tracer(E.scene_file(name))
    got = tr.occluded(b.rays)
    _check(name, mode, b.rays, b.cls, b.pair, got, _edge_flags(name, SEED))
    assert np.array_equal(got, tr.intersect(b.rays)[:, 0].astype(np.int8))
    if name in E.MEDIA:
        got2 = tr.occluded(b.rays, seed=SEED + 7)
        _check(name, f"{mode} seed 2", b.rays, b.cls, b.pair, got2, _edge_flags(name, SEED + 7))
        assert np.array_equal(got2, tr.intersect(b.rays, seed=SEED + 7)[:, 0].astype(np.int8))
    assert tr.stats()["overflow"] == 0
    tr.close()
    if name == BOOK2:
        monkeypatch.setenv("RT2_NO_LIST_ACCEL", "1")  # read at scene load
        sc, tr = _tracer(E.scene_file(name))
        _check(name, f"{mode} without the list tree", b.rays, b.cls, b.pair, tr.occluded(b.rays), _edge_flags(name, SEED))
        assert tr.stats()["overflow"] == 0
        tr.close()


@pytest.mark.parametrize("mode", KERNELS)
@pytest.mark.parametrize("name", ALL)
def test_flag_batches_against_the_oracle(have_gpu, monkeypatch, name, mode):
    """The shadow pairs and tmax triples: the byte equals the oracle's flag, and (a separate assertion, which says at
    once which side of a boundary moved) the kernel gives the two rays of every shadow pair different answers."""
    _set(monkeypatch, mode)
    b = O.batch(name)
    sc, tr = _tracer(E.scene_file(name))
    got = tr.occluded(b.rays)
    assert tr.stats()["overflow"] == 0
    tr.close()
    first = np.array([i for i in range(len(b.rays)) if b.cls[i] == "shadow" and i < b.pair[i]], np.int64)
    assert len(first) == O.N_SHADOW
    one = first[got[first] == got[b.pair[first]]]
    if one.size:
        i, j = int(one[0]), int(b.pair[one[0]])
        moved = i if got[i] != b.flag[i] else j
        pytest.fail(f"{name} {mode}: {one.size} shadow pairs get one answer from the kernel; ray {moved} moved across "
                    f"its boundary\n" + _describe(name, mode, b.rays, b.cls, b.pair, got, b.flag, np.array([moved])))
    _check(name, mode, b.rays, b.cls, b.pair, got, b.flag)


@pytest.mark.parametrize("mode", KERNELS)
@pytest.mark.parametrize("name", EDGE_FILES)
def test_against_the_reference(have_gpu, monkeypatch, name, mode):
    """The rays recorded in <scene>_edges.npy: the byte equals the compiled reference's own flag. No oracle."""
    _set(monkeypatch, mode)
    fx = np.load(os.path.join(REF, name + "_edges.npy"))
    assert fx.dtype == np.float32 and fx.shape[1] == 18 and 0 < len(fx) <= E.FIXTURE_RAYS
    rays, ref = np.ascontiguousarray(fx[:, :8]), fx[:, 8].astype(np.int8)
    assert (ref == 1).any() and (ref == 0).any()
    sc, tr = _tracer(E.scene_file(name))
    got = tr.occluded(rays)
    tr.close()
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, (f"{name} {mode}: {bad.size} of {len(fx)} answers differ from the reference; first: ray "
                           f"{bad[0]} {rays[bad[0]].tolist()}: kernel {got[bad[0]]}, reference {ref[bad[0]]}")


@pytest.mark.parametrize("name", SCENES)
def test_random_batches(have_gpu, name):
    rays, exp, _, _ = _batch(name)
    sc, tr = _tracer(name)
    got = tr.occluded(rays)
    tr.close()
    bad = np.flatnonzero(got != exp[:, 0].astype(np.int8))
    assert bad.size == 0, f"{name}: {bad.size} answers differ; first: ray {bad[0]} {rays[bad[0]].tolist()}"


def test_wave_and_chunk_edges(have_gpu, monkeypatch):
    b = O.batch(CORNELL)
    sc, tr = _tracer(CORNELL)
    full = tr.occluded(b.rays)
    assert np.array_equal(full, b.flag)
    for n in (1, 63, 64, 65, 257):
        assert np.array_equal(tr.occluded(b.rays[:n]), full[:n]), n
    for chunk in ("64", "128"):
        monkeypatch.setenv("RT2_QUERY_CHUNK", chunk)
        assert np.array_equal(tr.occluded(b.rays[:300]), full[:300]), chunk
    monkeypatch.delenv("RT2_QUERY_CHUNK")
    empty = tr.occluded(np.zeros((0, 8), F32))
    assert empty.shape == (0,) and empty.dtype == np.int8
    tr.close()


def test_device_entry_writes_exactly_n_bytes(have_gpu):
    import torch
    from raytrace2_amd._native import lib
    b = O.batch(CORNELL)
    sc, tr = _tracer(CORNELL)
    d_rays = torch.from_numpy(np.array(b.rays)).cuda()
    d_out = tr.occluded(d_rays)
    assert d_out.is_cuda and d_out.dtype == torch.int8 and np.array_equal(d_out.cpu().numpy(), b.flag)
    assert tr.intersect_time() >= 0  # the last query of either kind, finished
    for n in (1, 65, 257):
        out = torch.full((n + 64,), 0x55, dtype=torch.int8, device="cuda")
        torch.cuda.synchronize()
        rc = lib.rt2_tracer_occluded_device(tr._h, n, ctypes.c_void_p(d_rays.data_ptr()), SEED,
                                            ctypes.c_void_p(out.data_ptr()))
        assert rc == 0
        tr.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], b.flag[:n]), n
        assert (got[n:] == 0x55).all(), n
    tr.close()


@pytest.mark.parametrize("name", [CORNELL, "final_render_book_1"])
def test_invalid_rays_stay_out(have_gpu, name):
    """Invalid rays (NaN, zero direction, tmax <= 0.001, time 2, an origin at 2^65) scattered among valid ones answer
    -1 and their neighbours answer as they do alone; a batch of only invalid rays answers -1 throughout."""
    import raytrace2_amd as R
    b = O.batch(name)
    good, exp = np.array(b.rays[:450]), b.flag[:450]
    bad = []
    for k in range(150):
        r = good[k].copy()
        c = k % 5
        if c == 0:
            r[k % 8] = np.nan
        elif c == 1:
            r[4:7] = 0
        elif c == 2:
            r[3] = F32(0.001) if k % 2 else F32(0.0)
        elif c == 3:
            r[7] = 2
        else:
            r[k % 3] = F32(2.0 ** 65)
        bad.append(r)
    bad = np.array(bad, F32)
    assert not _valid(bad).any() and not R.ray_valid(bad).any()
    mixed = np.zeros((len(good) + len(bad), 8), F32)
    is_bad = np.arange(len(mixed)) % 4 == 3
    assert is_bad.sum() == len(bad)
    mixed[~is_bad] = good
    mixed[is_bad] = bad
    sc, tr = _tracer(name)
    alone = tr.occluded(good)
    assert np.array_equal(alone, exp)
    got = tr.occluded(mixed)
    assert np.array_equal(got[~is_bad], alone)
    assert (got[is_bad] == -1).all()
    assert (tr.occluded(bad) == -1).all() and (tr.occluded(bad[:64]) == -1).all()
    assert tr.stats()["overflow"] == 0
    tr.close()


def test_visible(have_gpu):
    """200 point pairs in the Cornell box against oracle.hit with d = b - a, tmax = 0.999: from the light quad's
    centre to points on the floor, to the points its rays reach first (blocks, walls, floor), between random
    interior points, and from above the light quad to interior points below it (blocked by the quad); a == b is not
    traced. (The two blocks are transformed children: their t is the reference's model-space t along a normalised
    direction, so they block a segment only where that t is below 0.999, and the oracle says so too.)"""
    g = np.random.default_rng(31)
    o_ = E.oracle(E.scene_file(CORNELL))
    light = np.array([343 - 65.0, 554, 332 - 52.5], F32)  # q + u / 2 + v / 2 of the light quad
    a, b = [], []
    for _ in range(100):  # the floor, some of it in the blocks' shadow or under them
        a.append(light)
        b.append(np.array([g.uniform(5, 550), 0, g.uniform(5, 550)], F32))
    while len(a) < 140:  # the first surface along a ray from the light: visible from it by construction
        d = E._unit(g.normal(size=3)).astype(F32)
        rec = o_.hit(light, d, time=0.0, seed=SEED)
        if rec[0] != 1:
            continue
        a.append(light)
        b.append(rec[2:5].astype(F32))
    for _ in range(39):
        a.append(g.uniform(5, 550, 3).astype(F32))
        b.append(g.uniform(5, 550, 3).astype(F32))
    for _ in range(20):  # from between the light quad and the ceiling, inside the quad's outline, to the room below
        a.append(np.array([g.uniform(220, 340), 554.5, g.uniform(232, 327)], F32))
        b.append(np.array([g.uniform(230, 330), g.uniform(300, 500), g.uniform(240, 320)], F32))
    a.append(np.array([100, 100, 100], F32))
    b.append(np.array([100, 100, 100], F32))
    a, b = np.array(a, F32), np.array(b, F32)
    assert len(a) == 200
    want = np.zeros(len(a), np.int8)
    d = b - a
    for i in range(len(a)):
        if not d[i].any():
            want[i] = -1
            continue
        want[i] = 1 - int(o_.hit(a[i], d[i], time=0.0, tmin=0.001, tmax=float(F32(0.999)), seed=SEED)[0])
    assert (want == 1).sum() >= 20 and (want == 0).sum() >= 20 and want[-1] == -1
    assert (want[179:199] == 0).all()
    assert (want[100:140] == 1).all()
    sc, tr = _tracer(CORNELL)
    got = tr.visible(a, b)
    tr.close()
    assert got.dtype == np.int8 and got.shape == (200,)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} pairs differ; first {bad[0]}: {a[bad[0]]} -> {b[bad[0]]}: {got[bad[0]]} vs {want[bad[0]]}"


def test_no_disturbance(have_gpu):
    """4 Updates, one occlusion query by each entry, 4 Updates equal 8 Updates bit for bit: accumulation, FrameIdx()
    and the ray counts; intersect_time() reports the finished occlusion query."""
    import torch
    b = O.batch(CORNELL)

    def tracer():
        sc, tr = _tracer(CORNELL)
        tr.enable_ray_counts(True)
        tr.OnResize((48, 48))
        return sc, tr
    sc, tr = tracer()
    for _ in range(8):
        tr.Update(sc)
    ref, ref_idx, ref_rc, ref_rays = tr.Accumulation(), tr.FrameIdx(), tr.ray_counts(), tr.stats()["rays"]
    tr.close()
    sc, tr = tracer()
    for _ in range(4):
        tr.Update(sc)
    got = tr.occluded(b.rays)
    assert tr.intersect_time() >= 0
    d_got = tr.occluded(torch.from_numpy(np.array(b.rays)).cuda())  # complete on return
    assert tr.intersect_time() >= 0
    assert tr.FrameIdx() == 4
    for _ in range(4):
        tr.Update(sc)
    assert tr.FrameIdx() == ref_idx == 8
    assert np.array_equal(tr.Accumulation().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(tr.ray_counts(), ref_rc) and tr.stats()["rays"] == ref_rays
    assert np.array_equal(got, b.flag) and np.array_equal(d_got.cpu().numpy(), b.flag)
    tr.close()


def test_refusals_on_a_live_tracer(have_gpu):
    """As intersect: a partitioned tracer answers the same (the scene is whole on every rank), a create_multi tracer
    refuses; a refused call leaves the output alone."""
    import raytrace2_amd as R
    from raytrace2_amd._native import lib
    b = O.batch(CORNELL)
    sc, tr = _tracer(CORNELL, (48, 48))
    tr.set_partition(8, 1, 2)
    assert np.array_equal(tr.occluded(b.rays), b.flag)
    out = np.full(4, 0x55, np.int8)
    rc = lib.rt2_tracer_occluded(tr._h, 1 << 31, b.rays.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), SEED,
                                 out.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)))
    assert rc == R._native.RT2_ERR_INVALID and lib.rt2_last_error().startswith(b"occluded: ") and (out == 0x55).all()
    tr.close()
    multi = R.RayTracer(sc, devices=[0, 0], band_h=8)
    with pytest.raises(R.Rt2Error) as e:
        multi.occluded(b.rays[:10])
    assert e.value.code == R._native.RT2_ERR_INVALID and "occluded: not on a create_multi tracer" in str(e.value)
    with pytest.raises(R.Rt2Error):
        multi.visible(b.rays[:10, 0:3], b.rays[:10, 0:3] + b.rays[:10, 4:7])
    multi.close()
