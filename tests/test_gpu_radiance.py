"""Radiance queries on the GPU (include/rt2.h "Radiance queries"): RayTracer.radiance on the camera's
own rays (tests/radiance_ref.py) bit for bit against the oracle's render of the same frames and against the tracer's
own accumulation and ray counts, in the threaded program and in the stack walk; max_depth, a second seed, book 2
without its list tree; samples summed in the kernel against single-sample answers under forced launch splits and
without refill; default stream words and chunks; arbitrary rays' first segment against intersect; invalid rays, the
device entry's exact words, no disturbance of a render, a partition, the refusals and rt2_headless --radiance. Every
test goes through a radiance entry, which the library did not have before."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import edge_rays as E
import radiance_ref as Rr
from bits import refused, same_bits
from conftest import ROOT
from helpers import SEED
from test_gpu_ambient import _bad_records
from test_gpu_parity import MODES
from test_gpu_query import _tracer, _valid

pytestmark = pytest.mark.gpu
F32 = np.float32
FLT_MAX = np.finfo(F32).max
KERNELS = ["linear", "stack_global"]
CORNELL = "cornell_box_original"
VOLUME = "cornell_box_volume"
BOOK2 = "book2_final_scene_10000_samples"
APP = os.path.join(ROOT, "raytrace2_amd", "lib", "rt2_headless")
FILL = 0x55555555
LIGHT = 4  # rt2_layout.h kMatDiffuseLight


def _set(monkeypatch, mode):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)


def _frames(tr, name, **kw):
    """One ray per (pixel, frame) of the case, samples = 1: (frames, n, 3) sums and (frames, n) counts."""
    rays, streams, fd = Rr.case_rays(name, kw.get("seed", SEED))
    f, n = rays.shape[:2]
    assert f * n <= 5376  # (book 1's 24x14 x 16 frames; 4,096 or fewer elsewhere)
    got, cnt = tr.radiance(rays.reshape(-1, 8), samples=1, streams=streams.reshape(-1, 2), first_draw=fd, counts=True, **kw)
    return got.reshape(f, n, 3), cnt.reshape(f, n)


def _explain(what, name, got, cnt, want_acc, want_rc, seed=SEED):
    """The per-pixel frame-order sum of got equals want_acc bit for bit and the counts' sum want_rc; a failure names
    the ray, its stream, the sample and both answers."""
    rays, streams, fd = Rr.case_rays(name, seed)
    acc = Rr.frame_sum(got)
    total = cnt.astype(np.uint64).sum(0)
    want_acc, want_rc = np.asarray(want_acc).reshape(-1, 3), np.asarray(want_rc).reshape(-1)
    bad = np.flatnonzero((acc.view(np.uint32) != want_acc.view(np.uint32)).any(-1) | (total != want_rc))
    if not bad.size:
        return
    i = int(bad[0])
    pytest.fail(f"{what}: {bad.size} of {len(acc)} pixels differ; first: pixel {i}: sum {acc[i].tolist()} rays {int(total[i])}, "
                f"expected {want_acc[i].tolist()} rays {int(want_rc[i])}\n  its rays: " +
                "; ".join(f"ray {rays[k, i].tolist()} stream {streams[k, i].tolist()} sample 0 first_draw {fd} -> "
                          f"{got[k, i].tolist()} ({int(cnt[k, i])} rays)" for k in range(min(3, len(got)))))


@pytest.mark.parametrize("mode", KERNELS)
@pytest.mark.parametrize("name", Rr.NAMES)
def test_render_equality(have_gpu, monkeypatch, name, mode):
    """The case's (pixel, frame) rays, summed per pixel in frame order on the host, equal the oracle's render of frames
    3..18 and its ray counts, and continue the tracer's own accumulation and ray counts from frame 3 to frame 19; then
    max_depth 5 (every scene but light_scene1) and max_depth 1."""
    _set(monkeypatch, mode)
    _, w, h = Rr.CASE[name][:3]
    o_acc, o_rc = Rr.case_render(name)
    assert int((o_acc.reshape(-1, 3) != 0).any(-1).sum()) >= Rr.MIN_INFORMATIVE
    sc, tr = _tracer(name)
    tr.SetSamplesPerPixel(Rr.SPP)
    tr.enable_ray_counts(True)
    tr.OnResize((w, h))
    got, cnt = _frames(tr, name)
    _explain(f"{name} {mode} against the oracle", name, got, cnt, o_acc, o_rc)
    assert tr.radiance_time() >= 0
    # the tracer's own frames: 0..2, then 3..18 continue that accumulation in frame order
    tr.Render(Rr.FRAME0)
    acc3, rc3 = tr.Accumulation().reshape(-1, 3), tr.ray_counts().reshape(-1).astype(np.uint64)
    tr.Render(Rr.FRAMES)
    acc19, rc19 = tr.Accumulation().reshape(-1, 3), tr.ray_counts().reshape(-1).astype(np.uint64)
    cont = np.array(acc3, F32)
    for s in got:
        cont = (cont + s).astype(F32)
    assert same_bits(cont, acc19), f"{name} {mode}: the tracer's own accumulation"
    assert np.array_equal(rc3 + cnt.astype(np.uint64).sum(0), rc19), f"{name} {mode}: the tracer's own ray counts"
    for depth in ([5] if name in Rr.DEPTH5 else []) + [1]:
        d_acc, d_rc = Rr.case_render(name, depth)
        g, c = _frames(tr, name, max_depth=depth)
        _explain(f"{name} {mode} max_depth {depth}", name, g, c, d_acc, d_rc)
        if depth == 1:
            assert (c == 1).all()
    assert tr.stats()["overflow"] == 0
    tr.close()


@pytest.mark.parametrize("mode", KERNELS)
def test_second_seed_and_list_tree(have_gpu, monkeypatch, mode):
    """Cornell volume under a second seed given to the call and not to the tracer; book 2 without the list tree."""
    _set(monkeypatch, mode)
    seed2 = SEED + 7
    sc, tr = _tracer(VOLUME)
    got, cnt = _frames(tr, VOLUME, seed=seed2)
    acc, rc = Rr.case_render(VOLUME, 50, seed2)
    _explain(f"{VOLUME} seed 2 {mode}", VOLUME, got, cnt, acc, rc, seed2)
    assert not same_bits(acc, Rr.case_render(VOLUME)[0])
    tr.close()
    monkeypatch.setenv("RT2_NO_LIST_ACCEL", "1")  # read at scene load
    sc, tr = _tracer(BOOK2)
    got, cnt = _frames(tr, BOOK2)
    _explain(f"{BOOK2} {mode} without the list tree", BOOK2, got, cnt, *Rr.case_render(BOOK2))
    tr.close()


@pytest.mark.parametrize("mode", KERNELS)
def test_samples_in_the_kernel(have_gpu, monkeypatch, mode):
    """37 rays with k = 1, 2, 63, 64, 65, 130 samples from frame word f0: the ordered float32 sum of the k
    single-sample answers at f0 .. f0 + k - 1 and the sum of their counts; the same bytes under forced launch splits
    (RT2_RADIANCE_ITEMS 64 and 100) and without refill; streams=None equals (i, 0x40000000), whole and in chunks."""
    _set(monkeypatch, mode)
    rays, streams, fd = Rr.case_rays(CORNELL)
    pick = np.flatnonzero((Rr.case_render(CORNELL)[0].reshape(-1, 3) != 0).any(-1))[:37]
    assert pick.size == 37
    r, st = np.array(rays[0, pick]), np.array(streams[0, pick])
    f0 = 1000
    st[:, 1] = f0
    sc, tr = _tracer(CORNELL)
    single, scnt = [], []
    for s in range(130):
        stk = st.copy()
        stk[:, 1] = f0 + s
        g, c = tr.radiance(r, samples=1, streams=stk, first_draw=fd, counts=True)
        single.append(g)
        scnt.append(c)
    single, scnt = np.array(single), np.array(scnt, np.uint64)
    assert len(np.unique(scnt)) >= 10 and (single != 0).any(-1).sum() >= 100
    whole = {}
    for k in (1, 2, 63, 64, 65, 130):
        want, wcnt = Rr.frame_sum(single[:k]), scnt[:k].sum(0)
        g, c = tr.radiance(r, samples=k, streams=st, first_draw=fd, counts=True)
        bad = np.flatnonzero((g.view(np.uint32) != want.view(np.uint32)).any(-1) | (c != wcnt))
        assert not bad.size, (f"{k} samples {mode}: ray {int(bad[0])} {r[bad[0]].tolist()} stream {st[bad[0]].tolist()}: "
                              f"{g[bad[0]].tolist()} / {int(c[bad[0]])} rays, expected {want[bad[0]].tolist()} / {int(wcnt[bad[0]])}")
        whole[k] = (g, c)
        assert same_bits(tr.radiance(r, samples=k, streams=st, first_draw=fd), g)  # (without counts)
    for env, val in (("RT2_RADIANCE_ITEMS", "64"), ("RT2_RADIANCE_ITEMS", "100"), ("RT2_RADIANCE_ITEMS", "7"),
                     ("RT2_RADIANCE_REFILL", "0")):
        monkeypatch.setenv(env, val)
        for k in (1, 2, 63, 64, 65, 130):
            g, c = tr.radiance(r, samples=k, streams=st, first_draw=fd, counts=True)
            assert same_bits(g, whole[k][0]) and np.array_equal(c, whole[k][1]), (env, val, k)
        monkeypatch.delenv(env)
    # default stream words
    big = np.tile(r, (6, 1))[:200]
    explicit = np.stack([np.arange(200, dtype=np.uint32), np.full(200, Rr.FRAME_WORD0, np.uint32)], -1)
    want = tr.radiance(big, samples=3, streams=explicit, counts=True)
    got = tr.radiance(big, samples=3, counts=True)
    assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])
    monkeypatch.setenv("RT2_QUERY_CHUNK", "64")
    got = tr.radiance(big, samples=3, counts=True)
    assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])
    got = tr.radiance(big, samples=3, streams=explicit, counts=True)
    assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])
    tr.close()


@pytest.mark.parametrize("mode", KERNELS)
def test_lanes_refill_from_their_wave_s_block(have_gpu, monkeypatch, mode):
    """A launch above 64 x 8,192 items, where a wave's block is longer than 64 items (launch_plan.h RadianceWaveItems)
    and a lane whose path ended takes further ones: 37 rays x 40,000 samples are 1.48 M items in blocks of 192, three
    per lane. Every sample is also asked on its own, as one ray of a samples = 1 call cut into launches of 37,000
    items (one item per lane, the launch shape held against the oracle above); the refilled answer equals the float32
    ordered sum of those and the sum of their counts, and the same bytes come back without refill and from sample
    ranges short enough to have none."""
    _set(monkeypatch, mode)
    rays, streams, fd = Rr.case_rays(CORNELL)
    pick = np.flatnonzero((Rr.case_render(CORNELL)[0].reshape(-1, 3) != 0).any(-1))[:37]
    r, st = np.array(rays[1, pick]), np.array(streams[1, pick])
    n, k, f0 = len(r), 40000, 5000
    assert n == 37 and n * k > 2 * 64 * 8192
    st[:, 1] = f0
    sc, tr = _tracer(CORNELL)
    # sample s of ray i as ray s * n + i of one call
    each = np.tile(r, (k, 1))
    each_st = np.tile(st, (k, 1))
    each_st[:, 1] = f0 + np.repeat(np.arange(k, dtype=np.uint32), n)
    monkeypatch.setenv("RT2_RADIANCE_ITEMS", str(n * 1000))
    single, scnt = tr.radiance(each, samples=1, streams=each_st, first_draw=fd, counts=True)
    single, scnt = single.reshape(k, n, 3), scnt.reshape(k, n)
    assert len(np.unique(scnt)) >= 20  # (paths of very different lengths share the waves)
    want, wcnt = Rr.frame_sum(single), scnt.astype(np.uint64).sum(0)
    ranges = tr.radiance(r, samples=k, streams=st, first_draw=fd, counts=True)  # 40 sample ranges of 1,000
    monkeypatch.delenv("RT2_RADIANCE_ITEMS")
    got, cnt = tr.radiance(r, samples=k, streams=st, first_draw=fd, counts=True)
    monkeypatch.setenv("RT2_RADIANCE_REFILL", "0")
    plain = tr.radiance(r, samples=k, streams=st, first_draw=fd, counts=True)
    for what, (g, c) in (("with refill", (got, cnt)), ("without refill", plain), ("in sample ranges", ranges)):
        bad = np.flatnonzero((g.view(np.uint32) != want.view(np.uint32)).any(-1) | (c != wcnt))
        assert not bad.size, (f"{mode} {what}: ray {int(bad[0])} {r[bad[0]].tolist()} stream {st[bad[0]].tolist()} samples {k}: "
                              f"{g[bad[0]].tolist()} / {int(c[bad[0]])} rays, expected {want[bad[0]].tolist()} / {int(wcnt[bad[0]])}")
    assert (want != 0).all(-1).sum() >= 30
    tr.close()


@pytest.mark.parametrize("mode", KERNELS)
@pytest.mark.parametrize("name", [s for s in E.SCENES if s not in E.MEDIA])
def test_first_segment_of_arbitrary_rays(have_gpu, monkeypatch, name, mode):
    """The edge batch (bounded tmax among it) at max_depth 1, first_draw 0, any stream: the background on intersect's
    miss, the record's albedo where its material is a diffuse_light, else 0; exactly, with one ray cast."""
    _set(monkeypatch, mode)
    b = E.batch(name)
    rays = np.array(b.rays, F32)
    assert (rays[:, 3] < FLT_MAX).sum() >= 10
    sc, tr = _tracer(name)
    rec = tr.intersect(rays)
    mats = Rr.oracle(name).materials()  # (rt2_scene_materials' rows: type, albedo, ...)
    assert (rec[:, 0] >= 0).all()
    want = np.zeros((len(rays), 3), F32)
    miss = rec[:, 0] == 0
    light = ~miss & np.array([int(mats[int(m)][0]) == LIGHT for m in rec[:, 9]])
    want[miss | light] = rec[miss | light, 10:13]
    assert miss.sum() >= 10 and (~miss).sum() >= 10
    streams = np.stack([np.arange(len(rays), dtype=np.uint32) * 977, np.arange(len(rays), dtype=np.uint32) % 50], -1)
    for st in (None, streams):
        got, cnt = tr.radiance(rays, streams=st, max_depth=1, counts=True)
        bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(-1))
        assert not bad.size, (f"{name} {mode}: ray {int(bad[0])} {rays[bad[0]].tolist()}: {got[bad[0]].tolist()}, "
                              f"expected {want[bad[0]].tolist()} from record {rec[bad[0]].tolist()}")
        assert (cnt == 1).all()
    tr.close()


@pytest.mark.parametrize("mode", KERNELS)
def test_invalid_rays_stay_out(have_gpu, monkeypatch, mode):
    """Invalid records at every fourth place answer 0, 0, 0 and 0xFFFFFFFF and their neighbours answer what they
    answer alone at their own stream words; a batch of only invalid records."""
    _set(monkeypatch, mode)
    rays, streams, fd = Rr.case_rays(CORNELL)
    good = np.array(rays[2, :120])
    bad = _bad_records(good[:40])
    assert not _valid(bad).any()
    mixed = np.zeros((160, 8), F32)
    is_bad = np.arange(160) % 4 == 3
    mixed[~is_bad], mixed[is_bad] = good, bad
    st = np.stack([np.arange(160, dtype=np.uint32), np.full(160, 5, np.uint32)], -1)
    sc, tr = _tracer(CORNELL)
    want, wcnt = tr.radiance(good, samples=5, streams=st[~is_bad], first_draw=fd, counts=True)
    got, cnt = tr.radiance(mixed, samples=5, streams=st, first_draw=fd, counts=True)
    assert same_bits(got[~is_bad], want) and np.array_equal(cnt[~is_bad], wcnt)
    assert (got[is_bad].view(np.uint32) == 0).all() and (cnt[is_bad] == Rr.INVALID).all()
    assert (want != 0).any() and len(np.unique(wcnt)) > 5
    g, c = tr.radiance(bad, samples=3, counts=True)
    assert (g.view(np.uint32) == 0).all() and (c == Rr.INVALID).all()
    g, c = tr.radiance(np.tile(bad, (2, 1))[:64], samples=64, counts=True)
    assert (g.view(np.uint32) == 0).all() and (c == Rr.INVALID).all()
    e = tr.radiance(np.zeros((0, 8), F32), counts=True)
    assert e[0].shape == (0, 3) and e[1].shape == (0,) and e[1].dtype == np.uint32
    tr.close()


def test_device_entry_writes_exactly_its_words(have_gpu):
    """The device entry into 3 (n + 64) and n + 64 words of 0x55555555: the answers in the first n, the last 64
    untouched; no host wait; the tensor form."""
    import torch
    from raytrace2_amd._native import RadianceParams, lib
    rays, streams, fd = Rr.case_rays(CORNELL)
    r, st = np.array(rays.reshape(-1, 8)[:300]), np.array(streams.reshape(-1, 2)[:300])
    sc, tr = _tracer(CORNELL)
    want, wcnt = tr.radiance(r, samples=4, streams=st, first_draw=fd, counts=True)
    d_r, d_st = torch.from_numpy(r).cuda(), torch.from_numpy(st.view(np.int32)).cuda()
    t_got, t_cnt = tr.radiance(d_r, samples=4, streams=d_st, first_draw=fd, counts=True)
    assert t_got.is_cuda and t_cnt.dtype == torch.int32
    assert same_bits(t_got.cpu().numpy(), want) and np.array_equal(t_cnt.cpu().numpy().view(np.uint32), wcnt)
    assert tr.radiance_time() >= 0
    prm = RadianceParams(4, 0, fd)
    for n in (1, 65, 257):
        out = torch.full((n + 64, 3), FILL, dtype=torch.int32, device="cuda")
        cnt = torch.full((n + 64,), FILL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        waits = tr.stats()["host_waits"]
        assert lib.rt2_tracer_radiance_device(tr._h, n, ctypes.c_void_p(d_r.data_ptr()), ctypes.c_void_p(d_st.data_ptr()),
                                              ctypes.byref(prm), SEED, ctypes.c_void_p(out.data_ptr()),
                                              ctypes.c_void_p(cnt.data_ptr())) == 0
        assert tr.stats()["host_waits"] == waits  # (it only enqueues)
        tr.synchronize()
        g, c = out.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
        assert np.array_equal(g[:n], want[:n].view(np.uint32)) and (g[n:] == FILL).all(), n
        assert np.array_equal(c[:n], wcnt[:n]) and (c[n:] == FILL).all(), n
    tr.close()


def test_no_disturbance_repeatable_and_a_partition(have_gpu):
    """4 Updates, a call by each entry, 4 Updates equal 8 Updates bit for bit; features() is unchanged; a second call
    returns the same bytes; a set_partition(2, 1, 3) tracer answers as the whole one."""
    import torch
    rays, streams, fd = Rr.case_rays(CORNELL)
    r, st = np.array(rays.reshape(-1, 8)[:500]), np.array(streams.reshape(-1, 2)[:500])

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
    feats = tr.features()
    got, cnt = tr.radiance(r, samples=3, streams=st, first_draw=fd, counts=True)
    again = tr.radiance(r, samples=3, streams=st, first_draw=fd, counts=True)
    assert same_bits(again[0], got) and np.array_equal(again[1], cnt)
    d = tr.radiance(torch.from_numpy(r).cuda(), samples=3, streams=torch.from_numpy(st.view(np.int32)).cuda(),
                    first_draw=fd, counts=True)
    assert same_bits(d[0].cpu().numpy(), got) and np.array_equal(d[1].cpu().numpy().view(np.uint32), cnt)
    assert same_bits(tr.features(), feats)
    assert tr.FrameIdx() == 4
    for _ in range(4):
        tr.Update(sc)
    assert tr.FrameIdx() == ref_idx == 8
    assert same_bits(tr.Accumulation(), ref)
    assert np.array_equal(tr.ray_counts(), ref_rc) and tr.stats()["rays"] == ref_rays
    tr.set_partition(2, 1, 3)
    part = tr.radiance(r, samples=3, streams=st, first_draw=fd, counts=True)
    assert same_bits(part[0], got) and np.array_equal(part[1], cnt)
    tr.close()


def test_refusals_on_a_live_tracer(have_gpu):
    """Every refusal on a tracer handle; a refused call leaves the output alone; a create_multi tracer refuses."""
    import raytrace2_amd as R
    from raytrace2_amd._native import RadianceParams, lib
    INVALID = R._native.RT2_ERR_INVALID
    rays, streams, fd = Rr.case_rays(CORNELL)
    r, st = np.array(rays[0, :10]), np.array(streams[0, :10])
    sc, tr = _tracer(CORNELL)  # (before on_resize)
    assert (tr.radiance(r, counts=True)[1] >= 1).all()
    out = np.full((10, 3), FILL, np.uint32)
    fp, up = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint32)
    po, pr, ps = out.ctypes.data_as(fp), r.ctypes.data_as(fp), st.ctypes.data_as(up)

    def call(n=10, rays=pr, streams=ps, prm=None, o=po, h=tr._h):
        return lib.rt2_tracer_radiance(h, n, rays, streams, ctypes.byref(prm) if prm else None, SEED, o, None)
    for prm in (RadianceParams(0, 0, 0), RadianceParams(65536, 0, 0), RadianceParams(1, -1, 0), RadianceParams(1, 65536, 0),
                RadianceParams(1, 0, 9)):
        assert call(prm=prm) == INVALID and lib.rt2_last_error().startswith(b"radiance: need 1 <= samples")
    for n in (-1, 1 << 31):
        assert call(n=n) == INVALID and lib.rt2_last_error().startswith(b"radiance: need 0 <= n < 2^31")
    assert call(rays=None) == INVALID and call(o=None) == INVALID and call(h=None) == INVALID
    wrap = st.copy()
    wrap[7, 1] = 0xFFFFFFFE
    assert call(streams=wrap.ctypes.data_as(up), prm=RadianceParams(3, 0, 0)) == INVALID
    assert b"passes 2^32 at ray 7" in lib.rt2_last_error()
    assert call(streams=wrap.ctypes.data_as(up), prm=RadianceParams(2, 0, 0)) == 0  # (0xFFFFFFFE + 2 = 2^32 fits)
    out[:] = FILL
    assert call(n=0) == 0 and (out == FILL).all()
    refused(lambda: tr.radiance(r, samples=0))
    tr.close()
    multi = R.RayTracer(sc, devices=[0, 0], band_h=8)
    multi.OnResize((16, 16))
    e = refused(lambda: multi.radiance(r))
    assert "radiance: not on a create_multi tracer" in str(e)
    multi.close()


def test_refusals_for_the_stack_depth_and_of_the_device_entry(have_gpu, tmp_path, monkeypatch):
    """A scene whose stack walk needs more than the kernel's 24 entries is served by the threaded program and refused
    by both entries without it, as intersect refuses it; the device entry's argument refusals on a live tracer leave
    the output alone."""
    import torch
    import raytrace2_amd as R
    from raytrace2_amd._native import RadianceParams, lib
    from test_loader import _graded_list
    INVALID = R._native.RT2_ERR_INVALID
    path = _graded_list(str(tmp_path / "nest.json"), nest=7)
    sc = R.Scene(path, SEED)
    assert sc.info().max_stack > 24 and sc.info().linear_steps > 0
    q = np.array([[0, 1, -20, FLT_MAX, 0, 0, 1, 0], [0, 5, -20, FLT_MAX, 0.1, -0.1, 1, 0.5]], F32)
    d_q = torch.from_numpy(q).cuda()
    out = torch.full((2, 3), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def device(tr, n=2, rays=d_q, prm=None, o=out):
        return lib.rt2_tracer_radiance_device(tr._h, n, ctypes.c_void_p(rays.data_ptr()) if rays is not None else None, None,
                                              ctypes.byref(prm) if prm else None, SEED,
                                              ctypes.c_void_p(o.data_ptr()) if o is not None else None, None)
    tr = R.RayTracer(sc, 0)
    got, cnt = tr.radiance(q, samples=4, counts=True)
    assert (cnt >= 4).all() and (cnt != Rr.INVALID).all()
    for prm in (RadianceParams(0, 0, 0), RadianceParams(65536, 0, 0), RadianceParams(1, 65536, 0), RadianceParams(1, 0, 9)):
        assert device(tr, prm=prm) == INVALID and lib.rt2_last_error().startswith(b"radiance_device: need 1 <= samples")
    for n in (-1, 1 << 31):
        assert device(tr, n=n) == INVALID and b"radiance_device: need 0 <= n < 2^31" in lib.rt2_last_error()
    assert device(tr, rays=None) == INVALID and device(tr, o=None) == INVALID
    assert device(tr, n=0) == 0
    tr.synchronize()
    assert (out.cpu().numpy() == FILL).all()
    assert device(tr, prm=RadianceParams(4, 0, 0)) == 0
    tr.synchronize()
    assert same_bits(out.cpu().numpy().view(F32), got)
    tr.close()
    monkeypatch.setenv("RT2_NO_LINEAR", "1")
    tr = R.RayTracer(sc, 0)
    e = refused(lambda: tr.intersect(q))
    assert "intersect: the scene needs a traversal stack" in str(e)
    e = refused(lambda: tr.radiance(q))
    assert "radiance: the scene needs a traversal stack" in str(e)
    out.fill_(FILL)
    torch.cuda.synchronize()
    assert device(tr) == INVALID and lib.rt2_last_error().startswith(b"radiance_device: the scene needs a traversal stack")
    tr.synchronize()
    assert (out.cpu().numpy() == FILL).all()
    tr.close()


def test_headless_radiance(have_gpu):
    """rt2_headless --radiance prints the mean and the ray count of the Python call on the same ray: straight up at the
    Cornell box's light, so every sample is its emission after one ray."""
    q = np.array([[278, 100, 280, FLT_MAX, 0, 1, 0, 0]], F32)
    assert (Rr.depth1_from_hits(CORNELL, q) == 15).all()
    args = [repr(float(v)) for v in (*q[0, 0:3], *q[0, 4:7])]
    r = subprocess.run([APP, E.scene_file(CORNELL), "--radiance", *args, "--samples", "64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    doc = json.loads(r.stdout.strip().splitlines()[-1])
    sc, tr = _tracer(CORNELL)
    got, cnt = tr.radiance(q, samples=64, counts=True)
    tr.close()
    mean = (got[0] / F32(64)).astype(F32)
    assert doc["samples"] == 64 and doc["rays"] == int(cnt[0]) == 64
    assert same_bits(np.array(doc["radiance"], F32), mean) and (mean == 15).all()
    # and a ray that bounces: from the camera's side into the room
    args = ["278", "278", "-800", "0.1", "-0.2", "1"]
    r = subprocess.run([APP, E.scene_file(CORNELL), "--radiance", *args, "--samples", "16"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    doc = json.loads(r.stdout.strip().splitlines()[-1])
    sc, tr = _tracer(CORNELL)
    got, cnt = tr.radiance(np.array([[278, 278, -800, FLT_MAX, 0.1, -0.2, 1, 0]], F32), samples=16, counts=True)
    tr.close()
    assert doc["rays"] == int(cnt[0]) > 16 and same_bits(np.array(doc["radiance"], F32), (got[0] / F32(16)).astype(F32))
