"""Ray queries on the GPU (include/rt2.h "Ray queries"): RayTracer.intersect against oracle.hit word for word on
caller-built rays over the nine parity scenes, threaded and stack traversal; against the feature pass; wave and
chunk edges; invalid rays; the device entry; no disturbance of a render; rt2_headless --pick. Every test goes
through intersect, which the library did not have before."""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from bits import f32_bits, same_bits
from conftest import ROOT, scene_path
from denoise_ref import feature_rays
from helpers import SEED
from test_gpu_parity import CASES, MODES

pytestmark = pytest.mark.gpu
F32 = np.float32
FLT_MAX = np.finfo(F32).max
SCENES = [c[0] for c in CASES]
MEDIA = ("cornell_box_volume", "book2_final_scene_10000_samples")
SPP = 16
APP = os.path.join(ROOT, "raytrace2_amd", "lib", "rt2_headless")


def _rays(o, d, tmax=FLT_MAX, time=0.0):
    """(n, 8) float32 ray records from origins (n, 3) or (3,), directions (n, 3), tmax and time (scalars or (n,))."""
    d = np.asarray(d, F32).reshape(-1, 3)
    r = np.zeros((len(d), 8), F32)
    r[:, 0:3] = np.asarray(o, F32)
    r[:, 3] = tmax
    r[:, 4:7] = d
    r[:, 7] = time
    return r


def _valid(r):
    """The numpy restatement of query.h QueryRayValid."""
    r = np.asarray(r, F32).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        m = np.abs(r[:, 4:7]).max(-1)
        return (np.isfinite(r).all(-1) & (m >= F32(2.0 ** -20)) & (m <= F32(2.0 ** 20))
                & (np.abs(r[:, 0:3]) <= F32(2.0 ** 64)).all(-1) & (r[:, 3] > F32(0.001)) & (r[:, 7] >= 0) & (r[:, 7] <= 1))


@functools.lru_cache(maxsize=None)
def _oracle(name):
    from oracle.oracle import OracleScene
    return OracleScene(scene_path(name), SEED)


def _expect(name, rays, seed):
    """The 16-float answers from oracle.hit: slots 0-9 its record, the albedo by the feature pass's rule from
    oracle.materials() and oracle.texture_value, dist in numpy float32; a miss carries the background; a ray that is
    not valid answers -1 and zeros."""
    o = _oracle(name)
    mats = o.materials()
    bg = np.array(list(o.info().background), F32)
    out = np.zeros((len(rays), 16), F32)
    ok = _valid(rays)
    for i, r in enumerate(rays):
        if not ok[i]:
            out[i, 0] = -1
            continue
        rec = o.hit(r[0:3], r[4:7], time=float(r[7]), tmin=0.001, tmax=float(r[3]), seed=seed)
        if rec[0] == 0:
            out[i, 10:13] = bg
            continue
        out[i, 0:10] = rec
        m = mats[int(rec[9])]
        if int(m[0]) == 2:
            out[i, 10:13] = 1
        elif int(m[0]) in (3, 4, 5):
            out[i, 10:13] = o.texture_value(int(m[6]), rec[2:5])[0]
        else:
            out[i, 10:13] = m[1:4]
        dp = out[i, 2:5] - r[0:3]
        out[i, 13] = np.sqrt((dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2])
    return out


@functools.lru_cache(maxsize=None)
def _family_r(name):
    """600 rays: origins uniform in a cube about the scene, unit directions, time in [0, 1), unbounded."""
    rng = np.random.default_rng(1)
    n = 600
    c, hw = (278.0, 600.0) if name.startswith("cornell_") else (0.0, 15.0)
    o = rng.uniform(c - hw, c + hw, (n, 3)).astype(F32)
    v = rng.normal(size=(n, 3))
    d = (v / np.sqrt((v * v).sum(-1, keepdims=True))).astype(F32)
    t = rng.uniform(0.0, 1.0, n).astype(F32)
    r = _rays(o, d, FLT_MAX, np.minimum(t, np.nextafter(F32(1), F32(0))))
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _batch(name):
    """One shuffled batch per scene (see test_against_the_oracle) with the oracle's answers at SEED, frozen, and the
    slices of its parts before the shuffle."""
    R0 = _family_r(name)
    e0 = _expect(name, R0, SEED)
    hit = e0[:, 0] == 1
    H, t = R0[hit], e0[hit, 1]
    parts = {"R": R0}
    half = H.copy()
    half[:, 3] = F32(0.5) * t
    parts["half"] = half
    at = H.copy()
    at[:, 3] = t
    parts["at"] = at
    below = H.copy()
    below[:, 3] = np.nextafter(t, F32(0))
    parts["below"] = below
    for key, s in (("x3.7", F32(3.7)), ("x2^-6", F32(2.0 ** -6))):
        sc = H.copy()
        sc[:, 4:7] = H[:, 4:7] * s
        parts[key] = sc
    one, two = R0[:90].copy(), R0[90:180].copy()
    for i in range(len(one)):  # one and two direction components exactly 0 (+0 and -0): infinite reciprocals
        one[i, 4 + i % 3] = F32(0.0) if i % 2 else F32(-0.0)
        two[i, 4 + i % 3] = F32(0.0)
        two[i, 4 + (i + 1) % 3] = F32(-0.0) if i % 2 else F32(0.0)
    parts["zero1"], parts["zero2"] = one, two
    # aimed along the axes at the scene from outside and from its middle, so that axis-parallel rays hit
    c = F32(278.0) if name.startswith("cornell_") else F32(0.0)
    ax = []
    for k in range(3):
        for s in (-1.0, 1.0):
            for off in ((0.0, 0.0), (37.5, -61.25), (0.3, 0.45)):
                o = np.array([c, c, c], F32)
                o[(k + 1) % 3] += F32(off[0])
                o[(k + 2) % 3] += F32(off[1])
                d = np.zeros(3, F32)
                d[k] = s
                ax.append(_rays(o, d, FLT_MAX, 0.25)[0])
                o2 = o.copy()
                o2[k] -= F32(s) * F32(2000.0 if name.startswith("cornell_") else 40.0)
                ax.append(_rays(o2, d, FLT_MAX, 0.25)[0])
    parts["axes"] = np.array(ax, F32)
    cp = _oracle(name).camera_params(32, 18, SPP)
    p00, du, dv, cc = cp[0:3], cp[3:6], cp[6:9], cp[9:12]
    x = np.arange(32).astype(F32)[None, :, None]
    y = np.arange(18).astype(F32)[:, None, None]
    pc = (p00 + x * du) + y * dv
    parts["pixels"] = _rays(cc, (pc - cc).reshape(-1, 3), FLT_MAX, 0.0)  # un-normalised pixel-centre rays
    allr = np.concatenate(list(parts.values()))
    if len(allr) % 64 == 0:
        allr = np.concatenate([allr, R0[:1]])
    assert len(allr) % 64 != 0
    perm = np.random.default_rng(2).permutation(len(allr))
    rays = np.ascontiguousarray(allr[perm])
    exp = _expect(name, rays, SEED)
    # what the oracle says about the bounded parts, asserted, not assumed
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    at0, info = 0, {}
    for key, p in parts.items():
        info[key] = exp[inv[at0:at0 + len(p)], 0].copy()
        at0 += len(p)
    rays.setflags(write=False)
    exp.setflags(write=False)
    return rays, exp, info, hit.sum()


def _tracer(name, size=None):
    import raytrace2_amd as R
    sc = R.Scene(scene_path(name), SEED)
    tr = R.RayTracer(sc, 0)
    tr.set_seed(SEED)
    tr.SetSamplesPerPixel(SPP)
    if size:
        tr.OnResize(size)
    return sc, tr


def _assert_records(got, exp, what):
    assert got.shape == exp.shape
    assert np.array_equal(got[:, 0], exp[:, 0]), f"flags differ {what}: {np.flatnonzero(got[:, 0] != exp[:, 0])[:8]}"
    bad = np.flatnonzero((f32_bits(got) != f32_bits(exp)).any(-1))
    assert bad.size == 0, f"{bad.size} records differ {what}; first {bad[0]}: {got[bad[0]]} vs {exp[bad[0]]}"


def test_oracle_batches_are_discriminating():
    """On the oracle's answers alone: every scene's batch has at least 10 % hits and 10 % misses (book 2's family R
    starts inside its ground boxes and always hits: its misses are the bounded rays), the oracle reports a miss for
    every hit ray whose tmax is halved, and the parts with zero direction components and along the axes hold hits
    and misses somewhere."""
    for name in SCENES:
        rays, exp, info, nhit = _batch(name)
        # a kernel that always answers one way cannot pass
        assert (exp[:, 0] == 1).mean() >= 0.10 and (exp[:, 0] == 0).mean() >= 0.10, name
        # tmax = fl(0.5 t): a miss everywhere (a ray whose 0.5 t is not above 0.001 is not traced at all)
        assert set(np.unique(info["half"])) <= {0.0, -1.0} and (info["half"] == 0).sum() >= 0.9 * nhit, name
        assert (info["x3.7"] == 1).mean() >= 0.9 and (info["x2^-6"] == 1).mean() >= 0.9, name
        assert (info["pixels"] == 1).any(), name
    both = np.concatenate([_batch(n)[2][k] for n in SCENES for k in ("zero1", "zero2", "axes")])
    assert (both == 1).any() and (both == 0).any()
    # quads accept t == tmax (Contains), spheres do not (Surrounds): the oracle decides, and both answers occur
    at = np.concatenate([_batch(n)[2]["at"] for n in SCENES])
    assert (at == 1).any() and (at == 0).any()


@pytest.mark.parametrize("mode", ["linear", "stack_global"])
@pytest.mark.parametrize("name", SCENES)
def test_against_the_oracle(have_gpu, monkeypatch, name, mode):
    """One batch per scene: family R; R's hits again with tmax = fl(0.5 t), with tmax = t and the float below it, with
    d scaled by 3.7 and by 2^-6; rays with one and two direction components exactly 0 and rays along the axes; the
    32x18 un-normalised pixel-centre rays; shuffled by a fixed permutation, n no multiple of 64. All 16 slots equal
    the oracle's record word for word, in the threaded program and in the stack walk; the media scenes again under
    a second seed, which changes some record."""
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    rays, exp, _, _ = _batch(name)
    sc, tr = _tracer(name)
    got = tr.intersect(rays)
    _assert_records(got, exp, f"{name} {mode}")
    assert tr.intersect_time() > 0
    if name in MEDIA:
        seed2 = SEED + 7
        got2 = tr.intersect(rays, seed=seed2)
        _assert_records(got2, _expect(name, rays, seed2), f"{name} {mode} seed 2")
        assert not same_bits(got, got2), "the seed does not reach the media"
    assert tr.stats()["overflow"] == 0
    tr.close()


@pytest.mark.parametrize("name", SCENES)
def test_against_the_feature_pass(have_gpu, name):
    """Normalised pixel-centre rays at 32x18, tmax FLT_MAX, time 0, the tracer's seed: intersect returns features()'s
    16 slots word for word, on every scene the feature pass accepts."""
    import raytrace2_amd as R
    sc, tr = _tracer(name, (32, 18))
    try:
        feat = tr.features()
    except R.Rt2Error as e:
        assert "stack" in str(e)
        tr.close()
        return
    o, d = feature_rays(sc.camera_params(32, 18, SPP), 32, 18)
    got = tr.intersect(_rays(o, d.reshape(-1, 3)))
    _assert_records(got, feat.reshape(-1, 16), name)
    tr.close()


def test_wave_and_chunk_edges(have_gpu, monkeypatch):
    rays, exp, _, _ = _batch("cornell_box_original")
    sc, tr = _tracer("cornell_box_original")
    full = tr.intersect(rays)
    _assert_records(full, exp, "full")
    for n in (1, 63, 64, 65, 1000):
        assert same_bits(tr.intersect(rays[:n]), full[:n]), n
    monkeypatch.setenv("RT2_QUERY_CHUNK", "128")
    assert same_bits(tr.intersect(rays[:1000]), full[:1000])
    monkeypatch.setenv("RT2_QUERY_CHUNK", "100")  # rounded up to 128
    assert same_bits(tr.intersect(rays[:257]), full[:257])
    monkeypatch.delenv("RT2_QUERY_CHUNK")
    empty = tr.intersect(np.zeros((0, 8), F32))
    assert empty.shape == (0, 16)
    tr.close()


@pytest.mark.parametrize("name", ["cornell_box_original", "final_render_book_1"])
def test_invalid_rays_stay_out(have_gpu, name):
    """Every fourth ray invalid (NaN and inf words, d = 0, tmax = 0, time = 2, an origin beyond the bound, a direction
    beyond its bounds): those answer -1 and zeros, the others what they answer without them."""
    import raytrace2_amd as R
    rays, exp, _, _ = _batch(name)
    keep = np.flatnonzero(_valid(rays))[:900]
    good, exp = np.array(rays[keep]), exp[keep]
    assert len(good) == 900
    bad = []
    for k in range(300):
        r = good[k].copy()
        c = k % 12
        if c < 8:
            r[c] = (np.nan, np.inf, -np.inf)[k % 3]
        elif c == 8:
            r[4:7] = 0
        elif c == 9:
            r[3] = 0
        elif c == 10:
            r[7] = 2
        else:
            r[k % 3] = F32(2.0 ** 64) * F32(1.5) if k % 2 else -np.nextafter(F32(2.0 ** 64), F32(np.inf))
        bad.append(r)
    bad += [np.concatenate([good[0][:4], F32([2.0 ** 21, 0, 0]), good[0][7:]]),
            np.concatenate([good[0][:4], F32([2.0 ** -21, 0, -2.0 ** -22]), good[0][7:]])]
    bad = np.array(bad, F32)
    assert not _valid(bad).any() and not R.ray_valid(bad).any()
    mixed = np.zeros((len(good) + len(good) // 3, 8), F32)
    is_bad = np.arange(len(mixed)) % 4 == 3
    mixed[~is_bad] = good
    mixed[is_bad] = bad[np.arange(is_bad.sum()) % len(bad)]
    sc, tr = _tracer(name)
    got = tr.intersect(mixed)
    alone = tr.intersect(good)
    _assert_records(alone, exp, "valid alone")
    assert same_bits(got[~is_bad], alone)
    assert (got[is_bad, 0] == -1).all() and (f32_bits(got[is_bad, 1:]) == 0).all()
    assert np.array_equal(R.ray_valid(mixed), ~is_bad)
    assert tr.stats()["overflow"] == 0
    tr.close()


def test_device_entry(have_gpu):
    import torch
    from raytrace2_amd._native import lib
    rays, exp, _, _ = _batch("cornell_box_original")
    sc, tr = _tracer("cornell_box_original")
    host = tr.intersect(rays)
    d_rays = torch.from_numpy(np.array(rays)).cuda()
    d_out = tr.intersect(d_rays)
    assert d_out.is_cuda and same_bits(d_out.cpu().numpy(), host)
    assert tr.intersect_time() > 0
    # the entry itself blocks nowhere: host_waits moves only by what stats() itself adds
    out2 = torch.empty((len(rays), 16), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    w0 = tr.stats()["host_waits"]
    w1 = tr.stats()["host_waits"]
    rc = lib.rt2_tracer_intersect_device(tr._h, len(rays), ctypes.c_void_p(d_rays.data_ptr()), SEED,
                                         ctypes.c_void_p(out2.data_ptr()))
    assert rc == 0
    w2 = tr.stats()["host_waits"]
    assert w2 - w1 == w1 - w0
    tr.synchronize()
    assert same_bits(out2.cpu().numpy(), host) and tr.intersect_time() > 0
    tr.close()


def test_no_disturbance(have_gpu):
    """4 Updates, one intersect, 4 Updates equal 8 Updates bit for bit; features() before and after are equal; a
    fresh tracer answers before OnResize, a partitioned one answers the same, a create_multi tracer refuses."""
    import raytrace2_amd as R
    rays, exp, _, _ = _batch("cornell_box_original")
    sc, tr = _tracer("cornell_box_original", (48, 48))
    for _ in range(8):
        tr.Update(sc)
    ref, ref_idx = tr.Accumulation(), tr.FrameIdx()
    tr.close()
    sc, tr = _tracer("cornell_box_original", (48, 48))
    f0 = tr.features()
    for _ in range(4):
        tr.Update(sc)
    got = tr.intersect(rays[:500])
    assert tr.FrameIdx() == 4
    for _ in range(4):
        tr.Update(sc)
    assert tr.FrameIdx() == ref_idx == 8
    assert same_bits(tr.Accumulation(), ref)
    assert same_bits(tr.features(), f0)
    _assert_records(got, exp[:500], "between updates")
    tr.set_partition(8, 1, 2)
    assert same_bits(tr.intersect(rays[:500]), got)
    tr.close()
    sc, tr = _tracer("cornell_box_original")  # no OnResize
    assert same_bits(tr.intersect(rays[:500]), got)
    tr.close()
    multi = R.RayTracer(sc, devices=[0, 0], band_h=8)
    with pytest.raises(R.Rt2Error) as e:
        multi.intersect(rays[:10])
    assert e.value.code == R._native.RT2_ERR_INVALID
    multi.close()


def test_headless_pick(have_gpu):
    r = subprocess.run([APP, scene_path("cornell_box_original"), "--pick", "16", "9", "--size", "32", "18"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    doc = json.loads(r.stdout.strip().splitlines()[-1])
    sc, tr = _tracer("cornell_box_original", (32, 18))
    assert doc["pick"] == [16, 9] and doc["size"] == [32, 18]
    assert same_bits(np.array(doc["record"], F32), tr.features()[9, 16])
    tr.close()
