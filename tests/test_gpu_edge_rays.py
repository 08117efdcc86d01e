"""The query kernel at the decision boundaries (tests/edge_rays.py): RayTracer.intersect on rays an ulp either side
of a silhouette and of either end of the interval, rays leaving a surface, rays aimed at corners and edges, and
the authored scene's ties, tangents and in-plane rays in both node orders. The kernels do not evaluate Hit as the
reference does (the QUADAA rectangle test, the box-level test with its certificate and fallback, div_by_inv, the
sphere root, the padded list tree, the normal under a transform), and random rays do not land where that shows.
All 16 slots against oracle.hit word for word, slots 0-9 against the compiled reference's recorded answers
(tests/golden/ref/*_edges.npy) without any oracle, in the threaded program and in the stack walk.
tests/test_edge_rays_host.py shows on the CPU that the batches are what they claim."""
import functools
import os

import numpy as np
import pytest

import edge_rays as E
from bits import f32_bits
from conftest import ROOT
from helpers import SEED
from test_gpu_parity import MODES
from test_gpu_query import _assert_records, _expect, _tracer

pytestmark = pytest.mark.gpu
REF = os.path.join(ROOT, "tests", "golden", "ref")
ALL = E.SCENES + list(E.TIES)
KERNELS = ["linear", "stack_global"]
EDGE_FILES = sorted(f[:-len("_edges.npy")] for f in os.listdir(REF) if f.endswith("_edges.npy"))
BOOK2 = "book2_final_scene_10000_samples"


@functools.lru_cache(maxsize=None)
def _expected(name, seed):
    """The oracle's 16 slots on the scene's batch, once for every test and mode."""
    e = _expect(E.scene_file(name), E.batch(name).rays, seed)
    e.setflags(write=False)
    return e


def _describe(name, what, b, got, exp, bad):
    """A failure's message: the class, the ray, its pair partner and both records."""
    i = int(bad[0])
    lines = [f"{name} {what}: {bad.size} of {len(got)} records differ, by class "
             f"{ {str(c): int((b.cls[bad] == c).sum()) for c in np.unique(b.cls[bad])} }",
             f"first: ray {i} of class {b.cls[i]}: {b.rays[i].tolist()}",
             f"  kernel   {got[i].tolist()}", f"  expected {exp[i].tolist()}"]
    j = int(b.pair[i])
    if j >= 0:
        lines += [f"its pair partner, ray {j}: {b.rays[j].tolist()}",
                  f"  kernel   {got[j].tolist()}", f"  expected {exp[j].tolist()}"]
    return "\n".join(lines)


def _check(name, what, b, got, exp):
    bad = np.flatnonzero((f32_bits(got) != f32_bits(exp)).any(-1))
    if bad.size:
        pytest.fail(_describe(name, what, b, got, exp, bad))
    _assert_records(got, exp, f"{name} {what}")


def _set(monkeypatch, mode):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("mode", KERNELS)
@pytest.mark.parametrize("name", ALL)
def test_against_the_oracle(have_gpu, monkeypatch, name, mode):
    """Every ray of the scene's batch: all 16 slots equal oracle.hit's answer word for word; the media scenes again
    under a second seed; book 2 again without the list acceleration; no stack overflow."""
    _set(monkeypatch, mode)
    b = E.batch(name)
    sc, tr = _tracer(E.scene_file(name))
    _check(name, mode, b, tr.intersect(b.rays), _expected(name, SEED))
    if name in E.MEDIA:
        _check(name, f"{mode} seed 2", b, tr.intersect(b.rays, seed=SEED + 7), _expected(name, SEED + 7))
    assert tr.stats()["overflow"] == 0
    tr.close()
    if name == BOOK2:
        monkeypatch.setenv("RT2_NO_LIST_ACCEL", "1")  # read at scene load
        sc, tr = _tracer(E.scene_file(name))
        _check(name, f"{mode} without the list tree", b, tr.intersect(b.rays), _expected(name, SEED))
        assert tr.stats()["overflow"] == 0
        tr.close()


@pytest.mark.parametrize("mode", KERNELS)
@pytest.mark.parametrize("name", EDGE_FILES)
def test_against_the_reference(have_gpu, monkeypatch, name, mode):
    """The rays recorded in <scene>_edges.npy: slots 0-9 equal the compiled reference's own Hit bit for bit (a miss
    is recorded as zeros, and answers its flag and nine zeros). No oracle is involved."""
    _set(monkeypatch, mode)
    fx = np.load(os.path.join(REF, name + "_edges.npy"))
    assert fx.dtype == np.float32 and fx.shape[1] == 18 and 0 < len(fx) <= E.FIXTURE_RAYS
    rays, ref = np.ascontiguousarray(fx[:, :8]), fx[:, 8:]
    assert (ref[:, 0] == 1).any() and (ref[:, 0] == 0).any()
    sc, tr = _tracer(E.scene_file(name))
    got = tr.intersect(rays)[:, :10]
    tr.close()
    bad = np.flatnonzero((f32_bits(got) != f32_bits(ref)).any(-1))
    assert bad.size == 0, (f"{name} {mode}: {bad.size} of {len(fx)} records differ from the reference; first: ray "
                           f"{bad[0]} {rays[bad[0]].tolist()}\n  kernel    {got[bad[0]].tolist()}\n  reference {ref[bad[0]].tolist()}")


def test_the_fixtures_cover_the_cases():
    assert set(EDGE_FILES) == (set(E.SCENES) - set(E.MEDIA)) | set(E.TIES)


@pytest.mark.parametrize("mode", KERNELS)
@pytest.mark.parametrize("name", E.SCENES)
def test_pairs_in_the_kernel(have_gpu, monkeypatch, name, mode):
    """Within one launch every silhouette and tmin pair gets two different keys from the kernel: it follows from
    test_against_the_oracle, and says at once which side of a boundary moved."""
    _set(monkeypatch, mode)
    b = E.batch(name)
    sc, tr = _tracer(E.scene_file(name))
    got = tr.intersect(b.rays)
    tr.close()
    exp = _expected(name, SEED)
    ks = E.keys(got)
    first = [i for i in range(len(ks)) if b.cls[i] in ("silhouette", "tmin") and i < b.pair[i]]
    assert len(first) == E.N_SILHOUETTE + E.N_TMIN
    one = np.array([i for i in first if ks[i] == ks[b.pair[i]]], np.int64)
    if one.size:
        i, j = int(one[0]), int(b.pair[one[0]])
        moved = i if E.key(got[i]) != E.key(exp[i]) else j
        pytest.fail(f"{name} {mode}: {one.size} pairs get one key from the kernel; ray {moved} moved across its "
                    f"boundary\n" + _describe(name, mode, b, got, exp, np.array([moved])))
