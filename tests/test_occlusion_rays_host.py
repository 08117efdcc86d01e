"""tests/occlusion_rays.py is what it claims, on the CPU oracle alone: every scene reaches its 120 shadow pairs within
the draw limit, a pair is at most 1 ulp apart and the oracle's flags of its two rays differ, every tmax triple
answers (0, ., 1) with both middle values somewhere, and every ray is one the kernel traces."""
import numpy as np
import pytest

import edge_rays as E
import occlusion_rays as O

F32 = np.float32


def _valid(r):
    """query.h QueryRayValid in numpy (tests/test_query_capi.py checks the library's against the same rule)."""
    r = np.asarray(r, F32).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        m = np.abs(r[:, 4:7]).max(-1)
        return (np.isfinite(r).all(-1) & (m >= F32(2.0 ** -20)) & (m <= F32(2.0 ** 20))
                & (np.abs(r[:, 0:3]) <= F32(2.0 ** 64)).all(-1) & (r[:, 3] > F32(0.001)) & (r[:, 7] >= 0) & (r[:, 7] <= 1))


@pytest.mark.parametrize("name", O.ALL)
def test_shadow_pairs(name):
    b = O.batch(name)
    st = b.stats
    first = [i for i in range(len(b.rays)) if b.cls[i] == "shadow" and i < b.pair[i]]
    assert len(first) == O.N_SHADOW, (name, st)
    assert st["draws"] <= O.DRAW_LIMIT and st["dropped"] <= 0.05 * st["candidates"], (name, st)
    for i in first:
        j = int(b.pair[i])
        assert b.pair[j] == i and b.cls[j] == "shadow"
        assert np.array_equal(b.rays[i, :4], b.rays[j, :4]) and b.rays[i, 7] == b.rays[j, 7]
        assert E.ulps(b.rays[i, 4:7], b.rays[j, 4:7]).max() <= 1, (name, i)
        assert {int(b.flag[i]), int(b.flag[j])} == {0, 1}, (name, i)
    assert np.isfinite(b.rays[b.cls == "shadow", 3]).all() and (b.rays[b.cls == "shadow", 3] < E.FLT_MAX).all()


@pytest.mark.parametrize("name", O.ALL)
def test_triples_and_validity(name):
    b = O.batch(name)
    tr = O.triples(b)
    assert tr.shape == (O.N_TMAX3, 3)
    t = b.rays[tr, 3]
    assert (np.nextafter(t[:, 1], F32(0)) == t[:, 0]).all() and (np.nextafter(t[:, 1], F32(np.inf)) == t[:, 2]).all()
    assert (t[:, 1] >= F32(0.002)).all()
    assert (b.flag[tr[:, 0]] == 0).all() and (b.flag[tr[:, 2]] == 1).all(), name
    assert _valid(b.rays).all()
    assert set(np.unique(b.flag)) == {0, 1} and len(b.rays) % 64 != 0


def test_both_middles_occur():
    mid = np.concatenate([O.batch(n).flag[O.triples(O.batch(n))[:, 1]] for n in E.SCENES])
    assert (mid == 0).any() and (mid == 1).any()
