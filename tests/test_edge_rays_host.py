"""The edge batches of tests/edge_rays.py on the oracle alone: that they are what they claim to be. A pair's two rays
differ by at most 1 ulp per component and are answered differently; every scene reaches its full counts; more than
40 % of the aimed rays change their answer when a direction component moves by 1 or 4 ulps (random rays: none);
the authored scene's ties are reached, resolved by node order, and by the rule; and every batch has hits and
misses. tests/test_gpu_edge_rays.py sends the same batches to the kernels."""
import numpy as np
import pytest

import edge_rays as E

ALL = E.SCENES + list(E.TIES)


@pytest.mark.parametrize("name", E.SCENES)
def test_pairs_differ_by_an_ulp_and_in_their_answer(name):
    b, ks = E.batch(name), E.keys(E.answers(name))
    for cls, n, moved, fixed in (("silhouette", E.N_SILHOUETTE, slice(4, 7), (0, 1, 2, 3, 7)),
                                 ("tmin", E.N_TMIN, slice(0, 3), (3, 4, 5, 6, 7))):
        first = [i for i in np.flatnonzero(b.cls == cls) if i < b.pair[i]]
        assert len(first) == n, f"{name} {cls}: {len(first)} pairs"
        st = b.stats[cls]
        assert st["dropped"] <= 0.2 * st["candidates"], (name, cls, st)
        for i in first:
            j = b.pair[i]
            assert b.cls[j] == cls and b.pair[j] == i
            assert ks[i] != ks[j], f"{name} {cls} pair ({i}, {j}) has one answer"
            assert E.ulps(b.rays[i, moved], b.rays[j, moved]).max() == 1, (name, cls, i, j)
            assert np.array_equal(E.bits(b.rays[i, fixed]), E.bits(b.rays[j, fixed]))
    assert (b.cls == "continue").sum() == E.N_CONTINUE


@pytest.mark.parametrize("name", E.SCENES)
def test_the_interval_ends(name):
    """tmin: one of the two origins has the surface it started from in front of it, accepted (t above 0.001 and
    below 0.003: s ends at 0.002, and a sphere of radius 1000 places its root within 1e-3 at best), the other
    passes it. tmax: the pair differs in tmax alone, by one float; with tmax below t nothing but a medium
    is hit, and with tmax = t both answers occur over the scenes (quads accept it, spheres do not)."""
    b, a = E.batch(name), E.answers(name)
    tmin = [i for i in np.flatnonzero(b.cls == "tmin") if i < b.pair[i]]
    near = sum(1 for i in tmin if ((a[[i, b.pair[i]], 0] == 1) & (a[[i, b.pair[i]], 1] < 0.003)).sum() == 1)
    assert near >= 0.9 * len(tmin), (name, near)
    first = [i for i in np.flatnonzero(b.cls == "tmax") if i < b.pair[i]]
    assert len(first) == E.N_TMAX
    for i in first:
        j = b.pair[i]
        assert E.ulps(b.rays[i, 3], b.rays[j, 3]) == 1 and np.array_equal(E.bits(b.rays[i, [0, 1, 2, 4, 5, 6, 7]]),
                                                                         E.bits(b.rays[j, [0, 1, 2, 4, 5, 6, 7]]))
        lower = i if b.rays[i, 3] < b.rays[j, 3] else j
        if name not in E.MEDIA:
            assert a[lower, 0] == 0, (name, lower)


def test_tmax_at_t_is_answered_both_ways():
    at = []
    for name in E.SCENES:
        b, a = E.batch(name), E.answers(name)
        at += [a[max(i, b.pair[i], key=lambda k: b.rays[k, 3]), 0] for i in np.flatnonzero(b.cls == "tmax") if i < b.pair[i]]
    at = np.array(at)
    assert (at == 1).sum() >= 100 and (at == 0).sum() >= 100


@pytest.mark.parametrize("name", E.AIMED)
def test_aimed_rays_sit_on_boundaries(name):
    """At least 40 % of the rays aimed at corners and edges change their key under a +-1 / +-4 ulp nudge of one
    direction component; test_random_rays_do_not is the contrast."""
    b = E.batch(name)
    idx = np.flatnonzero(b.cls == "aimed")
    assert len(idx) >= 600
    share = np.mean([E.nudged_keys_differ(name, b.rays[i]) for i in idx])
    assert share >= 0.40, share


def test_random_rays_do_not():
    """The contrast that motivates the batches: of 300 random rays on Cornell at most 5 % change their key under the
    nudges (a twentieth is an eighth of the aimed rays' 40 %; 2 of them do)."""
    g = np.random.default_rng(1)
    n = 0
    for _ in range(300):
        o, d, t = E._draw(g, "cornell_box_original")
        n += E.nudged_keys_differ("cornell_box_original", E.rays(o, d, E.FLT_MAX, t)[0])
    assert n <= 15, n


def test_ties_are_reached_and_follow_the_rule():
    """In every tie class at least half of the rays get bit-equal t and different materials from the two node
    orders, and where both orders hit at one t the winner is the later quad or box face, the earlier sphere."""
    b = E.batch("ties")
    a0, a1 = E.answers("ties"), E.answers("ties_swapped")
    assert np.array_equal(b.rays, E.batch("ties_swapped").rays)
    for cls in E.TIE_CLASSES:
        m = b.cls == cls
        assert m.sum() >= 100
        tied = m & (a0[:, 0] == 1) & (a1[:, 0] == 1) & (E.bits(a0[:, 1]) == E.bits(a1[:, 1]))
        swapped = tied & (a0[:, 9] != a1[:, 9])
        assert swapped.sum() >= 0.5 * m.sum(), (cls, swapped.sum(), m.sum())
        assert (b.rule[tied] >= 0).all()
        assert np.array_equal(a0[tied, 9], b.rule[tied, 0]) and np.array_equal(a1[tied, 9], b.rule[tied, 1]), cls
    # the rule's two halves give different winners: the later of the quads, the earlier of the spheres
    q, s = b.cls == "quads", b.cls == "twins"
    assert set(np.unique(a0[q, 9])) == {E.MATERIAL["q1"], E.MATERIAL["q2"]} and set(np.unique(a1[q, 9])) == {E.MATERIAL["floor"]}
    assert set(np.unique(a0[s, 9])) == {E.MATERIAL["s1"]} and set(np.unique(a1[s, 9])) == {E.MATERIAL["s2"]}
    w = b.cls == "below"
    assert set(np.unique(a0[w, 9])) == {E.MATERIAL["box_a"]} and set(np.unique(a1[w, 9])) == {E.MATERIAL["floor"]}


def test_ties_edge_classes_are_answered_both_ways():
    """Tangent rays hit and miss the sphere they graze; rays in a face's plane hit something or nothing; the
    classes reach the spheres, both boxes and the floor. The ties at the interval's end: with tmax = t the quads
    still answer (and still by node order), the twin spheres do not."""
    b, a0, a1 = E.batch("ties"), E.answers("ties"), E.answers("ties_swapped")
    sph = [E.MATERIAL[k] for k in ("s1", "s2", "s3", "s4")]
    t = b.cls == "tangent"
    on = t & (a0[:, 0] == 1) & np.isin(a0[:, 9], sph)
    assert on.sum() >= 20 and (t & ~on).sum() >= 20
    p = b.cls == "inplane"
    assert (p & (a0[:, 0] == 1)).sum() >= 20 and (p & (a0[:, 0] == 0)).sum() >= 10
    # |denominator| < 1e-8: from a hair off the floor's plane a slope of 2e-8 reaches the floor, one of 1e-9 does not
    floor = [E.MATERIAL[k] for k in ("floor", "q1", "q2")]
    lay = p & (np.abs(b.rays[:, 1]) < 1e-6) & (b.rays[:, 1] != 0)
    acc, rej = lay & (np.abs(b.rays[:, 5]) == E.F32(2e-8)), lay & (np.abs(b.rays[:, 5]) == E.F32(1e-9))
    assert acc.sum() >= 4 and rej.sum() >= 4
    assert (a0[acc, 0] == 1).all() and np.isin(a0[acc, 9], floor).all() and (a0[acc, 1] > 0.4).all()
    assert not ((a0[rej, 0] == 1) & np.isin(a0[rej, 9], floor)).any()
    e = b.cls == "box_edges"
    assert {E.MATERIAL["box_a"], E.MATERIAL["box_r"]} <= set(np.unique(a0[e & (a0[:, 0] == 1), 9]))
    x = np.flatnonzero(b.cls == "tmax")
    upper = np.array([i for i in x if b.rays[i, 3] > b.rays[b.pair[i], 3]])
    assert (a0[b.pair[upper], 0] == 0).all()
    hit = upper[a0[upper, 0] == 1]
    assert len(hit) >= 60 and (a0[hit, 9] != a1[hit, 9]).all()
    assert (a0[upper, 0] == 0).sum() >= 30  # the twins


@pytest.mark.parametrize("name", ALL)
def test_whole_batch(name):
    b, a = E.batch(name), E.answers(name)
    n = len(b.rays)
    assert n % 64 != 0 and n <= E.MAX_RAYS
    assert (a[:, 0] == 1).mean() >= 0.10 and (a[:, 0] == 0).mean() >= 0.10, (name, (a[:, 0] == 1).mean())
    from test_gpu_query import _valid
    assert _valid(b.rays).all()
    rows = E.fixture_rows(name)
    assert len(rows) <= E.FIXTURE_RAYS and len(set(rows)) == len(rows)
    assert set(b.cls[rows]) == set(b.cls)
    chosen = set(rows)
    assert all(b.pair[i] in chosen for i in rows if b.pair[i] >= 0)
