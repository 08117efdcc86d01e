"""The flat walk's certificate evaluated once per trace (render.hip trace_linear with kFlat; DESIGN.md §4 "Flat
walk of small BVHs"): the kernel keeps a lane's tmax at a transform's entry and evaluates the one rule after
the walk, on the winner's row of the certificate table, instead of the entry rule at every transform entry and
the end rule at the end. The decision is the same function of the same inputs, consulted under the same
condition, so nothing observable may move: the accumulation and the ray count stay the oracle's bit for bit
with the flat program (the default), without it (RT2_FLAT_BVH=0) and with a kernel that certifies no hit
(RT2_FLAT_BVH=2), and the fallback counters stay what the kernel with the eager rules counted for exactly
these configurations (tests/golden/flat_cert_counters.json, recorded with that build, three runs each).

What is compared how. `flat_uncertified` counts lanes, a function of the rays alone: it must equal the recorded
value in every mode (34 and 460 by default, the figures DESIGN.md lists). So must every counter without a flat
program (all 0) and `flat_fallback_hits` when nothing is certified (it is then the number of hits, and equals
`flat_uncertified`). `flat_wave_fallbacks` otherwise, and `flat_fallback_hits` by default, also depend on which
lanes share a wave, and waves reserve their work items dynamically: the recording build itself returned 1,614,
1,643 and 1,652 fallback hits in three runs of the Cornell box (this build 1,653, 1,653, 1,679), and 128
falling-back wave-bounces for cornell_box2 where DESIGN.md's earlier run has 133. Those are held to what the
lane count implies instead: ceil(lanes / 64) <= wave-bounces <= lanes, 0 < fallback hits <= 64 per
wave-bounce; the recorded runs are printed beside them. (On the box of the recording this build returned 33,
128, 156,930 and 33,055 wave-bounces in three runs each, as the recording build did.)

cornell_box_original at 128 x 128 and cornell_box2 at 64 x 64, 16 frames of 16 spp: the smallest sizes at which
both kinds of rule leave lanes uncertified."""
import json
import os

import numpy as np
import pytest

import raytrace2_amd as R
from conftest import ROOT, scene_path
from helpers import SEED, oracle_render

pytestmark = pytest.mark.gpu

COUNTERS = ("flat_uncertified", "flat_wave_fallbacks", "flat_fallback_hits")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "flat_cert_counters.json")))["configs"]


def render(path, w, h, spp, frames):
    sc = R.Scene(path, SEED)
    tr = R.RayTracer(sc, 0)
    tr.set_seed(SEED)
    tr.SetSamplesPerPixel(spp)
    tr.OnResize((w, h))
    tr.Render(frames)
    acc = tr.Accumulation().copy()
    st = tr.stats()
    variant = tr.last_launch()["variant"]
    tr.close()
    return sc.info(), acc, st, variant


@pytest.mark.parametrize("name,w,h", [("cornell_box_original", 128, 128), ("cornell_box2", 64, 64)])
def test_one_rule_per_trace_moves_no_bit_and_no_counter(have_gpu, monkeypatch, name, w, h):
    spp, frames = 16, 16
    o_acc, _, o_cnt = oracle_render(name, w, h, spp, frames)
    for env in (None, "0", "2"):
        if env is None:
            monkeypatch.delenv("RT2_FLAT_BVH", raising=False)
        else:
            monkeypatch.setenv("RT2_FLAT_BVH", env)
        info, acc, st, variant = render(scene_path(name), w, h, spp, frames)
        key = f"{name} {w}x{h} {spp}x{frames} RT2_FLAT_BVH={'unset' if env is None else env}"
        want = GOLDEN[key]
        print(key, {k: st[k] for k in ("rays", "paths") + COUNTERS}, "recorded:", want)
        assert variant == 0 and (info.flat_steps > 0) == (env != "0"), key
        assert np.array_equal(acc.view(np.uint32), o_acc.view(np.uint32)), key + ": differs from the oracle"
        assert st["rays"] == o_cnt["rays"] == want["rays"] and st["paths"] == want["paths"], (key, want)
        lanes, waves, hits = (st[k] for k in COUNTERS)
        assert lanes == want["flat_uncertified"], (key, lanes, want)
        if env == "0":
            assert lanes == waves == hits == 0 and set(want["flat_wave_fallbacks"] + want["flat_fallback_hits"]) == {0}, key
            continue
        assert lanes > 0 and (lanes + 63) // 64 <= waves <= lanes, (key, lanes, waves)
        assert 0 < hits <= min(64 * waves, st["rays"]), (key, lanes, waves, hits)
        if env == "2":  # every hit is uncertified: the fallback hits are the hits
            assert hits == lanes and set(want["flat_fallback_hits"]) == {lanes}, (key, hits, want)
            assert st["rays"] - st["paths"] <= hits, key
    monkeypatch.delenv("RT2_FLAT_BVH", raising=False)


def test_recorded_counters_match_the_documented_ones():
    """The cross-check: the recorded default-mode counters against those DESIGN.md §4 lists for these
    configurations (34 lanes in 33 wave-bounces; 460 lanes, in 133 wave-bounces there and 128 in the recording:
    the wave-bounces depend on the run), and both rule kinds leave lanes open in them."""
    a = GOLDEN["cornell_box_original 128x128 16x16 RT2_FLAT_BVH=unset"]
    b = GOLDEN["cornell_box2 64x64 16x16 RT2_FLAT_BVH=unset"]
    assert a["flat_uncertified"] == 34 and set(a["flat_wave_fallbacks"]) == {33}, a
    assert b["flat_uncertified"] == 460 and all(8 <= x <= 460 for x in b["flat_wave_fallbacks"]), b
