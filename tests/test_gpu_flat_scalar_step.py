"""The flat walk's step index as a scalar (render.hip trace_linear with kFlat; DESIGN.md §4 "Flat walk of small
BVHs", "The step index as a scalar"): the flat kernel keeps no per-lane `next`, tests no `next == at` and
searches no wave minimum; the wave's step comes from the step words alone. Per lane the walk is the same
sequence of the same tests, so no bit, no ray count and no certificate counter may move. The shapes are the
smallest at which a wave-uniform index could go wrong: partial waves (70 x 37 = 2,590 pixels, no multiple of
64), waves in which lanes sit out a trace that their neighbours run (max_depth 2: a path that ended waits for
the wave's longest), a flat program without a transform (quad_scene1) and a partitioned tracer (its rows
against the same rows of the one-GPU render).

The number of hits under RT2_FLAT_BVH=2: neither the oracle nor the counting kernels count hits, so, as in
test_gpu_flat_bvh.py, it is the flat kernel's own count of the hits its falling-back wave-bounces end with
(every wave-bounce with a hit, when nothing is certified), bounded from outside by rays - paths <= hits <=
rays (a path casts at most one ray that misses)."""
import pytest

import raytrace2_amd as R
from bits import same_bits
from conftest import scene_path
from helpers import SEED, oracle_render
from raytrace2_amd.tracer import local_rows

pytestmark = pytest.mark.gpu

COUNTERS = ("flat_uncertified", "flat_wave_fallbacks", "flat_fallback_hits")


def render(name, w, h, spp, frames, *, max_depth=50, partition=None):
    """The product kernel's render (no per-pixel counters): the kernel that walks the flat program."""
    sc = R.Scene(scene_path(name), SEED)
    tr = R.RayTracer(sc, 0)
    tr.set_seed(SEED)
    tr.SetSamplesPerPixel(spp)
    tr.max_depth = max_depth
    tr.OnResize((w, h))
    if partition is not None:
        tr.set_partition(*partition)
    tr.Render(frames)
    acc = tr.Accumulation().copy()
    st = tr.stats()
    variant = tr.last_launch()["variant"]
    tr.close()
    return sc.info(), acc, st, variant


@pytest.mark.parametrize("max_depth", [50, 2])
def test_partial_waves_and_masked_lanes_move_no_bit_and_no_counter(have_gpu, monkeypatch, max_depth):
    name, w, h, spp, frames = "cornell_box_original", 70, 37, 4, 4
    assert (w * h) % 64 != 0
    o_acc, _, o_cnt = oracle_render(name, w, h, spp, frames, max_depth=max_depth)
    monkeypatch.delenv("RT2_FLAT_BVH", raising=False)
    info, acc, st, variant = render(name, w, h, spp, frames, max_depth=max_depth)
    _, acc_b, st_b, _ = render(name, w, h, spp, frames, max_depth=max_depth)
    monkeypatch.setenv("RT2_FLAT_BVH", "0")  # the BVH-program kernel
    info0, acc0, st0, variant0 = render(name, w, h, spp, frames, max_depth=max_depth)
    monkeypatch.setenv("RT2_FLAT_BVH", "2")  # the flat kernel, certifying no hit
    info2, acc2, st2, variant2 = render(name, w, h, spp, frames, max_depth=max_depth)
    _, _, st2_b, _ = render(name, w, h, spp, frames, max_depth=max_depth)
    monkeypatch.delenv("RT2_FLAT_BVH")
    print(f"max_depth {max_depth}: oracle rays {o_cnt['rays']}; default", {k: st[k] for k in ("rays", "paths") + COUNTERS},
          "again", {k: st_b[k] for k in COUNTERS}, "RT2_FLAT_BVH=2", {k: st2[k] for k in ("rays", "paths") + COUNTERS})
    assert variant == variant0 == variant2 == 0  # the Cornell-box kernel
    assert info.flat_steps == info2.flat_steps == 22 and info0.flat_steps == 0
    assert same_bits(acc, o_acc), "the flat walk differs from the oracle"
    assert same_bits(acc_b, o_acc), "the flat walk's second run differs from the oracle"
    assert same_bits(acc0, o_acc), "RT2_FLAT_BVH=0 differs from the oracle"
    assert same_bits(acc2, o_acc), "RT2_FLAT_BVH=2 (every hit traced again) differs from the oracle"
    assert st["rays"] == st_b["rays"] == st0["rays"] == st2["rays"] == o_cnt["rays"]
    assert st["paths"] == st_b["paths"] == st0["paths"] == st2["paths"] == w * h * frames
    # the uncertified lanes are a function of the rays alone: the same in two runs, in both modes
    assert st["flat_uncertified"] == st_b["flat_uncertified"]
    assert st2["flat_uncertified"] == st2_b["flat_uncertified"]
    assert st0["flat_uncertified"] == st0["flat_wave_fallbacks"] == st0["flat_fallback_hits"] == 0
    # certifying nothing: every hit is uncertified, and the fallback's hits are the hits
    assert st2["flat_uncertified"] == st2["flat_fallback_hits"] == st2_b["flat_fallback_hits"]
    assert 0 < st2["rays"] - st2["paths"] <= st2["flat_uncertified"] <= st2["rays"]
    assert st["flat_uncertified"] <= st2["flat_uncertified"]


def test_a_flat_program_without_a_transform(have_gpu, monkeypatch):
    name, w, h, spp, frames = "quad_scene1", 64, 64, 16, 4
    monkeypatch.delenv("RT2_FLAT_BVH", raising=False)
    o_acc, _, o_cnt = oracle_render(name, w, h, spp, frames)
    info, acc, st, _ = render(name, w, h, spp, frames)
    monkeypatch.setenv("RT2_FLAT_BVH", "2")
    _, acc2, st2, _ = render(name, w, h, spp, frames)
    monkeypatch.delenv("RT2_FLAT_BVH")
    print(name, {k: st[k] for k in ("rays", "paths") + COUNTERS}, "RT2_FLAT_BVH=2", {k: st2[k] for k in COUNTERS},
          "flat_steps", info.flat_steps)
    assert info.flat_steps > 0 and info.xforms == 0
    assert same_bits(acc, o_acc), "the flat walk differs from the oracle"
    assert same_bits(acc2, o_acc), "RT2_FLAT_BVH=2 differs from the oracle"
    assert st["rays"] == st2["rays"] == o_cnt["rays"]
    # the flat kernel ran: it counted the hits it could not certify when told to certify none
    assert 0 < st2["flat_uncertified"] == st2["flat_fallback_hits"] <= st2["rays"]


def test_a_partitioned_tracer_renders_its_rows_of_the_one_gpu_image(have_gpu, monkeypatch):
    name, w, h, spp, frames = "cornell_box_original", 70, 37, 4, 4
    band_h, rank, world = 2, 1, 3
    monkeypatch.delenv("RT2_FLAT_BVH", raising=False)
    info, full, _, variant = render(name, w, h, spp, frames)
    _, part, st, variant_p = render(name, w, h, spp, frames, partition=(band_h, rank, world))
    rows = local_rows(h, band_h, rank, world)
    print("rank", rank, "of", world, "rows", rows, {k: st[k] for k in ("rays", "paths") + COUNTERS})
    assert variant == variant_p == 0 and info.flat_steps == 22
    assert 0 < len(rows) < h and part.shape[0] == len(rows)
    assert st["paths"] == len(rows) * w * frames
    assert same_bits(part, full[rows]), "the partition's rows differ from the one-GPU render's"
