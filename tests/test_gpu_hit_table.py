"""The hit table in LDS (rt2_layout.h HIT; render.hip resolve_hit_tab): the Cornell-box kernel stages the
flattened shading records of the scene's quads in LDS and resolves closest hits from there. It must
change no bit: against the same render with the table switched off (RT2_HIT_TABLE=0 at scene load, the
global-memory chain) and against the oracle; scenes whose table is too large for the kernel's LDS room,
and scenes with nested transforms, get no table and render through the global-memory path as before.

Other material kinds: the kernel that takes the table is the variant for scenes whose only feature is
transforms. A metal or dielectric material, a checker or noise texture, a sphere or a medium selects
another kernel variant (rt2_layout.h Feature), none of which reads the table, so those kinds cannot
reach this path; the kinds that can (lambertian, diffuse light and texture materials over solid
textures, under a transform or not, QUADAA and general quads) are all in the authored scenes below."""
import pytest

import raytrace2_amd as R
from bits import same_bits
from conftest import scene_path
from helpers import SEED, oracle_render
from raytrace2_amd import authoring as A

pytestmark = pytest.mark.gpu


def render(path, w, h, spp, frames, *, stats=False):
    """(info, accumulation, stats, kernel variant) of one render: the product kernel, or the counting one."""
    sc = R.Scene(path, SEED)
    tr = R.RayTracer(sc, 0)
    tr.set_seed(SEED)
    tr.SetSamplesPerPixel(spp)
    tr.OnResize((w, h))
    if stats:
        tr.enable_stats(True)
    tr.Render(frames)
    acc = tr.Accumulation().copy()
    st = tr.stats()
    variant = tr.last_launch()["variant"]
    tr.close()
    return sc.info(), acc, st, variant


def test_cornell_box_from_the_table_changes_no_bit(have_gpu, monkeypatch):
    name, w, h, spp, frames = "cornell_box_original", 64, 64, 1000, 6
    path = scene_path(name)
    monkeypatch.delenv("RT2_HIT_TABLE", raising=False)
    info, acc, st, variant = render(path, w, h, spp, frames)
    _, _, cst, _ = render(path, w, h, spp, frames, stats=True)
    monkeypatch.setenv("RT2_HIT_TABLE", "0")
    info0, acc0, st0, variant0 = render(path, w, h, spp, frames)
    _, cacc0, cst0, _ = render(path, w, h, spp, frames, stats=True)
    monkeypatch.delenv("RT2_HIT_TABLE")
    assert variant == variant0 == 0  # the Cornell-box kernel
    assert info.hit_table_bytes > 0 and info0.hit_table_bytes == 0
    # the product launch staged the whole table; the switched-off scene and the counting kernel none
    assert st["hit_table_bytes"] == info.hit_table_bytes
    assert st0["hit_table_bytes"] == 0 and cst["hit_table_bytes"] == 0
    assert same_bits(acc, acc0)
    assert same_bits(acc, cacc0)
    assert st["rays"] == st0["rays"] == cst["rays"] == cst0["rays"]
    assert cst["quad_tests"] == cst0["quad_tests"] > 0
    o_acc, _, o_cnt = oracle_render(name, w, h, spp, frames)
    assert same_bits(acc, o_acc), "the render from the hit table differs from the oracle"
    assert st["rays"] == o_cnt["rays"]


def blocks_scene(n_blocks):
    """The Cornell room with n_blocks rotated blocks (each a transformed MakeBox: six QUADAA records and
    its XFORM record in the table), one of them with a texture material over a solid texture, a slanted
    quad under a rotation (the general QUAD layout: its normal goes through the transform's inverse
    rows) and a slanted quad in world space."""
    doc = A.SceneDoc()
    A._cornell_room(doc)
    white = doc.lambertian([0.73, 0.73, 0.73])
    doc.textures.append({"type": "solid_color", "albedo": [0.2, 0.3, 0.7]})
    blue = doc.textured(len(doc.textures) - 1)
    for k in range(n_blocks):
        x, z = 40 + 100 * (k % 5), 60 + 150 * (k // 5)
        doc.node(doc.box([0, 0, 0], [60, 60 + 40 * (k % 3), 60], blue if k == 1 else white),
                 xform=A.transform([x, 0, z], [-18 + 11 * k, 0, 1, 0]))
    doc.node(doc.quad([0, 0, 0], [120, 30, 0], [0, 40, 90], blue), xform=A.transform([300, 300, 200], [25, 0, 1, 0]))
    doc.node(doc.quad([60, 380, 300], [100, 40, 0], [0, 30, 80], white))
    A._cornell_camera(doc)
    return doc


def table_bytes(path):
    return R.Scene(path, SEED).info().hit_table_bytes


def test_largest_table_that_fits_and_the_first_that_does_not(have_gpu, tmp_path, monkeypatch):
    """Scenes around the size limit: the largest authored scene whose table is still built is staged and
    renders, from the table, exactly what the oracle renders; one block more and the scene gets no
    table (hit_table_bytes == 0) and renders through the global-memory chain, also bit-identical."""
    monkeypatch.delenv("RT2_HIT_TABLE", raising=False)
    sizes = {}
    for n in range(2, 14):
        p = str(tmp_path / f"blocks{n}.json")
        blocks_scene(n).dump(p)
        sizes[n] = (p, table_bytes(p))
    fits = max(n for n, (_, b) in sizes.items() if b > 0)
    assert fits + 1 in sizes and sizes[fits + 1][1] == 0, sizes
    assert all(b > 0 for n, (_, b) in sizes.items() if n <= fits)
    w, h, spp, frames = 32, 32, 16, 3
    for n, staged in ((fits, True), (fits + 1, False)):
        p, nbytes = sizes[n]
        info, acc, st, variant = render(p, w, h, spp, frames)
        assert variant == 0 and info.xforms == n + 1
        assert st["hit_table_bytes"] == (nbytes if staged else 0)
        o_acc, _, o_cnt = oracle_render(p, w, h, spp, frames)
        assert st["rays"] == o_cnt["rays"]
        assert same_bits(acc, o_acc), f"{n} blocks (table {'staged' if staged else 'declined'}) differ from the oracle"
        if staged:  # and the switch changes nothing
            monkeypatch.setenv("RT2_HIT_TABLE", "0")
            _, acc0, st0, _ = render(p, w, h, spp, frames)
            monkeypatch.delenv("RT2_HIT_TABLE")
            assert st0["hit_table_bytes"] == 0 and same_bits(acc, acc0)


def test_nested_transforms_get_no_table(have_gpu, monkeypatch):
    """cornell_box_scene_graph nests its transforms: the compiler builds no table for it (the kernel's
    table path handles one transform level), and the render equals the oracle's as before."""
    monkeypatch.delenv("RT2_HIT_TABLE", raising=False)
    name, w, h, spp, frames = "cornell_box_scene_graph", 32, 32, 16, 3
    info, acc, st, _ = render(scene_path(name), w, h, spp, frames)
    assert info.xforms > 0 and info.hit_table_bytes == 0 and st["hit_table_bytes"] == 0
    o_acc, _, o_cnt = oracle_render(name, w, h, spp, frames)
    assert st["rays"] == o_cnt["rays"] and same_bits(acc, o_acc)
