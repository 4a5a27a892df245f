"""CPU tests of the textured reference (render_tex_ref.py): the numpy sampler against hand-derived answers, the sRGB table at its
breakpoint, the subclass against RenderRef when nothing is bound, the stable-pixel condition and the restatement figures of the
scene test_gpu_render_textures.py renders, and five deliberately wrong restatements that each miss the frame bar by a wide margin."""
import numpy as np
import pytest

import render_scenes as rs
import render_tex_ref as tr
import render_tex_scenes as ts
from render_ref import RenderRef, stable_pixels
from scene_ref import SceneRef

T2 = np.array([[[0, 10, 20, 255], [100, 110, 120, 0]], [[200, 210, 220, 51], [40, 50, 60, 102]]], np.uint8)


@pytest.mark.parametrize("ft", [np.float32, np.float64])
def test_the_sampler_on_a_2x2_texture(ft):
    f = lambda *c: np.array(c, np.float64) / 255.0
    t00, t10, t01, t11 = f(0, 10, 20, 255), f(100, 110, 120, 0), f(200, 210, 220, 51), f(40, 50, 60, 102)
    cases = [((0.25, 0.25), t00), ((0.75, 0.25), t10), ((0.25, 0.75), t01), ((0.75, 0.75), t11),   # texel centres
             ((0.5, 0.5), (t00 + t10 + t01 + t11) / 4),                                           # the midpoint
             ((0.5, 0.25), (t00 + t10) / 2), ((0.25, 0.5), (t00 + t01) / 2),
             ((0.0, 0.0), t00), ((1.0, 0.0), t10), ((0.0, 1.0), t01), ((1.0, 1.0), t11),           # the corners: clamp to edge
             ((-3.0, 0.25), t00), ((7.0, 0.75), t11), ((0.0, 0.5), (t00 + t01) / 2), ((1.0, 0.5), (t10 + t11) / 2),
             ((0.375, 0.25), t00 * 0.75 + t10 * 0.25)]
    got = tr.sample(T2, False, np.array([c[0] for c in cases]), ft)
    assert got.dtype == ft
    assert np.abs(got - np.array([c[1] for c in cases])).max() <= (2e-7 if ft is np.float32 else 1e-15)


def test_the_sampler_on_one_texel_and_odd_coordinates():
    t = np.array([[[255, 128, 0, 64]]], np.uint8)
    uv = np.array([[0.5, 0.5], [-2, 9], [np.nan, np.inf], [-np.inf, -0.0]], np.float32)
    got = tr.sample(t, False, uv, np.float32)
    assert np.array_equal(got, np.tile(np.array([255, 128, 0, 64], np.float32) / np.float32(255), (4, 1)))
    # NaN becomes 0 through fmax, +inf the last texel, -inf the first
    row = np.zeros((1, 3, 4), np.uint8); row[0, :, 0] = (0, 100, 255)
    got = tr.sample(row, False, np.array([[np.nan, 0], [np.inf, 0], [-np.inf, 0]], np.float32), np.float32)[:, 0]
    assert np.array_equal(got, np.array([0, 255, 0], np.float32) / np.float32(255))


def test_the_srgb_table_around_its_breakpoint():
    t = tr.srgb_table64()
    assert t[0] == 0 and abs(t[255] - 1) < 1e-15
    assert 10 / 255 <= 0.04045 < 11 / 255
    assert t[10] == (10 / 255) / 12.92 and t[11] == ((11 / 255 + 0.055) / 1.055) ** 2.4
    assert abs(t[10] - 0.0030352698) < 1e-9 and abs(t[11] - 0.0033465358) < 1e-9
    # decode happens before filtering, colour only: alpha stays linear
    srgb = tr.sample(T2, True, np.array([[0.5, 0.5]]), np.float64)[0]
    assert abs(srgb[0] - t[[0, 100, 200, 40]].mean()) < 1e-15 and abs(srgb[3] - (255 + 0 + 51 + 102) / 4 / 255) < 1e-15


@pytest.fixture(scope="module")
def world(sge):
    meshes, mesh_of, mats, material_of = ts.static_scene()
    scene = SceneRef(sge, meshes, mesh_of, mats)
    eye, target = rs.camera()
    try:
        yield {"scene": scene, "m": rs.materials(sge), "material_of": material_of, "lights": rs.lights(sge), "tex": ts.textures(),
               "f": rs.frame_record(sge, eye, target, 48, 32, 4)}
    finally:
        scene.close()


def test_nothing_bound_is_renderref_exactly(sge, world):
    w = world
    want = RenderRef(w["scene"], w["m"], w["material_of"], None, w["lights"]).render(w["f"], "A", shade=np.float32)
    empty = sge.abi.default_render_material_textures(7)
    empty["baseColor"][5], empty["normal"][1] = 20, 32  # an empty slot, an index beyond the slots
    for bind in (None, sge.abi.default_render_material_textures(7), empty):
        got = tr.TexRenderRef(w["scene"], w["m"], w["material_of"], None, w["lights"], w["tex"], bind).render(w["f"], "A", shade=np.float32)
        for k in ("rgb", "layers", "instance", "primitive", "distance", "shadow", "alpha", "queries", "flags"):
            assert np.array_equal(got[k], want[k]), k
        assert stable_pixels(got, want).all()


@pytest.mark.parametrize("normal_scale", [1, 6])
def test_the_scene_is_stable_and_wrong_restatements_miss_the_bar(sge, world, normal_scale):
    w = world
    name = "textured, normalScale %d" % normal_scale
    bind = ts.bindings(sge, float(normal_scale))
    make = lambda variant=None: tr.TexRenderRef(w["scene"], w["m"], w["material_of"], None, w["lights"], w["tex"], bind, variant=variant)
    ref = make()
    a, b, a32 = ref.render(w["f"], "A"), ref.render(w["f"], "B"), ref.render(w["f"], "A", shade=np.float32)
    term = ts.margin_term(w["tex"])
    stable = tr.tex_stable_pixels(a, b, term)
    print("%s: unstable %d of %d; margin term %.3g" % (name, (~stable).sum(), stable.size, term))
    assert (~stable).mean() <= 0.03
    rest = np.abs(a32["rgb"].astype(np.float64) - a["rgb"])[stable & tr.tex_stable_pixels(a, a32, term)].max()
    bar = ts.colour_bar(name, w["tex"], w["lights"], w["f"])
    print("%s: float32 restatement worst %.4g (constant %.3g), bar %.3g" % (name, rest, ts.RESTATEMENT_WORST[name], bar))
    assert rest <= ts.RESTATEMENT_WORST[name] and rest > 0.5 * ts.RESTATEMENT_WORST[name]
    assert np.abs(b["rgb"] - a["rgb"])[stable].max() <= bar, "path B, whose uvs differ by float32 rounding, is inside the bar"
    mirror_box = a["instance"] == sge.abi.SCENE_STATIC_BASE + 2
    assert ((a["flags"][mirror_box] & 1) != 0).any() and not ((a["flags"][mirror_box] & 1) != 0).all()
    for variant in ("no_offset", "wrap", "filter_first", "flip_y", "opaque_shadow"):
        wrong = make(variant).render(w["f"], "A")
        err = np.abs(wrong["rgb"] - a["rgb"])[stable & stable_pixels(a, wrong)].max()
        print("  %s: worst |rgb - ref| %.3g = %.0f x the bar" % (variant, err, err / bar))
        assert err > 100 * bar, variant
