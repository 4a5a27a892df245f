"""CPU tests of the shaded frame's reference (tests/render_ref.py): known answers derived by hand below, the stable-pixel condition
on the scenes test_gpu_render.py renders, and the distance of a float32 restatement of the shading from the float64 one (the
figure the GPU test's colour bar is four times of)."""
import math

import numpy as np
import pytest

import render_scenes as rs
from render_ref import BG, RenderRef, hash12_rt, stable_pixels
from scene_ref import STATIC_BASE, SceneRef

SH0 = (0.5, 0.4, 0.3)


def _flat_sh():
    sh = np.zeros((9, 3), np.float32)
    sh[0] = SH0
    return sh


def _dither(x, y):
    return (float(hash12_rt(np.array([x]), np.array([y]))[0]) - 0.5) / 255.0


def _brdf_by_hand(n, v, l, base, metallic, rough):
    """eval_brdf with python floats, written out from RayTracing.metalinc:21-59."""
    dot = lambda a, b: sum(x * y for x, y in zip(a, b))
    sat = lambda x: min(max(x, 0.0), 1.0)
    nol, nov = sat(dot(n, l)), sat(dot(n, v))
    h = [a + b for a, b in zip(v, l)]
    hn = math.sqrt(dot(h, h))
    h = [x / hn for x in h]
    noh, voh = sat(dot(n, h)), sat(dot(v, h))
    a = rough * rough
    a2 = a * a
    D = a2 / (3.14159265 * (noh * noh * (a2 - 1) + 1) ** 2)
    g1 = lambda c: 2 * c / max(c + math.sqrt(a2 + (1 - a2) * c * c), 1e-4)
    G = g1(nov) * g1(nol)
    out = []
    for b in base:
        f0 = 0.04 + (b - 0.04) * metallic
        F = f0 + (1 - f0) * sat(1 - voh) ** 5
        out.append(b * (1 - metallic) / 3.14159265 + D * G * F / max(4 * nov * nol, 1e-4))
    return out


def _top_down(sge, extra=(), extra_materials=(), light_dir=(0, -1, 0), eye_y=5.0, target_y=0.0, size=3):
    """A camera straight above (or below, looking up) a ground quad of the default material, one light. extra: (half, (x, y, z))
    horizontal quads; -> the render of path A and the centre pixel's coordinates."""
    meshes = {0: rs.quad(1.0)}
    mesh_of, mats = [0], [rs.transform((4, 1, 4))]
    for half, at in extra:
        mesh_of.append(0); mats.append(rs.transform((half, 1, half), 0.0, at))
    m = sge.abi.default_render_materials(2)
    m["alpha"][1] = 0.5
    l = np.zeros(1, sge.abi.render_light_dtype)
    l["direction"], l["intensity"], l["color"], l["enabled"] = light_dir, 2.0, (1.0, 0.9, 0.8), 1
    scene = SceneRef(sge, meshes, mesh_of, np.array(mats, np.float32))
    try:
        ref = RenderRef(scene, m, [0] + list(extra_materials), None, l)
        f = rs.frame_record(sge, (0, eye_y, 0), (0, target_y, 0), size, size, 1, up=(0, 0, -1), fovy=20.0, env_sh=_flat_sh())
        return ref.render(f, "A"), size // 2
    finally:
        scene.close()


AMBIENT = [s * 0.282095 * 0.25 for s in SH0]  # base 1 * (envSH0 * c0) * ambientIntensity * occlusion 1


def test_lit_ground_straight_below(sge):
    """N = V = L = (0, 1, 0): NoH = VoH = 1, alpha = 0.25, D = 1 / (pi a2) = 16 / pi, G = 1, F = 0.04: brdf = (1 + 0.16) / pi."""
    r, c = _top_down(sge)
    brdf = 1.16 / 3.14159265
    want = [brdf * 2.0 * k + a + _dither(c, c) for k, a in zip((1.0, 0.9, 0.8), AMBIENT)]
    assert np.abs(r["rgb"][c, c] - want).max() < 1e-6, (r["rgb"][c, c], want)
    assert (r["layers"][c, c], r["instance"][c, c], r["queries"][c, c], r["shadow"][c, c], r["alpha"][c, c]) == (1, STATIC_BASE, 2, 1.0, 1.0)
    assert abs(r["distance"][c, c] - 5.0) < 1e-5 and r["flags"][c, c] == 0


def test_opaque_occluder_leaves_the_ambient(sge):
    """L = (1, 1, 0) / sqrt 2; an opaque quad at (1, 1, 0), outside the centre ray, covers the shadow ray: shadow = 0."""
    r, c = _top_down(sge, extra=[(0.3, (1, 1, 0))], extra_materials=[0], light_dir=(-1, -1, 0))
    want = [a + _dither(c, c) for a in AMBIENT]
    assert np.abs(r["rgb"][c, c] - want).max() < 1e-6 and r["shadow"][c, c] == 0.0 and r["queries"][c, c] == 2


def test_two_half_transparent_occluders_quarter_the_light(sge):
    r, c = _top_down(sge, extra=[(0.3, (1, 1, 0)), (0.3, (2, 2, 0))], extra_materials=[1, 1], light_dir=(-1, -1, 0))
    s = 1 / math.sqrt(2)
    brdf = _brdf_by_hand((0, 1, 0), (0, 1, 0), (s, s, 0), (1, 1, 1), 0.0, 0.5)
    want = [b * 2.0 * k * (s * 0.25) + a + _dither(c, c) for b, k, a in zip(brdf, (1.0, 0.9, 0.8), AMBIENT)]
    assert np.abs(r["rgb"][c, c] - want).max() < 1e-6, (r["rgb"][c, c], want)
    assert r["shadow"][c, c] == 0.25 and r["queries"][c, c] == 4  # the layer's ray, two occluders, the miss behind them


def test_four_stacked_sheets_composite_three_layers(sge):
    r, c = _top_down(sge, extra=[(0.5, (0, y, 0)) for y in (1, 2, 3, 4)], extra_materials=[1, 1, 1, 1], eye_y=6.0)
    assert r["layers"][c, c] == 3 and r["alpha"][c, c] == 0.875 and r["instance"][c, c] == STATIC_BASE + 4
    # every layer: its ray + light 0's walk up through the sheets above it (0, 1, 2 occluders, then the miss)
    assert r["queries"][c, c] == (1 + 1) + (1 + 2) + (1 + 3)


def test_a_miss_is_the_background_and_the_dither(sge):
    r, c = _top_down(sge, eye_y=5.0, target_y=10.0)
    for y in range(3):
        for x in range(3):
            want = [b + _dither(x, y) for b in BG]
            assert np.abs(r["rgb"][y, x] - want).max() < 1e-9
    assert (r["layers"] == 0).all() and (r["instance"] == -1).all() and (r["queries"] == 1).all() and (r["alpha"] == 0).all()


@pytest.fixture(scope="module", params=["full", "rough"])
def statics_render(sge, request):
    """The static half of the GPU test's scene at 48 x 32: path A, path B, and path A shaded in float32."""
    meshes, mesh_of, mats, material_of = rs.static_scene()
    scene = SceneRef(sge, meshes, mesh_of, mats)
    try:
        ref = RenderRef(scene, rs.materials(sge, rough_only=request.param == "rough"), material_of, None, rs.lights(sge))
        eye, target = rs.camera()
        f = rs.frame_record(sge, eye, target, 48, 32, 4)
        yield request.param, ref.render(f, "A"), ref.render(f, "B"), ref.render(f, "A", shade=np.float32)
    finally:
        scene.close()


def test_the_gpu_scenes_are_stable_and_reach_every_branch(statics_render):
    name, a, b, a32 = statics_render
    stable = stable_pixels(a, b)
    print("%s: unstable pixels %d of %d" % (name, (~stable).sum(), stable.size))
    assert (~stable).mean() <= 0.03
    assert set(np.unique(a["layers"])) == {0, 1, 2, 3}
    if name == "full":
        assert (a["flags"] & 1).any()
    assert (a["flags"] & 2).any()
    assert (a["shadow"] < 1).any() and ((a["shadow"] > 0) & (a["shadow"] < 1)).any()
    assert a["queries"].max() >= 10
    err = np.abs(a32["rgb"].astype(np.float64) - a["rgb"])[stable & stable_pixels(a, a32)]
    print("%s: float32 restatement of the shading, worst |f32 - f64| per channel: %s (x 255: %s)" % (name, err.max(0), err.max(0) * 255))
    assert err.max() <= rs.RESTATEMENT_WORST[name], "the constant the GPU test's bar is four times of is this measurement"
    assert rs.colour_bar(name) < 0.25 / 255, "the dither (amplitude 1 / 255) is observable"
    assert np.isfinite(a["rgb"]).all() and (a["rgb"] >= 0).all()
