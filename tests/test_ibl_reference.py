"""CPU tests of the specular IBL reference (tests/ibl_ref.py, tests/render_ibl_ref.py) and of the host builders of
include/sge_amd_render_ibl.h: the default cube against the float64 restatement of IBLResources.init rounded to half, the default
table against it within ibl_ref's LUT_BAR, seven deliberately wrong restatements that each miss their bar by a wide factor, the
float32 sampler against the float64 one, and the figures the GPU frame tests' bar is built from."""
import numpy as np
import pytest

import ibl_ref as ir
import render_ibl_ref as rir
import render_ibl_scenes as isc
import render_scenes as rs
import render_tex_scenes as ts
from scene_ref import SceneRef


def _cube_check(got, want64):
    """-> (texels' channels that differ at all, worst distance in units in the last place of float16)"""
    w16 = want64.astype(np.float16)
    ulp = np.spacing(np.abs(w16)).astype(np.float64)
    return int((got.view(np.uint16) != w16.view(np.uint16)).sum()), float((np.abs(got.astype(np.float64) - w16.astype(np.float64)) / ulp).max())


@pytest.mark.parametrize("size,mips", [(8, 4), (1, 1)])
def test_the_default_cube(sge, size, mips):
    got = sge.ibl_default_env(size, mips)
    differ, worst = _cube_check(got, ir.join_levels(ir.default_env64(size, mips)))
    print("default cube %d, %d levels: %d of %d halves differ from the float64 restatement rounded to half; worst %.3g ulp" % (size, mips, differ, got.size, worst))
    assert got.shape == (sge.abi.env_texel_count(size, mips), 4) and worst <= 1.0
    assert (got[:, 3].view(np.uint16) == 0x3C00).all(), "alpha is exactly 1.0"


@pytest.mark.parametrize("size", [8, 1])
def test_the_default_table(sge, size):
    got = sge.ibl_default_brdf_lut(size, 256)
    want, bar = ir.default_brdf_lut64(size, 256, terms=True)
    ratio = np.abs(got[..., :2].astype(np.float64) - want) / bar[..., None]
    print("default table %d x %d, 256 samples: worst |builder - float64| = %.3f of LUT_BAR (bar %.3g .. %.3g)" % (size, size, ratio.max(), bar.min(), bar.max()))
    assert ratio.max() <= 1.0 and (got[..., 2:] == 0).all() and np.isfinite(got).all()


def _sampler_inputs(levels, count=4000, seed=11, margin=1e-3):
    """Random unit directions and lods, bounded away from face ties and from tap switches (a texel coordinate within `margin` texels
    of an integer, at either level used) by `margin`."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(count, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    lod = rng.uniform(0, len(levels) - 1, count)
    keep = ir.tie_margin(d) >= margin
    _, u, v = ir.cube_coord(d)
    for l in range(len(levels)):
        n = levels[l].shape[1]
        for c in (u, v):
            x = (c + 1) * 0.5 * n - 0.5
            keep &= np.abs(x - np.rint(x)) >= margin
    keep &= np.abs(lod - np.rint(lod)) >= margin
    return d[keep], lod[keep]


def test_the_float32_sampler_against_the_float64_one(sge):
    texels, levels, lut = isc.environment(sge)
    d, lod = _sampler_inputs(levels)
    e32 = ir.env_sample(levels, d, lod, np.float32).astype(np.float64)
    e64 = ir.env_sample(levels, d, lod, np.float64)
    uv = np.random.default_rng(3).uniform(0, 1, (4000, 2))
    l32, l64 = ir.lut_sample(lut, uv, np.float32).astype(np.float64), ir.lut_sample(lut, uv, np.float64)
    worst_env, worst_lut = np.abs(e32 - e64).max(), np.abs(l32 - l64).max()
    print("sampler float32 against float64 on %d directions (margin 1e-3): cube %.3g, table %.3g" % (len(d), worst_env, worst_lut))
    # a coordinate carries about 4 roundings of a value up to the face size; a texel's weight moves by that, between texels at most
    # adjacent_step apart, on two axes and two levels; the filter's own sums add a few units of the value
    bar = 2.0 ** -24 * (4 * isc.ENV_SIZE * ir.adjacent_step(levels) * 4 + 8)
    assert len(d) > 3000 and worst_env <= bar and worst_lut <= 2.0 ** -24 * (4 * isc.LUT_SIZE * 2 * np.abs(lut).max() + 8)


def test_wrong_restatements_miss_their_bars(sge):
    """Each deliberately wrong restatement, against what the right one is held to, misses by a wide, printed factor."""
    factors = {}
    got = sge.ibl_default_brdf_lut(8, 256)
    for variant in ("k_direct", "swap_ab", "unclamped_ndotv"):
        want, bar = ir.default_brdf_lut64(8, 256, variant=variant, terms=True)
        with np.errstate(all="ignore"):
            r = np.abs(got[..., :2].astype(np.float64) - want) / bar[..., None]
        factors[variant] = float(np.nanmax(np.where(np.isfinite(r), r, 1e30)))
    cube = sge.ibl_default_env(8, 4)
    factors["flip_v"] = _cube_check(cube, ir.join_levels(ir.default_env64(8, 4, variant="flip_v")))[1]
    # the sampler's variants, against the float32-to-float64 bar of the sampler test, through eval_spec_ibl on a rough metal
    texels, levels, lut = isc.environment(sge)
    rng = np.random.default_rng(5)
    k = 3000
    N = rng.normal(size=(k, 3)); N /= np.linalg.norm(N, axis=1, keepdims=True)
    V = rng.normal(size=(k, 3)); V /= np.linalg.norm(V, axis=1, keepdims=True)
    V = np.where(((N * V).sum(1) < 0)[:, None], -V, V)
    rough, metal, base = rng.uniform(0.05, 1, k), np.ones(k), np.tile([0.9, 0.8, 0.7], (k, 1))
    right = ir.eval_spec_ibl(levels, lut, N, V, rough, metal, base, np.float64)
    bar = 2.0 ** -24 * (4 * isc.ENV_SIZE * ir.adjacent_step(levels) * 4 + 8)
    for variant in ("face_clamp", "round_level", "reflect_v"):
        wrong = ir.eval_spec_ibl(levels, lut, N, V, rough, metal, base, np.float64, variant=variant)
        factors[variant] = float(np.abs(wrong - right).max() / bar)
    for variant, factor in factors.items():
        print("wrong restatement %-16s misses its bar by %.3g x" % (variant, factor))
        assert factor > 100, variant


@pytest.mark.parametrize("textured", [False, True])
def test_the_frame_reference_and_its_figures(sge, textured):
    """The static scene with the term, on the CPU: the float32 restatement figure that feeds the GPU test's bar does not exceed the
    constant of render_ibl_scenes; the reference's two paths alone leave at most 3 % of the pixels unstable; the term shows; a
    wrong R misses the frame's bar."""
    name = "ibl textured" if textured else "ibl"
    meshes, mesh_of, mats, material_of = ts.static_scene()
    scene = SceneRef(sge, meshes, mesh_of, mats)
    try:
        m, lights = isc.materials(sge), rs.lights(sge)
        assert {0.3, 0.7, 1.0} <= set(np.round(m["roughness"].astype(float), 3)) and {0.0, 0.5, 1.0} <= set(m["metallic"].astype(float))
        texels, levels, lut = isc.environment(sge)
        eye, target = rs.camera()
        f = rs.frame_record(sge, eye, target, isc.SMALL[0], isc.SMALL[1], 4)
        tex, bind = (ts.textures(), ts.bindings(sge, 1.0)) if textured else (None, None)
        ref = rir.IblRenderRef(scene, m, material_of, None, lights, tex, bind, levels=levels, lut=lut)
        a, b, a32 = ref.render(f, "A"), ref.render(f, "B"), ref.render(f, "A", shade=np.float32)
        term = ts.margin_term(tex) if textured else 0.0
        stable = rir.ibl_stable_pixels(a, b, term)
        both = stable & rir.ibl_stable_pixels(a, a32, term)
        rest = np.abs(a32["rgb"].astype(np.float64) - a["rgb"])[both].max()
        plain = rir.IblRenderRef(scene, m, material_of, None, lights, tex, bind).render(f, "A")
        base_bar = ts.colour_bar("textured, normalScale 1", tex, lights, f) if textured else rs.colour_bar("full")
        bar = isc.colour_bar(name, base_bar, levels, ref.spec_worst)
        wrong = rir.IblRenderRef(scene, m, material_of, None, lights, tex, bind, levels=levels, lut=lut, ibl_variant="reflect_v").render(f, "A")
        miss = np.abs(wrong["rgb"] - a["rgb"])[stable].max() / bar
        print("%s: unstable %d of %d; float32 restatement %.4g (constant %.3g); the term adds up to %.3g; bar %.3g; reflect(V, N) misses it by %.3g x" % (
            name, (~stable).sum(), stable.size, rest, isc.RESTATEMENT_WORST[name], np.abs(a["rgb"] - plain["rgb"]).max(), bar, miss))
        assert (~stable).mean() <= 0.03 and rest <= isc.RESTATEMENT_WORST[name]
        assert set(np.unique(a["layers"])) == {0, 1, 2, 3} and (a["flags"] & 1).any() and (a["flags"] & 2).any()
        assert np.abs(a["rgb"] - plain["rgb"]).max() > 0.05 and miss > 100
    finally:
        scene.close()
