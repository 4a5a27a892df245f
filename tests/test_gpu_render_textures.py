"""GPU tests of textures in the shaded frame (include/sge_amd_render_textures.h).

The sampler alone is held bit for bit to render_tex_ref.sample in float32 (the header's order, the library's own sRGB table, which is
held within 1 float32 ulp of the float64 formula). The frame is held to render_tex_ref.TexRenderRef by the checks of
test_gpu_render._check: the primary-ray AOV fields equal sge_scene_intersect_batch on every pixel; on stable pixels the integer AOV
fields are exact, distance / shadow / alpha within 1e-6 relative and rgb within render_tex_scenes.colour_bar — 4 x the scene's
float32 restatement figure plus what the uv bar of scene_ref.assert_records_match may move a sample by on its way into rgb. A pixel
is stable when paths A and B agree on its trace and no sampled value lies closer to a threshold it feeds than
render_tex_scenes.margin_term; unstable pixels are at most 3 % of the frame.

Measured on an MI355X (worst |rgb - ref| as a fraction of the bar): see COVERAGE.md (f)."""
import numpy as np
import pytest

import oracle_binding as ob
import render_scenes as rs
import render_tex_ref as tr
import render_tex_scenes as ts
from scene_ref import SceneRef
from scenes import build_scene

pytestmark = pytest.mark.gpu


# ---- the sampler, bit for bit ----

def _texture(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def _uvs(w, h):
    g = np.linspace(-0.5, 1.5, 33, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
    cx, cy = (np.arange(w, dtype=np.float32) + np.float32(0.5)) / np.float32(w), (np.arange(h, dtype=np.float32) + np.float32(0.5)) / np.float32(h)
    ex, ey = np.arange(w + 1, dtype=np.float32) / np.float32(w), np.arange(h + 1, dtype=np.float32) / np.float32(h)
    centres = np.stack(np.meshgrid(cx, cy), -1).reshape(-1, 2)
    edges = np.stack(np.meshgrid(ex, ey), -1).reshape(-1, 2)
    odd = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 0.37], np.float32)
    special = np.stack(np.meshgrid(odd, odd), -1).reshape(-1, 2)
    return np.ascontiguousarray(np.concatenate([lattice, centres, edges, special]), np.float32)


@pytest.fixture(scope="module")
def engine(sge):
    gpu = sge.CharacterEngine(0)
    try:
        yield gpu
    finally:
        gpu.close()


def test_the_srgb_table_is_the_formula_within_one_ulp(engine):
    table = engine.render_srgb_table()
    want = tr.srgb_table64()
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    err = np.abs(table.astype(np.float64) - want)
    print("sRGB table: worst |table - formula| = %.3g ulp" % (err[1:] / ulp[1:]).max())
    assert table[0] == 0 and table[255] == 1 and (err <= ulp).all() and (np.diff(table) > 0).all()


@pytest.mark.parametrize("size", [(1, 1), (2, 2), (1, 5), (5, 1), (3, 4), (64, 64)])
@pytest.mark.parametrize("srgb", [False, True])
def test_the_sampler_bit_for_bit(engine, size, srgb):
    w, h = size
    rgba = _texture(w, h, 7 * w + h)
    engine.render_texture_upload(3, rgba, srgb=srgb)
    assert engine.render_texture_info(3) == (w, h, int(srgb))
    uvs = _uvs(w, h)
    got = engine.render_texture_sample(3, uvs)
    want = tr.sample(rgba, srgb, uvs, np.float32, table=engine.render_srgb_table())
    bad = got.view(np.uint32) != want.view(np.uint32)
    print("%dx%d srgb=%d: %d samples, %d words differ" % (w, h, srgb, len(uvs), bad.sum()))
    assert not bad.any(), (uvs[bad.any(1)][:5], got[bad.any(1)][:5], want[bad.any(1)][:5])
    # the float64 sampler agrees to rounding: the pinned order is a restatement of the filter, not another filter
    finite = np.isfinite(uvs).all(1)
    w64 = tr.sample(rgba, srgb, uvs[finite].astype(np.float64), np.float64)
    assert np.abs(got[finite] - w64).max() <= 2e-6 * max(w, h)


def test_the_device_form_is_the_batch_form(sge, engine):
    import torch
    rgba = _texture(5, 3, 11)
    engine.render_texture_upload(4, rgba, srgb=True)
    uvs = _uvs(5, 3)
    d_uv = torch.from_numpy(uvs).to("cuda:0")
    d_out = torch.zeros((len(uvs), 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    engine.render_texture_sample_device(4, d_uv.data_ptr(), len(uvs), d_out.data_ptr())
    engine.synchronize()
    assert d_out.cpu().numpy().tobytes() == engine.render_texture_sample(4, uvs).tobytes()


# ---- the frame ----

def _check(name, rgba, aov, a, b, a32, gpu, frame, cam, tex, lights):
    H, W = a["layers"].shape
    assert rgba.shape == (H, W, 4) and np.isfinite(rgba).all() and (rgba[..., :3] >= 0).all() and (rgba[..., 3] == 1).all()
    prim = gpu.scene_intersect(np.tile(cam, (H * W, 1)), a["dir"], -1)
    assert np.array_equal(aov["instance"].ravel(), prim["instance"]) and np.array_equal(aov["primitive"].ravel(), prim["primitive"])
    assert np.array_equal(aov["distance"].ravel().view(np.uint32), prim["distance"].view(np.uint32))
    term = ts.margin_term(tex)
    stable = tr.tex_stable_pixels(a, b, term)
    print("%s: unstable pixels %d of %d (threshold margin %.3g)" % (name, (~stable).sum(), stable.size, term))
    assert (~stable).mean() <= 0.03
    for f in ("layers", "instance", "primitive", "queries", "flags"):
        bad = (aov[f] != a[f]) & stable
        assert not bad.any(), (name, f, np.argwhere(bad)[:5], aov[f][bad][:5], a[f][bad][:5])
    for f in ("distance", "shadow", "alpha"):
        err = np.abs(aov[f].astype(np.float64) - a[f])[stable].max()
        # shadow is a product over at most four occluders' sampled alphas, alpha a composite of at most three: each may move by term
        bar = 1e-6 * max(1.0, np.abs(a[f]).max()) + (4 * term if f != "distance" else 0.0)
        assert err <= bar, (name, f, err)
    both = stable & tr.tex_stable_pixels(a, a32, term)
    rest = np.abs(a32["rgb"].astype(np.float64) - a["rgb"])[both].max()
    bar = ts.colour_bar(name, tex, lights, frame)
    err = np.abs(rgba[..., :3].astype(np.float64) - a["rgb"])[stable]
    print("%s: float32 restatement worst %.4g (constant %.3g); GPU worst |rgb - ref| %.4g = %.2f of the bar %.3g" % (
        name, rest, ts.RESTATEMENT_WORST[name], err.max(), err.max() / bar, bar))
    assert rest <= ts.RESTATEMENT_WORST[name], (name, rest)
    assert err.max() <= bar, (name, err.max(), np.argwhere((np.abs(rgba[..., :3] - a["rgb"]).max(-1) > bar) & stable)[:5])


def _renders(ref, f):
    return ref.render(f, "A"), ref.render(f, "B"), ref.render(f, "A", shade=np.float32)


def _setup_statics(sge, gpu, u=1.0, origin=(0, 0, 0)):
    meshes, mesh_of, mats, material_of = ts.static_scene(u, origin)
    ts.upload_scene(gpu, meshes, mesh_of, mats)
    m = rs.materials(sge)
    gpu.render_materials(m)
    gpu.render_static_materials(material_of)
    lights = rs.lights(sge, reach=8.0 * u)
    gpu.render_lights(lights)
    return meshes, mesh_of, mats, material_of, m, lights


@pytest.fixture(scope="module")
def statics(sge):
    gpu = sge.CharacterEngine(0)
    meshes, mesh_of, mats, material_of, m, lights = _setup_statics(sge, gpu)
    scene = SceneRef(sge, meshes, mesh_of, mats)
    try:
        yield {"gpu": gpu, "scene": scene, "m": m, "material_of": material_of, "lights": lights, "eye": rs.camera()[0], "target": rs.camera()[1]}
    finally:
        gpu.close(); scene.close()


@pytest.mark.parametrize("normal_scale", [1, 6])
def test_statics_every_sampling_site(sge, statics, normal_scale):
    c = statics
    gpu = c["gpu"]
    tex, bind = ts.textures(), ts.bindings(sge, float(normal_scale))
    ts.upload_textures(gpu, tex)
    gpu.render_material_textures(bind)
    try:
        ref = tr.TexRenderRef(c["scene"], c["m"], c["material_of"], None, c["lights"], tex, bind, table32=gpu.render_srgb_table())
        f = rs.frame_record(sge, c["eye"], c["target"], 48, 32, 4)
        a, b, a32 = _renders(ref, f)
        mirror_box = a["instance"] == sge.abi.SCENE_STATIC_BASE + 2
        on_mirror = (a["flags"][mirror_box] & 1) != 0
        assert on_mirror.any() and not on_mirror.all(), "the metallic-roughness texture splits the mirror box"
        assert set(np.unique(a["layers"])) == {0, 1, 2, 3} and (a["flags"] & 2).any() and ((a["shadow"] > 0) & (a["shadow"] < 1)).any()
        rgba, aov = gpu.render_frame(f, aov=True)
        _check("textured, normalScale %d" % normal_scale, rgba, aov, a, b, a32, gpu, f, np.asarray(c["eye"], np.float32), tex, c["lights"])
        plain = rs.frame_record(sge, c["eye"], c["target"], 48, 32, 4)
        gpu.render_texture_clear(-1)
        assert np.abs(gpu.render_frame(plain)[..., :3] - rgba[..., :3]).max() > 0.05, "the textures show"
    finally:
        gpu.render_texture_clear(-1)
        gpu.render_material_textures(sge.abi.default_render_material_textures(1))


def test_untextured_identity(sge, statics):
    """Bindings that all name empty slots, and a frame after sge_render_texture_clear(-1), are the frame of a context that never saw
    a texture call, byte for byte (image and AOV records)."""
    c = statics
    f = rs.frame_record(sge, c["eye"], c["target"], 48, 32, 4)
    fresh = sge.CharacterEngine(0)
    try:
        _setup_statics(sge, fresh)
        want = fresh.render_frame(f, aov=True)
    finally:
        fresh.close()
    gpu = c["gpu"]
    try:
        gpu.render_texture_clear(-1)
        gpu.render_material_textures(ts.bindings(sge))
        got = gpu.render_frame(f, aov=True)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), "bindings that name empty slots"
        ts.upload_textures(gpu, ts.textures())
        assert gpu.render_frame(f)[..., :3].tobytes() != want[0][..., :3].tobytes()
        gpu.render_texture_clear(-1)
        got = gpu.render_frame(f, aov=True)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), "after sge_render_texture_clear(-1)"
    finally:
        gpu.render_texture_clear(-1)
        gpu.render_material_textures(sge.abi.default_render_material_textures(1))


# ---- the crowd: the skinned normal and tangent streams in the frame ----

def _crowd(sge, layout, n=3):
    gpu, cpu = sge.CharacterEngine(0), ob.oracle_engine()
    gpu.set_option(sge.abi.OPT_SKIN_LAYOUT, sge.abi.LAYOUT_PADDED16 if layout == "padded16" else sge.abi.LAYOUT_PACKED)
    for e in (gpu, cpu):
        build_scene(sge, e, n, terrain_cells=(24, 16), rings=9, segments=8, mixed=True, seed=5)
        e.blas_build(e.mesh["indices"])
    V = gpu.vertex_count
    uvs = np.ascontiguousarray(np.stack([(np.arange(V) % 17) / 16.0, (np.arange(V) % 29) / 28.0], -1), np.float32)
    for e in (gpu, cpu):
        e.blas_set_uvs(uvs)
    gpu.tick(stages=sge.abi.STAGE_ALL | sge.abi.STAGE_BLAS_REFIT)
    gp, gn, gt = gpu.skinned()
    ob.skinned_upload(cpu, gp, gn, gt)  # both sides look at the same skinned vertices
    return gpu, cpu, gp


def _crowd_view(gp):
    lo, hi = gp.min(0).astype(np.float64), gp.max(0).astype(np.float64)
    u = float(max((hi - lo).max(), 1e-3)) / 2.5
    origin = np.array([(lo[0] + hi[0]) / 2, lo[1] - 0.02 * u, hi[2] + 1.2 * u])
    eye = origin + (0.4 * u, 3.4 * u, 5.6 * u)
    target = np.array([(lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, (lo[2] + hi[2]) / 2 + 0.8 * u])
    return u, origin, eye, target


@pytest.mark.parametrize("layout", ["packed", "padded16"])
def test_crowd_after_a_tick(sge, layout):
    """Three characters with base colour and normal map on their material: the frame reads the skinned normal and tangent streams.
    Overlap modes 0, 1 and 2 give the same frame."""
    gpu, cpu, gp = _crowd(sge, layout)
    scene = None
    try:
        u, origin, eye, target = _crowd_view(gp)
        meshes, mesh_of, mats, material_of, m, lights = _setup_statics(sge, gpu, u=u, origin=origin)
        crowd_materials = [6, 6, 6]
        gpu.render_crowd_materials(crowd_materials)
        tex, bind = ts.textures(), ts.bindings(sge, 1.0)
        ts.upload_textures(gpu, tex)
        gpu.render_material_textures(bind)
        scene = SceneRef(sge, meshes, mesh_of, mats, crowd=cpu)
        ref = tr.TexRenderRef(scene, m, material_of, crowd_materials, lights, tex, bind, table32=gpu.render_srgb_table())
        f = rs.frame_record(sge, eye, target, 48, 32, 4)
        a, b, a32 = _renders(ref, f)
        assert {0, 1, 2} <= set(np.unique(a["instance"]).tolist())
        rgba, aov = gpu.render_frame(f, aov=True)
        _check("textured crowd %s" % layout, rgba, aov, a, b, a32, gpu, f, np.asarray(eye, np.float32), tex, lights)
        if layout == "packed":
            for overlap in (1, 2, 0):
                gpu.set_option(sge.abi.OPT_OVERLAP_SKIN, overlap)
                again = gpu.render_frame(f, aov=True)
                assert again[0].tobytes() == rgba.tobytes() and again[1].tobytes() == aov.tobytes(), overlap
    finally:
        gpu.close(); cpu.close()
        if scene is not None:
            scene.close()


# ---- a crowd with mesh variants: render_ragged_textured_kernel ----

@pytest.mark.parametrize("layout", ["packed", "padded16"])
def test_variant_crowd_against_the_reference(sge, layout):
    """Two genuinely different mesh variants (1,001 and 300 vertices, alternating over the 37 characters of the variant world) in the
    scene of tests/render_variant_scenes.py, its statics with uvs: base colour and normal map on the characters' material (each
    variant's own uvs, the ragged normal and tangent streams), the alpha checker on the translucent characters and the sheet, the
    metallic-roughness texture on the mirror wall. Held to TexRenderRef over SceneRef + VariantCrowdRef."""
    import render_variant_scenes as rv
    from test_gpu_variant_blas import CHARS, SHAPES, _Ctx, _cols, _mesh, _palettes
    from variant_scene_ref import VariantCrowdRef
    which = (1, 3)
    ctx = _Ctx(sge, layout, which)
    scene = crowd = None
    try:
        eng = ctx.eng
        ctx.write_palettes(_palettes())
        eng.blas_instances(_cols(rv.instances()))
        eng.set_mesh_variants(np.arange(CHARS) % 2)
        ctx.tick()
        st = eng.scene_crowd_status()
        assert (st.crowdReady, st.ragged) == (1, 1)
        off = eng.vertex_offsets()
        p, n, t = eng.skinned(0, int(off[-1]))
        _, rec = eng.blas_variant_bounds()
        _, mesh_of, mats, material_of = rv.statics()
        meshes = {0: ts.quad_uv(1.0), 1: ts.box_uv()}
        ts.upload_scene(eng, meshes, mesh_of, mats)
        m, lights = rs.materials(sge), rv.lights(sge)
        eng.render_materials(m)
        eng.render_static_materials(material_of)
        eng.render_crowd_materials(rv.crowd_materials())
        eng.render_lights(lights)
        tex, bind = ts.textures(), ts.bindings(sge, 1.0)
        ts.upload_textures(eng, tex)
        eng.render_material_textures(bind)
        vm = [dict(_mesh(v), tangents=np.tile(np.array([1, 0, 0, 1], np.float32), (SHAPES[v][0], 1))) for v in which]
        crowd = VariantCrowdRef(sge, vm, rec, off, p, n, t, _cols(rv.instances()))
        scene = SceneRef(sge, meshes, mesh_of, mats, crowd=crowd)
        ref = tr.TexRenderRef(scene, m, material_of, rv.crowd_materials(), lights, tex, bind, table32=eng.render_srgb_table())
        eye, target = rv.camera()
        f = rs.frame_record(sge, eye, target, rv.SIZE[0], rv.SIZE[1], 2)
        a, b, a32 = _renders(ref, f)
        seen = a["instance"][(a["instance"] >= 0) & (a["instance"] < CHARS)]
        assert set(rec[seen].tolist()) == {0, 1}, "primary hits on characters of both variants"
        rgba, aov = eng.render_frame(f, aov=True)
        _check("textured variants %s" % layout, rgba, aov, a, b, a32, eng, f, np.asarray(eye, np.float32), tex, lights)
    finally:
        ctx.eng.close()
        if scene is not None:
            scene.close()
        if crowd is not None:
            crowd.close()


# ---- the contract ----

def test_contract(sge, statics):
    c = statics
    gpu = c["gpu"]
    abi = sge.abi
    f = rs.frame_record(sge, c["eye"], c["target"], 8, 4, 4)
    gpu.render_texture_clear(-1)
    gpu.render_material_textures(abi.default_render_material_textures(1))
    plain = gpu.render_frame(f)
    good = np.full((2, 3, 4), 200, np.uint8)
    try:
        for slot, w, h, fmt, data, match in ((-1, 3, 2, 0, good, "slot"), (32, 3, 2, 0, good, "slot"), (0, 0, 2, 0, good, "dimension"), (0, 3, -1, 0, good, "dimension"),
                                             (0, abi.SGE_MAX_TEXTURE_DIM + 1, 1, 0, good, "dimension"), (0, 3, 2, 2, good, "format"), (0, 3, 2, -1, good, "format"),
                                             (0, 3, 2, 0, None, "bad argument")):
            with pytest.raises(sge.SgeError, match=match):
                gpu._call("render_texture_upload", slot, w, h, fmt, abi.ptr(data))
        assert all(gpu.render_texture_info(s) == (0, 0, 0) for s in range(32)), "every failed upload changed nothing"
        with pytest.raises(sge.SgeError, match="bad argument"):
            gpu.render_texture_clear(32)
        with pytest.raises(sge.SgeError, match="bad argument"):
            gpu.render_texture_clear(-2)
        with pytest.raises(sge.SgeError, match="bad argument"):
            gpu.render_texture_info(32)
        with pytest.raises(sge.SgeError, match="code %d.*holds no texture" % abi.SGE_ERR_STATE):
            gpu.render_texture_sample(0, np.zeros((1, 2), np.float32))
        with pytest.raises(sge.SgeError, match="bad argument"):
            gpu.render_texture_sample(32, np.zeros((1, 2), np.float32))
        with pytest.raises(sge.SgeError, match="bad argument"):
            gpu._call("render_texture_sample_batch", 0, None, 1, None)
        with pytest.raises(sge.SgeError, match="bad argument"):
            gpu._call("render_srgb_table_get", None)
        with pytest.raises(sge.SgeError, match="SGE_MAX_RENDER_MATERIALS"):
            gpu.render_material_textures(abi.default_render_material_textures(257))
        with pytest.raises(sge.SgeError, match="SGE_MAX_RENDER_MATERIALS"):
            gpu._call("render_material_textures_set", 0, abi.ptr(abi.default_render_material_textures(1)))
        # re-upload of a slot with another size replaces it
        gpu.render_texture_upload(0, good, srgb=False)
        assert gpu.render_texture_info(0) == (3, 2, 0)
        big = _texture(7, 5, 3)
        gpu.render_texture_upload(0, big, srgb=True)
        assert gpu.render_texture_info(0) == (7, 5, 1)
        uv = np.array([[0.3, 0.6]], np.float32)
        assert np.array_equal(gpu.render_texture_sample(0, uv), tr.sample(big, True, uv, np.float32, gpu.render_srgb_table()))
        # a non-finite normalScale changes nothing
        bind = abi.default_render_material_textures(7)
        bind["baseColor"][5] = 0
        gpu.render_material_textures(bind)
        ground = gpu.render_frame(f)
        assert not np.array_equal(ground, plain), "the ground is textured"
        bad = bind.copy(); bad["normalScale"][2] = np.nan; bad["baseColor"][5] = -1
        with pytest.raises(sge.SgeError, match="normalScale"):
            gpu.render_material_textures(bad)
        assert np.array_equal(gpu.render_frame(f), ground)
        # sge_render_materials_set keeps the bindings
        gpu.render_materials(rs.materials(sge))
        assert np.array_equal(gpu.render_frame(f), ground)
        # sge_render_material_textures_set resets the bindings beyond count
        gpu.render_material_textures(bind[:5])
        assert np.array_equal(gpu.render_frame(f), plain), "material 5 is beyond the new count: no texture"
        gpu.render_material_textures(bind)
        assert np.array_equal(gpu.render_frame(f), ground)
        # an index >= 32 or of an empty slot is no texture; clearing one slot
        odd = bind.copy(); odd["baseColor"][5] = 32; odd["normal"][1] = 9
        gpu.render_material_textures(odd)
        assert np.array_equal(gpu.render_frame(f), plain)
        gpu.render_material_textures(bind)
        gpu.render_texture_clear(0)
        assert gpu.render_texture_info(0) == (0, 0, 0) and np.array_equal(gpu.render_frame(f), plain)
    finally:
        gpu.render_texture_clear(-1)
        gpu.render_material_textures(abi.default_render_material_textures(1))


def test_the_example_draws_a_checkered_ground_and_a_textured_player(sge, tmp_path):
    """examples/demo_scene.py --render --image --textures: the same scene and camera as without the flag; the ground shows the
    checkerboard's two tones, the player's pixels change, the mirror's primary hits do not."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("demo_scene_textures", os.path.join(root, "examples", "demo_scene.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    images = {}
    for textures in (False, True):
        gpu = sge.CharacterEngine(0)
        try:
            demo.run(gpu, steps=30, scene=True, textures=textures)
            path = tmp_path / ("t%d.ppm" % textures)
            aov = demo.shaded_image(gpu, str(path), width=160, height=100, textures=textures)
            images[textures] = (np.frombuffer(path.read_bytes()[15:], np.uint8).reshape(100, 160, 3).astype(np.int32), aov)
        finally:
            gpu.close()
    (plain, aov0), (tex, aov1) = images[False], images[True]
    assert np.array_equal(aov0["instance"], aov1["instance"]) and np.array_equal(aov0["primitive"], aov1["primitive"])
    base = sge.abi.SCENE_STATIC_BASE
    ground = (aov1["instance"] == base) & (aov1["shadow"] == 1) & (aov1["layers"] == 1)
    player = aov1["instance"] == 0
    assert ground.sum() > 500 and player.any()
    spread = lambda img: np.ptp(img[ground].sum(1))
    print("ground: spread of r + g + b, plain %d, textured %d; player pixels that changed: %d of %d" % (
        spread(plain), spread(tex), (plain[player] != tex[player]).any(1).sum(), player.sum()))
    assert spread(tex) > spread(plain) + 60, "two tones on the ground"
    assert (plain[player] != tex[player]).any(1).mean() > 0.5
