"""GPU tests of specular IBL in the shaded frame (include/sge_amd_render_ibl.h).

The two samplers alone are held bit for bit to ibl_ref.env_sample / ibl_ref.lut_sample in float32 (the header's order). The frame is
held to render_ibl_ref.IblRenderRef: on stable pixels the integer AOV fields are exact and rgb lies within
render_ibl_scenes.colour_bar — the existing scene's bar, plus 4 x the float32 restatement figure of the scene with the term, plus
what the coordinate bar of R may move the term by. A pixel is stable when paths A and B agree on its trace, no sampled value lies
within the texture tests' margin of a threshold and no R lies within the coordinate bar of a face tie; unstable pixels are at most
3 % of the frame. With no environment, or only one of the two resources, the frame is byte for byte the frame without this header.

Measured on an MI355X (worst |rgb - ref| as a fraction of the bar): see COVERAGE.md (f)."""
import numpy as np
import pytest

import ibl_ref as ir
import render_ibl_ref as rir
import render_ibl_scenes as isc
import render_scenes as rs
import render_tex_scenes as ts
from scene_ref import SceneRef

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine(sge):
    gpu = sge.CharacterEngine(0)
    try:
        yield gpu
    finally:
        gpu.close()


# ---- the samplers, bit for bit ----

def _same_bits(got, want):
    return got.view(np.uint32) == want.view(np.uint32)


CUBES = [(size, mips) for size in (1, 2, 4, 8) for mips in range(1, size.bit_length() + 1)]


@pytest.mark.parametrize("size,mips", CUBES + [(8, 0)])
def test_the_cube_sampler_bit_for_bit(sge, engine, size, mips):
    """Random halves (denormals, the largest finite half) at every admissible mipCount, and (mips = 0) the default cube at 8."""
    if mips == 0:
        mips = 4
        texels = sge.ibl_default_env(size, mips)
    else:
        texels = isc.random_cube(size, mips, 31 * size + mips)
    engine.render_env_upload(size, mips, texels)
    assert engine.render_ibl_info()[:2] == (size, mips)
    dirs = isc.directions(seed=size + mips)
    lods = isc.lods(len(dirs), mips)
    got = engine.render_env_sample(dirs, lods)
    want = ir.env_sample(ir.split_levels(texels, size, mips), dirs, lods, np.float32)
    ok = _same_bits(got, want) | (np.isnan(got) & np.isnan(want))
    faces = set(ir.cube_coord(dirs[np.isfinite(dirs).all(1)])[0].tolist())
    print("cube %d, %d levels: %d samples, %d words differ; faces %s" % (size, mips, len(dirs), (~ok).sum(), sorted(faces)))
    assert faces == set(range(6))
    bad = ~ok.all(1)
    assert not bad.any(), (dirs[bad][:5], lods[bad][:5], got[bad][:5], want[bad][:5])
    engine.render_ibl_clear()


@pytest.mark.parametrize("size", [(1, 1), (2, 2), (5, 3), (16, 16)])
def test_the_table_sampler_bit_for_bit(sge, engine, size):
    w, h = size
    lut = np.random.default_rng(5 * w + h).uniform(-2, 2, (h, w, 4)).astype(np.float32) if w != 16 else sge.ibl_default_brdf_lut(16, 64)
    engine.render_brdf_lut_upload(lut)
    assert engine.render_ibl_info()[2:] == (w, h)
    g = np.linspace(-0.5, 1.5, 41, dtype=np.float32)
    odd = np.array([0.0, -0.0, 1.0, np.inf, -np.inf, np.nan, 0.37], np.float32)
    uvs = np.concatenate([np.stack(np.meshgrid(g, g), -1).reshape(-1, 2), np.stack(np.meshgrid(odd, odd), -1).reshape(-1, 2)]).astype(np.float32)
    got = engine.render_brdf_lut_sample(uvs)
    want = ir.lut_sample(lut, uvs, np.float32)
    bad = ~_same_bits(got, want).all(1)
    print("table %d x %d: %d samples, %d differ" % (w, h, len(uvs), bad.sum()))
    assert not bad.any(), (uvs[bad][:5], got[bad][:5], want[bad][:5])
    engine.render_ibl_clear()


def test_the_device_forms_are_the_batch_forms(sge, engine):
    import torch
    texels = isc.random_cube(4, 3, 9)
    lut = sge.ibl_default_brdf_lut(5, 16)
    engine.render_env_upload(4, 3, texels)
    engine.render_brdf_lut_upload(lut)
    dirs = isc.directions(seed=3, count=400)
    lods = isc.lods(len(dirs), 3)
    uvs = np.random.default_rng(2).uniform(-0.2, 1.2, (300, 2)).astype(np.float32)
    d_dirs, d_lods, d_uvs = (torch.from_numpy(x).to("cuda:0") for x in (dirs, lods, uvs))
    d_rgb = torch.zeros((len(dirs), 3), dtype=torch.float32, device="cuda:0")
    d_out = torch.zeros((len(uvs), 2), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    engine.render_env_sample_device(d_dirs.data_ptr(), d_lods.data_ptr(), len(dirs), d_rgb.data_ptr())
    engine.render_brdf_lut_sample_device(d_uvs.data_ptr(), len(uvs), d_out.data_ptr())
    engine.synchronize()
    assert d_rgb.cpu().numpy().tobytes() == engine.render_env_sample(dirs, lods).tobytes()
    assert d_out.cpu().numpy().tobytes() == engine.render_brdf_lut_sample(uvs).tobytes()
    engine.render_ibl_clear()


# ---- the frame ----

def _check(name, rgba, aov, a, b, a32, gpu, cam, term, bar, restatement_bar):
    H, W = a["layers"].shape
    assert rgba.shape == (H, W, 4) and np.isfinite(rgba).all() and (rgba[..., :3] >= 0).all() and (rgba[..., 3] == 1).all()
    prim = gpu.scene_intersect(np.tile(cam, (H * W, 1)), a["dir"], -1)
    assert np.array_equal(aov["instance"].ravel(), prim["instance"]) and np.array_equal(aov["primitive"].ravel(), prim["primitive"])
    stable = rir.ibl_stable_pixels(a, b, term)
    print("%s: unstable pixels %d of %d" % (name, (~stable).sum(), stable.size))
    assert (~stable).mean() <= 0.03
    for f in ("layers", "instance", "primitive", "queries", "flags"):
        bad = (aov[f] != a[f]) & stable
        assert not bad.any(), (name, f, np.argwhere(bad)[:5], aov[f][bad][:5], a[f][bad][:5])
    both = stable & rir.ibl_stable_pixels(a, a32, term)
    rest = np.abs(a32["rgb"].astype(np.float64) - a["rgb"])[both].max()
    err = np.abs(rgba[..., :3].astype(np.float64) - a["rgb"])[stable]
    print("%s: float32 restatement worst %.4g (bar %.3g); GPU worst |rgb - ref| %.4g = %.3f of the bar %.3g" % (
        name, rest, restatement_bar, err.max(), err.max() / bar, bar))
    assert rest <= restatement_bar, (name, rest)
    assert err.max() <= bar, (name, err.max(), np.argwhere((np.abs(rgba[..., :3] - a["rgb"]).max(-1) > bar) & stable)[:5])


def _renders(ref, f):
    return ref.render(f, "A"), ref.render(f, "B"), ref.render(f, "A", shade=np.float32)


def _setup_statics(sge, gpu):
    meshes, mesh_of, mats, material_of = ts.static_scene()
    ts.upload_scene(gpu, meshes, mesh_of, mats)
    m = isc.materials(sge)
    gpu.render_materials(m)
    gpu.render_static_materials(material_of)
    lights = rs.lights(sge)
    gpu.render_lights(lights)
    return meshes, mesh_of, mats, material_of, m, lights


@pytest.fixture(scope="module")
def statics(sge):
    gpu = sge.CharacterEngine(0)
    meshes, mesh_of, mats, material_of, m, lights = _setup_statics(sge, gpu)
    scene = SceneRef(sge, meshes, mesh_of, mats)
    texels, levels, lut = isc.environment(sge)
    eye, target = rs.camera()
    try:
        yield {"gpu": gpu, "scene": scene, "m": m, "material_of": material_of, "lights": lights, "eye": eye, "target": target,
               "texels": texels, "levels": levels, "lut": lut, "f": rs.frame_record(sge, eye, target, isc.SMALL[0], isc.SMALL[1], 4)}
    finally:
        gpu.close(); scene.close()


def _upload_environment(gpu, c):
    gpu.render_env_upload(isc.ENV_SIZE, isc.ENV_MIPS, c["texels"])
    gpu.render_brdf_lut_upload(c["lut"])


def _reset(sge, gpu):
    gpu.render_ibl_clear()
    gpu.render_texture_clear(-1)
    gpu.render_material_textures(sge.abi.default_render_material_textures(1))


@pytest.mark.parametrize("textured", [False, True])
def test_statics_against_the_reference(sge, statics, textured):
    """render_ibl_kernel / render_ibl_tex_kernel: roughness 0.05 .. 1, metallic 0 .. 1, the mirror, three translucent layers, an
    occlusion below 1. The three overlap modes give the same frame."""
    c = statics
    gpu, f = c["gpu"], c["f"]
    name = "ibl textured" if textured else "ibl"
    tex, bind = (ts.textures(), ts.bindings(sge, 1.0)) if textured else (None, None)
    try:
        plain = gpu.render_frame(f)
        if textured:
            ts.upload_textures(gpu, tex)
            gpu.render_material_textures(bind)
        _upload_environment(gpu, c)
        ref = rir.IblRenderRef(c["scene"], c["m"], c["material_of"], None, c["lights"], tex, bind, table32=gpu.render_srgb_table() if textured else None,
                               levels=c["levels"], lut=c["lut"])
        a, b, a32 = _renders(ref, f)
        assert set(np.unique(a["layers"])) == {0, 1, 2, 3} and (a["flags"] & 1).any() and (a["flags"] & 2).any()
        rgba, aov = gpu.render_frame(f, aov=True)
        assert np.abs(rgba[..., :3] - plain[..., :3]).max() > 0.05, "the environment shows"
        base_bar = ts.colour_bar("textured, normalScale 1", tex, c["lights"], f) if textured else rs.colour_bar("full")
        term = ts.margin_term(tex) if textured else 0.0
        bar = isc.colour_bar(name, base_bar, c["levels"], ref.spec_worst)
        _check(name, rgba, aov, a, b, a32, gpu, np.asarray(c["eye"], np.float32), term, bar, isc.RESTATEMENT_WORST[name])
        for overlap in (1, 2, 0):
            gpu.set_option(sge.abi.OPT_OVERLAP_SKIN, overlap)
            again = gpu.render_frame(f, aov=True)
            assert again[0].tobytes() == rgba.tobytes() and again[1].tobytes() == aov.tobytes(), overlap
    finally:
        _reset(sge, gpu)


@pytest.mark.parametrize("textured", [False, True])
def test_identity_without_an_environment(sge, statics, textured):
    """Nothing uploaded, only the cube, only the table, and after sge_render_ibl_clear: byte for byte the frame of a context that never
    saw an IBL call (image and AOV). A cube of zeros: the same values."""
    c = statics
    gpu, f = c["gpu"], c["f"]
    try:
        if textured:
            ts.upload_textures(gpu, ts.textures())
            gpu.render_material_textures(ts.bindings(sge, 1.0))
        want = gpu.render_frame(f, aov=True)
        same = lambda what: [g.tobytes() for g in gpu.render_frame(f, aov=True)] == [w.tobytes() for w in want] or pytest.fail(what)
        gpu.render_env_upload(isc.ENV_SIZE, isc.ENV_MIPS, c["texels"])
        assert gpu.render_ibl_info() == (isc.ENV_SIZE, isc.ENV_MIPS, 0, 0)
        same("only the cube")
        gpu.render_ibl_clear()
        gpu.render_brdf_lut_upload(c["lut"])
        assert gpu.render_ibl_info() == (0, 0, isc.LUT_SIZE, isc.LUT_SIZE)
        same("only the table")
        gpu.render_env_upload(isc.ENV_SIZE, isc.ENV_MIPS, c["texels"])
        assert gpu.render_frame(f)[..., :3].tobytes() != want[0][..., :3].tobytes()
        zeros = np.zeros_like(c["texels"])
        gpu.render_env_upload(isc.ENV_SIZE, isc.ENV_MIPS, zeros)
        got = gpu.render_frame(f, aov=True)
        assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes(), "a cube of zeros adds 0"
        gpu.render_ibl_clear()
        assert gpu.render_ibl_info() == (0, 0, 0, 0)
        same("after sge_render_ibl_clear")
    finally:
        _reset(sge, gpu)


# ---- a crowd with mesh variants: render_ragged_ibl_kernel, render_ragged_ibl_tex_kernel ----

@pytest.mark.parametrize("layout", ["packed", "padded16"])
def test_variant_crowd_against_the_reference(sge, layout):
    """The scene of test_gpu_render_textures.test_variant_crowd_against_the_reference (two genuinely different mesh variants) with
    the materials' roughness and metallic spread out, untextured and textured. The restatement figure is measured here, beside the
    GPU, between the reference's float32 and float64 shading (the crowd needs the GPU's skinned vertices), and held to the constant of
    render_ibl_scenes."""
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
        m, lights = isc.materials(sge), rv.lights(sge)
        eng.render_materials(m)
        eng.render_static_materials(material_of)
        eng.render_crowd_materials(rv.crowd_materials())
        eng.render_lights(lights)
        texels, levels, lut = isc.environment(sge)
        eng.render_env_upload(isc.ENV_SIZE, isc.ENV_MIPS, texels)
        eng.render_brdf_lut_upload(lut)
        vm = [dict(_mesh(v), tangents=np.tile(np.array([1, 0, 0, 1], np.float32), (SHAPES[v][0], 1))) for v in which]
        crowd = VariantCrowdRef(sge, vm, rec, off, p, n, t, _cols(rv.instances()))
        scene = SceneRef(sge, meshes, mesh_of, mats, crowd=crowd)
        eye, target = rv.camera()
        f = rs.frame_record(sge, eye, target, rv.SIZE[0], rv.SIZE[1], 2)
        for textured in (False, True):
            tex, bind = (ts.textures(), ts.bindings(sge, 1.0)) if textured else (None, None)
            if textured:
                ts.upload_textures(eng, tex)
                eng.render_material_textures(bind)
            ref = rir.IblRenderRef(scene, m, material_of, rv.crowd_materials(), lights, tex, bind, table32=eng.render_srgb_table() if textured else None,
                                   levels=levels, lut=lut)
            a, b, a32 = _renders(ref, f)
            seen = a["instance"][(a["instance"] >= 0) & (a["instance"] < CHARS)]
            assert set(rec[seen].tolist()) == {0, 1}, "primary hits on characters of both variants"
            rgba, aov = eng.render_frame(f, aov=True)
            term = ts.margin_term(tex) if textured else 0.0
            name = "ibl textured variants" if textured else "ibl variants"
            base_bar = ts.colour_bar("textured variants %s" % layout, tex, lights, f) if textured else rs.colour_bar("variants")
            bar = isc.colour_bar(name, base_bar, levels, ref.spec_worst)
            _check("%s %s" % (name, layout), rgba, aov, a, b, a32, eng, np.asarray(eye, np.float32), term, bar, isc.RESTATEMENT_WORST[name])
    finally:
        ctx.eng.close()
        if scene is not None:
            scene.close()
        if crowd is not None:
            crowd.close()


# ---- the contract ----

def test_contract(sge, statics):
    c = statics
    gpu, f, abi = c["gpu"], c["f"], sge.abi
    _reset(sge, gpu)
    plain = gpu.render_frame(f)
    halves = np.zeros(4 * abi.env_texel_count(4, 3), np.uint16)
    lut = np.zeros((2, 3, 4), np.float32)
    one = np.zeros(8, np.float32)
    try:
        for size, mips, data in ((0, 1, halves), (-4, 1, halves), (3, 1, halves), (6, 2, halves), (4096, 1, halves), (4, 0, halves), (4, 4, halves), (4, 3, None)):
            with pytest.raises(sge.SgeError, match="code %d" % abi.SGE_ERR_INVALID):
                gpu._call("render_env_upload", size, mips, abi.ptr(data))
        for w, h, data in ((0, 2, lut), (3, -1, lut), (4097, 1, lut), (3, 2, None)):
            with pytest.raises(sge.SgeError, match="code %d" % abi.SGE_ERR_INVALID):
                gpu._call("render_brdf_lut_upload", w, h, abi.ptr(data))
        assert gpu.render_ibl_info() == (0, 0, 0, 0), "every failed upload changed nothing"
        with pytest.raises(sge.SgeError, match="code %d.*no environment cube" % abi.SGE_ERR_STATE):
            gpu.render_env_sample(np.ones((1, 3), np.float32), np.zeros(1, np.float32))
        with pytest.raises(sge.SgeError, match="code %d.*no BRDF table" % abi.SGE_ERR_STATE):
            gpu.render_brdf_lut_sample(np.zeros((1, 2), np.float32))
        with pytest.raises(sge.SgeError, match="code %d.*no environment cube" % abi.SGE_ERR_STATE):
            gpu._call("render_env_sample_device", abi.ptr(one), abi.ptr(one), 1, abi.ptr(one))
        with pytest.raises(sge.SgeError, match="code %d.*no BRDF table" % abi.SGE_ERR_STATE):
            gpu._call("render_brdf_lut_sample_device", abi.ptr(one), 1, abi.ptr(one))
        assert np.array_equal(gpu.render_frame(f), plain)
        _upload_environment(gpu, c)
        lit = gpu.render_frame(f)
        assert not np.array_equal(lit, plain)
        for size, mips in ((3, 1), (4, 4)):  # a failed upload leaves the cube, and the frame, as they were
            with pytest.raises(sge.SgeError):
                gpu._call("render_env_upload", size, mips, abi.ptr(halves))
        with pytest.raises(sge.SgeError):
            gpu._call("render_brdf_lut_upload", 0, 1, abi.ptr(lut))
        for name, args in (("render_env_sample_batch", (None, None, 1, None)), ("render_brdf_lut_sample_batch", (None, 1, None)),
                           ("render_env_sample_batch", (abi.ptr(one), abi.ptr(one), -1, abi.ptr(one))), ("render_ibl_info_get", (None, None, None, None))):
            with pytest.raises(sge.SgeError, match="bad argument"):
                gpu._call(name, *args)
        assert gpu.render_ibl_info() == (isc.ENV_SIZE, isc.ENV_MIPS, isc.LUT_SIZE, isc.LUT_SIZE)
        assert np.array_equal(gpu.render_frame(f), lit)
        assert gpu.render_env_sample(np.zeros((0, 3), np.float32), np.zeros(0, np.float32)).shape == (0, 3)
        # uploading again replaces the cube: another size, another mipCount
        small = isc.random_cube(2, 1, 4)
        gpu.render_env_upload(2, 1, small)
        assert gpu.render_ibl_info()[:2] == (2, 1)
        d, l = np.array([[0.3, -0.8, 0.5]], np.float32), np.array([0.7], np.float32)
        assert np.array_equal(gpu.render_env_sample(d, l).view(np.uint32), ir.env_sample(ir.split_levels(small, 2, 1), d, l).view(np.uint32))
    finally:
        _reset(sge, gpu)


def test_the_example_shows_the_environment_on_its_platforms(sge, tmp_path):
    """examples/demo_scene.py --render --ibl --image: the same scene and camera as without the flag; the platforms, a rough metal with
    the flag, change; the primary hits do not."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("demo_scene_ibl", os.path.join(root, "examples", "demo_scene.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    images = {}
    for ibl in (False, True):
        gpu = sge.CharacterEngine(0)
        try:
            demo.run(gpu, steps=30, scene=True)
            path = tmp_path / ("i%d.ppm" % ibl)
            aov = demo.shaded_image(gpu, str(path), width=160, height=100, ibl=ibl)
            assert gpu.render_ibl_info() == ((128, 8, 128, 128) if ibl else (0, 0, 0, 0))
            images[ibl] = (np.frombuffer(path.read_bytes()[15:], np.uint8).reshape(100, 160, 3).astype(np.int32), aov)
        finally:
            gpu.close()
    (plain, aov0), (lit, aov1) = images[False], images[True]
    assert np.array_equal(aov0["instance"], aov1["instance"]) and np.array_equal(aov0["primitive"], aov1["primitive"])
    platforms = aov1["instance"] >= sge.abi.SCENE_STATIC_BASE + 2
    assert platforms.sum() > 50
    changed = (plain[platforms] != lit[platforms]).any(1)
    print("platform pixels that changed with --ibl: %d of %d" % (changed.sum(), platforms.sum()))
    assert changed.mean() > 0.9
