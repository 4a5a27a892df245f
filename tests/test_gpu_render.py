"""GPU tests of the shaded frame (include/sge_amd_render.h): raytraceKernel's layers, lights and bounces over the ray scene.

Reference: render_ref.RenderRef — the Metal text over scene_ref.SceneRef's triangle scan, path A (float32 rays in the header's
pinned order) and path B (float64 rays); a pixel is *stable* when both issue the same queries with the same answers and branches.
Bars: the primary-ray AOV fields equal sge_scene_intersect_batch on path A's primary rays on every pixel; on stable pixels layers /
instance / primitive / queries / flags are exact, distance / shadow / alpha within the 1e-6 relative bar of assert_records_match, and
rgb within 4 x the scene's float32 restatement figure (render_scenes.RESTATEMENT_WORST); on unstable pixels values are finite, >= 0, alpha 1.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import render_scenes as rs
from render_ref import BG, RenderRef, hash12_rt, stable_pixels
from scene_ref import STATIC_BASE, SceneRef, columns
from scenes import build_scene

pytestmark = pytest.mark.gpu

# rgb bar of a scene: 4 x the worst |float32 restatement - float64| of the shading over its stable pixels, the rule of the float64
# pins (COVERAGE.md); the per-scene figures are the constants of render_scenes.RESTATEMENT_WORST.


def _check(name, rgba, aov, a, b, a32, gpu, frame, cam):
    H, W = a["layers"].shape
    assert rgba.shape == (H, W, 4) and np.isfinite(rgba).all() and (rgba[..., :3] >= 0).all() and (rgba[..., 3] == 1).all()
    # the primary ray: the whole-scene query on path A's rays, every pixel
    prim = gpu.scene_intersect(np.tile(cam, (H * W, 1)), a["dir"], -1)
    assert np.array_equal(aov["instance"].ravel(), prim["instance"]) and np.array_equal(aov["primitive"].ravel(), prim["primitive"])
    assert np.array_equal(aov["distance"].ravel().view(np.uint32), prim["distance"].view(np.uint32))
    stable = stable_pixels(a, b)
    print("%s: unstable pixels %d of %d" % (name, (~stable).sum(), stable.size))
    assert (~stable).mean() <= 0.03
    for f in ("layers", "instance", "primitive", "queries", "flags"):
        bad = (aov[f] != a[f]) & stable
        assert not bad.any(), (name, f, np.argwhere(bad)[:5], aov[f][bad][:5], a[f][bad][:5])
    for f in ("distance", "shadow", "alpha"):
        err = np.abs(aov[f].astype(np.float64) - a[f])[stable].max()
        assert err <= 1e-6 * max(1.0, np.abs(a[f]).max()), (name, f, err)
    both = stable & stable_pixels(a, a32)
    rest = np.abs(a32["rgb"].astype(np.float64) - a["rgb"])[both].max()
    bar = rs.colour_bar(name)
    err = np.abs(rgba[..., :3].astype(np.float64) - a["rgb"])[stable]
    print("%s: float32 restatement worst %.4g (constant %.3g); GPU worst |rgb - ref| %.4g = %.2f of the bar %.3g" % (
        name, rest, rs.RESTATEMENT_WORST[name], err.max(), err.max() / bar, bar))
    assert rest <= rs.RESTATEMENT_WORST[name], (name, rest)
    assert err.max() <= bar, (name, err.max(), np.argwhere((np.abs(rgba[..., :3] - a["rgb"]).max(-1) > bar) & stable)[:5])


def _renders(ref, f):
    return ref.render(f, "A"), ref.render(f, "B"), ref.render(f, "A", shade=np.float32)


def _setup_statics(sge, gpu, rough=False, u=1.0, origin=(0, 0, 0)):
    meshes, mesh_of, mats, material_of = rs.static_scene(u, origin)
    rs.upload_scene(gpu, meshes, mesh_of, mats)
    m = rs.materials(sge, rough_only=rough)
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
        yield {"gpu": gpu, "scene": scene, "ref": RenderRef(scene, m, material_of, None, lights), "mats": mats, "material_of": material_of,
               "lights": lights, "eye": rs.camera()[0], "target": rs.camera()[1]}
    finally:
        gpu.close(); scene.close()


@pytest.mark.parametrize("variant", ["full", "rough"])
def test_statics_every_branch(sge, statics, variant):
    c = statics
    gpu = c["gpu"]
    m = rs.materials(sge, rough_only=variant == "rough")
    gpu.render_materials(m)
    try:
        ref = RenderRef(c["scene"], m, c["material_of"], None, c["lights"])
        f = rs.frame_record(sge, c["eye"], c["target"], 48, 32, 4)
        a, b, a32 = _renders(ref, f)
        assert set(np.unique(a["layers"])) == {0, 1, 2, 3} and (a["flags"] & 2).any() and ((a["shadow"] > 0) & (a["shadow"] < 1)).any()
        assert (a["flags"] & 1).any() == (variant == "full")
        rgba, aov = gpu.render_frame(f, aov=True)
        _check(variant, rgba, aov, a, b, a32, gpu, f, np.asarray(c["eye"], np.float32))
        assert np.array_equal(gpu.render_frame(f), rgba), "without the AOV records the image is the same"
    finally:
        gpu.render_materials(rs.materials(sge))


@pytest.mark.parametrize("shape", [(1, 1, 4), (65, 3, 4), (48, 32, 0)])
def test_edge_shapes(sge, statics, shape):
    c = statics
    w, h, nl = shape
    f = rs.frame_record(sge, c["eye"], c["target"], w, h, nl)
    a, b, a32 = _renders(c["ref"], f)
    rgba, aov = c["gpu"].render_frame(f, aov=True)
    _check("%dx%d, %d lights" % shape, rgba, aov, a, b, a32, c["gpu"], f, np.asarray(c["eye"], np.float32))
    if nl == 0:
        assert (aov["shadow"] == 1).all() and aov["queries"].max() <= 9


def test_an_empty_scene_is_the_background_and_the_dither(sge):
    gpu = sge.CharacterEngine(0)
    try:
        f = rs.frame_record(sge, (0, 1, 5), (0, 0, 0), 48, 32, 0)
        rgba, aov = gpu.render_frame(f, aov=True)
        gy, gx = np.divmod(np.arange(48 * 32), 48)
        dither = (hash12_rt(gx, gy).astype(np.float64) - 0.5) / 255.0
        want = (np.array(BG)[None, :] + dither[:, None]).reshape(32, 48, 3)
        # the float32 restatement of this frame: the background and the dither added in float32
        want32 = np.maximum(np.array(BG, np.float32)[None, :] + ((hash12_rt(gx, gy) - np.float32(0.5)) * (np.float32(1.0) / np.float32(255.0)))[:, None], 0)
        rest = np.abs(want32.astype(np.float64).reshape(32, 48, 3) - want).max()
        err = np.abs(rgba[..., :3] - want).max()
        print("empty scene: float32 restatement worst %.3g; GPU worst |rgb - (background + dither)| = %.3g (bar %.3g)" % (rest, err, 4 * rest))
        assert err <= 4 * rest and (rgba[..., 3] == 1).all()
        assert (aov["layers"] == 0).all() and (aov["instance"] == -1).all() and (aov["primitive"] == -1).all() and (aov["queries"] == 1).all()
        assert (aov["distance"] == 0).all() and (aov["alpha"] == 0).all() and (aov["shadow"] == 1).all() and (aov["flags"] == 0).all()
        assert len(np.unique(rgba[..., 0])) > 100, "the dither varies from pixel to pixel"
    finally:
        gpu.close()


def _crowd(sge, layout, n=3):
    gpu, cpu = sge.CharacterEngine(0), ob.oracle_engine()
    gpu.set_option(sge.abi.OPT_SKIN_LAYOUT, sge.abi.LAYOUT_PADDED16 if layout == "padded16" else sge.abi.LAYOUT_PACKED)
    for e in (gpu, cpu):
        build_scene(sge, e, n, terrain_cells=(24, 16), rings=9, segments=8, mixed=True, seed=5)
        e.blas_build(e.mesh["indices"])
    gpu.tick(stages=sge.abi.STAGE_ALL | sge.abi.STAGE_BLAS_REFIT)
    gp, gn, gt = gpu.skinned()
    ob.skinned_upload(cpu, gp, gn, gt)  # both sides look at the same skinned vertices
    return gpu, cpu, gp


def _crowd_view(gp):
    """The static scene's size and place and a camera for a crowd with skinned positions gp: the boxes stand in front of it."""
    lo, hi = gp.min(0).astype(np.float64), gp.max(0).astype(np.float64)
    u = float(max((hi - lo).max(), 1e-3)) / 2.5
    origin = np.array([(lo[0] + hi[0]) / 2, lo[1] - 0.02 * u, hi[2] + 1.2 * u])
    eye = origin + (0.4 * u, 3.4 * u, 5.6 * u)
    target = np.array([(lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, (lo[2] + hi[2]) / 2 + 0.8 * u])
    return u, origin, eye, target


@pytest.mark.parametrize("layout,with_statics", [("packed", True), ("padded16", True), ("packed", False)])
def test_crowd_after_a_tick(sge, layout, with_statics):
    gpu, cpu, gp = _crowd(sge, layout)
    scene = None
    try:
        u, origin, eye, target = _crowd_view(gp)
        if with_statics:
            meshes, mesh_of, mats, material_of, m, lights = _setup_statics(sge, gpu, u=u, origin=origin)
        else:
            meshes, mesh_of, mats, material_of = {}, [], np.zeros((0, 4, 4), np.float32), None
            m, lights = rs.materials(sge), rs.lights(sge, reach=8.0 * u)
            gpu.render_materials(m); gpu.render_lights(lights)
        crowd_materials = [6, 2, 3]  # a rough one, a mirror one, a glass one
        gpu.render_crowd_materials(crowd_materials)
        assert gpu.scene_info().crowdReady == 1
        scene = SceneRef(sge, meshes, mesh_of, mats, crowd=cpu)
        ref = RenderRef(scene, m, material_of, crowd_materials, lights)
        f = rs.frame_record(sge, eye, target, 48, 32, 4)
        a, b, a32 = _renders(ref, f)
        seen = set(np.unique(a["instance"]).tolist())
        assert {0, 1, 2} <= seen, seen
        rgba, aov = gpu.render_frame(f, aov=True)
        _check("crowd %s%s" % (layout, "" if with_statics else ", no statics"), rgba, aov, a, b, a32, gpu, f, np.asarray(eye, np.float32))
    finally:
        gpu.close(); cpu.close()
        if scene is not None:
            scene.close()


def test_a_context_with_mesh_variants_shows_the_statics_only(sge):
    gpu = sge.CharacterEngine(0)
    scene = None
    try:
        build_scene(sge, gpu, 2, terrain_cells=(24, 16), rings=9, segments=8, seed=5)
        gpu.blas_build(gpu.mesh["indices"])
        gpu.tick(stages=sge.abi.STAGE_ALL | sge.abi.STAGE_BLAS_REFIT)
        gp = gpu.skinned()[0]
        u, origin, eye, target = _crowd_view(gp)
        meshes, mesh_of, mats, material_of, m, lights = _setup_statics(sge, gpu, u=u, origin=origin)
        f = rs.frame_record(sge, eye, target, 48, 32, 4)
        with_crowd = gpu.render_frame(f, aov=True)[1]
        assert ((with_crowd["instance"] >= 0) & (with_crowd["instance"] < 2)).any(), "the crowd is in view until a variant is uploaded"
        gpu.upload_mesh_variant(1, gpu.mesh)
        assert gpu.scene_info().crowdReady == 0
        scene = SceneRef(sge, meshes, mesh_of, mats)
        a, b, a32 = _renders(RenderRef(scene, m, material_of, None, lights), f)
        rgba, aov = gpu.render_frame(f, aov=True)
        _check("variants", rgba, aov, a, b, a32, gpu, f, np.asarray(eye, np.float32))
        assert (aov["instance"][aov["instance"] >= 0] >= STATIC_BASE).all()
    finally:
        gpu.close()
        if scene is not None:
            scene.close()


@pytest.mark.parametrize("overlap", [0, 1, 2])
def test_device_form_behind_a_tick_and_an_instances_update(sge, overlap):
    """tick (skin + refit), sge_scene_instances_update, sge_render_frame_device on a caller's stream, nothing synchronised in
    between: bit for bit the batch form's frame of the same state, and the moved instance is where the update put it."""
    import torch
    gpu, cpu, gp = _crowd(sge, "packed")
    try:
        gpu.set_option(sge.abi.OPT_OVERLAP_SKIN, overlap)
        stream = torch.cuda.Stream()
        assert gpu.t.lib.sge_context_set_stream(gpu.h, C.c_void_p(stream.cuda_stream)) == 0
        u, origin, eye, target = _crowd_view(gp)
        meshes, mesh_of, mats, material_of, m, lights = _setup_statics(sge, gpu, u=u, origin=origin)
        gpu.render_crowd_materials([6, 2, 3])
        f = rs.frame_record(sge, eye, target, 48, 32, 4)
        before = gpu.render_frame(f, aov=True)[1]
        d_rgba = torch.zeros(32 * 48 * 4, dtype=torch.float32, device="cuda:0")
        d_aov = torch.zeros(32 * 48 * sge.abi.render_aov_dtype.itemsize, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        moved = mats.copy()
        moved[1][:3, 3] += (0.0, 0.9 * u, 0.0)  # the opaque box rises
        gpu.tick(stages=sge.abi.STAGE_ALL | sge.abi.STAGE_BLAS_REFIT)
        mm = columns(moved[1:2]).copy()
        gpu.scene_instances_update(mm, first=1)
        mm[:] = np.nan
        gpu.render_frame_device(f, d_rgba.data_ptr(), d_aov.data_ptr())
        gpu.synchronize()
        got_rgba = d_rgba.cpu().numpy().reshape(32, 48, 4)
        got_aov = d_aov.cpu().numpy().view(sge.abi.render_aov_dtype).reshape(32, 48)
        rgba, aov = gpu.render_frame(f, aov=True)
        assert got_rgba.tobytes() == rgba.tobytes() and got_aov.tobytes() == aov.tobytes()
        was, now = before["instance"] == STATIC_BASE + 1, aov["instance"] == STATIC_BASE + 1
        assert was.any() and now.any() and (was != now).any(), "the frame shows the box at its new place"
        assert np.argwhere(now)[:, 0].mean() < np.argwhere(was)[:, 0].mean() - 1, "higher in the image"
        assert gpu.t.lib.sge_context_set_stream(gpu.h, None) == 0
    finally:
        gpu.close(); cpu.close()


def test_contract(sge, statics):
    c = statics
    gpu = c["gpu"]
    f = rs.frame_record(sge, c["eye"], c["target"], 8, 4, 4)
    good = gpu.render_frame(f)

    def untouched(frame, match):
        rgba = np.full((4 * 8, 4), 7.0, np.float32)
        aov = np.full(4 * 8, 7, sge.abi.render_aov_dtype)
        with pytest.raises(sge.SgeError, match=match):
            gpu._call("render_frame_batch", sge.abi.ptr(frame), sge.abi.ptr(rgba), sge.abi.ptr(aov))
        assert (rgba == 7).all() and (aov["queries"] == 7).all()

    for field, value, match in (("invViewProj", np.nan, "non-finite"), ("cameraPosition", np.inf, "non-finite"), ("envSH", np.nan, "non-finite"),
                                ("ambientIntensity", np.nan, "non-finite"), ("width", 0, "size"), ("height", -1, "size"), ("dirLightCount", 5, "dirLightCount"),
                                ("dirLightCount", -1, "dirLightCount")):
        bad = f.copy()
        if field in ("invViewProj", "cameraPosition"):
            bad[field][0][1] = value
        elif field == "envSH":
            bad[field][0][8][2] = value
        else:
            bad[field] = value
        untouched(bad, match)
    big = f.copy(); big["width"], big["height"] = 1 << 14, (1 << 12) + 1
    untouched(big, "SGE_MAX_RENDER_PIXELS")
    with pytest.raises(sge.SgeError, match="non-finite"):
        gpu.render_frame_device(_poison(f), 1, 0)
    with pytest.raises(sge.SgeError, match="bad argument"):
        gpu._call("render_frame_device", sge.abi.ptr(f), None, None)
    # lights
    l = c["lights"].copy()
    l["color"][1][0] = np.nan
    with pytest.raises(sge.SgeError, match="non-finite"):
        gpu.render_lights(l)
    with pytest.raises(sge.SgeError, match="SGE_MAX_DIR_LIGHTS"):
        gpu.render_lights(np.zeros(9, sge.abi.render_light_dtype))
    # materials: counts, indices, shrinking below an index in use
    with pytest.raises(sge.SgeError, match="count differs"):
        gpu.render_static_materials(c["material_of"][:-1])
    with pytest.raises(sge.SgeError, match="count differs"):
        gpu.render_crowd_materials([0])
    with pytest.raises(sge.SgeError, match="outside the table"):
        gpu.render_static_materials([7] * len(c["material_of"]))
    with pytest.raises(sge.SgeError, match="still in use"):
        gpu.render_materials(rs.materials(sge)[:5])
    with pytest.raises(sge.SgeError, match="SGE_MAX_RENDER_MATERIALS"):
        gpu.render_materials(sge.abi.default_render_materials(257))
    nan = rs.materials(sge); nan["ior"][3] = np.nan
    with pytest.raises(sge.SgeError, match="non-finite"):
        gpu.render_materials(nan)
    assert np.array_equal(gpu.render_frame(f), good), "every failed call left the state as it was"
    # sge_scene_instances_set resets the instances to material 0: with another count the assignment is dropped
    try:
        gpu.scene_instances([0], columns(c["mats"][:1]))
        one = gpu.render_frame(f, aov=True)
        gpu.render_static_materials([0])
        assert np.array_equal(gpu.render_frame(f), one[0]) and (one[1]["instance"] == STATIC_BASE).any()
        gpu.render_materials(rs.materials(sge)[:1])  # nothing names a material above 0 any more
    finally:
        meshes, mesh_of, mats, material_of = rs.static_scene()
        gpu.render_materials(rs.materials(sge))
        gpu.scene_instances(mesh_of, columns(mats))
        gpu.render_static_materials(material_of)
    assert np.array_equal(gpu.render_frame(f), good)
    # 8 -> 1 -> 8 instances: the assignment made for the first list of 8 is dropped when the list of 1 is seen and does not come
    # back with another list of 8; every instance of the new list shades with material 0
    try:
        gpu.scene_instances([0], columns(c["mats"][:1]))
        gpu.render_frame(f)
        gpu.scene_instances(mesh_of, columns(mats))
        stale = gpu.render_frame(f)
        gpu.render_static_materials([0] * len(mesh_of))
        assert np.array_equal(gpu.render_frame(f), stale) and not np.array_equal(stale, good)
        gpu.render_materials(rs.materials(sge)[:1])  # the table may shrink: nothing names a material above 0
    finally:
        gpu.render_materials(rs.materials(sge))
        gpu.scene_instances(mesh_of, columns(mats))
        gpu.render_static_materials(material_of)
    assert np.array_equal(gpu.render_frame(f), good)
    bad = f.copy(); bad["flags"] = 1
    untouched(bad, "flags")


def _poison(f):
    bad = f.copy()
    bad["invViewProj"][0][3] = np.nan
    return bad


def test_the_example_writes_a_shaded_image_of_the_whole_scene(sge, tmp_path):
    """examples/demo_scene.py --render --image: the PPM shows the ground, the mirror (through the mirror path), both platforms
    and the shadowed player."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("demo_scene_image", os.path.join(root, "examples", "demo_scene.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    gpu = sge.CharacterEngine(0)
    try:
        demo.run(gpu, steps=60, scene=True)
        path = tmp_path / "out.ppm"
        aov = demo.shaded_image(gpu, str(path), width=160, height=100)
        data = path.read_bytes()
        assert data.startswith(b"P6\n160 100\n255\n") and len(data) == 15 + 160 * 100 * 3
        img = np.frombuffer(data[15:], np.uint8).reshape(100, 160, 3)
        ids = aov["instance"]
        base = sge.abi.SCENE_STATIC_BASE
        counts = {name: int((ids == i).sum()) for name, i in (("ground", base), ("mirror", base + 1), ("platform 0", base + 2), ("platform 1", base + 3), ("player", 0))}
        print(counts, "mirror path", int((aov["flags"] & 1).sum()), "shadowed", int((aov["shadow"] < 1).sum()))
        assert all(v > 0 for v in counts.values()), counts
        assert ((aov["flags"] & 1) != 0)[ids == base + 1].all(), "every mirror pixel takes the mirror path"
        assert ((aov["shadow"] < 1) & (ids == base)).any(), "a shadow falls on the ground"
        assert len(np.unique(img.reshape(-1, 3), axis=0)) > 50
    finally:
        gpu.close()
