"""Diagnostic: ms per shaded frame (include/sge_amd_render.h) on one MI355X, image and AOV records resident on the device.

The scene of tools/scene_ray_bench.py: the settled 10,000-character crowd, the 17-Cheese render mesh as one static instance and
1,000 instances of a small box, with a mix of opaque, mirror and glass materials on the characters and the boxes, two lights (light
0 shadowed). One process; sge_render_frame_device at 1280 x 720 from a camera above the crowd's edge, timed with HIP events on the
context's stream after a warm-up frame; queries per second from the sum of the AOV records' `queries`. For context only, in the
same run and alternating with the frames: sge_scene_intersect_device on the frame's primary rays alone.
With --variants, behind those lines and in the same process: the same frame, statics, materials and lights for the crowd with three
mesh variants chosen by sge_lod_select from the camera (tools/variant_crowd.py) — first the control, whose variants all hold the full
mesh (the ragged frame kernel over the uniform crowd's geometry), then full / half / quarter vertex count.
With --textures, behind the first line and in the same process and context: the same frame with every material bound to a 256 x 256
sRGB base-colour texture and the characters' materials also to a 256 x 256 normal map (include/sge_amd_render_textures.h; uvs on the
statics are planar, the characters use the mesh's own), and the textured frame's median as a ratio to the untextured one.
With --ibl, behind those lines in the same process and context: the same frame(s) with the reference's default environment (the
128 cube with its 8 levels, the 128 x 128 BRDF table; include/sge_amd_render_ibl.h) — the untextured frame with the term, and with
--textures also the textured frame with the term — each as a ratio to its own line without the term.
usage: render_bench.py [--chars N] [--boxes K] [--width W] [--height H] [--frames F] [--variants] [--textures] [--ibl] [--out FILE]"""
import importlib, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sge = importlib.import_module("swift-game-engine_amd")
abi = sge.abi
import torch

arg = lambda k, d, cast=int: cast(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d
n, boxes, W, H, frames = arg("--chars", 10000), arg("--boxes", 1000), arg("--width", 1280), arg("--height", 720), arg("--frames", 5)
out_path = arg("--out", None, str)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def flat_normals(pos, idx):
    tri = np.asarray(idx, np.int64).reshape(-1, 3)
    fn = np.cross(pos[tri[:, 1]] - pos[tri[:, 0]], pos[tri[:, 2]] - pos[tri[:, 0]]).astype(np.float64)
    nrm = np.zeros(pos.shape, np.float64)
    for k in range(3):
        np.add.at(nrm, tri[:, k], fn)
    length = np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.where(length > 0, nrm / np.maximum(length, 1e-30), (0.0, 1.0, 0.0)).astype(np.float32)


def upload_mesh(eng, mesh, pos, idx, uvs=None):
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(idx, np.uint32).reshape(-1)
    return eng.scene_mesh_upload(mesh, pos, flat_normals(pos, idx), np.tile(np.array([1, 0, 0, 1], np.float32), (len(pos), 1)), idx, uvs=uvs)


eng = sge.CharacterEngine(0)
ybot = sge.assets.YBotAssets()
sge.crowd.upload_character_assets(eng, ybot)
terrain = sge.crowd.upload_terrain(eng)
sge.crowd.spawn_crowd(eng, ybot, n, terrain, mode="ccd")
eng.blas_build(eng.mesh["indices"])
for _ in range(130):
    eng.tick(stages=abi.STAGE_ALL | abi.STAGE_BLAS_REFIT)
b = eng.download(what=("bodies",))["bodies"]
P = b["position"].astype(np.float32)
mats = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
mats[:, 3, :3] = P                                            # column-major: translation in the last column
eng.blas_instances(mats.reshape(n, 16))

# statics as in scene_ray_bench.py
cheese = sge.crowd._load_static_parts("cheese")[0]
cpos = np.asarray(cheese["positions"], np.float32).reshape(-1, 3)
info = upload_mesh(eng, 0, cpos, cheese["indices"])
bp = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)
bi = np.array([0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3], np.uint32)
upload_mesh(eng, 1, bp, bi)
rng = np.random.default_rng(1)
lo, hi = P.min(0), P.max(0)
scale = np.float32((hi - lo)[[0, 2]].max() / 6 / max(np.ptp(cpos, axis=0).max(), 1e-6))
S = np.tile(np.eye(4, dtype=np.float32), (1 + boxes, 1, 1))
S[0, :3, :3] *= scale
S[0, 3, :3] = (lo + hi) / 2 - scale * (cpos.min(0) + cpos.max(0)) / 2 * (1, 0, 1) - (0, scale * cpos[:, 1].min(), 0)
S[1:, 3, :3] = np.stack([rng.uniform(lo[0], hi[0], boxes), rng.uniform(lo[1], hi[1], boxes) + 1.0, rng.uniform(lo[2], hi[2], boxes)], 1)
eng.scene_instances(np.array([0] + [1] * boxes, np.int32), S.reshape(-1, 16))

# materials: 0 opaque rough, 1 mirror, 2 glass; a third of the characters and of the boxes each
m = abi.default_render_materials(3)
m["baseColor"][0], m["roughness"][0] = (0.7, 0.6, 0.5), 0.7
m["baseColor"][1], m["metallic"][1], m["roughness"][1] = (0.9, 0.9, 0.95), 1.0, 0.0
m["baseColor"][2], m["transmission"][2], m["alpha"][2], m["ior"][2] = (0.7, 0.9, 0.8), 0.8, 0.4, 1.5
eng.render_materials(m)
eng.render_static_materials(np.concatenate([[0], np.arange(boxes) % 3]).astype(np.int32))
eng.render_crowd_materials((np.arange(n) % 3).astype(np.int32))
light = np.zeros(2, abi.render_light_dtype)
light["direction"], light["intensity"], light["color"], light["enabled"] = [(-0.2, -1.0, -0.4), (0.5, -0.6, 0.4)], [2.6, 0.5], [(1.0, 0.95, 0.85), (0.6, 0.7, 1.0)], 1.0
light["maxDistance"] = [0.0, 0.0]
eng.render_lights(light)

# the camera: above the middle of the crowd's front edge, looking at its centre
ext = float((hi - lo)[[0, 2]].max())
centre = ((lo + hi) / 2).astype(np.float64)
eye = centre + (0.0, 0.18 * ext, 0.62 * ext)
fwd = (centre - eye) / np.linalg.norm(centre - eye)
right = np.cross(fwd, (0, 1, 0)); right /= np.linalg.norm(right)
up = np.cross(right, fwd)
view = np.eye(4)
view[0, :3], view[1, :3], view[2, :3] = right, up, -fwd
view[:3, 3] = -view[:3, :3] @ eye
t, near, far = 1.0 / np.tan(np.radians(50.0) / 2), 0.1, 2000.0
proj = np.zeros((4, 4))
proj[0, 0], proj[1, 1], proj[2, 2], proj[2, 3], proj[3, 2] = t * H / W, t, far / (near - far), far * near / (near - far), -1
sh = np.zeros((9, 3), np.float32)
sh[0], sh[1] = np.array([0.5, 0.525, 0.6]) / 0.282095, np.array([0.2, 0.275, 0.4]) / 0.488603
inv = np.linalg.inv(proj @ view)
frame = eng.render_frame_record(inv, eye.astype(np.float32), W, H, 2, ambient_intensity=0.25, env_sh=sh)

# the frame's primary rays, for the context figure
gy, gx = np.divmod(np.arange(W * H), W)
ndc = np.stack([(gx + 0.5) / W * 2 - 1, (1 - (gy + 0.5) / H) * 2 - 1, np.ones(W * H), np.ones(W * H)], 1)
world = ndc @ inv.T
d = world[:, :3] / world[:, 3:4] - eye
d /= np.linalg.norm(d, axis=1, keepdims=True)
r = np.zeros(W * H, abi.blas_ray_dtype)
r["origin"], r["direction"], r["minDistance"], r["maxDistance"], r["instance"] = eye.astype(np.float32), d.astype(np.float32), 0.001, 1e6, -1
d_r = torch.from_numpy(r.view(np.uint8).copy()).to("cuda:0")
d_h = torch.zeros(W * H * abi.blas_hit_dtype.itemsize, dtype=torch.uint8, device="cuda:0")
d_rgba = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
d_aov = torch.zeros(W * H * abi.render_aov_dtype.itemsize, dtype=torch.uint8, device="cuda:0")
torch.cuda.synchronize()

def measure(eng, label, uniform=None):
    """frames alternating with the primary-ray launch; prints the lines -> median ms of the frame"""
    stream = torch.cuda.ExternalStream(eng.stream_handle(), device="cuda:0")
    forms = {"render_frame_device": lambda: eng.render_frame_device(frame, d_rgba.data_ptr(), d_aov.data_ptr()),
             "scene_intersect_device": lambda: eng.scene_intersect_device(d_r.data_ptr(), W * H, d_h.data_ptr())}
    for k in forms:
        forms[k]()
    eng.synchronize()
    ms = {k: [] for k in forms}
    for _ in range(frames):
        for k in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            forms[k]()
            e1.record(stream)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    eng.synchronize()
    aov = d_aov.cpu().numpy().view(abi.render_aov_dtype)
    hits = d_h.cpu().numpy().view(abi.blas_hit_dtype)
    rgba = d_rgba.cpu().numpy().reshape(H, W, 4)
    queries = int(aov["queries"].sum())

    say(label)
    v = np.array(ms["render_frame_device"])
    say("  sge_render_frame_device     %s ms  median %.3f  min %.3f  max %.3f" % (" ".join("%.3f" % x for x in v), np.median(v), v.min(), v.max()))
    say("    = %.2f Mpixels/s, %.1f M queries/s (%d queries per frame, %.2f per pixel, at most %d in one pixel)" % (
        W * H / np.median(v) / 1e3, queries / np.median(v) / 1e3, queries, queries / (W * H), aov["queries"].max()))
    say("    pixels: %.0f %% hit; layers 0/1/2/3: %s; %.1f %% through the mirror path, %.1f %% through the refraction path, %.1f %% with light 0 shadowed" % (
        100 * (aov["instance"] >= 0).mean(), " ".join("%.1f %%" % (100 * (aov["layers"] == k).mean()) for k in range(4)),
        100 * ((aov["flags"] & 1) != 0).mean(), 100 * ((aov["flags"] & 2) != 0).mean(), 100 * (aov["shadow"] < 1).mean()))
    p = np.array(ms["scene_intersect_device"])
    say("  context: sge_scene_intersect_device on the frame's primary rays alone  %s ms  median %.3f = %.1f M rays/s (%.0f %% hit)" % (
        " ".join("%.3f" % x for x in p), np.median(p), W * H / np.median(p) / 1e3, 100 * hits["hit"].mean()))
    say("  the frame's queries per second / the primary rays' rays per second = %.2f" % ((queries / np.median(v)) / (W * H / np.median(p))))
    assert np.isfinite(rgba).all() and (rgba[..., 3] == 1).all()
    if uniform is not None:
        say("  frame median / the uniform line's median = %.3f" % (np.median(v) / uniform))
    return float(np.median(v))


def planar_uvs(pos, tiles=1):
    """x / z over the mesh's extent in [0, 1], y mixed in so that walls vary too"""
    span = np.maximum(np.ptp(pos, axis=0), 1e-6)
    q = (pos - pos.min(0)) / span
    return np.ascontiguousarray(np.stack([q[:, 0] * 0.8 + q[:, 1] * 0.2, q[:, 2] * 0.8 + q[:, 1] * 0.2], -1), np.float32)


def dress(eng, uvs=False):
    """statics, materials and lights of the frame"""
    upload_mesh(eng, 0, cpos, cheese["indices"], planar_uvs(cpos, 1) if uvs else None)
    upload_mesh(eng, 1, bp, bi, planar_uvs(bp, 1) if uvs else None)
    eng.scene_instances(np.array([0] + [1] * boxes, np.int32), S.reshape(-1, 16))
    eng.render_materials(m)
    eng.render_static_materials(np.concatenate([[0], np.arange(boxes) % 3]).astype(np.int32))
    eng.render_crowd_materials((np.arange(n) % 3).astype(np.int32))
    eng.render_lights(light)


def with_ibl(eng, label, base_ms):
    """the frame as it is set up now, with the default environment; the environment is cleared again"""
    eng.render_env_upload(128, 8, sge.ibl_default_env(128))
    eng.render_brdf_lut_upload(sge.ibl_default_brdf_lut(128, 256))
    ms = measure(eng, label, base_ms)
    eng.render_ibl_clear()
    return ms


uniform_ms = measure(eng, "render_bench: %d x %d, %d characters + 17-Cheese (%d triangles) + %d boxes, opaque / mirror / glass materials, 2 lights" % (W, H, n, info.triangleCount, boxes))
if "--ibl" in sys.argv:
    with_ibl(eng, "(ibl) the same frame with specular IBL: the default 128 cube (8 levels) and 128 x 128 BRDF table", uniform_ms)
if "--textures" in sys.argv:
    # the same context: uvs on every mesh, materials 3..5 = 0..2 for the characters (so that only they carry the normal map)
    dress(eng, uvs=True)
    eng.blas_set_uvs(eng.mesh["uvs"])
    eng.render_materials(np.concatenate([m, m]))
    eng.render_crowd_materials((3 + np.arange(n) % 3).astype(np.int32))
    yy, xx = np.mgrid[0:256, 0:256]
    base = np.full((256, 256, 4), 255, np.uint8)
    cell = ((xx // 16 + yy // 16) % 2).astype(bool)
    base[..., :3] = np.clip(np.where(cell[..., None], (230, 220, 200), (110, 120, 140)) + ((xx * 7 + yy * 13) % 11)[..., None] - 5, 0, 255)
    nx, ny = 0.3 * np.cos(xx * np.pi / 16) * np.sin(yy * np.pi / 16), 0.3 * np.sin(xx * np.pi / 16) * np.cos(yy * np.pi / 16)
    nn = np.stack([nx, ny, np.ones_like(nx)], -1)
    nn /= np.linalg.norm(nn, axis=-1, keepdims=True)
    bumps = np.full((256, 256, 4), 255, np.uint8)
    bumps[..., :3] = np.rint((nn * 0.5 + 0.5) * 255)
    eng.render_texture_upload(0, base, srgb=True)
    eng.render_texture_upload(1, bumps, srgb=False)
    bind = abi.default_render_material_textures(6)
    bind["baseColor"] = 0
    bind["normal"][3:] = 1
    eng.render_material_textures(bind)
    textured_ms = measure(eng, "(textures) the same frame, every material with a 256 x 256 sRGB base colour, the characters' also with a 256 x 256 normal map", uniform_ms)
    if "--ibl" in sys.argv:
        with_ibl(eng, "(ibl, textures) the textured frame with specular IBL (the ratio is to the textured line)", textured_ms)
eng.close()
if "--variants" in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from variant_crowd import settled_crowd
    for mode, what in (("control", "three variants that all hold the full mesh"), ("lod", "full / half / quarter vertex count")):
        eng, P2, per, verts = settled_crowd(sge, n, mode, lambda a, b: eye)
        dress(eng)
        measure(eng, "(%s) mesh variants, %s: vertices per variant %s, characters per variant %s (sge_lod_select from the camera)" % (mode, what, verts, per), uniform_ms)
        eng.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
