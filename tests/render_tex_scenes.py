"""TEST INFRASTRUCTURE: the textured scene of the shaded-frame tests (test_render_tex_reference.py on the CPU,
test_gpu_render_textures.py on the GPU): render_scenes.static_scene with uvs and a shading frame on its meshes, seven small
textures and the bindings that put every sampling site of the text to work."""
import numpy as np

import render_scenes as rs
import render_tex_ref as tr


def quad_uv(half=1.0):
    m = rs.quad(half)
    p = m["positions"]
    m["uvs"] = np.ascontiguousarray(np.stack([(p[:, 0] + half) / (2 * half), (p[:, 2] + half) / (2 * half)], -1), np.float32)
    return m


def box_uv():
    """render_scenes.box with uvs that vary over every face, normals that point away from the centre and tangents around the y
    axis: a shading frame that is nowhere degenerate."""
    m = rs.box()
    p = m["positions"].astype(np.float64)
    n = p / np.linalg.norm(p, axis=1, keepdims=True)
    t = np.stack([n[:, 2], np.zeros(len(n)), -n[:, 0]], -1)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    m["normals"] = np.ascontiguousarray(n, np.float32)
    m["tangents"] = np.ascontiguousarray(np.concatenate([t, np.ones((len(t), 1))], 1), np.float32)
    m["uvs"] = np.ascontiguousarray(np.stack([(p[:, 0] + 0.5) * 0.6 + (p[:, 1] + 0.5) * 0.3, (p[:, 2] + 0.5) * 0.6 + (p[:, 1] + 0.5) * 0.3], -1), np.float32)
    return m


def static_scene(u=1.0, origin=(0, 0, 0)):
    _, mesh_of, mats, material_of = rs.static_scene(u, origin)
    return {0: quad_uv(1.0), 1: box_uv()}, mesh_of, mats, material_of


def upload_scene(gpu, meshes, mesh_of, mats):
    for m, mesh in meshes.items():
        gpu.scene_mesh_upload(m, mesh["positions"], mesh["normals"], mesh["tangents"], mesh["indices"], uvs=mesh["uvs"])
    gpu.scene_instances(mesh_of, rs.columns(mats))


def textures():
    """{slot: (uint8 [H][W][4], srgb)}: 0 a checker with varying alpha (the translucent sheets: sample_alpha in the shadow walk);
    1 metallic-roughness, half of it below the mirror test's metallic; 2 emissive; 3 occlusion, 2 x 2; 4 a normal map; 5 one texel;
    6 an opaque checker (the ground)."""
    yy, xx = np.mgrid[0:8, 0:8]
    check = ((xx + yy) % 2).astype(bool)
    t0 = np.zeros((8, 8, 4), np.uint8)
    t0[..., :3] = np.where(check[..., None], (230, 200, 90), (60, 90, 200))
    t0[..., 3] = 80 + 25 * ((xx * 3 + yy * 5) % 8)
    t1 = np.zeros((4, 4, 4), np.uint8)
    t1[..., 1], t1[..., 2], t1[..., 3] = 255, 255, 255
    t1[:, 2:, 2] = 120
    t1[2:, :, 1] = 200
    t2 = np.zeros((8, 8, 4), np.uint8)
    t2[..., 0], t2[..., 1], t2[..., 2], t2[..., 3] = 30 * xx, 255, 250 - 30 * yy, 255
    t3 = np.array([[[255, 0, 0, 255], [150, 0, 0, 255]], [[200, 0, 0, 255], [90, 0, 0, 255]]], np.uint8)
    ang = (xx + 0.5) / 8 * 2 * np.pi, (yy + 0.5) / 8 * 2 * np.pi
    n = np.stack([0.12 * np.sin(ang[0]), 0.12 * np.cos(ang[1]), np.ones((8, 8))], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    t4 = np.full((8, 8, 4), 255, np.uint8)
    t4[..., :3] = np.round((n * 0.5 + 0.5) * 255)
    t5 = np.array([[[200, 170, 140, 255]]], np.uint8)
    t6 = np.full((8, 8, 4), 255, np.uint8)
    t6[..., :3] = np.where(check[..., None], (210, 210, 200), (120, 130, 120))
    return {0: (t0, True), 1: (t1, False), 2: (t2, False), 3: (t3, False), 4: (t4, False), 5: (t5, True), 6: (t6, True)}


def bindings(sge, normal_scale=1.0):
    """For render_scenes.materials: 1 (the rough box) the one-texel base colour and the normal map; 2 (the mirror box)
    metallic-roughness; 3 (glass) a base colour in an empty slot, which is no texture; 4 (the sheets) the alpha checker; 5 (the
    ground) base colour, emissive, occlusion; 6 (the characters) base colour and normal map."""
    b = sge.abi.default_render_material_textures(7)
    b["baseColor"][1], b["normal"][1], b["normalScale"][1] = 5, 4, normal_scale
    b["metallicRoughness"][2] = 1
    b["baseColor"][3] = 20
    b["baseColor"][4] = 0
    b["baseColor"][5], b["emissive"][5], b["occlusion"][5] = 6, 2, 3
    b["baseColor"][6], b["normal"][6], b["normalScale"][6] = 6, 4, normal_scale
    return b


def upload_textures(gpu, tex):
    for slot, (rgba, srgb) in tex.items():
        gpu.render_texture_upload(slot, rgba, srgb=srgb)


# The normal map's gain on a sampled value: nTex = 2 c - 1, times ns * graze <= 4 + (6 - 4) * 0.25 = 4.5 at normalScale 6.
NORMAL_GAIN = 2 * 4.5
NORMAL_SLOTS = {4: NORMAL_GAIN}


def margin_term(tex):
    """A pixel with a threshold-feeding value closer to its threshold than this counts as unstable: what the uv bar may move a
    sampled value by (render_tex_ref.value_term), the normal map's samples weighed by their gain on N."""
    return tr.value_term(tex, gains=NORMAL_SLOTS)


def colour_gain(lights, frame):
    """The factor a sampled value is multiplied by on its way into rgb, bounded from the frame's own inputs: the radiance of every
    enabled light (eval_brdf's diffuse term is base / pi, its specular term is weighed by F <= 1; NdotL, shadow <= 1), the SH
    ambient at its largest (the nine coefficients' magnitudes summed, times ambientIntensity) and 1 for the emissive term. The
    mixes and the compositing are convex, so bounces and layers add nothing."""
    f = np.asarray(frame).reshape(-1)[0]
    light = sum(float(l["intensity"]) * float(np.max(l["color"])) for l in lights[:int(f["dirLightCount"])] if l["enabled"] >= 0.5)
    ambient = float(f["ambientIntensity"]) * float(np.abs(f["envSH"]).sum(0).max())
    return light + ambient + 1.0


# The worst |float32 restatement of the shading - float64| over stable pixels, per scene, measured on the CPU by
# test_render_tex_reference.py (the static scenes) or beside the GPU by test_gpu_render_textures.py (the crowds need the GPU's skinned
# vertices) between the float32 and the float64 shading of the reference, never from the GPU's image; rounded up to three digits.
RESTATEMENT_WORST = {
    "textured, normalScale 1": 9.79e-8,                   # measured 9.784e-8
    "textured, normalScale 6": 9.74e-8,                   # 9.731e-8
    "textured crowd packed": 2.04e-7,                     # 2.031e-7
    "textured crowd padded16": 1.33e-7,                   # 1.327e-7
    "textured variants packed": 2.35e-7,                  # 2.345e-7; 40 of 1,536 pixels unstable in the reference alone
    "textured variants padded16": 2.35e-7,                # 2.345e-7
}


def colour_bar(name, tex, lights, frame):
    """4 x the scene's float32 restatement figure, plus what the uv bar may move a sample by on its way into rgb."""
    return 4 * RESTATEMENT_WORST[name] + margin_term(tex) * colour_gain(lights, frame)
