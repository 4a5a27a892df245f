"""TEST INFRASTRUCTURE: the scenes, cameras, materials and lights of the shaded-frame tests (test_render_reference.py on the CPU,
test_gpu_render.py on the GPU), so that the CPU test checks the stable-pixel condition on the very inputs the GPU test renders."""
import numpy as np

from scene_ref import columns


def dress(pos, idx):
    """Streams for a position / index set: the renderer reads positions and indices only (no textures: the shading normal is the
    geometric one), so normals and tangents are constants."""
    V = len(pos)
    return {"positions": np.ascontiguousarray(pos, np.float32), "normals": np.tile(np.array([0, 1, 0], np.float32), (V, 1)),
            "tangents": np.tile(np.array([1, 0, 0, 1], np.float32), (V, 1)), "uvs": None, "indices": np.ascontiguousarray(idx, np.uint32).reshape(-1)}


def quad(half=1.0):
    """A horizontal square in the plane y = 0, facing +y."""
    p = np.array([[-half, 0, -half], [half, 0, -half], [half, 0, half], [-half, 0, half]], np.float32)
    return dress(p, [0, 2, 1, 0, 3, 2])


def box():
    """The unit cube centred at the origin: 8 vertices, 12 triangles."""
    p = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float32)
    f = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    idx = [i for a, b, c, d in f for i in (a, b, c, a, c, d)]
    return dress(p, idx)


def transform(scale=(1, 1, 1), yaw=0.0, at=(0, 0, 0)):
    m = np.eye(4, dtype=np.float64)
    c, s = np.cos(yaw), np.sin(yaw)
    m[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag(scale)
    m[:3, 3] = at
    return m.astype(np.float32)


def look_at(eye, target, up=(0, 1, 0)):
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    f = target - eye; f /= np.linalg.norm(f)
    s = np.cross(f, up); s /= np.linalg.norm(s)
    u = np.cross(s, f)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = s, u, -f
    m[:3, 3] = -m[:3, :3] @ eye
    return m


def perspective(fovy_deg, aspect, near=0.1, far=100.0):
    t = 1.0 / np.tan(np.radians(fovy_deg) / 2)
    m = np.zeros((4, 4))
    m[0, 0], m[1, 1] = t / aspect, t
    m[2, 2], m[2, 3] = far / (near - far), far * near / (near - far)
    m[3, 2] = -1
    return m


def frame_record(sge, eye, target, width, height, lights, up=(0, 1, 0), fovy=50.0, ambient=0.25, env_sh=None):
    inv = np.linalg.inv(perspective(fovy, width / height) @ look_at(eye, target, up))
    if env_sh is None:  # a sky / ground hemisphere, as RayTracingRenderer.makeHemisphereSH, plus second-order terms so all nine count
        env_sh = np.zeros((9, 3), np.float32)
        env_sh[0], env_sh[1] = (0.9, 0.95, 1.1), (0.35, 0.45, 0.65)
        env_sh[2:] = np.linspace(-0.08, 0.1, 21).reshape(7, 3)
    return sge.CharacterEngine.render_frame_record(inv, np.asarray(eye, np.float32), width, height, lights, ambient_intensity=ambient, env_sh=env_sh)


def materials(sge, rough_only=False):
    """0 default, 1 opaque rough, 2 mirror, 3 glass, 4 translucent sheet, 5 emissive ground, 6 character. rough_only: the variant
    whose materials all have roughness >= 0.3 (the mirror becomes a rough metal)."""
    m = sge.abi.default_render_materials(7)
    m["baseColor"][1], m["roughness"][1] = (0.8, 0.3, 0.2), 0.7
    m["baseColor"][2], m["metallic"][2], m["roughness"][2] = (0.9, 0.85, 0.7), 1.0, (0.3 if rough_only else 0.0)
    m["baseColor"][3], m["transmission"][3], m["alpha"][3], m["ior"][3], m["roughness"][3] = (0.7, 0.9, 0.8), 0.8, 0.4, 1.5, 0.4
    m["baseColor"][4], m["alpha"][4], m["roughness"][4] = (0.2, 0.4, 0.9), 0.5, 0.6
    m["baseColor"][5], m["emissive"][5], m["roughness"][5], m["occlusionStrength"][5] = (0.6, 0.6, 0.55), (0.01, 0.0, 0.02), 0.9, 0.8
    m["baseColor"][6], m["roughness"][6], m["metallic"][6] = (0.5, 0.7, 0.4), 0.45, 0.2
    return m


def lights(sge, reach=8.0):
    """light 0 shadowed; light 1 unshadowed with maxDistance = 0; light 2 disabled; light 3 with a maxDistance that some hits exceed."""
    l = np.zeros(4, sge.abi.render_light_dtype)
    l["direction"] = [(-0.35, -1.0, -0.25), (0.5, -0.6, 0.4), (0.0, -1.0, 0.0), (0.2, -0.7, -0.6)]
    l["intensity"] = [2.2, 0.6, 5.0, 0.9]
    l["color"] = [(1.0, 0.95, 0.85), (0.6, 0.7, 1.0), (1, 1, 1), (1.0, 0.5, 0.3)]
    l["enabled"] = [1, 1, 0, 1]
    l["maxDistance"] = [200.0, 0.0, 50.0, reach]
    return l


def static_scene(u=1.0, origin=(0, 0, 0)):
    """The ground, three boxes (opaque rough, mirror, glass) and four stacked translucent sheets, sized by u around `origin` (the
    ground's centre). -> meshes, mesh_of, matrices [S][4][4], material_of"""
    o = np.asarray(origin, np.float64)
    meshes = {0: quad(1.0), 1: box()}
    mesh_of, mats, material_of = [0], [transform((12 * u, 1, 12 * u), 0.0, o)], [5]
    for x, yaw, mat in ((-1.7, 0.35, 1), (0.0, -0.3, 2), (1.7, 0.5, 3)):
        mesh_of.append(1); mats.append(transform((u, u, u), yaw, o + (x * u, 0.5 * u + 0.01 * u, 0.0))); material_of.append(mat)
    for k in range(4):
        mesh_of.append(0); mats.append(transform((0.6 * u, 1, 0.6 * u), 0.2, o + (0.4 * u, (0.3 + 0.3 * k) * u, 1.9 * u))); material_of.append(4)
    return meshes, mesh_of, np.array(mats, np.float32), material_of


def camera(u=1.0, origin=(0, 0, 0)):
    o = np.asarray(origin, np.float64)
    return o + (0.3 * u, 3.1 * u, 5.2 * u), o + (0.0, 0.45 * u, 0.4 * u)


def upload_scene(gpu, meshes, mesh_of, mats):
    for m, mesh in meshes.items():
        gpu.scene_mesh_upload(m, mesh["positions"], mesh["normals"], mesh["tangents"], mesh["indices"], uvs=None)
    gpu.scene_instances(mesh_of, columns(mats))


# The worst |float32 restatement of the shading - float64| over stable pixels, per scene (render_ref: path A shaded in float32
# against path A shaded in float64), as measured and rounded up to three digits. The colour bar of a scene is 4 x its figure, the
# rule of the float64 pins (COVERAGE.md); the tests that render a scene assert that what they measure does not exceed its figure.
# The two static 48 x 32 scenes are measured by test_render_reference.py on the CPU; the others by test_gpu_render.py, where the
# reference runs on the CPU beside the GPU (the crowd scenes need the GPU's skinned vertices).
RESTATEMENT_WORST = {
    "full": 1.46e-7, "rough": 1.46e-7,                   # measured 1.448e-7 (3.7e-5 / 255)
    "1x1, 4 lights": 3.34e-8,                            # 3.33e-8
    "65x3, 4 lights": 1.10e-7,                           # 1.09e-7
    "48x32, 0 lights": 1.45e-8,                          # 1.44e-8
    "crowd packed": 1.31e-7,                             # 1.30e-7
    "crowd padded16": 1.68e-7,                           # 1.67e-7
    "crowd packed, no statics": 1.10e-7,                 # 1.09e-7
    "variants": 1.52e-7,                                 # 1.51e-7
}


def colour_bar(name):
    return 4 * RESTATEMENT_WORST[name]
