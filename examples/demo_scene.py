#!/usr/bin/env python3
"""The physical content of the reference's DemoScene (Game/DemoScene.swift) on the MI355X path, system by system:

  ground plane 80 x 80 at y = -3                                  DemoScene.swift:103-130
  ornate mirror: its two collision hulls, x8, offset (-10, 1, 4)  :296-376 (17-Cheese / Semla hulls need Blender)
  two kinematic platforms (box 4.0 scaled (1.5, 0.2, 1.5))        :379-452: elevator at (16, -1, 0), mover at (-16, -2, 12)
  the player: a Y-Bot with the CharacterFactory defaults          CharacterFactory.swift:60-110, dropped at (0, 7.5, 0)

and the fixed-step order of DemoScene.swift:56-75:
  KinematicPlatformMotionSystem -> CollisionQueryRefreshSystem -> PhysicsIntentSystem -> GravitySystem ->
  KinematicMoveStopSystem -> LocomotionProfileSystem -> ActionAnimationSystem -> PoseStackSystem -> PhysicsWritebackSystem
  (+ the skinning encode of RayTracingScene.buildGeometryBuffers).

and what the renderer does next with the skinned vertices (RayTracingScene.buildGeometryBuffers ->
RTAccelerationBuilder.build, RTAccelerationBuilder.swift:75-185; raytraceKernel primary rays, RayTracing.metalinc:225-300):
the player's acceleration structure is refitted behind the skinning of every step, its instance matrix is the entity's
TransformComponent. With `--render` the static items go the same way (include/sge_amd_ray_scene.h): the ground, the mirror's
render mesh and the platform box are uploaded once as scene meshes (cachedStaticBLAS, RTAccelerationBuilder.swift:37-71), instanced
with their model matrices (:168-185), the platforms' matrices are updated every step, and after the last step a small image of
primary rays is shot at the whole scene, one shadow ray per hit towards a fixed sun (RayTracing.metalinc:319-338), and the depth
is printed as ASCII with the shadowed pixels marked.

Usage:  python examples/demo_scene.py [--steps 600] [--oracle] [--render]   (--oracle runs the CPU checker instead of the GPU;
the checker has no ray scene: `--oracle --render` shoots at the characters only)
The player walks to the ground mover, rides it, then heads for the elevator.
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sge = importlib.import_module("swift-game-engine_amd")
A, F = sge.abi, sge.formats


def box_mesh(size=4.0):
    """ProceduralMeshes.box (ProceduralMeshes.swift:183-230): 24 vertices, 12 triangles."""
    s = size * 0.5
    faces = [((0, 0, 1), [(-s, -s, s), (s, -s, s), (s, s, s), (-s, s, s)]), ((0, 0, -1), [(s, -s, -s), (-s, -s, -s), (-s, s, -s), (s, s, -s)]),
             ((1, 0, 0), [(s, -s, s), (s, -s, -s), (s, s, -s), (s, s, s)]), ((-1, 0, 0), [(-s, -s, -s), (-s, -s, s), (-s, s, s), (-s, s, -s)]),
             ((0, 1, 0), [(-s, s, s), (s, s, s), (s, s, -s), (-s, s, -s)]), ((0, -1, 0), [(-s, -s, -s), (s, -s, -s), (s, -s, s), (-s, -s, s)])]
    pos, idx = [], []
    for _, quad in faces:
        b = len(pos)
        pos += quad
        idx += [b, b + 1, b + 2, b, b + 2, b + 3]
    return np.asarray(pos, np.float32), np.asarray(idx, np.uint32)


class Platform:
    """KinematicPlatformComponent + KinematicPlatformMotionSystem (Components.swift:484-505, Systems.swift:122-155)."""

    def __init__(self, entity, origin, axis, amplitude, speed, phase):
        self.e, self.origin, self.amplitude, self.speed, self.phase, self.time = entity, np.asarray(origin, np.float32), amplitude, speed, phase, np.float32(0)
        ax = np.asarray(axis, np.float32)
        n = np.float32(np.sqrt((ax * ax).sum()))
        self.axis = ax / n if n > 1e-4 else np.array([0, 1, 0], np.float32)

    def step(self, dt):
        self.time = np.float32(self.time + np.float32(dt))
        offset = np.float32(np.sin(np.float32(self.time * np.float32(self.speed) + np.float32(self.phase)))) * np.float32(self.amplitude)
        new = self.origin + self.axis * offset
        self.e["prevPosition"] = self.e["position"]     # PhysicsBeginStepSystem (Systems.swift:183-202)
        self.e["translation"] = tuple(new)
        self.e["position"] = tuple(float(v) for v in new)


def build(engine):
    ybot = sge.assets.YBotAssets()
    sge.crowd.upload_ybot_mesh(engine, ybot)
    gp, gi, _ = sge.assets.ground_plane()
    ident = (0, 0, 0, 1)
    world = [{"id": 1, "translation": (0, -3, 0), "rotation": ident, "scale": (1, 1, 1), "positions": gp, "indices": gi,
              "bodyType": A.BODY_STATIC, "material": (0.9, 0.8, 0)}]
    z = np.load(os.path.join(sge.assets.GOLDEN_DIR, "ornate_mirror_static.npz"))
    t = F.transform_from_matrix(F.matrix_from_array_row_major(z["transformRowMajor"]))
    upright = F.quat_angle_axis(np.float32(float.fromhex("0x1.921fb4p+1")) * np.float32(0.5), (1, 0, 0))
    flip = F.quat_angle_axis(np.float32(float.fromhex("0x1.921fb4p+1")), (1, 0, 0))
    t["rotation"] = F.quat_mul(t["rotation"], F.quat_mul(upright, flip))       # DemoScene.swift:331-335
    t["scale"] = t["scale"] * np.float32(8.0)
    t["translation"] = t["translation"] + np.array([-10, 1, 4], np.float32)
    for k in range(2):
        world.append({"id": 10 + k, "translation": tuple(t["translation"]), "rotation": tuple(t["rotation"]), "scale": tuple(t["scale"]),
                      "positions": z[f"hull{k}.positions"], "indices": z[f"hull{k}.indices"], "bodyType": A.BODY_STATIC,
                      "material": (0.6, 0.5, 0), "layer": 1 << 4})
    bp, bi = box_mesh(4.0)
    platforms = []
    for eid, origin, axis, amp, speed, phase in ((20, (16, -1.0, 0), (0, 1, 0), 2.0, 1.1, 0.0), (21, (-16, -2.0, 12), (1, 0, 0), 4.0, 0.9, 0.7)):
        e = {"id": eid, "translation": origin, "rotation": ident, "scale": (1.5, 0.2, 1.5), "positions": bp, "indices": bi,
             "bodyType": A.BODY_KINEMATIC, "platform": True, "position": origin, "prevPosition": origin, "material": (0.9, 0.7, 0)}
        world.append(e)
        platforms.append(Platform(e, origin, axis, amp, speed, phase))
    service = sge.services.CollisionQueryService(engine)
    service.rebuild(world)
    engine.resize(1)
    state = {"bodies": sge.assets.default_bodies(1, np.array([[0.0, 7.5, 0.0]])), "params": sge.assets.default_controller_params(1),
             "controllers": sge.assets.default_controller_state(1), "intents": sge.assets.default_intents(1),
             "locomotion": sge.assets.default_locomotion(1, ybot), "actions": sge.assets.default_actions(1, ybot, present=True)}
    engine.upload(**state)
    engine.blas_build(engine.mesh["indices"])           # encoder.build of the skinned item (RTAccelerationBuilder.swift:75-112)
    return ybot, world, platforms, service


def vertex_normals(pos, idx):
    """Area-weighted vertex normals of a static mesh (the demo's items carry none in the collision world)."""
    tri = np.asarray(idx, np.int64).reshape(-1, 3)
    p = np.asarray(pos, np.float64)
    fn = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
    n = np.zeros_like(p)
    for k in range(3):
        np.add.at(n, tri[:, k], fn)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(length > 0, n / np.maximum(length, 1e-30), (0.0, 1.0, 0.0)).astype(np.float32)


def entity_matrix(e):
    return F.model_matrix({"translation": np.asarray(e["translation"], np.float32), "rotation": np.asarray(e["rotation"], np.float32),
                           "scale": np.asarray(e["scale"], np.float32)})


def procedural_textures():
    """Three small procedural textures in numpy (the idea of the reference's ProceduralTextures: a checkerboard for the ground, a
    tinted weave and a bump pattern for the player) -> {slot: (rgba uint8 [H][W][4], srgb)}."""
    yy, xx = np.mgrid[0:64, 0:64]
    cell = ((xx // 8 + yy // 8) % 2).astype(bool)
    grain = ((xx * 7 + yy * 13) % 5).astype(np.int32) - 2
    ground = np.full((64, 64, 4), 255, np.uint8)
    ground[..., :3] = np.clip(np.where(cell[..., None], (225, 225, 215), (95, 105, 100)) + 3 * grain[..., None], 0, 255)
    yy, xx = np.mgrid[0:32, 0:32]
    weave = 0.5 + 0.5 * np.sin(xx * np.pi / 4) * np.sin(yy * np.pi / 4)
    cloth = np.full((32, 32, 4), 255, np.uint8)
    cloth[..., :3] = np.rint(255 * (0.55 + 0.45 * weave[..., None] * np.array([1.0, 0.9, 0.8])))
    nx, ny = 0.35 * np.cos(xx * np.pi / 4) * np.sin(yy * np.pi / 4), 0.35 * np.sin(xx * np.pi / 4) * np.cos(yy * np.pi / 4)
    n = np.stack([nx, ny, np.ones_like(nx)], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    bumps = np.full((32, 32, 4), 255, np.uint8)
    bumps[..., :3] = np.rint((n * 0.5 + 0.5) * 255)
    return {0: (ground, True), 1: (cloth, True), 2: (bumps, False)}


def scene_upload(engine, world, textures=False):
    """The static items of RayTracingScene.buildGeometryBuffers as scene meshes and instances: mesh 0 the ground plane, mesh 1 the
    mirror's render mesh (placed like its hulls), mesh 2 the platform box, instanced twice. -> index of the first platform instance"""
    z = np.load(os.path.join(sge.assets.GOLDEN_DIR, "ornate_mirror_static.npz"))
    ground, hull, plats = world[0], world[1], [e for e in world if e.get("platform")]
    for mesh, (pos, idx) in enumerate(((ground["positions"], ground["indices"]), (z["positions"], z["indices"]), (plats[0]["positions"], plats[0]["indices"]))):
        pos = np.asarray(pos, np.float32).reshape(-1, 3)
        uvs = np.ascontiguousarray(pos[:, [0, 2]] / 4.0) if textures and mesh == 0 else None   # the ground: one checker tile per 4 units
        engine.scene_mesh_upload(mesh, pos, vertex_normals(pos, idx), np.tile(np.array([1, 0, 0, 1], np.float32), (len(pos), 1)), idx, uvs=uvs)
    items = [(0, ground), (1, hull)] + [(2, e) for e in plats]
    scene_upload.items = [(z["positions"] if m == 1 else e["positions"], e) for m, e in items]   # what shaded_image frames
    engine.scene_instances([m for m, _ in items], np.stack([entity_matrix(e) for _, e in items]))
    return 2


SUN = np.array([0.35, 0.8, 0.45], np.float32) / np.linalg.norm(np.array([0.35, 0.8, 0.45], np.float32))   # L = normalize(-light.direction)


def render_probe(engine, width=56, height=28, fov_y=0.6, scene=False):
    """Primary rays of the raytraceKernel (RayTracing.metalinc:225-235: origin = camera, direction through the pixel centre,
    min_distance 0.001, max_distance 1e6) against the skinned items (here: the player) -> (hit mask, distances, hit records);
    scene=True: against the whole ray scene, + the mask of hits whose shadow ray towards SUN is occluded or that face away from it."""
    b = engine.download(what=("bodies",))["bodies"]
    pos = b["position"][0].astype(np.float32)
    m = F.model_matrix({"translation": pos, "rotation": b["transformRotation"][0], "scale": np.ones(3, np.float32)})
    engine.blas_instances(np.asarray(m, np.float32).reshape(1, 16))   # instance descriptor = item.modelMatrix (:168-185)
    eye = pos + np.array([0.0, 0.3, 9.0], np.float32)
    target = pos + np.array([0.0, -0.2, 0.0], np.float32)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, (0, 1, 0)); right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    ys, xs = np.meshgrid((np.arange(height) + 0.5) / height, (np.arange(width) + 0.5) / width, indexing="ij")
    th = np.tan(fov_y / 2)
    d = fwd + ((xs * 2 - 1) * th * width / height * 0.5)[..., None] * right + ((1 - ys * 2) * th)[..., None] * up
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3).astype(np.float32)
    if scene:
        h = engine.scene_intersect(np.tile(eye, (len(d), 1)), d, -1)
        hit = h["hit"] == 1
        # RayTracing.metalinc:318-338: hitPos, bias = shadow_bias(distance) (:61), origin = hitPos + N * bias, min_distance = bias / 2
        bias = np.maximum(np.float32(0.002), h["distance"] * np.float32(0.002)).astype(np.float32)
        pos_hit = eye + d * h["distance"][:, None]
        lit = hit & ((h["geomNormal"] * SUN).sum(1) > 0)      # NdotL <= 0: no light from the sun, no ray
        occ = engine.scene_occluded(pos_hit + h["geomNormal"] * bias[:, None], np.tile(SUN, (len(d), 1)), -1, min_distance=bias * np.float32(0.5), max_distance=1e6)
        shadow = hit & (~lit | (occ == 1))
        return hit.reshape(height, width), h["distance"].reshape(height, width), h, shadow.reshape(height, width)
    h = engine.blas_intersect(np.tile(eye, (len(d), 1)), d, np.full(len(d), -1, np.int32))   # instance < 0: against every skinned item
    return h["hit"].reshape(height, width) == 1, h["distance"].reshape(height, width), h


def shaded_image(engine, path, width=320, height=200, fov_y=0.9, textures=False, ibl=False):
    """The shaded frame (include/sge_amd_render.h: raytraceKernel's layers, lights and bounces in one launch) as a binary PPM, from a
    camera of its own that is pulled back until the mirror (a smooth metal: the mirror path), both platforms and the player are in
    view above the ground. -> the AOV records"""
    b = engine.download(what=("bodies",))["bodies"]
    pos = b["position"][0].astype(np.float64)
    m = F.model_matrix({"translation": pos.astype(np.float32), "rotation": b["transformRotation"][0], "scale": np.ones(3, np.float32)})
    engine.blas_instances(np.asarray(m, np.float32).reshape(1, 16))
    # the world-space centres of the mirror and the platforms (instances 1 ..; a matrix is stored by column), and the player
    points = [pos + (0.0, 1.0, 0.0)]
    for p, e in scene_upload.items[1:]:
        M = np.asarray(entity_matrix(e), np.float64).reshape(4, 4)
        w = np.asarray(p, np.float64).reshape(-1, 3) @ M[:3, :3] + M[3, :3]
        points.append((w.min(0) + w.max(0)) / 2)
    points = np.array(points)
    target = (points.min(0) + points.max(0)) / 2
    radius = np.linalg.norm(points - target, axis=1).max() + 4.0
    eye = target + np.array([0.0, 0.45, 1.0]) * (radius / np.tan(fov_y / 2) / np.linalg.norm([0.45, 1.0]))
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, (0, 1, 0)); right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    view = np.eye(4)
    view[0, :3], view[1, :3], view[2, :3] = right, up, -fwd
    view[:3, 3] = -view[:3, :3] @ eye
    t, near, far = 1.0 / np.tan(fov_y / 2), 0.1, 500.0
    proj = np.zeros((4, 4))
    proj[0, 0], proj[1, 1], proj[2, 2], proj[2, 3], proj[3, 2] = t * height / width, t, far / (near - far), far * near / (near - far), -1
    mats = A.default_render_materials(4)   # 0 ground, 1 mirror, 2 platforms, 3 player
    mats["baseColor"][0], mats["roughness"][0] = (0.55, 0.6, 0.5), 0.9
    mats["baseColor"][1], mats["metallic"][1], mats["roughness"][1] = (0.9, 0.9, 0.95), 1.0, 0.0
    mats["baseColor"][2], mats["roughness"][2] = (0.8, 0.45, 0.2), 0.6
    mats["baseColor"][3], mats["roughness"][3] = (0.3, 0.5, 0.9), 0.5
    if ibl:   # include/sge_amd_render_ibl.h: IBLResources' default cube and table; the platforms become a rough metal that shows them
        mats["metallic"][2], mats["roughness"][2] = 1.0, 0.4
        engine.render_env_upload(128, 8, sge.ibl_default_env(128))
        engine.render_brdf_lut_upload(sge.ibl_default_brdf_lut(128, 256))
    engine.render_materials(mats)
    engine.render_static_materials([0, 1] + [2] * (engine.scene_info().staticInstances - 2))
    engine.render_crowd_materials([3])
    if textures:   # include/sge_amd_render_textures.h: the ground's checkerboard; the player's base colour and normal map
        for slot, (rgba, srgb) in procedural_textures().items():
            engine.render_texture_upload(slot, rgba, srgb=srgb)
        bind = A.default_render_material_textures(4)
        bind["baseColor"][0] = 0
        bind["baseColor"][3], bind["normal"][3] = 1, 2
        engine.render_material_textures(bind)
    light = np.zeros(1, A.render_light_dtype)   # RayTracingRenderer.swift:163-168's default light, from SUN's side
    light["direction"], light["intensity"], light["color"], light["enabled"], light["maxDistance"] = -SUN, 2.6, (1.0, 0.95, 0.85), 1.0, 200.0
    engine.render_lights(light)
    sh = np.zeros((9, 3), np.float32)           # makeHemisphereSH's two terms (RayTracingRenderer.swift:190-198)
    sh[0], sh[1] = np.array([0.5, 0.525, 0.6]) / 0.282095, np.array([0.2, 0.275, 0.4]) / 0.488603
    frame = engine.render_frame_record(np.linalg.inv(proj @ view), eye.astype(np.float32), width, height, 1, ambient_intensity=0.25, env_sh=sh)
    rgba, aov = engine.render_frame(frame, aov=True)
    img = np.rint(np.clip(rgba[..., :3], 0.0, 1.0) * 255.0).astype(np.uint8)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (width, height))
        f.write(img.tobytes())
    return aov


def ascii_depth(mask, dist, shadow=None):
    """Depth as a ramp of characters; with `shadow`, shadowed pixels are drawn as 's'."""
    ramp = "@%#*+=-:."
    lo, hi = (dist[mask].min(), dist[mask].max()) if mask.any() else (0.0, 1.0)
    rows = []
    for r in range(mask.shape[0]):
        rows.append("".join(("s" if shadow is not None and shadow[r, c] else ramp[min(len(ramp) - 1, int((dist[r, c] - lo) / max(hi - lo, 1e-6) * len(ramp)))])
                            if mask[r, c] else " " for c in range(mask.shape[1])))
    return "\n".join(rows)


def run(engine, steps=600, dt=1.0 / 60.0, log=None, scene=False, textures=False):
    ybot, world, platforms, service = build(engine)
    first_platform = scene_upload(engine, world, textures) if scene else 0
    if scene and textures:   # the player's uvs: the mesh's own, or a planar wrap of its bind pose
        p = np.asarray(engine.mesh["positions"], np.float32).reshape(-1, 3)
        span = np.maximum(p.max(0) - p.min(0), 1e-6)
        uvs = engine.mesh.get("uvs")
        engine.blas_set_uvs(uvs if uvs is not None else np.stack([(p[:, 0] - p[:, 0].min()) / span[0] * 4, (p[:, 1] - p[:, 1].min()) / span[1] * 8], -1))
    trace = []
    for s in range(steps):
        for p in platforms:
            p.step(dt)                                  # KinematicPlatformMotionSystem
        if scene:                                       # the instance descriptors of the moving items (RTAccelerationBuilder.swift:177)
            engine.scene_instances_update(np.stack([entity_matrix(p.e) for p in platforms]), first=first_platform)
        service.update(world)                           # CollisionQueryRefreshSystem -> updateDynamicTransforms + refit
        service.upload_platforms(world)                 # the platform list KinematicMoveStopSystem reads
        pos = engine.download(what=("bodies",))["bodies"]["position"][0]
        mover = np.asarray(world[-1]["translation"], np.float64)
        target = mover + (0, 0, 0) if s < 420 else np.array([16.0, 0, 0])   # walk to the mover, later to the elevator
        d = np.array([target[0] - pos[0], 0.0, target[2] - pos[2]])
        dist = np.linalg.norm(d)
        v = d / dist * min(4.5, dist * 4) if dist > 0.05 else np.zeros(3)
        engine.upload(intents=sge.assets.default_intents(1, v.astype(np.float32)[None]))
        engine.tick(dt=dt, stages=A.STAGE_ALL | A.STAGE_BLAS_REFIT)   # ... skinning encode, then the acceleration-structure refit
        if s % 30 == 29 or s == steps - 1:
            b = engine.download(what=("bodies", "controllers", "locomotion"))
            trace.append((s + 1, b["bodies"]["position"][0].copy(), int(b["controllers"]["flags"][0]), int(b["controllers"]["groundTriangleIndex"][0]),
                          int(b["locomotion"]["state"][0])))
            if log:
                log("step %4d  player (%7.3f %7.3f %7.3f)  flags %x  ground triangle %4d  locomotion %d  mover x %.3f  elevator y %.3f" % (
                    s + 1, *trace[-1][1], trace[-1][2], trace[-1][3], trace[-1][4], world[-1]["translation"][0], world[-2]["translation"][1]))
    return trace, engine.skinned()[0]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--oracle", action="store_true", help="run the CPU checker (tests/oracle_binding.py) instead of the GPU library")
    ap.add_argument("--render", action="store_true", help="shoot primary rays and shadow rays at the whole scene (ground, mirror, platforms, player) after the last step and "
                    "print the depth image with shadowed pixels marked; with --oracle: primary rays at the characters only")
    ap.add_argument("--image", metavar="PATH", help="with --render (GPU library): also write the shaded frame of the scene (ground, mirror, platforms, shadowed player; a wider camera of its own) as a binary PPM")
    ap.add_argument("--ibl", action="store_true", help="with --render --image: specular IBL from the reference's default environment cube and BRDF table; the platforms are a rough metal")
    ap.add_argument("--textures", action="store_true", help="with --render --image: a procedural checkerboard (sRGB) on the ground, a base-colour and a normal texture on the player")
    args = ap.parse_args()
    if args.oracle:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_binding
        eng = oracle_binding.oracle_engine()
    else:
        eng = sge.CharacterEngine(0)
    scene = args.render and not args.oracle
    trace, skinned = run(eng, args.steps, log=print, scene=scene, textures=args.textures)
    print("skinned vertices: %d, bounds %s .. %s" % (len(skinned), skinned.min(0).round(3), skinned.max(0).round(3)))
    if scene:
        mask, dist, hits, shadow = render_probe(eng, scene=True)
        ids = hits["instance"][hits["hit"] == 1]
        print("primary rays: %d of %d hit the scene (%d the player, %d static instances), %d shadowed, distances %.3f .. %.3f" % (
            mask.sum(), mask.size, (ids < A.SCENE_STATIC_BASE).sum(), (ids >= A.SCENE_STATIC_BASE).sum(), shadow.sum(), dist[mask].min(), dist[mask].max()))
        print(ascii_depth(mask, dist, shadow))
        if args.image:
            aov = shaded_image(eng, args.image, textures=args.textures, ibl=args.ibl)
            ids = aov["instance"]
            print("shaded frame %s: %d x %d, %d queries; pixels: %d ground, %d mirror (%d through the mirror path), %d platforms, %d player, %d with the sun shadowed" % (
                args.image, aov.shape[1], aov.shape[0], aov["queries"].sum(), (ids == A.SCENE_STATIC_BASE).sum(), (ids == A.SCENE_STATIC_BASE + 1).sum(),
                (aov["flags"] & 1).sum(), (ids >= A.SCENE_STATIC_BASE + 2).sum(), (ids == 0).sum(), (aov["shadow"] < 1).sum()))
    elif args.render:
        mask, dist, hits = render_probe(eng)
        print("primary rays: %d of %d hit the player, distances %.3f .. %.3f" % (mask.sum(), mask.size, dist[mask].min(), dist[mask].max()))
        print(ascii_depth(mask, dist))
