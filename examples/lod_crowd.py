#!/usr/bin/env python3
"""A crowd with per-character mesh variants chosen by distance (include/sge_amd_variants.h).

Three meshes over one skeleton (the synthetic tube mesh at full, half and quarter vertex count), a few hundred characters walking
over the synthetic terrain, and every step `lod_select` picks each character's mesh on the device from its distance to an eye
point, with no host synchronisation between the selection and the skin launch. Prints, every few steps, the split, the vertices the skin
stage wrote against what the full mesh would have cost, and one character's slice of the ragged streams.

`--render` draws the mixed crowd over a ground plane with one light and its shadow rays (include/sge_amd_variant_scene.h: the
shaded frame over a crowd with mesh variants) and prints the primary hits per variant from the AOV records.

    python examples/lod_crowd.py [--chars 512] [--steps 60] [--rays N] [--render [--image out.ppm]]        (needs an MI355X)"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chars", type=int, default=512)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rays", type=int, default=0, help="refit the acceleration structures every step and shoot this many rays down at the crowd")
    ap.add_argument("--render", action="store_true", help="after the last step, draw the mixed crowd over a ground plane (one light, shadow rays)")
    ap.add_argument("--image", default=None, help="with --render: write the frame as a binary PPM")
    ap.add_argument("--size", type=int, nargs=2, default=(160, 96), metavar=("W", "H"))
    args = ap.parse_args()
    trace = args.rays or args.render
    import __graft_entry__
    sge = __graft_entry__.build()
    ybot = sge.assets.YBotAssets()
    eng = sge.CharacterEngine(0)
    try:
        built, mesh = sge.crowd.upload_character_assets(eng, ybot)           # variant 0: 14,080 vertices
        full = dict(mesh, tangents=eng.mesh["tangents"])
        counts = [mesh["positions"].shape[0]]
        meshes = [mesh]
        for variant, keep in ((1, 0.5), (2, 0.25)):
            # ray queries need complete meshes with index buffers of their own: the synthetic mesh at a lower resolution
            m = sge.crowd.synthetic_lod_mesh(eng, built, ybot, 11, 10 if variant == 1 else 5) if trace else sge.assets.decimate_skinned_mesh(full, keep)
            eng.upload_mesh_variant(variant, m)
            counts.append(m["positions"].shape[0])
            meshes.append(m)
        terrain = sge.crowd.upload_terrain(eng, cells=(96, 64))
        state = sge.crowd.spawn_crowd(eng, ybot, args.chars, terrain, seed=7, mode="ccd")
        pos = state["bodies"]["position"]
        eye = (float(pos[:, 0].mean()), float(pos[:, 1].mean()) + 8.0, float(pos[:, 2].min()) - 10.0)
        near, far = np.quantile(np.linalg.norm(pos - np.array(eye), axis=1), [0.1, 0.4])
        stages = sge.abi.STAGE_ALL
        if trace:                                     # one acceleration structure per variant (include/sge_amd_variant_blas.h)
            eng.blas_build(mesh["indices"])
            for variant, m in enumerate(meshes[1:], 1):
                eng.blas_variant_build(variant, m["indices"])
            stages |= sge.abi.STAGE_BLAS_REFIT
            rng = np.random.default_rng(5)
        for step in range(args.steps):
            eng.lod_select(eye, [near, far])        # on the device, in front of the tick that uses it
            eng.tick(stages=stages)
            if args.rays and step % 20 == 19:
                # aimed straight down through skinned vertices of a few characters (instance matrices stay the identity: the
                # rays live in the space the streams are in)
                picks = rng.integers(0, args.chars, 8)
                verts = np.concatenate([eng.skinned_character(int(c), normals=False, tangents=False)[0] for c in picks])
                target = verts[rng.integers(0, len(verts), args.rays)]
                origin = target + (0.0, 30.0, 0.0)
                hits = eng.blas_intersect(origin, np.tile(np.array([0, -1, 0], np.float32), (args.rays, 1)), np.full(args.rays, -1, np.int32))
                _, record = eng.blas_variant_bounds()
                hit = hits["hit"] == 1
                per = np.bincount(record[hits["instance"][hit]], minlength=3)[:3]
                print("step %3d: %d rays, %d hits; hits per variant %s" % (step + 1, args.rays, int(hit.sum()), per.tolist()))
            if step % 20 == 19:
                plan = eng.skin_plan()                # waits for the skin launch
                off = eng.vertex_offsets()
                p, n, t = eng.skinned_character(0)
                print("step %3d: characters per variant %s, %d vertices written (%.0f %% of the full mesh for all), dropped %d; "
                      "character 0 owns vertices [%d, %d) = %d positions" %
                      (step + 1, list(plan.perVariant)[:3], plan.totalVertices, 100.0 * plan.totalVertices / (args.chars * counts[0]),
                       plan.dropped, off[0], off[1], p.shape[0]))
        if args.render:
            render(sge, eng, eye, args)
    finally:
        eng.close()


def render(sge, eng, eye, args):
    """The crowd as the newest refit left it, over a ground plane, from the eye point of the LOD selection."""
    A = sge.abi
    st = eng.scene_crowd_status()
    assert st.crowdReady == 1 and st.ragged == 1, (st.reason, st.variant)
    off = eng.vertex_offsets()
    pos = eng.skinned(0, int(off[-1]), normals=False, tangents=False)[0]
    lo, hi = pos.min(0), pos.max(0)
    y = float(lo[1]) - 0.02
    ground = np.array([[lo[0] - 20, y, lo[2] - 20], [hi[0] + 20, y, lo[2] - 20], [hi[0] + 20, y, hi[2] + 20], [lo[0] - 20, y, hi[2] + 20]], np.float32)
    eng.scene_mesh_upload(0, ground, np.tile(np.array([0, 1, 0], np.float32), (4, 1)), np.tile(np.array([1, 0, 0, 1], np.float32), (4, 1)),
                          np.array([0, 2, 1, 0, 3, 2], np.uint32))
    eng.scene_instances([0], np.eye(4, dtype=np.float32).reshape(1, 16))
    mats = A.default_render_materials(2)
    mats["baseColor"][0], mats["baseColor"][1] = (0.55, 0.6, 0.5), (0.9, 0.55, 0.35)
    eng.render_materials(mats)
    eng.render_static_materials([0])
    eng.render_crowd_materials(np.ones(eng.count, np.int32))
    light = np.zeros(1, A.render_light_dtype)
    light["direction"], light["intensity"], light["color"], light["enabled"], light["maxDistance"] = (-0.4, -1.0, 0.3), 2.6, (1.0, 0.95, 0.85), 1.0, 1e4
    eng.render_lights(light)
    W, H = args.size
    eye = np.array(eye, np.float64)
    target = (lo + hi) / 2
    f = target - eye; f /= np.linalg.norm(f)
    s = np.cross(f, (0.0, 1.0, 0.0)); s /= np.linalg.norm(s)
    u = np.cross(s, f)
    view = np.eye(4); view[0, :3], view[1, :3], view[2, :3] = s, u, -f
    view[:3, 3] = -view[:3, :3] @ eye
    t, near, far = 1.0 / np.tan(0.5), 0.1, 5000.0
    proj = np.array([[t * H / W, 0, 0, 0], [0, t, 0, 0], [0, 0, far / (near - far), near * far / (near - far)], [0, 0, -1, 0]])
    frame = sge.CharacterEngine.render_frame_record(np.linalg.inv(proj @ view), eye, W, H, 1)
    rgba, aov = eng.render_frame(frame, aov=True)
    _, record = eng.blas_variant_bounds()
    on_crowd = (aov["instance"] >= 0) & (aov["instance"] < eng.count)
    per = np.bincount(record[aov["instance"][on_crowd]], minlength=3)[:3]
    print("frame %d x %d: %d pixels on the crowd, primary hits per variant %s, %d on the ground, %d in shadow of light 0" %
          (W, H, int(on_crowd.sum()), per.tolist(), int((aov["instance"] >= A.SCENE_STATIC_BASE).sum()), int(((aov["instance"] >= 0) & (aov["shadow"] < 0.5)).sum())))
    if args.image:
        px = (np.clip(rgba[..., :3], 0.0, 1.0) ** (1 / 2.2) * 255.0 + 0.5).astype(np.uint8)
        with open(args.image, "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (W, H))
            fh.write(px.tobytes())
        print("wrote", args.image)


if __name__ == "__main__":
    main()
