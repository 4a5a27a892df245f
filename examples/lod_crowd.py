#!/usr/bin/env python3
"""A crowd with per-character mesh variants chosen by distance (include/sge_amd_variants.h).

Three meshes over one skeleton (the synthetic tube mesh at full, half and quarter vertex count), a few hundred characters walking
over the synthetic terrain, and every step `lod_select` picks each character's mesh on the device from its distance to an eye
point, with no host synchronisation between the selection and the skin launch. Prints, every few steps, the split, the vertices the skin
stage wrote against what the full mesh would have cost, and one character's slice of the ragged streams.

    python examples/lod_crowd.py [--chars 512] [--steps 60]        (needs an MI355X)"""
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
    args = ap.parse_args()
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
            m = sge.crowd.synthetic_lod_mesh(eng, built, ybot, 11, 10 if variant == 1 else 5) if args.rays else sge.assets.decimate_skinned_mesh(full, keep)
            eng.upload_mesh_variant(variant, m)
            counts.append(m["positions"].shape[0])
            meshes.append(m)
        terrain = sge.crowd.upload_terrain(eng, cells=(96, 64))
        state = sge.crowd.spawn_crowd(eng, ybot, args.chars, terrain, seed=7, mode="ccd")
        pos = state["bodies"]["position"]
        eye = (float(pos[:, 0].mean()), float(pos[:, 1].mean()) + 8.0, float(pos[:, 2].min()) - 10.0)
        near, far = np.quantile(np.linalg.norm(pos - np.array(eye), axis=1), [0.1, 0.4])
        stages = sge.abi.STAGE_ALL
        if args.rays:                                 # one acceleration structure per variant (include/sge_amd_variant_blas.h)
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
    finally:
        eng.close()


if __name__ == "__main__":
    main()
