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
    args = ap.parse_args()
    import __graft_entry__
    sge = __graft_entry__.build()
    ybot = sge.assets.YBotAssets()
    eng = sge.CharacterEngine(0)
    try:
        _, mesh = sge.crowd.upload_character_assets(eng, ybot)           # variant 0: 14,080 vertices
        full = dict(mesh, tangents=eng.mesh["tangents"])
        counts = [mesh["positions"].shape[0]]
        for variant, keep in ((1, 0.5), (2, 0.25)):
            m = sge.assets.decimate_skinned_mesh(full, keep)
            eng.upload_mesh_variant(variant, m)
            counts.append(m["positions"].shape[0])
        terrain = sge.crowd.upload_terrain(eng, cells=(96, 64))
        state = sge.crowd.spawn_crowd(eng, ybot, args.chars, terrain, seed=7, mode="ccd")
        pos = state["bodies"]["position"]
        eye = (float(pos[:, 0].mean()), float(pos[:, 1].mean()) + 8.0, float(pos[:, 2].min()) - 10.0)
        near, far = np.quantile(np.linalg.norm(pos - np.array(eye), axis=1), [0.1, 0.4])
        for step in range(args.steps):
            eng.lod_select(eye, [near, far])        # on the device, in front of the tick that uses it
            eng.tick()
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
