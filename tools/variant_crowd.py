"""Shared by scene_ray_bench.py and render_bench.py (--variants): the committed workload's settled crowd with three mesh variants
(include/sge_amd_variants.h, include/sge_amd_variant_scene.h), chosen every step by sge_lod_select from an eye point.

  control   all three variants hold the full mesh (14,080 vertices): the kernels walk the per-variant table, the geometry is the
            uniform crowd's, so its time against the uniform line of the same run is the price of the ragged walk alone
  lod       full, half and quarter vertex count (the synthetic mesh at 22 x 10, 11 x 10 and 11 x 5 vertices per bone)
The thresholds are the terciles of the spawn distances to the eye, so each variant holds about a third of the characters."""
import numpy as np


def settled_crowd(sge, n, mode, eye_of, ticks=130):
    """mode 'control' | 'lod'; eye_of(lo, hi) -> eye point from the spawn positions' bounds. -> engine (ticked `ticks` times with
    the refit, instance matrices set as the benches set them), body positions, characters per variant of the newest skin launch."""
    abi = sge.abi
    eng = sge.CharacterEngine(0)
    ybot = sge.assets.YBotAssets()
    built, mesh = sge.crowd.upload_character_assets(eng, ybot)
    full = dict(mesh, tangents=eng.mesh["tangents"])
    lods = [full, full] if mode == "control" else [sge.crowd.synthetic_lod_mesh(eng, built, ybot, 11, 10), sge.crowd.synthetic_lod_mesh(eng, built, ybot, 11, 5)]
    for k, m in enumerate(lods, 1):
        eng.upload_mesh_variant(k, m)
    terrain = sge.crowd.upload_terrain(eng)
    state = sge.crowd.spawn_crowd(eng, ybot, n, terrain, mode="ccd")
    eng.blas_build(eng.mesh["indices"])
    for k, m in enumerate(lods, 1):
        eng.blas_variant_build(k, m["indices"])
    pos = np.asarray(state["bodies"]["position"], np.float64)
    eye = np.asarray(eye_of(pos.min(0), pos.max(0)), np.float64)
    near, far = np.quantile(np.linalg.norm(pos - eye, axis=1), [1 / 3, 2 / 3])
    for _ in range(ticks):
        eng.lod_select(tuple(eye), [near, far])
        eng.tick(stages=abi.STAGE_ALL | abi.STAGE_BLAS_REFIT)
    P = eng.download(what=("bodies",))["bodies"]["position"].astype(np.float32)
    mats = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    mats[:, 3, :3] = P
    eng.blas_instances(mats.reshape(n, 16))
    st = eng.scene_crowd_status()
    assert st.crowdReady == 1 and st.ragged == 1, (st.reason, st.variant)
    plan = eng.skin_plan()
    return eng, P, list(plan.perVariant)[:3], [full["positions"].shape[0]] + [m["positions"].shape[0] for m in lods]
