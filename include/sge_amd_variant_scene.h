/*
 * sge_amd_variant_scene.h — a crowd with mesh variants in the ray scene and in the shaded frame.
 *
 * An addition to sge_amd_render.h (same conventions, same library, SGE_ABI_VERSION stays 2). sge_amd_variants.h gives every
 * character one of up to SGE_MAX_MESH_VARIANTS meshes and sge_amd_variant_blas.h one acceleration structure per variant;
 * sge_amd_ray_scene.h and sge_amd_render.h trace and shade static instances beside the crowd. With this header the two meet: every
 * SkinnedMeshComponent feeds RTAccelerationBuilder whatever mesh it holds (RTAccelerationBuilder.swift:148-185), so a crowd of
 * mixed variants is traced by sge_scene_intersect_*, occludes in sge_scene_occluded_* and is drawn by sge_render_frame_*. No
 * prototype of an older header changes; this header adds the contract and one entry point that says why a crowd is left out.
 *
 * When the crowd is traced. A context with at least one mesh variant beyond variant 0 reports crowdReady = 1 exactly when all of
 * these hold: the context is READY in the sense of sge_amd_variant_blas.h (sge_blas_build for variant 0 and sge_blas_variant_build
 * for every other uploaded variant, each newer than that variant's mesh); sge_characters_resize gave a count > 0; the
 * per-character box table, the record of every character's variant, the vertex offsets, the instance matrices and the three
 * skinned output streams exist for that count. Until then the context behaves as before: the statics are traced alone,
 * crowdReady = 0, a ray that names a character misses, and no entry point fails. A context without mesh variants is unchanged.
 *
 * Per character (sge_amd_variant_blas.h). Queries read the record the newest refit left, not the variant bytes a later
 * sge_lod_select or sge_character_variants_set wrote: a character is traced with the structure, the vertices and the index buffer
 * of the variant it was skinned and refitted as. A character without a record — dropped at the capacity cut of the ragged streams
 * (sge_crowd_reserve_vertices), or any character after sge_characters_resize or after a skin stage that no refit followed — is
 * not in the scene: a ray that names it misses, a whole-scene ray never reports it, it occludes nothing and is not in the frame.
 * crowdReady stays 1 through all of this; the next refit brings the characters back. hit.primitive and aov.primitive name a
 * triangle of the index buffer of the hit character's variant; hit.uv is interpolated from that variant's uvs (0 without).
 * sge_render_crowd_materials assigns per character, whatever its variant. The closest-hit key (distance bits, scene id, primitive
 * id), the tie rule between the halves and the hit record are those of sge_amd_ray_scene.h: a hit on a character is field for
 * field that of sge_blas_intersect_batch on the same context.
 *
 * Ordering is unchanged: the *_batch forms synchronise; the *_device forms are enqueued on the context's stream behind the skin
 * and refit launches of the newest sge_tick under every SGE_OPT_OVERLAP_SKIN mode, and every query refreshes the crowd's world
 * boxes itself.
 */
#ifndef SGE_AMD_VARIANT_SCENE_H
#define SGE_AMD_VARIANT_SCENE_H

#include "sge_amd_variant_blas.h"
#include "sge_amd_render.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGE_HAS_VARIANT_SCENE 1

/* sge_scene_crowd_status.reason: the first of these that applies, in this order */
#define SGE_SCENE_CROWD_OK 0
#define SGE_SCENE_CROWD_NO_MESH 1           /* no sge_skinned_mesh_upload */
#define SGE_SCENE_CROWD_NO_STRUCTURE 2      /* no sge_blas_build newer than the mesh (variant 0's) */
#define SGE_SCENE_CROWD_NO_CHARACTERS 3     /* sge_characters_resize gave no character */
#define SGE_SCENE_CROWD_VARIANT_NOT_BUILT 4 /* a variant lacks sge_blas_variant_build newer than its mesh */
#define SGE_SCENE_CROWD_NO_BUFFERS 5        /* a per-character buffer or an output stream does not exist for the count */

/* (a struct tag, not a typedef, as sge_scene_info) */
struct sge_scene_crowd_status {
    int32_t crowdReady; /* as sge_scene_info */
    int32_t ragged;     /* 1: the crowd is traced through the per-variant table */
    int32_t reason;     /* why crowdReady is 0: SGE_SCENE_CROWD_*; SGE_SCENE_CROWD_OK exactly when crowdReady is 1 */
    int32_t variant;    /* for SGE_SCENE_CROWD_VARIANT_NOT_BUILT: the lowest such variant, else -1 */
};

/* What sge_scene_* and sge_render_frame_* will do with the crowd, and what to call when they leave it out. Never fails for a valid
 * context; touches no device state. */
int sge_scene_crowd_status_get(sge_context* ctx, struct sge_scene_crowd_status* out);

#ifdef __cplusplus
}
#endif

#endif /* SGE_AMD_VARIANT_SCENE_H */
