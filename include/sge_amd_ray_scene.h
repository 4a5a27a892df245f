/*
 * sge_amd_ray_scene.h — the ray scene: static mesh instances and occlusion rays beside the skinned crowd.
 *
 * An addition to sge_amd_variant_blas.h (same conventions, same library, SGE_ABI_VERSION stays 2). RTAccelerationBuilder.build
 * puts two kinds of primitive structure under its instance structure (RTAccelerationBuilder.swift:148-185): cachedDynamicBLAS,
 * one per skinned item, refitted every frame — that is sge_blas_* of sge_amd.h — and cachedStaticBLAS, one per static slice, built
 * once (:37-71) and instanced with item.modelMatrix (:177). This header adds the second kind and the queries over both: the
 * closest hit with everything raytraceKernel derives at a hit (RayTracing.metalinc:246-300), and the any-hit question its shadow
 * rays ask (:334-343: is anything between min_distance and max_distance).
 *
 * Scene instance id. `instance` in a ray or a hit is a scene id: character c is c, as in sge_amd.h; static instance s is
 * SGE_SCENE_STATIC_BASE + s. A ray with instance < 0 asks the whole scene, a ray with instance >= 0 that one instance; an id
 * that names nothing (a character beyond the crowd, a character while the crowd cannot be traced, a static instance beyond the
 * list) is a miss.
 *
 * Closest hit. The winner is the minimum over (distance bits, scene id, primitive id): at equal distance the smaller scene id
 * wins, so a character beats a static instance, then the smaller primitive id. A hit on a static instance carries the record
 * sge_blas_intersect_batch fills for a character, computed by the same expressions from the mesh's own streams and the
 * instance's matrix; hit.primitive is a triangle of the mesh's index buffer. A hit on a character is field for field that of
 * sge_blas_intersect_batch.
 *
 * The crowd is optional. A context with no skinned mesh, no characters or no sge_blas_build traces the static half alone, and a
 * ray that names a character misses. A context with mesh variants (sge_amd_variants.h) is traced through these entry points once
 * every variant has its structure: sge_amd_variant_scene.h states that contract and the per-character semantics. While a variant
 * lacks its structure such a context traces the statics only and sge_scene_info_get reports crowdReady = 0.
 * sge_blas_intersect_* is unchanged and sees characters only.
 * Where sge_blas_intersect_* returns SGE_ERR_STATE, these entry points do not fail: they leave the crowd out and report
 * crowdReady = 0 (sge_amd_variant_scene.h adds the reason). For a crowd that shares one mesh crowdReady is 1 exactly when all of
 * these hold: sge_skinned_mesh_upload
 * and sge_blas_build have been called, the latter after the newest mesh upload; sge_characters_resize gave a count > 0; the
 * per-character boxes and instance matrices exist for that count (sge_blas_build or sge_characters_resize, whichever came
 * last, allocates them) and so do the skinned output streams. A renderer checks it once after setting up the crowd.
 *
 * Ordering. The *_batch forms synchronise. The *_device forms and sge_scene_instances_update are enqueued on the context's stream
 * (sge_context_set_stream), behind the skin and refit launches of the newest sge_tick under every SGE_OPT_OVERLAP_SKIN mode,
 * exactly as sge_blas_intersect_device. Whole-scene rays are always allowed: every query refreshes the crowd's world boxes itself.
 */
#ifndef SGE_AMD_RAY_SCENE_H
#define SGE_AMD_RAY_SCENE_H

#include "sge_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGE_HAS_RAY_SCENE 1

#define SGE_SCENE_STATIC_BASE 0x40000000 /* scene id of static instance 0 */
#define SGE_MAX_SCENE_MESHES 64
#define SGE_MAX_SCENE_INSTANCES 262144

/* (a struct tag, not a typedef, as sge_blas_variant_layout) */
struct sge_scene_info {
    int32_t meshes;          /* uploaded static meshes */
    int32_t staticInstances; /* length of the static instance list */
    int32_t characters;      /* sge_characters_resize */
    int32_t crowdReady;      /* 1: the crowd has a built structure these entry points trace (see "The crowd is optional") */
};

/* encoder.build for one static slice (RTAccelerationBuilder.swift:37-71): mesh 0 .. SGE_MAX_SCENE_MESHES - 1 from
 * positions[vertex_count][3], normals[vertex_count][3], tangents[vertex_count][4], uvs[vertex_count][2] (or NULL: hits carry
 * uv = 0) and indices[index_count] (uint32, three per triangle). The topology is the 64-wide tree of sge_blas_build; the entry
 * boxes are computed once. index_count <= 0, an index >= vertex_count and a hierarchy too deep for the traversal stack fail
 * exactly as sge_blas_build fails them. Uploading again a mesh that instances name is allowed: later queries see the new mesh.
 * Synchronises. */
int sge_scene_mesh_upload(sge_context* ctx, int32_t mesh, const float* positions, const float* normals, const float* tangents,
                          const float* uvs, int32_t vertex_count, const uint32_t* indices, int32_t index_count);

/* sge_blas_info of one static mesh's structure. SGE_ERR_INVALID for a mesh that was never uploaded. */
int sge_scene_mesh_info_get(sge_context* ctx, int32_t mesh, sge_blas_info* info);

/* bounds[entryCount + 1][6] of one static mesh (object space; the last row is the root box). Synchronises. */
int sge_scene_mesh_bounds_download(sge_context* ctx, int32_t mesh, float* bounds);

/* The instance descriptors of the static items (RTAccelerationBuilder.swift:168-185): replaces the whole list. count = 0 clears
 * it. mesh_of_instance[count]; model_matrices[count][16], column-major as in sge_blas_instances_upload (item.modelMatrix, :177).
 * A mesh id that was never uploaded, a non-finite matrix entry, a 3x3 part whose determinant is 0 and count >
 * SGE_MAX_SCENE_INSTANCES give SGE_ERR_INVALID and leave the scene as it was. Synchronises. */
int sge_scene_instances_set(sge_context* ctx, int32_t count, const int32_t* mesh_of_instance, const float* model_matrices);

/* New matrices for instances [first, first + count) (kinematic platforms, every frame: RTAccelerationBuilder.swift:177 reads
 * item.modelMatrix per build). Validated like sge_scene_instances_set. The host array may be reused on return; the copy and the
 * refresh of the instances' world boxes are enqueued on the context's stream. */
int sge_scene_instances_update(sge_context* ctx, int32_t first, int32_t count, const float* model_matrices);

/* Never fails for a valid context. */
int sge_scene_info_get(sge_context* ctx, struct sge_scene_info* info);

/* intersector.intersect(ray, accel) + the reads at the hit (RayTracing.metalinc:242-300) over the whole scene. Host arrays. */
int sge_scene_intersect_batch(sge_context* ctx, const sge_blas_ray* rays, int32_t count, sge_blas_hit* hits);

/* The same over device-resident sge_blas_ray / sge_blas_hit records; enqueued (see Ordering). */
int sge_scene_intersect_device(sge_context* ctx, const void* d_rays, int32_t count, void* d_hits);

/* The shadow ray's question (RayTracing.metalinc:334-343): occluded[i] = 1 when any triangle of the asked instances is hit with
 * max(minDistance, 0) <= t <= maxDistance, else 0 — the `hit` of sge_scene_intersect_batch for the same ray. Host arrays. */
int sge_scene_occluded_batch(sge_context* ctx, const sge_blas_ray* rays, int32_t count, int32_t* occluded);

/* The same over device-resident rays and int32 words; enqueued (see Ordering). */
int sge_scene_occluded_device(sge_context* ctx, const void* d_rays, int32_t count, void* d_occluded);

#ifdef __cplusplus
}
#endif

#endif /* SGE_AMD_RAY_SCENE_H */
