/*
 * sge_amd_variant_blas.h — acceleration structures, refit and ray queries for a crowd with mesh variants.
 *
 * An addition to sge_amd_variants.h (same conventions, same library, SGE_ABI_VERSION stays 2). In the reference every character's
 * own SkinnedMeshComponent feeds RTAccelerationBuilder (build once, refit every frame) and raytraceKernel reads the skinned streams
 * at a hit. sge_amd.h does that for a crowd that shares ONE mesh; with this header a context whose characters name one of several
 * meshes (sge_amd_variants.h) gets one topology per variant, a refit over the ragged streams and closest-hit queries against
 * characters of mixed variants.
 *
 * Ready. The context is READY when variant 0 has sge_blas_build and every variant 1..N has sge_blas_variant_build newer than its
 * latest mesh upload. Uploading a variant (new or replaced), re-uploading variant 0, and sge_blas_build (for every variant's
 * structure) make it not ready again. While it is not ready, everything sge_amd_variants.h lists as out of scope is refused as
 * that header says. Once it is ready:
 *   - SGE_STAGE_BLAS_REFIT together with SGE_STAGE_SKIN (whole crowd) refits right behind the skin launch, on the stream that
 *     launch ran on and in front of the event sge_skin_wait waits for: a consumer ordered by sge_skin_wait sees the boxes of the
 *     same launch as the streams. SGE_OPT_FUSE_BLAS_REFIT is ignored (always separate launches).
 *   - SGE_STAGE_BLAS_REFIT alone and sge_blas_refit(0, all) refit over the plan of the newest skin launch (SGE_ERR_STATE when no
 *     skin stage with variants has run, SGE_ERR_STATE naming the "whole crowd" for a sub-range).
 *   - sge_blas_intersect_batch / sge_blas_intersect_device: hit.primitive is a triangle of the index buffer of the hit
 *     character's variant. sge_blas_instances_upload works as always.
 *   - sge_blas_refit_buffers stays refused (caller-owned buffers carry no vertex offsets) and sge_blas_bounds_download returns
 *     SGE_ERR_STATE (its row shape is variant 0's): use sge_blas_variant_bounds_download.
 *
 * Layout of the boxes. Character c owns bounds[c][rowStride][6], rowStride = the maximum over the variants of entryCount_v + 1.
 * Rows 0 .. entryCount_v are meaningful, the root box is row entryCount_v of the character's own variant; rows beyond are never
 * written by a refit. Beside the boxes sits uint8_t charVariant[count], written by the refit: the variant whose structure the
 * boxes of c describe, 0xFF after sge_characters_resize and for a character the newest plan dropped at the capacity cut
 * (sge_crowd_reserve_vertices). Ray queries read THIS record, not the live variant bytes, so boxes and index buffer stay those
 * of the newest refit even after a later sge_lod_select. The vertex offsets the queries use are those of the newest skin launch;
 * the two are kept in step this way: a skin stage WITHOUT SGE_STAGE_BLAS_REFIT sets every record to 0xFF on the stream of its
 * launch (its offsets belong to another plan than the boxes in place), and the next refit (SGE_STAGE_BLAS_REFIT alone,
 * sge_blas_refit, or the next tick with both stages) writes them again. A ray that names a character with record 0xFF misses; a
 * ray with instance < 0 never reports such a character. With the context ready, sge_blas_buffers hands out NULL for d_bounds
 * (variant 0's uniform box table is released; the boxes are those of sge_blas_variant_buffers).
 */
#ifndef SGE_AMD_VARIANT_BLAS_H
#define SGE_AMD_VARIANT_BLAS_H

#include "sge_amd_variants.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGE_HAS_VARIANT_BLAS 1

/* encoder.build for variant 1 .. SGE_MAX_MESH_VARIANTS - 1: the topology comes from that variant's uploaded source positions and
 * indices[index_count] (uint32, three per triangle). variant == 0 is SGE_ERR_INVALID (use sge_blas_build), a variant that was
 * never uploaded is SGE_ERR_INVALID, SGE_ERR_STATE before sge_blas_build. index_count <= 0, an index >= the variant's vertex
 * count and a hierarchy too deep for the traversal stack fail exactly as sge_blas_build fails them. Synchronises. */
int sge_blas_variant_build(sge_context* ctx, int32_t variant, const uint32_t* indices, int32_t index_count);

/* Optional, like sge_blas_set_uvs: uvs[vertex_count][2] of the variant's mesh; hits on its characters then carry interp_uv.
 * variant 0 is accepted (the same as sge_blas_set_uvs). */
int sge_blas_variant_set_uvs(sge_context* ctx, int32_t variant, const float* uvs, int32_t vertex_count);

/* sge_blas_info of one variant's structure (variant 0: that of sge_blas_build). SGE_ERR_STATE when it is not built. */
int sge_blas_variant_info_get(sge_context* ctx, int32_t variant, sge_blas_info* info);

/* (a struct tag, not a typedef: the function below carries the same name, so C and C++ callers write `struct sge_blas_variant_layout`) */
struct sge_blas_variant_layout {
    int32_t ready;      /* 1: every uploaded variant has a structure (see Ready) */
    int32_t variants;   /* uploaded meshes, variant 0 included */
    int32_t rowStride;  /* rows of six floats per character; 0 while not ready */
    int32_t _pad;
    int32_t entryCount[SGE_MAX_MESH_VARIANTS]; /* per variant; 0 where no structure is built */
};

/* Never fails for a valid context: ready = 0 says why nothing else here works yet. */
int sge_blas_variant_layout(sge_context* ctx, struct sge_blas_variant_layout* out);

/* bounds[count][rowStride][6] and variants[count] (the charVariant record; either pointer may be NULL) of characters
 * [first, first + count). Synchronises. SGE_ERR_STATE while not ready. */
int sge_blas_variant_bounds_download(sge_context* ctx, int32_t first, int32_t count, float* bounds, uint8_t* variants);

/* Device pointers: the boxes, the charVariant record and every variant's index buffer (NULL beyond the uploaded variants). Any
 * out pointer may be NULL. Valid until the context stops being ready or sge_characters_resize. SGE_ERR_STATE while not ready. */
int sge_blas_variant_buffers(sge_context* ctx, void** d_bounds, void** d_char_variants, void* d_indices[SGE_MAX_MESH_VARIANTS]);

#ifdef __cplusplus
}
#endif

#endif /* SGE_AMD_VARIANT_BLAS_H */
