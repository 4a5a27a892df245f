/*
 * sge_amd_variants.h — per-character mesh variants and distance LOD for the skinned crowd.
 *
 * An addition to sge_amd.h (same conventions, same library, SGE_ABI_VERSION stays 2). The reference gives every character its
 * own SkinnedMeshComponent and RTSkinningJob (Game/RTSkinningEncoder.swift:37-54); a context of sge_amd.h owns ONE skinned mesh.
 * With this header a context holds up to SGE_MAX_MESH_VARIANTS meshes over one skeleton, every character names one of them
 * by a byte that may change every step without a host synchronisation, and the skin stage of sge_tick writes a RAGGED layout:
 * character c owns vertices [off[c], off[c+1]) of the three streams of sge_crowd_buffers, off = the exclusive scan of the
 * characters' vertex counts, computed on the device in front of every skin launch.
 *
 * Nothing changes for a context that never uploads a variant >= 1: its skin stage takes the code path it always took.
 *
 * Ordering. sge_characters_set_mesh_variants and sge_lod_select are enqueued on the context's stream (sge_context_set_stream) and
 * return at once. The skin stage of sge_tick copies the variant array on that stream when the tick is issued, so a skin launch sees
 * exactly the writes enqueued in front of its tick, also under SGE_OPT_OVERLAP_SKIN (1 or 2), where the launch itself runs later on
 * the context's second stream; a write behind the tick never changes the array under a launch in flight. A caller's own kernel
 * that writes the buffer of sge_crowd_variant_buffer runs on the context's stream, or is ordered in front of the next sge_tick.
 * The offsets (sge_crowd_vertex_offsets) are written by the skin launch: a consumer on another stream reads them after
 * sge_skin_wait and calls sge_skin_consumed after its last read, exactly as for the streams themselves.
 *
 * Out of scope while a variant >= 1 exists (SGE_ERR_STATE, text via sge_last_error):
 *   - SGE_STAGE_BLAS_REFIT (fused or not), sge_blas_refit, sge_blas_refit_buffers, sge_blas_intersect_batch and
 *     sge_blas_intersect_device, until every uploaded variant has an acceleration structure (sge_amd_variant_blas.h says
 *     when that is and what opens up then; sge_blas_refit_buffers stays refused): the structure of variant 0 alone does not
 *     describe the ragged streams;
 *   - SGE_STAGE_SKIN on a sub-range of the crowd (first / count other than the whole crowd): the offsets are a scan over all.
 */
#ifndef SGE_AMD_VARIANTS_H
#define SGE_AMD_VARIANTS_H

#include "sge_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGE_HAS_MESH_VARIANTS 1
#define SGE_MAX_MESH_VARIANTS 8

/* Mesh number `variant` (1 .. SGE_MAX_MESH_VARIANTS - 1) of the context. Variant 0 is the mesh of sge_skinned_mesh_upload and is
 * replaced only through that call (variant == 0 here: SGE_ERR_INVALID). Variants share the skeleton and variant 0's inverse bind
 * matrices: desc->invBindModel must be NULL (else SGE_ERR_INVALID); a bone index >= the skeleton's bone count is SGE_ERR_INVALID;
 * any vertexCount >= 1 is accepted. Variants are numbered without gaps: `variant` is an existing one (replaced) or the next free
 * index (else SGE_ERR_INVALID). SGE_ERR_STATE before sge_skinned_mesh_upload. Synchronises; the output streams are reallocated
 * (their pointers may move) when the default capacity grows. */
int sge_skinned_mesh_variant_upload(sge_context* ctx, int32_t variant, const sge_skinned_mesh_desc* desc);

/* variants[count] (host) for characters [first, first + count); every character starts at 0 (sge_characters_resize). An index
 * of a variant that was never uploaded is SGE_ERR_INVALID. Asynchronous on the context's stream; the host array may be reused
 * when the call returns. */
int sge_characters_set_mesh_variants(sge_context* ctx, int32_t first, int32_t count, const uint8_t* variants);

/* The device array uint8_t[count] the calls above write, for a caller's own selection kernel (see Ordering). The next skin
 * launch clamps values >= the number of uploaded variants to the highest uploaded one. Valid until sge_characters_resize. */
int sge_crowd_variant_buffer(sge_context* ctx, void** d_variants);

/* Distance LOD on the device: variant[c] = number of i < n with |position[c] - eye|^2 >= distances[i]^2, clamped to the highest
 * uploaded variant. n <= SGE_MAX_MESH_VARIANTS - 1, distances strictly ascending and >= 0 (else SGE_ERR_INVALID). position is
 * sge_body_state.position of the newest move stage, and the arithmetic is float64 without contraction:
 * ((dx * dx + dy * dy) + dz * dz) >= (double)distances[i] * (double)distances[i]. Asynchronous on the context's stream. */
int sge_lod_select(sge_context* ctx, const double eye[3], const float* distances, int32_t n);

/* Capacity of the three output streams in vertices. 0 restores the default, count x the largest uploaded vertexCount; fewer
 * than `count` vertices is SGE_ERR_INVALID. A value > 0 needs a variant >= 1 (SGE_ERR_STATE without one: the uniform launch
 * forms write count x vertexCount vertices and know no capacity); sge_characters_resize drops the reservation. A character
 * whose slice [off[c], off[c+1]) would end beyond the capacity is not skinned that step and counted in
 * sge_skin_plan_info.dropped; nothing is ever stored at or beyond the capacity. Synchronises;
 * the streams are reallocated when the capacity exceeds what is allocated (a smaller capacity keeps the allocation). */
int sge_crowd_reserve_vertices(sge_context* ctx, int64_t vertices);

/* The device array int64_t[count + 1] of vertex offsets the newest skin launch wrote (see Ordering). SGE_ERR_STATE for a
 * context without a variant >= 1: its layout is the uniform one, character c at c x vertexCount. */
int sge_crowd_vertex_offsets(sge_context* ctx, void** d_offsets);

typedef struct sge_skin_plan_info {
    int64_t totalVertices;    /* off[count]: what the crowd asks for, dropped characters included */
    int64_t capacityVertices; /* the capacity the launch was planned against */
    int32_t perVariant[SGE_MAX_MESH_VARIANTS]; /* characters skinned per variant (after clamping, without the dropped) */
    int32_t units;            /* work units of the launch: (variant, group of up to charsPerUnit characters, vertex split) */
    int32_t dropped;          /* characters left out because their slice would end beyond the capacity */
    int32_t charsPerUnit;
    int32_t _pad;
} sge_skin_plan_info;

/* Waits for the newest skin launch and reads its plan. SGE_ERR_STATE when no skin stage with variants has run. */
int sge_skin_plan_read(sge_context* ctx, sge_skin_plan_info* out);

#ifdef __cplusplus
}
#endif

#endif /* SGE_AMD_VARIANTS_H */
