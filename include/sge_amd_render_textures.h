/*
 * sge_amd_render_textures.h — textures in the shaded frame: the bilinear sampler, sample_material, sample_alpha and the normal map
 * of raytraceKernel (RayTracing.metalinc:132-195, :283-316, :357, :425-460, :514, :596-630, :684).
 *
 * An addition to sge_amd_render.h (same conventions, same library, SGE_ABI_VERSION stays 2). That header's frame behaves as the
 * reference does with frame.textureCount == 0; this one adds the texture array (up to SGE_MAX_RENDER_TEXTURES slots), the texture
 * indices of RTInstanceInfo (ShaderTypes.h:118-124, filled from the item's material by RTGeometryCache.swift:328-353) as one entry
 * per material of the table, and the five places the text samples. CDNA has no sampler to lean on: the filter is a HIP function
 * over plain global loads of packed 32-bit texels, which is also what lets it be pinned bit for bit (below).
 *
 * Textures (TextureResource.swift): rgba8Unorm or rgba8Unorm_srgb, mipmapped: false. Every sampler of the text is
 * constexpr sampler(mip_filter::linear, mag_filter::linear, min_filter::linear) (:153, :160, :166, :171, :189, :303): normalised
 * coordinates, the default clamp-to-edge address mode, and — a compute kernel has no derivatives — level 0 with a bilinear filter.
 *
 * A slot that holds no texture is what `index >= textureCount` is in the text: a material that names it behaves as if it named
 * none. When no material binds a slot that holds a texture, the frame is the frame of sge_amd_render.h, byte for byte (the same
 * kernel runs).
 *
 * Where the text samples, with (uv, normal, tangent, bitangent) the fields of the hit record of sge_scene_intersect_* at that hit
 * (interp_uv :106-119 and :283-302, by the expressions of that record; a mesh without uvs has uv = (0, 0)):
 *   sample_material (:132-176), at the layer's surface and at both bounce surfaces, after the factor clamps of :143-150:
 *     base *= tex.xyz and alpha *= tex.w (baseColor); roughness *= mr.y and metallic *= mr.z (metallicRoughness);
 *     emissive *= em.xyz (emissive); occlusion *= occ.x (occlusion). The mirror test, the Fresnel mixes, the transmission mix and the
 *     compositing alpha use these sampled values of the layer's surface.
 *   sample_alpha (:178-195), for every occluder of a shadow walk: clamp(mrFactors.y, 0, 1) * tex.w of the occluder's baseColor
 *     texture at the occluder's uv.
 *   the normal map (:283-316), at all three surfaces, with V = normalize(-direction) of the ray that found the surface:
 *     nTex = sample.xyz * 2 - 1; NoV = sat(dot(Ngeom, V)); t = sat((NoV - 0.05) / (0.5 - 0.05)), graze = (t * t) * (3 - 2 * t);
 *     ns = 4 + max(normalScale - 4, 0) * 0.25 (as :308-310 write it: there is no min); x = nTex.x * (ns * graze), y = nTex.y *
 *     (ns * graze); z = sqrt(max(1 - (x * x + y * y), 0)); N = normalize((tangent * x + bitangent * y) + normal * z), negated when
 *     dot(N, direction) > 0. This N is the N of everything behind it: NdotL, the shadow origin hitPos + N * bias, eval_brdf, the SH
 *     ambient, reflect, refract and NoV of the mixes. normalize and dot are those of sge_amd_render.h.
 *
 * The pinned sampler (float32, no contraction, every expression evaluated as written, left to right).
 *   Decode, before filtering: a unorm channel is (float)c / 255.0f. For SGE_TEX_RGBA8_UNORM_SRGB r, g and b go through a table of
 *   256 floats, computed once on the host in double and rounded to float32: with s = c / 255, s <= 0.04045 ? s / 12.92 :
 *   pow((s + 0.055) / 1.055, 2.4); alpha stays (float)c / 255.0f. sge_render_srgb_table_get returns the table.
 *   Coordinates: x = fminf(fmaxf(u * (float)W - 0.5f, 0.0f), (float)(W - 1)); x0 = (int)floorf(x); x1 = min(x0 + 1, W - 1);
 *   fx = x - (float)x0; the same for y with v and H. This is clamp-to-edge (clamping the coordinate is clamping the two indices).
 *   A NaN coordinate becomes 0 through fmaxf; +inf becomes W - 1, -inf becomes 0.
 *   Filter, per channel, with tXY the decoded texel (xX, yY): top = t00 * (1 - fx) + t10 * fx; bot = t01 * (1 - fx) + t11 * fx;
 *   out = top * (1 - fy) + bot * fy.
 *
 * Ordering. Every entry point here but sge_render_texture_sample_device synchronises. sge_render_texture_sample_device is enqueued on
 * the context's stream.
 */
#ifndef SGE_AMD_RENDER_TEXTURES_H
#define SGE_AMD_RENDER_TEXTURES_H

#include "sge_amd_render.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGE_HAS_RENDER_TEXTURES 1

#define SGE_MAX_RENDER_TEXTURES 32 /* MAX_RT_TEXTURES */
#define SGE_TEX_RGBA8_UNORM 0
#define SGE_TEX_RGBA8_UNORM_SRGB 1
#define SGE_MAX_TEXTURE_DIM 8192

/* The texture indices of RTInstanceInfo (ShaderTypes.h:118-124) and normalScale (Material.swift:46: 1), per material. An index
 * that is < 0, >= SGE_MAX_RENDER_TEXTURES, or names an empty slot means no texture. 32 bytes. */
struct sge_render_material_textures {
    int32_t baseColor;         /*  0 */
    int32_t normal;            /*  4 */
    int32_t metallicRoughness; /*  8 */
    int32_t emissive;          /* 12 */
    int32_t occlusion;         /* 16 */
    float normalScale;         /* 20 */
    int32_t pad[2];            /* 24 */
};

/* texture.replace: rgba[height][width][4] bytes, rows tightly packed, row 0 first. slot 0 .. SGE_MAX_RENDER_TEXTURES - 1, each
 * dimension 1 .. SGE_MAX_TEXTURE_DIM. A bad slot, dimension or format, or a NULL pointer, gives SGE_ERR_INVALID and changes
 * nothing. Uploading a slot again replaces it. Synchronises. */
int sge_render_texture_upload(sge_context* ctx, int32_t slot, int32_t width, int32_t height, int32_t format, const uint8_t* rgba);

/* Empties a slot; slot = -1: every slot. Any other slot outside 0 .. SGE_MAX_RENDER_TEXTURES - 1 gives SGE_ERR_INVALID. */
int sge_render_texture_clear(sge_context* ctx, int32_t slot);

/* Binds entries [0, count) of the material table, 1 <= count <= SGE_MAX_RENDER_MATERIALS; every other material returns to
 * {-1, -1, -1, -1, -1, 1.0}, which is also the state of a fresh context. sge_render_materials_set leaves the bindings alone.
 * A non-finite normalScale gives SGE_ERR_INVALID and changes nothing. */
int sge_render_material_textures_set(sge_context* ctx, int32_t count, const struct sge_render_material_textures* table);

/* Width, height and format of a slot; all three 0 for an empty slot. */
int sge_render_texture_info_get(sge_context* ctx, int32_t slot, int32_t* width, int32_t* height, int32_t* format);

/* The sRGB decode table the kernels use (see the pinned sampler). */
int sge_render_srgb_table_get(sge_context* ctx, float table[256]);

/* The sampler alone: rgba[count][4] = the texture of `slot` at uvs[count][2], through the device function the frame kernels
 * call, in a kernel of its own. count >= 0. An empty slot gives SGE_ERR_STATE. Synchronises. */
int sge_render_texture_sample_batch(sge_context* ctx, int32_t slot, const float* uvs, int32_t count, float* rgba);

/* The same over device memory; enqueued on the context's stream. */
int sge_render_texture_sample_device(sge_context* ctx, int32_t slot, const void* d_uvs, int32_t count, void* d_rgba);

#ifdef __cplusplus
}
#endif

#endif /* SGE_AMD_RENDER_TEXTURES_H */
