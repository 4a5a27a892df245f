/*
 * sge_amd_render.h — the shaded frame: what raytraceKernel does between its queries (RayTracing.metalinc:197-730).
 *
 * An addition to sge_amd_ray_scene.h (same conventions, same library, SGE_ABI_VERSION stays 2). The ray scene answers the two
 * questions raytraceKernel asks of its acceleration structure; this header adds the kernel around them: the camera ray per pixel
 * (:225-235), up to three alpha-composited layers (:237-241, :715-721), per-instance PBR factors (sample_material, :132-176),
 * directional lights with a shadow ray that walks through up to four translucent occluders (:322-376), SH ambient (:65-86, :378),
 * the one-bounce mirror (:382-542) and refraction (:544-713) paths, the dither and the image write (:724-729). One launch per frame;
 * the pixel's chain of queries stays on the device.
 *
 * Two omissions.
 *  1. No textures in this header. On its own the kernel behaves as the reference does with frame.textureCount == 0: every
 *     `...TexIndex < textureCount` test is false, so a material is its factors (:143-150) and the shading normal N is the
 *     geometric normal (:267-268). sge_amd_render_textures.h adds the texture slots, the per-material texture indices and the
 *     sampling sites of the text; while no material binds a slot that holds a texture, the frame is the one described here.
 *  2. No specular IBL in this header. On its own eval_spec_ibl (:88-104, :379) contributes 0. sge_amd_render_ibl.h adds the
 *     environment cube, the BRDF table, their pinned samplers and the term; while either resource is missing, the frame is the
 *     one described here.
 * Everything else is the text: maxLayers = 3 with the accumAlpha < 0.99 cut; shadow_bias; every enabled light, skipped when
 * camDist > maxDist or NdotL <= 0 (maxDistance <= 0 means 1e6); the shadow walk for light 0 only on the primary and mirror paths
 * but for every light on the refraction path (:654-689; the asymmetry is the reference's) — at most 4 occluders while shadow > 0.02,
 * shadow *= 1 - alpha of the occluder's material, origin advanced by L * bias * 2, min_distance 0.001 afterwards; eval_brdf and the
 * 9-term eval_env_sh; color = direct + ambient + emissive; the mirror path when roughness <= 0.08 && metallic >= 0.8 (after
 * sample_material's clamp of roughness to [0.05, 1]), one bounce with its own shading, the miss colour (0.02, 0.02, 0.03) *
 * (1 - reflAlpha), the Fresnel mix; the refraction path when transmission > 0.001, the eta and normal flip, length(T) > 0, the SH
 * background, the final two mixes; compositing, the advance by direction * (bias * 2), the background, the hash12_rt dither of
 * amplitude 1/255, max(., 0), alpha 1. (The `triBase` guard of :248-251 is vacuous here: a hit names a triangle of its mesh.)
 *
 * A query is the whole-scene closest hit of sge_scene_intersect_*: tMin = max(min_distance, 0), the (distance bits, scene id,
 * primitive id) key, the same hit record. The record's geomNormal is normalize(cross(w1 - w0, w2 - w0)) of the three world
 * vertices, negated when its dot with the ray direction is > 0 — the face-forwarded N of :263-268, computed by the expressions
 * of sge_scene_intersect_* (there normalize(v) = v * (1 / sqrt(dot(v, v)))); the kernel uses it as N.
 *
 * Pinned float32 forms. Everything that decides a ray is float32 with no contraction, IEEE sqrt and /, in this order: dot(a, b) =
 * (a.x * b.x + a.y * b.y) + a.z * b.z; normalize(v) = v / sqrt(dot(v, v)); M * v = ((c0 * v.x + c1 * v.y) + c2 * v.z) + c3 * v.w,
 * columns 0 to 3; reflect(I, N) = I - (2 * dot(N, I)) * N; refract(I, N, eta): d = dot(N, I), k = 1 - (eta * eta) * (1 - d * d),
 * 0 when k < 0, else eta * I - (eta * d + sqrt(k)) * N; step(e, x) = x < e ? 0 : 1; fract(x) = x - floor(x). The camera ray:
 * pixel = (gid + 0.5) / size, ndc = (pixel.x * 2 - 1, (1 - pixel.y) * 2 - 1), world = invViewProj * (ndc, 1, 1), direction =
 * normalize(world.xyz / world.w - cameraPosition), origin cameraPosition, min_distance 0.001, max_distance 1e6. hitPos = origin +
 * direction * distance; bias = max(0.002, distance * 0.002); a shadow, mirror ray starts at hitPos + N * bias, a refraction ray at
 * hitPos + T * bias, each with min_distance = bias * 0.5; L = normalize(-light.direction); an occluder advances the shadow ray to
 * ((origin + L * distance) + (L * bias) * 2); a layer advances the ray to hitPos + direction * (bias * 2). V = normalize(-direction).
 *
 * Materials. Material 0 is Material.swift:37-44's defaults until sge_render_materials_set replaces the table. Every static
 * instance and every character names a material; sge_scene_instances_set resets every static instance to material 0, and so
 * does sge_characters_resize with another count for the characters. Both are observed by the next sge_render_* call, through the
 * count and the identity of the list: an assignment made for a list that has been replaced is dropped there for good, so a later
 * list of the same length starts from material 0 again. (Two sge_scene_instances_set calls with no sge_render_* call between them
 * are one replacement.)
 *
 * The crowd is optional, exactly as in sge_amd_ray_scene.h: with crowdReady == 0 the frame shows the statics only. A crowd with
 * mesh variants is in the frame once every variant has its structure (sge_amd_variant_scene.h).
 *
 * Ordering. sge_render_frame_batch synchronises. sge_render_frame_device is enqueued on the context's stream with exactly the
 * contract of sge_scene_intersect_device: behind the skin and refit launches of the newest sge_tick under every
 * SGE_OPT_OVERLAP_SKIN mode, behind earlier sge_scene_instances_update calls, and it refreshes the crowd's world boxes itself.
 * The sge_render_*_set / *_materials entry points synchronise.
 */
#ifndef SGE_AMD_RENDER_H
#define SGE_AMD_RENDER_H

#include "sge_amd_ray_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGE_HAS_RENDER 1

#define SGE_MAX_RENDER_MATERIALS 256
#define SGE_MAX_DIR_LIGHTS 8
#define SGE_MAX_RENDER_PIXELS 67108864 /* width * height <= 2^26 */

/* RTInstanceInfo's factors (ShaderTypes.h:111-117), defaults of Material.swift:37-44. 48 bytes. */
struct sge_render_material {
    float baseColor[3];      /*  0: baseColorFactor (1, 1, 1) */
    float metallic;          /* 12: metallicFactor 0 */
    float emissive[3];       /* 16: emissiveFactor (0, 0, 0) */
    float occlusionStrength; /* 28: 1 */
    float roughness;         /* 32: mrFactors.x 0.5 */
    float alpha;             /* 36: mrFactors.y 1 */
    float transmission;      /* 40: transmissionFactor 0 */
    float ior;               /* 44: 1.5 */
};

/* RTDirectionalLight (ShaderTypes.h:128-136; RayTracingRenderer.swift:153-180 fills it). 48 bytes. */
struct sge_render_light {
    float direction[3]; /*  0: the direction the light travels; L = normalize(-direction) */
    float intensity;    /* 12 */
    float color[3];     /* 16 */
    float enabled;      /* 28: < 0.5 = skipped (RayTracing.metalinc:324) */
    float maxDistance;  /* 32: <= 0 means 1e6 (:325) */
    float pad[3];       /* 36 */
};

/* RTFrameUniforms without the texture and IBL fields (ShaderTypes.h:80-102; RayTracingRenderer.swift:76-97). 204 bytes. */
struct sge_render_frame {
    float invViewProj[16];    /*   0: column-major (RayTracingRenderer.swift:66-67) */
    float cameraPosition[3];  /*  64 */
    float ambientIntensity;   /*  76 */
    int32_t width;            /*  80: imageSize.x */
    int32_t height;           /*  84: imageSize.y */
    int32_t dirLightCount;    /*  88: <= the count of sge_render_lights_set */
    int32_t flags;            /*  92: must be 0 */
    float envSH[9][3];        /*  96: envSH0 .. envSH8 */
};

/* What the kernel knows about a pixel besides its colour. 32 bytes, one per pixel. */
struct sge_render_aov {
    int32_t layers;    /*  0: layers composited (0 .. 3) */
    int32_t instance;  /*  4: the first layer's hit: scene id as in sge_amd_ray_scene.h, -1 on a miss */
    int32_t primitive; /*  8: -1 on a miss */
    float distance;    /* 12: 0 on a miss */
    float shadow;      /* 16: the light-0 shadow factor of the first layer; 1 where no shadow ray was shot */
    float alpha;       /* 20: the final accumAlpha */
    int32_t queries;   /* 24: closest-hit queries the pixel issued in total */
    int32_t flags;     /* 28: bit 0: the first layer took the mirror path; bit 1: it took the refraction path */
};

/* Replaces the whole material table: materials[count], 1 <= count <= SGE_MAX_RENDER_MATERIALS. A non-finite field, and a count
 * at or below a material index that a static instance or a character still names, give SGE_ERR_INVALID and change nothing. */
int sge_render_materials_set(sge_context* ctx, int32_t count, const struct sge_render_material* materials);

/* material_of_instance[count] for the static instances; count must equal the static instance count and every index must be
 * inside the material table, else SGE_ERR_INVALID and nothing changes. */
int sge_render_static_materials(sge_context* ctx, int32_t count, const int32_t* material_of_instance);

/* material_of_character[count]; count must equal sge_characters_resize's count. Characters never assigned use material 0. */
int sge_render_crowd_materials(sge_context* ctx, int32_t count, const int32_t* material_of_character);

/* dirLights (RayTracingRenderer.swift:153-180): lights[count], 0 <= count <= SGE_MAX_DIR_LIGHTS. A non-finite field gives
 * SGE_ERR_INVALID. */
int sge_render_lights_set(sge_context* ctx, int32_t count, const struct sge_render_light* lights);

/* raytraceKernel over the scene (RayTracingRenderer.swift:111-151, :182-188 dispatch it): host float rgba[height][width][4]; aov
 * [height][width] or NULL. A frame with a non-finite entry, width or height < 1, width * height > SGE_MAX_RENDER_PIXELS, or
 * dirLightCount above the uploaded count, or flags != 0 gives SGE_ERR_INVALID and leaves the outputs untouched. Synchronises. */
int sge_render_frame_batch(sge_context* ctx, const struct sge_render_frame* frame, float* rgba, struct sge_render_aov* aov);

/* The same into device memory (d_aov may be NULL); enqueued (see Ordering). The frame is read before the call returns. */
int sge_render_frame_device(sge_context* ctx, const struct sge_render_frame* frame, void* d_rgba, void* d_aov);

#ifdef __cplusplus
}
#endif

#endif /* SGE_AMD_RENDER_H */
