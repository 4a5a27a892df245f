/*
 * sge_amd_render_ibl.h — specular IBL in the shaded frame: IBLResources (Game/IBLResources.swift, whole file) and eval_spec_ibl of
 * raytraceKernel (RayTracing.metalinc:88-104, bound at :199-200, applied at :378-380; RayTracingRenderer.swift:86 sets
 * frame.envMipCount from the cube, :141 binds brdfLUT).
 *
 * An addition to sge_amd_render.h and sge_amd_render_textures.h (same conventions, same library, SGE_ABI_VERSION stays 2). Those
 * headers' frame has eval_spec_ibl contribute 0; this one adds the environment cube (rgba16Float, mip-mapped), the BRDF table
 * (rgba32Float) and the term. CDNA has no sampler to lean on: both filters are HIP functions over plain global loads, pinned below
 * in float32 so that they can be held bit for bit to a restatement.
 *
 * When specular IBL is active: when both the cube and the table are present. sge_render_frame and sge_render_frame_device are
 * unchanged, `flags` stays 0, envMipCount is the uploaded cube's. While either is missing every frame is the frame of the two
 * older headers, byte for byte (the same kernels run).
 *
 * eval_spec_ibl (:88-104), float32, no contraction, every expression evaluated as written, left to right:
 *   NoV = sat(dot(N, V)); R = reflect(-V, N) with the reflect of sge_amd_render.h, I - (2 * dot(N, I)) * N;
 *   mip = roughness * fmaxf((float)(mipCount - 1), 0); prefiltered = envMap.sample(samp, R, level(mip)).xyz;
 *   brdf = brdfLUT.sample(samp, (NoV, roughness)).xy; F0 = 0.04 + (base - 0.04) * metallic per channel, as evalBrdf has it;
 *   spec = prefiltered * (F0 * brdf.x + brdf.y).
 *   It applies at the layer's own surface only (:379); the bounce surfaces (:525-530, :694-699) have no such term.
 *   color = ((direct + ambient) + spec * occlusion) + emissive (:380).
 *   N, V, base, metallic, roughness and occlusion are the sampled surface's when textures are bound: the normal-mapped N and
 *   the values after sample_material.
 *
 * The table sample, brdfLUT.sample(samp, (u, v)): exactly the coordinate and filter expressions of the pinned sampler of
 * sge_amd_render_textures.h (clamp-to-edge, level 0) over the float texels; there is no decode step. x and y are read.
 *
 * The cube sample, envMap.sample(samp, R, level(mip)):
 *   Level: mip = fminf(fmaxf(mip, 0), (float)(mipCount - 1)); l0 = (int)floorf(mip); l1 = min(l0 + 1, mipCount - 1);
 *   fl = mip - (float)l0; out = c0 * (1 - fl) + c1 * fl with cK the bilinear sample of level lK (both are always evaluated).
 *   Face selection, with ax, ay, az the absolute values of the direction: face X when ax >= ay && ax >= az; else face Y when
 *   ay >= az; else face Z. The negative face when the component is < 0. (u, v) is the inverse of cubeDirection
 *   (IBLResources.swift:93-104):
 *     +X (-z, -y) / ax    -X (z, -y) / ax    +Y (x, z) / ay    -Y (x, -z) / ay    +Z (x, -y) / az    -Z (-x, -y) / az
 *   Texel coordinate in a level whose faces are n x n: x = fminf(fmaxf(((u + 1) * 0.5f) * (float)n - 0.5f, -0.5f), (float)n - 0.5f);
 *   x0 = (int)floorf(x); x1 = x0 + 1; fx = x - (float)x0; the same for y with v. The coordinate is not clamped to the face's own
 *   texels: x0 may be -1 and x1 may be n.
 *   Seamless taps: a tap (i, j) outside 0 .. n-1 reads the texel of the same level that holds the direction of the tap's centre:
 *   uc = (2 * ((float)i + 0.5f)) / (float)n - 1, the same for vc; d = cubeDirection(face, uc, vc), not normalised; the face
 *   selection above applied to d gives (face', u', v'); the texel is min(max((int)floorf(((u' + 1) * 0.5f) * (float)n), 0), n - 1)
 *   and the same for v'. (Apple GPUs filter across cube edges; a filter clamped per face would show six flat colours at the
 *   1 x 1 level. The tie rule of the face selection makes corner taps deterministic.)
 *   Filter, on r, g, b (a half converts to float exactly): top = t00 * (1 - fx) + t10 * fx; bot = t01 * (1 - fx) + t11 * fx;
 *   out = top * (1 - fy) + bot * fy.
 *
 * Hostile inputs. No input bits produce a load outside the allocation:
 *   a NaN lod becomes level 0 through fmaxf; a negative lod level 0; a lod above the top, or +inf, level mipCount - 1;
 *   a NaN component of the direction fails every >= of the face selection it enters (the remaining components choose, a direction
 *   of three NaNs is face +Z); a NaN u or v (a NaN component, the zero vector's 0 / 0, inf / inf) becomes the coordinate -0.5
 *   through fmaxf: the taps -1 and 0 with weight 0.5 each, the outside one reprojected as any other; an infinite component
 *   wins its face and the finite ones become u = v = 0, the face's centre; -0 is not < 0: the positive face;
 *   the zero vector is face +X. Reprojected taps are clamped to 0 .. n - 1 and come from a finite, non-zero d.
 *   The table: a NaN coordinate becomes 0, +inf the last texel, -inf 0, as in sge_amd_render_textures.h.
 *
 * The defaults, IBLResources.init in float32 as written (host only, no context): see the two builders below.
 *
 * Ordering. Every entry point here but the two _device forms synchronises; those are enqueued on the context's stream.
 */
#ifndef SGE_AMD_RENDER_IBL_H
#define SGE_AMD_RENDER_IBL_H

#include "sge_amd_render_textures.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SGE_HAS_RENDER_IBL 1

#define SGE_MAX_ENV_SIZE 2048
#define SGE_MAX_ENV_MIPS 12 /* log2(SGE_MAX_ENV_SIZE) + 1 */
#define SGE_MAX_BRDF_LUT_DIM 4096

/* env.replace for every level and slice: the cube in rgba16Float, texels[...][4] halves. size is a power of two,
 * 1 .. SGE_MAX_ENV_SIZE; mipCount is 1 .. log2(size) + 1; level m has faces of max(size >> m, 1) squared. Order: level-major, then
 * face 0..5 = +X, -X, +Y, -Y, +Z, -Z (Metal's slices), rows tightly packed, row 0 first. Bad arguments give SGE_ERR_INVALID and
 * change nothing. Uploading again replaces the cube. Synchronises. */
int sge_render_env_upload(sge_context* ctx, int32_t size, int32_t mipCount, const uint16_t* texels);

/* lut.replace: rgba[height][width][4] floats (rgba32Float), row 0 first. Each dimension 1 .. SGE_MAX_BRDF_LUT_DIM. The kernel
 * reads x and y. Bad arguments give SGE_ERR_INVALID and change nothing. Synchronises. */
int sge_render_brdf_lut_upload(sge_context* ctx, int32_t width, int32_t height, const float* rgba);

/* Returns both to empty: the frame is the frame of the older headers again. */
int sge_render_ibl_clear(sge_context* ctx);

/* The cube's size and mipCount and the table's width and height; zeros for a resource that is empty. */
int sge_render_ibl_info_get(sge_context* ctx, int32_t* size, int32_t* mipCount, int32_t* lutWidth, int32_t* lutHeight);

/* The samplers alone, through the device functions the frame kernels call, in a kernel of their own: rgb[count][3] = the cube at
 * dirs[count][3] and level of detail lods[count]; out[count][2] = the table's x and y at uvs[count][2]. count >= 0. An empty
 * resource gives SGE_ERR_STATE. Synchronise. */
int sge_render_env_sample_batch(sge_context* ctx, const float* dirs, const float* lods, int32_t count, float* rgb);
int sge_render_brdf_lut_sample_batch(sge_context* ctx, const float* uvs, int32_t count, float* out);

/* The same over device memory; enqueued on the context's stream. */
int sge_render_env_sample_device(sge_context* ctx, const void* d_dirs, const void* d_lods, int32_t count, void* d_rgb);
int sge_render_brdf_lut_sample_device(sge_context* ctx, const void* d_uvs, int32_t count, void* d_out);

/* IBLResources.init's cube (IBLResources.swift:16-58, cubeDirection :93-104, sampleEnvColor :106-121) in float32 as written, with
 * normalize(v) = v / sqrtf(dot(v, v)), dot summed left to right, and Float16(x) as round to nearest even. Level m is painted at
 * roughness (float)m / (float)(mipCount - 1), or 0 when mipCount is 1; alpha is 1. texels receives what sge_render_env_upload
 * takes. The arguments are those of sge_render_env_upload; bad ones give SGE_ERR_INVALID. Host only: no context, no device. */
int sge_ibl_default_env_build(int32_t size, int32_t mipCount, uint16_t* texels);

/* IBLResources.init's table (:60-89; integrateBRDF :123-144, hammersley :146-148, radicalInverseVdC :150-158,
 * importanceSampleGGX :160-167, geometrySmith :169-175) in float32 as written: rgba[size][size][4] with z = w = 0; row y is
 * roughness fmaxf((float)y / (float)(size - 1), 0.001f), column x is nDotV by the same expression (at size 1 the quotient is
 * 0 / 0 and fmaxf gives 0.001). size 1 .. SGE_MAX_BRDF_LUT_DIM, sampleCount 1 .. 65536. Host only. */
int sge_ibl_default_brdf_lut_build(int32_t size, int32_t sampleCount, float* rgba);

#ifdef __cplusplus
}
#endif

#endif /* SGE_AMD_RENDER_IBL_H */
