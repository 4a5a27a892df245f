// The shaded frame for gfx950 (include/sge_amd_render.h): raytraceKernel (RayTracing.metalinc:197-730) over the ray scene, with
// frame.textureCount == 0 and without specular IBL; and its textured form (include/sge_amd_render_textures.h).
//
// render_frame_kernel — one wavefront per pixel, plain launch, the LDS traversal stack and the closest-hit walk of
// scene_trace_kernel (sge_ray_scene_dev.hpp, sge_blas_trace_dev.hpp). The reference inlines its intersector at seven call sites
// (the layer's ray, its shadow walk, the mirror ray and its shadow walk, the refraction ray and its shadow walks). Here the pixel
// is a small state machine around ONE closest-hit scan per half of the scene: every pass of the loop issues the pending query
// (qo, qd, qmin, qmax), then advances the state — `mode` says whether the query was a surface ray or a step of a shadow walk,
// `phase` which surface is being shaded (0: the layer's own, 1: the mirror bounce, 2: the refraction bounce) — until the next
// query is set up or the pixel is done. The sections behind the scan run at most once per pass and each exists once in the
// code: the shadow step, the surface set-up, the light loop (eval_brdf), the surface's colour, the end of a bounce (the two
// mixes), the refraction set-up, the compositing. Shading is wave-uniform: the winner of the scan is made scalar
// (readfirstlane), every lane computes the same colour, lane 0 writes it.
//
// Every loop is bounded by a count read before it starts: a pixel issues at most 3 * (1 + 4 + 1 + 4 + 1 + 4 * lights) queries
// (three layers; the layer's ray and light 0's walk, the same for the mirror bounce, the refraction ray and a walk per light),
// the light loop runs at most lights + 1 times per pass.
//
// Textures. render_textured_kernel is the same text with TEX = true (sge_render_frame_body.inc): at a surface it takes the hit
// record's uv and shading frame (blasHitRecord, wave-uniformly: the winner's barycentrics are made scalar too), runs
// sample_material and the normal map through texSample (sge_render_dev.hpp) and keeps the sampled surface, 48 bytes, in the
// pixel's LDS state for the light loop, the mirror test, the mixes and the compositing; an occluder of a shadow walk gets
// sample_alpha. All 64 lanes hold the same surface, so every texel address is wave-uniform: four loads per sample, no lanes
// spread over taps. The host launches it only when a bound slot holds a texture; render_frame_kernel is untouched by it (its
// own kernel, its own name: the register figures of the untextured frame are what they were).
//
// Specular IBL (include/sge_amd_render_ibl.h). render_ibl_kernel and render_ibl_tex_kernel are the two texts above with IBL = true:
// when the layer's own surface is done (phase 0, the surfaceDone section) they add eval_spec_ibl. R, the roughness and NoV are the
// same in every lane and are made scalar, so the taps (8 of the cube over two levels, each possibly reprojected across an edge,
// 4 of the table) are scalar loads of packed halves / floats. The host launches them only when both the cube and the table are
// present; the four older kernels are untouched (IBL = false discards the arm unseen).
//
// Built with -ffp-contract=off: what decides a ray is the float32 expression the header pins, as written.
#include "sge_render_dev.hpp"

namespace sge {

// STRIDE: floats per vertex of the crowd's skinned positions. The body is a text shared with render_ragged_frame_kernel
// (sge_scene_variants.hip), here over a crowd that shares one mesh.
template <int STRIDE>
__global__ __launch_bounds__(kWave) void render_frame_kernel(const RenderArgs* A) {
    const UniformCrowd<STRIDE> C{A->S.T};
    constexpr bool TEX = STRIDE == 0; // false (a constant that depends on STRIDE: see the body)
    constexpr bool IBL = STRIDE == 0; // false
#include "sge_render_frame_body.inc"
}

template <int STRIDE>
__global__ __launch_bounds__(kWave) void render_textured_kernel(const RenderArgs* A) {
    const UniformCrowd<STRIDE> C{A->S.T};
    constexpr bool TEX = STRIDE != 0; // true
    constexpr bool IBL = STRIDE == 0; // false
#include "sge_render_frame_body.inc"
}

// the forms with specular IBL (include/sge_amd_render_ibl.h): the same text again, eval_spec_ibl at the layer's surface
template <int STRIDE>
__global__ __launch_bounds__(kWave) void render_ibl_kernel(const RenderArgs* A) {
    const UniformCrowd<STRIDE> C{A->S.T};
    constexpr bool TEX = STRIDE == 0; // false
    constexpr bool IBL = STRIDE != 0; // true
#include "sge_render_frame_body.inc"
}

template <int STRIDE>
__global__ __launch_bounds__(kWave) void render_ibl_tex_kernel(const RenderArgs* A) {
    const UniformCrowd<STRIDE> C{A->S.T};
    constexpr bool TEX = STRIDE != 0; // true
    constexpr bool IBL = STRIDE != 0; // true
#include "sge_render_frame_body.inc"
}

// the IBL samplers alone (sge_render_env_sample_*, sge_render_brdf_lut_sample_*): one thread per sample through the frame kernels'
// envSample and brdfLutSample. dirs null: the table at uvs[n][2] -> out[n][2]; else the cube at dirs[n][3], lods[n] -> out[n][3].
__global__ __launch_bounds__(256) void ibl_sample_kernel(const RenderIBL* I, const float* dirs, const float* lods, const float* uvs, int n, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (dirs) {
        const F3 c = envSample(*I, arr3(dirs + (size_t)i * 3), lods[i]);
        float* o = out + (size_t)i * 3;
        o[0] = c.x; o[1] = c.y; o[2] = c.z;
    } else {
        float c[2];
        brdfLutSample(*I, uvs[(size_t)i * 2], uvs[(size_t)i * 2 + 1], c);
        out[(size_t)i * 2] = c[0]; out[(size_t)i * 2 + 1] = c[1];
    }
}

// the sampler alone (sge_render_texture_sample_*): one thread per sample through the frame kernels' texSample
__global__ __launch_bounds__(256) void texture_sample_kernel(DevRenderTexture tex, const float* srgb, const float* uvs, int n, float* rgba) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float c[4];
    texSample(tex, srgb, uvs[(size_t)i * 2], uvs[(size_t)i * 2 + 1], c);
    float* o = rgba + (size_t)i * 4;
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = c[3];
}

void launch_render_frame(const RenderArgs& host, const RenderArgs* d_args, hipStream_t s) {
    const int n = host.R.frame.width * host.R.frame.height;
    if (n <= 0) return;
    if (host.S.crowd && host.S.T.layout == SGE_LAYOUT_PADDED16) hipLaunchKernelGGL((render_frame_kernel<4>), dim3(n), dim3(kWave), 0, s, d_args);
    else hipLaunchKernelGGL((render_frame_kernel<3>), dim3(n), dim3(kWave), 0, s, d_args);
}

void launch_render_frame_textured(const RenderArgs& host, const RenderArgs* d_args, hipStream_t s) {
    const int n = host.R.frame.width * host.R.frame.height;
    if (n <= 0) return;
    if (host.S.crowd && host.S.T.layout == SGE_LAYOUT_PADDED16) hipLaunchKernelGGL((render_textured_kernel<4>), dim3(n), dim3(kWave), 0, s, d_args);
    else hipLaunchKernelGGL((render_textured_kernel<3>), dim3(n), dim3(kWave), 0, s, d_args);
}

void launch_render_frame_ibl(const RenderArgs& host, const RenderArgs* d_args, bool textured, hipStream_t s) {
    const int n = host.R.frame.width * host.R.frame.height;
    if (n <= 0) return;
    const bool padded = host.S.crowd && host.S.T.layout == SGE_LAYOUT_PADDED16;
    if (textured) {
        if (padded) hipLaunchKernelGGL((render_ibl_tex_kernel<4>), dim3(n), dim3(kWave), 0, s, d_args);
        else hipLaunchKernelGGL((render_ibl_tex_kernel<3>), dim3(n), dim3(kWave), 0, s, d_args);
    } else {
        if (padded) hipLaunchKernelGGL((render_ibl_kernel<4>), dim3(n), dim3(kWave), 0, s, d_args);
        else hipLaunchKernelGGL((render_ibl_kernel<3>), dim3(n), dim3(kWave), 0, s, d_args);
    }
}

// (d_ibl: the device copy of the record the frame kernels read through RenderArgs)
void launch_env_sample(const RenderIBL* d_ibl, const float* d_dirs, const float* d_lods, int n, float* d_rgb, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(ibl_sample_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_ibl, d_dirs, d_lods, (const float*)nullptr, n, d_rgb);
}

void launch_brdf_lut_sample(const RenderIBL* d_ibl, const float* d_uvs, int n, float* d_out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(ibl_sample_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_ibl, (const float*)nullptr, (const float*)nullptr, d_uvs, n, d_out);
}

void launch_texture_sample(const DevRenderTexture& tex, const float* srgb, const float* d_uvs, int n, float* d_rgba, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(texture_sample_kernel, dim3((n + 255) / 256), dim3(256), 0, s, tex, srgb, d_uvs, n, d_rgba);
}

} // namespace sge
