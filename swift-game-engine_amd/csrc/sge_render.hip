// The shaded frame for gfx950 (include/sge_amd_render.h): raytraceKernel (RayTracing.metalinc:197-730) over the ray scene, with
// frame.textureCount == 0 and without specular IBL.
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
// Built with -ffp-contract=off: what decides a ray is the float32 expression the header pins, as written.
#include "sge_render_dev.hpp"

namespace sge {

// STRIDE: floats per vertex of the crowd's skinned positions. The body is a text shared with render_ragged_frame_kernel
// (sge_scene_variants.hip), here over a crowd that shares one mesh.
template <int STRIDE>
__global__ __launch_bounds__(kWave) void render_frame_kernel(const RenderArgs* A) {
    const UniformCrowd<STRIDE> C{A->S.T};
#include "sge_render_frame_body.inc"
}

void launch_render_frame(const RenderArgs& host, const RenderArgs* d_args, hipStream_t s) {
    const int n = host.R.frame.width * host.R.frame.height;
    if (n <= 0) return;
    if (host.S.crowd && host.S.T.layout == SGE_LAYOUT_PADDED16) hipLaunchKernelGGL((render_frame_kernel<4>), dim3(n), dim3(kWave), 0, s, d_args);
    else hipLaunchKernelGGL((render_frame_kernel<3>), dim3(n), dim3(kWave), 0, s, d_args);
}

} // namespace sge
