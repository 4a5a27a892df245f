// The ray scene and the shaded frame over a crowd with mesh variants (include/sge_amd_variant_scene.h): the three whole-scene
// kernels of sge_ray_scene.hip and sge_render.hip with the crowd half taken per character, as blas_intersect_ragged_kernel takes
// it (sge_blas_variants.hip).
//
// Nothing of the walk is restated here. The bodies are the texts sge_scene_trace_body.inc, sge_scene_occlusion_body.inc and
// sge_render_frame_body.inc, included inside the uniform kernels and inside these, with RaggedCrowd (sge_ray_scene_dev.hpp) as the
// crowd half's accessor: when the wavefront enters a character it loads the record the newest refit left for it (one byte; 0xFF:
// the character is left at once), that variant's row of the device table (topology and, at a hit, index buffer and uvs) and the
// character's first vertex off[c]; its boxes are row c * rowStride of the box table. All of it is wave-uniform and is dropped when
// the character is left: the instance scan holds what it holds in the uniform kernels. The instance level is the one
// buildInstanceLevel builds for a RaggedTrace: a character without a structure has a NaN world box, which no slab test passes and
// no group box takes up.
//
// Kernels of their own, not template arguments of the uniform ones, and texts, not functions that take the launch record: the
// uniform kernels' machine code is what it was before these existed (checked by a disassembly diff; as functions they differed).
//
// Built with -ffp-contract=off, as the uniform kernels are: a frame over variants that hold the same mesh is the uniform frame bit
// for bit.
#include "sge_render_dev.hpp"

namespace sge {

template <int STRIDE>
__global__ __launch_bounds__(kWave) void scene_ragged_trace_kernel(SceneTrace S, SceneRagged G, const sge_blas_ray* rays, int n, sge_blas_hit* hits) {
    const RaggedCrowd<STRIDE> C{S.T, G};
#include "sge_scene_trace_body.inc"
}

template <int STRIDE>
__global__ __launch_bounds__(kWave) void scene_ragged_occlusion_kernel(SceneTrace S, SceneRagged G, const sge_blas_ray* rays, int n, int32_t* occluded) {
    const RaggedCrowd<STRIDE> C{S.T, G};
#include "sge_scene_occlusion_body.inc"
}

// (the ragged record is read from device memory where a character is entered, like the two records in front of it)
template <int STRIDE>
__global__ __launch_bounds__(kWave) void render_ragged_frame_kernel(const RenderArgs* A) {
    const RaggedCrowd<STRIDE> C{A->S.T, A->G};
    constexpr bool TEX = STRIDE == 0; // false (a constant that depends on STRIDE: see the body)
    constexpr bool IBL = STRIDE == 0; // false
#include "sge_render_frame_body.inc"
}

// the textured form (include/sge_amd_render_textures.h; see sge_render.hip)
template <int STRIDE>
__global__ __launch_bounds__(kWave) void render_ragged_textured_kernel(const RenderArgs* A) {
    const RaggedCrowd<STRIDE> C{A->S.T, A->G};
    constexpr bool TEX = STRIDE != 0; // true
    constexpr bool IBL = STRIDE == 0; // false
#include "sge_render_frame_body.inc"
}

// the forms with specular IBL (include/sge_amd_render_ibl.h; see sge_render.hip)
template <int STRIDE>
__global__ __launch_bounds__(kWave) void render_ragged_ibl_kernel(const RenderArgs* A) {
    const RaggedCrowd<STRIDE> C{A->S.T, A->G};
    constexpr bool TEX = STRIDE == 0; // false
    constexpr bool IBL = STRIDE != 0; // true
#include "sge_render_frame_body.inc"
}

template <int STRIDE>
__global__ __launch_bounds__(kWave) void render_ragged_ibl_tex_kernel(const RenderArgs* A) {
    const RaggedCrowd<STRIDE> C{A->S.T, A->G};
    constexpr bool TEX = STRIDE != 0; // true
    constexpr bool IBL = STRIDE != 0; // true
#include "sge_render_frame_body.inc"
}

void launch_scene_trace_ragged(const SceneTrace& S, const SceneRagged& G, const sge_blas_ray* d_rays, int n, sge_blas_hit* d_hits, hipStream_t s) {
    if (n <= 0) return;
    if (S.T.layout == SGE_LAYOUT_PADDED16) hipLaunchKernelGGL((scene_ragged_trace_kernel<4>), dim3(n), dim3(kWave), 0, s, S, G, d_rays, n, d_hits);
    else hipLaunchKernelGGL((scene_ragged_trace_kernel<3>), dim3(n), dim3(kWave), 0, s, S, G, d_rays, n, d_hits);
}

void launch_scene_occlusion_ragged(const SceneTrace& S, const SceneRagged& G, const sge_blas_ray* d_rays, int n, int32_t* d_occluded, hipStream_t s) {
    if (n <= 0) return;
    if (S.T.layout == SGE_LAYOUT_PADDED16) hipLaunchKernelGGL((scene_ragged_occlusion_kernel<4>), dim3(n), dim3(kWave), 0, s, S, G, d_rays, n, d_occluded);
    else hipLaunchKernelGGL((scene_ragged_occlusion_kernel<3>), dim3(n), dim3(kWave), 0, s, S, G, d_rays, n, d_occluded);
}

void launch_render_frame_ragged(const RenderArgs& host, const RenderArgs* d_args, hipStream_t s) {
    const int n = host.R.frame.width * host.R.frame.height;
    if (n <= 0) return;
    if (host.S.T.layout == SGE_LAYOUT_PADDED16) hipLaunchKernelGGL((render_ragged_frame_kernel<4>), dim3(n), dim3(kWave), 0, s, d_args);
    else hipLaunchKernelGGL((render_ragged_frame_kernel<3>), dim3(n), dim3(kWave), 0, s, d_args);
}

void launch_render_frame_ragged_textured(const RenderArgs& host, const RenderArgs* d_args, hipStream_t s) {
    const int n = host.R.frame.width * host.R.frame.height;
    if (n <= 0) return;
    if (host.S.T.layout == SGE_LAYOUT_PADDED16) hipLaunchKernelGGL((render_ragged_textured_kernel<4>), dim3(n), dim3(kWave), 0, s, d_args);
    else hipLaunchKernelGGL((render_ragged_textured_kernel<3>), dim3(n), dim3(kWave), 0, s, d_args);
}

void launch_render_frame_ragged_ibl(const RenderArgs& host, const RenderArgs* d_args, bool textured, hipStream_t s) {
    const int n = host.R.frame.width * host.R.frame.height;
    if (n <= 0) return;
    const bool padded = host.S.T.layout == SGE_LAYOUT_PADDED16;
    if (textured) {
        if (padded) hipLaunchKernelGGL((render_ragged_ibl_tex_kernel<4>), dim3(n), dim3(kWave), 0, s, d_args);
        else hipLaunchKernelGGL((render_ragged_ibl_tex_kernel<3>), dim3(n), dim3(kWave), 0, s, d_args);
    } else {
        if (padded) hipLaunchKernelGGL((render_ragged_ibl_kernel<4>), dim3(n), dim3(kWave), 0, s, d_args);
        else hipLaunchKernelGGL((render_ragged_ibl_kernel<3>), dim3(n), dim3(kWave), 0, s, d_args);
    }
}

} // namespace sge
