// The ray scene for gfx950 (include/sge_amd_ray_scene.h): what RTAccelerationBuilder.build puts under its instance structure
// beside the skinned characters — cachedStaticBLAS, one primitive structure per static slice, built once
// (RTAccelerationBuilder.swift:37-71) and instanced with item.modelMatrix (:168-185) — and the two questions raytraceKernel asks
// of the whole: the closest hit with the reads at the hit (RayTracing.metalinc:242-300) and the shadow ray's "is anything
// between min_distance and max_distance" (:334-343).
//
// Data. A device table of static meshes (DevSceneMesh: the 64-wide tree of HostBlas::build, entry boxes computed once on the
// host, the mesh's streams), per static instance a mesh id and a matrix, one world box per instance and one per 64 consecutive
// instances in index order — the flat form the crowd keeps as SGE_BLAS_FLAT_INSTANCES: a ray scans ceil(S / 4096) steps of
// group boxes. A scene has a handful to a few thousand static instances (the limit is 2^18); no grid order is needed.
//
// scene_trace_kernel — one wavefront per ray, plain launch, every loop bounded by a count read before it starts. The static
// half first (group scan, then blasTraverseClosest per instance the ray may hit), then the crowd half exactly as
// blas_intersect_kernel walks it (the same device functions, sge_blas_trace_dev.hpp), with the best hit carried across the halves.
// The key is (distance bits, scene id, primitive id): a static instance's id is SGE_SCENE_STATIC_BASE + s, above every character's,
// so at equal distance a character takes the hit from a static instance whichever half found it first.
//
// scene_occlusion_kernel — the same scans with early outs: boxes are tested against maxDistance (no shrinking bound), the
// wavefront stops at the first cluster that reports a triangle in range (decided from a ballot: wave-uniform), no key
// reduction, no barycentrics, no epilogue; one int32 per ray.
#include "sge_ray_scene_dev.hpp"

namespace sge {

// The world box of the eight transformed corners of every instance's root row, and one box per 64 consecutive instances.
// One wavefront per group of 64 instances.
__global__ __launch_bounds__(kWave) void scene_instance_boxes_kernel(SceneTrace S, int firstGroup) {
    const int g = firstGroup + blockIdx.x, i = g * kWave + threadIdx.x;
    F3 mn{kFloatMax, kFloatMax, kFloatMax}, mx{-kFloatMax, -kFloatMax, -kFloatMax};
    if (i < S.statics) {
        const Aff M = loadInstance(S.matrices, i);
        const DevSceneMesh& m = S.meshes[S.meshOf[i]];
        const float* bx = m.boxes + (size_t)m.entryCount * 6;
        for (int k = 0; k < 8; ++k) {
            const F3 c = affMulPoint(M, F3{bx[(k & 1) ? 3 : 0], bx[(k & 2) ? 4 : 1], bx[(k & 4) ? 5 : 2]});
            mn = vmin(mn, c);
            mx = vmax(mx, c);
        }
        float* o = S.boxes + (size_t)i * 6;
        o[0] = mn.x; o[1] = mn.y; o[2] = mn.z; o[3] = mx.x; o[4] = mx.y; o[5] = mx.z;
    }
    for (int off = 32; off > 0; off >>= 1) {
        mn = vmin(mn, F3{__shfl_xor(mn.x, off, kWave), __shfl_xor(mn.y, off, kWave), __shfl_xor(mn.z, off, kWave)});
        mx = vmax(mx, F3{__shfl_xor(mx.x, off, kWave), __shfl_xor(mx.y, off, kWave), __shfl_xor(mx.z, off, kWave)});
    }
    if (threadIdx.x == 0) {
        float* o = S.boxes + ((size_t)S.statics + g) * 6;
        o[0] = mn.x; o[1] = mn.y; o[2] = mn.z; o[3] = mx.x; o[4] = mx.y; o[5] = mx.z;
    }
}

// STRIDE: floats per vertex of the crowd's skinned positions and normals (the static meshes' streams are packed). The bodies are
// texts shared with the kernels for a crowd with mesh variants (sge_scene_variants.hip), here over a crowd that shares one mesh.
template <int STRIDE>
__global__ __launch_bounds__(kWave) void scene_trace_kernel(SceneTrace S, const sge_blas_ray* rays, int n, sge_blas_hit* hits) {
    const UniformCrowd<STRIDE> C{S.T};
#include "sge_scene_trace_body.inc"
}

template <int STRIDE>
__global__ __launch_bounds__(kWave) void scene_occlusion_kernel(SceneTrace S, const sge_blas_ray* rays, int n, int32_t* occluded) {
    const UniformCrowd<STRIDE> C{S.T};
#include "sge_scene_occlusion_body.inc"
}

void launch_scene_instance_boxes(const SceneTrace& S, int firstGroup, int groups, hipStream_t s) {
    if (groups > 0) hipLaunchKernelGGL(scene_instance_boxes_kernel, dim3(groups), dim3(kWave), 0, s, S, firstGroup);
}

void launch_scene_trace(const SceneTrace& S, const sge_blas_ray* d_rays, int n, sge_blas_hit* d_hits, hipStream_t s) {
    if (n <= 0) return;
    if (S.crowd && S.T.layout == SGE_LAYOUT_PADDED16) hipLaunchKernelGGL((scene_trace_kernel<4>), dim3(n), dim3(kWave), 0, s, S, d_rays, n, d_hits);
    else hipLaunchKernelGGL((scene_trace_kernel<3>), dim3(n), dim3(kWave), 0, s, S, d_rays, n, d_hits);
}

void launch_scene_occlusion(const SceneTrace& S, const sge_blas_ray* d_rays, int n, int32_t* d_occluded, hipStream_t s) {
    if (n <= 0) return;
    if (S.crowd && S.T.layout == SGE_LAYOUT_PADDED16) hipLaunchKernelGGL((scene_occlusion_kernel<4>), dim3(n), dim3(kWave), 0, s, S, d_rays, n, d_occluded);
    else hipLaunchKernelGGL((scene_occlusion_kernel<3>), dim3(n), dim3(kWave), 0, s, S, d_rays, n, d_occluded);
}

} // namespace sge
