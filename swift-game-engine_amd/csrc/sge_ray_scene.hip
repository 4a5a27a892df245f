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

// STRIDE: floats per vertex of the crowd's skinned positions and normals (the static meshes' streams are packed)
template <int STRIDE>
__global__ __launch_bounds__(kWave) void scene_trace_kernel(SceneTrace S, const sge_blas_ray* rays, int n, sge_blas_hit* hits) {
    __shared__ int stack[kBlasStack];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= n) return;
    const sge_blas_ray R = rays[blockIdx.x];
    const BlasTrace& T = S.T;
    const F3 wo{R.origin[0], R.origin[1], R.origin[2]}, wd{R.direction[0], R.direction[1], R.direction[2]};
    const float tMin = smax(R.minDistance, 0.0f);
    BlasBest best{R.maxDistance, 0, 0, 0u, -1};

    auto visitStatic = [&](int s) {
        blasTraverseClosest<3, true>(stack, lane, sceneTree(S.meshes[S.meshOf[s]]), loadInstance(S.matrices, s), wo, wd, tMin, R.maxDistance,
                               SGE_SCENE_STATIC_BASE + s, best);
        return false;
    };
    auto visitCharacter = [&](int inst) {
        blasTraverseClosest<STRIDE, true>(stack, lane, crowdTree<STRIDE>(T, inst), loadInstance(T.instances, inst), wo, wd, tMin, R.maxDistance, inst, best);
        return false;
    };

    // a ray names one instance (a scene id) or asks both halves; an id that names nothing enters neither scan
    const F3 inv = invDir(wd);
    const int id = R.instance, sOnly = id >= SGE_SCENE_STATIC_BASE ? id - SGE_SCENE_STATIC_BASE : -1;
    if (S.statics > 0 && (id < 0 || (sOnly >= 0 && sOnly < S.statics)))
        sceneScan(S.boxes, S.boxes + (size_t)S.statics * 6, nullptr, nullptr, S.statics, sOnly, lane, wo, inv, tMin, best.t, visitStatic);
    // (a named character is walked directly: routed through the scan as the statics are, the kernel spilled scalar registers)
    if (S.crowd && id >= 0) {
        if (id < T.chars) visitCharacter(id);
    } else if (S.crowd) {
        const int* order = T.instOrder; // null: the flat form (SGE_BLAS_FLAT_INSTANCES)
        sceneScan(T.worldBoxes, order ? T.groupBoxes : T.worldBoxes + (size_t)T.chars * 6, order ? T.superBoxes : nullptr, order, T.chars, -1, lane,
                  wo, inv, tMin, best.t, visitCharacter);
    }
    if (lane != 0) return;
    sge_blas_hit H{};
    H.primitive = -1;
    H.instance = -1;
    if (best.inst >= SGE_SCENE_STATIC_BASE) {
        const int s = best.inst - SGE_SCENE_STATIC_BASE;
        const DevSceneMesh& m = S.meshes[S.meshOf[s]];
        blasHitRecord<3>(loadInstance(S.matrices, s), m.positions, m.normals, m.tangents, m.uvs, m.indices + (size_t)best.prim * 3, wd, best, H);
        H.instance = best.inst;
    } else if (best.inst >= 0) {
        const size_t vbase = (size_t)best.inst * T.blas.vertexCount;
        blasHitRecord<STRIDE>(loadInstance(T.instances, best.inst), reinterpret_cast<const float*>(T.positions) + vbase * STRIDE,
                              reinterpret_cast<const float*>(T.normals) + vbase * STRIDE, T.tangents + vbase * 4, T.uvs,
                              T.indices + (size_t)best.prim * 3, wd, best, H);
        H.instance = best.inst;
    }
    hits[blockIdx.x] = H;
}

// Is any triangle of one instance hit with tMin <= t <= maxDistance? The walk of blasTraverseClosest without a bound that
// shrinks and without a key: the first cluster with a triangle in range ends it. The result is the same in every lane.
template <int STRIDE>
__device__ __forceinline__ bool sceneOccludedOne(int* stack, int lane, const BlasTreeRef& G, const Aff& M, F3 wo, F3 wd, float tMin, float maxDistance) {
    const Inv3 Mi = inverse3(M);
    const F3 o = mul3(Mi, wo - M.c3), d = mul3(Mi, wd);
    const F3 inv = invDir(d);
    bool any = false;
    int sp = 1;
    if (lane == 0) stack[0] = 0;
    __syncthreads();
    while (sp > 0 && !any) {
        const int w = stack[sp - 1];
        --sp;
        __syncthreads();
        const int first = G.wideFirst[w], cnt = G.wideFirst[w + 1] - first;
        bool pass = false;
        int2 link = make_int2(0, 0);
        if (lane < cnt) {
            link = G.entryLink[first + lane];
            pass = slabPassPadded(G.boxes + (size_t)(first + lane) * 6, o, inv, tMin, maxDistance);
        }
        const unsigned long long inner = __ballot(pass && link.x >= 0), leaves = __ballot(pass && link.x < 0);
        if (pass && link.x >= 0) {
            const int at = sp + __popcll(inner & ((1ull << lane) - 1));
            if (at < kBlasStack) stack[at] = link.x;
        }
        sp = min(sp + __popcll(inner), kBlasStack);
        unsigned long long m = leaves;
        while (m && !any) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int firstSlot = ~__shfl(link.x, src, kWave), count = __shfl(link.y, src, kWave);
            bool hit = false;
            if (lane < count) {
                const uint32_t* ix = G.slotIndices + (size_t)(firstSlot + lane) * 3;
                const F3 p0 = loadP<STRIDE>(G.P, ix[0]), p1 = loadP<STRIDE>(G.P, ix[1]), p2 = loadP<STRIDE>(G.P, ix[2]);
                float t, u, v;
                hit = rayTriangleUV(o, d, p0, p1, p2, 1e-6f, t, u, v) && t >= tMin && t <= maxDistance;
            }
            any = __ballot(hit) != 0;
        }
        __syncthreads();
    }
    return any;
}

template <int STRIDE>
__global__ __launch_bounds__(kWave) void scene_occlusion_kernel(SceneTrace S, const sge_blas_ray* rays, int n, int32_t* occluded) {
    __shared__ int stack[kBlasStack];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= n) return;
    const sge_blas_ray R = rays[blockIdx.x];
    const BlasTrace& T = S.T;
    const F3 wo{R.origin[0], R.origin[1], R.origin[2]}, wd{R.direction[0], R.direction[1], R.direction[2]};
    const float tMin = smax(R.minDistance, 0.0f);
    const float bound = R.maxDistance;

    auto visitStatic = [&](int s) {
        return sceneOccludedOne<3>(stack, lane, sceneTree(S.meshes[S.meshOf[s]]), loadInstance(S.matrices, s), wo, wd, tMin, bound);
    };
    auto visitCharacter = [&](int inst) {
        return sceneOccludedOne<STRIDE>(stack, lane, crowdTree<STRIDE>(T, inst), loadInstance(T.instances, inst), wo, wd, tMin, bound);
    };

    bool occ = false;
    const F3 inv = invDir(wd);
    const int id = R.instance, sOnly = id >= SGE_SCENE_STATIC_BASE ? id - SGE_SCENE_STATIC_BASE : -1;
    if (S.statics > 0 && (id < 0 || (sOnly >= 0 && sOnly < S.statics)))
        occ = sceneScan(S.boxes, S.boxes + (size_t)S.statics * 6, nullptr, nullptr, S.statics, sOnly, lane, wo, inv, tMin, bound, visitStatic);
    if (!occ && S.crowd && id < T.chars && T.chars > 0) {
        const int* order = id < 0 ? T.instOrder : nullptr;
        occ = sceneScan(T.worldBoxes, order ? T.groupBoxes : T.worldBoxes + (size_t)T.chars * 6, order ? T.superBoxes : nullptr, order, T.chars, id, lane,
                        wo, inv, tMin, bound, visitCharacter);
    }
    if (lane == 0) occluded[blockIdx.x] = occ ? 1 : 0;
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
