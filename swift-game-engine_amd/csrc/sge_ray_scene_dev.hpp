// Device-side pieces of the whole-scene queries shared by scene_trace_kernel / scene_occlusion_kernel (sge_ray_scene.hip),
// render_frame_kernel (sge_render.hip) and their forms for a crowd with mesh variants (sge_scene_variants.hip): the tree of a
// static mesh or of one character as blasTraverseClosest takes it, the instance level of either half as one loop nest, the
// any-hit walk of one instance, and the accessors that say where a character's tree and streams are found. The kernels' bodies are
// the texts sge_scene_trace_body.inc, sge_scene_occlusion_body.inc and sge_render_frame_body.inc.
#pragma once
#include "sge_blas_trace_dev.hpp"

namespace sge {

constexpr int kWave = kTraceWave;
constexpr int kSceneNoVariant = 0xFF; // a character's record when no refit describes it (include/sge_amd_variant_blas.h)

__device__ __forceinline__ int uniformInt(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ BlasTreeRef sceneTree(const DevSceneMesh& m) {
    return BlasTreeRef{m.wideFirst, m.entryLink, m.slotIndices, m.slotTriangle, m.boxes, m.positions};
}
template <int STRIDE>
__device__ __forceinline__ BlasTreeRef crowdTree(const BlasTrace& T, int inst) {
    const DevBlas& B = T.blas;
    return BlasTreeRef{B.wideFirst, B.entryLink, B.slotIndices, B.slotTriangle, T.bounds + (size_t)inst * (B.entryCount + 1) * 6,
                       reinterpret_cast<const float*>(T.positions) + (size_t)inst * B.vertexCount * STRIDE};
}

// ---- the crowd half's accessor: where one character's tree and streams are. record(inst) is kSceneNoVariant for a character
// that is never entered, else what tree(inst, record) takes; streams() is asked only about a character a walk has reported. ----
struct CrowdStreams { size_t vbase; const uint32_t* indices; const float* uvs; }; // first vertex in the skinned streams, [T][3], [V][2] or null

// every character holds the one mesh of T.blas
template <int STRIDE>
struct UniformCrowd {
    const BlasTrace& T;
    __device__ __forceinline__ int record(int) const { return 0; }
    __device__ __forceinline__ BlasTreeRef tree(int inst, int) const { return crowdTree<STRIDE>(T, inst); }
    __device__ __forceinline__ CrowdStreams streams(int inst) const { return CrowdStreams{(size_t)inst * T.blas.vertexCount, T.indices, T.uvs}; }
};
// Mesh variants, as blas_intersect_ragged_kernel takes them (sge_blas_variants.hip): the record the newest refit left says whose
// structure the character's boxes describe; topology, index buffer and uvs are that variant's row of the table, the vertices start
// at off[inst], the boxes at row inst * rowStride. Everything is loaded when the character is entered, wave-uniformly (`inst` is
// the same in every lane), and nothing of it is held across the instance scan.
template <int STRIDE>
struct RaggedCrowd {
    const BlasTrace& T;
    const SceneRagged& G;
    // 0xFF: dropped at the capacity cut, or never refitted: no boxes, no vertices
    __device__ __forceinline__ int record(int inst) const { return uniformInt((int)G.charVariant[uniformInt(inst)]); }
    __device__ __forceinline__ BlasTreeRef tree(int instAny, int v) const {
        const int inst = uniformInt(instAny);
        const DevBlas& B = G.table[v].blas;
        return BlasTreeRef{B.wideFirst, B.entryLink, B.slotIndices, B.slotTriangle, T.bounds + (size_t)inst * G.rowStride * 6,
                           reinterpret_cast<const float*>(T.positions) + (size_t)G.off[inst] * STRIDE};
    }
    __device__ __forceinline__ CrowdStreams streams(int inst) const {
        const DevVariantBlas& row = G.table[G.charVariant[inst]]; // (reported by a walk: the record names a variant)
        return CrowdStreams{(size_t)G.off[inst], row.indices, row.uvs};
    }
};

// The instance level of either half as one loop nest, so that each kernel inlines one walk per half: 64 super-group boxes per
// step, the 64 groups of every super-group the ray may hit, the 64 instances of every such group. `order` null: slot i is
// instance i; `superBoxes` null: every super-group is entered, which is the flat scan of 64 group boxes per step. `only` >= 0
// (with `order` null): the ray names that instance; the one super-group, group and slot that hold it are entered without a box
// test. visit(i) is called wave-uniformly and returns true to end the scan; `bound` is read again before every box test (a
// closest-hit visitor shrinks it). Every loop is bounded by a count read before it starts or by the bits of a ballot.
// (A character without a structure has a NaN world box: every comparison of slabPassPadded is false for it, and the min / max
// that form a group's box skip it; a group of nothing else has an inverted box, which at worst is entered for nothing.)
template <class Visit>
__device__ __forceinline__ bool sceneScan(const float* boxes, const float* groupBoxes, const float* superBoxes, const int* order, int count, int only,
                                          int lane, F3 wo, F3 inv, float tMin, const float& bound, Visit&& visit) {
    const int groups = (count + kWave - 1) / kWave, supers = (groups + kWave - 1) / kWave;
    const int sBegin = only >= 0 ? ((only >> 12) & ~(kWave - 1)) : 0, sEnd = only >= 0 ? sBegin + 1 : supers;
    for (int sbase = sBegin; sbase < sEnd; sbase += kWave) {
        const int sg = sbase + lane;
        const bool sIn = sg < supers && (only >= 0 ? sg == (only >> 12) : (!superBoxes || slabPassPadded(superBoxes + (size_t)sg * 6, wo, inv, tMin, bound)));
        unsigned long long sm = __ballot(sIn);
        while (sm) {
            const int ssrc = __ffsll((long long)sm) - 1;
            sm &= sm - 1;
            const int g = (sbase + ssrc) * kWave + lane;
            const bool gIn = g < groups && (only >= 0 ? g == (only >> 6) : slabPassPadded(groupBoxes + (size_t)g * 6, wo, inv, tMin, bound));
            unsigned long long gm = __ballot(gIn);
            while (gm) {
                const int gsrc = __ffsll((long long)gm) - 1;
                gm &= gm - 1;
                const int slot = ((sbase + ssrc) * kWave + gsrc) * kWave + lane;
                const int inst = slot < count ? (order ? order[slot] : slot) : -1;
                const bool pass = inst >= 0 && (only >= 0 ? inst == only : slabPassPadded(boxes + (size_t)inst * 6, wo, inv, tMin, bound));
                unsigned long long m = __ballot(pass);
                while (m) {
                    const int src = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    if (visit(__shfl(inst, src, kWave))) return true;
                }
            }
        }
    }
    return false;
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


} // namespace sge
