// Device-side pieces of the whole-scene queries shared by scene_trace_kernel / scene_occlusion_kernel (sge_ray_scene.hip) and
// render_frame_kernel (sge_render.hip): the tree of a static mesh or of one character as blasTraverseClosest takes it, and the
// instance level of either half as one loop nest.
#pragma once
#include "sge_blas_trace_dev.hpp"

namespace sge {

constexpr int kWave = kTraceWave;

__device__ __forceinline__ BlasTreeRef sceneTree(const DevSceneMesh& m) {
    return BlasTreeRef{m.wideFirst, m.entryLink, m.slotIndices, m.slotTriangle, m.boxes, m.positions};
}
template <int STRIDE>
__device__ __forceinline__ BlasTreeRef crowdTree(const BlasTrace& T, int inst) {
    const DevBlas& B = T.blas;
    return BlasTreeRef{B.wideFirst, B.entryLink, B.slotIndices, B.slotTriangle, T.bounds + (size_t)inst * (B.entryCount + 1) * 6,
                       reinterpret_cast<const float*>(T.positions) + (size_t)inst * B.vertexCount * STRIDE};
}

// The instance level of either half as one loop nest, so that each kernel inlines one walk per half: 64 super-group boxes per
// step, the 64 groups of every super-group the ray may hit, the 64 instances of every such group. `order` null: slot i is
// instance i; `superBoxes` null: every super-group is entered, which is the flat scan of 64 group boxes per step. `only` >= 0
// (with `order` null): the ray names that instance; the one super-group, group and slot that hold it are entered without a box
// test. visit(i) is called wave-uniformly and returns true to end the scan; `bound` is read again before every box test (a
// closest-hit visitor shrinks it). Every loop is bounded by a count read before it starts or by the bits of a ballot.
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

} // namespace sge
