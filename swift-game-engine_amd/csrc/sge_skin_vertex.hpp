// The per-vertex arithmetic of the linear-blend skinning kernels over palettes staged in the pair layout, as a function:
// skinVertex is the expression tree of skinRange / skinRangeMulti (sge_skin.hip), term for term, so that a character's bytes do not
// depend on the form that wrote them (tests/test_gpu_mesh_variants.py holds the variant kernel to the uniform forms bit for bit).
// sge_skin_variants.hip includes it. sge_skin.hip keeps its own text: with its two lambdas routed through this header the
// compiler schedules skin_kernel / skin_ticket_multi_kernel differently (same instructions, another order, 873 lines of
// disassembly moved), and those kernels' schedule is what the measured step rests on.
// Compile the including translation unit with the default -ffp-contract=fast (see the header of sge_skin.hip).
#pragma once
#include "sge_internal.hpp"

namespace sge {

#ifndef SGE_SKIN_BLOCK
#define SGE_SKIN_BLOCK 256
#endif
constexpr int kSkinBlock = SGE_SKIN_BLOCK;

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

struct VertexIn { float3 p, n; float4 t; ushort4 idx; float4 w; };

template <int SRC_STRIDE>
__device__ __forceinline__ VertexIn loadVertex(const SkinLaunch& L, int gid) {
    VertexIn v;
#ifdef SGE_SKIN_EXPERIMENT_SMALL_SOURCE // diagnostic build: every load hits the same 256 source vertices (L1 resident)
    gid &= 255;
#endif
    const float* sp = reinterpret_cast<const float*>(L.srcPos) + (unsigned)gid * SRC_STRIDE;
    const float* sn = reinterpret_cast<const float*>(L.srcNrm) + (unsigned)gid * SRC_STRIDE;
    v.p = make_float3(sp[0], sp[1], sp[2]);
    v.n = make_float3(sn[0], sn[1], sn[2]);
    v.t = reinterpret_cast<const float4*>(L.srcTan)[gid];
    v.idx = reinterpret_cast<const ushort4*>(L.srcIdx)[gid];
    v.w = reinterpret_cast<const float4*>(L.srcWgt)[gid];
    return v;
}

// stage one palette of `bones` bones: thread -> one float4 COLUMN (coalesced), scattered into the pair layout, 12 floats per bone
// (m_rc = row r, column c of the bone's 3x4 affine part):  (m00 m10 | m01 m11) (m02 m12 | m03 m13) (m20 m21 | m22 m23)
__device__ __forceinline__ void stagePalettePairs(const float4* gp, int bones, float* dst, int tid) {
    for (int i = tid; i < bones * 4; i += kSkinBlock) {
        float4 col = gp[i];
        int bone = i >> 2, cc = i & 3;
        float* d = dst + bone * 12;
        d[2 * cc + 0] = col.x;
        d[2 * cc + 1] = col.y;
        d[8 + cc] = col.z;
    }
}

struct SkinnedVertex { v2f pxy; float pz; v2f nxy; float nz; v2f txy; float tz; };

// One vertex against one staged palette P (pair layout): blend the influences' matrices, transform position / normal / tangent once.
// sum_j w_j (M_j v) = (sum_j w_j M_j) v (the Metal kernel transforms per influence and blends the results, RayTracing.metalinc:
// 758-775); the first two influences are taken unconditionally with the weight clamped at 0 (a weight <= 0 contributes exactly
// nothing, as the reference's `w > 0` test does); the rarer third and fourth stay behind their tests.
__device__ __forceinline__ SkinnedVertex skinVertex(const v4f* P, const VertexIn& v) {
    const float w0 = fmaxf(v.w.x, 0.0f), w1 = fmaxf(v.w.y, 0.0f);
    v2f A, B, C, D, E, F;
    {
        const v4f q0 = P[v.idx.x * 3 + 0], q1 = P[v.idx.x * 3 + 1], q2 = P[v.idx.x * 3 + 2];
        A = q0.xy * w0; B = q0.zw * w0; C = q1.xy * w0; D = q1.zw * w0; E = q2.xy * w0; F = q2.zw * w0;
    }
#define SGE_BLEND(BONE, WGT)                                                                   \
    {                                                                                          \
        const v4f q0 = P[(BONE) * 3 + 0], q1 = P[(BONE) * 3 + 1], q2 = P[(BONE) * 3 + 2];      \
        A += q0.xy * (WGT); B += q0.zw * (WGT); C += q1.xy * (WGT); D += q1.zw * (WGT);        \
        E += q2.xy * (WGT); F += q2.zw * (WGT);                                                \
    }
    SGE_BLEND(v.idx.y, w1)
    if (v.w.z > 0.0f) SGE_BLEND(v.idx.z, v.w.z)
    if (v.w.w > 0.0f) SGE_BLEND(v.idx.w, v.w.w)
#undef SGE_BLEND
    SkinnedVertex r;
    // x, y: packed column sums; z: row 2 = (E.x, E.y, F.x, F.y)
    r.pxy = A * v.p.x + (B * v.p.y + (C * v.p.z + D));
    const v2f pe = E * v2f{v.p.x, v.p.y};
    r.pz = (pe.x + pe.y) + (F.x * v.p.z + F.y);
    r.nxy = A * v.n.x + (B * v.n.y + C * v.n.z);
    const v2f ne = E * v2f{v.n.x, v.n.y};
    r.nz = (ne.x + ne.y) + F.x * v.n.z;
    r.txy = A * v.t.x + (B * v.t.y + C * v.t.z);
    const v2f te = E * v2f{v.t.x, v.t.y};
    r.tz = (te.x + te.y) + F.x * v.t.z;
    {
        const v2f sq = r.nxy * r.nxy;
        const float s = __builtin_amdgcn_rsqf((sq.x + sq.y) + r.nz * r.nz);
        r.nxy *= s; r.nz *= s;
    }
    {
        const v2f sq = r.txy * r.txy;
        const float s = __builtin_amdgcn_rsqf((sq.x + sq.y) + r.tz * r.tz);
        r.txy *= s; r.tz *= s;
    }
    return r;
}

// streaming output: non-temporal stores (0.95-1.07 ms vs 1.10 ms with plain stores on MI355X)
template <int DST_STRIDE>
__device__ __forceinline__ void storeSkinnedVertex(float* op, float* on, v4f* ot, const SkinnedVertex& r, float tangentW) {
    if (DST_STRIDE == 4) {
        __builtin_nontemporal_store(v4f{r.pxy.x, r.pxy.y, r.pz, 0.f}, reinterpret_cast<v4f*>(op));
        __builtin_nontemporal_store(v4f{r.nxy.x, r.nxy.y, r.nz, 0.f}, reinterpret_cast<v4f*>(on));
    } else {
        __builtin_nontemporal_store(r.pxy.x, op); __builtin_nontemporal_store(r.pxy.y, op + 1); __builtin_nontemporal_store(r.pz, op + 2);
        __builtin_nontemporal_store(r.nxy.x, on); __builtin_nontemporal_store(r.nxy.y, on + 1); __builtin_nontemporal_store(r.nz, on + 2);
    }
    __builtin_nontemporal_store(v4f{r.txy.x, r.txy.y, r.tz, tangentW}, ot);
}

} // namespace sge
