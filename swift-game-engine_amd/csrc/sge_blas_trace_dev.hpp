// Device-side pieces of the closest-hit query shared by blas_intersect_kernel / blas_world_boxes_kernel (sge_blas.hip: one
// topology for the whole crowd) and their ragged forms (sge_blas_variants.hip: one topology per mesh variant): the ray-triangle
// test, the instance transform and the widened slab test. A header of its own, not sge_blas_dev.hpp: that one is also included
// by sge_skin.hip, which has helpers of the same names.
#pragma once
#include "sge_internal.hpp"

namespace sge {

// Moller-Trumbore as the engine's own rayTriangle (CollisionQuery.swift:1575-1601), also returning the barycentrics
__device__ __forceinline__ bool rayTriangleUV(F3 origin, F3 direction, F3 v0, F3 v1, F3 v2, float eps, float& tOut, float& uOut, float& vOut) {
    F3 e1 = v1 - v0, e2 = v2 - v0;
    F3 pvec = cross(direction, e2);
    float det = dot(e1, pvec);
    if (fabsf(det) < eps) return false;
    float invDet = 1.0f / det;
    F3 tvec = origin - v0;
    float u = dot(tvec, pvec) * invDet;
    if (u < 0 || u > 1) return false;
    F3 qvec = cross(tvec, e1);
    float v = dot(direction, qvec) * invDet;
    if (v < 0 || (u + v) > 1) return false;
    float t = dot(e2, qvec) * invDet;
    if (!(t >= 0)) return false;
    tOut = t + 0.0f; // -0 -> +0
    uOut = u;
    vOut = v;
    return true;
}

struct Inv3 { F3 r0, r1, r2; float ok; }; // rows of the inverse of the 3x3 part
__device__ __forceinline__ Inv3 inverse3(const Aff& m) {
    const F3 a = m.c0, b = m.c1, c = m.c2;
    const F3 bc = cross(b, c), ca = cross(c, a), ab = cross(a, b);
    const float det = dot(a, bc);
    const float r = 1.0f / det;
    return Inv3{bc * r, ca * r, ab * r, det};
}
__device__ __forceinline__ F3 mul3(const Inv3& m, F3 v) { return F3{dot(m.r0, v), dot(m.r1, v), dot(m.r2, v)}; }

template <int STRIDE>
__device__ __forceinline__ F3 loadP(const float* base, uint32_t i) { const float* p = base + (size_t)i * STRIDE; return F3{p[0], p[1], p[2]}; }

constexpr int kBlasStack = kBlasTraversalStackCap;
constexpr int kTraceWave = 64;

__device__ __forceinline__ Aff loadInstance(const float* instances, int inst) {
    const float* Mf = instances + (size_t)inst * 16;
    return Aff{F3{Mf[0], Mf[1], Mf[2]}, F3{Mf[4], Mf[5], Mf[6]}, F3{Mf[8], Mf[9], Mf[10]}, F3{Mf[12], Mf[13], Mf[14]}};
}

// widened slab test (CollisionQuery.swift:1603-1630 form): a box is only skipped when it is clearly off the ray or clearly
// behind the best hit
__device__ __forceinline__ bool slabPass(const float* bx, F3 o, F3 inv, float tMin, float bestT) {
    float t0 = (bx[0] - o.x) * inv.x, t1 = (bx[3] - o.x) * inv.x;
    float lo = fminf(t0, t1), hi = fmaxf(t0, t1);
    t0 = (bx[1] - o.y) * inv.y; t1 = (bx[4] - o.y) * inv.y;
    lo = fmaxf(lo, fminf(t0, t1)); hi = fminf(hi, fmaxf(t0, t1));
    t0 = (bx[2] - o.z) * inv.z; t1 = (bx[5] - o.z) * inv.z;
    lo = fmaxf(lo, fminf(t0, t1)); hi = fminf(hi, fmaxf(t0, t1));
    const float slack = 1e-3f * fmaxf(fabsf(lo), fabsf(hi)) + 1e-4f;
    return (lo - slack <= hi + slack) && (hi + slack >= tMin) && (lo - slack <= bestT);
}
// The form the scene kernels use (sge_ray_scene.hip): the box is also widened by a hair in position (1e-5 of the coordinates +
// 1e-6). A ray with a zero direction component that runs IN a face of the box — through a vertex that is an extreme of its
// cluster — is inside that slab only by the rounding of its object-space origin, which the slack in t (times inv = FLT_MAX
// there) cannot cover; the triangle test counts its edges in. (slabPass above has this weakness; blas_intersect_kernel and the
// ragged form keep it unchanged.)
__device__ __forceinline__ bool slabPassPadded(const float* bx, F3 o, F3 inv, float tMin, float bestT) {
    float pad = 1e-5f * fmaxf(fmaxf(fabsf(bx[0]), fabsf(bx[3])), fabsf(o.x)) + 1e-6f;
    float t0 = ((bx[0] - pad) - o.x) * inv.x, t1 = ((bx[3] + pad) - o.x) * inv.x;
    float lo = fminf(t0, t1), hi = fmaxf(t0, t1);
    pad = 1e-5f * fmaxf(fmaxf(fabsf(bx[1]), fabsf(bx[4])), fabsf(o.y)) + 1e-6f;
    t0 = ((bx[1] - pad) - o.y) * inv.y; t1 = ((bx[4] + pad) - o.y) * inv.y;
    lo = fmaxf(lo, fminf(t0, t1)); hi = fminf(hi, fmaxf(t0, t1));
    pad = 1e-5f * fmaxf(fmaxf(fabsf(bx[2]), fabsf(bx[5])), fabsf(o.z)) + 1e-6f;
    t0 = ((bx[2] - pad) - o.z) * inv.z; t1 = ((bx[5] + pad) - o.z) * inv.z;
    lo = fmaxf(lo, fminf(t0, t1)); hi = fminf(hi, fmaxf(t0, t1));
    const float slack = 1e-3f * fmaxf(fabsf(lo), fabsf(hi)) + 1e-4f;
    return (lo - slack <= hi + slack) && (hi + slack >= tMin) && (lo - slack <= bestT);
}
__device__ __forceinline__ F3 invDir(F3 d) {
    return F3{d.x != 0 ? 1.0f / d.x : kFloatMax, d.y != 0 ? 1.0f / d.y : kFloatMax, d.z != 0 ? 1.0f / d.z : kFloatMax};
}

// ---- the closest-hit walk of one instance and the record at the hit, shared by blas_intersect_kernel (sge_blas.hip) and the
// scene kernels (sge_ray_scene.hip). One wavefront per ray; `stack` is kBlasStack ints of LDS. ----

// The best hit of a ray so far. `inst` is whatever id the caller orders instances by (< 0: none yet).
struct BlasBest { float t, u, v; uint32_t prim; int inst; };

// One 64-wide tree in object space: entry boxes [entryCount + 1][6], positions with STRIDE floats per vertex.
struct BlasTreeRef {
    const int* wideFirst; const int2* entryLink; const uint32_t* slotIndices; const uint32_t* slotTriangle;
    const float* boxes; const float* P;
};

// closest hit inside one instance; accepted when closer than best.t (equal: only the instance with the smaller id keeps it).
// PADDED: the entry boxes are tested with slabPassPadded.
template <int STRIDE, bool PADDED = false>
__device__ __forceinline__ void blasTraverseClosest(int* stack, int lane, const BlasTreeRef& G, const Aff& M, F3 wo, F3 wd, float tMin, float maxDistance,
                                                    int inst, BlasBest& B) {
    const Inv3 Mi = inverse3(M);
    const F3 o = mul3(Mi, wo - M.c3), d = mul3(Mi, wd);
    const F3 inv = invDir(d);
    const float* P = G.P;
    const float* boxes = G.boxes;
    // (distance bits, primitive id); distances are >= 0, so their bit patterns order like the values. An instance found
    // earlier keeps a tie: the starting key carries primitive 0, which nothing is smaller than at equal distance.
    // (with the instances visited in another order than that of their ids, an instance with a smaller id than the holder of
    // the best hit so far may still take it at equal distance: its starting key accepts any primitive there)
    unsigned long long best = ((unsigned long long)__float_as_uint(B.t) << 32) | ((B.inst < 0 || inst < B.inst) ? 0xffffffffull : 0ull);
    float u0 = 0, v0 = 0;
    bool found = false;
    int sp = 1;
    if (lane == 0) stack[0] = 0;
    __syncthreads();
    while (sp > 0) {
        const int w = stack[sp - 1];
        --sp;
        __syncthreads();
        const int first = G.wideFirst[w], cnt = G.wideFirst[w + 1] - first;
        bool pass = false;
        int2 link = make_int2(0, 0);
        if (lane < cnt) {
            link = G.entryLink[first + lane];
            const float bound = __uint_as_float((unsigned)(best >> 32));
            pass = PADDED ? slabPassPadded(boxes + (size_t)(first + lane) * 6, o, inv, tMin, bound) : slabPass(boxes + (size_t)(first + lane) * 6, o, inv, tMin, bound);
        }
        const unsigned long long inner = __ballot(pass && link.x >= 0), leaves = __ballot(pass && link.x < 0);
        if (pass && link.x >= 0) {
            const int at = sp + __popcll(inner & ((1ull << lane) - 1));
            if (at < kBlasStack) stack[at] = link.x;
        }
        sp = min(sp + __popcll(inner), kBlasStack);
        unsigned long long m = leaves;
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int firstSlot = ~__shfl(link.x, src, kTraceWave), count = __shfl(link.y, src, kTraceWave);
            unsigned long long key = ~0ull;
            float u = 0, v = 0;
            if (lane < count) {
                const uint32_t* ix = G.slotIndices + (size_t)(firstSlot + lane) * 3;
                const F3 p0 = loadP<STRIDE>(P, ix[0]), p1 = loadP<STRIDE>(P, ix[1]), p2 = loadP<STRIDE>(P, ix[2]);
                float t;
                if (rayTriangleUV(o, d, p0, p1, p2, 1e-6f, t, u, v) && t >= tMin && t <= maxDistance)
                    key = ((unsigned long long)__float_as_uint(t) << 32) | G.slotTriangle[firstSlot + lane];
            }
            unsigned long long k = key;
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned lo32 = __shfl_xor((unsigned)k, off, kTraceWave), hi32 = __shfl_xor((unsigned)(k >> 32), off, kTraceWave);
                const unsigned long long other = ((unsigned long long)hi32 << 32) | lo32;
                k = other < k ? other : k;
            }
            if (k != ~0ull && k < best) {
                best = k;
                found = true;
                const int winner = __ffsll((long long)__ballot(key == k)) - 1;
                u0 = __shfl(u, winner, kTraceWave);
                v0 = __shfl(v, winner, kTraceWave);
            }
        }
        __syncthreads();
    }
    if (found) {
        B.t = __uint_as_float((unsigned)(best >> 32));
        B.prim = (uint32_t)best;
        B.u = u0; B.v = v0;
        B.inst = inst;
    }
}

// The face-forwarded geometric normal of a hit triangle with object-space vertices v0, v1, v2 (RayTracing.metalinc:258-268): the
// geomNormal of the hit record, and the N the shaded frame (sge_render.hip) shades with.
__device__ __forceinline__ F3 blasFaceNormal(const Aff& M, F3 v0, F3 v1, F3 v2, F3 wd) {
    const F3 w0 = affMulPoint(M, v0), w1 = affMulPoint(M, v1), w2 = affMulPoint(M, v2);
    F3 N = normalize(cross(w1 - w0, w2 - w0));
    if (dot(N, wd) > 0.0f) N = -N;
    return N;
}

// What raytraceKernel derives at a hit (RayTracing.metalinc:258-300) from one instance's streams: P and NB with STRIDE floats per
// vertex, TB with four, uvs with two (or null), `ix` the three indices of the hit triangle. Fills everything but H.instance.
template <int STRIDE>
__device__ __forceinline__ void blasHitRecord(const Aff& M, const float* P, const float* NB, const float* TB, const float* uvs, const uint32_t* ix,
                                              F3 wd, const BlasBest& B, sge_blas_hit& H) {
    const uint32_t i0 = ix[0], i1 = ix[1], i2 = ix[2];
    const F3 N = blasFaceNormal(M, loadP<STRIDE>(P, i0), loadP<STRIDE>(P, i1), loadP<STRIDE>(P, i2), wd);
    // :283-300
    const float bx = B.u, by = B.v, bw = 1.0f - bx - by;
    const F3 n0 = loadP<STRIDE>(NB, i0), n1 = loadP<STRIDE>(NB, i1), n2 = loadP<STRIDE>(NB, i2);
    const float* q0 = TB + (size_t)i0 * 4; const float* q1 = TB + (size_t)i1 * 4; const float* q2 = TB + (size_t)i2 * 4;
    const F3 nObj = normalize((n0 * bw + n1 * bx) + n2 * by);
    float t4[4];
    for (int k = 0; k < 4; ++k) t4[k] = (q0[k] * bw + q1[k] * bx) + q2[k] * by;
    const float r4 = 1.0f / sqrtf(((t4[0] * t4[0] + t4[1] * t4[1]) + t4[2] * t4[2]) + t4[3] * t4[3]);
    const F3 tObj = normalize(F3{t4[0] * r4, t4[1] * r4, t4[2] * r4});
    const float tw = t4[3] * r4;
    const F3 nW = normalize((M.c0 * nObj.x + M.c1 * nObj.y) + M.c2 * nObj.z);
    const F3 tW = normalize((M.c0 * tObj.x + M.c1 * tObj.y) + M.c2 * tObj.z);
    const F3 bW = normalize(cross(nW, tW) * tw);
    H.hit = 1; H.primitive = (int32_t)B.prim; H.distance = B.t; H.bary[0] = bx; H.bary[1] = by;
    H.geomNormal[0] = N.x; H.geomNormal[1] = N.y; H.geomNormal[2] = N.z;
    H.normal[0] = nW.x; H.normal[1] = nW.y; H.normal[2] = nW.z;
    H.tangent[0] = tW.x; H.tangent[1] = tW.y; H.tangent[2] = tW.z;
    H.bitangent[0] = bW.x; H.bitangent[1] = bW.y; H.bitangent[2] = bW.z;
    if (uvs) { // interp_uv, RayTracing.metalinc:106-119
        const float* a0 = uvs + (size_t)i0 * 2; const float* a1 = uvs + (size_t)i1 * 2; const float* a2 = uvs + (size_t)i2 * 2;
        H.uv[0] = (a0[0] * bw + a1[0] * bx) + a2[0] * by;
        H.uv[1] = (a0[1] * bw + a1[1] * bx) + a2[1] * by;
    }
}

// The instance level of a ray that names no instance. visit(i) is called, wave-uniformly, for every instance whose world box the
// ray may hit within `bound` (read again before every test: a closest-hit visitor shrinks it) and returns true to end the scan.
// The flat form: one box per instance, then one per 64 consecutive instances (`boxes[count ..]`), scanned 64 groups per step.
template <class Visit>
__device__ __forceinline__ bool blasScanFlat(const float* boxes, int count, int lane, F3 wo, F3 inv, float tMin, const float& bound, Visit&& visit) {
    const int groups = (count + kTraceWave - 1) / kTraceWave;
    const float* groupBoxes = boxes + (size_t)count * 6;
    for (int gbase = 0; gbase < groups; gbase += kTraceWave) {
        const int g = gbase + lane;
        unsigned long long gm = __ballot(g < groups && slabPass(groupBoxes + (size_t)g * 6, wo, inv, tMin, bound));
        while (gm) {
            const int gsrc = __ffsll((long long)gm) - 1;
            gm &= gm - 1;
            const int base = (gbase + gsrc) * kTraceWave, i = base + lane;
            const bool pass = i < count && slabPass(boxes + (size_t)i * 6, wo, inv, tMin, bound);
            unsigned long long m = __ballot(pass);
            while (m) {
                const int src = __ffsll((long long)m) - 1;
                m &= m - 1;
                if (visit(base + src)) return true;
            }
        }
    }
    return false;
}
// The grid-ordered form: three scans of 64 boxes: super-groups (4,096 instances each: 62 of them hold 250,000 characters, one
// step), the groups of the ones the ray may hit, the instances of those groups — grouped by where they ARE (grid order), not by
// their index
template <class Visit>
__device__ __forceinline__ bool blasScanGrid(const BlasTrace& T, int lane, F3 wo, F3 inv, float tMin, const float& bound, Visit&& visit) {
    const int groups = (T.chars + kTraceWave - 1) / kTraceWave, supers = (groups + kTraceWave - 1) / kTraceWave;
    for (int sbase = 0; sbase < supers; sbase += kTraceWave) {
        const int sg = sbase + lane;
        unsigned long long sm = __ballot(sg < supers && slabPass(T.superBoxes + (size_t)sg * 6, wo, inv, tMin, bound));
        while (sm) {
            const int ssrc = __ffsll((long long)sm) - 1;
            sm &= sm - 1;
            const int g = (sbase + ssrc) * kTraceWave + lane;
            unsigned long long gm = __ballot(g < groups && slabPass(T.groupBoxes + (size_t)g * 6, wo, inv, tMin, bound));
            while (gm) {
                const int gsrc = __ffsll((long long)gm) - 1;
                gm &= gm - 1;
                const int slot = ((sbase + ssrc) * kTraceWave + gsrc) * kTraceWave + lane;
                const int inst = slot < T.chars ? T.instOrder[slot] : -1;
                const bool pass = inst >= 0 && slabPass(T.worldBoxes + (size_t)inst * 6, wo, inv, tMin, bound);
                unsigned long long m = __ballot(pass);
                while (m) {
                    const int src = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    if (visit(__shfl(inst, src, kTraceWave))) return true;
                }
            }
        }
    }
    return false;
}

} // namespace sge
