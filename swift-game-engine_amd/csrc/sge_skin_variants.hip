// Linear-blend skinning of a crowd whose characters name one of up to SGE_MAX_MESH_VARIANTS source meshes each
// (include/sge_amd_variants.h). Two launches on one stream, no host round trip between them:
//
//   variant_plan_kernel    one workgroup: the exclusive 64-bit scan off[chars + 1] of the characters' vertex counts, the
//                          characters grouped by variant (lists), and the plan header the skin launch reads its size from
//   skin_variant_kernel    resident workgroups drawing work units from a ticket counter (the protocol of
//                          skin_ticket_multi_kernel, sge_skin.hip); a unit = (variant, group of up to CPW characters of that
//                          variant's list, vertex split): every source vertex is loaded once and skinned with the group's palettes
//
// and lod_select_kernel, which fills the variant array from the bodies' distance to an eye point.
// The per-vertex arithmetic is skinVertex (sge_skin_vertex.hpp), the expression tree of the uniform forms: this translation unit
// is compiled like sge_skin.hip, with the default -ffp-contract=fast. The distance arithmetic of the LOD kernel is kept
// uncontracted by a pragma of its own.
#include <algorithm>
#include "sge_skin_vertex.hpp"

namespace sge {

namespace {

constexpr int kPlanBlock = 1024;
constexpr int kPlanWaves = kPlanBlock / 64;
constexpr int kMaxVariants = SGE_MAX_MESH_VARIANTS;

template <class T>
__device__ __forceinline__ T waveInclusiveScan(T v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// exclusive scan of one value per thread over the workgroup; `total` = the sum over all threads. waveTotals: kPlanWaves entries of LDS.
template <class T>
__device__ __forceinline__ T blockExclusiveScan(T v, T* waveTotals, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T inc = waveInclusiveScan(v, lane);
    if (lane == 63) waveTotals[wave] = inc;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kPlanWaves; ++w) {
        const T t = waveTotals[w];
        if (w < wave) before += t;
        all += t;
    }
    __syncthreads(); // waveTotals is free for the next scan
    total = all;
    return before + inc - v;
}

// One workgroup; thread t owns the characters [t * chunk, (t + 1) * chunk), so lists keep the characters of a variant in index order.
// Three walks over the variant bytes (vertex sums; offsets, fit and per-variant counts; scatter) around two rounds of scans.
__global__ __launch_bounds__(kPlanBlock) void variant_plan_kernel(VariantSkinLaunch L, int cpw) {
    __shared__ long long sWave64[kPlanWaves];
    __shared__ int sWave32[kPlanWaves];
    __shared__ int sVerts[kMaxVariants], sSplits[kMaxVariants];
    const int tid = threadIdx.x;
    if (tid < kMaxVariants) {
        sVerts[tid] = tid < L.variants ? L.table[tid].mesh.vertexCount : 0;
        sSplits[tid] = tid < L.variants ? L.table[tid].splits : 0;
    }
    __syncthreads();
    const int chunk = (L.chars + kPlanBlock - 1) / kPlanBlock;
    const int c0 = min(tid * chunk, L.chars), c1 = min(c0 + chunk, L.chars);
    const int top = L.variants - 1; // values beyond the uploaded variants are clamped to the highest one

    long long sum = 0;
    for (int c = c0; c < c1; ++c) sum += sVerts[min((int)L.variantOf[c], top)];
    long long total = 0;
    const long long base = blockExclusiveScan(sum, sWave64, total);

    int cnt[kMaxVariants], dropped = 0;
#pragma unroll
    for (int k = 0; k < kMaxVariants; ++k) cnt[k] = 0;
    long long run = base;
    for (int c = c0; c < c1; ++c) {
        const int v = min((int)L.variantOf[c], top);
        L.off[c] = run;
        run += sVerts[v];
        const bool keep = run <= L.capacityVertices; // a slice that would end beyond the capacity is left out
        dropped += keep ? 0 : 1;
#pragma unroll
        for (int k = 0; k < kMaxVariants; ++k) cnt[k] += (keep && v == k) ? 1 : 0;
    }
    if (tid == 0) L.off[L.chars] = total;

    int pre[kMaxVariants], listBase[kMaxVariants + 1];
    listBase[0] = 0;
#pragma unroll
    for (int k = 0; k < kMaxVariants; ++k) {
        int tot = 0;
        pre[k] = 0;
        if (k < L.variants) pre[k] = blockExclusiveScan(cnt[k], sWave32, tot); // (uniform branch)
        listBase[k + 1] = listBase[k] + tot;
    }
    int droppedTotal = 0;
    (void)blockExclusiveScan(dropped, sWave32, droppedTotal);

    run = base;
    for (int c = c0; c < c1; ++c) {
        const int v = min((int)L.variantOf[c], top);
        run += sVerts[v];
        if (run > L.capacityVertices) continue;
#pragma unroll
        for (int k = 0; k < kMaxVariants; ++k)
            if (v == k) { L.lists[listBase[k] + pre[k]] = c; pre[k] += 1; }
    }

    if (tid == 0) {
        SkinPlan P;
        P.totalVertices = total;
        P.capacityVertices = L.capacityVertices;
        int units = 0;
#pragma unroll
        for (int k = 0; k < kMaxVariants; ++k) {
            const int kept = listBase[k + 1] - listBase[k];
            P.kept[k] = kept;
            P.listBase[k] = listBase[k];
            P.unitBase[k] = units;
            units += (kept + cpw - 1) / cpw * sSplits[k];
        }
        P.listBase[kMaxVariants] = listBase[kMaxVariants];
        P.unitBase[kMaxVariants] = units;
        P.units = units;
        P.dropped = droppedTotal;
        P.charsPerUnit = cpw;
        P.variants = L.variants;
        *L.plan = P;
    }
}

__device__ __forceinline__ int uniformInt(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ long long uniformInt64(long long x) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)x);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)x >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// The work of one unit: vertices [vBegin, vEnd) of the mesh behind L for the nChars (1..CPW) characters chars[0..nChars): their
// palettes staged in the pair layout, every source vertex loaded once, character k's slice of the streams at vertex off[chars[k]].
template <int DST_STRIDE, int CPW>
__device__ __forceinline__ void skinRangeGroup(const SkinLaunch& L, const int* __restrict__ chars, const int nChars,
                                               const long long* __restrict__ off, const int vBegin, const int vEnd, float4* pal) {
    const int tid = threadIdx.x;
    int gid = vBegin + tid;
    VertexIn cur{};
    if (gid < vEnd) cur = loadVertex<3>(L, gid);
    const int rows = L.paletteCount * 3; // float4 rows of one staged palette
    float* palf = reinterpret_cast<float*>(pal);
    long long base[CPW];
#pragma unroll
    for (int k = 0; k < CPW; ++k) {
        const int c = uniformInt(chars[min(k, nChars - 1)]); // (a partial group repeats its last character: never stored)
        base[k] = uniformInt64(off[c]);
        if (k < nChars)
            stagePalettePairs(reinterpret_cast<const float4*>(L.palettes + (size_t)c * L.paletteCount * 16), L.paletteCount,
                              palf + (size_t)k * rows * 4, tid);
    }
    __syncthreads();
    float* const opBase = reinterpret_cast<float*>(L.outPos);
    float* const onBase = reinterpret_cast<float*>(L.outNrm);
    v4f* const otBase = reinterpret_cast<v4f*>(L.outTan);

    auto skinAll = [&](const VertexIn& v, int g) {
#pragma unroll
        for (int k = 0; k < CPW; ++k) {
            if (k >= nChars) break;
            const v4f* P = reinterpret_cast<const v4f*>(pal) + (size_t)k * rows;
            const SkinnedVertex r = skinVertex(P, v);
            float* op = opBase + (size_t)base[k] * DST_STRIDE + (unsigned)g * DST_STRIDE;
            float* on = onBase + (size_t)base[k] * DST_STRIDE + (unsigned)g * DST_STRIDE;
            storeSkinnedVertex<DST_STRIDE>(op, on, otBase + (size_t)base[k] + (unsigned)g, r, v.t.w);
        }
    };

    // the next chunk's source vertex is requested when the current one is done with (skinRangeMulti's form for four characters per
    // vertex; here for every CPW: with the chunk in flight kept as well, the two-character instance needs 100 registers)
    if (gid >= vEnd) return;
    while (true) {
        skinAll(cur, gid);
        gid += kSkinBlock;
        if (gid >= vEnd) break;
        cur = loadVertex<3>(L, gid);
    }
}

// the ticket words are left at zero by the launch itself (ticketsDone, sge_skin.hip): queue[1] counts the workgroups that have
// drawn their last ticket, and the last of them clears both words
__device__ __forceinline__ void variantTicketsDone(int* __restrict__ queue) {
    if (threadIdx.x == 0 && atomicAdd(queue + 1, 1) == (int)gridDim.x - 1) {
        __hip_atomic_store(queue, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(queue + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Resident workgroups; the number of units is the plan's (device memory: the launch is sized before the plan has run, a
// workgroup beyond the units only signs off). Unit u belongs to the variant with the highest unitBase <= u: a search over the
// <= 8 bases (a variant without characters has the base of its successor and is never found). Dynamic LDS: CPW palettes of
// paletteCount bones + the ticket slot behind them.
template <int DST_STRIDE, int CPW>
__global__ __launch_bounds__(kSkinBlock, 1) void skin_variant_kernel(const DevVariant* __restrict__ table, const SkinPlan* __restrict__ plan,
                                                                     const int* __restrict__ lists, const long long* __restrict__ off,
                                                                     const float* __restrict__ palettes, int paletteCount,
                                                                     void* outPos, void* outNrm, void* outTan, int* __restrict__ queue) {
    extern __shared__ float4 palDyn[];
    int* const sNextUnit = reinterpret_cast<int*>(palDyn + (size_t)CPW * paletteCount * 3); // (behind the palettes: their 16-byte alignment stays)
    const int units = uniformInt(plan->units);
    for (int u = blockIdx.x; u < units;) {
        int v = 0;
#pragma unroll
        for (int k = 1; k < kMaxVariants; ++k) v += u >= plan->unitBase[k] ? 1 : 0;
        v = uniformInt(v);
        const int local = u - uniformInt(plan->unitBase[v]);
        const DevVariant* row = table + v;
        const int splits = uniformInt(row->splits), vertsPerSplit = uniformInt(row->vertsPerSplit), vertexCount = uniformInt(row->mesh.vertexCount);
        const int gidx = local / splits;
        const int sp = local - gidx * splits;
        const int vBegin = sp * vertsPerSplit;
        const int n0 = gidx * CPW;
        const int nChars = min(CPW, uniformInt(plan->kept[v]) - n0);
        const int* chars = lists + uniformInt(plan->listBase[v]) + n0;
        SkinLaunch L{row->mesh.positions, row->mesh.normals, row->mesh.tangents, row->mesh.boneIndices, row->mesh.boneWeights,
                     palettes, paletteCount, vertexCount, nChars, 0,
                     SGE_LAYOUT_PACKED, DST_STRIDE == 4 ? SGE_LAYOUT_PADDED16 : SGE_LAYOUT_PACKED, outPos, outNrm, outTan};
        int ticket = 0;
        if (threadIdx.x == 0) ticket = atomicAdd(queue, 1);
        skinRangeGroup<DST_STRIDE, CPW>(L, chars, nChars, off, vBegin, min(vertexCount, vBegin + vertsPerSplit), palDyn);
        if (threadIdx.x == 0) *sNextUnit = (int)gridDim.x + ticket;
        __syncthreads(); // also: every thread is done with the palettes
        u = *sNextUnit;
    }
    variantTicketsDone(queue);
}

struct LodThresholds { double squared[kMaxVariants - 1]; int n; };

// variant = number of thresholds the squared distance has reached (>=), clamped. float64, every product and sum rounded by itself:
// a numpy restatement decides the same way.
__global__ __launch_bounds__(256) void lod_select_kernel(const sge_body_state* __restrict__ bodies, int count, double ex, double ey, double ez,
                                                         LodThresholds T, int highestVariant, uint8_t* __restrict__ variantOf) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= count) return;
    int v = 0;
    {
#pragma clang fp contract(off)
        const double dx = bodies[c].position[0] - ex, dy = bodies[c].position[1] - ey, dz = bodies[c].position[2] - ez;
        const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
        const double xy = xx + yy;
        const double d2 = xy + zz;
#pragma unroll
        for (int i = 0; i < kMaxVariants - 1; ++i) v += (i < T.n && d2 >= T.squared[i]) ? 1 : 0;
    }
    variantOf[c] = (uint8_t)min(v, highestVariant);
}

template <int DST_STRIDE, int CPW>
void launchVariantKernel(const VariantSkinLaunch& L, dim3 grid, size_t lds, int* queue, hipStream_t s) {
    hipLaunchKernelGGL((skin_variant_kernel<DST_STRIDE, CPW>), grid, dim3(kSkinBlock), lds, s, L.table, L.plan, L.lists, L.off, L.palettes, L.paletteCount,
                       L.outPos, L.outNrm, L.outTan, queue);
}

} // namespace

// the rule of launch_skin: CPW palettes of 48 bytes per bone + the 16-byte ticket slot fit the 64 KB a kernel may ask for
// without an attribute, else half as many characters per unit. At most four: with eight characters' stream bases held in scalar
// registers the kernel passes the 96 vector registers the overlap schedule counts on (101).
int variantCharsPerUnit(int paletteCount, int charsPerUnit) {
    int cpw = charsPerUnit >= 4 ? 4 : charsPerUnit >= 2 ? 2 : 1;
    while (cpw >= 2 && (size_t)cpw * paletteCount * 48 + 16 > (size_t)64 * 1024) cpw /= 2;
    return cpw;
}

void variantSplits(int vertexCount, int groups, int& splits, int& vertsPerSplit) {
    int sp = 1;
    while ((long long)groups * sp < 8192 && sp < 64 && (vertexCount + sp - 1) / sp > 2 * kSkinBlock) sp *= 2;
    vertsPerSplit = ((vertexCount + sp - 1) / sp + kSkinBlock - 1) / kSkinBlock * kSkinBlock;
    splits = (vertexCount + vertsPerSplit - 1) / vertsPerSplit;
}

int launch_skin_variants(const VariantSkinLaunch& L, hipStream_t s, int* residentQueue, int residentQuarters, int charsPerUnit, hipEvent_t planDone) {
    if (L.chars <= 0 || L.variants <= 0 || L.variants > kMaxVariants || !residentQueue) return 0;
    const int cpw = variantCharsPerUnit(L.paletteCount, charsPerUnit);
    hipLaunchKernelGGL(variant_plan_kernel, dim3(1), dim3(kPlanBlock), 0, s, L, cpw);
    if (planDone) (void)hipEventRecord(planDone, s); // the plan has read its copy of the variant bytes
    // the grid is sized by what the plan can ask for at most (every variant's last group partial, the largest split count: 64)
    const size_t unitsAtMost = ((size_t)(L.chars + cpw - 1) / cpw + L.variants) * 64;
    const size_t resident = std::max<size_t>(1, (size_t)currentDeviceCUs() * std::max(1, residentQuarters) / 4);
    const dim3 grid((unsigned)std::min(unitsAtMost, resident));
    const size_t lds = (size_t)cpw * L.paletteCount * 48 + 16;
    const bool padded = L.dstLayout == SGE_LAYOUT_PADDED16;
    switch (cpw) {
    case 1: padded ? launchVariantKernel<4, 1>(L, grid, lds, residentQueue, s) : launchVariantKernel<3, 1>(L, grid, lds, residentQueue, s); break;
    case 2: padded ? launchVariantKernel<4, 2>(L, grid, lds, residentQueue, s) : launchVariantKernel<3, 2>(L, grid, lds, residentQueue, s); break;
    default: padded ? launchVariantKernel<4, 4>(L, grid, lds, residentQueue, s) : launchVariantKernel<3, 4>(L, grid, lds, residentQueue, s); break;
    }
    return cpw;
}

void launch_lod_select(const sge_body_state* bodies, int count, const double eye[3], const float* distances, int n, int highestVariant,
                       uint8_t* variantOf, hipStream_t s) {
    if (count <= 0) return;
    LodThresholds T{};
    T.n = n;
    for (int i = 0; i < n && i < kMaxVariants - 1; ++i) T.squared[i] = (double)distances[i] * (double)distances[i]; // exact: 24-bit significands
    hipLaunchKernelGGL(lod_select_kernel, dim3((count + 255) / 256), dim3(256), 0, s, bodies, count, eye[0], eye[1], eye[2], T, highestVariant, variantOf);
}

} // namespace sge
