// Acceleration structures of a crowd whose characters name one of several meshes (include/sge_amd_variant_blas.h; DESIGN.md
// 3.5a): the refit over the RAGGED streams the variant skin launch writes, and closest-hit queries against characters of mixed
// variants. One topology per variant (sge_blas_variant_build); character c's boxes are bounds[c][rowStride][6] with rowStride the
// largest entryCount_v + 1, and charVariant[c] says whose structure they describe (0xFF: none).
//
// blas_refit_ragged_kernel — blas_refit_kernel (sge_blas.hip) once per uploaded variant, over that variant's list of the plan the
// skin launch left on the device: persistent workgroups, a ticket counter, one LDS tile, the lane-sequential walk and
// blasFinishCharacter are the same code (sge_blas_dev.hpp). What differs is where a character's vertices start: ticket k is
// character c = lists[listBase[v] + k], its positions start at vertex off[c]. That chain must never stand in front of a tile's
// position loads (memory loads return in order), so (a) it is read with SCALAR loads, which have a counter of their
// own and do not queue behind the vector loads in flight, and (b) it is resolved a whole character ahead: the ticket drawn at the
// start of character i names the character AFTER the next one, its (c, off[c]) are requested in the last step of character i and
// sit in scalar registers through character i + 1, at whose end the first tile behind them is requested.
//
// blas_intersect_ragged_kernel / blas_world_boxes_ragged_kernel — blas_intersect_kernel / blas_world_boxes_kernel with a
// device table of one row per variant (topology, index buffer, uvs): the wavefront loads the character's record and row when it
// enters the character (wave-uniform, scalar loads), the vertex base from off[c], the root row at entryCount_v. Tie rules and
// the three-level instance scan are unchanged. A character with record 0xFF gets a NaN world box (no slab test passes it, min /
// max reductions ignore it) and is left at once when named.
#include <algorithm>
#include "sge_blas_dev.hpp"
#include "sge_blas_trace_dev.hpp"

namespace sge {

namespace {

constexpr int kWave = 64;
constexpr int kNoVariant = 0xFF;
typedef float v4f __attribute__((ext_vector_type(4)));

// wave-uniform loads from memory no launch in flight writes: through the constant address space, i.e. the scalar cache
__device__ __forceinline__ int uload(const int* p) { return *reinterpret_cast<const __attribute__((address_space(4))) int*>((size_t)p); }
__device__ __forceinline__ long long uload(const long long* p) { return *reinterpret_cast<const __attribute__((address_space(4))) long long*>((size_t)p); }
__device__ __forceinline__ int uniformInt(int x) { return __builtin_amdgcn_readfirstlane(x); }

} // namespace

template <int STRIDE, int TILE>
__global__ __launch_bounds__(kBlasRefitBlock) void blas_refit_ragged_kernel(DevBlas B, int variant, const SkinPlan* __restrict__ plan,
                                                                            const int* __restrict__ lists, const long long* __restrict__ off,
                                                                            const float* __restrict__ positions, float* __restrict__ bounds,
                                                                            int rowStride, uint8_t* __restrict__ charVariant, int* __restrict__ queue) {
    extern __shared__ float lds[];
    // the host does not know how many characters the variant holds: the grid is what stays resident, the count is the plan's
    const int chars = uload(plan->kept + variant);
    if ((int)blockIdx.x >= chars) return; // (uniform over the workgroup, in front of every barrier)
    const int* list = lists + uload(plan->listBase + variant);
    const int rows = B.entryCount + 1, tid = threadIdx.x;
    float* tab = lds;
    float* X = lds + rows * 6; // Y = X + TILE, Z = X + 2 * TILE
    int* trs = reinterpret_cast<int*>(X + 3 * TILE);
    int& sNext = trs[B.tileCount + 1]; // list position a ticket names, behind the round ranges (see blas_refit_kernel)
    int* topo = trs + B.tileCount + 2;
    blasTableInit(tab, rows, tid, kBlasRefitBlock);
    blasTopoStage(B, topo, tid, kBlasRefitBlock);
    for (int i = tid; i <= B.tileCount; i += kBlasRefitBlock) trs[i] = B.tileRoundStart[i];
    if (tid == 0) sNext = (int)gridDim.x + atomicAdd(queue, 1); // this workgroup's second character
    __syncthreads();
    const int lane = tid & (kWave - 1), wave = tid / kWave;
    constexpr int kWaves = kBlasRefitBlock / kWave, kPerThread = TILE / kBlasRefitBlock;
    const int n = B.tileCount, lastRound = trs[n] - 1;

    float px[kPerThread], py[kPerThread], pz[kPerThread];
    // a character's first vertex may be odd in the packed layout: nothing here assumes more than the 4-byte (packed) or 16-byte
    // (padded: one vertex) alignment of a single vertex
    auto fetchPos = [&](long long firstVertex, int tile) {
        const float* P = positions + (size_t)firstVertex * STRIDE;
        const int base = tile * B.tileVerts, nv = min(B.tileVerts, B.vertexCount - base);
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int v = min(tid + k * kBlasRefitBlock, nv - 1); // past the end: reload the last vertex (never stored), no branch
            const float* p = P + (size_t)(base + v) * STRIDE;
            if (STRIDE == 4) { const v4f q = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p)); px[k] = q.x; py[k] = q.y; pz[k] = q.z; }
            else { px[k] = __builtin_nontemporal_load(p); py[k] = __builtin_nontemporal_load(p + 1); pz[k] = __builtin_nontemporal_load(p + 2); }
        }
    };
    // list position -> (character, first vertex); a position past the list resolves to the list's last character, whose
    // vertices may be loaded (inside the stream: the plan kept it) and are never used
    auto resolve = [&](int k, int& c, long long& o) {
        c = uload(list + uniformInt(min(k, chars - 1)));
        o = uload(off + c);
    };
    int kNext = uniformInt(sNext);
    int c, cNext;
    long long o, oNext;
    resolve((int)blockIdx.x, c, o);
    resolve(kNext, cNext, oNext);
    int tile = c % n, done = 0, ticket = 0;
    fetchPos(o, tile);
    while (true) {
        const int nv = min(B.tileVerts, B.vertexCount - tile * B.tileVerts);
        if (done == 0 && tid == 0) ticket = atomicAdd(queue, 1); // the character after the next; kept in a register until the last step
        __syncthreads(); // the previous step's rounds have read X/Y/Z; a finished character's table has been re-initialised
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int v = tid + k * kBlasRefitBlock;
            if (v < nv) { X[v] = px[k]; X[v + TILE] = py[k]; X[v + 2 * TILE] = pz[k]; }
        }
        const bool last = done + 1 == n;
        if (last && tid == 0) sNext = (int)gridDim.x + ticket; // read below in this step, behind the barrier
        __syncthreads();
        const int rEnd = trs[tile + 1];
        int r = trs[tile] + wave;
        BlasRound R;
        if (r < rEnd) blasFetchRound(B, r, lastRound, lane, R); // wave-uniform; a wavefront without a round in this tile loads nothing
        // the next step: this character's next tile, or the next character's first — its offset has been in a scalar register for
        // a whole character
        const int tileNext = last ? cNext % n : (tile + 1 == n ? 0 : tile + 1);
        fetchPos(last ? oNext : o, tileNext); // unconditional; after the last step: unused
        int k2 = 0, c2 = 0;
        long long o2 = 0;
        if (last) { // scalar loads: not behind the position loads just issued
            k2 = uniformInt(sNext);
            resolve(k2, c2, o2);
        }
        if (r < rEnd) blasWalk<TILE>(tab, rows, X, R); // wave-uniform
        for (r += kWaves; r < rEnd; r += kWaves) { // only when a tile has more rounds than the workgroup has wavefronts
            blasFetchRound(B, r, lastRound, lane, R);
            blasWalk<TILE>(tab, rows, X, R);
        }
        if (last) {
            blasFinishCharacter(B, topo, tab, rows, tid, kBlasRefitBlock, bounds + (size_t)c * rowStride * 6);
            if (tid == 0) charVariant[c] = (uint8_t)variant;
            if (kNext >= chars) return;
            c = cNext; o = oNext;
            kNext = k2; cNext = c2; oNext = o2;
            done = 0;
        } else {
            ++done;
        }
        tile = tileNext;
    }
}

namespace {

template <int TILE>
int launchRaggedTile(const RaggedRefitLaunch& L, int v, int grid, size_t lds, hipStream_t s) {
    static bool attrSet[kMaxDevices] = {};
    const int devSlot = currentDeviceSlot();
    if (!attrSet[devSlot]) {
        SGE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(blas_refit_ragged_kernel<3, TILE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBlasMaxLdsBytes + 64));
        SGE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(blas_refit_ragged_kernel<4, TILE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBlasMaxLdsBytes + 64));
        attrSet[devSlot] = true;
    }
    const float* p = reinterpret_cast<const float*>(L.positions);
    int* queue = L.queues + v * 16;
    if (L.layout == SGE_LAYOUT_PADDED16)
        hipLaunchKernelGGL((blas_refit_ragged_kernel<4, TILE>), dim3(grid), dim3(kBlasRefitBlock), lds, s, L.blas[v], v, L.plan, L.lists, L.off, p, L.bounds, L.rowStride, L.charVariant, queue);
    else
        hipLaunchKernelGGL((blas_refit_ragged_kernel<3, TILE>), dim3(grid), dim3(kBlasRefitBlock), lds, s, L.blas[v], v, L.plan, L.lists, L.off, p, L.bounds, L.rowStride, L.charVariant, queue);
    return SGE_OK;
}

} // namespace

int launch_blas_refit_ragged(const RaggedRefitLaunch& L, hipStream_t s) {
    if (L.chars <= 0 || L.variants <= 0) return SGE_OK;
    for (int v = 0; v < L.variants; ++v) // (in front of everything that is enqueued)
        if (L.blas[v].entryCount + 1 > L.rowStride) { set_error("refit over mesh variants: a variant's structure has more rows than the box table's stride"); return SGE_ERR_STATE; }
    SGE_HIP(hipMemsetAsync(L.queues, 0, (size_t)SGE_MAX_MESH_VARIANTS * 64, s));
    SGE_HIP(hipMemsetAsync(L.charVariant, kNoVariant, (size_t)L.chars, s)); // a character the plan dropped keeps no structure
    const int cus = currentDeviceCUs();
    for (int v = 0; v < L.variants; ++v) {
        const DevBlas& B = L.blas[v];
        const size_t lds = blasRefitLdsBytes(B.entryCount, B.tileCount, B.tileCap) + blasTopoBytes(B.wideCount, B.levels) + 16; // + the ticket slot
        // as many workgroups as stay resident together (launch_blas_refit's rule), at most one per character of the crowd: how many of
        // them find a character of this variant is the plan's to say
        const int perCU = (int)std::max<size_t>(1, std::min<size_t>(4, (size_t)(160 * 1024) / (lds + 256)));
        const int grid = std::min(L.chars, cus * perCU);
        int rc;
        switch (B.tileCap) {
        case 3072: rc = launchRaggedTile<3072>(L, v, grid, lds, s); break;
        case 2048: rc = launchRaggedTile<2048>(L, v, grid, lds, s); break;
        default: rc = launchRaggedTile<4096>(L, v, grid, lds, s); break;
        }
        if (rc != SGE_OK) return rc;
    }
    return SGE_OK;
}

// ---------------------------------------------------------------------------
// world boxes and closest hit over characters of mixed variants
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void blas_world_boxes_ragged_kernel(RaggedTrace G, float* worldBoxes) {
    const BlasTrace& T = G.T;
    const int i = blockIdx.x * kWave + threadIdx.x;
    F3 mn{kFloatMax, kFloatMax, kFloatMax}, mx{-kFloatMax, -kFloatMax, -kFloatMax};
    if (i < T.chars) {
        const int v = G.charVariant[i];
        float* o = worldBoxes + (size_t)i * 6;
        if (v != kNoVariant) {
            const Aff M = loadInstance(T.instances, i);
            const int root = G.table[v].blas.entryCount;
            const float* bx = T.bounds + ((size_t)i * G.rowStride + root) * 6;
            for (int k = 0; k < 8; ++k) {
                const F3 c = affMulPoint(M, F3{bx[(k & 1) ? 3 : 0], bx[(k & 2) ? 4 : 1], bx[(k & 4) ? 5 : 2]});
                mn = vmin(mn, c);
                mx = vmax(mx, c);
            }
            o[0] = mn.x; o[1] = mn.y; o[2] = mn.z; o[3] = mx.x; o[4] = mx.y; o[5] = mx.z;
        } else { // no structure: a box no slab test passes and no min / max reduction takes up
            const float nan = __builtin_nanf("");
            o[0] = nan; o[1] = nan; o[2] = nan; o[3] = nan; o[4] = nan; o[5] = nan;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        mn = vmin(mn, F3{__shfl_xor(mn.x, off, kWave), __shfl_xor(mn.y, off, kWave), __shfl_xor(mn.z, off, kWave)});
        mx = vmax(mx, F3{__shfl_xor(mx.x, off, kWave), __shfl_xor(mx.y, off, kWave), __shfl_xor(mx.z, off, kWave)});
    }
    if (threadIdx.x == 0) {
        float* o = worldBoxes + ((size_t)T.chars + blockIdx.x) * 6;
        o[0] = mn.x; o[1] = mn.y; o[2] = mn.z; o[3] = mx.x; o[4] = mx.y; o[5] = mx.z;
    }
}

// blas_intersect_kernel with the topology, index buffer, uvs, vertex base and row count taken per character: see there for the
// traversal and the tie rules, which are the same lines.
template <int STRIDE>
__global__ __launch_bounds__(kWave) void blas_intersect_ragged_kernel(RaggedTrace G, const sge_blas_ray* rays, int n, sge_blas_hit* hits) {
    __shared__ int stack[kBlasStack];
    const BlasTrace& T = G.T;
    const int lane = threadIdx.x;
    const sge_blas_ray R = rays[blockIdx.x];
    sge_blas_hit H{};
    H.primitive = -1;
    H.instance = -1;
    if (R.instance >= T.chars) { if (lane == 0) hits[blockIdx.x] = H; return; }
    const F3 wo{R.origin[0], R.origin[1], R.origin[2]}, wd{R.direction[0], R.direction[1], R.direction[2]};
    const float tMin = smax(R.minDistance, 0.0f);

    float bestT = R.maxDistance, bestU = 0, bestV = 0;
    uint32_t bestPrim = 0;
    int bestInst = -1;

    auto traverse = [&](int instAny) {
        const int inst = uniformInt(instAny);
        // the record the newest refit left: whose structure the boxes describe — loaded on entry, for every character entered
        const int v = uniformInt((int)G.charVariant[inst]);
        if (v == kNoVariant) return; // dropped at the capacity cut, or never refitted: no boxes, no vertices
        const DevVariantBlas* row = G.table + v;
        const int* wideFirst = row->blas.wideFirst;
        const int2* entryLink = row->blas.entryLink;
        const uint32_t* slotIndices = row->blas.slotIndices;
        const uint32_t* slotTriangle = row->blas.slotTriangle;
        const Aff M = loadInstance(T.instances, inst);
        const Inv3 Mi = inverse3(M);
        const F3 o = mul3(Mi, wo - M.c3), d = mul3(Mi, wd);
        const F3 inv = invDir(d);
        const float* P = reinterpret_cast<const float*>(T.positions) + (size_t)G.off[inst] * STRIDE;
        const float* boxes = T.bounds + (size_t)inst * G.rowStride * 6;
        unsigned long long best = ((unsigned long long)__float_as_uint(bestT) << 32) | ((bestInst < 0 || inst < bestInst) ? 0xffffffffull : 0ull);
        float u0 = 0, v0 = 0;
        bool found = false;
        int sp = 1;
        if (lane == 0) stack[0] = 0;
        __syncthreads();
        while (sp > 0) {
            const int w = stack[sp - 1];
            --sp;
            __syncthreads();
            const int first = wideFirst[w], cnt = wideFirst[w + 1] - first;
            bool pass = false;
            int2 link = make_int2(0, 0);
            if (lane < cnt) {
                link = entryLink[first + lane];
                pass = slabPass(boxes + (size_t)(first + lane) * 6, o, inv, tMin, __uint_as_float((unsigned)(best >> 32)));
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
                const int firstSlot = ~__shfl(link.x, src, kWave), count = __shfl(link.y, src, kWave);
                unsigned long long key = ~0ull;
                float u = 0, vv = 0;
                if (lane < count) {
                    const uint32_t* ix = slotIndices + (size_t)(firstSlot + lane) * 3;
                    const F3 p0 = loadP<STRIDE>(P, ix[0]), p1 = loadP<STRIDE>(P, ix[1]), p2 = loadP<STRIDE>(P, ix[2]);
                    float t;
                    if (rayTriangleUV(o, d, p0, p1, p2, 1e-6f, t, u, vv) && t >= tMin && t <= R.maxDistance)
                        key = ((unsigned long long)__float_as_uint(t) << 32) | slotTriangle[firstSlot + lane];
                }
                unsigned long long k = key;
                for (int off = 32; off > 0; off >>= 1) {
                    const unsigned lo32 = __shfl_xor((unsigned)k, off, kWave), hi32 = __shfl_xor((unsigned)(k >> 32), off, kWave);
                    const unsigned long long other = ((unsigned long long)hi32 << 32) | lo32;
                    k = other < k ? other : k;
                }
                if (k != ~0ull && k < best) {
                    best = k;
                    found = true;
                    const int winner = __ffsll((long long)__ballot(key == k)) - 1;
                    u0 = __shfl(u, winner, kWave);
                    v0 = __shfl(vv, winner, kWave);
                }
            }
            __syncthreads();
        }
        if (found) {
            bestT = __uint_as_float((unsigned)(best >> 32));
            bestPrim = (uint32_t)best;
            bestU = u0; bestV = v0;
            bestInst = inst;
        }
    };

    if (R.instance >= 0) {
        traverse(R.instance);
    } else if (T.worldBoxesValid && T.instOrder) {
        const F3 inv = invDir(wd);
        const int groups = (T.chars + kWave - 1) / kWave, supers = (groups + kWave - 1) / kWave;
        for (int sbase = 0; sbase < supers; sbase += kWave) {
            const int sg = sbase + lane;
            unsigned long long sm = __ballot(sg < supers && slabPass(T.superBoxes + (size_t)sg * 6, wo, inv, tMin, bestT));
            while (sm) {
                const int ssrc = __ffsll((long long)sm) - 1;
                sm &= sm - 1;
                const int g = (sbase + ssrc) * kWave + lane;
                unsigned long long gm = __ballot(g < groups && slabPass(T.groupBoxes + (size_t)g * 6, wo, inv, tMin, bestT));
                while (gm) {
                    const int gsrc = __ffsll((long long)gm) - 1;
                    gm &= gm - 1;
                    const int slot = ((sbase + ssrc) * kWave + gsrc) * kWave + lane;
                    const int inst = slot < T.chars ? T.instOrder[slot] : -1;
                    const bool pass = inst >= 0 && slabPass(T.worldBoxes + (size_t)inst * 6, wo, inv, tMin, bestT);
                    unsigned long long m = __ballot(pass);
                    while (m) {
                        const int src = __ffsll((long long)m) - 1;
                        m &= m - 1;
                        traverse(__shfl(inst, src, kWave));
                    }
                }
            }
        }
    } else if (T.worldBoxesValid) {
        const F3 inv = invDir(wd);
        const int groups = (T.chars + kWave - 1) / kWave;
        const float* groupBoxes = T.worldBoxes + (size_t)T.chars * 6;
        for (int gbase = 0; gbase < groups; gbase += kWave) {
            const int g = gbase + lane;
            unsigned long long gm = __ballot(g < groups && slabPass(groupBoxes + (size_t)g * 6, wo, inv, tMin, bestT));
            while (gm) {
                const int gsrc = __ffsll((long long)gm) - 1;
                gm &= gm - 1;
                const int base = (gbase + gsrc) * kWave, i = base + lane;
                const bool pass = i < T.chars && slabPass(T.worldBoxes + (size_t)i * 6, wo, inv, tMin, bestT);
                unsigned long long m = __ballot(pass);
                while (m) {
                    const int src = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    traverse(base + src);
                }
            }
        }
    }
    if (lane != 0) return;
    if (bestInst >= 0) {
        const DevVariantBlas* row = G.table + G.charVariant[bestInst];
        const Aff M = loadInstance(T.instances, bestInst);
        const size_t vbase = (size_t)G.off[bestInst];
        const float* P = reinterpret_cast<const float*>(T.positions) + vbase * STRIDE;
        const uint32_t* ix = row->indices + (size_t)bestPrim * 3;
        const uint32_t i0 = ix[0], i1 = ix[1], i2 = ix[2];
        const F3 w0 = affMulPoint(M, loadP<STRIDE>(P, i0)), w1 = affMulPoint(M, loadP<STRIDE>(P, i1)), w2 = affMulPoint(M, loadP<STRIDE>(P, i2));
        F3 N = normalize(cross(w1 - w0, w2 - w0));
        if (dot(N, wd) > 0.0f) N = -N;
        const float* NB = reinterpret_cast<const float*>(T.normals) + vbase * STRIDE;
        const float* TB = T.tangents + vbase * 4;
        const float bx = bestU, by = bestV, bw = 1.0f - bx - by;
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
        H.hit = 1; H.primitive = (int32_t)bestPrim; H.instance = bestInst; H.distance = bestT; H.bary[0] = bx; H.bary[1] = by;
        H.geomNormal[0] = N.x; H.geomNormal[1] = N.y; H.geomNormal[2] = N.z;
        H.normal[0] = nW.x; H.normal[1] = nW.y; H.normal[2] = nW.z;
        H.tangent[0] = tW.x; H.tangent[1] = tW.y; H.tangent[2] = tW.z;
        H.bitangent[0] = bW.x; H.bitangent[1] = bW.y; H.bitangent[2] = bW.z;
        const float* uvs = row->uvs;
        if (uvs) {
            const float* a0 = uvs + (size_t)i0 * 2; const float* a1 = uvs + (size_t)i1 * 2; const float* a2 = uvs + (size_t)i2 * 2;
            H.uv[0] = (a0[0] * bw + a1[0] * bx) + a2[0] * by;
            H.uv[1] = (a0[1] * bw + a1[1] * bx) + a2[1] * by;
        }
    }
    hits[blockIdx.x] = H;
}

void launch_blas_world_boxes_ragged(const RaggedTrace& R, float* worldBoxes, hipStream_t s) {
    if (R.T.chars > 0) hipLaunchKernelGGL(blas_world_boxes_ragged_kernel, dim3((R.T.chars + kWave - 1) / kWave), dim3(kWave), 0, s, R, worldBoxes);
}

void launch_blas_intersect_ragged(RaggedTrace R, const sge_blas_ray* d_rays, int n, sge_blas_hit* d_hits, bool anyInstance, hipStream_t s) {
    BlasTrace& T = R.T;
    T.worldBoxesValid = anyInstance && T.worldBoxes != nullptr ? 1 : 0;
    if (n <= 0) return;
    if (anyInstance && T.chars > 0 && !T.instOrder && !T.worldBoxes) T.worldBoxesValid = 0; // nothing refreshed: rays without an instance miss
    if (T.layout == SGE_LAYOUT_PADDED16) hipLaunchKernelGGL((blas_intersect_ragged_kernel<4>), dim3(n), dim3(kWave), 0, s, R, d_rays, n, d_hits);
    else hipLaunchKernelGGL((blas_intersect_ragged_kernel<3>), dim3(n), dim3(kWave), 0, s, R, d_rays, n, d_hits);
}

} // namespace sge
