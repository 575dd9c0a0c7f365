// svo_kernels_guide.hip — the guided search of the descriptor index (include/svo.h, "Guided search"; the rules are in svo_guide.hpp,
// the search's integer rules in svo_match.hpp).
//
// k_guide_project: one lane per row of [row_lo, row_hi).  It reads the row's 16-byte point, projects it with the prior in f64
//   (guide_project) and writes one float2 to uv[row]; an invisible row gets (+inf, +inf).
// k_desc_match_guided: k_desc_match with the gate in front.  grid = row chunks x query tiles, one wave per block, one lane per query
//   slot; lane `slot` serves query order[slot] and holds its eight dwords and its pixel in VGPRs.  A row's projection, descriptor and
//   id are read through wave-uniform addresses, so they arrive in SGPRs.  Rows go eight at a time: their eight projections are
//   loaded together (one scalar-load latency per eight rows instead of one per row: the walk is bound by that latency), each lane
//   tests each against its pixel (two subtractions, two compares), and the __ballots of the compares say whether any lane admits
//   it.  When no lane admits any of the eight the wave skips them with one uniform branch; a row nobody admits costs no descriptor load and no popcount.  For a row somebody
//   admits every lane computes the distance and the admitting lanes alone call match_update.  The lane's (k1, k2) leaves as one
//   16-byte store per (query, chunk) under the query's own number, so k_desc_match_merge, k_reloc_select and the PnP kernels run
//   unchanged behind it.
// No LDS, no atomics.
#include "svo_guide_internal.hpp"

#define GUIDE_PROJECT_BLOCK 256
__global__ void __launch_bounds__(GUIDE_PROJECT_BLOCK) k_guide_project(const RelocPoint* __restrict__ points, GuidePose g, int row_lo, int row_hi,
                                                                       float2* __restrict__ uv) {
    const int row = row_lo + (int)(blockIdx.x * GUIDE_PROJECT_BLOCK + threadIdx.x);    // row_hi <= 2^24: no overflow
    if (row >= row_hi) return;
    const float4 p = reinterpret_cast<const float4*>(points)[row];
    float u, v;
    guide_project(g, p.x, p.y, p.z, __float_as_int(p.w), u, v);
    uv[row] = make_float2(u, v);
}

// one row somebody admits: row, and so both addresses, are wave-uniform
static __device__ __forceinline__ void guided_row(MatchState& s, const uint32_t (&qd)[8], const uint32_t* __restrict__ desc,
                                                  const uint64_t* __restrict__ ids, int row, bool admits) {
    const uint4* rp = reinterpret_cast<const uint4*>(desc + (size_t)row * 8);
    const match_key k = match_make_key(match_dist(qd, rp[0], rp[1]), (uint32_t)row);
    const uint64_t id = ids[row];
    if (admits) match_update(s, k, id);
}

// the lanes that admit the row projected to p: the gate's two compares balloted one by one and ANDed as masks, which leaves each
// compare's lane mask where the instruction wrote it (a ballot of the ANDed flag costs two more VALU instructions per row)
static __device__ __forceinline__ unsigned long long guided_ballot(const float2 p, const float2 px, float radius) {
    return __ballot(guide_admits_axis(p.x, px.x, radius)) & __ballot(guide_admits_axis(p.y, px.y, radius));
}

#ifndef GUIDED_GROUP
#define GUIDED_GROUP 8                                // rows whose projections one scalar load brings in (DESIGN.md has 4, 8 and 16 timed)
#endif
#define GUIDED_BLOCK 64                               // one wave per block, one lane per query slot
__global__ void __launch_bounds__(GUIDED_BLOCK) k_desc_match_guided(const uint32_t* __restrict__ desc, const uint64_t* __restrict__ ids,
                                                                    const float2* __restrict__ uv, const uint32_t* __restrict__ query,
                                                                    const float2* __restrict__ qxy, const int32_t* __restrict__ order, int n,
                                                                    float radius, MatchRange r, MatchPartial* __restrict__ part) {
    const int slot = blockIdx.y * GUIDED_BLOCK + threadIdx.x;
    if (slot >= n) return;                            // a lane beyond n reads nothing, writes nothing and takes no part in a ballot
    const int q = order[slot];
    int r0, r1;
    match_chunk_rows(r, blockIdx.x, r0, r1);
    uint32_t qd[8];
    match_load_query(query, q, qd);
    const float2 px = qxy[q];
    MatchState s = match_empty();
    int row = r0;
    for (; row + GUIDED_GROUP <= r1; row += GUIDED_GROUP) {
        float2 p[GUIDED_GROUP];
        unsigned long long b[GUIDED_GROUP], any = 0;
#pragma unroll
        for (int i = 0; i < GUIDED_GROUP; i++) p[i] = uv[row + i];
#pragma unroll
        for (int i = 0; i < GUIDED_GROUP; i++) { b[i] = guided_ballot(p[i], px, radius); any |= b[i]; }
        if (any == 0) continue;                       // wave-uniform: nobody wants any row of the group
#pragma unroll
        for (int i = 0; i < GUIDED_GROUP; i++)
            if (b[i]) guided_row(s, qd, desc, ids, row + i, guide_admits(p[i].x, p[i].y, px.x, px.y, radius));
    }
    for (; row < r1; row++) {
        const float2 p = uv[row];
        if (guided_ballot(p, px, radius) == 0) continue;
        guided_row(s, qd, desc, ids, row, guide_admits(p.x, p.y, px.x, px.y, radius));
    }
    part[(size_t)q * r.n_chunks + blockIdx.x] = MatchPartial{s.k1, s.k2};
}

void launch_guide_project(const RelocPoint* points, const GuidePose& g, int row_lo, int row_hi, float2* uv, hipStream_t s) {
    if (row_hi <= row_lo) return;
    const int blocks = (row_hi - row_lo + GUIDE_PROJECT_BLOCK - 1) / GUIDE_PROJECT_BLOCK;
    hipLaunchKernelGGL(k_guide_project, dim3(blocks), dim3(GUIDE_PROJECT_BLOCK), 0, s, points, g, row_lo, row_hi, uv);
}

void launch_desc_match_guided(const uint32_t* desc, const uint64_t* ids, const float2* uv, const uint32_t* query, const float2* qxy,
                              const int32_t* order, int n, float radius, const MatchRange& r, MatchPartial* part, hipStream_t s) {
    if (n <= 0 || r.n_chunks <= 0) return;
    hipLaunchKernelGGL(k_desc_match_guided, dim3(r.n_chunks, (n + GUIDED_BLOCK - 1) / GUIDED_BLOCK), dim3(GUIDED_BLOCK), 0, s, desc, ids, uv, query,
                       qxy, order, n, radius, r, part);
}
