// svo_kernels_match.hip — the exact 2-nearest-neighbour Hamming search of the descriptor index (include/svo.h, "Descriptor index";
// the integer rules are in svo_match.hpp).
//
// k_desc_match: grid = row chunks x query tiles, one wave per block, one lane per query.  A lane holds its query's eight dwords in
//   VGPRs for the whole walk.  An index row is the same for all 64 lanes, so it is read through a wave-uniform address — the kernel's
//   arguments, blockIdx and the loop counter only — which the compiler turns into scalar loads: the row's eight dwords and its id
//   arrive in SGPRs and feed the VALU as scalar operands.  Per row and lane: 8 XORs, 8 popcounts and their sum, the key, and
//   match_update — 38 VALU instructions as built (DESIGN.md has the count against the issue floor).  The lane's (k1, k2) leaves as one 16-byte store per (query, chunk).
// k_desc_match_merge: one wave per query.  Lane l folds chunks l, l + 64, ... with match_merge (the id of a partial state's best is
//   ids[its row]), a butterfly of match_merge folds the 64 lanes — the rule is symmetric and the chunks are disjoint, so every order
//   gives the definition's answer — and lane 0 writes the 32-byte result row as two 16-byte stores.
// No LDS, no atomics.
#include "svo_match_internal.hpp"

#define MATCH_BLOCK 64                                // one wave per block, one lane per query
__global__ void __launch_bounds__(MATCH_BLOCK) k_desc_match(const uint32_t* __restrict__ desc, const uint64_t* __restrict__ ids,
                                                            const uint32_t* __restrict__ query, int n, MatchRange r,
                                                            MatchPartial* __restrict__ part) {
    const int q = blockIdx.y * MATCH_BLOCK + threadIdx.x;
    if (q >= n) return;                               // a lane beyond n reads nothing and writes nothing
    int r0, r1;
    match_chunk_rows(r, blockIdx.x, r0, r1);
    uint32_t qd[8];
    match_load_query(query, q, qd);
    MatchState s = match_empty();
#pragma unroll 4
    for (int row = r0; row < r1; row++) {             // row, and so both addresses below, are wave-uniform
        const uint4* rp = reinterpret_cast<const uint4*>(desc + (size_t)row * 8);
        match_update(s, match_make_key(match_dist(qd, rp[0], rp[1]), (uint32_t)row), ids[row]);
    }
    part[(size_t)q * r.n_chunks + blockIdx.x] = MatchPartial{s.k1, s.k2};
}

static __device__ __forceinline__ MatchState match_load_partial(const MatchPartial p, const uint64_t* __restrict__ ids) {
    return MatchState{p.k1, p.k2, match_key_none(p.k1) ? 0 : ids[match_key_row(p.k1)]};
}

__global__ void __launch_bounds__(64) k_desc_match_merge(const MatchPartial* __restrict__ part, const uint64_t* __restrict__ ids, int n, int n_chunks,
                                                         svo_desc_match* __restrict__ out) {
    const int q = blockIdx.x;                         // < n: the grid is n blocks
    const int lane = threadIdx.x;
    MatchState s = match_empty();
    const MatchPartial* mine = part + (size_t)q * n_chunks;
    for (int j = lane; j < n_chunks; j += 64) s = match_merge(s, match_load_partial(mine[j], ids));
    for (int off = 32; off > 0; off >>= 1) {
        MatchState t;
        t.k1 = __shfl_xor((unsigned long long)s.k1, off, 64);
        t.k2 = __shfl_xor((unsigned long long)s.k2, off, 64);
        t.id1 = __shfl_xor((unsigned long long)s.id1, off, 64);
        s = match_merge(s, t);
    }
    if (lane != 0) return;
    const int32_t row = match_key_row(s.k1), row2 = match_key_row(s.k2);
    const uint64_t id2 = row2 < 0 ? 0 : ids[row2];
    const uint32_t dists = match_key_dist(s.k1) | match_key_dist(s.k2) << 16;      // dist, dist2: two uint16, little-endian
    uint4* o = reinterpret_cast<uint4*>(out + q);
    o[0] = make_uint4((uint32_t)s.id1, (uint32_t)(s.id1 >> 32), (uint32_t)id2, (uint32_t)(id2 >> 32));
    o[1] = make_uint4((uint32_t)row, (uint32_t)row2, dists, 0u);
}

void launch_desc_match(const uint32_t* desc, const uint64_t* ids, const uint32_t* query, int n, const MatchRange& r, MatchPartial* part, hipStream_t s) {
    if (n <= 0 || r.n_chunks <= 0) return;
    hipLaunchKernelGGL(k_desc_match, dim3(r.n_chunks, (n + MATCH_BLOCK - 1) / MATCH_BLOCK), dim3(MATCH_BLOCK), 0, s, desc, ids, query, n, r, part);
}

void launch_desc_match_merge(const MatchPartial* part, const uint64_t* ids, int n, const MatchRange& r, svo_desc_match* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_desc_match_merge, dim3(n), dim3(64), 0, s, part, ids, n, r.n_chunks, out);
}
