// svo_kernels_fuse.hip — the landmark fusion's kernels (include/svo.h, "Landmark fusion"; the rules are in svo_fuse.hpp, the search's
// integer rules in svo_match.hpp).  All run on the index's stream, as separate launches the stream orders: no kernel waits for
// another workgroup.  The pairing between the search and the map step is k_align_pairs (svo_kernels_align.hip), unchanged.
//
// k_desc_match_near: k_desc_match_guided with a 3-D gate.  grid = row chunks x source tiles, one wave per block, one lane per source
//   row, in row order.  The lane holds its row's eight descriptor dwords and its point in VGPRs, read from the index itself.  A
//   destination row's point, descriptor and id are read through wave-uniform addresses, so they arrive in SGPRs.  Rows go
//   NEAR_GROUP at a time: their 16-byte points are loaded together, each lane tests each against its own point (three subtractions,
//   three compares), each axis is balloted and the masks ANDed; a destination row without a point clears its mask.  When no lane
//   admits any row of the group the wave skips it with one uniform branch, before any descriptor load or popcount.  For a row
//   somebody admits every lane computes the distance and the admitting lanes alone call match_update.  The lane's (k1, k2) leaves as
//   one 16-byte store per (source row, chunk), so k_desc_match_merge runs unchanged behind it.  No LDS, no atomics.
// k_fuse_map: one lane per pair.  from = ids[pair_src], to = ids[pair_dst], both lists written whole before anything is relabelled;
//   n_same and n_fused by ballot, popcount and one integer atomicAdd per wave.
// k_fuse_insert: one lane per list entry, fuse_table_insert with atomicCAS and atomicMin on the slot.  The slots hold list positions
//   and are keyed through from[], which nothing writes while the table lives.
// k_fuse_sweep: one lane per row of the relabel span.  The id is loaded coalesced, probed (fuse_table_find) and stored only where it
//   changes; the changed rows are counted by ballot, popcount and one integer atomicAdd per wave, spread over FUSE_COUNT_SLOTS cache
//   lines.  No LDS.
// As built for gfx950 (no scratch, no spills, no AGPRs, no LDS; tests/test_fuse_code_object.py has the counts).
#include "svo_fuse_internal.hpp"

#ifndef NEAR_GROUP
#define NEAR_GROUP 4                                  // rows whose points one scalar load brings in, 64 bytes (DESIGN.md has 2, 4, 8 and 16 timed: alike)
#endif
#define NEAR_BLOCK 64                                 // one wave per block, one lane per source row
#define FUSE_BLOCK 256

// the lanes that admit the destination point p: one ballot per axis, ANDed as masks (guided_ballot's form); has: the lane's own row
// carries a point.  p.w, the destination's tag, is wave-uniform.
static __device__ __forceinline__ unsigned long long near_ballot(const float4 p, const float4 sp, bool has, float radius) {
    const unsigned long long b = __ballot(has && fuse_admits_axis(p.x, sp.x, radius)) & __ballot(fuse_admits_axis(p.y, sp.y, radius)) &
                                 __ballot(fuse_admits_axis(p.z, sp.z, radius));
    return __float_as_int(p.w) != FUSE_POINT_NONE ? b : 0ull;
}

// one row somebody admits: row, and so both addresses, are wave-uniform
static __device__ __forceinline__ void near_row(MatchState& s, const uint32_t (&qd)[8], const uint32_t* __restrict__ desc,
                                                const uint64_t* __restrict__ ids, int row, bool admits) {
    const uint4* rp = reinterpret_cast<const uint4*>(desc + (size_t)row * 8);
    const match_key k = match_make_key(match_dist(qd, rp[0], rp[1]), (uint32_t)row);
    const uint64_t id = ids[row];
    if (admits) match_update(s, k, id);
}

__global__ void __launch_bounds__(NEAR_BLOCK) k_desc_match_near(const uint32_t* __restrict__ desc, const uint64_t* __restrict__ ids,
                                                                const float4* __restrict__ points, int src_row, int n, float radius,
                                                                MatchRange r, MatchPartial* __restrict__ part) {
    const int q = blockIdx.y * NEAR_BLOCK + threadIdx.x;
    if (q >= n) return;                               // a lane beyond n reads nothing, writes nothing and takes no part in a ballot
    int r0, r1;
    match_chunk_rows(r, blockIdx.x, r0, r1);
    uint32_t qd[8];
    match_load_query(desc, src_row + q, qd);          // the query is the source row's own descriptor: nothing is uploaded
    const float4 sp = points[src_row + q];
    const bool has = __float_as_int(sp.w) != FUSE_POINT_NONE;
    const unsigned long long me = 1ull << threadIdx.x;
    MatchState s = match_empty();
    int row = r0;
    for (; row + NEAR_GROUP <= r1; row += NEAR_GROUP) {
        float4 p[NEAR_GROUP];
        unsigned long long b[NEAR_GROUP], any = 0;
#pragma unroll
        for (int i = 0; i < NEAR_GROUP; i++) p[i] = points[row + i];
#pragma unroll
        for (int i = 0; i < NEAR_GROUP; i++) { b[i] = near_ballot(p[i], sp, has, radius); any |= b[i]; }
        if (any == 0) continue;                       // wave-uniform: nobody wants any row of the group
#pragma unroll
        for (int i = 0; i < NEAR_GROUP; i++)
            if (b[i]) near_row(s, qd, desc, ids, row + i, (b[i] & me) != 0);
    }
    for (; row < r1; row++) {
        const unsigned long long b = near_ballot(points[row], sp, has, radius);
        if (b == 0) continue;
        near_row(s, qd, desc, ids, row, (b & me) != 0);
    }
    part[(size_t)q * r.n_chunks + blockIdx.x] = MatchPartial{s.k1, s.k2};
}

__global__ void __launch_bounds__(FUSE_BLOCK) k_fuse_map(const int32_t* __restrict__ n_pairs, int cap, const int32_t* __restrict__ pair_src,
                                                        const int32_t* __restrict__ pair_dst, const uint64_t* __restrict__ ids,
                                                        uint64_t* __restrict__ from, uint64_t* __restrict__ to, FuseCtl* ctl) {
    const int c = (int)(blockIdx.x * FUSE_BLOCK + threadIdx.x);
    const int n = *n_pairs < cap ? *n_pairs : cap;    // the lists hold no more
    bool same = false, fused = false;
    if (c < n) {
        const uint64_t f = ids[pair_src[c]], t = ids[pair_dst[c]];    // rows of the index: k_align_pairs wrote them
        from[c] = f; to[c] = t;
        fused = fuse_maps(f, t);
        same = !fused;
    }
    const int n_same = __popcll(__ballot(same)), n_fused = __popcll(__ballot(fused));
    if ((threadIdx.x & 63) == 0) {
        if (n_same) atomicAdd(&ctl->n_same, n_same);
        if (n_fused) atomicAdd(&ctl->n_fused, n_fused);
    }
}

struct FuseAtomicSlot {
    __device__ int32_t cas(int32_t* p, int32_t expect, int32_t v) const { return atomicCAS(p, expect, v); }
    __device__ void min(int32_t* p, int32_t v) const { atomicMin(p, v); }
};

__global__ void __launch_bounds__(FUSE_BLOCK) k_fuse_insert(const uint64_t* __restrict__ from, const uint64_t* __restrict__ to,
                                                           const int32_t* __restrict__ n_dev, int n, int32_t* table, uint32_t mask, FuseCtl* ctl) {
    const int c = (int)(blockIdx.x * FUSE_BLOCK + threadIdx.x);       // n <= 2^20: no overflow
    if (n_dev) n = *n_dev < n ? *n_dev : n;
    if (c >= n) return;
    if (!fuse_table_insert(table, mask, from, to, c, FuseAtomicSlot{})) ctl->table_full = 1;
}

__global__ void __launch_bounds__(FUSE_BLOCK) k_fuse_sweep(const uint64_t* __restrict__ from, const uint64_t* __restrict__ to,
                                                          const int32_t* __restrict__ table, uint32_t mask, uint64_t* __restrict__ ids, int row_lo,
                                                          int row_hi, FuseCtl* ctl) {
    const int row = row_lo + (int)(blockIdx.x * FUSE_BLOCK + threadIdx.x);         // row_hi <= 2^24: no overflow
    bool changed = false;
    if (row < row_hi) {
        const int32_t at = fuse_table_find(table, mask, from, ids[row]);
        if (at >= 0) { ids[row] = to[at]; changed = true; }           // an inserted entry has to != from: the id changes
    }
    const int n_changed = __popcll(__ballot(changed));
    if ((threadIdx.x & 63) == 0 && n_changed) atomicAdd(&ctl->counts[blockIdx.x % FUSE_COUNT_SLOTS].n_rows_relabelled, n_changed);
}

void launch_desc_match_near(const uint32_t* desc, const uint64_t* ids, const RelocPoint* points, int src_row, int n, float radius,
                            const MatchRange& r, MatchPartial* part, hipStream_t s) {
    if (n <= 0 || r.n_chunks <= 0) return;
    hipLaunchKernelGGL(k_desc_match_near, dim3(r.n_chunks, (n + NEAR_BLOCK - 1) / NEAR_BLOCK), dim3(NEAR_BLOCK), 0, s, desc, ids,
                       reinterpret_cast<const float4*>(points), src_row, n, radius, r, part);
}

static inline int fuse_blocks(int n) { return (n + FUSE_BLOCK - 1) / FUSE_BLOCK; }

void launch_fuse_map(const int32_t* n_pairs, int cap, const int32_t* pair_src, const int32_t* pair_dst, const uint64_t* ids, uint64_t* from,
                     uint64_t* to, FuseCtl* ctl, hipStream_t s) {
    if (cap <= 0) return;
    hipLaunchKernelGGL(k_fuse_map, dim3(fuse_blocks(cap)), dim3(FUSE_BLOCK), 0, s, n_pairs, cap, pair_src, pair_dst, ids, from, to, ctl);
}

void launch_fuse_relabel(const uint64_t* from, const uint64_t* to, const int32_t* n_dev, int n, int32_t* table, uint32_t slots, uint64_t* ids,
                         int row_lo, int row_hi, FuseCtl* ctl, hipStream_t s) {
    if (n <= 0 || row_hi <= row_lo) return;
    hipLaunchKernelGGL(k_fuse_insert, dim3(fuse_blocks(n)), dim3(FUSE_BLOCK), 0, s, from, to, n_dev, n, table, slots - 1, ctl);
    hipLaunchKernelGGL(k_fuse_sweep, dim3(fuse_blocks(row_hi - row_lo)), dim3(FUSE_BLOCK), 0, s, from, to, table, slots - 1, ids, row_lo, row_hi, ctl);
}
