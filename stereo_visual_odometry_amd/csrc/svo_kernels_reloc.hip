// svo_kernels_reloc.hip — the relocaliser's selection stage (include/svo.h, "Relocalisation"; the rules are in svo_reloc.hpp).
//
// k_reloc_select: ONE block of 1024 threads behind k_desc_match_merge on the index's stream, n <= 4096 queries.
//   1. Accept (rule 1), 1024 queries per pass: a thread reads its query's result row and the tag of the best row's point.  The
//      accepted queries are packed in increasing j into LDS as (id, key = dist << 16 | j): ballot, prefix inside the wave by
//      popcount of the lower lanes, the 16 wave totals through LDS, a running base across the passes.
//   2. One pixel per landmark (rule 2), over the accepted list only: a thread holds up to four entries in registers and walks the
//      whole list — every lane reads the same LDS address, a broadcast, four entries per step — marking an entry that loses to
//      another of its id.  O(accepted^2) compares in all; the walk is built for 1, 2, 3 or 4 entries per thread.
//   3. The survivors are packed the same way (the accepted list is in increasing j, so the candidates are too) and written out:
//      the pixel and the point of candidate c go to element c of the stage context's PnP inputs, (query, row) to the result lists.
//   4. Thread 0 writes the count and the state row's fields the frame pipeline's compaction writes: the live flag, the track count,
//      or fail_reason 2 (too few tracks) when the gate fails, which every PnP kernel behind takes as "nothing to do".
// Static LDS: 32 KiB of ids + 16 KiB of keys + the wave totals.  No scratch, no atomics.
#include "svo_reloc_internal.hpp"

#define RELOC_THREADS 1024
#define RELOC_WAVES (RELOC_THREADS / 64)
#define RELOC_PASSES (SVO_RELOC_MAX_QUERIES / RELOC_THREADS)
#define RELOC_STEP 4                                  // entries of the accepted list one step of rule 2's walk loads

// Order-preserving ranks inside the block: the number of set flags below this thread, and the block's total.  Every thread calls it;
// the second barrier frees `totals` for the next call.
static __device__ __forceinline__ int reloc_rank(bool flag, int lane, int wave, int* totals, int& all) {
    const unsigned long long b = __ballot(flag);
    if (lane == 0) totals[wave] = __popcll(b);
    __syncthreads();
    int before = 0;
    all = 0;
#pragma unroll
    for (int w = 0; w < RELOC_WAVES; w++) {
        const int t = totals[w];
        before += w < wave ? t : 0;
        all += t;
    }
    __syncthreads();
    return before + __popcll(b & ((1ull << lane) - 1ull));
}

// Rule 2's walk for a thread's first P entries: the whole accepted list (padded to n_walk), RELOC_STEP entries' loads in flight
// together — every lane reads the same addresses, and a walk of single loads is bound by the LDS latency.
template <int P>
static __device__ __forceinline__ void reloc_walk(const uint64_t* s_id, const uint32_t* s_key, int n_walk, const uint64_t (&id_e)[RELOC_PASSES],
                                                  const uint32_t (&key_e)[RELOC_PASSES], bool (&lost)[RELOC_PASSES]) {
    for (int b0 = 0; b0 < n_walk; b0 += RELOC_STEP) {
        uint64_t id_b[RELOC_STEP];
        uint32_t key_b[RELOC_STEP];
#pragma unroll
        for (int k = 0; k < RELOC_STEP; k++) { id_b[k] = s_id[b0 + k]; key_b[k] = s_key[b0 + k]; }
#pragma unroll
        for (int k = 0; k < RELOC_STEP; k++) {
#pragma unroll
            for (int p = 0; p < P; p++) lost[p] = lost[p] || reloc_loses(id_e[p], key_e[p], id_b[k], key_b[k]);
        }
    }
}

__global__ void __launch_bounds__(RELOC_THREADS) k_reloc_select(RelocArgs a) {
    __shared__ uint64_t s_id[SVO_RELOC_MAX_QUERIES];
    __shared__ uint32_t s_key[SVO_RELOC_MAX_QUERIES];
    __shared__ int s_tot[RELOC_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n < SVO_RELOC_MAX_QUERIES ? a.n : SVO_RELOC_MAX_QUERIES;      // the LDS lists hold no more
    // ---- rule 1, packed in increasing j
    int n_acc = 0;
    for (int j0 = 0; j0 < n; j0 += RELOC_THREADS) {
        const int j = j0 + tid;
        bool acc = false;
        uint64_t id = 0;
        uint32_t key = 0;
        if (j < n) {
            const uint4* m = reinterpret_cast<const uint4*>(a.match + j);
            const uint4 lo = m[0], hi = m[1];           // id, id2 | row, row2, dist | dist2 << 16, reserved
            const int32_t row = (int32_t)hi.x, dist = (int32_t)(hi.z & 0xFFFFu), dist2 = (int32_t)(hi.z >> 16);
            const int32_t tag = row >= 0 ? a.points[row].tag : SVO_RELOC_POINT_NONE;
            acc = reloc_accept(row, tag, dist, dist2, a.rule);
            id = (uint64_t)lo.y << 32 | lo.x;
            key = reloc_key(dist, j);
        }
        int all;
        const int at = n_acc + reloc_rank(acc, lane, wave, s_tot, all);
        if (acc) { s_id[at] = id; s_key[at] = key; }    // at < n <= 4096
        n_acc += all;
    }
    // the list padded to a multiple of RELOC_STEP with entries nobody loses to (the largest key), so that the walk below needs no tail
    const int n_walk = (n_acc + RELOC_STEP - 1) / RELOC_STEP * RELOC_STEP;         // <= 4096
    if (tid < RELOC_STEP && n_acc + tid < n_walk) { s_id[n_acc + tid] = 0; s_key[n_acc + tid] = 0xFFFFFFFFu; }
    __syncthreads();
    // ---- rule 2: entry e = p * 1024 + tid of the accepted list, against the whole list
    uint64_t id_e[RELOC_PASSES];
    uint32_t key_e[RELOC_PASSES];
    bool lost[RELOC_PASSES];
#pragma unroll
    for (int p = 0; p < RELOC_PASSES; p++) {
        const int e = p * RELOC_THREADS + tid;
        id_e[p] = e < n_acc ? s_id[e] : 0;
        key_e[p] = e < n_acc ? s_key[e] : 0;            // key 0 loses to nothing
        lost[p] = false;
    }
    const int n_pass = (n_acc + RELOC_THREADS - 1) / RELOC_THREADS;                // block-uniform: the entries beyond it are empty
    if (n_pass <= 1) reloc_walk<1>(s_id, s_key, n_walk, id_e, key_e, lost);
    else if (n_pass == 2) reloc_walk<2>(s_id, s_key, n_walk, id_e, key_e, lost);
    else if (n_pass == 3) reloc_walk<3>(s_id, s_key, n_walk, id_e, key_e, lost);
    else reloc_walk<RELOC_PASSES>(s_id, s_key, n_walk, id_e, key_e, lost);
    // ---- rule 3: the survivors in increasing j
    int n_cand = 0;
#pragma unroll
    for (int p = 0; p < RELOC_PASSES; p++) {
        if (p * RELOC_THREADS >= n_acc) break;          // block-uniform
        const bool keep = p * RELOC_THREADS + tid < n_acc && !lost[p];
        int all;
        const int c = n_cand + reloc_rank(keep, lane, wave, s_tot, all);
        if (keep) {
            const int j = reloc_key_query(key_e[p]);
            const int32_t row = a.match[j].row;         // accepted: a row of the index that carries a point
            const RelocPoint pt = a.points[row];
            a.cand_query[c] = j; a.cand_row[c] = row;
            a.out_xy[c] = a.xy[j];
            a.out_xyz[3 * c] = pt.x; a.out_xyz[3 * c + 1] = pt.y; a.out_xyz[3 * c + 2] = pt.z;
        }
        n_cand += all;
    }
    // ---- rule 4, and the state row as the frame pipeline's compaction leaves it
    if (tid == 0) {
        *a.n_cand = n_cand;
        SeqState& s = *a.st;
        s.active = 1; s.n_tracks = n_cand; s.n_feat = n_cand;
        s.fail_reason = n_cand >= a.min_candidates ? 0 : 2;
    }
}

void launch_reloc_select(const RelocArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_reloc_select, dim3(1), dim3(RELOC_THREADS), 0, s, a);
}
