// svo_kernels_reloc_batch.hip — the batched relocalisation (include/svo.h, "Batched relocalisation"): many cameras against one index
// in one call.  The rules are the single calls' — svo_match.hpp, svo_guide.hpp, svo_reloc.hpp — and the plan is svo_reloc_batch.hpp's.
//
// k_desc_match_guided_batch: the guided search with the projection fused in; no array of projections exists.  grid = (row chunk,
//   camera of the group, tile group); a block of up to 16 waves serves up to 1024 query slots of ONE camera, lane `slot` the query
//   order[begin[camera] + slot] (or begin[camera] + slot without an order), whose eight dwords and pixel it holds in VGPRs.  The
//   block walks its chunk tile by tile, RB_TILE_ROWS rows each: every thread projects rows of the tile with the camera's prior
//   (guide_project, f64) into LDS; after a barrier each wave walks the tile as k_desc_match_guided walks a chunk — eight projections
//   at a time, now through one LDS address for all lanes (a broadcast), the two ballots per row, the uniform skip; descriptors and
//   ids still come through wave-uniform global addresses — and a second barrier frees the tile.  A lane without a query (slot >= n)
//   projects and meets every barrier like the others; its pixel is NaN, which no compare admits, so it is in no ballot, and it
//   neither loads a query nor stores a state.  A block whose first slot is beyond its camera's slice leaves as a whole, before the
//   first barrier.  The lane's (k1, k2) leaves under the query's number inside the group, so k_desc_match_merge runs unchanged.
//   LDS: RB_TILE_ROWS x 8 = 8192 bytes, whatever the chunk's length.
// k_reloc_batch_order: one block per camera sorts (cell key, j) of its slice in LDS — bitonic, 4096 x 8 bytes = 32768 — and writes
//   the slice of the order as global query numbers.
// k_reloc_select_batch: k_reloc_select's rules (svo_kernels_reloc.hip), restated with one block per camera: its slice of the result
//   rows and pixels, row `camera` of the state rows, rows camera x CAP of the PnP inputs, its slice of the candidate lists (queries
//   numbered inside the slice).  LDS as there: 32 KiB of ids + 16 KiB of keys + 64 bytes of wave totals = 49216.
// k_reloc_batch_inliers: the PnP's inlier flags of every camera's candidates, from the stage context's rows into the cameras' slices.
// No scratch, no atomics.
#include "svo_reloc_batch_internal.hpp"

// ---------------------------------------------------------------------------------------------------------------- the guided search
// one row somebody admits: row, and so both addresses, are wave-uniform (svo_kernels_guide.hip, guided_row)
static __device__ __forceinline__ void rb_row(MatchState& s, const uint32_t (&qd)[8], const uint32_t* __restrict__ desc,
                                              const uint64_t* __restrict__ ids, int row, bool admits) {
    const uint4* rp = reinterpret_cast<const uint4*>(desc + (size_t)row * 8);
    const match_key k = match_make_key(match_dist(qd, rp[0], rp[1]), (uint32_t)row);
    const uint64_t id = ids[row];
    if (admits) match_update(s, k, id);
}
static __device__ __forceinline__ unsigned long long rb_ballot(const float2 p, const float2 px, float radius) {
    return __ballot(guide_admits_axis(p.x, px.x, radius)) & __ballot(guide_admits_axis(p.y, px.y, radius));
}

#define RB_GROUP 8                                    // projections one step of the walk reads together, as k_desc_match_guided
__global__ void __launch_bounds__(RB_BLOCK_SLOTS) k_desc_match_guided_batch(RelocBatchSearch a) {
    __shared__ float2 s_uv[RB_TILE_ROWS];
    const int cam = a.cam0 + blockIdx.y;
    const int q_lo = a.begin[cam], n = a.begin[cam + 1] - q_lo;
    const int slot0 = blockIdx.z * blockDim.x;
    if (slot0 >= n) return;                           // the whole block: nobody is left at a barrier
    const int slot = slot0 + threadIdx.x;
    const bool live = slot < n;
    const RelocBatchCam c = a.cams[cam];
    const float radius = c.radius;
    int r0, r1;
    rb_chunk_rows(a.r, blockIdx.x, r0, r1);
    int q = 0;
    uint32_t qd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float2 px = make_float2(__builtin_nanf(""), __builtin_nanf(""));               // admits nothing: a dead lane is in no ballot
    if (live) {
        q = a.order ? a.order[q_lo + slot] : q_lo + slot;
        match_load_query(a.query, q, qd);
        px = a.qxy[q];
    }
    MatchState s = match_empty();
    for (int t0 = r0; t0 < r1; t0 += RB_TILE_ROWS) {
        const int tn = r1 - t0 < RB_TILE_ROWS ? r1 - t0 : RB_TILE_ROWS;
        for (int i = threadIdx.x; i < tn; i += blockDim.x) {
            const float4 p = reinterpret_cast<const float4*>(a.points)[t0 + i];
            float u, v;
            guide_project(c.pose, p.x, p.y, p.z, __float_as_int(p.w), u, v);
            s_uv[i] = make_float2(u, v);
        }
        __syncthreads();
        int i = 0;
        for (; i + RB_GROUP <= tn; i += RB_GROUP) {
            float2 p[RB_GROUP];
            unsigned long long b[RB_GROUP], any = 0;
#pragma unroll
            for (int k = 0; k < RB_GROUP; k++) p[k] = s_uv[i + k];
#pragma unroll
            for (int k = 0; k < RB_GROUP; k++) { b[k] = rb_ballot(p[k], px, radius); any |= b[k]; }
            if (any == 0) continue;                   // wave-uniform: nobody wants any row of the group
#pragma unroll
            for (int k = 0; k < RB_GROUP; k++)
                if (b[k]) rb_row(s, qd, a.desc, a.ids, t0 + i + k, guide_admits(p[k].x, p[k].y, px.x, px.y, radius));
        }
        for (; i < tn; i++) {
            const float2 p = s_uv[i];
            if (rb_ballot(p, px, radius) == 0) continue;
            rb_row(s, qd, a.desc, a.ids, t0 + i, guide_admits(p.x, p.y, px.x, px.y, radius));
        }
        __syncthreads();                              // the tile is free for the next projections
    }
    if (live) a.part[(size_t)(q - a.q0) * a.r.n_chunks + blockIdx.x] = MatchPartial{s.k1, s.k2};
}

void launch_desc_match_guided_batch(const RelocBatchSearch& a, const RbGrid& g, hipStream_t s) {
    if (g.x <= 0) return;
    hipLaunchKernelGGL(k_desc_match_guided_batch, dim3(g.x, g.y, g.z), dim3(g.threads), 0, s, a);
}

// -------------------------------------------------------------------------------------------------------------------- the lane order
#define RB_ORDER_THREADS 1024
__global__ void __launch_bounds__(RB_ORDER_THREADS) k_reloc_batch_order(const float2* __restrict__ qxy, const int32_t* __restrict__ begin,
                                                                        const RelocBatchCam* __restrict__ cams, int32_t* __restrict__ order) {
    __shared__ uint64_t s_e[RB_MAX_SLICE];
    const int cam = blockIdx.x, tid = threadIdx.x;
    const int q_lo = begin[cam];
    int n = begin[cam + 1] - q_lo;
    n = n < RB_MAX_SLICE ? n : RB_MAX_SLICE;          // the LDS list holds no more
    if (n <= 0) return;                               // the whole block
    const float radius = cams[cam].radius;
    int P = 64;                                       // the sorted length: a power of two that holds the slice
    while (P < n) P *= 2;
    for (int j = tid; j < P; j += RB_ORDER_THREADS) {
        uint64_t e = ~(uint64_t)0;                    // padding: behind every entry of the slice
        if (j < n) { const float2 p = qxy[q_lo + j]; e = rb_order_entry(rb_cell_key(p.x, p.y, radius), j); }
        s_e[j] = e;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += RB_ORDER_THREADS) {
                const int o = i ^ j;
                if (o > i) {
                    const uint64_t x = s_e[i], y = s_e[o];
                    if ((x > y) == ((i & k) == 0)) { s_e[i] = y; s_e[o] = x; }
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < n; i += RB_ORDER_THREADS) order[q_lo + i] = q_lo + rb_entry_query(s_e[i]);
}

void launch_reloc_batch_order(const float2* qxy, const int32_t* begin, const RelocBatchCam* cams, int n_cameras, int32_t* order, hipStream_t s) {
    if (n_cameras <= 0) return;
    hipLaunchKernelGGL(k_reloc_batch_order, dim3(n_cameras), dim3(RB_ORDER_THREADS), 0, s, qxy, begin, cams, order);
}

// -------------------------------------------------------------------------------------------------------------------- the selection
#define RBS_THREADS 1024
#define RBS_WAVES (RBS_THREADS / 64)
#define RBS_PASSES (SVO_RELOC_MAX_QUERIES / RBS_THREADS)
// entries of the accepted list one step of rule 2's walk loads: 2, where the lone kernel has 4.  With the cameras' offsets beside the
// arguments, 4 costs 18 spilled SGPRs; two blocks of other cameras share the CU and cover the LDS latency a deeper step would
#define RBS_STEP 2

// order-preserving ranks inside the block (svo_kernels_reloc.hip, reloc_rank): every thread calls it
static __device__ __forceinline__ int rbs_rank(bool flag, int lane, int wave, int* totals, int& all) {
    const unsigned long long b = __ballot(flag);
    if (lane == 0) totals[wave] = __popcll(b);
    __syncthreads();
    int before = 0;
    all = 0;
#pragma unroll
    for (int w = 0; w < RBS_WAVES; w++) {
        const int t = totals[w];
        before += w < wave ? t : 0;
        all += t;
    }
    __syncthreads();
    return before + __popcll(b & ((1ull << lane) - 1ull));
}

// rule 2's walk for a thread's first P entries (svo_kernels_reloc.hip, reloc_walk)
template <int P>
static __device__ __forceinline__ void rbs_walk(const uint64_t* s_id, const uint32_t* s_key, int n_walk, const uint64_t (&id_e)[RBS_PASSES],
                                                const uint32_t (&key_e)[RBS_PASSES], bool (&lost)[RBS_PASSES]) {
    for (int b0 = 0; b0 < n_walk; b0 += RBS_STEP) {
        uint64_t id_b[RBS_STEP];
        uint32_t key_b[RBS_STEP];
#pragma unroll
        for (int k = 0; k < RBS_STEP; k++) { id_b[k] = s_id[b0 + k]; key_b[k] = s_key[b0 + k]; }
#pragma unroll
        for (int k = 0; k < RBS_STEP; k++) {
#pragma unroll
            for (int p = 0; p < P; p++) lost[p] = lost[p] || reloc_loses(id_e[p], key_e[p], id_b[k], key_b[k]);
        }
    }
}

__global__ void __launch_bounds__(RBS_THREADS) k_reloc_select_batch(RelocBatchSelect a) {
    __shared__ uint64_t s_id[SVO_RELOC_MAX_QUERIES];
    __shared__ uint32_t s_key[SVO_RELOC_MAX_QUERIES];
    __shared__ int s_tot[RBS_WAVES];
    const int cam = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q_lo = a.begin[cam];
    int n = a.begin[cam + 1] - q_lo;
    n = n < SVO_RELOC_MAX_QUERIES ? n : SVO_RELOC_MAX_QUERIES;                      // the LDS lists hold no more
    // The camera's own: query j of its slice is entry q_lo + j of the result rows, the pixels and the lists, candidate c is element
    // cam * cap + c of the PnP inputs.  The offsets are applied where an entry is touched: pointers derived up front would have to
    // live in SGPRs across the walk, which has none to spare.
    // ---- rule 1, packed in increasing j
    int n_acc = 0;
    for (int j0 = 0; j0 < n; j0 += RBS_THREADS) {
        const int j = j0 + tid;
        bool acc = false;
        uint64_t id = 0;
        uint32_t key = 0;
        if (j < n) {
            const uint4* m = reinterpret_cast<const uint4*>(a.match + q_lo + j);
            const uint4 lo = m[0], hi = m[1];           // id, id2 | row, row2, dist | dist2 << 16, reserved
            const int32_t row = (int32_t)hi.x, dist = (int32_t)(hi.z & 0xFFFFu), dist2 = (int32_t)(hi.z >> 16);
            const int32_t tag = row >= 0 ? a.points[row].tag : SVO_RELOC_POINT_NONE;
            acc = reloc_accept(row, tag, dist, dist2, a.rule);
            id = (uint64_t)lo.y << 32 | lo.x;
            key = reloc_key(dist, j);
        }
        int all;
        const int at = n_acc + rbs_rank(acc, lane, wave, s_tot, all);
        if (acc) { s_id[at] = id; s_key[at] = key; }    // at < n <= 4096
        n_acc += all;
    }
    // the list padded to a multiple of RBS_STEP with entries nobody loses to (the largest key)
    const int n_walk = (n_acc + RBS_STEP - 1) / RBS_STEP * RBS_STEP;               // <= 4096
    if (tid < RBS_STEP && n_acc + tid < n_walk) { s_id[n_acc + tid] = 0; s_key[n_acc + tid] = 0xFFFFFFFFu; }
    __syncthreads();
    // ---- rule 2: entry e = p * 1024 + tid of the accepted list, against the whole list
    uint64_t id_e[RBS_PASSES];
    uint32_t key_e[RBS_PASSES];
    bool lost[RBS_PASSES];
#pragma unroll
    for (int p = 0; p < RBS_PASSES; p++) {
        const int e = p * RBS_THREADS + tid;
        id_e[p] = e < n_acc ? s_id[e] : 0;
        key_e[p] = e < n_acc ? s_key[e] : 0;            // key 0 loses to nothing
        lost[p] = false;
    }
    const int n_pass = (n_acc + RBS_THREADS - 1) / RBS_THREADS;                    // block-uniform
    if (n_pass <= 1) rbs_walk<1>(s_id, s_key, n_walk, id_e, key_e, lost);
    else if (n_pass == 2) rbs_walk<2>(s_id, s_key, n_walk, id_e, key_e, lost);
    else if (n_pass == 3) rbs_walk<3>(s_id, s_key, n_walk, id_e, key_e, lost);
    else rbs_walk<RBS_PASSES>(s_id, s_key, n_walk, id_e, key_e, lost);
    // ---- rule 3: the survivors in increasing j
    int n_cand = 0;
#pragma unroll
    for (int p = 0; p < RBS_PASSES; p++) {
        if (p * RBS_THREADS >= n_acc) break;            // block-uniform
        const bool keep = p * RBS_THREADS + tid < n_acc && !lost[p];
        int all;
        const int c = n_cand + rbs_rank(keep, lane, wave, s_tot, all);
        if (keep) {
            const int j = reloc_key_query(key_e[p]);
            const int32_t row = a.match[q_lo + j].row;  // accepted: a row of the index that carries a point
            const RelocPoint pt = a.points[row];
            const size_t o = (size_t)cam * a.cap + c;
            a.cand_query[q_lo + c] = j; a.cand_row[q_lo + c] = row;
            a.out_xy[o] = a.xy[q_lo + j];
            a.out_xyz[3 * o] = pt.x; a.out_xyz[3 * o + 1] = pt.y; a.out_xyz[3 * o + 2] = pt.z;
        }
        n_cand += all;
    }
    // ---- rule 4, and the state row as the frame pipeline's compaction leaves it
    if (tid == 0) {
        a.n_cand[cam] = n_cand;
        SeqState& s = a.st[cam];
        s.active = 1; s.n_tracks = n_cand; s.n_feat = n_cand;
        s.fail_reason = n_cand >= a.min_candidates ? 0 : 2;
    }
}

void launch_reloc_select_batch(const RelocBatchSelect& a, int n_cameras, hipStream_t s) {
    if (n_cameras <= 0) return;
    hipLaunchKernelGGL(k_reloc_select_batch, dim3(n_cameras), dim3(RBS_THREADS), 0, s, a);
}

// ---------------------------------------------------------------------------------------------------------------- the inlier flags
#define RB_INLIER_THREADS 256
__global__ void __launch_bounds__(RB_INLIER_THREADS) k_reloc_batch_inliers(const uint8_t* __restrict__ inlier, int cap, const int32_t* __restrict__ begin,
                                                                           const int32_t* __restrict__ n_cand, uint8_t* __restrict__ out) {
    const int cam = blockIdx.y, c = blockIdx.x * RB_INLIER_THREADS + threadIdx.x;
    if (c < n_cand[cam]) out[begin[cam] + c] = inlier[(size_t)cam * cap + c];      // n_cand <= the slice's length <= cap
}

void launch_reloc_batch_inliers(const uint8_t* inlier, int cap, const int32_t* begin, const int32_t* n_cand, int n_cameras, int max_slice,
                                uint8_t* out, hipStream_t s) {
    if (n_cameras <= 0 || max_slice <= 0) return;
    hipLaunchKernelGGL(k_reloc_batch_inliers, dim3((max_slice + RB_INLIER_THREADS - 1) / RB_INLIER_THREADS, n_cameras), dim3(RB_INLIER_THREADS), 0, s,
                       inlier, cap, begin, n_cand, out);
}
