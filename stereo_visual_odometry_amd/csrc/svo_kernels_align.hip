// svo_kernels_align.hip — the map alignment's kernels (include/svo.h, "Map alignment"; the rules are in svo_align.hpp and
// svo_reloc.hpp).  All three run behind k_desc_match_merge on the index's stream; none waits for another workgroup, none uses
// atomics, and every floating-point sum is taken in an order that depends on the pair numbers only.
//
// k_align_pairs: ONE block of 1024 threads, n <= 4096 source rows — k_reloc_select's accept, pack and walk restated, twice.
//   1. Accept (rule 2): a thread reads source row j's result row, the tag of the best row's point and the source row's own tag; the
//      accepted rows are packed in increasing j into LDS as (destination id, key = dist << 16 | j).
//   2. Rule 3: every entry against the whole list, two entries a step, an entry losing to a smaller key of its id.
//   3. The survivors are packed again, in place of the first list, as (source id, key), and walked the same way: rule 4.
//   4. The survivors of that, in increasing j, are the pairs: their rows into the two lists, their points as six floats into the
//      packed array, their inlier flags cleared; thread 0 writes the count and clears the result row.
//   Static LDS: 32 KiB of ids + 16 KiB of keys + the wave totals = 49 216 bytes, k_reloc_select's.
// k_align_score: one wave per hypothesis, four waves a block.  The wave draws its three pairs and solves Horn's closed form
//   wave-uniformly in f64 (every lane the same arithmetic: no broadcast), then its 64 lanes stride over the packed pairs and the
//   inliers are counted by ballot and popcount: one count and one model stored per hypothesis.  No LDS.
// k_align_fit: ONE block of 256 threads, 16 pairs a thread (pair c at thread c % 256).  The best hypothesis by (count, -h) through a
//   shuffle maximum; then up to refit_rounds times the inliers' centroids and centred cross-covariance as block-wide f64 sums — per
//   thread in increasing c, a xor butterfly inside the wave, the four wave sums added in order — the Jacobi on wave 0, the model
//   through LDS, the new inlier set; the flags, rms and the result row.  Static LDS: 880 bytes as laid out (4 x 16 doubles, the
//   model, the wave counts, the block-wide OR's word).
// As built for gfx950 (no scratch, no spills, no AGPRs; tests/test_align_code_object.py): k_align_pairs 51 VGPRs / 98 SGPRs /
// 49216 B LDS, k_align_score 124 / 36 / 0 B, k_align_fit 178 / 48 / 880 B.  The walks take two entries a step: with four, and with
// the lost flags as lane masks instead of a word, the pair kernel spilled SGPRs.
#include "svo_align_internal.hpp"

#define ALIGN_PAIR_THREADS 1024
#define ALIGN_PAIR_WAVES (ALIGN_PAIR_THREADS / 64)
#define ALIGN_PAIR_PASSES (ALIGN_MAX_ROWS / ALIGN_PAIR_THREADS)
#define ALIGN_STEP 2                                  // entries of a list one step of a walk loads
#define ALIGN_SCORE_WAVES 4
#define ALIGN_FIT_THREADS 256
#define ALIGN_FIT_WAVES (ALIGN_FIT_THREADS / 64)
#define ALIGN_FIT_PAIRS (ALIGN_MAX_ROWS / ALIGN_FIT_THREADS)

// reloc_rank (svo_kernels_reloc.hip): the number of set flags below this thread, and the block's total; every thread calls it
static __device__ __forceinline__ int align_rank(bool flag, int lane, int wave, int* totals, int& all) {
    const unsigned long long b = __ballot(flag);
    if (lane == 0) totals[wave] = __popcll(b);
    __syncthreads();
    int before = 0;
    all = 0;
#pragma unroll
    for (int w = 0; w < ALIGN_PAIR_WAVES; w++) {
        const int t = totals[w];
        before += w < wave ? t : 0;
        all += t;
    }
    __syncthreads();
    return before + __popcll(b & ((1ull << lane) - 1ull));
}

// reloc_walk: a thread's first P entries against the whole list (padded to n_walk), ALIGN_STEP broadcast loads in flight together
template <int P>
static __device__ __forceinline__ void align_walk(const uint64_t* s_id, const uint32_t* s_key, int n_walk, const uint64_t (&id_e)[ALIGN_PAIR_PASSES],
                                                  const uint32_t (&key_e)[ALIGN_PAIR_PASSES], uint32_t& lost) {
    for (int b0 = 0; b0 < n_walk; b0 += ALIGN_STEP) {
        uint64_t id_b[ALIGN_STEP];
        uint32_t key_b[ALIGN_STEP];
#pragma unroll
        for (int k = 0; k < ALIGN_STEP; k++) { id_b[k] = s_id[b0 + k]; key_b[k] = s_key[b0 + k]; }
#pragma unroll
        for (int k = 0; k < ALIGN_STEP; k++) {
#pragma unroll
            for (int p = 0; p < P; p++) lost |= (uint32_t)reloc_loses(id_e[p], key_e[p], id_b[k], key_b[k]) << p;
        }
    }
}

// One "smallest key per id" pass over the list s_id / s_key[0 .. n_list): pads the list, loads entry e = p * 1024 + tid into the
// thread's registers and marks the ones that lose (bit p of lost).  Every thread calls it; the list is complete in LDS when it returns.
static __device__ __forceinline__ void align_one_per_id(uint64_t* s_id, uint32_t* s_key, int n_list, int tid, uint64_t (&id_e)[ALIGN_PAIR_PASSES],
                                                        uint32_t (&key_e)[ALIGN_PAIR_PASSES], uint32_t& lost) {
    const int n_walk = (n_list + ALIGN_STEP - 1) / ALIGN_STEP * ALIGN_STEP;         // <= 4096
    if (tid < ALIGN_STEP && n_list + tid < n_walk) { s_id[n_list + tid] = 0; s_key[n_list + tid] = 0xFFFFFFFFu; }   // nobody loses to the largest key
    __syncthreads();
#pragma unroll
    for (int p = 0; p < ALIGN_PAIR_PASSES; p++) {
        const int e = p * ALIGN_PAIR_THREADS + tid;
        id_e[p] = e < n_list ? s_id[e] : 0;
        key_e[p] = e < n_list ? s_key[e] : 0;           // key 0 loses to nothing
    }
    lost = 0;
    const int n_pass = (n_list + ALIGN_PAIR_THREADS - 1) / ALIGN_PAIR_THREADS;      // block-uniform
    if (n_pass <= 1) align_walk<1>(s_id, s_key, n_walk, id_e, key_e, lost);
    else if (n_pass == 2) align_walk<2>(s_id, s_key, n_walk, id_e, key_e, lost);
    else if (n_pass == 3) align_walk<3>(s_id, s_key, n_walk, id_e, key_e, lost);
    else align_walk<ALIGN_PAIR_PASSES>(s_id, s_key, n_walk, id_e, key_e, lost);
}

__global__ void __launch_bounds__(ALIGN_PAIR_THREADS) k_align_pairs(AlignPairsArgs a) {
    __shared__ uint64_t s_id[ALIGN_MAX_ROWS];
    __shared__ uint32_t s_key[ALIGN_MAX_ROWS];
    __shared__ int s_tot[ALIGN_PAIR_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n < ALIGN_MAX_ROWS ? a.n : ALIGN_MAX_ROWS;                      // the LDS lists hold no more
    // ---- rule 2, packed in increasing j
    int n_acc = 0;
    for (int j0 = 0; j0 < n; j0 += ALIGN_PAIR_THREADS) {
        const int j = j0 + tid;
        bool acc = false;
        uint64_t id = 0;
        uint32_t key = 0;
        if (j < n) {
            const uint4* m = reinterpret_cast<const uint4*>(a.match + j);
            const uint4 lo = m[0], hi = m[1];           // id, id2 | row, row2, dist | dist2 << 16, reserved
            const int32_t row = (int32_t)hi.x, dist = (int32_t)(hi.z & 0xFFFFu), dist2 = (int32_t)(hi.z >> 16);
            const int32_t tag = row >= 0 ? a.points[row].tag : SVO_RELOC_POINT_NONE;
            acc = a.points[a.src_lo + j].tag != SVO_RELOC_POINT_NONE && reloc_accept(row, tag, dist, dist2, a.rule);
            id = (uint64_t)lo.y << 32 | lo.x;
            key = reloc_key(dist, j);
        }
        int all;
        const int at = n_acc + align_rank(acc, lane, wave, s_tot, all);
        if (acc) { s_id[at] = id; s_key[at] = key; }    // at < n <= 4096
        n_acc += all;
    }
    uint64_t id_e[ALIGN_PAIR_PASSES];
    uint32_t key_e[ALIGN_PAIR_PASSES];
    uint32_t lost;                                      // bit p: the thread's entry p loses (a word, not flags: lane masks would take SGPR pairs)
    // ---- rule 3: one source row per destination landmark
    align_one_per_id(s_id, s_key, n_acc, tid, id_e, key_e, lost);
    // ---- rule 4: the survivors, still in increasing j, under their source ids.  The first barrier inside align_rank comes after
    // every thread's walk, so the list is no longer read when the first entry is overwritten.
    int n_sur = 0;
#pragma unroll
    for (int p = 0; p < ALIGN_PAIR_PASSES; p++) {
        if (p * ALIGN_PAIR_THREADS >= n_acc) break;     // block-uniform
        const bool keep = p * ALIGN_PAIR_THREADS + tid < n_acc && !(lost >> p & 1u);
        int all;
        const int at = n_sur + align_rank(keep, lane, wave, s_tot, all);
        if (keep) { s_id[at] = a.ids[a.src_lo + reloc_key_query(key_e[p])]; s_key[at] = key_e[p]; }   // at <= its old place
        n_sur += all;
    }
    align_one_per_id(s_id, s_key, n_sur, tid, id_e, key_e, lost);
    // ---- rule 5: the pairs in increasing j
    int n_pairs = 0;
#pragma unroll
    for (int p = 0; p < ALIGN_PAIR_PASSES; p++) {
        if (p * ALIGN_PAIR_THREADS >= n_sur) break;     // block-uniform
        const bool keep = p * ALIGN_PAIR_THREADS + tid < n_sur && !(lost >> p & 1u);
        int all;
        const int c = n_pairs + align_rank(keep, lane, wave, s_tot, all);
        if (keep) {                                     // c < n_sur <= n
            const int j = reloc_key_query(key_e[p]);
            const int32_t row = a.match[j].row;         // accepted: a row of the index that carries a point
            const RelocPoint ps = a.points[a.src_lo + j], pd = a.points[row];
            a.pair_src[c] = a.src_lo + j; a.pair_dst[c] = row; a.pair_inlier[c] = 0;
            float2* pq = reinterpret_cast<float2*>(a.pairs + (size_t)c * ALIGN_PAIR_FLOATS);
            pq[0] = make_float2(ps.x, ps.y); pq[1] = make_float2(ps.z, pd.x); pq[2] = make_float2(pd.y, pd.z);
        }
        n_pairs += all;
    }
    if (tid == 0) {
        AlignOut o = {};
        o.n_pairs = n_pairs; o.best_hypothesis = -1;
        *a.out = o;
    }
}

void launch_align_pairs(const AlignPairsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_align_pairs, dim3(1), dim3(ALIGN_PAIR_THREADS), 0, s, a);
}

// a pair's six floats as three 8-byte loads
static __device__ __forceinline__ void align_load_pair(const float* pairs, int c, float (&pq)[ALIGN_PAIR_FLOATS]) {
    const float2* p = reinterpret_cast<const float2*>(pairs + (size_t)c * ALIGN_PAIR_FLOATS);
    const float2 a = p[0], b = p[1], d = p[2];
    pq[0] = a.x; pq[1] = a.y; pq[2] = b.x; pq[3] = b.y; pq[4] = d.x; pq[5] = d.y;
}

__global__ void __launch_bounds__(ALIGN_SCORE_WAVES * 64) k_align_score(AlignFitArgs a) {
    const int lane = threadIdx.x & 63;
    const int h = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * ALIGN_SCORE_WAVES + (threadIdx.x >> 6)));
    const int n_pairs = a.out->n_pairs;
    if (h >= a.hypotheses || n_pairs < a.min_pairs) return;                         // min_pairs >= 3: the sampler has its three
    int32_t pick[3];
    align_sample((uint32_t)h, n_pairs, pick);
    float p0[ALIGN_PAIR_FLOATS], p1[ALIGN_PAIR_FLOATS], p2[ALIGN_PAIR_FLOATS];
    align_load_pair(a.pairs, pick[0], p0); align_load_pair(a.pairs, pick[1], p1); align_load_pair(a.pairs, pick[2], p2);
    AlignModel m;
    align_model3(p0, p1, p2, m);
    int count = 0;
    for (int c0 = 0; c0 < n_pairs; c0 += 64) {
        const int c = c0 + lane;
        bool in = false;
        if (c < n_pairs) {
            float pq[ALIGN_PAIR_FLOATS];
            align_load_pair(a.pairs, c, pq);
            in = align_is_inlier(m, pq, a.dist2);
        }
        count += __popcll(__ballot(in));
    }
    if (!align_model_finite(m)) count = 0;
    if (lane == 0) { a.counts[h] = count; a.models[h] = m; }
}

void launch_align_score(const AlignFitArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_align_score, dim3((a.hypotheses + ALIGN_SCORE_WAVES - 1) / ALIGN_SCORE_WAVES), dim3(ALIGN_SCORE_WAVES * 64), 0, s, a);
}

// Block-wide sums of K doubles per thread in a fixed tree: a xor butterfly inside the wave (every lane ends with the wave's sum),
// then the wave sums added in wave order.  Every thread calls it and gets the totals.
template <int K>
static __device__ __forceinline__ void align_block_sum(double (&v)[K], double (*s_red)[16], int lane, int wave) {
#pragma unroll
    for (int k = 0; k < K; k++) {
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) v[k] += __shfl_xor(v[k], off);
        if (lane == 0) s_red[wave][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k];
    __syncthreads();
}
static __device__ __forceinline__ int align_block_count(uint32_t mask, int* s_cnt, int lane, int wave) {
    int v = __popc(mask);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
    if (lane == 0) s_cnt[wave] = v;
    __syncthreads();
    v = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    __syncthreads();
    return v;
}

// the thread's pairs within dist2 of m as bits (bit k: pair k * 256 + tid), and the sum of their squared residuals in increasing k
static __device__ __forceinline__ uint32_t align_classify(const AlignModel& m, const float* pairs, int n_pairs, int tid, double dist2, double& ss) {
    uint32_t mask = 0;
    ss = 0.;
    for (int k = 0; k < ALIGN_FIT_PAIRS; k++) {
        const int c = k * ALIGN_FIT_THREADS + tid;
        if (c >= n_pairs) break;
        float pq[ALIGN_PAIR_FLOATS];
        align_load_pair(pairs, c, pq);
        const double r2 = align_residual2(m, pq);
        if (r2 <= dist2) { mask |= 1u << k; ss += r2; }
    }
    return mask;
}

__global__ void __launch_bounds__(ALIGN_FIT_THREADS) k_align_fit(AlignFitArgs a) {
    __shared__ double s_red[ALIGN_FIT_WAVES][16];
    __shared__ AlignModel s_model;
    __shared__ int s_cnt[ALIGN_FIT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_pairs = a.out->n_pairs;
    if (n_pairs < a.min_pairs) return;                  // rule 5: k_align_pairs has written the result row
    // ---- rule 8: the largest count, at equal counts the smallest h.  count <= 4096 and h < 1024 share a word
    uint32_t best = 0;
#pragma unroll
    for (int k = 0; k < ALIGN_MAX_HYPOTHESES / ALIGN_FIT_THREADS; k++) {
        const int h = k * ALIGN_FIT_THREADS + tid;
        if (h < a.hypotheses) {
            const uint32_t key = (uint32_t)a.counts[h] << 10 | (uint32_t)(ALIGN_MAX_HYPOTHESES - 1 - h);
            best = key > best ? key : best;
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)best, off); best = o > best ? o : best; }
    if (lane == 0) s_cnt[wave] = (int)best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < ALIGN_FIT_WAVES; w++) best = (uint32_t)s_cnt[w] > best ? (uint32_t)s_cnt[w] : best;
    __syncthreads();
    const int best_h = ALIGN_MAX_HYPOTHESES - 1 - (int)(best & (ALIGN_MAX_HYPOTHESES - 1)), best_count = (int)(best >> 10);
    AlignModel m = a.models[best_h];
    // ---- rule 9
    double ss;
    uint32_t mask = align_classify(m, a.pairs, n_pairs, tid, a.dist2, ss);
    int n_in = align_block_count(mask, s_cnt, lane, wave), rounds = 0;
    for (int r = 0; r < a.refit_rounds && n_in >= 3; r++) {
        double c6[6] = {0, 0, 0, 0, 0, 0};
        for (int k = 0; k < ALIGN_FIT_PAIRS; k++) {
            if (!(mask >> k & 1u)) continue;
            float pq[ALIGN_PAIR_FLOATS];
            align_load_pair(a.pairs, k * ALIGN_FIT_THREADS + tid, pq);
#pragma unroll
            for (int i = 0; i < 6; i++) c6[i] += (double)pq[i];
        }
        align_block_sum<6>(c6, s_red, lane, wave);
        double cp[3], cq[3], s9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 3; i++) { cp[i] = c6[i] / (double)n_in; cq[i] = c6[3 + i] / (double)n_in; }
        for (int k = 0; k < ALIGN_FIT_PAIRS; k++) {
            if (!(mask >> k & 1u)) continue;
            float pq[ALIGN_PAIR_FLOATS];
            align_load_pair(a.pairs, k * ALIGN_FIT_THREADS + tid, pq);
#pragma unroll
            for (int i = 0; i < 3; i++) {
#pragma unroll
                for (int j = 0; j < 3; j++) s9[3 * i + j] += ((double)pq[i] - cp[i]) * ((double)pq[3 + j] - cq[j]);
            }
        }
        align_block_sum<9>(s9, s_red, lane, wave);
        if (wave == 0) {
            AlignModel fit;
            align_horn(cp, cq, s9, fit);
            if (lane == 0) s_model = fit;
        }
        __syncthreads();
        m = s_model;
        const uint32_t now = align_classify(m, a.pairs, n_pairs, tid, a.dist2, ss);
        const int changed = __syncthreads_or(now != mask);  // also: every thread has read s_model
        mask = now;
        n_in = align_block_count(mask, s_cnt, lane, wave);
        rounds++;
        if (!changed) break;
    }
    // ---- rule 10
    for (int k = 0; k < ALIGN_FIT_PAIRS; k++) {
        const int c = k * ALIGN_FIT_THREADS + tid;
        if (c < n_pairs) a.pair_inlier[c] = (uint8_t)(mask >> k & 1u);
    }
    double s1[1] = {ss};
    align_block_sum<1>(s1, s_red, lane, wave);
    if (tid == 0) {
        AlignOut o = {};
        o.n_pairs = n_pairs; o.n_inliers = n_in; o.best_hypothesis = best_h; o.best_count = best_count; o.refit_rounds_run = rounds;
        o.success = n_in >= a.min_pairs;
        if (o.success) {
#pragma unroll
            for (int i = 0; i < 9; i++) o.R[i] = m.R[i];
#pragma unroll
            for (int i = 0; i < 3; i++) o.t[i] = m.t[i];
            o.rms = sqrt(s1[0] / (double)n_in);
        }
        *a.out = o;
    }
}

void launch_align_fit(const AlignFitArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_align_fit, dim3(1), dim3(ALIGN_FIT_THREADS), 0, s, a);
}
