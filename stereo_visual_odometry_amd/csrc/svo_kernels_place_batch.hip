// svo_kernels_place_batch.hip — the batched place candidates' kernels (include/svo.h, "Batched place candidates"; the rules are in
// svo_place_batch.hpp).  All run on the index's stream, as separate launches the stream orders: no kernel waits for another
// workgroup.  Rule 1 in front of them is the unguided search and k_reloc_select_batch (svo_kernels_reloc_batch.hip), unchanged.
//
// k_place_batch_list: a block per camera.  cam[p] = the camera of list position p, PB_CAM_NONE beyond the camera's entries; for
//   places_batch the list itself, gathered as ids[cand_row[p]] from the batched selection's lists where they lie: no host round trip.
// k_place_batch_insert: a block per camera, behind the former (an insert reads other cameras' positions).  Every live position goes
//   into the ONE global table: a plain look at each probed slot, a 32-bit atomicCAS on one that looks empty; an insert that meets its
//   own (id, camera) pair — a position of its own camera's range with its id — counts nothing.
//   The block's fresh inserts are summed through shuffles and four LDS words and stored: n_landmarks needs no atomic.
// k_place_batch_sweep: one lane per row, blocks of 256 threads over runs of consecutive tiles, as k_place_sweep, but with nothing in
//   LDS: the table is global and shared by all cameras.  The camera-independent bin {rows, first_inv, end} takes k_place_sweep's
//   wave-combined runs — the ballot of the first remaining lane's tag, popcounts, a run carried across the wave's tiles, one set of
//   atomics when another tag follows.  A qualifying row walks the table from hash(id) to the first empty slot and adds 1 to
//   votes[camera][bin] for every slot that holds its id: a row is read once however many cameras there are, and a row nobody
//   holds costs one slot of the table (most such walks end at once: the load is 1/2 at most).  The votes are not combined within
//   a wave: the lanes of a run share the bin but not the camera.
// k_place_batch_pick: a block of 1024 threads per camera, rule 3 over the camera's row of votes (pb_in_p: no key list).  The first
//   round also counts the voted tags.  The block's maximum goes through a wave shuffle and 16 LDS words, as k_place_pick's.
// All atomics are 32-bit integer adds, maxima and one compare-and-swap whose winner does not show: the same bits on every run.
#include "svo_place_batch_internal.hpp"

#define PB_BLOCK 256
#define PB_WAVES (PB_BLOCK / 64)
#define PB_SWEEP_BLOCKS 2048                          // eight blocks of four waves on each of 256 CUs: a walk is latency, not bandwidth
#define PB_PICK_THREADS 1024
#define PB_PICK_WAVES (PB_PICK_THREADS / 64)

struct PbGlobalSlot {
    __device__ int32_t peek(const int32_t* p) const { return *p; }
    __device__ int32_t cas(int32_t* p, int32_t expect, int32_t v) const { return atomicCAS(p, expect, v); }
};

__global__ void __launch_bounds__(PB_BLOCK) k_place_batch_list(PbTableArgs a) {
    const int b = blockIdx.x, lo = a.begin[b], slice = a.begin[b + 1] - lo;
    int n = slice;
    if (a.n_dev) n = a.n_dev[b] < n ? a.n_dev[b] : n;                     // the slice holds no more
    for (int c = threadIdx.x; c < slice; c += PB_BLOCK) {
        const int p = lo + c;                         // < the call's total
        const bool live = c < n;
        if (live && a.m_rows) a.list[p] = a.ids[a.m_rows[p]];             // a candidate's row is a row of the index
        a.cam[p] = live ? b : PB_CAM_NONE;
    }
}

__global__ void __launch_bounds__(PB_BLOCK) k_place_batch_insert(PbTableArgs a) {
    __shared__ int s_fresh[PB_WAVES];
    const int b = blockIdx.x, lo = a.begin[b], slice = a.begin[b + 1] - lo;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n = slice;
    if (a.n_dev) n = a.n_dev[b] < n ? a.n_dev[b] : n; // k_place_batch_list's live positions
    int fresh = 0;
    bool full = false;
    for (int c = tid; c < n; c += PB_BLOCK) {
        const PlaceInsert r = pb_insert(a.table, a.mask, a.list, lo, lo + n, lo + c, PbGlobalSlot{});
        fresh += r == PLACE_SET_NEW;
        full = full || r == PLACE_SET_FULL;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) fresh += __shfl_xor(fresh, off);
    if (lane == 0) s_fresh[wave] = fresh;
    __syncthreads();
    if (tid == 0) {
        int all = 0;
#pragma unroll
        for (int w = 0; w < PB_WAVES; w++) all += s_fresh[w];
        a.cams[b].n_landmarks = all;
    }
    if (full) a.cams[b].set_full = 1;
}

// some rows of one tag into the shared bin: a sum and two maxima, in any order
static __device__ __forceinline__ void pb_add(PlaceBin* b, int32_t rows, int32_t first_inv, int32_t end) {
    atomicAdd(&b->rows, rows);
    atomicMax(&b->first_inv, first_inv);
    atomicMax(&b->end, end);
}

__global__ void __launch_bounds__(PB_BLOCK) k_place_batch_sweep(PbSweepArgs a) {
    const int tid = threadIdx.x, lane = tid & 63;
    // a block's tiles are consecutive, and tile is block-uniform, so every lane of a wave reaches every ballot
    const int n_tiles = a.row_hi > a.row_lo ? (a.row_hi - a.row_lo + PB_BLOCK - 1) / PB_BLOCK : 0;                // <= 65 536
    const int per_block = (n_tiles + (int)gridDim.x - 1) / (int)gridDim.x;
    const int tile_end = ((int)blockIdx.x + 1) * per_block < n_tiles ? ((int)blockIdx.x + 1) * per_block : n_tiles;
    // the wave's run in progress, wave-uniform: the bin and what its rows have added so far; it goes out when another bin follows
    int32_t run_bin = -1, run_rows = 0, run_first = 0, run_end = 0;
    for (int tile = (int)blockIdx.x * per_block; tile < tile_end; tile++) {
        const int r = a.row_lo + tile * PB_BLOCK + tid;                   // < 2^24 + 256: no overflow
        bool q = false;
        int32_t bin = -1;
        if (r < a.row_hi) {
            const int32_t tag = a.points[r].tag;
            q = place_tag_qualifies(tag, a.tag_lo, a.tag_hi);
            if (q) {
                bin = tag - a.tag_lo;                 // 0 .. n_bins - 1 (the caller checked the span)
                int32_t* const votes = a.votes + bin;
                const int32_t* const cam = a.cam;
                const size_t n_bins = (size_t)a.n_bins;
                // an inserted position has a camera 0 .. n_cameras - 1: the index is below n_cameras x n_bins <= 2^24
                pb_visit(a.table, a.mask, a.list, a.ids[r], [=](int32_t at) { atomicAdd(votes + (size_t)cam[at] * n_bins, 1); });
            }
        }
        // a lane whose two neighbours carry other tags has nobody to combine with nearby: it adds its own row, beside the others like it
        const int32_t before = __shfl_up(bin, 1), after = __shfl_down(bin, 1);
        const bool solo = (lane == 0 || before != bin) && (lane == 63 || after != bin);
        if (q && solo) pb_add(a.bins + bin, 1, place_first_inv(r), r + 1);
        const int wave_row = r - lane;                // lane 0's row
        unsigned long long rest = __ballot(q && !solo);
        while (rest) {                                // wave-uniform
            const int lead = __ffsll((long long)rest) - 1;
            const int32_t t = __shfl(bin, lead);
            const unsigned long long same = __ballot(q && !solo && bin == t);
            if (t != run_bin) {
                if (run_bin >= 0 && lane == 0) pb_add(a.bins + run_bin, run_rows, run_first, run_end);
                run_bin = t; run_rows = 0; run_first = 0; run_end = 0;
            }
            const int32_t first = place_first_inv(wave_row + lead), end = wave_row + (63 - __clzll((long long)same)) + 1;
            run_rows += __popcll(same);
            run_first = first > run_first ? first : run_first; run_end = end > run_end ? end : run_end;
            rest &= ~same;
        }
    }
    if (run_bin >= 0 && lane == 0) pb_add(a.bins + run_bin, run_rows, run_first, run_end);
}

__global__ void __launch_bounds__(PB_PICK_THREADS) k_place_batch_pick(const int32_t* __restrict__ votes, const PlaceBin* __restrict__ bins, int n_bins,
                                                                      int32_t tag_lo, int32_t min_votes, int32_t separation, int32_t max_places,
                                                                      PlaceOut* __restrict__ places, PbCam* __restrict__ cams) {
    __shared__ uint64_t s_best[PB_PICK_WAVES];
    __shared__ int s_voted[PB_PICK_WAVES];
    __shared__ int32_t s_chosen[PLACE_MAX_PLACES];
    const int cam = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* v = votes + (size_t)cam * (size_t)n_bins;
    int n_places = 0, voted = 0;
    unsigned long long last_key = 0;
    while (n_places < max_places) {                   // block-uniform
        unsigned long long best = 0;
        for (int b = tid; b < n_bins; b += PB_PICK_THREADS) {
            const int32_t vb = v[b];
            if (n_places == 0) voted += vb >= 1;
            if (vb < min_votes || vb < 1) continue;
            const unsigned long long key = place_key(vb, b);
            if (key > best && pb_in_p(key, last_key, s_chosen, n_places, separation)) best = key;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off);
            best = o > best ? o : best;
            if (n_places == 0) voted += __shfl_xor(voted, off);
        }
        if (lane == 0) { s_best[wave] = best; s_voted[wave] = voted; }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < PB_PICK_WAVES; w++) best = s_best[w] > best ? s_best[w] : best;
        if (n_places == 0 && tid == 0) {
            int all = 0;
#pragma unroll
            for (int w = 0; w < PB_PICK_WAVES; w++) all += s_voted[w];
            cams[cam].n_tags_voted = all;
        }
        if (best == 0) break;
        last_key = best;
        const int32_t bin = place_key_bin(best);
        if (tid == 0) {
            s_chosen[n_places] = bin;                 // n_places < max_places <= 64
            places[(size_t)cam * (size_t)max_places + n_places] = place_out(bin, tag_lo, pb_bin(place_key_votes(best), bins[bin]));
        }
        n_places++;
        __syncthreads();                              // s_chosen is written, s_best is free for the next round
    }
    if (tid == 0) cams[cam].n_places = n_places;
}

void launch_place_batch_table(const PbTableArgs& a, int n_cameras, hipStream_t s) {
    if (n_cameras <= 0) return;
    hipLaunchKernelGGL(k_place_batch_list, dim3(n_cameras), dim3(PB_BLOCK), 0, s, a);
    hipLaunchKernelGGL(k_place_batch_insert, dim3(n_cameras), dim3(PB_BLOCK), 0, s, a);
}

void launch_place_batch_sweep(const PbSweepArgs& a, hipStream_t s) {
    const int rows = a.row_hi > a.row_lo ? a.row_hi - a.row_lo : 0;
    if (rows == 0) return;                            // the bins and the votes stay zero
    int blocks = (rows + PB_BLOCK - 1) / PB_BLOCK;
    blocks = blocks > PB_SWEEP_BLOCKS ? PB_SWEEP_BLOCKS : blocks;
    hipLaunchKernelGGL(k_place_batch_sweep, dim3(blocks), dim3(PB_BLOCK), 0, s, a);
}

void launch_place_batch_pick(const int32_t* votes, const PlaceBin* bins, int n_bins, int32_t tag_lo, int32_t min_votes, int32_t separation,
                             int32_t max_places, PlaceOut* places, PbCam* cams, int n_cameras, hipStream_t s) {
    if (n_cameras <= 0) return;
    hipLaunchKernelGGL(k_place_batch_pick, dim3(n_cameras), dim3(PB_PICK_THREADS), 0, s, votes, bins, n_bins, tag_lo, min_votes, separation, max_places,
                       places, cams);
}
