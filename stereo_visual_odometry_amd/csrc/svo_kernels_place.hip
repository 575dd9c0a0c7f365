// svo_kernels_place.hip — the place candidates' kernels (include/svo.h, "Place candidates"; the rules are in svo_place.hpp).  All run
// on the index's stream, as separate launches the stream orders: no kernel waits for another workgroup.  Rule 1 in front of them is
// the search and k_reloc_select (svo_kernels_reloc.hip), unchanged.
//
// k_place_sweep: blocks of 256 threads, at most PLACE_SWEEP_BLOCKS of them, each over its own run of consecutive tiles of 256 rows.
//   A block first builds M in its own LDS: the id list (at most 4096 ids, 32 KiB; for svo_desc_index_places the ids of the
//   candidates' rows, read through k_reloc_select's cand_row) and a set of list positions over it (fuse_table_slots: at most 8192
//   slots, 32 KiB), inserted with an LDS atomicCAS, so a duplicate id is harmless and no id value is a sentinel.  64 KiB a block at
//   most: two blocks a CU.  Block 0 also counts the distinct ids.  Then per row: the tag dword of its 16-byte point row and, where the
//   tag qualifies, its 8-byte id and a probe of the set.  The rows of one keyframe are contiguous, so most of a wave's 64 rows share
//   a tag: the lanes of the first remaining lane's tag are balloted, their count and their hits are popcounts, the smallest and the
//   largest row are the first and the last set bit of the ballot (a wave's rows increase with the lane), and the sums go into
//   wave-uniform registers — the run in progress — which ONE lane adds to the bin (one atomicAdd per count, one atomicMax per bound)
//   when another tag follows or the wave's tiles end: a keyframe longer than a tile costs a wave one set of atomics, not one a tile.
//   A lane whose neighbours on both sides carry other tags stays out of that loop and adds its own row, so rows that each have their
//   own tag cost what the plain form costs.  The plain form (every qualifying row its own four atomics) is the same kernel built
//   with COMBINE = false; profiles/ has both timed.
// k_place_compact: one lane per bin.  The bins with votes >= 1 are counted and those with votes >= min_votes get a slot of the key
//   list, one atomicAdd per wave each.  The list's order is arbitrary; rule 3 does not depend on it.
// k_place_pick: ONE block of 1024 threads.  Up to max_places rounds: a thread walks its entries of the list, drops those the last
//   emitted place suppresses (the key becomes 0: the flag), and keeps its largest key; the block's maximum goes through a wave
//   shuffle and 16 LDS words; thread 0 emits the place.
// All atomics are integer adds and maxima: the same bits on every run.
#include "svo_place_internal.hpp"

#define PLACE_BLOCK 256
#define PLACE_SWEEP_BLOCKS 512                        // two blocks of 64 KiB LDS on each of 256 CUs
#define PLACE_PICK_THREADS 1024
#define PLACE_PICK_WAVES (PLACE_PICK_THREADS / 64)

struct PlaceLdsSlot {
    __device__ int32_t cas(int32_t* p, int32_t expect, int32_t v) const { return atomicCAS(p, expect, v); }
};

// rows, votes and the two bounds of some rows of one tag into its bin: sums and maxima, in any order
static __device__ __forceinline__ void place_add(PlaceBin* b, int32_t rows, int32_t votes, int32_t first_inv, int32_t end) {
    atomicAdd(&b->rows, rows);
    if (votes) atomicAdd(&b->votes, votes);
    atomicMax(&b->first_inv, first_inv);
    atomicMax(&b->end, end);
}

template <bool COMBINE>
__global__ void __launch_bounds__(PLACE_BLOCK) k_place_sweep(PlaceSweepArgs a, uint32_t mask) {
    extern __shared__ uint64_t s_mem[];
    const int tid = threadIdx.x, lane = tid & 63;
    int m = a.n;
    if (a.n_dev) m = *a.n_dev < m ? *a.n_dev : m;     // the list holds no more than n
    uint64_t* s_ids = s_mem;                          // [max(n, 1)]
    int32_t* s_table = reinterpret_cast<int32_t*>(s_mem + (a.n > 0 ? a.n : 1));      // [mask + 1]
    // ---- M: the list, then the set over it
    for (uint32_t i = tid; i <= mask; i += PLACE_BLOCK) s_table[i] = PLACE_EMPTY;
    for (int c = tid; c < m; c += PLACE_BLOCK) s_ids[c] = a.m_rows ? a.ids[a.m_rows[c]] : a.list[c];
    __syncthreads();
    int fresh = 0;
    bool full = false;
    for (int c = tid; c < m; c += PLACE_BLOCK) {
        const PlaceInsert r = place_set_insert(s_table, mask, s_ids, c, PlaceLdsSlot{});
        fresh += r == PLACE_SET_NEW;
        full = full || r == PLACE_SET_FULL;
    }
    if (blockIdx.x == 0) {
        if (fresh) atomicAdd(&a.ctl->n_landmarks, fresh);
        if (full) a.ctl->set_full = 1;
    }
    __syncthreads();
    // ---- rule 2: a block's tiles are consecutive, and tile is block-uniform, so every lane of a wave reaches every ballot
    const int n_tiles = a.row_hi > a.row_lo ? (a.row_hi - a.row_lo + PLACE_BLOCK - 1) / PLACE_BLOCK : 0;           // <= 65 536
    const int per_block = (n_tiles + (int)gridDim.x - 1) / (int)gridDim.x;
    const int tile_end = ((int)blockIdx.x + 1) * per_block < n_tiles ? ((int)blockIdx.x + 1) * per_block : n_tiles;
    // the wave's run in progress, wave-uniform: the bin and what its rows have added so far; it goes out when another bin follows
    int32_t run_bin = -1, run_rows = 0, run_votes = 0, run_first = 0, run_end = 0;
    for (int tile = (int)blockIdx.x * per_block; tile < tile_end; tile++) {
        const int r = a.row_lo + tile * PLACE_BLOCK + tid;            // < 2^24 + 256: no overflow
        bool q = false, hit = false;
        int32_t bin = -1;
        if (r < a.row_hi) {
            const int32_t tag = a.points[r].tag;
            q = place_tag_qualifies(tag, a.tag_lo, a.tag_hi);
            if (q) {
                bin = tag - a.tag_lo;                 // 0 .. 2^20 - 1 (the caller checked the span)
                hit = place_set_has(s_table, mask, s_ids, a.ids[r]);
            }
        }
        // a lane whose two neighbours carry other tags has nobody to combine with nearby: it adds its own row, beside the others like it
        const int32_t before = __shfl_up(bin, 1), after = __shfl_down(bin, 1);
        const bool solo = !COMBINE || ((lane == 0 || before != bin) && (lane == 63 || after != bin));
        if (q && solo) place_add(a.bins + bin, 1, hit ? 1 : 0, place_first_inv(r), r + 1);
        if (COMBINE) {
            const int wave_row = r - lane;            // lane 0's row
            unsigned long long rest = __ballot(q && !solo);
            const unsigned long long hits = __ballot(hit);
            while (rest) {                            // wave-uniform
                const int lead = __ffsll((long long)rest) - 1;
                const int32_t t = __shfl(bin, lead);
                const unsigned long long same = __ballot(q && !solo && bin == t);
                if (t != run_bin) {
                    if (run_bin >= 0 && lane == 0) place_add(a.bins + run_bin, run_rows, run_votes, run_first, run_end);
                    run_bin = t; run_rows = 0; run_votes = 0; run_first = 0; run_end = 0;
                }
                const int32_t first = place_first_inv(wave_row + lead), end = wave_row + (63 - __clzll((long long)same)) + 1;
                run_rows += __popcll(same); run_votes += __popcll(same & hits);
                run_first = first > run_first ? first : run_first; run_end = end > run_end ? end : run_end;
                rest &= ~same;
            }
        }
    }
    if (run_bin >= 0 && lane == 0) place_add(a.bins + run_bin, run_rows, run_votes, run_first, run_end);
}

__global__ void __launch_bounds__(PLACE_BLOCK) k_place_compact(const PlaceBin* __restrict__ bins, int n_bins, int32_t min_votes,
                                                              uint64_t* __restrict__ keys, PlaceCtl* ctl) {
    const int i = (int)(blockIdx.x * PLACE_BLOCK + threadIdx.x);      // n_bins <= 2^20: no overflow
    const int lane = threadIdx.x & 63;
    const int32_t votes = i < n_bins ? bins[i].votes : 0;
    const unsigned long long voted = __ballot(votes >= 1), keep = __ballot(votes >= min_votes && votes >= 1);
    int at = 0;
    if (lane == 0) {
        if (voted) atomicAdd(&ctl->n_tags_voted, __popcll(voted));
        if (keep) at = atomicAdd(&ctl->n_list, __popcll(keep));
    }
    at = __shfl(at, 0);
    if (keep >> lane & 1ull) keys[at + __popcll(keep & ((1ull << lane) - 1ull))] = place_key(votes, i);   // at + rank < n_bins: one slot a bin
}

__global__ void __launch_bounds__(PLACE_PICK_THREADS) k_place_pick(uint64_t* __restrict__ keys, const PlaceBin* __restrict__ bins, int32_t tag_lo,
                                                                  int32_t separation, int32_t max_places, PlaceCtl* ctl) {
    __shared__ uint64_t s_best[PLACE_PICK_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = ctl->n_list;
    int n_places = 0;
    int32_t last = -1;
    while (n_places < max_places) {                   // block-uniform
        unsigned long long best = 0;
        for (int e = tid; e < n; e += PLACE_PICK_THREADS) {           // a thread's entries are its own: no other thread reads or writes them
            const unsigned long long k = keys[e];
            if (k == 0) continue;
            if (last >= 0 && place_suppresses(place_key_bin(k), last, separation)) { keys[e] = 0; continue; }
            best = k > best ? k : best;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off);
            best = o > best ? o : best;
        }
        if (lane == 0) s_best[wave] = best;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < PLACE_PICK_WAVES; w++) best = s_best[w] > best ? s_best[w] : best;
        __syncthreads();                              // s_best is free for the next round
        if (best == 0) break;
        last = place_key_bin(best);
        if (tid == 0) ctl->places[n_places] = place_out(last, tag_lo, bins[last]);
        n_places++;
    }
    if (tid == 0) ctl->n_places = n_places;
}

void launch_place_sweep(const PlaceSweepArgs& a, bool combine, hipStream_t s) {
    const int rows = a.row_hi > a.row_lo ? a.row_hi - a.row_lo : 0;
    int blocks = (rows + PLACE_BLOCK - 1) / PLACE_BLOCK;
    blocks = blocks < 1 ? 1 : blocks > PLACE_SWEEP_BLOCKS ? PLACE_SWEEP_BLOCKS : blocks;      // one at least: block 0 counts M
    const uint32_t mask = fuse_table_slots(a.n) - 1;
    const size_t lds = place_lds_bytes(a.n);          // <= 64 KiB
    if (combine) hipLaunchKernelGGL(k_place_sweep<true>, dim3(blocks), dim3(PLACE_BLOCK), lds, s, a, mask);
    else hipLaunchKernelGGL(k_place_sweep<false>, dim3(blocks), dim3(PLACE_BLOCK), lds, s, a, mask);
}

void launch_place_pick(PlaceBin* bins, int n_bins, int32_t tag_lo, int32_t min_votes, int32_t separation, int32_t max_places, uint64_t* keys,
                       PlaceCtl* ctl, hipStream_t s) {
    hipLaunchKernelGGL(k_place_compact, dim3((n_bins + PLACE_BLOCK - 1) / PLACE_BLOCK), dim3(PLACE_BLOCK), 0, s, bins, n_bins, min_votes, keys, ctl);
    hipLaunchKernelGGL(k_place_pick, dim3(1), dim3(PLACE_PICK_THREADS), 0, s, keys, bins, tag_lo, separation, max_places, ctl);
}
