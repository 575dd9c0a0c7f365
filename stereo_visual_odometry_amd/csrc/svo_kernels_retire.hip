// svo_kernels_retire.hip — the maintenance of the descriptor index (include/svo.h, "Index maintenance"; the rules are in
// svo_retire.hpp).  One lane per row everywhere, blocks of RETIRE_BLOCK lanes, separate launches ordered by the stream: no kernel
// waits for another workgroup.
//
// k_retire_flags: keep[i] = alive1 of row row_lo + i.  Reads the row's tag (BY_TAG) and id (BY_IDS: a binary search in the sorted
//   list).  No atomics.
// k_retire_insert / k_retire_latest (LATEST_PER_ID): an open-addressing table of row numbers.  An alive row probes from the hash of
//   its id: an empty slot takes it by a 32-bit atomicCAS, a slot whose row has the same id takes atomicMax, any other slot sends it
//   on, wrapping.  A slot only changes between rows of one id, so ids[slot's row] is a stable key, every 64-bit id is legal, and
//   the slot ends at the id's largest alive row whatever order the atomics arrive in.  The second launch keeps a row iff its id's
//   slot holds it.  Both probes end after `slots` steps and raise RetireCtl::table_full there.
// k_retire_count, k_retire_scan (twice), k_retire_rank: the exclusive ranks of the keep flags.  Ranks inside a wave come from
//   __ballot and __popcll, the four waves of a block meet in 16 bytes of LDS, the block counts are scanned 256 to a block with
//   wave shuffles, and the 256 sums of that by one more block: 2^24 rows are 65 536 blocks are 256 sums.
// k_retire_gather, k_retire_put: one slab of the in-place compaction.  A block's destination range overlaps the source rows of
//   earlier blocks, so dst <= src does not make a parallel in-place move safe: the kept rows of a slab go to a bounce buffer first
//   (at rank[i] - rank[slab's first row]) and come down in a second launch, slab after slab in row order.  A row is read before
//   anything could have overwritten it: a slab's put writes below the slab's end, and every later slab reads at or above it.
//   Descriptors and points move as 16-byte accesses.
// k_transform_points: a 16-byte load, the f64 arithmetic of retire_map_coord, a 16-byte store when every coordinate is finite; the
//   two counts by one integer atomicAdd per wave, spread over RETIRE_COUNT_SLOTS cache lines.  No LDS.
#include "svo_retire_internal.hpp"

// the exclusive rank of this lane's flag among the block's lanes, and the block's count; every lane of the block calls it
static __device__ __forceinline__ int block_rank(bool flag, int* sh, int& total) {
    const unsigned long long b = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int in_wave = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) sh[wave] = __popcll(b);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < RETIRE_BLOCK / 64; w++) { const int c = sh[w]; before += w < wave ? c : 0; total += c; }
    return before + in_wave;
}

__global__ void __launch_bounds__(RETIRE_BLOCK) k_retire_flags(const uint4* __restrict__ points, const uint64_t* __restrict__ ids, int row_lo, int n,
                                                              uint32_t flags, int32_t tag_lo, int32_t tag_hi, const uint64_t* __restrict__ sorted,
                                                              int32_t n_sorted, uint8_t* __restrict__ keep) {
    const int i = (int)(blockIdx.x * RETIRE_BLOCK + threadIdx.x);     // n <= 2^24: no overflow
    if (i >= n) return;
    const int row = row_lo + i;
    const int32_t tag = (flags & RETIRE_BY_TAG) ? (int32_t)points[row].w : 0;
    const bool listed = (flags & RETIRE_BY_IDS) ? retire_id_listed(sorted, n_sorted, ids[row]) : false;
    keep[i] = retire_alive1(flags, tag, tag_lo, tag_hi, listed) ? 1 : 0;
}

__global__ void __launch_bounds__(RETIRE_BLOCK) k_retire_insert(const uint64_t* __restrict__ ids, int row_lo, int n, const uint8_t* __restrict__ keep,
                                                               int32_t* table, uint32_t mask, RetireCtl* ctl) {
    const int i = (int)(blockIdx.x * RETIRE_BLOCK + threadIdx.x);
    if (i >= n || !keep[i]) return;
    const int row = row_lo + i;
    const uint64_t id = ids[row];
    uint32_t slot = retire_slot_first(id, mask);
    for (uint32_t step = 0; step <= mask; step++, slot = retire_slot_next(slot, mask)) {
        const int32_t old = atomicCAS(&table[slot], RETIRE_EMPTY, row);
        if (old == RETIRE_EMPTY) return;              // the slot was empty and is this row's now
        if (ids[old] == id) { atomicMax(&table[slot], row); return; }   // old: a row of the scope, written by a lane of this launch
    }
    ctl->table_full = 1;
}

__global__ void __launch_bounds__(RETIRE_BLOCK) k_retire_latest(const uint64_t* __restrict__ ids, int row_lo, int n, uint8_t* __restrict__ keep,
                                                               const int32_t* __restrict__ table, uint32_t mask, RetireCtl* ctl) {
    const int i = (int)(blockIdx.x * RETIRE_BLOCK + threadIdx.x);
    if (i >= n || !keep[i]) return;
    const int row = row_lo + i;
    const uint64_t id = ids[row];
    uint32_t slot = retire_slot_first(id, mask);
    for (uint32_t step = 0; step <= mask; step++, slot = retire_slot_next(slot, mask)) {
        const int32_t at = table[slot];
        if (at == RETIRE_EMPTY) break;                // an inserted id's probe never meets an empty slot
        if (ids[at] == id) { keep[i] = at == row ? 1 : 0; return; }
    }
    ctl->table_full = 1;
}

__global__ void __launch_bounds__(RETIRE_BLOCK) k_retire_count(const uint8_t* __restrict__ keep, int n, int32_t* __restrict__ counts) {
    __shared__ int sh[RETIRE_BLOCK / 64];
    const int i = (int)(blockIdx.x * RETIRE_BLOCK + threadIdx.x);
    int total;
    (void)block_rank(i < n && keep[i], sh, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// v[0 .. n) becomes its exclusive scan inside each block's 256 entries; sums[block] = the block's total
__global__ void __launch_bounds__(RETIRE_BLOCK) k_retire_scan(int32_t* __restrict__ v, int n, int32_t* __restrict__ sums) {
    __shared__ int sh[RETIRE_BLOCK / 64];
    const int i = (int)(blockIdx.x * RETIRE_BLOCK + threadIdx.x);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int mine = i < n ? v[i] : 0;
    int inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d *= 2) { const int up = __shfl_up(inc, d, 64); inc += lane >= d ? up : 0; }
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < RETIRE_BLOCK / 64; w++) { const int c = sh[w]; before += w < wave ? c : 0; total += c; }
    if (i < n) v[i] = before + inc - mine;
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// counts: the block counts scanned inside groups of 256, then the groups' sums scanned
__global__ void __launch_bounds__(RETIRE_BLOCK) k_retire_rank(const uint8_t* __restrict__ keep, int n, const int32_t* __restrict__ counts,
                                                             const int32_t* __restrict__ sums, int32_t* __restrict__ rank) {
    __shared__ int sh[RETIRE_BLOCK / 64];
    const int i = (int)(blockIdx.x * RETIRE_BLOCK + threadIdx.x);
    const bool flag = i < n && keep[i];
    int total;
    const int r = sums[blockIdx.x / RETIRE_BLOCK] + counts[blockIdx.x] + block_rank(flag, sh, total);
    if (i < n) rank[i] = r;
    if (i == n - 1) rank[n] = r + (flag ? 1 : 0);
}

// the bounce buffer of one slab: slab_rows descriptors, then as many points, then as many ids
struct RetireBounce { uint4* desc; uint4* points; uint64_t* ids; };

__global__ void __launch_bounds__(RETIRE_BLOCK) k_retire_gather(RetireRows x, int row, int n, const uint8_t* __restrict__ keep,
                                                               const int32_t* __restrict__ rank, RetireBounce b) {
    const int i = (int)(blockIdx.x * RETIRE_BLOCK + threadIdx.x);
    if (i >= n || (keep && !keep[i])) return;
    const size_t src = (size_t)(row + i), j = (size_t)(rank ? rank[i] - rank[0] : i);   // j <= i: a rank grows by at most one a row
    b.desc[2 * j] = x.desc[2 * src];
    b.desc[2 * j + 1] = x.desc[2 * src + 1];
    b.ids[j] = x.ids[src];
    if (x.points) b.points[j] = x.points[src];
}

__global__ void __launch_bounds__(RETIRE_BLOCK) k_retire_put(RetireRows x, int n, const int32_t* __restrict__ rank, int dst, RetireBounce b) {
    const int count = rank ? rank[n] - rank[0] : n;   // the slab's kept rows
    const int i = (int)(blockIdx.x * RETIRE_BLOCK + threadIdx.x);
    if (i >= count) return;
    const size_t to = (size_t)(dst + (rank ? rank[0] : 0) + i), j = (size_t)i;          // to <= the slab's row i
    x.desc[2 * to] = b.desc[2 * j];
    x.desc[2 * to + 1] = b.desc[2 * j + 1];
    x.ids[to] = b.ids[j];
    if (x.points) x.points[to] = b.points[j];
}

__global__ void __launch_bounds__(RETIRE_BLOCK) k_transform_points(uint4* __restrict__ points, RetireT T, int row_lo, int row_hi, int32_t tag_lo,
                                                                  int32_t tag_hi, RetireCtl* ctl) {
    const int row = row_lo + (int)(blockIdx.x * RETIRE_BLOCK + threadIdx.x);
    bool moved = false, skipped = false;
    if (row < row_hi) {
        const uint4 p = points[row];
        if (retire_tag_selected((int32_t)p.w, tag_lo, tag_hi)) {
            const float x = __uint_as_float(p.x), y = __uint_as_float(p.y), z = __uint_as_float(p.z);
            uint4 q = p;                              // the tag's bits stay
            q.x = __float_as_uint(retire_map_coord(T.m, 0, x, y, z));
            q.y = __float_as_uint(retire_map_coord(T.m, 1, x, y, z));
            q.z = __float_as_uint(retire_map_coord(T.m, 2, x, y, z));
            moved = retire_finite_bits(q.x) && retire_finite_bits(q.y) && retire_finite_bits(q.z);
            skipped = !moved;
            if (moved) points[row] = q;
        }
    }
    const int n_moved = __popcll(__ballot(moved)), n_skipped = __popcll(__ballot(skipped));
    if ((threadIdx.x & 63) == 0) {
        RetireCounts* c = &ctl->counts[blockIdx.x % RETIRE_COUNT_SLOTS];
        if (n_moved) atomicAdd(&c->n_moved, n_moved);
        if (n_skipped) atomicAdd(&c->n_skipped, n_skipped);
    }
}

static inline int retire_blocks(int n) { return (n + RETIRE_BLOCK - 1) / RETIRE_BLOCK; }

void launch_retire_flags(const RetireRows& x, int row_lo, int n, uint32_t flags, int32_t tag_lo, int32_t tag_hi, const uint64_t* sorted,
                         int32_t n_sorted, uint8_t* keep, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_retire_flags, dim3(retire_blocks(n)), dim3(RETIRE_BLOCK), 0, s, x.points, x.ids, row_lo, n, flags, tag_lo, tag_hi, sorted,
                       n_sorted, keep);
}

void launch_retire_latest(const RetireRows& x, int row_lo, int n, uint8_t* keep, int32_t* table, uint32_t slots, RetireCtl* ctl, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_retire_insert, dim3(retire_blocks(n)), dim3(RETIRE_BLOCK), 0, s, x.ids, row_lo, n, keep, table, slots - 1, ctl);
    hipLaunchKernelGGL(k_retire_latest, dim3(retire_blocks(n)), dim3(RETIRE_BLOCK), 0, s, x.ids, row_lo, n, keep, table, slots - 1, ctl);
}

void launch_retire_ranks(const uint8_t* keep, int n, int32_t* counts, int32_t* rank, hipStream_t s) {
    if (n <= 0) return;
    const int blocks = retire_blocks(n), groups = retire_blocks(blocks);      // n <= 2^24: groups <= RETIRE_BLOCK
    int32_t* sums = counts + blocks;                  // RETIRE_BLOCK entries, then the total
    hipLaunchKernelGGL(k_retire_count, dim3(blocks), dim3(RETIRE_BLOCK), 0, s, keep, n, counts);
    hipLaunchKernelGGL(k_retire_scan, dim3(groups), dim3(RETIRE_BLOCK), 0, s, counts, blocks, sums);
    hipLaunchKernelGGL(k_retire_scan, dim3(1), dim3(RETIRE_BLOCK), 0, s, sums, groups, sums + RETIRE_BLOCK);
    hipLaunchKernelGGL(k_retire_rank, dim3(blocks), dim3(RETIRE_BLOCK), 0, s, keep, n, counts, sums, rank);
}

void launch_retire_slab(const RetireRows& x, int row, int n, const uint8_t* keep, const int32_t* rank, int dst, void* bounce, int slab_rows,
                        hipStream_t s) {
    if (n <= 0) return;
    RetireBounce b;
    b.desc = (uint4*)bounce; b.points = b.desc + 2 * (size_t)slab_rows; b.ids = (uint64_t*)(b.points + (size_t)slab_rows);
    hipLaunchKernelGGL(k_retire_gather, dim3(retire_blocks(n)), dim3(RETIRE_BLOCK), 0, s, x, row, n, keep, rank, b);
    hipLaunchKernelGGL(k_retire_put, dim3(retire_blocks(n)), dim3(RETIRE_BLOCK), 0, s, x, n, rank, dst, b);
}

void launch_transform_points(uint4* points, const RetireT& T, int row_lo, int row_hi, int32_t tag_lo, int32_t tag_hi, RetireCtl* ctl, hipStream_t s) {
    if (row_hi <= row_lo) return;
    hipLaunchKernelGGL(k_transform_points, dim3(retire_blocks(row_hi - row_lo)), dim3(RETIRE_BLOCK), 0, s, points, T, row_lo, row_hi, tag_lo, tag_hi, ctl);
}
