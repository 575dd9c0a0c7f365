// svo_kernels_consolidate.hip — the landmark consolidation of the descriptor index (include/svo.h, "Landmark consolidation"; the
// rules are in svo_consolidate.hpp).  Blocks of RETIRE_BLOCK lanes, separate launches ordered by the stream: no kernel waits for
// another workgroup.  32-bit integer atomics only, no LDS but the scan's 16 bytes.
//
// k_cons_insert: keep[i] = 1; a member probes retire's open-addressing table from the hash of its id — an empty slot takes the row
//   by atomicCAS, a slot whose row has the same id takes atomicMax, any other slot sends it on — and adds one to the slot's count.
//   The slot ends at the group's latest row and its size whatever order the atomics arrive in.
// k_cons_place: offset[i] = the group's size where row i is its group's latest row, else 0.
// k_cons_scan (three levels), k_cons_offsets: the exclusive scan of that, 256 entries to a block with wave shuffles: offset[i] is
//   where the group whose latest row is i starts in the member list, offset[i + 1] - offset[i] its size.
// k_cons_scatter: a member takes a place of its group's segment by counting the slot's count down (atomicSub) and writes its row
//   number there; one that is not the latest clears its keep flag.  The order inside a segment is whatever the atomics gave; the
//   group kernel sorts.
// k_cons_group: a wave serves 64 rows of the scope and, one after another, the groups of two or more whose latest row is among
//   them.  View i of the group sits in lane i: a segment of more than 64 first yields its 64 largest rows (a bisection on the row
//   number, counting by ballot), the rows are ranked and handed to the lane of their rank by lane broadcasts, each lane loads its
//   row's descriptor and point, accumulates its sum of distances against every broadcast view, the wave reduces (sum, lane) to the
//   medoid, and every lane adds the near views' points in lane order in f64.  Then the medoid's lane writes its descriptor and the
//   last lane the point into the latest row: all of the group's reads precede these writes, and no other wave reads these rows.
//   Nothing is written when the table overflowed.
// The compaction from the keep flags is retire's, unchanged.
#include "svo_consolidate_internal.hpp"

// where the slot of id is, or the table's size when the probe ran out
static __device__ __forceinline__ uint32_t cons_find(const uint64_t* __restrict__ ids, const int32_t* __restrict__ table, uint32_t mask, uint64_t id) {
    uint32_t slot = retire_slot_first(id, mask);
    for (uint32_t step = 0; step <= mask; step++, slot = retire_slot_next(slot, mask)) {
        const int32_t at = table[slot];
        if (at == RETIRE_EMPTY) break;                // an inserted id's probe never meets an empty slot
        if (ids[at] == id) return slot;
    }
    return mask + 1;
}

static __device__ __forceinline__ void cons_count(int32_t* counter, bool flag) {
    const int c = __popcll(__ballot(flag));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(counter, c);
}

__global__ void __launch_bounds__(RETIRE_BLOCK) k_cons_insert(const uint4* __restrict__ points, const uint64_t* __restrict__ ids, ConsWork w) {
    const int i = (int)(blockIdx.x * RETIRE_BLOCK + threadIdx.x);     // n <= 2^24: no overflow
    const int row = w.row_lo + i;
    const bool member = i < w.n && cons_member((int32_t)points[row].w, w.tag_lo, w.tag_hi);
    if (i < w.n) w.keep[i] = 1;
    if (member) {
        const uint32_t mask = w.slots - 1;
        const uint64_t id = ids[row];
        uint32_t slot = retire_slot_first(id, mask);
        bool placed = false;
        for (uint32_t step = 0; step <= mask && !placed; step++) {
            const int32_t old = atomicCAS(&w.table[slot], RETIRE_EMPTY, row);
            if (old == RETIRE_EMPTY) placed = true;   // the slot was empty and is this row's now
            else if (ids[old] == id) { atomicMax(&w.table[slot], row); placed = true; }   // old: a row of the scope, written by a lane of this launch
            else slot = retire_slot_next(slot, mask);
        }
        if (placed) atomicAdd(&w.count[slot], 1);
        else w.ctl->table_full = 1;
    }
    cons_count(&w.ctl->counts[blockIdx.x % CONS_COUNT_SLOTS].n_members, member);
}

__global__ void __launch_bounds__(RETIRE_BLOCK) k_cons_place(const uint4* __restrict__ points, const uint64_t* __restrict__ ids, ConsWork w) {
    const int i = (int)(blockIdx.x * RETIRE_BLOCK + threadIdx.x);
    if (i >= w.n) return;
    const int row = w.row_lo + i;
    int32_t size = 0;
    if (cons_member((int32_t)points[row].w, w.tag_lo, w.tag_hi)) {
        const uint32_t slot = cons_find(ids, w.table, w.slots - 1, ids[row]);
        if (slot == w.slots) w.ctl->table_full = 1;
        else if (w.table[slot] == row) size = w.count[slot];
    }
    w.offset[i] = size;
}

// v[0 .. n) becomes its exclusive scan inside each block's 256 entries; sums[block] = the block's total
__global__ void __launch_bounds__(RETIRE_BLOCK) k_cons_scan(int32_t* __restrict__ v, int n, int32_t* __restrict__ sums) {
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
    for (int k = 0; k < RETIRE_BLOCK / 64; k++) { const int c = sh[k]; before += k < wave ? c : 0; total += c; }
    if (i < n) v[i] = before + inc - mine;
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums: the block sums scanned inside groups of 256, then (sums + blocks) the groups' sums scanned, then their total
__global__ void __launch_bounds__(RETIRE_BLOCK) k_cons_offsets(int32_t* __restrict__ offset, int n, const int32_t* __restrict__ sums, int blocks) {
    const int i = (int)(blockIdx.x * RETIRE_BLOCK + threadIdx.x);
    if (i >= n) return;
    offset[i] += sums[blockIdx.x] + sums[blocks + blockIdx.x / RETIRE_BLOCK];
    if (i == n - 1) offset[n] = sums[blocks + RETIRE_BLOCK];
}

__global__ void __launch_bounds__(RETIRE_BLOCK) k_cons_scatter(const uint4* __restrict__ points, const uint64_t* __restrict__ ids, ConsWork w) {
    const int i = (int)(blockIdx.x * RETIRE_BLOCK + threadIdx.x);
    if (i >= w.n) return;
    const int row = w.row_lo + i;
    if (!cons_member((int32_t)points[row].w, w.tag_lo, w.tag_hi)) return;
    const uint32_t slot = cons_find(ids, w.table, w.slots - 1, ids[row]);
    if (slot == w.slots) { w.ctl->table_full = 1; return; }
    const int latest = w.table[slot];                 // a row of the scope
    const int at = atomicSub(&w.count[slot], 1) - 1;  // 0 .. the group's size - 1, each once
    const int first = w.offset[latest - w.row_lo];
    if (at >= 0 && first + at < w.n) w.list[first + at] = row;
    if (row != latest) w.keep[i] = 0;
}

static __device__ __forceinline__ uint32_t lane_get(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }

__global__ void __launch_bounds__(RETIRE_BLOCK) k_cons_group(RetireRows x, ConsWork w, float radius) {
    const int lane = threadIdx.x & 63;
    const int i = (int)(blockIdx.x * RETIRE_BLOCK + threadIdx.x);
    int first = 0, size = 0;
    if (i < w.n) { first = w.offset[i]; size = w.offset[i + 1] - first; }
    if (w.ctl->table_full) return;                    // a refused call writes nothing
    const int wave_row = w.row_lo + i - lane;         // the row of this wave's lane 0
    int n_far = 0, n_capped = 0;
    unsigned long long todo = __ballot(size >= 2);
    while (todo) {
        const int g = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
        todo &= todo - 1;
        const int gfirst = (int)lane_get((uint32_t)first, g), gsize = (int)lane_get((uint32_t)size, g);
        const int32_t* __restrict__ seg = w.list + gfirst;
        const int n = cons_views(gsize);
        // ---- the views' rows, in any order: row >= 0 in lanes 0 .. n - 1
        int row = -1;
        if (gsize <= CONS_MAX_VIEWS) {
            if (lane < gsize) row = seg[lane];
        } else {
            n_capped++;
            int lo = w.row_lo, hi = wave_row + g + 1; // #{rows >= lo} >= 64 > #{rows >= hi}: the latest row is wave_row + g
            while (hi - lo > 1) {
                const int mid = lo + (hi - lo) / 2;
                int c = 0;
                for (int j0 = 0; j0 < gsize; j0 += 64) c += __popcll(__ballot(j0 + lane < gsize && seg[j0 + lane] >= mid));
                if (c >= CONS_MAX_VIEWS) lo = mid; else hi = mid;
            }
            int taken = 0;                            // the rows are distinct: exactly 64 of them are >= lo
            for (int j0 = 0; j0 < gsize; j0 += 64) {
                const int v = j0 + lane < gsize ? seg[j0 + lane] : -1;
                unsigned long long in = __ballot(v >= lo);
                while (in) {
                    const int b = __builtin_amdgcn_readfirstlane(__ffsll((long long)in) - 1);
                    in &= in - 1;
                    const int r = (int)lane_get((uint32_t)v, b);
                    if (lane == taken) row = r;
                    taken++;
                }
            }
        }
        // ---- lane i takes the view of rank i: ascending rows
        int rank = 0;
        for (int j = 0; j < n; j++) rank += (int)lane_get((uint32_t)row, j) < row ? 1 : 0;
        int mine = -1;
        for (int j = 0; j < n; j++) {
            const int r = (int)lane_get((uint32_t)row, j), k = (int)lane_get((uint32_t)rank, j);
            if (k == lane) mine = r;
        }
        const bool view = lane < n;
        if (__ballot(view && (mine < w.row_lo || mine >= w.row_lo + w.n))) {      // a member list the scatter did not fill: ruled out, never followed
            if (lane == 0) w.ctl->table_full = 1;
            continue;
        }
        uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0, p = d0;
        if (view) { d0 = x.desc[2 * (size_t)mine]; d1 = x.desc[2 * (size_t)mine + 1]; p = x.points[mine]; }
        // ---- rule 3
        int sum = 0;
        for (int j = 0; j < n; j++) {
            sum += __popc(d0.x ^ lane_get(d0.x, j)) + __popc(d0.y ^ lane_get(d0.y, j)) + __popc(d0.z ^ lane_get(d0.z, j)) + __popc(d0.w ^ lane_get(d0.w, j));
            sum += __popc(d1.x ^ lane_get(d1.x, j)) + __popc(d1.y ^ lane_get(d1.y, j)) + __popc(d1.z ^ lane_get(d1.z, j)) + __popc(d1.w ^ lane_get(d1.w, j));
        }
        // the smaller sum, then the larger row, which is the larger lane: sum <= 63 x 256 < 2^14
        int key = view ? (sum << 6) | (63 - lane) : 0x7FFFFFFF;
#pragma unroll
        for (int d = 32; d >= 1; d /= 2) { const int o = __shfl_xor(key, d, 64); key = o < key ? o : key; }
        const int medoid = 63 - (__builtin_amdgcn_readfirstlane(key) & 63);
        // ---- rule 4
        const float qx = __uint_as_float(lane_get(p.x, medoid)), qy = __uint_as_float(lane_get(p.y, medoid)), qz = __uint_as_float(lane_get(p.z, medoid));
        const unsigned long long near = __ballot(view && cons_near(__uint_as_float(p.x), __uint_as_float(p.y), __uint_as_float(p.z), qx, qy, qz, radius));
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int n_near = 0;
        for (int j = 0; j < n; j++) {
            if (!((near >> j) & 1ull)) continue;
            sx = sx + (double)__uint_as_float(lane_get(p.x, j));
            sy = sy + (double)__uint_as_float(lane_get(p.y, j));
            sz = sz + (double)__uint_as_float(lane_get(p.z, j));
            n_near++;
        }
        n_far += n - n_near;
        // ---- rule 5: lane n - 1 holds the latest row
        const int latest = (int)lane_get((uint32_t)mine, n - 1);
        if (lane == medoid) { x.desc[2 * (size_t)latest] = d0; x.desc[2 * (size_t)latest + 1] = d1; }
        if (lane == n - 1) {
            p.x = __float_as_uint(cons_mean(sx, n_near)); p.y = __float_as_uint(cons_mean(sy, n_near)); p.z = __float_as_uint(cons_mean(sz, n_near));
            x.points[latest] = p;                     // its own tag stays
        }
    }
    ConsCounts* c = &w.ctl->counts[blockIdx.x % CONS_COUNT_SLOTS];
    cons_count(&c->n_groups, size >= 1);
    if (lane == 0) {
        if (n_far) atomicAdd(&c->n_far_views, n_far);
        if (n_capped) atomicAdd(&c->n_capped_groups, n_capped);
    }
}

void launch_consolidate(const RetireRows& x, const ConsWork& w, float radius, hipStream_t s) {
    if (w.n <= 0) return;
    const int blocks = (w.n + RETIRE_BLOCK - 1) / RETIRE_BLOCK, groups = (blocks + RETIRE_BLOCK - 1) / RETIRE_BLOCK;   // n <= 2^24: groups <= RETIRE_BLOCK
    const dim3 grid(blocks), block(RETIRE_BLOCK);
    hipLaunchKernelGGL(k_cons_insert, grid, block, 0, s, x.points, x.ids, w);
    hipLaunchKernelGGL(k_cons_place, grid, block, 0, s, x.points, x.ids, w);
    hipLaunchKernelGGL(k_cons_scan, grid, block, 0, s, w.offset, w.n, w.sums);
    hipLaunchKernelGGL(k_cons_scan, dim3(groups), block, 0, s, w.sums, blocks, w.sums + blocks);
    hipLaunchKernelGGL(k_cons_scan, dim3(1), block, 0, s, w.sums + blocks, groups, w.sums + blocks + RETIRE_BLOCK);
    hipLaunchKernelGGL(k_cons_offsets, grid, block, 0, s, w.offset, w.n, w.sums, blocks);
    hipLaunchKernelGGL(k_cons_scatter, grid, block, 0, s, x.points, x.ids, w);
    hipLaunchKernelGGL(k_cons_group, grid, block, 0, s, x, w, radius);
}
