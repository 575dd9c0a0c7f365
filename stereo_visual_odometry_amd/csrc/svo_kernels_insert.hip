// svo_kernels_insert.hip — the batched insertion of the descriptor index (include/svo.h, "Batched insertion"; the rules are in
// svo_insert.hpp).  Three launches ordered by the stream: no kernel waits for another workgroup, no atomics, so the order of the
// rows is fixed.  The observation and descriptor rows are read where the launch is given them: a slot of the context's host-mapped
// rings, in place over the host link, or a staged group in device memory.
//
// k_insert_count: a block per tile of 256 rows, a lane per row.  The lane reads the 4 bytes of its row's flags; each wave stores its
//   64 keep bits (__ballot) as one mask.  The masks are what the other two kernels read: the flags cross the link once.
// k_insert_scan: one block of 1024 lanes walks the tiles 1024 at a time: a tile's count is the popcount of its four masks, the
//   exclusive scan runs through wave shuffles and 64 bytes of LDS, a carry joins the rounds.  Then the lanes write the entries' counts
//   (differences of offsets) and lane 0 the control block: the total, and whether it exceeds the room.
// k_insert_put: returns at once, in every lane, when the control block says the rows do not fit.  Otherwise a lane whose bit is set
//   recomputes its rank from the tile's masks and writes its row at `at + offset[tile] + rank`: the descriptor (two 16-byte loads and
//   stores), the id plus the entry's offset, and on an index with points the 16-byte point row — through the entry's transform in
//   f64 (reloc_map_point), as it is, or SVO_POINT_NONE for the plain call.  A point that is not finite raises the control block's
//   flag with a plain store; the host then leaves `size` where it was, and rows beyond `size` are never read.
// Only the lanes of kept rows read more than the flags: 8 bytes of id, 12 of xyz and the 32 of the descriptor.
#include "svo_insert_internal.hpp"

// the tile's entry b, and the lane's row in it; false beyond the entry's rows
static __device__ __forceinline__ bool insert_lane_row(const InsertWork& w, int tile, int& b, InsertEntry& e, int& row) {
    b = insert_tile_entry(w.entry, w.n, tile);
    e = w.entry[b];
    const int r = (tile - e.tile0) * INSERT_TILE + (int)threadIdx.x;
    row = e.begin + r;
    return r < e.rows;
}

__global__ void __launch_bounds__(INSERT_TILE) k_insert_count(InsertWork w) {
    const int tile = (int)blockIdx.x;
    InsertEntry e; int b, row;
    bool keep = false;
    if (insert_lane_row(w, tile, b, e, row)) keep = insert_keep(*(const int32_t*)(w.obs + (size_t)row * INSERT_OBS_BYTES + INSERT_OBS_FLAGS), w.need);
    const uint64_t m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) w.mask[(size_t)tile * INSERT_TILE_WAVES + (threadIdx.x >> 6)] = m;
}

__global__ void __launch_bounds__(INSERT_SCAN_BLOCK) k_insert_scan(InsertWork w) {
    __shared__ int sh[INSERT_SCAN_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int t0 = 0; t0 < w.tiles; t0 += INSERT_SCAN_BLOCK) {         // uniform: every lane runs every round
        const int t = t0 + (int)threadIdx.x;
        const int mine = t < w.tiles ? insert_tile_count(w.mask + (size_t)t * INSERT_TILE_WAVES) : 0;
        int v = mine;
        for (int d = 1; d < 64; d <<= 1) { const int u = __shfl_up(v, d); if (lane >= d) v += u; }
        if (lane == 63) sh[wave] = v;
        __syncthreads();
        int before = 0, all = 0;
        for (int k = 0; k < INSERT_SCAN_BLOCK / 64; k++) { const int s = sh[k]; if (k < wave) before += s; all += s; }
        if (t < w.tiles) w.offset[t] = carry + before + v - mine;
        carry += all;
        __syncthreads();                                              // sh is free for the next round
    }
    if (threadIdx.x == 0) {
        w.offset[w.tiles] = carry;
        w.ctl->total = carry; w.ctl->over = carry > w.room ? 1 : 0; w.ctl->nonfinite = 0;
    }
    __syncthreads();                                                  // the offsets, written by this block, are read back by it
    for (int b = (int)threadIdx.x; b < w.n; b += INSERT_SCAN_BLOCK) {
        const InsertEntry e = w.entry[b];
        w.n_added[b] = w.offset[e.tile0 + insert_tiles(e.rows)] - w.offset[e.tile0];
    }
}

__global__ void __launch_bounds__(INSERT_TILE) k_insert_put(InsertRows x, InsertWork w) {
    if (w.ctl->over) return;                                          // the same word in every lane of every block
    const int tile = (int)blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t mask[INSERT_TILE_WAVES];
    for (int k = 0; k < INSERT_TILE_WAVES; k++) mask[k] = w.mask[(size_t)tile * INSERT_TILE_WAVES + k];
    if (!insert_kept(mask, wave, lane)) return;                       // a set bit is a row inside its entry
    InsertEntry e; int b, row;
    insert_lane_row(w, tile, b, e, row);
    const size_t to = (size_t)(w.at + w.offset[tile] + insert_rank(mask, wave, lane));   // < at + total <= at + room: inside the index
    const uint4* d = (const uint4*)(w.desc + (size_t)row * INSERT_DESC_BYTES);
    const uint4 d0 = d[0], d1 = d[1];
    uint4* out = (uint4*)(x.desc + to * INSERT_DESC_BYTES);
    out[0] = d0; out[1] = d1;
    const uint8_t* o = w.obs + (size_t)row * INSERT_OBS_BYTES;
    x.ids[to] = insert_id(*(const int64_t*)(o + INSERT_OBS_ID), e.id_base);
    if (!x.points) return;
    uint4 pt = make_uint4(0u, 0u, 0u, (uint32_t)SVO_RELOC_POINT_NONE);
    if (w.with_points) {
        const float* xyz = (const float*)(o + INSERT_OBS_XYZ);
        const float p[3] = {xyz[0], xyz[1], xyz[2]};
        float q[3];
        insert_point(w.T ? w.T + 12 * (size_t)b : nullptr, p, q);
        if (!insert_point_ok(q)) w.ctl->nonfinite = 1;
        pt = make_uint4(__float_as_uint(q[0]), __float_as_uint(q[1]), __float_as_uint(q[2]), (uint32_t)e.tag);
    }
    x.points[to] = pt;
}

void launch_insert(const InsertRows& x, const InsertWork& w, hipStream_t s) {
    if (w.tiles <= 0) return;
    hipLaunchKernelGGL(k_insert_count, dim3((unsigned)w.tiles), dim3(INSERT_TILE), 0, s, w);
    hipLaunchKernelGGL(k_insert_scan, dim3(1), dim3(INSERT_SCAN_BLOCK), 0, s, w);
    hipLaunchKernelGGL(k_insert_put, dim3((unsigned)w.tiles), dim3(INSERT_TILE), 0, s, x, w);
}
