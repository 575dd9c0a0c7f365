// svo_match_api.hip — host side of the descriptor index (include/svo.h, "Descriptor index"): the index object, the append copies,
// the batched search and the C-ABI.  An index owns one non-blocking stream and its own pinned staging; add and match wait for that
// stream alone, so they are legal beside any context's frames in flight.  The kernels are in svo_kernels_match.hip.
#include "svo_match_internal.hpp"
#include <stdio.h>
#include <string.h>
#include <vector>

#define MATCH_STAGE_ROWS 4096                         // rows of one staged upload, queries of one staged search
#define MATCH_DEFAULT_CHUNK 1024                      // rows of the index one block walks, unless svo_desc_index_set_chunk_rows says otherwise
#define MATCH_PART_BUDGET ((size_t)1 << 22)           // partial states of one launch (64 MiB): more chunks mean fewer queries per launch
#define MATCH_PART_FIRST ((size_t)1 << 12)            // the scratch's first size in partial states (64 KiB); it doubles from there

#define MHIP(expr)                                                                                \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            char _b[512];                                                                         \
            snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            svo_set_error(_b);                                                                    \
            return SVO_ERR_HIP;                                                                   \
        }                                                                                         \
    } while (0)

static int fail(int rc, const char* msg) { svo_set_error(msg); return rc; }

struct svo_desc_index {
    int device = 0, capacity = 0, size = 0, chunk_rows = MATCH_DEFAULT_CHUNK;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};            // around the two kernels of a launch, recorded while `timing` is on
    bool timing = false;                              // svo_desc_index_set_timing
    float last_ms = 0.f;                              // the last timed search's kernels, summed over its launches
    uint8_t* d_desc = nullptr;                        // [capacity][32]
    uint64_t* d_ids = nullptr;                        // [capacity]
    uint8_t* h_stage = nullptr;                       // pinned: MATCH_STAGE_ROWS descriptors (or queries), then MATCH_STAGE_ROWS ids
    svo_desc_match* h_out = nullptr;                  // pinned: MATCH_STAGE_ROWS result rows
    uint8_t* d_query = nullptr;                       // [MATCH_STAGE_ROWS][32]
    svo_desc_match* d_out = nullptr;                  // [MATCH_STAGE_ROWS]
    MatchPartial* d_part = nullptr;                   // [part_cap]: grows by doubling, never shrinks (part_room)
    size_t part_cap = 0, outgrown_states = 0;
    int part_allocs = 0;
    std::vector<void*> outgrown;                      // earlier d_part buffers: hipFree waits for the whole device, so they go with the index
};

static_assert(sizeof(svo_desc_match) == 32, "svo_desc_match is 32 bytes");

extern "C" void svo_desc_index_destroy(svo_desc_index* x) {
    if (!x) return;
    if (hipSetDevice(x->device) == hipSuccess) {
        if (x->stream) (void)hipStreamSynchronize(x->stream);
        for (hipEvent_t e : x->ev) if (e) (void)hipEventDestroy(e);
        for (void* p : x->outgrown) (void)hipFree(p);
        (void)hipFree(x->d_part); (void)hipFree(x->d_out); (void)hipFree(x->d_query); (void)hipFree(x->d_ids); (void)hipFree(x->d_desc);
        (void)hipHostFree(x->h_out); (void)hipHostFree(x->h_stage);
        if (x->stream) (void)hipStreamDestroy(x->stream);
    }
    delete x;
}

static int index_alloc(svo_desc_index* x) {
    MHIP(hipSetDevice(x->device));
    MHIP(hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking));
    MHIP(hipEventCreate(&x->ev[0])); MHIP(hipEventCreate(&x->ev[1]));
    MHIP(hipMalloc((void**)&x->d_desc, (size_t)x->capacity * SVO_DESC_BYTES));
    MHIP(hipMalloc((void**)&x->d_ids, (size_t)x->capacity * sizeof(uint64_t)));
    MHIP(hipMalloc((void**)&x->d_query, (size_t)MATCH_STAGE_ROWS * SVO_DESC_BYTES));
    MHIP(hipMalloc((void**)&x->d_out, (size_t)MATCH_STAGE_ROWS * sizeof(svo_desc_match)));
    MHIP(hipHostMalloc((void**)&x->h_stage, (size_t)MATCH_STAGE_ROWS * (SVO_DESC_BYTES + sizeof(uint64_t)), hipHostMallocDefault));
    MHIP(hipHostMalloc((void**)&x->h_out, (size_t)MATCH_STAGE_ROWS * sizeof(svo_desc_match), hipHostMallocDefault));
    return SVO_OK;
}

extern "C" int svo_desc_index_create(int device, int capacity, svo_desc_index** out) {
    if (!out) return fail(SVO_ERR_ARG, "svo_desc_index_create: null out");
    *out = nullptr;
    if (capacity < 1 || capacity > SVO_MATCH_MAX_ROWS) return fail(SVO_ERR_ARG, "svo_desc_index_create: capacity must be 1 .. 1 << 24 rows");
    svo_desc_index* x = new svo_desc_index;
    x->device = device; x->capacity = capacity;
    const int rc = index_alloc(x);
    if (rc != SVO_OK) { svo_desc_index_destroy(x); return rc; }
    *out = x;
    return SVO_OK;
}

extern "C" int svo_desc_index_size(const svo_desc_index* x) { return x ? x->size : fail(SVO_ERR_ARG, "null index"); }

extern "C" int svo_desc_index_truncate(svo_desc_index* x, int n_rows) {
    if (!x) return fail(SVO_ERR_ARG, "null index");
    if (n_rows < 0 || n_rows > x->size) return fail(SVO_ERR_ARG, "svo_desc_index_truncate: n_rows must be 0 .. size");
    x->size = n_rows;                                 // rows beyond size are never read: a search's range ends at size
    return SVO_OK;
}

extern "C" int svo_desc_index_set_chunk_rows(svo_desc_index* x, int rows) {
    if (!x) return fail(SVO_ERR_ARG, "null index");
    if (rows < 0 || rows > SVO_MATCH_MAX_ROWS) return fail(SVO_ERR_ARG, "svo_desc_index_set_chunk_rows: rows must be 0 (default) .. 1 << 24");
    x->chunk_rows = rows ? rows : MATCH_DEFAULT_CHUNK;
    return SVO_OK;
}
extern "C" int svo_desc_index_get_chunk_rows(const svo_desc_index* x) { return x ? x->chunk_rows : fail(SVO_ERR_ARG, "null index"); }

extern "C" int svo_desc_index_set_timing(svo_desc_index* x, int on) {
    if (!x) return fail(SVO_ERR_ARG, "null index");
    x->timing = on != 0; x->last_ms = 0.f;
    return SVO_OK;
}

extern "C" int svo_desc_index_get_stats(const svo_desc_index* x, svo_desc_index_stats* st) {
    if (!x || !st) return fail(SVO_ERR_ARG, "null index / stats");
    st->last_kernels_ms = x->last_ms;
    st->scratch_allocations = x->part_allocs;
    st->scratch_bytes = (uint64_t)x->part_cap * sizeof(MatchPartial);
    st->scratch_bytes_outgrown = (uint64_t)x->outgrown_states * sizeof(MatchPartial);
    return SVO_OK;
}

extern "C" int svo_desc_index_add(svo_desc_index* x, int n, const uint8_t* desc, const uint64_t* ids, int* first_row) {
    if (!x || n < 0 || (n > 0 && (!desc || !ids))) return fail(SVO_ERR_ARG, "svo_desc_index_add: bad index / n / desc / ids");
    if (n > x->capacity - x->size) return fail(SVO_ERR_ARG, "svo_desc_index_add: size + n exceeds the index's capacity (nothing was added)");
    if (first_row) *first_row = x->size;
    if (n == 0) return SVO_OK;
    MHIP(hipSetDevice(x->device));
    uint8_t* h_ids = x->h_stage + (size_t)MATCH_STAGE_ROWS * SVO_DESC_BYTES;
    for (int i0 = 0; i0 < n; i0 += MATCH_STAGE_ROWS) {  // size moves only after the last copy: a failure on the way adds nothing
        const size_t m = (size_t)(n - i0 < MATCH_STAGE_ROWS ? n - i0 : MATCH_STAGE_ROWS), at = (size_t)x->size + i0;
        memcpy(x->h_stage, desc + (size_t)i0 * SVO_DESC_BYTES, m * SVO_DESC_BYTES);
        memcpy(h_ids, ids + i0, m * sizeof(uint64_t));
        MHIP(hipMemcpyAsync(x->d_desc + at * SVO_DESC_BYTES, x->h_stage, m * SVO_DESC_BYTES, hipMemcpyHostToDevice, x->stream));
        MHIP(hipMemcpyAsync(x->d_ids + at, h_ids, m * sizeof(uint64_t), hipMemcpyHostToDevice, x->stream));
        MHIP(hipStreamSynchronize(x->stream));        // the staging is free again
    }
    x->size += n;
    return SVO_OK;
}

extern "C" int svo_desc_index_add_frame(svo_desc_index* x, svo_context* ctx, int seq, uint32_t need_flags, int* first_row, int* n_added) {
    if (!x) return fail(SVO_ERR_ARG, "null index");
    int n_tracks = 0;
    int rc = svo_get_last_track_descriptors(ctx, seq, 0, nullptr, &n_tracks);     // its refusals are this call's: context, seq, the frame's state
    if (rc < 0) return rc;
    std::vector<svo_track_obs> obs((size_t)(n_tracks > 0 ? n_tracks : 0));
    std::vector<uint8_t> desc(obs.size() * SVO_DESC_BYTES);
    const int n_obs = svo_get_last_track_obs(ctx, seq, (int)obs.size(), obs.data(), nullptr);
    if (n_obs < 0) return n_obs;
    rc = svo_get_last_track_descriptors(ctx, seq, n_obs, desc.data(), nullptr);
    if (rc < 0) return rc;
    std::vector<uint64_t> ids;
    int n = 0;
    for (int i = 0; i < rc; i++) {                    // the rows that carry need_flags, packed in row order
        if (((uint32_t)obs[i].flags & need_flags) != need_flags) continue;
        if (n != i) memcpy(&desc[(size_t)n * SVO_DESC_BYTES], &desc[(size_t)i * SVO_DESC_BYTES], SVO_DESC_BYTES);
        ids.push_back((uint64_t)obs[i].id);
        n++;
    }
    if (n_added) *n_added = 0;
    rc = svo_desc_index_add(x, n, desc.data(), ids.data(), first_row);
    if (rc == SVO_OK && n_added) *n_added = n;
    return rc;
}

// Room for `need` partial states.  The scratch at least doubles whenever it grows (from MATCH_PART_FIRST), so an index whose searches
// lengthen frame by frame allocates O(log) times and the buffers it has outgrown — kept until the index goes, since hipFree waits for
// the whole device — sum to less than the one in use.  Up to MATCH_PART_BUDGET the doubling stops at the budget, which every search
// of at most 65 536 chunks fits (svo_desc_index_match sizes its batches to it); beyond, a search needs 64 queries x its chunks.
static int part_room(svo_desc_index* x, size_t need) {
    if (need <= x->part_cap) return SVO_OK;
    size_t cap = x->part_cap ? 2 * x->part_cap : MATCH_PART_FIRST;
    while (cap < need) cap *= 2;
    if (need <= MATCH_PART_BUDGET && cap > MATCH_PART_BUDGET) cap = MATCH_PART_BUDGET;
    MatchPartial* p = nullptr;
    MHIP(hipMalloc((void**)&p, cap * sizeof(MatchPartial)));
    if (x->d_part) { x->outgrown.push_back(x->d_part); x->outgrown_states += x->part_cap; }
    x->d_part = p; x->part_cap = cap; x->part_allocs++;
    return SVO_OK;
}

extern "C" int svo_desc_index_match(svo_desc_index* x, int n, const uint8_t* query, int row_lo, int row_hi, svo_desc_match* out) {
    if (!x || n < 0 || (n > 0 && (!query || !out))) return fail(SVO_ERR_ARG, "svo_desc_index_match: bad index / n / query / out");
    if (row_hi == -1) row_hi = x->size;
    if (row_lo < 0 || row_hi > x->size || row_lo > row_hi) return fail(SVO_ERR_ARG, "svo_desc_index_match: the row range must satisfy 0 <= row_lo <= row_hi <= size");
    x->last_ms = 0.f;
    if (n == 0) return SVO_OK;
    MHIP(hipSetDevice(x->device));
    const MatchRange r = match_range(row_lo, row_hi, x->chunk_rows);
    size_t batch = MATCH_STAGE_ROWS;
    if (r.n_chunks > 0) {
        size_t fit = MATCH_PART_BUDGET / (size_t)r.n_chunks / 64 * 64;
        if (fit < 64) fit = 64;
        if (fit < batch) batch = fit;
        if ((size_t)n < batch) batch = (size_t)n;
        const int rc = part_room(x, batch * (size_t)r.n_chunks);
        if (rc != SVO_OK) return rc;
    }
    for (size_t i0 = 0; i0 < (size_t)n; i0 += batch) {
        const int m = (int)((size_t)n - i0 < batch ? (size_t)n - i0 : batch);
        memcpy(x->h_stage, query + i0 * SVO_DESC_BYTES, (size_t)m * SVO_DESC_BYTES);
        MHIP(hipMemcpyAsync(x->d_query, x->h_stage, (size_t)m * SVO_DESC_BYTES, hipMemcpyHostToDevice, x->stream));
        if (x->timing) MHIP(hipEventRecord(x->ev[0], x->stream));
        launch_desc_match((const uint32_t*)x->d_desc, x->d_ids, (const uint32_t*)x->d_query, m, r, x->d_part, x->stream);
        launch_desc_match_merge(x->d_part, x->d_ids, m, r, x->d_out, x->stream);
        MHIP(hipGetLastError());
        if (x->timing) MHIP(hipEventRecord(x->ev[1], x->stream));
        MHIP(hipMemcpyAsync(x->h_out, x->d_out, (size_t)m * sizeof(svo_desc_match), hipMemcpyDeviceToHost, x->stream));
        MHIP(hipStreamSynchronize(x->stream));
        memcpy(out + i0, x->h_out, (size_t)m * sizeof(svo_desc_match));
        if (x->timing) {
            float ms = 0.f;
            MHIP(hipEventElapsedTime(&ms, x->ev[0], x->ev[1]));
            x->last_ms += ms;
        }
    }
    return SVO_OK;
}
