// svo_match_api.hip — host side of the descriptor index (include/svo.h, "Descriptor index" to "Batched insertion"): the index object,
// the append copies, the search and the C-ABI.  An index owns one non-blocking stream and its own pinned staging; every call waits
// for that stream alone, so it is legal beside any context's frames in flight.
//
// Memory: every block of an index, device or pinned, comes from index_block, which records it; svo_desc_index_destroy frees what is
// recorded and nothing is freed before (hipFree waits for the whole device).  An allocate-once pointer takes its block through room,
// a buffer that grows — the partial states, the maintenance scratch, the pinned blocks of places and of staged rows — through grow,
// by the capacity rule of svo_match.hpp; the batch's staging keeps its own rule (rb_grow).
// Timing (svo_desc_index_set_timing): a call marks the one span it times (span_mark) and reads it after its wait (span_read) into its
// figure: last_ms, the maintenance calls' retire_ms, the batched insertion's insert_ms.  match times one span per stage and sums.
//
// The search: row_range settles the rows, search_plan the launch geometry and its room, stage_queries puts up to MATCH_STAGE_ROWS
// queries and their pixels on the device, and search_enqueue puts the search on the stream — k_desc_match, or with a guide
// k_guide_project and k_desc_match_guided, or for a near plan k_desc_match_near, then k_desc_match_merge — and leaves d_out[0 .. n)
// without waiting.  rows_down ends a call, or a stage, that returns those rows: match, match_guided, match_rows, match_near.
//
// Relocalisation: reloc_run, behind select and localize with or without a guide, puts the selection (select_enqueue) and the
// RANSAC-PnP kernels behind the search, the candidate lists down (cands_down) and waits once.  localize_batch (the kernels are in
// svo_kernels_reloc_batch.hip, the plan in svo_reloc_batch.hpp) is that for many cameras, with a staging (batch_room) and a PnP stage
// context of its own; both share the parameters' refusals, the state row (reloc_state_row) and the reading of a camera (reloc_read).
//
// The pair stage (pairs_enqueue, pairs_read) follows a search whose queries are rows of the index.  align_run, behind match_rows,
// pair_rows and align (svo_kernels_align.hip, svo_align.hpp), adds k_align_score and k_align_fit; fuse_run, behind match_near,
// pair_near and fuse (svo_kernels_fuse.hip, svo_fuse.hpp), searches near and adds k_fuse_map and the relabelling, which relabel runs
// alone on host lists (fuse_begin puts either's lists, control block and table in place).  One copy back, or two, and one wait.
//
// Place candidates (svo_kernels_place.hip, svo_place.hpp): place_run, behind tag_votes, places and places_from_ids, is — for places —
// the unguided search and the selection, else the id list up (upload_list), then the sweep and the pick, the copies back, one wait.
// place_batch_run (svo_kernels_place_batch.hip, svo_place_batch.hpp), behind tag_votes_batch, places_batch and places_from_ids_batch,
// is that for many cameras: localize_batch's staging, unguided search and selection without its PnP, or the offsets and the ids up,
// then one table of (id, camera) pairs, one sweep for all cameras and a pick block per camera, one copy back or two, one wait.
//
// Maintenance (svo_kernels_retire.hip, svo_kernels_consolidate.hip): retire puts its flags, table and ranks on the stream, consolidate
// the group kernel and the ranks; retire_finish is the end of both — the first wait, before which nothing has moved, the ranks down,
// the move of the rows slab by slab and the second wait, the map, size.  transform_points is one launch and one wait.  read_rows is
// index_add's staging run downwards.
//
// Batched insertion (svo_kernels_insert.hip, svo_insert.hpp): add_frames and add_frames_points settle their refusals and the
// entries' rows from the context's last-frame view, then insert_group puts the entries up, runs the kernels over the ring slot in
// place — or, group by group, over rows staged through a pinned buffer (insert_staged, which is all of add_obs) — brings the counts
// and the flags back and waits; size moves once, at the end.  The single calls (add_frame_rows) are untouched.
#include "svo_guide_internal.hpp"
#include "svo_retire_internal.hpp"
#include "svo_reloc_batch_internal.hpp"
#include "svo_align_internal.hpp"
#include "svo_fuse_internal.hpp"
#include "svo_place_internal.hpp"
#include "svo_place_batch_internal.hpp"
#include "svo_consolidate_internal.hpp"
#include "svo_insert_internal.hpp"
#include <algorithm>
#include <math.h>
#include <stddef.h>
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
// the refusal of a call that needs points on an index without them, under the call's prefix (svo_set_error copies its argument)
static int no_points(const char* prefix) {
    char b[192];
    snprintf(b, sizeof(b), "%s: the index has no points (svo_desc_index_enable_points)", prefix);
    return fail(SVO_ERR_STATE, b);
}

struct RelocDevOut;
struct RelocHost;
struct RetireDown { RetireCtl ctl; int32_t kept, pad[3]; };   // a retire call reads ctl.table_full and kept, a transform the whole ctl
// A buffer that grows by match_grow_capacity and never shrinks: its bytes, the bytes of the buffers it has outgrown, its allocations
struct GrowBuf { uint8_t* p = nullptr; size_t cap = 0, outgrown = 0; int allocs = 0; };
struct svo_desc_index {
    int device = 0, capacity = 0, size = 0, chunk_rows = MATCH_DEFAULT_CHUNK;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};            // around the span a call times, recorded while `timing` is on (span_mark)
    bool timing = false;                              // svo_desc_index_set_timing
    float last_ms = 0.f;                              // the last call's timed span, summed over its stages (span_read)
    uint8_t* d_desc = nullptr;                        // [capacity][32]
    uint64_t* d_ids = nullptr;                        // [capacity]
    uint8_t* h_stage = nullptr;                       // pinned: MATCH_STAGE_ROWS descriptors (or queries), then MATCH_STAGE_ROWS ids (or pixels)
    svo_desc_match* h_out = nullptr;                  // pinned: MATCH_STAGE_ROWS result rows
    uint8_t* d_query = nullptr;                       // [MATCH_STAGE_ROWS][32]
    svo_desc_match* d_out = nullptr;                  // [MATCH_STAGE_ROWS]
    std::vector<void*> dev_blocks, pinned_blocks;     // every block the index has allocated (index_block), outgrown ones included: hipFree waits for the whole device, so all go with the index
    GrowBuf part;                                     // the partial states of a search, as bytes (grow, PART_*)
    MatchPartial* d_part() const { return (MatchPartial*)part.p; }
    // svo_desc_index_enable_points: all null without
    RelocPoint* d_points = nullptr;                   // [capacity]
    float2* d_qxy = nullptr;                          // [MATCH_STAGE_ROWS] the queries' pixels
    RelocDevOut* d_reloc = nullptr;                   // what k_reloc_select reports
    RelocHost* h_reloc = nullptr;                     // pinned: the point rows of an upload, a call's state row and everything it reads back
    // the guided search: null until the first guided call (guide_room)
    float2* d_uv = nullptr;                           // [capacity] the rows' projections of the call in progress
    int32_t* d_order = nullptr;                       // [MATCH_STAGE_ROWS] the query each lane slot serves
    int32_t* h_order = nullptr;                       // pinned, likewise
    bool guided_sort = true;                          // svo_desc_index_set_guided_sort
    // index maintenance: null until the first call that needs them (retire_ctl_room, grow)
    int retire_slab = RETIRE_DEFAULT_SLAB;            // svo_desc_index_set_retire_slab_rows
    GrowBuf retire;                                   // the maintenance scratch, cut by retire_layout and the later features' layouts
    float retire_ms = 0.f;                            // the last maintenance call's kernels, with timing on
    RetireCtl* d_retire_ctl = nullptr;
    RetireDown* h_retire = nullptr;                   // pinned: what a call reads back before it decides
    // batched relocalisation: all null until the first svo_desc_index_localize_batch (batch_room)
    uint8_t* d_batch = nullptr;                       // the device staging: room for rb_layout(batch_cams, batch_queries), cut per call
    uint8_t* h_batch = nullptr;                       // pinned: its first down_end bytes, cut alike
    SeqState* h_batch_st = nullptr;                   // pinned: [2][batch_cams] the state rows going up, and as k_pnp_final left them
    size_t batch_cams = 0, batch_queries = 0;         // each at least doubles when it grows
    svo_context* batch_ctx = nullptr;                 // the PnP stage context of B sequences (svo_reloc_batch_ctx)
    std::vector<svo_context*> batch_ctx_outgrown;     // earlier ones, destroyed with the index
    int batch_last_cams = 0, batch_total = -1;                             // the last batch call's queries (-1: none yet), and whether d_batch holds its order
    bool batch_ordered = false;
    // map alignment: null until the first svo_desc_index_pair_rows or svo_desc_index_align (align_room)
    uint8_t* d_align = nullptr;                       // align_layout(ALIGN_MAX_ROWS, ALIGN_MAX_HYPOTHESES)
    uint8_t* h_align = nullptr;                       // pinned: its first down_end bytes
    // landmark fusion: null until the first pair_near, relabel or fuse (fuse_ctl_room); the lists and the table live in the maintenance scratch
    FuseCtl* h_fuse = nullptr;                        // pinned: what a call reads back
    // place candidates: null until the first tag_votes, places or places_from_ids (grow); the device side lives in the maintenance scratch
    GrowBuf place;                                    // pinned: a PlaceCtl, then tag_votes' bins; a batch call's PbStage
    bool place_combine = true;                        // svo_desc_index_set_place_combine
    // batched insertion: null until the first add_frames, add_frames_points or add_obs (insert_host_room, grow); the device side lives in the maintenance scratch
    uint8_t* h_insert = nullptr;                      // pinned: the entries and transforms going up, then (at INSERT_HOST_DOWN) the control block and the counts coming down
    GrowBuf insert_rows;                              // pinned: a staged group's observation rows, then its descriptor rows
    float insert_ms = 0.f;                            // the last batched insertion's kernels, with timing on
    int insert_path = 0;                              // SVO_INSERT_PATH_* of the last batched insertion
    uint64_t insert_scanned = 0, insert_added = 0;
};

// k_reloc_select's result lists, on the device and in the pinned block: the count and the queries lead, so that one copy takes both
struct RelocDevOut { int32_t n_cand, pad[3]; int32_t cand_query[MATCH_STAGE_ROWS], cand_row[MATCH_STAGE_ROWS]; };
struct RelocHost {
    RelocPoint points[MATCH_STAGE_ROWS];
    SeqState up, down;                                // the state row going in, and as k_pnp_final left it
    RelocDevOut out;
    uint8_t inlier[MATCH_STAGE_ROWS];
    float cand_xy[MATCH_STAGE_ROWS * 2], cand_xyz[MATCH_STAGE_ROWS * 3];
};
static_assert(sizeof(RelocPoint) == 16, "a point row is 16 bytes");
static_assert(MATCH_STAGE_ROWS == SVO_RELOC_MAX_QUERIES, "one staged search per relocalisation");

static_assert(sizeof(svo_desc_match) == 32, "svo_desc_match is 32 bytes");

extern "C" void svo_desc_index_destroy(svo_desc_index* x) {
    if (!x) return;
    if (hipSetDevice(x->device) == hipSuccess) {
        if (x->stream) (void)hipStreamSynchronize(x->stream);
        for (void* p : x->dev_blocks) (void)hipFree(p);
        for (void* p : x->pinned_blocks) (void)hipHostFree(p);
        for (svo_context* c : x->batch_ctx_outgrown) svo_destroy(c);
        svo_destroy(x->batch_ctx);
        for (hipEvent_t e : x->ev) if (e) (void)hipEventDestroy(e);
        if (x->stream) (void)hipStreamDestroy(x->stream);
    }
    delete x;
}

// The one allocator: a block of device or pinned memory that the index owns from here on and frees when it goes, not before.
static int index_block(svo_desc_index* x, void** p, size_t bytes, bool pinned) {
    if (pinned) MHIP(hipHostMalloc(p, bytes, hipHostMallocDefault)); else MHIP(hipMalloc(p, bytes));
    (pinned ? x->pinned_blocks : x->dev_blocks).push_back(*p);
    return SVO_OK;
}
// An allocate-once pointer: a block for it unless it has one.  A room of several is one of these each, so a call that comes back
// after a failed allocation takes up where that one stopped.
template <class T> static int room(svo_desc_index* x, T*& p, size_t bytes, bool pinned) { return p ? SVO_OK : index_block(x, (void**)&p, bytes, pinned); }
#define ROOM(call) do { if (const int _rc = (call); _rc != SVO_OK) return _rc; } while (0)

// Room for `need` bytes in a growable buffer, by the rule of match_grow_capacity (svo_match.hpp).  The buffer it outgrows stays the
// index's block until the index goes; its bytes are counted.
static int grow(svo_desc_index* x, GrowBuf& b, size_t need, size_t first, size_t clamp, bool pinned) {
    const size_t cap = match_grow_capacity(b.cap, need, first, clamp);
    if (cap == b.cap) return SVO_OK;
    void* p = nullptr;
    ROOM(index_block(x, &p, cap, pinned));
    b.outgrown += b.cap; b.p = (uint8_t*)p; b.cap = cap; b.allocs++;
    return SVO_OK;
}

static int index_alloc(svo_desc_index* x) {
    MHIP(hipSetDevice(x->device));
    MHIP(hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking));
    MHIP(hipEventCreate(&x->ev[0])); MHIP(hipEventCreate(&x->ev[1]));
    ROOM(room(x, x->d_desc, (size_t)x->capacity * SVO_DESC_BYTES, false));
    ROOM(room(x, x->d_ids, (size_t)x->capacity * sizeof(uint64_t), false));
    ROOM(room(x, x->d_query, (size_t)MATCH_STAGE_ROWS * SVO_DESC_BYTES, false));
    ROOM(room(x, x->d_out, (size_t)MATCH_STAGE_ROWS * sizeof(svo_desc_match), false));
    ROOM(room(x, x->h_stage, (size_t)MATCH_STAGE_ROWS * (SVO_DESC_BYTES + sizeof(uint64_t)), true));
    ROOM(room(x, x->h_out, (size_t)MATCH_STAGE_ROWS * sizeof(svo_desc_match), true));
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
    st->scratch_allocations = x->part.allocs;
    st->scratch_bytes = (uint64_t)x->part.cap;
    st->scratch_bytes_outgrown = (uint64_t)x->part.outgrown;
    return SVO_OK;
}

// the append behind svo_desc_index_add (pts null) and svo_desc_index_add_points: on an index with points a row without one is SVO_POINT_NONE
static int index_add(svo_desc_index* x, int n, const uint8_t* desc, const uint64_t* ids, const RelocPoint* pts, int* first_row) {
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
        if (x->d_points) {
            for (size_t i = 0; i < m; i++) x->h_reloc->points[i] = pts ? pts[i0 + i] : RelocPoint{0.f, 0.f, 0.f, SVO_POINT_NONE};
            MHIP(hipMemcpyAsync(x->d_points + at, x->h_reloc->points, m * sizeof(RelocPoint), hipMemcpyHostToDevice, x->stream));
        }
        MHIP(hipStreamSynchronize(x->stream));        // the staging is free again
    }
    x->size += n;
    return SVO_OK;
}

extern "C" int svo_desc_index_add(svo_desc_index* x, int n, const uint8_t* desc, const uint64_t* ids, int* first_row) {
    if (!x || n < 0 || (n > 0 && (!desc || !ids))) return fail(SVO_ERR_ARG, "svo_desc_index_add: bad index / n / desc / ids");
    return index_add(x, n, desc, ids, nullptr, first_row);
}

extern "C" int svo_desc_index_enable_points(svo_desc_index* x) {
    if (!x) return fail(SVO_ERR_ARG, "null index");
    if (x->size != 0) return fail(SVO_ERR_STATE, "svo_desc_index_enable_points: the index already holds rows (points are enabled on an empty index)");
    MHIP(hipSetDevice(x->device));
    ROOM(room(x, x->h_reloc, sizeof(RelocHost), true));
    ROOM(room(x, x->d_qxy, (size_t)MATCH_STAGE_ROWS * sizeof(float2), false));
    ROOM(room(x, x->d_reloc, sizeof(RelocDevOut), false));
    return room(x, x->d_points, (size_t)x->capacity * sizeof(RelocPoint), false);          // d_points is what says "enabled"
}

// the point rows of an append: finite coordinates, tags >= 0 (null: 0)
static int make_points(int n, const float* xyz, const int32_t* tags, int32_t tag, std::vector<RelocPoint>& pts) {
    pts.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        const int32_t t = tags ? tags[i] : tag;
        if (t < 0) return fail(SVO_ERR_ARG, "a point's tag must be >= 0 (nothing was added)");
        if (!isfinite(xyz[3 * i]) || !isfinite(xyz[3 * i + 1]) || !isfinite(xyz[3 * i + 2])) return fail(SVO_ERR_ARG, "a point has a non-finite coordinate (nothing was added)");
        pts[(size_t)i] = RelocPoint{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], t};
    }
    return SVO_OK;
}

extern "C" int svo_desc_index_add_points(svo_desc_index* x, int n, const uint8_t* desc, const uint64_t* ids, const float* xyz,
                                         const int32_t* tags, int* first_row) {
    if (!x || n < 0 || (n > 0 && (!desc || !ids || !xyz))) return fail(SVO_ERR_ARG, "svo_desc_index_add_points: bad index / n / desc / ids / xyz");
    if (!x->d_points) return no_points("svo_desc_index_add_points");
    std::vector<RelocPoint> pts;
    const int rc = make_points(n, xyz, tags, 0, pts);
    if (rc != SVO_OK) return rc;
    return index_add(x, n, desc, ids, pts.data(), first_row);
}

// svo_desc_index_add_frame (T null, no points) and svo_desc_index_add_frame_points (with_points: every row's xyz through T, or as it is)
static int add_frame_rows(svo_desc_index* x, svo_context* ctx, int seq, uint32_t need_flags, bool with_points, const double* T, int32_t tag,
                          int* first_row, int* n_added) {
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
    std::vector<float> xyz;
    int n = 0;
    for (int i = 0; i < rc; i++) {                    // the rows that carry need_flags, packed in row order
        if (((uint32_t)obs[i].flags & need_flags) != need_flags) continue;
        if (n != i) memcpy(&desc[(size_t)n * SVO_DESC_BYTES], &desc[(size_t)i * SVO_DESC_BYTES], SVO_DESC_BYTES);
        ids.push_back((uint64_t)obs[i].id);
        if (with_points) {
            float p[3] = {obs[i].xyz[0], obs[i].xyz[1], obs[i].xyz[2]};
            if (T) reloc_map_point(T, obs[i].xyz, p);
            xyz.insert(xyz.end(), p, p + 3);
        }
        n++;
    }
    if (n_added) *n_added = 0;
    std::vector<RelocPoint> pts;
    if (with_points && (rc = make_points(n, xyz.data(), nullptr, tag, pts)) != SVO_OK) return rc;
    rc = index_add(x, n, desc.data(), ids.data(), with_points ? pts.data() : nullptr, first_row);
    if (rc == SVO_OK && n_added) *n_added = n;
    return rc;
}

extern "C" int svo_desc_index_add_frame(svo_desc_index* x, svo_context* ctx, int seq, uint32_t need_flags, int* first_row, int* n_added) {
    if (!x) return fail(SVO_ERR_ARG, "null index");
    return add_frame_rows(x, ctx, seq, need_flags, false, nullptr, 0, first_row, n_added);
}

extern "C" int svo_desc_index_add_frame_points(svo_desc_index* x, svo_context* ctx, int seq, uint32_t need_flags, const double* cam_to_map,
                                               int32_t tag, int* first_row, int* n_added) {
    if (!x) return fail(SVO_ERR_ARG, "null index");
    if (!x->d_points) return no_points("svo_desc_index_add_frame_points");
    if (tag < 0) return fail(SVO_ERR_ARG, "svo_desc_index_add_frame_points: the tag must be >= 0");
    if (cam_to_map) for (int i = 0; i < 16; i++) if (!isfinite(cam_to_map[i])) return fail(SVO_ERR_ARG, "svo_desc_index_add_frame_points: cam_to_map has a non-finite entry");
    return add_frame_rows(x, ctx, seq, need_flags | SVO_OBS_HAS_XYZ, true, cam_to_map, tag, first_row, n_added);
}

// ---- the search: rows, plan, staging, enqueue, timing (the header comment has the path) ----
// the one row-range rule: row_hi == -1 is the index's size
static int row_range(const svo_desc_index* x, int& row_lo, int& row_hi) {
    if (row_hi == -1) row_hi = x->size;
    if (row_lo < 0 || row_hi > x->size || row_lo > row_hi) return fail(SVO_ERR_ARG, "the row range must satisfy 0 <= row_lo <= row_hi <= size");
    return SVO_OK;
}

// Room for `states` partial states (grow).  Up to the budget the doubling stops at the budget, which every search of at most 65 536
// chunks fits (search_plan sizes a launch to it); beyond, a search needs 64 queries x its chunks.
static int part_states(svo_desc_index* x, size_t states) {
    return grow(x, x->part, states * sizeof(MatchPartial), MATCH_PART_FIRST * sizeof(MatchPartial), MATCH_PART_BUDGET * sizeof(MatchPartial), false);
}

// the buffers of the guided search, allocated at the first guided call
static int guide_room(svo_desc_index* x) {
    ROOM(room(x, x->h_order, (size_t)MATCH_STAGE_ROWS * sizeof(int32_t), true));
    ROOM(room(x, x->d_order, (size_t)MATCH_STAGE_ROWS * sizeof(int32_t), false));
    return room(x, x->d_uv, (size_t)x->capacity * sizeof(float2), false);
}

// a guided search's prior as the kernels read it, and the caller's pixels, which order its lanes (guide_order)
struct SearchGuide { GuidePose pose; float radius; const float* xy; };

// a guided call's own refusals, and its guide
static int guide_check(const svo_desc_index* x, const float* K, const svo_reloc_guide* g, const float* xy, SearchGuide* sg) {
    if (!x || !K || !g) return fail(SVO_ERR_ARG, "guided search: null index / K / guide");
    if (!x->d_points) return no_points("guided search");
    if (!isfinite(g->radius) || g->radius < 0.f) return fail(SVO_ERR_ARG, "guided search: the radius must be finite and >= 0");
    for (int i = 0; i < 9; i++) if (!isfinite(g->R[i]) || !isfinite(K[i])) return fail(SVO_ERR_ARG, "guided search: R or K has a non-finite entry");
    for (int i = 0; i < 3; i++) if (!isfinite(g->t[i])) return fail(SVO_ERR_ARG, "guided search: t has a non-finite entry");
    *sg = SearchGuide{guide_pose(g->R, g->t, K), g->radius, xy};
    return SVO_OK;
}

// The order in which the lanes of a guided search serve the n queries, into h_order.  A wave skips a row only when none of its 64
// queries admits it, so queries that sit close together in the image share a wave: sorted by image cell (side 2 * radius, 1 px at
// least; cells in raster order; a non-finite pixel last), ties by j.  Sort off: 0 .. n - 1.  The results do not depend on it.
static void guide_order(const svo_desc_index* x, int n, const float* xy, float radius, int32_t* order) {
    for (int j = 0; j < n; j++) order[j] = j;
    if (!x->guided_sort || !xy) return;
    const double side = 2. * (double)radius > 1. ? 2. * (double)radius : 1.;
    const int64_t lim = (int64_t)1 << 30;
    std::vector<int64_t> key((size_t)n);
    for (int j = 0; j < n; j++) {
        const double cx = floor((double)xy[2 * j] / side), cy = floor((double)xy[2 * j + 1] / side);
        if (!isfinite(cx) || !isfinite(cy)) { key[(size_t)j] = INT64_MAX; continue; }
        const int64_t ix = cx < (double)-lim ? -lim : cx > (double)lim ? lim : (int64_t)cx, iy = cy < (double)-lim ? -lim : cy > (double)lim ? lim : (int64_t)cy;
        key[(size_t)j] = (iy + lim) * (2 * lim + 1) + (ix + lim);
    }
    std::sort(order, order + n, [&](int32_t a, int32_t b) { return key[(size_t)a] != key[(size_t)b] ? key[(size_t)a] < key[(size_t)b] : a < b; });
}

// The plan of a search of n <= MATCH_STAGE_ROWS queries: its rows in chunks, the queries of one launch, and the guide if it has one.
// near_lo >= 0: the queries are rows near_lo .. of the index and a row competes only within near_radius of the query's point (fuse_run).
struct SearchPlan { MatchRange r; int batch; const SearchGuide* guide; int near_lo = -1; float near_radius = 0.f; };

// The two ways a search fits the partial-state budget, and the room for the one chosen.  Unguided: the chunks stay as they are set
// and the queries go in launches of the largest multiple of 64 (64 at least) whose partial states fit.  Guided: the partial states
// are stored under the queries' own numbers, so the search is one launch over all of them, and the rows of a chunk double until it
// fits (n <= 4096 and at most 1 << 24 rows: 16 384 rows a chunk at most).  The results depend on neither.
static int search_plan(svo_desc_index* x, int n, int row_lo, int row_hi, const SearchGuide* guide, SearchPlan* p) {
    int chunk_rows = x->chunk_rows;
    *p = SearchPlan{match_range(row_lo, row_hi, chunk_rows), n, guide};    // not near: fuse_run says so itself
    if (guide) {
        if (const int rc = guide_room(x); rc != SVO_OK) return rc;
        while ((size_t)n * (size_t)p->r.n_chunks > MATCH_PART_BUDGET) p->r = match_range(row_lo, row_hi, chunk_rows *= 2);
    } else if (p->r.n_chunks > 0) {
        size_t fit = MATCH_PART_BUDGET / (size_t)p->r.n_chunks / 64 * 64;
        if (fit < 64) fit = 64;
        if (fit < (size_t)n) p->batch = (int)fit;
    }
    return p->batch > 0 && p->r.n_chunks > 0 ? part_states(x, (size_t)p->batch * (size_t)p->r.n_chunks) : SVO_OK;
}

// The one staging step: n <= MATCH_STAGE_ROWS queries into d_query and, for a call that has pixels, their pixels into d_qxy (xy
// null: zeros).  The pixels ride in the ids' part of the pinned staging, 8 bytes a row.  The staging is free: every call ends in a wait.
static int stage_queries(svo_desc_index* x, int n, const uint8_t* query, bool pixels, const float* xy) {
    if (n <= 0) return SVO_OK;
    memcpy(x->h_stage, query, (size_t)n * SVO_DESC_BYTES);
    MHIP(hipMemcpyAsync(x->d_query, x->h_stage, (size_t)n * SVO_DESC_BYTES, hipMemcpyHostToDevice, x->stream));
    if (!pixels) return SVO_OK;
    float* h_xy = (float*)(x->h_stage + (size_t)MATCH_STAGE_ROWS * SVO_DESC_BYTES);
    if (xy) memcpy(h_xy, xy, (size_t)n * sizeof(float2)); else memset(h_xy, 0, (size_t)n * sizeof(float2));
    MHIP(hipMemcpyAsync(x->d_qxy, h_xy, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, x->stream));
    return SVO_OK;
}

// The timing bracket.  A call begins by clearing last_ms; it marks both edges of the one span it times (`here`: this is that span),
// and reads the span after its wait into its figure: last_ms, or the maintenance calls' retire_ms, or the batched insertion's
// insert_ms.  With timing off nothing is recorded and the figure stays 0.
static hipError_t call_begin(svo_desc_index* x) { x->last_ms = 0.f; return hipSetDevice(x->device); }
static hipError_t span_mark(svo_desc_index* x, bool here, int edge) { return x->timing && here ? hipEventRecord(x->ev[edge], x->stream) : hipSuccess; }
static hipError_t span_read(svo_desc_index* x, float& figure) {
    float ms = 0.f;
    const hipError_t e = x->timing ? hipEventElapsedTime(&ms, x->ev[0], x->ev[1]) : hipSuccess;
    figure += ms;
    return e;
}

// The one enqueue: the search of the n staged queries (stage_queries) by plan p on the index's stream, d_out[0 .. n) when it has run;
// no wait.  Guided: the lane order up, the projection, and one launch of the guided kernel.  Unguided: launches of p.batch queries
// (a multiple of 64 rows, or all of them) back to back, of the plain kernel or, for a near plan, the gated one.  timed: the search is
// the span the call times, or its beginning.  from: the queries where they are not the staged ones — rows of the index itself (align_run).
static int search_enqueue(svo_desc_index* x, const SearchPlan& p, int n, bool timed, const uint8_t* from = nullptr) {
    const SearchGuide* g = p.guide;
    if (g && n > 0) {
        guide_order(x, n, g->xy, g->radius, x->h_order);
        MHIP(hipMemcpyAsync(x->d_order, x->h_order, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, x->stream));
    }
    MHIP(span_mark(x, timed, 0));
    if (g) launch_guide_project(x->d_points, g->pose, p.r.row_lo, p.r.row_hi, x->d_uv, x->stream);
    for (int i0 = 0; i0 < n; i0 += p.batch) {         // guided: p.batch == n
        const int m = n - i0 < p.batch ? n - i0 : p.batch;
        const uint32_t* query = (const uint32_t*)((from ? from : x->d_query) + (size_t)i0 * SVO_DESC_BYTES);
        if (g) launch_desc_match_guided((const uint32_t*)x->d_desc, x->d_ids, x->d_uv, query, x->d_qxy, x->d_order, m, g->radius, p.r, x->d_part(), x->stream);
        else if (p.near_lo >= 0) launch_desc_match_near((const uint32_t*)x->d_desc, x->d_ids, x->d_points, p.near_lo + i0, m, p.near_radius, p.r, x->d_part(), x->stream);
        else launch_desc_match((const uint32_t*)x->d_desc, x->d_ids, query, m, p.r, x->d_part(), x->stream);
        launch_desc_match_merge(x->d_part(), x->d_ids, m, p.r, x->d_out + i0, x->stream);
    }
    MHIP(hipGetLastError());
    MHIP(span_mark(x, timed, 1));
    return SVO_OK;
}

// The end of a call, or of a stage, that returns the search's result rows: d_out[0 .. n) down, the wait, the rows out, the span read.
static int rows_down(svo_desc_index* x, int n, svo_desc_match* out) {
    if (n > 0) MHIP(hipMemcpyAsync(x->h_out, x->d_out, (size_t)n * sizeof(svo_desc_match), hipMemcpyDeviceToHost, x->stream));
    MHIP(hipStreamSynchronize(x->stream));
    if (n > 0) memcpy(out, x->h_out, (size_t)n * sizeof(svo_desc_match));
    MHIP(span_read(x, x->last_ms));
    return SVO_OK;
}

// What match and match_guided share: the row range, then stage by stage (a guided call is one stage) the queries up, the search,
// the result rows back and the wait.  times: the search kernels (guided: with the projection), one span per stage
static int match_run(svo_desc_index* x, const SearchGuide* guide, int n, const uint8_t* query, int row_lo, int row_hi, svo_desc_match* out) {
    int rc = row_range(x, row_lo, row_hi);
    if (rc != SVO_OK) return rc;
    MHIP(call_begin(x));
    if (n == 0) return SVO_OK;
    SearchPlan plan;
    if ((rc = search_plan(x, n < MATCH_STAGE_ROWS ? n : MATCH_STAGE_ROWS, row_lo, row_hi, guide, &plan)) != SVO_OK) return rc;
    for (int i0 = 0; i0 < n; i0 += MATCH_STAGE_ROWS) {
        const int m = n - i0 < MATCH_STAGE_ROWS ? n - i0 : MATCH_STAGE_ROWS;
        if ((rc = stage_queries(x, m, query + (size_t)i0 * SVO_DESC_BYTES, guide != nullptr, guide ? guide->xy : nullptr)) != SVO_OK ||
            (rc = search_enqueue(x, plan, m, true)) != SVO_OK || (rc = rows_down(x, m, out + i0)) != SVO_OK) return rc;
    }
    return SVO_OK;
}

extern "C" int svo_desc_index_match(svo_desc_index* x, int n, const uint8_t* query, int row_lo, int row_hi, svo_desc_match* out) {
    if (!x || n < 0 || (n > 0 && (!query || !out))) return fail(SVO_ERR_ARG, "svo_desc_index_match: bad index / n / query / out");
    return match_run(x, nullptr, n, query, row_lo, row_hi, out);
}

// ---- the guided search (include/svo.h, "Guided search") ----
extern "C" int svo_desc_index_set_guided_sort(svo_desc_index* x, int on) {
    if (!x) return fail(SVO_ERR_ARG, "null index");
    x->guided_sort = on != 0;
    return SVO_OK;
}

// times: the projection kernel
extern "C" int svo_desc_index_project(svo_desc_index* x, const float K[9], const svo_reloc_guide* g, int row_lo, int row_hi, float* uv) {
    SearchGuide sg;
    int rc = guide_check(x, K, g, nullptr, &sg);
    if (rc != SVO_OK || (rc = row_range(x, row_lo, row_hi)) != SVO_OK) return rc;
    if (row_hi > row_lo && !uv) return fail(SVO_ERR_ARG, "svo_desc_index_project: null uv");
    MHIP(call_begin(x));
    if (row_hi == row_lo) return SVO_OK;
    SearchPlan plan;                                  // a guided search of no queries is the projection
    if ((rc = search_plan(x, 0, row_lo, row_hi, &sg, &plan)) != SVO_OK || (rc = search_enqueue(x, plan, 0, true)) != SVO_OK) return rc;
    MHIP(hipMemcpyAsync(uv, x->d_uv + row_lo, (size_t)(row_hi - row_lo) * sizeof(float2), hipMemcpyDeviceToHost, x->stream));
    MHIP(hipStreamSynchronize(x->stream));
    MHIP(span_read(x, x->last_ms));
    return SVO_OK;
}

extern "C" int svo_desc_index_match_guided(svo_desc_index* x, const float K[9], const svo_reloc_guide* g, int n, const uint8_t* query,
                                           const float* xy, int row_lo, int row_hi, svo_desc_match* out) {
    SearchGuide sg;
    int rc = guide_check(x, K, g, xy, &sg);
    if (rc != SVO_OK) return rc;
    if (n < 0 || (n > 0 && (!query || !xy || !out))) return fail(SVO_ERR_ARG, "svo_desc_index_match_guided: bad n / query / xy / out");
    if (n > SVO_RELOC_MAX_QUERIES) return fail(SVO_ERR_ARG, "svo_desc_index_match_guided: at most 4096 queries per call");
    return match_run(x, &sg, n, query, row_lo, row_hi, out);
}

// ---- the relocaliser (include/svo.h, "Relocalisation") ----
extern "C" void svo_reloc_params_default(svo_reloc_params* p) {
    if (!p) return;
    svo_config cfg; svo_config_default(&cfg);
    p->row_lo = 0; p->row_hi = -1; p->max_dist = 40; p->ratio_num = 7; p->ratio_den = 10; p->min_candidates = 6;
    p->ransac_iterations = cfg.ransac_iterations; p->reproj_error = cfg.ransac_reprojection_error; p->confidence = cfg.ransac_confidence;
}

// What a relocalising call asks for — K: the camera matrix of the guide's projection and of the PnP; guide: null for the unguided
// search — and where its results go, each null when not wanted.  res says "localize": without it the call is the selection alone.
struct RelocRequest { const float* K; const svo_reloc_guide* guide; int n; const uint8_t* query; const float* xy; const svo_reloc_params* p; };
struct RelocOutputs { int* n_candidates; int32_t* cand_query; int32_t* cand_row; float* cand_xy; float* cand_xyz; svo_reloc_result* res = nullptr; uint8_t* cand_inlier = nullptr; };

// ---- the pieces the single calls and the batch share
// the refusals over a call's parameters, behind those of its rows
static int reloc_params_check(const svo_reloc_params* p) {
    if (p->max_dist < 0 || p->max_dist > 256) return fail(SVO_ERR_ARG, "relocalisation: max_dist must be 0 .. 256");
    if (p->ratio_num < 1 || p->ratio_num > SVO_RELOC_MAX_RATIO || p->ratio_den < 1 || p->ratio_den > SVO_RELOC_MAX_RATIO)
        return fail(SVO_ERR_ARG, "relocalisation: ratio_num and ratio_den must be 1 .. 1 << 20");
    if (p->min_candidates < 6) return fail(SVO_ERR_ARG, "relocalisation: min_candidates must be >= 6 (4 and 5 points take svo_camera_to_world's direct routes)");
    return SVO_OK;
}

// a camera's state row going up, as svo_camera_to_world sets it; the selection kernel fills in the count
static void reloc_state_row(SeqState& hs, const float* K, const svo_reloc_result& guess) {
    memset(&hs, 0, sizeof(hs));
    hs.active = 1; hs.fail_reason = 0; hs.feat_buf = 0;
    memcpy(hs.K, K, sizeof(float) * 9); memcpy(hs.R, guess.R, sizeof(double) * 9); memcpy(hs.t, guess.t, sizeof(double) * 3);
}

// a camera's result from its state row as k_pnp_final left it, its nc candidates and their inlier flags
static void reloc_read(const SeqState& hs, int nc, int min_candidates, const uint8_t* inlier, svo_reloc_result* res, uint8_t* cand_inlier) {
    res->success = 0; res->n_candidates = nc; res->n_inliers = 0; res->iters_run = 0;
    memset(res->T, 0, sizeof(res->T));
    if (cand_inlier) memset(cand_inlier, 0, (size_t)nc);
    if (nc < min_candidates) return;                  // rule 4: every PnP kernel found the row not live
    res->iters_run = hs.pnp_iters;
    if (hs.pnp_best < 0) return;                      // no pose: R, t untouched, as svo_camera_to_world leaves them
    memcpy(res->R, hs.R, sizeof(double) * 9); memcpy(res->t, hs.t, sizeof(double) * 3); memcpy(res->T, hs.last_T, sizeof(double) * 16);
    res->success = 1; res->n_inliers = hs.n_inliers;
    if (cand_inlier) memcpy(cand_inlier, inlier, (size_t)nc);
}

// k_reloc_select over the n results in d_out, for the single calls and for places: the candidates' pixels, points and count into the
// stage context d, their queries and rows into d_reloc
static void select_enqueue(svo_desc_index* x, const DevBuffers* d, int n, RelocRule rule, int min_candidates) {
    RelocArgs a;
    a.match = x->d_out; a.points = x->d_points; a.xy = x->d_qxy; a.n = n;
    a.rule = rule; a.min_candidates = min_candidates;
    a.out_xy = d->tl1; a.out_xyz = d->world; a.st = d->st;
    a.cand_query = x->d_reloc->cand_query; a.cand_row = x->d_reloc->cand_row; a.n_cand = &x->d_reloc->n_cand;
    launch_reloc_select(a, x->stream);
}
// the candidate lists on their way down into h_reloc->out: the count and the queries in one copy, the rows in another ...
static int cands_down(svo_desc_index* x, int n) {
    MHIP(hipMemcpyAsync(&x->h_reloc->out, x->d_reloc, offsetof(RelocDevOut, cand_query) + (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, x->stream));
    if (n > 0) MHIP(hipMemcpyAsync(x->h_reloc->out.cand_row, x->d_reloc->cand_row, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, x->stream));
    return SVO_OK;
}
// ... and, after the wait, out to the caller -> their number
static int cands_read(const svo_desc_index* x, int32_t* cand_query, int32_t* cand_row) {
    const RelocDevOut& o = x->h_reloc->out;
    if (cand_query) memcpy(cand_query, o.cand_query, (size_t)o.n_cand * sizeof(int32_t));
    if (cand_row) memcpy(cand_row, o.cand_row, (size_t)o.n_cand * sizeof(int32_t));
    return o.n_cand;
}

// What select and localize share, with and without a guide.  Everything is enqueued on the index's stream — the uploads, the search,
// k_reloc_select, the PnP kernels for localize, the copies back — and the host waits once.
// times: a guided call its projection and guided search kernels, an unguided one the selection kernel
static int reloc_run(svo_desc_index* x, const RelocRequest& q, const RelocOutputs& o) {
    const int n = q.n;
    const svo_reloc_params* p = q.p; svo_reloc_result* res = o.res;
    if (!x || !p || n < 0 || (n > 0 && !q.query)) return fail(SVO_ERR_ARG, "relocalisation: bad index / params / n / query");
    if (!x->d_points) return no_points("relocalisation");
    if (n > SVO_RELOC_MAX_QUERIES) return fail(SVO_ERR_ARG, "relocalisation: at most 4096 queries per call");
    if (n > 0 && !q.xy && (res || o.cand_xy || q.guide)) return fail(SVO_ERR_ARG, "relocalisation: null xy");
    SearchGuide sg;
    int rc, row_lo = p->row_lo, row_hi = p->row_hi;
    if (q.guide && (rc = guide_check(x, q.K, q.guide, q.xy, &sg)) != SVO_OK) return rc;
    if ((rc = row_range(x, row_lo, row_hi)) != SVO_OK) return rc;
    if ((rc = reloc_params_check(p)) != SVO_OK) return rc;
    const bool times_search = q.guide != nullptr;
    MHIP(call_begin(x));
    const DevBuffers* d = nullptr;
    SearchPlan plan;
    if ((rc = svo_reloc_stage_ctx(x->device, n > 64 ? n : 64, p->ransac_iterations, p->reproj_error, p->confidence, &d)) != SVO_OK ||
        (rc = search_plan(x, n, row_lo, row_hi, q.guide ? &sg : nullptr, &plan)) != SVO_OK || (rc = stage_queries(x, n, q.query, true, q.xy)) != SVO_OK) return rc;
    RelocHost* h = x->h_reloc;
    if (res) {
        reloc_state_row(h->up, q.K, *res);
        MHIP(hipMemcpyAsync(d->st, &h->up, sizeof(SeqState), hipMemcpyHostToDevice, x->stream));
    }
    if ((rc = search_enqueue(x, plan, n, times_search)) != SVO_OK) return rc;
    MHIP(span_mark(x, !times_search, 0));
    select_enqueue(x, d, n, RelocRule{p->max_dist, p->ratio_num, p->ratio_den}, p->min_candidates);
    MHIP(span_mark(x, !times_search, 1));
    if (res) { launch_pnp_subsets(*d, x->stream); launch_pnp(*d, x->stream); }
    MHIP(hipGetLastError());
    if ((rc = cands_down(x, n)) != SVO_OK) return rc;
    if (n > 0) {
        if (o.cand_xy) MHIP(hipMemcpyAsync(h->cand_xy, d->tl1, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost, x->stream));
        if (o.cand_xyz) MHIP(hipMemcpyAsync(h->cand_xyz, d->world, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, x->stream));
        if (res) MHIP(hipMemcpyAsync(h->inlier, d->inlier, (size_t)n, hipMemcpyDeviceToHost, x->stream));
    }
    if (res) MHIP(hipMemcpyAsync(&h->down, d->st, sizeof(SeqState), hipMemcpyDeviceToHost, x->stream));
    MHIP(hipStreamSynchronize(x->stream));            // the call's one wait
    MHIP(span_read(x, x->last_ms));
    const int nc = cands_read(x, o.cand_query, o.cand_row);
    if (o.n_candidates) *o.n_candidates = nc;
    if (o.cand_xy) memcpy(o.cand_xy, h->cand_xy, (size_t)nc * sizeof(float2));
    if (o.cand_xyz) memcpy(o.cand_xyz, h->cand_xyz, (size_t)nc * 3 * sizeof(float));
    if (res) reloc_read(h->down, nc, p->min_candidates, h->inlier, res, o.cand_inlier);
    return SVO_OK;
}

extern "C" int svo_desc_index_select(svo_desc_index* x, int n, const uint8_t* query, const float* xy, const svo_reloc_params* p,
                                     int* n_candidates, int32_t* cand_query, int32_t* cand_row, float* cand_xy, float* cand_xyz) {
    return reloc_run(x, RelocRequest{nullptr, nullptr, n, query, xy, p}, RelocOutputs{n_candidates, cand_query, cand_row, cand_xy, cand_xyz});
}

extern "C" int svo_desc_index_localize(svo_desc_index* x, const float K[9], int n, const uint8_t* query, const float* xy,
                                       const svo_reloc_params* p, svo_reloc_result* res, int32_t* cand_query, int32_t* cand_row,
                                       uint8_t* cand_inlier) {
    if (!K || !res) return fail(SVO_ERR_ARG, "svo_desc_index_localize: null K / result");
    return reloc_run(x, RelocRequest{K, nullptr, n, query, xy, p}, RelocOutputs{nullptr, cand_query, cand_row, nullptr, nullptr, res, cand_inlier});
}

extern "C" int svo_desc_index_select_guided(svo_desc_index* x, const float K[9], const svo_reloc_guide* g, int n, const uint8_t* query,
                                            const float* xy, const svo_reloc_params* p, int* n_candidates, int32_t* cand_query,
                                            int32_t* cand_row, float* cand_xy, float* cand_xyz) {
    if (!K || !g) return fail(SVO_ERR_ARG, "svo_desc_index_select_guided: null K / guide");
    return reloc_run(x, RelocRequest{K, g, n, query, xy, p}, RelocOutputs{n_candidates, cand_query, cand_row, cand_xy, cand_xyz});
}

extern "C" int svo_desc_index_localize_guided(svo_desc_index* x, const float K[9], const svo_reloc_guide* g, int n, const uint8_t* query,
                                              const float* xy, const svo_reloc_params* p, svo_reloc_result* res, int32_t* cand_query,
                                              int32_t* cand_row, uint8_t* cand_inlier) {
    if (!K || !g || !res) return fail(SVO_ERR_ARG, "svo_desc_index_localize_guided: null K / guide / result");
    return reloc_run(x, RelocRequest{K, g, n, query, xy, p}, RelocOutputs{nullptr, cand_query, cand_row, nullptr, nullptr, res, cand_inlier});
}

// ---- batched relocalisation (include/svo.h, "Batched relocalisation"; the kernels are in svo_kernels_reloc_batch.hip, the plan and
// the staging's layout in svo_reloc_batch.hpp) ----
#define BATCH_FIRST_CAMS 16                           // the staging's first room: cameras, queries
#define BATCH_FIRST_QUERIES 4096

// Room for a call of `cams` cameras and `queries` queries in the batch's staging: a device block, a pinned block and the pinned state
// rows.  Either capacity at least doubles when it is outgrown (rb_grow); the outgrown blocks go with the index, like every block.
static int batch_room(svo_desc_index* x, size_t cams, size_t queries) {
    if (x->d_batch && cams <= x->batch_cams && queries <= x->batch_queries) return SVO_OK;
    const size_t nc = rb_grow(x->batch_cams, cams, BATCH_FIRST_CAMS), nq = rb_grow(x->batch_queries, queries, BATCH_FIRST_QUERIES);
    const RbLayout l = rb_layout(nc, nq);
    uint8_t *d = nullptr, *h = nullptr;               // all three, then the switch: a failure leaves the staging as it was
    SeqState* hs = nullptr;
    ROOM(room(x, d, l.total, false));
    ROOM(room(x, h, l.down_end, true));
    ROOM(room(x, hs, 2 * nc * sizeof(SeqState), true));
    x->d_batch = d; x->h_batch = h; x->h_batch_st = hs; x->batch_cams = nc; x->batch_queries = nq;
    x->batch_total = -1;                              // the order of the last call stayed in the old block
    return SVO_OK;
}

// the refusal of a batch's offsets under the call's name: `begin` names the offsets' argument, `what` what they count
static int batch_offsets_fail(RbOffsets e, const char* call, const char* begin, const char* what) {
    char b[192];
    switch (e) {
    case RB_OFFSETS_COUNT: snprintf(b, sizeof(b), "%s: n_cameras must be 0 .. 1024", call); break;
    case RB_OFFSETS_NULL: snprintf(b, sizeof(b), "%s: null %s", call, begin); break;
    case RB_OFFSETS_FIRST: snprintf(b, sizeof(b), "%s: %s[0] must be 0", call, begin); break;
    case RB_OFFSETS_ORDER: snprintf(b, sizeof(b), "%s: %s must not decrease", call, begin); break;
    case RB_OFFSETS_SLICE: snprintf(b, sizeof(b), "%s: at most 4096 %s per camera", call, what); break;
    default: snprintf(b, sizeof(b), "%s: at most 1 << 20 %s in all", call, what); break;
    }
    return fail(SVO_ERR_ARG, b);
}

// the partial states the largest group of a batch's search writes (rb_next_group)
static size_t batch_group_states(int n_cameras, const int32_t* begin, int n_chunks) {
    size_t states = 0;
    for (int cam = 0; cam < n_cameras;) {
        const RbGroup g = rb_next_group(n_cameras, begin, cam, n_chunks);
        states = rb_group_states(g, n_chunks) > states ? rb_group_states(g, n_chunks) : states;
        cam = g.cam1;
    }
    return states;
}

// Everything is decided first — the refusals of the single calls for every camera, and the offsets' own — then one upload, the order,
// the search group by group (rb_next_group), the selection, the PnP over n_cameras sequences, the inlier flags, the copies back, and
// the call's one wait.
// times: from the first kernel to the last
extern "C" int svo_desc_index_localize_batch(svo_desc_index* x, int n_cameras, const float* K, const svo_reloc_guide* guides,
                                             const int32_t* query_begin, const uint8_t* query, const float* xy, const svo_reloc_params* p,
                                             svo_reloc_result* results, int32_t* cand_query, int32_t* cand_row, uint8_t* cand_inlier) {
    if (!x || !p) return fail(SVO_ERR_ARG, "svo_desc_index_localize_batch: null index / params");
    if (const RbOffsets e = rb_check_offsets(n_cameras, query_begin); e != RB_OFFSETS_OK)
        return batch_offsets_fail(e, "svo_desc_index_localize_batch", "query_begin", "queries");
    if (n_cameras > 0 && (!K || !results)) return fail(SVO_ERR_ARG, "svo_desc_index_localize_batch: null K / results");
    const int total = n_cameras > 0 ? query_begin[n_cameras] : 0;
    if (total > 0 && (!query || !xy)) return fail(SVO_ERR_ARG, "svo_desc_index_localize_batch: null query / xy");
    if (!x->d_points) return no_points("relocalisation");
    std::vector<SearchGuide> sg((size_t)(guides ? n_cameras : 0));
    int rc, row_lo = p->row_lo, row_hi = p->row_hi;
    for (int b = 0; b < n_cameras && guides; b++)
        if ((rc = guide_check(x, K + 9 * b, guides + b, nullptr, &sg[(size_t)b])) != SVO_OK) return rc;
    if ((rc = row_range(x, row_lo, row_hi)) != SVO_OK) return rc;
    if ((rc = reloc_params_check(p)) != SVO_OK) return rc;
    MHIP(call_begin(x));
    if (n_cameras == 0) return SVO_OK;
    // ---- room: the plan's partial states, the staging, the stage context
    const int max_slice = rb_max_slice(n_cameras, query_begin);
    const RbRange r = rb_plan_range(row_lo, row_hi, x->chunk_rows, max_slice);
    const MatchRange mr{r.row_lo, r.row_hi, r.chunk_rows, r.chunk0, r.n_chunks};
    const size_t states = batch_group_states(n_cameras, query_begin, r.n_chunks);
    DevBuffers d;
    svo_context* old = nullptr;
    rc = svo_reloc_batch_ctx(x->device, n_cameras, max_slice > 64 ? max_slice : 64, p->ransac_iterations, p->reproj_error, p->confidence,
                             &x->batch_ctx, &old, &d);
    if (old) x->batch_ctx_outgrown.push_back(old);
    if (rc != SVO_OK || (states > 0 && (rc = part_states(x, states)) != SVO_OK) || (rc = batch_room(x, (size_t)n_cameras, (size_t)total)) != SVO_OK) return rc;
    // ---- the upload: one copy of the staging's first part, one of the state rows
    const RbLayout l = rb_layout((size_t)n_cameras, (size_t)total);             // cut for this call: it fits the blocks, and the copies carry no slack
    uint8_t *h = x->h_batch, *dv = x->d_batch;
    memcpy(h + l.query, query, (size_t)total * SVO_DESC_BYTES);
    memcpy(h + l.xy, xy, (size_t)total * sizeof(float2));
    memcpy(h + l.begin, query_begin, (size_t)(n_cameras + 1) * sizeof(int32_t));
    RelocBatchCam* h_cams = (RelocBatchCam*)(h + l.cams);
    SeqState *h_up = x->h_batch_st, *h_down = x->h_batch_st + x->batch_cams;
    for (int b = 0; b < n_cameras; b++) {
        h_cams[b] = guides ? RelocBatchCam{sg[(size_t)b].pose, sg[(size_t)b].radius, 0} : RelocBatchCam{};
        reloc_state_row(h_up[b], K + 9 * b, results[b]);
    }
    MHIP(hipMemcpyAsync(dv, h, l.up_end, hipMemcpyHostToDevice, x->stream));
    MHIP(hipMemcpyAsync(d.st, h_up, (size_t)n_cameras * sizeof(SeqState), hipMemcpyHostToDevice, x->stream));
    const uint32_t* d_query = (const uint32_t*)(dv + l.query);
    const float2* d_qxy = (const float2*)(dv + l.xy);
    const int32_t* d_begin = (const int32_t*)(dv + l.begin);
    const RelocBatchCam* d_cams = (const RelocBatchCam*)(dv + l.cams);
    int32_t *d_order = (int32_t*)(dv + l.order), *d_ncand = (int32_t*)(dv + l.n_cand);
    int32_t *d_cq = (int32_t*)(dv + l.cand_query), *d_cr = (int32_t*)(dv + l.cand_row);
    svo_desc_match* d_match = (svo_desc_match*)(dv + l.match);
    // ---- the kernels
    const bool ordered = guides && x->guided_sort && total > 0;
    MHIP(span_mark(x, true, 0));
    if (ordered) launch_reloc_batch_order(d_qxy, d_begin, d_cams, n_cameras, d_order, x->stream);
    for (int cam = 0; cam < n_cameras;) {             // a group's partial states are merged before the next group overwrites them
        const RbGroup g = rb_next_group(n_cameras, query_begin, cam, r.n_chunks);
        const int m = g.q1 - g.q0;
        if (guides) {
            const RelocBatchSearch a{(const uint32_t*)x->d_desc, x->d_ids, x->d_points, d_cams, d_begin, d_query, d_qxy, ordered ? d_order : nullptr,
                                     r, g.cam0, g.q0, x->d_part()};
            launch_desc_match_guided_batch(a, rb_guided_grid(g, r.n_chunks), x->stream);
        } else {
            launch_desc_match((const uint32_t*)x->d_desc, x->d_ids, d_query + (size_t)g.q0 * 8, m, mr, x->d_part(), x->stream);
        }
        launch_desc_match_merge(x->d_part(), x->d_ids, m, mr, d_match + g.q0, x->stream);
        cam = g.cam1;
    }
    const RelocBatchSelect sel{d_match, x->d_points, d_qxy, d_begin, RelocRule{p->max_dist, p->ratio_num, p->ratio_den}, p->min_candidates,
                               d.tl1, d.world, d.st, d.CAP, d_cq, d_cr, d_ncand};
    launch_reloc_select_batch(sel, n_cameras, x->stream);
    launch_pnp_subsets(d, x->stream);
    launch_pnp(d, x->stream);
    launch_reloc_batch_inliers(d.inlier, d.CAP, d_begin, d_ncand, n_cameras, max_slice, dv + l.inlier, x->stream);
    MHIP(hipGetLastError());
    MHIP(span_mark(x, true, 1));
    x->batch_total = total; x->batch_last_cams = n_cameras; x->batch_ordered = ordered;
    // ---- back: the counts, the lists and the flags in one copy, the state rows in another
    MHIP(hipMemcpyAsync(h + l.n_cand, dv + l.n_cand, l.down_end - l.n_cand, hipMemcpyDeviceToHost, x->stream));
    MHIP(hipMemcpyAsync(h_down, d.st, (size_t)n_cameras * sizeof(SeqState), hipMemcpyDeviceToHost, x->stream));
    MHIP(hipStreamSynchronize(x->stream));            // the call's one wait
    MHIP(span_read(x, x->last_ms));
    const int32_t* h_ncand = (const int32_t*)(h + l.n_cand);
    const int32_t *h_cq = (const int32_t*)(h + l.cand_query), *h_cr = (const int32_t*)(h + l.cand_row);
    for (int b = 0; b < n_cameras; b++) {
        const int q0 = query_begin[b], nc = h_ncand[b];
        if (cand_query) memcpy(cand_query + q0, h_cq + q0, (size_t)nc * sizeof(int32_t));
        if (cand_row) memcpy(cand_row + q0, h_cr + q0, (size_t)nc * sizeof(int32_t));
        reloc_read(h_down[b], nc, p->min_candidates, h + l.inlier + q0, results + b, cand_inlier ? cand_inlier + q0 : nullptr);
    }
    return SVO_OK;
}

// diagnostic: the lane order of the last batch call as global query numbers (the identity where k_reloc_batch_order did not run)
extern "C" int svo_desc_index_get_batch_order(const svo_desc_index* x, int cap, int32_t* order, int* n) {
    if (!x || !n || cap < 0 || (cap > 0 && !order)) return fail(SVO_ERR_ARG, "svo_desc_index_get_batch_order: null index / n / order");
    if (x->batch_total < 0) return fail(SVO_ERR_STATE, "svo_desc_index_get_batch_order: no batch call has been made (or the staging has grown since)");
    *n = x->batch_total;
    const int m = cap < x->batch_total ? cap : x->batch_total;
    if (m == 0) return SVO_OK;
    if (!x->batch_ordered) { for (int i = 0; i < m; i++) order[i] = i; return SVO_OK; }
    MHIP(hipSetDevice(x->device));
    const RbLayout l = rb_layout((size_t)x->batch_last_cams, (size_t)x->batch_total);
    MHIP(hipMemcpyAsync(order, x->d_batch + l.order, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, x->stream));
    MHIP(hipStreamSynchronize(x->stream));
    return SVO_OK;
}

// ---- map alignment (include/svo.h, "Map alignment"; the kernels are in svo_kernels_align.hip, the rules in svo_align.hpp) ----
extern "C" void svo_align_params_default(svo_align_params* p, float inlier_dist) {
    if (!p) return;
    svo_reloc_params r; svo_reloc_params_default(&r);
    p->src_lo = 0; p->src_hi = -1; p->dst_lo = 0; p->dst_hi = -1;
    p->max_dist = r.max_dist; p->ratio_num = r.ratio_num; p->ratio_den = r.ratio_den;
    p->min_pairs = 6; p->hypotheses = 256; p->refit_rounds = 4; p->inlier_dist = inlier_dist; p->reserved = 0;
}

extern "C" int svo_align_sample(uint32_t h, int32_t n_pairs, int32_t* out) {
    if (!out || n_pairs < 3) return fail(SVO_ERR_ARG, "svo_align_sample: null out / n_pairs < 3");
    int32_t pick[3];
    align_sample(h, n_pairs, pick);
    memcpy(out, pick, sizeof(pick));
    return SVO_OK;
}

static const char* align_refusal_text(AlignRefusal e) {
    switch (e) {
    case ALIGN_SRC_RANGE: return "map alignment: the source span must satisfy 0 <= src_lo <= src_hi <= size";
    case ALIGN_DST_RANGE: return "map alignment: the destination span must satisfy 0 <= dst_lo <= dst_hi <= size";
    case ALIGN_ROWS: return "map alignment: at most 4096 source rows per call";
    case ALIGN_OVERLAP: return "map alignment: the source and the destination span share a row";
    case ALIGN_MAX_DIST: return "map alignment: max_dist must be 0 .. 256";
    case ALIGN_RATIO: return "map alignment: ratio_num and ratio_den must be 1 .. 1 << 20";
    case ALIGN_MIN_PAIRS: return "map alignment: min_pairs must be 3 .. 4096";
    case ALIGN_HYPOTHESES: return "map alignment: hypotheses must be 1 .. 1024";
    case ALIGN_REFIT: return "map alignment: refit_rounds must be 0 .. 8";
    default: return "map alignment: inlier_dist must be finite and > 0";
    }
}

// the alignment's device block and its pinned twin, allocated at the first call that pairs
static int align_room(svo_desc_index* x) {
    const AlignLayout l = align_layout(ALIGN_MAX_ROWS, ALIGN_MAX_HYPOTHESES);
    ROOM(room(x, x->h_align, l.down_end, true));
    return room(x, x->d_align, l.total, false);
}

// ---- the pair stage that the alignment and the fusion share: k_align_pairs over the n results in d_out, the queries being rows
// src_lo .. of the index, into the alignment's block, cut here
struct PairStage { AlignLayout l; AlignOut* out; int32_t *src, *dst; uint8_t* inlier; float* pairs; };
static PairStage pairs_enqueue(svo_desc_index* x, int src_lo, int n, RelocRule rule) {
    const AlignLayout l = align_layout(ALIGN_MAX_ROWS, ALIGN_MAX_HYPOTHESES);
    uint8_t* dv = x->d_align;
    const PairStage s{l, (AlignOut*)(dv + l.out), (int32_t*)(dv + l.pair_src), (int32_t*)(dv + l.pair_dst), dv + l.pair_inlier, (float*)(dv + l.pairs)};
    launch_align_pairs(AlignPairsArgs{x->d_out, x->d_points, x->d_ids, src_lo, n, rule, s.src, s.dst, s.inlier, s.pairs, s.out}, x->stream);
    return s;
}
// the pairs out of the pinned twin, after the wait -> their number
static int pairs_read(const svo_desc_index* x, const AlignLayout& l, int* n_pairs, int32_t* pair_src, int32_t* pair_dst) {
    const uint8_t* h = x->h_align;
    const int np = ((const AlignOut*)(h + l.out))->n_pairs;
    if (n_pairs) *n_pairs = np;
    if (pair_src) memcpy(pair_src, h + l.pair_src, (size_t)np * sizeof(int32_t));
    if (pair_dst) memcpy(pair_dst, h + l.pair_dst, (size_t)np * sizeof(int32_t));
    return np;
}

// What match_rows (stage 1), pair_rows (2) and align (3) share.  q: the request, checked and with its spans resolved.  Everything is
// enqueued on the index's stream — the search with rows [src_lo, src_hi) of the index as its queries, the pair kernel, the two
// RANSAC kernels, one copy back — and the host waits once.
// times: from the first kernel to the last
static int align_run(svo_desc_index* x, const AlignRequest& q, int stage, svo_desc_match* rows, int* n_pairs, svo_align_result* res,
                     int32_t* pair_src, int32_t* pair_dst, uint8_t* pair_inlier) {
    const int n = q.src_hi - q.src_lo;
    int rc;
    MHIP(call_begin(x));
    SearchPlan plan;
    if ((stage > 1 && (rc = align_room(x)) != SVO_OK) || (rc = search_plan(x, n, q.dst_lo, q.dst_hi, nullptr, &plan)) != SVO_OK) return rc;
    if ((rc = search_enqueue(x, plan, n, true, x->d_desc + (size_t)q.src_lo * SVO_DESC_BYTES)) != SVO_OK) return rc;
    if (stage == 1) return rows_down(x, n, rows);
    const PairStage ps = pairs_enqueue(x, q.src_lo, n, RelocRule{q.max_dist, q.ratio_num, q.ratio_den});
    const AlignLayout& l = ps.l;
    uint8_t *dv = x->d_align, *h = x->h_align;
    if (stage == 3) {
        const AlignFitArgs fa{ps.pairs, q.hypotheses, q.min_pairs, q.refit_rounds, align_dist2(q.inlier_dist),
                              (int32_t*)(dv + l.counts), (AlignModel*)(dv + l.models), ps.inlier, ps.out};
        launch_align_score(fa, x->stream);
        launch_align_fit(fa, x->stream);
    }
    MHIP(hipGetLastError());
    MHIP(span_mark(x, true, 1));                      // the span's end moves from the search's last kernel to the call's
    MHIP(hipMemcpyAsync(h, dv, l.down_end, hipMemcpyDeviceToHost, x->stream));
    MHIP(hipStreamSynchronize(x->stream));            // the call's one wait
    MHIP(span_read(x, x->last_ms));
    const AlignOut& o = *(const AlignOut*)(h + l.out);
    const int np = pairs_read(x, l, n_pairs, pair_src, pair_dst);
    if (pair_inlier) memcpy(pair_inlier, h + l.pair_inlier, (size_t)np);
    if (!res) return SVO_OK;
    memset(res, 0, sizeof(*res));
    res->success = o.success; res->n_pairs = np; res->n_inliers = o.n_inliers; res->best_hypothesis = o.best_hypothesis;
    res->best_count = o.best_count; res->refit_rounds_run = o.refit_rounds_run;
    if (!o.success) return SVO_OK;
    memcpy(res->R, o.R, sizeof(o.R)); memcpy(res->t, o.t, sizeof(o.t)); res->rms = o.rms;
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) res->T[4 * r + c] = o.R[3 * r + c]; res->T[4 * r + 3] = o.t[r]; }
    res->T[15] = 1.;
    return SVO_OK;
}

static AlignRequest align_request(const svo_align_params* p) {
    return AlignRequest{p->src_lo, p->src_hi, p->dst_lo, p->dst_hi, p->max_dist, p->ratio_num, p->ratio_den, p->min_pairs, p->hypotheses,
                        p->refit_rounds, p->inlier_dist};
}

extern "C" int svo_desc_index_match_rows(svo_desc_index* x, int src_lo, int src_hi, int dst_lo, int dst_hi, svo_desc_match* out) {
    if (!x) return fail(SVO_ERR_ARG, "null index");
    AlignRequest q{src_lo, src_hi, dst_lo, dst_hi, 0, 1, 1, 3, 1, 0, 1.f};
    if (const AlignRefusal e = align_check_spans(q, x->size); e != ALIGN_OK) return fail(SVO_ERR_ARG, align_refusal_text(e));
    if (q.src_hi > q.src_lo && !out) return fail(SVO_ERR_ARG, "svo_desc_index_match_rows: null out");
    return align_run(x, q, 1, out, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int svo_desc_index_pair_rows(svo_desc_index* x, const svo_align_params* p, int* n_pairs, int32_t* pair_src, int32_t* pair_dst) {
    if (!x || !p) return fail(SVO_ERR_ARG, "svo_desc_index_pair_rows: null index / params");
    if (!x->d_points) return no_points("map alignment");
    AlignRequest q = align_request(p);
    if (const AlignRefusal e = align_check(q, x->size); e != ALIGN_OK) return fail(SVO_ERR_ARG, align_refusal_text(e));
    return align_run(x, q, 2, nullptr, n_pairs, nullptr, pair_src, pair_dst, nullptr);
}

extern "C" int svo_desc_index_align(svo_desc_index* x, const svo_align_params* p, svo_align_result* res, int32_t* pair_src, int32_t* pair_dst,
                                    uint8_t* pair_inlier) {
    if (!x || !p || !res) return fail(SVO_ERR_ARG, "svo_desc_index_align: null index / params / result");
    if (!x->d_points) return no_points("map alignment");
    AlignRequest q = align_request(p);
    if (const AlignRefusal e = align_check(q, x->size); e != ALIGN_OK) return fail(SVO_ERR_ARG, align_refusal_text(e));
    return align_run(x, q, 3, nullptr, nullptr, res, pair_src, pair_dst, pair_inlier);
}

// ---- index maintenance (include/svo.h, "Index maintenance") ----
#define RETIRE_SCRATCH_FIRST ((size_t)1 << 16)        // the scratch's first size in bytes; it doubles from there
#define RETIRE_STAGE_BYTES ((size_t)MATCH_STAGE_ROWS * (SVO_DESC_BYTES + sizeof(uint64_t)))   // h_stage, which carries the ids up and kept_before down

static int retire_ctl_room(svo_desc_index* x) {
    ROOM(room(x, x->h_retire, sizeof(RetireDown), true));
    return room(x, x->d_retire_ctl, sizeof(RetireCtl), false);
}

// Room for `need` bytes of maintenance scratch (grow): 64 KiB times a power of two, the smallest that holds the largest call so far.
static int retire_scratch(svo_desc_index* x, size_t need) { return grow(x, x->retire, need, RETIRE_SCRATCH_FIRST, 0, false); }

extern "C" int svo_desc_index_set_retire_slab_rows(svo_desc_index* x, int rows) {
    if (!x) return fail(SVO_ERR_ARG, "null index");
    if (rows < 0 || rows > RETIRE_MAX_ROWS) return fail(SVO_ERR_ARG, "svo_desc_index_set_retire_slab_rows: rows must be 0 (default) .. 1 << 24");
    x->retire_slab = rows ? rows : RETIRE_DEFAULT_SLAB;
    return SVO_OK;
}
extern "C" int svo_desc_index_get_retire_slab_rows(const svo_desc_index* x) { return x ? x->retire_slab : fail(SVO_ERR_ARG, "null index"); }

extern "C" int svo_desc_index_get_retire_stats(const svo_desc_index* x, svo_desc_retire_stats* st) {
    if (!x || !st) return fail(SVO_ERR_ARG, "null index / stats");
    st->last_kernels_ms = x->retire_ms;
    st->scratch_allocations = x->retire.allocs;
    st->scratch_bytes = (uint64_t)x->retire.cap;
    st->scratch_bytes_outgrown = (uint64_t)x->retire.outgrown;
    return SVO_OK;
}

// The one list upload: n 64-bit values onto the device through the pinned staging, piece by piece, with a wait behind each piece,
// which frees the staging again — but for the last one's where the caller puts up one piece and waits once itself (wait_last false).
static int upload_list(svo_desc_index* x, const uint64_t* src, size_t n, uint64_t* d_dst, bool wait_last = true) {
    const size_t piece = RETIRE_STAGE_BYTES / sizeof(uint64_t);
    for (size_t i0 = 0; i0 < n; i0 += piece) {
        const size_t m = n - i0 < piece ? n - i0 : piece;
        memcpy(x->h_stage, src + i0, m * sizeof(uint64_t));
        MHIP(hipMemcpyAsync(d_dst + i0, x->h_stage, m * sizeof(uint64_t), hipMemcpyHostToDevice, x->stream));
        if (wait_last || i0 + m < n) MHIP(hipStreamSynchronize(x->stream));
    }
    return SVO_OK;
}

// kept_before[row_lo + i] = row_lo + rank[i] for the scope's rows, piece by piece through the pinned staging
static int retire_download_ranks(svo_desc_index* x, const int32_t* d_rank, int row_lo, int m, int32_t* kept_before) {
    const int piece = (int)(RETIRE_STAGE_BYTES / sizeof(int32_t));
    const int32_t* h = (const int32_t*)x->h_stage;
    for (int i0 = 0; i0 < m; i0 += piece) {
        const int n = m - i0 < piece ? m - i0 : piece;
        MHIP(hipMemcpyAsync(x->h_stage, d_rank + i0, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, x->stream));
        MHIP(hipStreamSynchronize(x->stream));
        for (int i = 0; i < n; i++) kept_before[row_lo + i0 + i] = row_lo + h[i];
    }
    return SVO_OK;
}

// The move of a call that keeps `kept` of its scope's m rows, kept < m: the scope's slabs, then the rows behind it, which all stay and
// move down; the call's second wait.
static int retire_move_rows(svo_desc_index* x, const RetireRows& rows, int row_lo, int row_hi, int kept, const uint8_t* keep, const int32_t* rank,
                            void* bounce, int slab) {
    const int n0 = x->size, m = row_hi - row_lo;
    MHIP(span_mark(x, true, 0));
    for (int a = 0; a < m; a += slab)
        launch_retire_slab(rows, row_lo + a, m - a < slab ? m - a : slab, keep + a, rank + a, row_lo, bounce, slab, x->stream);
    for (int a = row_hi; a < n0; a += slab)
        launch_retire_slab(rows, a, n0 - a < slab ? n0 - a : slab, nullptr, nullptr, row_lo + kept + (a - row_hi), bounce, slab, x->stream);
    MHIP(hipGetLastError());
    MHIP(span_mark(x, true, 1));
    MHIP(hipStreamSynchronize(x->stream));
    MHIP(span_read(x, x->retire_ms));
    return SVO_OK;
}

// kept_before outside the scope, and inside it where the ranks did not come down because every row of the scope stayed
static void retire_fill_map(int32_t* kept_before, int row_lo, int row_hi, int n0, int kept, bool ranks_down) {
    for (int r = 0; r <= row_lo; r++) kept_before[r] = r;
    if (!ranks_down) for (int r = row_lo; r < row_hi; r++) kept_before[r] = r;
    for (int r = row_hi; r <= n0; r++) kept_before[r] = r - (row_hi - row_lo - kept);
}

// The end that retire and consolidate share, from where the kernels that flag and rank the scope's rows are on the stream to where
// size has moved.  keep, rank: the scope's flags and ranks in the scratch (null: no kernel ran, every row stays); ctl_bytes: how much
// of the control block the caller reads.  The control block and the count of kept rows come down and the first wait ends the part
// that changes nothing: with the table's flag up the call ends there, under `overflow`.  Then the ranks down where the caller wants
// the map, the move of the rows and its wait (retire_move_rows), the rest of the map, and size.  -> *kept of the scope's rows.
static int retire_finish(svo_desc_index* x, const RetireRows& rows, int row_lo, int row_hi, const uint8_t* keep, const int32_t* rank, void* bounce,
                         size_t ctl_bytes, const char* overflow, int32_t* kept_before, int* kept) {
    const int n0 = x->size, m = row_hi - row_lo, slab = n0 - row_lo < x->retire_slab ? n0 - row_lo : x->retire_slab;
    int rc;
    bool ranks_down = false;
    *kept = m;
    if (keep) {
        MHIP(hipMemcpyAsync(&x->h_retire->ctl, x->d_retire_ctl, ctl_bytes, hipMemcpyDeviceToHost, x->stream));
        MHIP(hipMemcpyAsync(&x->h_retire->kept, rank + m, sizeof(int32_t), hipMemcpyDeviceToHost, x->stream));
        MHIP(hipStreamSynchronize(x->stream));        // nothing has moved yet: a failure up to here changes nothing
        MHIP(span_read(x, x->retire_ms));
        if (x->h_retire->ctl.table_full) return fail(SVO_ERR_INTERNAL, overflow);
        *kept = x->h_retire->kept;
        if (kept_before && *kept < m) {
            if ((rc = retire_download_ranks(x, rank, row_lo, m, kept_before)) != SVO_OK) return rc;
            ranks_down = true;
        }
        if (*kept < m && (rc = retire_move_rows(x, rows, row_lo, row_hi, *kept, keep, rank, bounce, slab)) != SVO_OK) return rc;
    }
    if (kept_before) retire_fill_map(kept_before, row_lo, row_hi, n0, *kept, ranks_down);
    x->size = n0 - (m - *kept);
    return SVO_OK;
}
static_assert(offsetof(RetireCtl, table_full) == 0 && offsetof(ConsCtl, table_full) == 0, "retire_finish reads the flag where both control blocks keep it");

extern "C" int svo_desc_index_retire(svo_desc_index* x, const svo_retire_rule* rule, int32_t* kept_before, int* n_kept) {
    if (!x || !rule) return fail(SVO_ERR_ARG, "svo_desc_index_retire: null index / rule");
    const uint32_t flags = rule->flags;
    if (flags & ~RETIRE_ALL_FLAGS) return fail(SVO_ERR_ARG, "svo_desc_index_retire: unknown flag bits");
    int row_lo = rule->row_lo, row_hi = rule->row_hi;
    int rc = row_range(x, row_lo, row_hi);
    if (rc != SVO_OK) return rc;
    if (rule->n_ids < 0 || rule->n_ids > RETIRE_MAX_IDS) return fail(SVO_ERR_ARG, "svo_desc_index_retire: n_ids must be 0 .. 1 << 24");
    if ((flags & RETIRE_BY_IDS) && rule->n_ids > 0 && !rule->ids) return fail(SVO_ERR_ARG, "svo_desc_index_retire: null ids");
    if ((flags & RETIRE_BY_TAG) && !x->d_points) return fail(SVO_ERR_STATE, "svo_desc_index_retire: BY_TAG on an index without points (svo_desc_index_enable_points)");
    x->retire_ms = 0.f;
    MHIP(hipSetDevice(x->device));
    const int n0 = x->size, m = row_hi - row_lo;
    const RetireRows rows{(uint4*)x->d_desc, x->d_ids, (uint4*)x->d_points};
    const uint8_t* keep = nullptr;                    // stays null where no kernel runs
    int32_t* rank = nullptr;
    void* bounce = nullptr;
    if (flags != 0 && m > 0) {
        std::vector<uint64_t> sorted;
        if (flags & RETIRE_BY_IDS) {
            sorted.assign(rule->ids, rule->ids + rule->n_ids);
            std::sort(sorted.begin(), sorted.end());
            sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
        }
        const RetireLayout l = retire_layout(m, n0 - row_lo, (int32_t)sorted.size(), x->retire_slab, flags);
        if ((rc = retire_ctl_room(x)) != SVO_OK || (rc = retire_scratch(x, l.total)) != SVO_OK) return rc;
        uint8_t* d_keep = x->retire.p + l.keep;
        rank = (int32_t*)(x->retire.p + l.rank);
        int32_t* counts = (int32_t*)(x->retire.p + l.counts);
        int32_t* table = (int32_t*)(x->retire.p + l.table);
        uint64_t* d_sorted = (uint64_t*)(x->retire.p + l.ids);
        keep = d_keep; bounce = x->retire.p + l.bounce;
        if ((rc = upload_list(x, sorted.data(), sorted.size(), d_sorted)) != SVO_OK) return rc;
        MHIP(hipMemsetAsync(&x->d_retire_ctl->table_full, 0, sizeof(int32_t), x->stream));
        const uint32_t slots = retire_table_slots(m);
        if (flags & RETIRE_LATEST_PER_ID) MHIP(hipMemsetAsync(table, 0xFF, (size_t)slots * sizeof(int32_t), x->stream));   // RETIRE_EMPTY
        MHIP(span_mark(x, true, 0));
        launch_retire_flags(rows, row_lo, m, flags, rule->tag_lo, rule->tag_hi, d_sorted, (int32_t)sorted.size(), d_keep, x->stream);
        if (flags & RETIRE_LATEST_PER_ID) launch_retire_latest(rows, row_lo, m, d_keep, table, slots, x->d_retire_ctl, x->stream);
        launch_retire_ranks(d_keep, m, counts, rank, x->stream);
        MHIP(hipGetLastError());
        MHIP(span_mark(x, true, 1));
    }
    int kept = m;                                     // of the scope's rows
    if ((rc = retire_finish(x, rows, row_lo, row_hi, keep, rank, bounce, sizeof(int32_t),
                            "svo_desc_index_retire: the latest-per-id table overflowed (nothing was changed)", kept_before, &kept)) != SVO_OK) return rc;
    if (n_kept) *n_kept = x->size;
    return SVO_OK;
}

extern "C" int svo_desc_index_transform_points(svo_desc_index* x, const double T[16], int row_lo, int row_hi, int32_t tag_lo, int32_t tag_hi,
                                               int* n_moved, int* n_skipped) {
    if (!x || !T) return fail(SVO_ERR_ARG, "svo_desc_index_transform_points: null index / T");
    if (!x->d_points) return no_points("svo_desc_index_transform_points");
    for (int i = 0; i < 16; i++) if (!isfinite(T[i])) return fail(SVO_ERR_ARG, "svo_desc_index_transform_points: T has a non-finite entry");
    int rc = row_range(x, row_lo, row_hi);
    if (rc != SVO_OK) return rc;
    x->retire_ms = 0.f;
    MHIP(hipSetDevice(x->device));
    int moved = 0, skipped = 0;
    if (row_hi > row_lo) {
        if ((rc = retire_ctl_room(x)) != SVO_OK) return rc;
        RetireT t;
        memcpy(t.m, T, sizeof(t.m));
        MHIP(hipMemsetAsync(x->d_retire_ctl, 0, sizeof(RetireCtl), x->stream));
        MHIP(span_mark(x, true, 0));
        launch_transform_points((uint4*)x->d_points, t, row_lo, row_hi, tag_lo, tag_hi, x->d_retire_ctl, x->stream);
        MHIP(hipGetLastError());
        MHIP(span_mark(x, true, 1));
        MHIP(hipMemcpyAsync(&x->h_retire->ctl, x->d_retire_ctl, sizeof(RetireCtl), hipMemcpyDeviceToHost, x->stream));
        MHIP(hipStreamSynchronize(x->stream));
        MHIP(span_read(x, x->retire_ms));
        for (const RetireCounts& c : x->h_retire->ctl.counts) { moved += c.n_moved; skipped += c.n_skipped; }
    }
    if (n_moved) *n_moved = moved;
    if (n_skipped) *n_skipped = skipped;
    return SVO_OK;
}

// ---- landmark fusion (include/svo.h, "Landmark fusion"; the kernels are in svo_kernels_fuse.hip, the rules in svo_fuse.hpp) ----
extern "C" void svo_fuse_params_default(svo_fuse_params* p, float radius) {
    if (!p) return;
    svo_reloc_params r; svo_reloc_params_default(&r);
    p->src_lo = 0; p->src_hi = -1; p->dst_lo = 0; p->dst_hi = -1; p->relabel_lo = 0; p->relabel_hi = -1;
    p->max_dist = r.max_dist; p->ratio_num = r.ratio_num; p->ratio_den = r.ratio_den;
    p->radius = radius; p->reserved = 0;
}

static const char* fuse_refusal_text(FuseRefusal e) {
    switch (e) {
    case FUSE_SRC_RANGE: return "landmark fusion: the source span must satisfy 0 <= src_lo <= src_hi <= size";
    case FUSE_DST_RANGE: return "landmark fusion: the destination span must satisfy 0 <= dst_lo <= dst_hi <= size";
    case FUSE_RELABEL_RANGE: return "landmark fusion: the relabel span must satisfy 0 <= relabel_lo <= relabel_hi <= size";
    case FUSE_ROWS: return "landmark fusion: at most 4096 source rows per call";
    case FUSE_OVERLAP: return "landmark fusion: the source and the destination span share a row";
    case FUSE_RADIUS: return "landmark fusion: the radius must be finite and >= 0";
    case FUSE_MAX_DIST: return "landmark fusion: max_dist must be 0 .. 256";
    default: return "landmark fusion: ratio_num and ratio_den must be 1 .. 1 << 20";
    }
}

static int fuse_ctl_room(svo_desc_index* x) { return room(x, x->h_fuse, sizeof(FuseCtl), true); }

// A call's lists and table in the maintenance scratch (room for fuse_layout(n) is there): the host lists of a relabel call up,
// where k_fuse_map would put a fuse call's, then the control block and the table cleared.
struct FuseDev { FuseCtl* ctl; uint64_t *from, *to; int32_t* table; };
static int fuse_begin(svo_desc_index* x, int n, const uint64_t* from_ids, const uint64_t* to_ids, FuseDev* f) {
    const FuseLayout fl = fuse_layout(n);
    uint8_t* d = x->retire.p;
    *f = FuseDev{(FuseCtl*)(d + fl.ctl), (uint64_t*)(d + fl.from), (uint64_t*)(d + fl.to), (int32_t*)(d + fl.table)};
    if (from_ids) { ROOM(upload_list(x, from_ids, (size_t)n, f->from)); ROOM(upload_list(x, to_ids, (size_t)n, f->to)); }
    MHIP(hipMemsetAsync(f->ctl, 0, sizeof(FuseCtl), x->stream));
    MHIP(hipMemsetAsync(f->table, 0xFF, (size_t)fuse_table_slots(n) * sizeof(int32_t), x->stream));      // FUSE_EMPTY
    return SVO_OK;
}

// the counts of a call as the host reads them after its wait; the table's flag cannot be raised at load <= 1/2
static int fuse_counts(const FuseCtl& c, int* n_rows) {
    if (c.table_full) return fail(SVO_ERR_INTERNAL, "landmark fusion: the table overflowed");
    int rows = 0;
    for (const FuseCount& k : c.counts) rows += k.n_rows_relabelled;
    *n_rows = rows;
    return SVO_OK;
}

// What match_near (stage 1), pair_near (2) and fuse (3) share.  q: the request, checked and with its spans resolved.  Everything is
// enqueued on the index's stream — the clears, the near search with rows [src_lo, src_hi) of the index as its queries (the unguided
// plan, marked near), the pair kernel, the map, the table and the sweep, the copies back — and the host waits once.
// times: from the first kernel to the last
static int fuse_run(svo_desc_index* x, const FuseRequest& q, int stage, svo_desc_match* rows, int* n_pairs, svo_fuse_result* res,
                    int32_t* pair_src, int32_t* pair_dst) {
    const int n = q.src_hi - q.src_lo;
    int rc;
    MHIP(call_begin(x));
    SearchPlan plan;
    if ((stage > 1 && (rc = align_room(x)) != SVO_OK) || (stage > 2 && ((rc = fuse_ctl_room(x)) != SVO_OK || (rc = retire_scratch(x, fuse_layout(n).total)) != SVO_OK)) ||
        (rc = search_plan(x, n, q.dst_lo, q.dst_hi, nullptr, &plan)) != SVO_OK) return rc;
    plan.near_lo = q.src_lo; plan.near_radius = q.radius;
    FuseDev f{};
    if ((stage > 2 && (rc = fuse_begin(x, n, nullptr, nullptr, &f)) != SVO_OK) || (rc = search_enqueue(x, plan, n, true)) != SVO_OK) return rc;
    if (stage == 1) return rows_down(x, n, rows);
    const PairStage ps = pairs_enqueue(x, q.src_lo, n, RelocRule{q.max_dist, q.ratio_num, q.ratio_den});
    if (stage == 3) {
        launch_fuse_map(&ps.out->n_pairs, n, ps.src, ps.dst, x->d_ids, f.from, f.to, f.ctl, x->stream);
        launch_fuse_relabel(f.from, f.to, &ps.out->n_pairs, n, f.table, fuse_table_slots(n), x->d_ids, q.relabel_lo, q.relabel_hi, f.ctl, x->stream);
    }
    MHIP(hipGetLastError());
    MHIP(span_mark(x, true, 1));                      // the span's end moves from the search's last kernel to the call's
    MHIP(hipMemcpyAsync(x->h_align, x->d_align, ps.l.pair_inlier, hipMemcpyDeviceToHost, x->stream));   // the result row and the two row lists
    if (stage == 3) MHIP(hipMemcpyAsync(x->h_fuse, f.ctl, sizeof(FuseCtl), hipMemcpyDeviceToHost, x->stream));
    MHIP(hipStreamSynchronize(x->stream));            // the call's one wait
    MHIP(span_read(x, x->last_ms));
    int n_rows = 0;
    if (stage == 3 && (rc = fuse_counts(*x->h_fuse, &n_rows)) != SVO_OK) return rc;
    const int np = pairs_read(x, ps.l, n_pairs, pair_src, pair_dst);
    if (res) { res->n_pairs = np; res->n_same = x->h_fuse->n_same; res->n_fused = x->h_fuse->n_fused; res->n_rows_relabelled = n_rows; }
    return SVO_OK;
}

static FuseRequest fuse_request(const svo_fuse_params* p) {
    return FuseRequest{p->src_lo, p->src_hi, p->dst_lo, p->dst_hi, p->relabel_lo, p->relabel_hi, p->max_dist, p->ratio_num, p->ratio_den, p->radius};
}

extern "C" int svo_desc_index_match_near(svo_desc_index* x, int src_lo, int src_hi, int dst_lo, int dst_hi, float radius, svo_desc_match* out) {
    if (!x) return fail(SVO_ERR_ARG, "null index");
    if (!x->d_points) return no_points("landmark fusion");
    FuseRequest q{src_lo, src_hi, dst_lo, dst_hi, 0, -1, 0, 1, 1, radius};
    if (const FuseRefusal e = fuse_check_search(q, x->size); e != FUSE_OK) return fail(SVO_ERR_ARG, fuse_refusal_text(e));
    if (q.src_hi > q.src_lo && !out) return fail(SVO_ERR_ARG, "svo_desc_index_match_near: null out");
    return fuse_run(x, q, 1, out, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int svo_desc_index_pair_near(svo_desc_index* x, const svo_fuse_params* p, int* n_pairs, int32_t* pair_src, int32_t* pair_dst) {
    if (!x || !p) return fail(SVO_ERR_ARG, "svo_desc_index_pair_near: null index / params");
    if (!x->d_points) return no_points("landmark fusion");
    FuseRequest q = fuse_request(p);
    if (const FuseRefusal e = fuse_check(q, x->size); e != FUSE_OK) return fail(SVO_ERR_ARG, fuse_refusal_text(e));
    return fuse_run(x, q, 2, nullptr, n_pairs, nullptr, pair_src, pair_dst);
}

extern "C" int svo_desc_index_fuse(svo_desc_index* x, const svo_fuse_params* p, svo_fuse_result* res, int32_t* pair_src, int32_t* pair_dst) {
    if (!x || !p) return fail(SVO_ERR_ARG, "svo_desc_index_fuse: null index / params");
    if (!x->d_points) return no_points("landmark fusion");
    FuseRequest q = fuse_request(p);
    if (const FuseRefusal e = fuse_check(q, x->size); e != FUSE_OK) return fail(SVO_ERR_ARG, fuse_refusal_text(e));
    return fuse_run(x, q, 3, nullptr, nullptr, res, pair_src, pair_dst);
}

// times: the insert and the sweep
extern "C" int svo_desc_index_relabel(svo_desc_index* x, int n, const uint64_t* from_ids, const uint64_t* to_ids, int row_lo, int row_hi,
                                      int* n_rows_relabelled) {
    if (!x) return fail(SVO_ERR_ARG, "null index");
    if (n < 0 || n > FUSE_MAX_LIST) return fail(SVO_ERR_ARG, "svo_desc_index_relabel: n must be 0 .. 1 << 20");
    if (n > 0 && (!from_ids || !to_ids)) return fail(SVO_ERR_ARG, "svo_desc_index_relabel: null from_ids / to_ids");
    int rc = row_range(x, row_lo, row_hi);
    if (rc != SVO_OK) return rc;
    MHIP(call_begin(x));
    int n_rows = 0;
    if (n > 0 && row_hi > row_lo) {
        FuseDev f;
        if ((rc = fuse_ctl_room(x)) != SVO_OK || (rc = retire_scratch(x, fuse_layout(n).total)) != SVO_OK || (rc = fuse_begin(x, n, from_ids, to_ids, &f)) != SVO_OK) return rc;
        MHIP(span_mark(x, true, 0));
        launch_fuse_relabel(f.from, f.to, nullptr, n, f.table, fuse_table_slots(n), x->d_ids, row_lo, row_hi, f.ctl, x->stream);
        MHIP(hipGetLastError());
        MHIP(span_mark(x, true, 1));
        MHIP(hipMemcpyAsync(x->h_fuse, f.ctl, sizeof(FuseCtl), hipMemcpyDeviceToHost, x->stream));
        MHIP(hipStreamSynchronize(x->stream));
        MHIP(span_read(x, x->last_ms));
        if ((rc = fuse_counts(*x->h_fuse, &n_rows)) != SVO_OK) return rc;
    }
    if (n_rows_relabelled) *n_rows_relabelled = n_rows;
    return SVO_OK;
}

// ---- place candidates (include/svo.h, "Place candidates"; the kernels are in svo_kernels_place.hip, the rules in svo_place.hpp) ----
extern "C" void svo_place_params_default(svo_place_params* p) {
    if (!p) return;
    svo_reloc_params r; svo_reloc_params_default(&r);
    p->row_lo = 0; p->row_hi = -1; p->max_dist = r.max_dist; p->ratio_num = r.ratio_num; p->ratio_den = r.ratio_den;
    p->tag_lo = 0; p->tag_hi = SVO_PLACE_MAX_TAGS - 1; p->min_votes = 1; p->separation = 0; p->max_places = 8;
}

extern "C" int svo_desc_index_set_place_combine(svo_desc_index* x, int on) {
    if (!x) return fail(SVO_ERR_ARG, "null index");
    x->place_combine = on != 0;
    return SVO_OK;
}

static const char* place_refusal_text(PlaceRefusal e) {
    switch (e) {
    case PLACE_ROW_RANGE: return "place candidates: the row range must satisfy 0 <= row_lo <= row_hi <= size";
    case PLACE_TAG_LO: return "place candidates: tag_lo must be >= 0";
    case PLACE_TAG_HI: return "place candidates: tag_hi must be >= tag_lo";
    case PLACE_TAG_SPAN: return "place candidates: at most 1 << 20 tags per call";
    case PLACE_MIN_VOTES: return "place candidates: min_votes must be >= 1";
    case PLACE_SEPARATION: return "place candidates: separation must be >= 0";
    case PLACE_MAX_PLACES_RANGE: return "place candidates: max_places must be 1 .. 64";
    case PLACE_MAX_DIST: return "place candidates: max_dist must be 0 .. 256";
    default: return "place candidates: ratio_num and ratio_den must be 1 .. 1 << 20";
    }
}

// where a call's results go, each null when not wanted
struct PlaceOutputs {
    int32_t *votes, *rows, *row_first, *row_end;      // tag_votes: one entry per bin
    svo_place_result* res; svo_place* places;         // the two places calls
    int32_t *cand_query, *cand_row;                   // places
};

// What tag_votes (pick false, query null), places_from_ids (pick, query null) and places (pick, with queries) share.  q: the request,
// checked and with its row range resolved.  Everything is enqueued on the index's stream — for places the queries up, the search and
// k_reloc_select; else the id list up — then the clearing of the bins, the sweep, the compaction and the pick, the copies back, and
// the host waits once.  times: from the clearing to the last place kernel
static int place_run(svo_desc_index* x, const PlaceRequest& q, bool pick, int n, const uint8_t* query, const uint64_t* ids, const PlaceOutputs& o) {
    int rc;
    MHIP(call_begin(x));
    const int n_bins = q.tag_hi - q.tag_lo + 1;
    const PlaceLayout l = place_layout(n, n_bins, pick);
    const size_t down = sizeof(PlaceCtl) + (pick ? 0 : sizeof(PlaceBin) * (size_t)n_bins);
    if ((rc = retire_scratch(x, l.total)) != SVO_OK || (rc = grow(x, x->place, down, RETIRE_SCRATCH_FIRST, 0, true)) != SVO_OK) return rc;
    PlaceCtl* ctl = (PlaceCtl*)(x->retire.p + l.ctl);
    uint64_t* d_list = (uint64_t*)(x->retire.p + l.ids);
    PlaceBin* bins = (PlaceBin*)(x->retire.p + l.bins);
    PlaceSweepArgs a{d_list, nullptr, nullptr, n, x->d_ids, x->d_points, q.row_lo, q.row_hi, q.tag_lo, q.tag_hi, bins, ctl};
    if (query) {                                      // rule 1: svo_desc_index_select's path, without pixels and without its copies back
        const DevBuffers* d = nullptr;
        SearchPlan plan;
        svo_reloc_params rp; svo_reloc_params_default(&rp);
        if ((rc = svo_reloc_stage_ctx(x->device, n > 64 ? n : 64, rp.ransac_iterations, rp.reproj_error, rp.confidence, &d)) != SVO_OK ||
            (rc = search_plan(x, n, q.row_lo, q.row_hi, nullptr, &plan)) != SVO_OK || (rc = stage_queries(x, n, query, true, nullptr)) != SVO_OK ||
            (rc = search_enqueue(x, plan, n, false)) != SVO_OK) return rc;
        select_enqueue(x, d, n, RelocRule{q.max_dist, q.ratio_num, q.ratio_den}, rp.min_candidates);
        a.list = nullptr; a.m_rows = x->d_reloc->cand_row; a.n_dev = &x->d_reloc->n_cand;
    } else if ((rc = upload_list(x, ids, (size_t)n, d_list, false)) != SVO_OK) {    // n <= 4096 ids: one piece of the pinned staging, no wait
        return rc;
    }
    MHIP(span_mark(x, true, 0));
    MHIP(hipMemsetAsync(ctl, 0, sizeof(PlaceCtl), x->stream));
    MHIP(hipMemsetAsync(bins, 0, sizeof(PlaceBin) * (size_t)n_bins, x->stream));
    launch_place_sweep(a, x->place_combine, x->stream);
    if (pick) launch_place_pick(bins, n_bins, q.tag_lo, q.min_votes, q.separation, q.max_places, (uint64_t*)(x->retire.p + l.keys), ctl, x->stream);
    MHIP(hipGetLastError());
    MHIP(span_mark(x, true, 1));
    uint8_t* h = x->place.p;
    MHIP(hipMemcpyAsync(h, ctl, sizeof(PlaceCtl), hipMemcpyDeviceToHost, x->stream));
    if (!pick) MHIP(hipMemcpyAsync(h + sizeof(PlaceCtl), bins, sizeof(PlaceBin) * (size_t)n_bins, hipMemcpyDeviceToHost, x->stream));
    if (query && (rc = cands_down(x, n)) != SVO_OK) return rc;            // a call with queries has n > 0
    MHIP(hipStreamSynchronize(x->stream));            // the call's one wait
    MHIP(span_read(x, x->last_ms));
    const PlaceCtl& c = *(const PlaceCtl*)h;
    if (c.set_full) return fail(SVO_ERR_INTERNAL, "place candidates: the set overflowed");
    if (!pick) {
        const PlaceBin* b = (const PlaceBin*)(h + sizeof(PlaceCtl));
        for (int i = 0; i < n_bins; i++) {
            if (o.votes) o.votes[i] = b[i].votes;
            if (o.rows) o.rows[i] = b[i].rows;
            if (o.row_first) o.row_first[i] = place_row_first(b[i]);
            if (o.row_end) o.row_end[i] = place_row_end(b[i]);
        }
        return SVO_OK;
    }
    if (o.res) { o.res->n_landmarks = c.n_landmarks; o.res->n_tags_voted = c.n_tags_voted; o.res->n_places = c.n_places; }
    if (o.places) memcpy(o.places, c.places, (size_t)c.n_places * sizeof(svo_place));
    if (query) cands_read(x, o.cand_query, o.cand_row);
    return SVO_OK;
}

static int place_ids_check(const svo_desc_index* x, int n_ids, const uint64_t* ids) {
    if (!x) return fail(SVO_ERR_ARG, "null index");
    if (!x->d_points) return no_points("place candidates");
    if (n_ids < 0 || n_ids > SVO_PLACE_MAX_IDS) return fail(SVO_ERR_ARG, "place candidates: n_ids must be 0 .. 4096");
    if (n_ids > 0 && !ids) return fail(SVO_ERR_ARG, "place candidates: null ids");
    return SVO_OK;
}

static PlaceRequest place_request(const svo_place_params* p) {
    return PlaceRequest{p->row_lo, p->row_hi, p->max_dist, p->ratio_num, p->ratio_den, p->tag_lo, p->tag_hi, p->min_votes, p->separation, p->max_places};
}

extern "C" int svo_desc_index_tag_votes(svo_desc_index* x, int n_ids, const uint64_t* ids, int row_lo, int row_hi, int32_t tag_lo, int32_t tag_hi,
                                        int32_t* votes, int32_t* rows, int32_t* row_first, int32_t* row_end) {
    if (const int rc = place_ids_check(x, n_ids, ids); rc != SVO_OK) return rc;
    PlaceRequest q{row_lo, row_hi, 0, 1, 1, tag_lo, tag_hi, 1, 0, 1};
    if (const PlaceRefusal e = place_check_votes(q, x->size); e != PLACE_OK) return fail(SVO_ERR_ARG, place_refusal_text(e));
    return place_run(x, q, false, n_ids, nullptr, ids, PlaceOutputs{votes, rows, row_first, row_end, nullptr, nullptr, nullptr, nullptr});
}

extern "C" int svo_desc_index_places_from_ids(svo_desc_index* x, int n_ids, const uint64_t* ids, const svo_place_params* p,
                                              svo_place_result* res, svo_place* places) {
    if (const int rc = place_ids_check(x, n_ids, ids); rc != SVO_OK) return rc;
    if (!p) return fail(SVO_ERR_ARG, "svo_desc_index_places_from_ids: null params");
    PlaceRequest q = place_request(p);
    if (const PlaceRefusal e = place_check_pick(q, x->size); e != PLACE_OK) return fail(SVO_ERR_ARG, place_refusal_text(e));
    return place_run(x, q, true, n_ids, nullptr, ids, PlaceOutputs{nullptr, nullptr, nullptr, nullptr, res, places, nullptr, nullptr});
}

extern "C" int svo_desc_index_places(svo_desc_index* x, int n, const uint8_t* query, const svo_place_params* p, svo_place_result* res,
                                     svo_place* places, int32_t* cand_query, int32_t* cand_row) {
    if (!x || !p) return fail(SVO_ERR_ARG, "svo_desc_index_places: null index / params");
    if (!x->d_points) return no_points("place candidates");
    if (n < 0 || n > SVO_RELOC_MAX_QUERIES) return fail(SVO_ERR_ARG, "svo_desc_index_places: n must be 0 .. 4096");
    if (n > 0 && !query) return fail(SVO_ERR_ARG, "svo_desc_index_places: null query");
    PlaceRequest q = place_request(p);
    if (const PlaceRefusal e = place_check(q, x->size); e != PLACE_OK) return fail(SVO_ERR_ARG, place_refusal_text(e));
    if (n == 0) return place_run(x, q, true, 0, nullptr, nullptr, PlaceOutputs{nullptr, nullptr, nullptr, nullptr, res, places, nullptr, nullptr});
    return place_run(x, q, true, n, query, nullptr, PlaceOutputs{nullptr, nullptr, nullptr, nullptr, res, places, cand_query, cand_row});
}

// ---- batched place candidates (include/svo.h, "Batched place candidates"; the kernels are in svo_kernels_place_batch.hip, the rules
// and the layouts in svo_place_batch.hpp) ----
// where a batch call's results go, each null when not wanted
struct PlaceBatchOutputs {
    int32_t *votes, *rows, *row_first, *row_end;      // tag_votes_batch: cameras x bins, then one entry per bin each
    svo_place_result* res; svo_place* places;         // the two places calls: one per camera, max_places per camera
    int32_t *cand_query, *cand_row;                   // places_batch: every camera's at its slice
};

// What tag_votes_batch (pick false, query null), places_from_ids_batch (pick, query null) and places_batch (pick, with queries)
// share.  q: the request, checked and with its row range resolved; begin: the checked offsets.  Everything is enqueued on the index's
// stream — for places_batch the queries up through the batched relocalisation's staging, the unguided search group by group and
// k_reloc_select_batch; else the offsets and the id list up — then the clearing, the table, the sweep and the pick, the copies back,
// and the host waits once.  times: from the clearing to the last place kernel
static int place_batch_run(svo_desc_index* x, const PlaceRequest& q, bool pick, int n_cameras, const int32_t* begin, const uint8_t* query,
                           const uint64_t* ids, const PlaceBatchOutputs& o) {
    int rc;
    MHIP(call_begin(x));
    if (n_cameras == 0) return SVO_OK;
    const int total = begin[n_cameras], n_bins = q.tag_hi - q.tag_lo + 1;
    const size_t C = (size_t)n_cameras, P = pick ? (size_t)q.max_places : 0;
    const bool searched = query && total > 0;         // cameras without queries recognise nothing: empty lists
    const PbLayout l = pb_layout(C, (size_t)total, (size_t)n_bins, P);
    const PbStage hs = pb_stage(l, C, (size_t)total, pick);
    if ((rc = retire_scratch(x, l.total)) != SVO_OK || (rc = grow(x, x->place, hs.total, RETIRE_SCRATCH_FIRST, 0, true)) != SVO_OK) return rc;
    uint8_t *dv = x->retire.p, *h = x->place.p;
    PbCam* d_cams = (PbCam*)(dv + l.cams);
    PlaceBin* d_bins = (PlaceBin*)(dv + l.bins);
    int32_t* d_votes = (int32_t*)(dv + l.votes);
    PbTableArgs t{(const int32_t*)(dv + l.begin), nullptr, nullptr, x->d_ids, (uint64_t*)(dv + l.list), (int32_t*)(dv + l.cam), (int32_t*)(dv + l.table),
                  fuse_table_slots(total) - 1, d_cams};
    RbLayout bl{};
    if (searched) {                                   // rule 1: svo_desc_index_localize_batch's path without guides, pixels and PnP
        const int max_slice = rb_max_slice(n_cameras, begin);
        const RbRange r = rb_plan_range(q.row_lo, q.row_hi, x->chunk_rows, max_slice);
        const MatchRange mr{r.row_lo, r.row_hi, r.chunk_rows, r.chunk0, r.n_chunks};
        const size_t states = batch_group_states(n_cameras, begin, r.n_chunks);
        svo_reloc_params rp; svo_reloc_params_default(&rp);
        DevBuffers d;
        svo_context* old = nullptr;
        rc = svo_reloc_batch_ctx(x->device, n_cameras, max_slice > 64 ? max_slice : 64, rp.ransac_iterations, rp.reproj_error, rp.confidence,
                                 &x->batch_ctx, &old, &d);
        if (old) x->batch_ctx_outgrown.push_back(old);
        if (rc != SVO_OK || (states > 0 && (rc = part_states(x, states)) != SVO_OK) || (rc = batch_room(x, C, (size_t)total)) != SVO_OK) return rc;
        bl = rb_layout(C, (size_t)total);
        uint8_t *hb = x->h_batch, *db = x->d_batch;
        memcpy(hb + bl.query, query, (size_t)total * SVO_DESC_BYTES);
        memset(hb + bl.xy, 0, bl.begin - bl.xy);      // no pixels
        memcpy(hb + bl.begin, begin, (C + 1) * sizeof(int32_t));
        memset(hb + bl.cams, 0, bl.up_end - bl.cams); // no priors
        MHIP(hipMemcpyAsync(db, hb, bl.up_end, hipMemcpyHostToDevice, x->stream));
        x->batch_total = -1;                          // the staging no longer holds a localize_batch's order
        const uint32_t* d_query = (const uint32_t*)(db + bl.query);
        const int32_t* d_begin = (const int32_t*)(db + bl.begin);
        svo_desc_match* d_match = (svo_desc_match*)(db + bl.match);
        for (int cam = 0; cam < n_cameras;) {         // a group's partial states are merged before the next group overwrites them
            const RbGroup g = rb_next_group(n_cameras, begin, cam, r.n_chunks);
            const int m = g.q1 - g.q0;
            launch_desc_match((const uint32_t*)x->d_desc, x->d_ids, d_query + (size_t)g.q0 * 8, m, mr, x->d_part(), x->stream);
            launch_desc_match_merge(x->d_part(), x->d_ids, m, mr, d_match + g.q0, x->stream);
            cam = g.cam1;
        }
        const RelocBatchSelect sel{d_match, x->d_points, (const float2*)(db + bl.xy), d_begin, RelocRule{q.max_dist, q.ratio_num, q.ratio_den},
                                   rp.min_candidates, d.tl1, d.world, d.st, d.CAP, (int32_t*)(db + bl.cand_query), (int32_t*)(db + bl.cand_row),
                                   (int32_t*)(db + bl.n_cand)};
        launch_reloc_select_batch(sel, n_cameras, x->stream);
        t.begin = d_begin; t.n_dev = (const int32_t*)(db + bl.n_cand); t.m_rows = (const int32_t*)(db + bl.cand_row);
    } else {                                          // the offsets and the ids in one copy
        memcpy(h + hs.begin, begin, (C + 1) * sizeof(int32_t));
        if (total > 0 && ids) memcpy(h + hs.ids, ids, (size_t)total * sizeof(uint64_t));
        MHIP(hipMemcpyAsync(dv + l.begin, h, hs.up_end, hipMemcpyHostToDevice, x->stream));         // [begin, list) of the scratch is cut alike
    }
    MHIP(span_mark(x, true, 0));
    MHIP(hipMemsetAsync(dv + l.cams, 0, l.down_end, x->stream));          // the records, the places, the bins, the votes
    MHIP(hipMemsetAsync(t.table, 0xFF, 4 * ((size_t)t.mask + 1), x->stream));                        // PLACE_EMPTY
    launch_place_batch_table(t, n_cameras, x->stream);
    launch_place_batch_sweep(PbSweepArgs{t.table, t.mask, t.list, t.cam, x->d_ids, x->d_points, q.row_lo, q.row_hi, q.tag_lo, q.tag_hi, n_bins, d_bins,
                                         d_votes}, x->stream);
    if (pick) launch_place_batch_pick(d_votes, d_bins, n_bins, q.tag_lo, q.min_votes, q.separation, q.max_places, (PlaceOut*)(dv + l.places), d_cams,
                                      n_cameras, x->stream);
    MHIP(hipGetLastError());
    MHIP(span_mark(x, true, 1));
    uint8_t* down = h + hs.down;
    MHIP(hipMemcpyAsync(down, dv + l.cams, pick ? l.bins : l.down_end, hipMemcpyDeviceToHost, x->stream));
    if (searched) MHIP(hipMemcpyAsync(x->h_batch + bl.n_cand, x->d_batch + bl.n_cand, bl.inlier - bl.n_cand, hipMemcpyDeviceToHost, x->stream));
    MHIP(hipStreamSynchronize(x->stream));            // the call's one wait
    MHIP(span_read(x, x->last_ms));
    const PbCam* c = (const PbCam*)(down + l.cams);
    for (int b = 0; b < n_cameras; b++)
        if (c[b].set_full) return fail(SVO_ERR_INTERNAL, "batched place candidates: the table overflowed");
    if (!pick) {
        const PlaceBin* bins = (const PlaceBin*)(down + l.bins);
        if (o.votes) memcpy(o.votes, down + l.votes, C * (size_t)n_bins * sizeof(int32_t));
        for (int i = 0; i < n_bins; i++) {
            if (o.rows) o.rows[i] = bins[i].rows;
            if (o.row_first) o.row_first[i] = place_row_first(bins[i]);
            if (o.row_end) o.row_end[i] = place_row_end(bins[i]);
        }
        return SVO_OK;
    }
    const svo_place* places = (const svo_place*)(down + l.places);
    const int32_t* h_ncand = (const int32_t*)(x->h_batch + bl.n_cand);
    for (int b = 0; b < n_cameras; b++) {
        if (o.res) { o.res[b].n_landmarks = c[b].n_landmarks; o.res[b].n_tags_voted = c[b].n_tags_voted; o.res[b].n_places = c[b].n_places; }
        if (o.places) memcpy(o.places + (size_t)b * P, places + (size_t)b * P, (size_t)c[b].n_places * sizeof(svo_place));
        if (!searched) continue;
        const int q0 = begin[b], nc = h_ncand[b];
        if (o.cand_query) memcpy(o.cand_query + q0, x->h_batch + bl.cand_query + (size_t)q0 * 4, (size_t)nc * sizeof(int32_t));
        if (o.cand_row) memcpy(o.cand_row + q0, x->h_batch + bl.cand_row + (size_t)q0 * 4, (size_t)nc * sizeof(int32_t));
    }
    return SVO_OK;
}

// the refusals the three batch calls share, in the single calls' order: the index, the offsets, the points, the list
static int place_batch_check(const svo_desc_index* x, const char* call, int n_cameras, const int32_t* begin, const void* list, const char* begin_name,
                             const char* what) {
    if (!x) return fail(SVO_ERR_ARG, "null index");
    if (const RbOffsets e = rb_check_offsets(n_cameras, begin); e != RB_OFFSETS_OK) return batch_offsets_fail(e, call, begin_name, what);
    if (!x->d_points) return no_points("place candidates");
    if (n_cameras > 0 && begin[n_cameras] > 0 && !list) return fail(SVO_ERR_ARG, "batched place candidates: null ids / query");
    return SVO_OK;
}
static int place_batch_bins_check(int n_cameras, const PlaceRequest& q) {
    if (pb_check_bins(n_cameras, q.tag_lo, q.tag_hi) != PB_OK)
        return fail(SVO_ERR_ARG, "batched place candidates: n_cameras x (tag_hi - tag_lo + 1) exceeds 1 << 24 bins: narrow the tag window (or split the cameras over calls)");
    return SVO_OK;
}

extern "C" int svo_desc_index_tag_votes_batch(svo_desc_index* x, int n_cameras, const int32_t* id_begin, const uint64_t* ids, int row_lo, int row_hi,
                                              int32_t tag_lo, int32_t tag_hi, int32_t* votes, int32_t* rows, int32_t* row_first, int32_t* row_end) {
    if (const int rc = place_batch_check(x, "svo_desc_index_tag_votes_batch", n_cameras, id_begin, ids, "id_begin", "ids"); rc != SVO_OK) return rc;
    PlaceRequest q{row_lo, row_hi, 0, 1, 1, tag_lo, tag_hi, 1, 0, 1};
    if (const PlaceRefusal e = place_check_votes(q, x->size); e != PLACE_OK) return fail(SVO_ERR_ARG, place_refusal_text(e));
    if (const int rc = place_batch_bins_check(n_cameras, q); rc != SVO_OK) return rc;
    return place_batch_run(x, q, false, n_cameras, id_begin, nullptr, ids, PlaceBatchOutputs{votes, rows, row_first, row_end, nullptr, nullptr, nullptr, nullptr});
}

extern "C" int svo_desc_index_places_from_ids_batch(svo_desc_index* x, int n_cameras, const int32_t* id_begin, const uint64_t* ids,
                                                    const svo_place_params* p, svo_place_result* results, svo_place* places) {
    if (const int rc = place_batch_check(x, "svo_desc_index_places_from_ids_batch", n_cameras, id_begin, ids, "id_begin", "ids"); rc != SVO_OK) return rc;
    if (!p) return fail(SVO_ERR_ARG, "svo_desc_index_places_from_ids_batch: null params");
    PlaceRequest q = place_request(p);
    if (const PlaceRefusal e = place_check_pick(q, x->size); e != PLACE_OK) return fail(SVO_ERR_ARG, place_refusal_text(e));
    if (const int rc = place_batch_bins_check(n_cameras, q); rc != SVO_OK) return rc;
    return place_batch_run(x, q, true, n_cameras, id_begin, nullptr, ids, PlaceBatchOutputs{nullptr, nullptr, nullptr, nullptr, results, places, nullptr, nullptr});
}

extern "C" int svo_desc_index_places_batch(svo_desc_index* x, int n_cameras, const int32_t* query_begin, const uint8_t* query, const svo_place_params* p,
                                           svo_place_result* results, svo_place* places, int32_t* cand_query, int32_t* cand_row) {
    if (const int rc = place_batch_check(x, "svo_desc_index_places_batch", n_cameras, query_begin, query, "query_begin", "queries"); rc != SVO_OK) return rc;
    if (!p) return fail(SVO_ERR_ARG, "svo_desc_index_places_batch: null params");
    PlaceRequest q = place_request(p);
    if (const PlaceRefusal e = place_check(q, x->size); e != PLACE_OK) return fail(SVO_ERR_ARG, place_refusal_text(e));
    if (const int rc = place_batch_bins_check(n_cameras, q); rc != SVO_OK) return rc;
    return place_batch_run(x, q, true, n_cameras, query_begin, query, nullptr, PlaceBatchOutputs{nullptr, nullptr, nullptr, nullptr, results, places, cand_query, cand_row});
}

// ---- landmark consolidation (include/svo.h, "Landmark consolidation"; the kernels are in svo_kernels_consolidate.hip, the rules in
// svo_consolidate.hpp): the flags, the table, the member list and the group kernel on the stream, then retire's ranks, one wait for
// the counts and the table's flag, and retire's move of the rows and its second wait ----
extern "C" void svo_consolidate_params_default(svo_consolidate_params* p, float radius) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->row_lo = 0; p->row_hi = -1; p->tag_lo = 0; p->tag_hi = INT32_MAX; p->radius = radius;
}

extern "C" int svo_desc_index_consolidate(svo_desc_index* x, const svo_consolidate_params* p, svo_consolidate_result* res, int32_t* kept_before) {
    if (!x || !p) return fail(SVO_ERR_ARG, "svo_desc_index_consolidate: null index / params");
    if (!x->d_points) return no_points("svo_desc_index_consolidate");
    ConsRequest q{p->row_lo, p->row_hi, p->tag_lo, p->tag_hi, p->radius};
    switch (cons_check(q, x->size)) {
        case CONS_RANGE: return fail(SVO_ERR_ARG, "svo_desc_index_consolidate: the row range must satisfy 0 <= row_lo <= row_hi <= size");
        case CONS_RADIUS: return fail(SVO_ERR_ARG, "svo_desc_index_consolidate: radius must be finite and >= 0");
        case CONS_OK: break;
    }
    x->retire_ms = 0.f;
    MHIP(hipSetDevice(x->device));
    const int row_lo = q.row_lo, row_hi = q.row_hi, n0 = x->size, m = row_hi - row_lo;
    int rc, kept = m;                                 // of the scope's rows
    svo_consolidate_result r;
    memset(&r, 0, sizeof(r));
    const RetireRows rows{(uint4*)x->d_desc, x->d_ids, (uint4*)x->d_points};
    ConsWork w{};                                     // w.keep stays null where no kernel runs
    void* bounce = nullptr;
    if (m > 0) {
        const ConsLayout l = cons_layout(m, n0 - row_lo, x->retire_slab);
        if ((rc = retire_ctl_room(x)) != SVO_OK || (rc = retire_scratch(x, l.total)) != SVO_OK) return rc;
        ConsCtl* d_ctl = (ConsCtl*)x->d_retire_ctl;
        w.row_lo = row_lo; w.n = m; w.tag_lo = q.tag_lo; w.tag_hi = q.tag_hi;
        w.keep = x->retire.p + l.keep;
        w.offset = (int32_t*)(x->retire.p + l.rank);
        w.sums = (int32_t*)(x->retire.p + l.counts);
        w.table = (int32_t*)(x->retire.p + l.table);
        w.count = (int32_t*)(x->retire.p + l.count);
        w.slots = retire_table_slots(m);
        w.list = (int32_t*)(x->retire.p + l.list);
        w.ctl = d_ctl;
        bounce = x->retire.p + l.bounce;
        MHIP(hipMemsetAsync(d_ctl, 0, sizeof(ConsCtl), x->stream));
        MHIP(hipMemsetAsync(w.table, 0xFF, (size_t)w.slots * sizeof(int32_t), x->stream));   // RETIRE_EMPTY
        MHIP(hipMemsetAsync(w.count, 0, (size_t)w.slots * sizeof(int32_t), x->stream));
        MHIP(span_mark(x, true, 0));
        launch_consolidate(rows, w, q.radius, x->stream);
        launch_retire_ranks(w.keep, m, w.sums, w.offset, x->stream);             // the offsets have served: their room takes the ranks
        MHIP(hipGetLastError());
        MHIP(span_mark(x, true, 1));
    }
    if ((rc = retire_finish(x, rows, row_lo, row_hi, w.keep, w.offset, bounce, sizeof(ConsCtl),
                            "svo_desc_index_consolidate: the table of ids overflowed (nothing was changed)", kept_before, &kept)) != SVO_OK) return rc;
    if (m > 0)
        for (const ConsCounts& c : ((const ConsCtl*)&x->h_retire->ctl)->counts) {
            r.n_members += c.n_members; r.n_groups += c.n_groups; r.n_far_views += c.n_far_views; r.n_capped_groups += c.n_capped_groups;
        }
    r.n_dropped = m - kept;
    r.n_kept = x->size;
    if (res) *res = r;
    return SVO_OK;
}

// ---- svo_desc_index_read_rows (include/svo.h, "Landmark consolidation"): the rows come down MATCH_STAGE_ROWS at a time through the
// pinned staging an append goes up through ----
extern "C" int svo_desc_index_read_rows(svo_desc_index* x, int row_lo, int row_hi, uint8_t* desc, uint64_t* ids, float* xyz, int32_t* tags) {
    if (!x) return fail(SVO_ERR_ARG, "null index");
    if ((xyz || tags) && !x->d_points) return no_points("svo_desc_index_read_rows");
    if (const int rc = row_range(x, row_lo, row_hi); rc != SVO_OK) return rc;
    MHIP(hipSetDevice(x->device));
    uint8_t* h_ids = x->h_stage + (size_t)MATCH_STAGE_ROWS * SVO_DESC_BYTES;
    for (int r0 = row_lo; r0 < row_hi; r0 += MATCH_STAGE_ROWS) {
        const size_t m = (size_t)(row_hi - r0 < MATCH_STAGE_ROWS ? row_hi - r0 : MATCH_STAGE_ROWS), at = (size_t)r0, to = (size_t)(r0 - row_lo);
        if (desc) MHIP(hipMemcpyAsync(x->h_stage, x->d_desc + at * SVO_DESC_BYTES, m * SVO_DESC_BYTES, hipMemcpyDeviceToHost, x->stream));
        if (ids) MHIP(hipMemcpyAsync(h_ids, x->d_ids + at, m * sizeof(uint64_t), hipMemcpyDeviceToHost, x->stream));
        if (xyz || tags) MHIP(hipMemcpyAsync(x->h_reloc->points, x->d_points + at, m * sizeof(RelocPoint), hipMemcpyDeviceToHost, x->stream));
        MHIP(hipStreamSynchronize(x->stream));
        if (desc) memcpy(desc + to * SVO_DESC_BYTES, x->h_stage, m * SVO_DESC_BYTES);
        if (ids) memcpy(ids + to, h_ids, m * sizeof(uint64_t));
        for (size_t i = 0; i < m && (xyz || tags); i++) {
            const RelocPoint& pt = x->h_reloc->points[i];
            const bool none = pt.tag == SVO_POINT_NONE;
            if (tags) tags[to + i] = pt.tag;
            if (xyz) { xyz[3 * (to + i)] = none ? INFINITY : pt.x; xyz[3 * (to + i) + 1] = none ? INFINITY : pt.y; xyz[3 * (to + i) + 2] = none ? INFINITY : pt.z; }
        }
    }
    return SVO_OK;
}

// ---- batched insertion (include/svo.h, "Batched insertion") ----
#define INSERT_STAGE_FIRST ((size_t)1 << 16)          // the row staging's first size in bytes; it doubles from there
static const size_t INSERT_HOST_DOWN = insert_layout(INSERT_MAX_ENTRIES, 0, 0).up_end;   // where h_insert keeps what comes down
static_assert(sizeof(InsertEntry) == 32 && sizeof(InsertCtl) == 64, "the entry and the control block as the kernels read them");
static_assert(sizeof(svo_track_obs) == INSERT_OBS_BYTES && offsetof(svo_track_obs, id) == INSERT_OBS_ID && offsetof(svo_track_obs, xyz) == INSERT_OBS_XYZ &&
              offsetof(svo_track_obs, flags) == INSERT_OBS_FLAGS && SVO_DESC_BYTES == INSERT_DESC_BYTES && SVO_OBS_HAS_XYZ == INSERT_HAS_XYZ &&
              SVO_INSERT_MAX_ENTRIES == INSERT_MAX_ENTRIES && SVO_INSERT_MAX_OBS_ROWS == INSERT_MAX_OBS_ROWS, "svo_insert.hpp restates include/svo.h");

// what a call asks for beyond its entries: per-entry arrays indexed by the call's entry number, each may be null
struct InsertCall { uint32_t need; bool with_points; const uint64_t* id_base; const double* cam_to_map; const int32_t* tags; };

static int insert_host_room(svo_desc_index* x) {
    const InsertLayout l = insert_layout(INSERT_MAX_ENTRIES, 0, 0);
    return room(x, x->h_insert, INSERT_HOST_DOWN + (l.down_end - l.down), true);
}

// the refusals every batched insertion shares (rules 6 and 7, the part that needs no rows)
static int insert_check(const svo_desc_index* x, int n, const InsertCall& c) {
    if (c.with_points && !x->d_points) return no_points("batched insertion with points");
    for (int b = 0; b < n && c.tags; b++) if (c.tags[b] < 0) return fail(SVO_ERR_ARG, "batched insertion: a tag must be >= 0 (nothing was added)");
    for (size_t i = 0; c.cam_to_map && i < (size_t)16 * n; i++)
        if (!isfinite(c.cam_to_map[i])) return fail(SVO_ERR_ARG, "batched insertion: cam_to_map has a non-finite entry (nothing was added)");
    return SVO_OK;
}

// entry k of a group of n_group entries, entry b of the call, into the pinned block: its rows, its tag, its id offset, its transform
static void insert_entry_fill(svo_desc_index* x, int n_group, int k, int b, int32_t begin, int32_t rows, const InsertCall& c) {
    ((InsertEntry*)x->h_insert)[k] = InsertEntry{begin, rows, 0, c.tags ? c.tags[b] : 0, c.id_base ? c.id_base[b] : 0, 0};
    if (c.cam_to_map) memcpy(x->h_insert + insert_layout(n_group, 0, 0).T + (size_t)k * 12 * sizeof(double), c.cam_to_map + (size_t)16 * b, 12 * sizeof(double));
}

// One group of n entries, filled in the pinned block (insert_entry_fill): the entries up, the kernels, the counts and flags down, one
// wait.  The rows are read at obs, desc (device addresses: the ring slot) or, with staged_rows > 0, from h_insert_rows through the
// scratch.  The kept rows go to rows at + 0 ..; n_added[0 .. n), *total.  Rule 6's refusals that only the device sees end it here.
static int insert_group(svo_desc_index* x, int n, const InsertCall& c, const uint8_t* obs, const uint8_t* desc, int staged_rows, int at,
                        int32_t* n_added, int* total) {
    const int tiles = insert_plan(n, (InsertEntry*)x->h_insert);
    *total = 0;
    if (tiles == 0) { memset(n_added, 0, sizeof(int32_t) * (size_t)n); return SVO_OK; }
    const InsertLayout l = insert_layout(n, tiles, staged_rows);
    if (const int rc = retire_scratch(x, l.total); rc != SVO_OK) return rc;
    uint8_t* d = x->retire.p;
    if (staged_rows > 0) {
        MHIP(hipMemcpyAsync(d + l.obs, x->insert_rows.p, (size_t)staged_rows * INSERT_OBS_BYTES, hipMemcpyHostToDevice, x->stream));
        MHIP(hipMemcpyAsync(d + l.desc, x->insert_rows.p + (size_t)staged_rows * INSERT_OBS_BYTES, (size_t)staged_rows * INSERT_DESC_BYTES, hipMemcpyHostToDevice, x->stream));
        obs = d + l.obs; desc = d + l.desc;
    }
    MHIP(hipMemcpyAsync(d, x->h_insert, c.cam_to_map ? l.up_end : l.T, hipMemcpyHostToDevice, x->stream));
    InsertWork w;
    w.obs = obs; w.desc = desc;
    w.entry = (const InsertEntry*)(d + l.entry); w.T = c.cam_to_map ? (const double*)(d + l.T) : nullptr;
    w.n = n; w.tiles = tiles;
    w.mask = (uint64_t*)(d + l.mask); w.offset = (int32_t*)(d + l.offset);
    w.ctl = (InsertCtl*)(d + l.down); w.n_added = (int32_t*)(d + l.n_added);
    w.need = c.need; w.with_points = c.with_points ? 1 : 0;
    w.at = at; w.room = x->capacity - at;
    MHIP(span_mark(x, true, 0));
    launch_insert(InsertRows{x->d_desc, x->d_ids, (uint4*)x->d_points}, w, x->stream);
    MHIP(hipGetLastError());
    MHIP(span_mark(x, true, 1));
    uint8_t* down = x->h_insert + INSERT_HOST_DOWN;
    MHIP(hipMemcpyAsync(down, d + l.down, sizeof(InsertCtl) + sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, x->stream));
    MHIP(hipStreamSynchronize(x->stream));
    MHIP(span_read(x, x->insert_ms));
    const InsertCtl* ctl = (const InsertCtl*)down;
    if (ctl->over) return fail(SVO_ERR_ARG, "batched insertion: the kept rows exceed the index's capacity (nothing was added)");
    if (ctl->nonfinite) return fail(SVO_ERR_ARG, "batched insertion: a kept row's point has a non-finite coordinate (nothing was added)");
    memcpy(n_added, down + sizeof(InsertCtl), sizeof(int32_t) * (size_t)n);
    *total = ctl->total;
    return SVO_OK;
}

// the call's begin and end around its groups
static int insert_begin(svo_desc_index* x, int path) {
    MHIP(call_begin(x));
    x->insert_ms = 0.f; x->insert_path = path; x->insert_scanned = x->insert_added = 0;
    return insert_host_room(x);
}
static void insert_end(svo_desc_index* x, int n, const int32_t* counts, int total, int32_t* first_row, int32_t* n_added) {
    int32_t at = x->size;
    for (int b = 0; b < n; b++) {
        if (first_row) first_row[b] = at;
        if (n_added) n_added[b] = counts[b];
        at += counts[b];
    }
    x->size += total;                                 // the one place size moves
    x->insert_added = (uint64_t)total;
}

// Entries whose rows are in host memory — entry b has rows[b] rows from row begin[b] of obs and desc — through the row staging in
// groups of whole entries of at most INSERT_MAX_OBS_ROWS rows (an entry has at most that many).  counts: n entries; *total.
static int insert_staged(svo_desc_index* x, int n, const int64_t* begin, const int32_t* rows, const uint8_t* obs, const uint8_t* desc,
                         const InsertCall& c, int32_t* counts, int* total) {
    *total = 0;
    for (int g0 = 0; g0 < n;) {
        int g1 = g0; int32_t m = 0;
        while (g1 < n && (g1 == g0 || m + rows[g1] <= INSERT_MAX_OBS_ROWS)) m += rows[g1++];
        if (const int rc = grow(x, x->insert_rows, (size_t)m * (INSERT_OBS_BYTES + INSERT_DESC_BYTES), INSERT_STAGE_FIRST, 0, true); rc != SVO_OK) return rc;
        for (int b = g0, at = 0; b < g1; at += rows[b], b++) {
            insert_entry_fill(x, g1 - g0, b - g0, b, at, rows[b], c);
            if (rows[b] == 0) continue;
            memcpy(x->insert_rows.p + (size_t)at * INSERT_OBS_BYTES, obs + (size_t)begin[b] * INSERT_OBS_BYTES, (size_t)rows[b] * INSERT_OBS_BYTES);
            memcpy(x->insert_rows.p + (size_t)m * INSERT_OBS_BYTES + (size_t)at * INSERT_DESC_BYTES, desc + (size_t)begin[b] * INSERT_DESC_BYTES, (size_t)rows[b] * INSERT_DESC_BYTES);
        }
        int added = 0;
        if (const int rc = insert_group(x, g1 - g0, c, nullptr, nullptr, m, x->size + *total, counts + g0, &added); rc != SVO_OK) return rc;
        *total += added; x->insert_scanned += (uint64_t)m;
        g0 = g1;
    }
    return SVO_OK;
}

// svo_desc_index_add_frames (with_points false) and svo_desc_index_add_frames_points
static int add_frames_run(svo_desc_index* x, svo_context* ctx, int n, const int32_t* seqs, const InsertCall& c, int32_t* first_row, int32_t* n_added) {
    if (!x) return fail(SVO_ERR_ARG, "null index");
    if (n < 1 || n > INSERT_MAX_ENTRIES) return fail(SVO_ERR_ARG, "batched insertion: n must be 1 .. 1024 entries");
    int rc = insert_check(x, n, c);
    if (rc != SVO_OK) return rc;
    SvoLastRowsView v;
    const int state = svo_last_rows_view(ctx, &v);    // a null context; the frame's state comes after the entries' sequences, as in the single call
    if (state == SVO_ERR_ARG) return state;
    for (int b = 0; b < n; b++) { const int s = seqs ? seqs[b] : b; if (s < 0 || s >= v.B) return fail(SVO_ERR_ARG, "batched insertion: an entry's sequence is outside the context"); }
    if (state != SVO_OK) return state;
    const bool ring = v.in_ring && v.device == x->device;
    if ((rc = insert_begin(x, ring ? SVO_INSERT_PATH_RING : SVO_INSERT_PATH_STAGED)) != SVO_OK) return rc;
    std::vector<int32_t> rows((size_t)n), counts((size_t)n);
    std::vector<int64_t> begin((size_t)n);
    for (int b = 0; b < n; b++) {                     // the rows the single call scans: min(n_rows, max(n_tracks, 0)), inside the pitch
        const int s = seqs ? seqs[b] : b, cap = v.hdr[2 * s] > 0 ? v.hdr[2 * s] : 0;
        int32_t r = v.hdr[2 * s + 1] < cap ? v.hdr[2 * s + 1] : cap;
        if (r < 0) r = 0;
        if ((size_t)r > v.pitch) r = (int32_t)v.pitch;
        rows[(size_t)b] = r; begin[(size_t)b] = (int64_t)s * (int64_t)v.pitch;
    }
    int total = 0;
    if (ring) {
        for (int b = 0; b < n; b++) { insert_entry_fill(x, n, b, b, (int32_t)begin[(size_t)b], rows[(size_t)b], c); x->insert_scanned += (uint64_t)rows[(size_t)b]; }
        rc = insert_group(x, n, c, (const uint8_t*)v.obs_m, v.desc_m, 0, x->size, counts.data(), &total);
    } else {
        rc = insert_staged(x, n, begin.data(), rows.data(), (const uint8_t*)v.obs_h, v.desc_h, c, counts.data(), &total);
    }
    if (rc != SVO_OK) return rc;
    insert_end(x, n, counts.data(), total, first_row, n_added);
    return SVO_OK;
}

extern "C" int svo_desc_index_add_frames(svo_desc_index* x, svo_context* ctx, int n, const int32_t* seqs, uint32_t need_flags, const uint64_t* id_base,
                                         int32_t* first_row, int32_t* n_added) {
    return add_frames_run(x, ctx, n, seqs, InsertCall{insert_need(need_flags, false), false, id_base, nullptr, nullptr}, first_row, n_added);
}

extern "C" int svo_desc_index_add_frames_points(svo_desc_index* x, svo_context* ctx, int n, const int32_t* seqs, uint32_t need_flags, const uint64_t* id_base,
                                                const double* cam_to_map, const int32_t* tags, int32_t* first_row, int32_t* n_added) {
    return add_frames_run(x, ctx, n, seqs, InsertCall{insert_need(need_flags, true), true, id_base, cam_to_map, tags}, first_row, n_added);
}

extern "C" int svo_desc_index_add_obs(svo_desc_index* x, int n, const int32_t* row_begin, const svo_track_obs* obs, const uint8_t* desc, uint32_t need_flags,
                                      const uint64_t* id_base, int with_points, const double* cam_to_map, const int32_t* tags, int32_t* first_row, int32_t* n_added) {
    if (!x) return fail(SVO_ERR_ARG, "null index");
    if (n < 0 || n > INSERT_MAX_ENTRIES || (n > 0 && !row_begin)) return fail(SVO_ERR_ARG, "svo_desc_index_add_obs: n must be 0 .. 1024 entries, with their row_begin");
    if (n == 0) return SVO_OK;
    if (row_begin[0] != 0) return fail(SVO_ERR_ARG, "svo_desc_index_add_obs: row_begin[0] must be 0");
    for (int b = 0; b < n; b++) if (row_begin[b + 1] < row_begin[b]) return fail(SVO_ERR_ARG, "svo_desc_index_add_obs: row_begin must not decrease");
    if (row_begin[n] > INSERT_MAX_OBS_ROWS) return fail(SVO_ERR_ARG, "svo_desc_index_add_obs: at most 1 << 18 rows per call");
    if (row_begin[n] > 0 && (!obs || !desc)) return fail(SVO_ERR_ARG, "svo_desc_index_add_obs: null obs / desc");
    const InsertCall c{insert_need(need_flags, with_points != 0), with_points != 0, id_base, with_points ? cam_to_map : nullptr, with_points ? tags : nullptr};
    int rc = insert_check(x, n, c);
    if (rc != SVO_OK || (rc = insert_begin(x, SVO_INSERT_PATH_STAGED)) != SVO_OK) return rc;
    std::vector<int32_t> rows((size_t)n), counts((size_t)n);
    std::vector<int64_t> begin((size_t)n);
    for (int b = 0; b < n; b++) { begin[(size_t)b] = row_begin[b]; rows[(size_t)b] = row_begin[b + 1] - row_begin[b]; }
    int total = 0;
    if ((rc = insert_staged(x, n, begin.data(), rows.data(), (const uint8_t*)obs, desc, c, counts.data(), &total)) != SVO_OK) return rc;
    insert_end(x, n, counts.data(), total, first_row, n_added);
    return SVO_OK;
}

extern "C" int svo_desc_index_get_insert_stats(const svo_desc_index* x, svo_desc_insert_stats* st) {
    if (!x || !st) return fail(SVO_ERR_ARG, "null index / stats");
    st->last_kernels_ms = x->insert_ms; st->last_path = x->insert_path;
    st->rows_scanned = x->insert_scanned; st->rows_added = x->insert_added;
    return SVO_OK;
}
