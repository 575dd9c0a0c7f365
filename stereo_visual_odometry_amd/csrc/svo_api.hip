// svo_api.hip — host side of libsvo_hip.so: context, frame pipeline, C-ABI (include/svo.h).
// The per-frame orchestration of VisualOdometry::stereo_callback (reference src/vo.cpp:41-137) is
// expressed as a fixed sequence of kernel launches on one HIP stream; every data-dependent decision
// (second FAST pass, too-few-tracks gate, RANSAC failure, motion gate, stale-pyramid quirk) is taken
// on the device from SeqState, so a frame needs no host round trip until its pose is read back.
#include "svo_internal.hpp"
#include "svo_prior.hpp"
#include "svo_match_internal.hpp"
#include "svo_reloc_internal.hpp"
#include "svo_reloc_batch_internal.hpp"
#include <stdio.h>
#include <string.h>
#include <stddef.h>
#include <stdlib.h>
#include <string>
#include <atomic>
#include <mutex>
#include <vector>
#include <algorithm>
#include <initializer_list>
#include <math.h>

static thread_local std::string g_err;
extern "C" const char* svo_last_error(void) { return g_err.c_str(); }
void svo_set_error(const char* msg) { g_err = msg; }                 // for the library's other host files (svo_match_internal.hpp declares it)
static thread_local int g_stage_path = 0;                            // svo_get_last_frame_path(NULL): this thread's last stage call

// SVO_FORCE_LEAN=1 (test knob): every context, stage contexts included, takes the 96-register builds of the f64 kernels
static bool env_on(const char* name) { const char* e = getenv(name); return e && atoi(e) != 0; }
static bool force_lean() { static const bool on = env_on("SVO_FORCE_LEAN"); return on; }
// The one place that picks the build of the f64 kernels (svo_kernels_pnp.hip: pnp_build) for the launches to come: the 96-register
// builds when the context shares its device with another many-sequence context's LK grid, or under the test knob.
static hipError_t choose_pnp_build(DevBuffers& d, bool shares_device) {
    d.co_resident = (shares_device || force_lean()) ? 1 : 0;
    return d.co_resident ? prepare_pnp_lean() : hipSuccess;
}

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            char _b[512];                                                                         \
            snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            g_err = _b;                                                                           \
            return SVO_ERR_HIP;                                                                   \
        }                                                                                         \
    } while (0)

static int fail_arg(const char* msg) { g_err = msg; return SVO_ERR_ARG; }

// The LK kernel of a many-sequence context fills the whole GPU.  When several such contexts share a device (bench.py interleaves
// two, so that one's latency-bound PnP kernels run under the other's LK), their LK launches are chained through one event per
// device: two LK grids resident together only halve each other's CUs, and HIP-event durations of either would include the other.
struct LkGate { std::mutex mu; hipEvent_t ev = nullptr; bool armed = false; std::atomic<int> contexts{0}; };
static LkGate g_lk_gate[SVO_MAX_DEVICES];

extern "C" int svo_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" void svo_config_default(svo_config* c) {
    c->bucket_start_row = 4; c->buckets_along_height = 92; c->buckets_along_width = 160;
    c->features_per_bucket = 1; c->features_threshold = 15; c->pre_matching_feature_threshold = 100;
    c->age_threshold = 20; c->fast_threshold = 20; c->ransac_reprojection_error = 8.f;
    c->ransac_iterations = 100; c->optical_flow_min_eig_threshold = 0.001;
    c->circular_matching_success_threshold = .15; c->max_translation_norm = .1; c->max_rotation_norm = .5;
    c->win_w = 10; c->win_h = 10; c->max_level = 3; c->lk_max_count = 30; c->lk_epsilon = 0.0001;
    c->ransac_confidence = 0.98f; c->max_features = 0; c->channels = 1; c->lk_float_sums = 0;
}

// cv::buildOpticalFlowPyramid's level rule: level 0 always, stop as soon as
// the NEXT level would have width <= win or height <= win.
static void make_geometry(Geometry& g, int W, int H, int win, int max_level, int pad) {
    memset(&g, 0, sizeof(g));
    g.W = W; g.H = H; g.pad = pad;
    if (max_level > SVO_MAX_LEVELS - 1) max_level = SVO_MAX_LEVELS - 1;
    int w = W, h = H, base = 0;
    for (int l = 0; l <= max_level; l++) {
        const int stride = (w + 2 * pad + 15) & ~15;
        g.lv[l].w = w; g.lv[l].h = h; g.lv[l].stride = stride; g.lv[l].off = base + pad * stride + pad;
        base += stride * (h + 2 * pad);
        g.nlevels = l + 1;
        w = (w + 1) / 2; h = (h + 1) / 2;
        if (w <= win || h <= win) break;
    }
    g.pyr_bytes = base;
}

// One pinned host table of SVO_RING slots, `pitch` elements apart: slot k is the row of the frame in ring slot k, free once that
// frame has been collected.  Two flavours (rings_alloc):
//  * RING_MAPPED: kernels read or write the host table in place; `m` is its device address.
//  * RING_UPLOADED: kernels read a device copy `d`, filled by one upload(slot, stream) per frame on the frame's stream.
// The motion-prior ring is both: its explicit rows are uploaded, and k_prior_predict writes the rows it predicts into the host
// table in place.
enum RingKind { RING_MAPPED = 1, RING_UPLOADED = 2 };
template <typename T> struct Ring {
    T *h = nullptr, *m = nullptr, *d = nullptr;
    size_t pitch = 0;
    T* row(int slot) const { return h + (size_t)slot * pitch; }
    T* mapped_row(int slot) const { return m + (size_t)slot * pitch; }
    T* dev_row(int slot) const { return (d ? d : m) + (size_t)slot * pitch; }          // what the frame's kernels are given
    hipError_t upload(int slot, hipStream_t st) const { return hipMemcpyAsync((void*)dev_row(slot), (const void*)row(slot), sizeof(T) * pitch, hipMemcpyHostToDevice, st); }
};

// Everything a frame is issued with that a setter can change.  The context holds the record of the frames to come (`next`: the
// setters write it and nothing else); enqueue_frame copies it into the frame's ring slot BEFORE the frame is issued, with the
// facts of that one frame, and everything that issues the frame reads the slot's record; collect_frame copies it into `last`.
struct FrameSettings {
    int in_format = SVO_INPUT_MONO8;             // svo_set_input_format; in.bpp <= 1 is mono8.  The kernels are chosen at issue time and take `in` as arguments
    GreyIn in = {};
    int cov_mode = SVO_COV_OFF; double cov_sigma2 = 1.;   // svo_set_pose_covariance
    bool clahe_on = false;                       // svo_set_clahe
    double clahe_clip = 0.; int clahe_tx = 0, clahe_ty = 0;
    bool track_on = false, desc_on = false;      // svo_set_track_output, svo_set_descriptor_output (the descriptors ride on the track output)
    int prior_mode = SVO_PRIOR_EXPLICIT;         // svo_set_motion_prior_mode
    // the facts of one frame (enqueue_frame; false in `next`)
    bool ragged = false;                         // it came with an active list: the act ring's row holds its flags
    bool has_masks = false;                      // its detection applies a mask to some sequence: its row of the mask ring is uploaded
    bool has_priors = false;                     // it has motion-prior rows: its row of the prior ring holds them
    bool desc() const { return track_on && desc_on; }
};
// the SVO_PATH_* bits that follow from the settings alone
static int settings_path(const FrameSettings& s) {
    return (s.in.bpp > 1 ? SVO_PATH_INPUT_CONVERTED : 0) | (s.cov_mode ? SVO_PATH_POSE_COV : 0) | (s.clahe_on ? SVO_PATH_CLAHE : 0) |
           (s.track_on ? SVO_PATH_TRACK_IDS : 0) | (s.desc() ? SVO_PATH_DESCRIPTORS : 0);
}

// One slot of the results ring: everything a frame in flight owns besides its rows of the pinned rings.
enum StageEvent { EV_F0, EV_PYR, EV_LK0, EV_LK1, EV_TRI, EV_DONE, EV_COUNT };   // stage boundaries, in svo_get_stage_timing's order
struct GraphKey {                                // what a slot's graph was captured with: the settings it bakes in (input format, covariance mode), image stride, LK grid, co-resident builds
    FrameSettings fs; int stride, gn, co;
    bool operator==(const GraphKey& o) const {
        return stride == o.stride && gn == o.gn && co == o.co && fs.in_format == o.fs.in_format && fs.cov_mode == o.fs.cov_mode &&
               (fs.cov_mode != SVO_COV_FIXED_SIGMA || fs.cov_sigma2 == o.fs.cov_sigma2);
    }
};
struct RingSlot {
    hipEvent_t ev[EV_COUNT] = {};                // EV_F0 and EV_DONE always recorded, the four between on request (stage_timing)
    hipEvent_t ev_img = nullptr;                 // the frame's pyramids stand (image stream; created with it)
    hipGraphExec_t gexec = nullptr;              // SVO_GRAPH=1: the slot fixes the pointer table, the result record and the copies
    GraphKey key = {};
    int g_path = 0;                              // the SVO_PATH_* bits of that capture
    bool staged = false;                         // the slot's stage events were recorded (launch-list mode only)
    FrameSettings fs;                            // what the slot's frame was issued with
};
// Detection masks (svo_set_detection_mask): the two slots of one scope (a sequence, or the shared pair).  cur: the slot in force for
// the frames submitted from now on (-1: none); last: the slot the most recent frame of this scope recorded for its left image — that
// frame's image is scanned by the NEXT call, so the setter writes the other one.
struct MaskPair { uint8_t* buf[2] = {nullptr, nullptr}; int cur = -1, last = -1; };

// The last collected frame: what it was issued with, and its optional rows, under one of two policies.
//  * Small rows (covariance, motion prior) are copied here when the frame is collected.
//  * Large rows (observations, their headers, descriptors) are read in place, in ring slot obs_slot, and copied into kept_* only
//    when that slot is about to be written again (keep_last_obs: a submit eight frames later, or a re-allocation of the rings).
struct LastFrame {
    int slot = -1;                               // its ring slot (-1: no frame collected yet); the slot's events time it
    FrameSettings fs;
    std::vector<PoseCovRow> cov;                 // [B], valid when fs.cov_mode
    std::vector<PriorRow> prior;                 // [B], valid when fs.has_priors
    int obs_slot = -1, obs_rows = 0;             // the slot while the rings still hold the rows, else -1: the copies below do; the row pitch (max_rows) of whichever holds them
    std::vector<svo_track_obs> kept_obs;
    std::vector<int> kept_hdr;
    std::vector<uint8_t> kept_desc;              // [B][obs_rows][32] beside kept_obs
};

struct svo_context {
    int device = 0;
    hipStream_t stream = nullptr;
    DevBuffers d = {};
    // Ownership: device memory registers in `allocs` and pinned host memory in `pinned` when it is allocated (dev_alloc,
    // pinned_alloc, rings_alloc), and svo_destroy frees by walking the two.  Only the buffers that are replaced while frames may
    // still name them have owners of their own: the rectification maps, the CLAHE buffers and the mask pairs (retire).
    std::vector<void*> allocs, pinned;
    FrameSettings next;                          // the settings of the frames submitted from now on
    LastFrame last;
    Ring<FrameResult> results;                   // [B] mapped: k_frame_end stores the records there directly (d.results)
    Ring<const uint8_t*> ptrs;                   // [2][B] mapped: the frame's image pointers, read in place by the ingest (d.img_ptrs)
    Ring<int> act;                               // [2 B] uploaded: a ragged frame's active list and flags (DevBuffers::act)
    RingSlot ring[SVO_RING];
    // many-sequence contexts build the NEXT frame's pyramids on a second stream while the current frame is in its LK kernel (issue_frame)
    hipStream_t img_stream = nullptr;
    hipEvent_t ev_begin = nullptr;
    bool begin_recorded = false;
    bool staged_inputs = false;                  // this frame's images were copied in on `stream` (host-image calls): the image stream must wait for them
    int head = 0, tail = 0, inflight = 0;        // ring indices: head = next to enqueue, tail = oldest outstanding
    uint8_t* staging = nullptr;                  // device [2][B][W*H] for host-image calls
    uint8_t* h_staging = nullptr;                // pinned host mirror of `staging`
    size_t staging_bytes = 0;                    // size of both (host-image calls of a rectifying context stage raw frames)
    uint8_t* h_upload = nullptr;                 // pinned [6][W*H]: the stage entry points' image uploads (slot x camera)
    bool projection_set = false;
    int lk_grid = 0;
    int lk_hint = 0;                             // feature count seen in the last collected frame (sizes the LK grid; 0 = unknown)
    bool use_graph = false;                      // hipGraph replay of the frame's launch list (RingSlot::gexec, replay_graph)
    bool capturing = false;                      // inside hipStreamBeginCapture / EndCapture
    bool counted = false;                        // this context is in its device's LkGate count
    int lk_room = -1;                            // lk_registers_left(d), asked once
    int k_alloc = 0;                             // RANSAC hypotheses the PnP buffers were allocated for
    bool stage_timing = false;                   // record the four stage-boundary events of a frame (svo_set_stage_timing; SVO_STAGE_TIMING=1)
    int last_path = 0;                           // SVO_PATH_* of the most recently issued frame (svo_get_last_frame_path)
    // rectification (svo_set_rectification_maps): raw_w > 0 makes the context take RAW frames.  A map is one device buffer
    // ([W*H] short2 + [W*H] u16) per camera; shared[cam] serves every sequence whose own[seq][cam] is null.  Each frame names its
    // maps in its row of the map ring (read in place by the ingest kernels, beside ptrs), so a map replaced with frames in flight
    // is only retired: freed once every frame enqueued before its replacement has been collected.
    int raw_w = 0, raw_h = 0;
    uint8_t* shared_map[2] = {};
    std::vector<uint8_t*> own_map;               // [B][2]
    Ring<const uint8_t*> maps;                   // [2][B] mapped
    struct Retired { uint8_t* p; long long after; };
    std::vector<Retired> retired;                // freed when n_collected >= after
    long long n_enqueued = 0, n_collected = 0;
    Ring<PoseCovRow> cov;                        // [B] mapped, written by k_pose_cov in place; allocated when a mode is first switched on
    // detection masks (svo_set_detection_mask).  Everything below is empty until the first mask is set.  A mask belongs to a left
    // image: img_mask[seq] is the mask of the sequence's last submitted left image — what the sequence's NEXT detection applies —
    // and a frame's row of mask_rows is filled from it when the frame is enqueued.
    MaskPair shared_mask;
    std::vector<MaskPair> own_mask;              // [B]
    std::vector<const uint8_t*> img_mask;        // [B]
    Ring<const uint8_t*> mask_rows;              // [B] uploaded: the device copy is what the masked FAST kernels read
    uint8_t* h_mask_stage = nullptr;             // pinned [W*H]: a host mask's packed rows on their way to the device
    hipEvent_t ev_mask_stage = nullptr;          // that copy has run: the staging buffer may be written again
    // CLAHE buffers, at first use (clahe_buffers): one allocation holds the device table of the staging frames' addresses ([2][B],
    // what the frame's ingest takes in place of the caller's pointer table) and the frames themselves (in_width x in_height mono8,
    // packed, `clahe_pitch` bytes apart); the LUTs are [B][2][tiles_y][tiles_x][256].
    // ONE staging set per context is enough only because a frame's CLAHE launches and the ingest that consumes them are adjacent
    // on ONE stream — img_stream for build-ahead contexts, `stream` otherwise, the same one for every CLAHE frame of a context
    // (they are never captured into a graph) — so frame N + 1's equalisation is ordered behind frame N's ingest.  A path that
    // fills the staging frames from another stream must order itself with an event.
    uint8_t* clahe_buf = nullptr;                // [table | frames]
    size_t clahe_pitch = 0;
    int clahe_w = 0, clahe_h = 0;                // the frame size clahe_buf was allocated for
    uint8_t* clahe_lut = nullptr;
    int clahe_lut_tiles = 0;                     // tiles per image clahe_lut has room for
    // track ids and observation rows (svo_set_track_output), empty until the output is first switched on; switching is refused with
    // frames in flight.  The id buffers are device memory of the context; the rings are written in place (k_track_obs,
    // k_track_desc) and re-allocated when max_rows changes.  The descriptor ring has the shape of the observation ring, a row of
    // 32 bytes beside every observation row: the same max_rows, headers, slot and moment for the host copy (keep_last_obs).
    int track_rows = 0;                          // max_rows of the observation ring as allocated
    IdArgs ids = {};
    Ring<svo_track_obs> obs;                     // [B][track_rows] mapped
    Ring<int> obs_hdr;                           // [B] {n_tracks, n_rows} mapped
    Ring<uint8_t> desc;                          // [B][track_rows as it was allocated][32] mapped
    // motion priors (svo_set_motion_prior).  Everything below is empty until the first setter.  prior_next[seq] is the prior the
    // sequence's next frame will use (has = 1) — consumed when that frame is enqueued (take_priors): the frame's rows go into its
    // row of the prior ring and from there, with one upload on the frame's stream, into the device row that k_lk_chain_prior reads.
    // A frame issued in SVO_PRIOR_LAST_ROTATION always has its device row; k_prior_predict, first on the frame's stream, fills the
    // rows no explicit prior filled, for the sequences listed in the frame's row of prior_act.
    std::vector<PriorRow> prior_next;            // [B]
    int n_prior = 0;                             // how many of them are pending
    Ring<PriorRow> prior;                        // [B] mapped and uploaded
    Ring<int> prior_act;                         // [B] mapped
};

template <typename T> static int dev_alloc(svo_context* c, T** p, size_t count) {
    void* q = nullptr;
    const size_t bytes = count * sizeof(T) > 0 ? count * sizeof(T) : 16;
    HIPCHK(hipMalloc(&q, bytes));
    c->allocs.push_back(q);                                           // registered first: a failed clear leaves nothing behind
    HIPCHK(hipMemsetAsync(q, 0, bytes, c->stream));
    *p = (T*)q;
    return SVO_OK;
}
template <typename T> static int pinned_alloc(svo_context* c, T** p, size_t bytes) {
    HIPCHK(hipHostMalloc((void**)p, bytes));
    c->pinned.push_back((void*)*p);
    return SVO_OK;
}
// free a registered buffer ahead of the context's end (a buffer that grows, a ring re-allocated at another pitch)
static void unregister(std::vector<void*>& reg, const void* p) { reg.erase(std::remove(reg.begin(), reg.end(), p), reg.end()); }
static void dev_free(svo_context* c, void* p) { if (p) { unregister(c->allocs, p); (void)hipFree(p); } }
static void pinned_free(svo_context* c, void* p) { if (p) { unregister(c->pinned, p); (void)hipHostFree(p); } }

// The one allocation of rings: a set of EMPTY rings, each cleared, all or nothing — on any failure everything this call allocated is
// freed, the rings are empty again and the HIP error is returned.  The device copy of an uploaded ring is cleared on the context's
// stream: before any frame that names its rows.
struct RingSpec { void **h, **m, **d; size_t* pitch_out; size_t elem, pitch; int kind; };
template <typename T> static RingSpec ring_spec(Ring<T>& r, size_t pitch, int kind) { return {(void**)&r.h, (void**)&r.m, (void**)&r.d, &r.pitch, sizeof(T), pitch, kind}; }
static hipError_t rings_alloc(svo_context* c, std::initializer_list<RingSpec> set) {
    hipError_t e = hipSuccess;
    for (const RingSpec& s : set) {
        const size_t bytes = s.elem * s.pitch * SVO_RING;
        if (e == hipSuccess) e = hipHostMalloc(s.h, bytes, (s.kind & RING_MAPPED) ? hipHostMallocMapped : hipHostMallocDefault);
        if (e == hipSuccess) memset(*s.h, 0, bytes);
        if (e == hipSuccess && (s.kind & RING_MAPPED)) { e = hipHostGetDevicePointer(s.m, *s.h, 0); if (e == hipSuccess && !*s.m) e = hipErrorInvalidDevicePointer; }
        if (e == hipSuccess && (s.kind & RING_UPLOADED)) e = hipMalloc(s.d, bytes);
        if (e == hipSuccess && *s.d) e = hipMemsetAsync(*s.d, 0, bytes, c->stream);
        *s.pitch_out = s.pitch;
    }
    for (const RingSpec& s : set) {
        if (e == hipSuccess) { c->pinned.push_back(*s.h); if (*s.d) c->allocs.push_back(*s.d); continue; }
        if (*s.h) (void)hipHostFree(*s.h);
        if (*s.d) (void)hipFree(*s.d);
        *s.h = *s.m = *s.d = nullptr; *s.pitch_out = 0;
    }
    return e;
}
template <typename T> static void ring_free(svo_context* c, Ring<T>& r) { pinned_free(c, (void*)r.h); dev_free(c, (void*)r.d); r = Ring<T>(); }

static int read_state(svo_context* c, int seq, SeqState* hs) {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(hs, c->d.st + seq, sizeof(SeqState), hipMemcpyDeviceToHost));
    return SVO_OK;
}
static int set_state(svo_context* c, const SeqState& hs) {
    HIPCHK(hipMemcpyAsync(c->d.st, &hs, sizeof(SeqState), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));      // hs is a stack object
    return SVO_OK;
}
// the sequences a setter's `seq` names: [*s0, *s1), -1 being all of them
static int seq_range(const svo_context* c, int seq, int* s0 = nullptr, int* s1 = nullptr) {
    if (seq < -1 || seq >= c->d.B) return fail_arg("seq out of range");
    if (s0) { *s0 = seq < 0 ? 0 : seq; *s1 = seq < 0 ? c->d.B : seq + 1; }
    return SVO_OK;
}
// a buffer that frames in flight may still name (a replaced map, CLAHE buffer): freed once every frame enqueued so far has been collected
static void retire(svo_context* c, uint8_t* p) {
    if (!p) return;
    if (c->inflight == 0) (void)hipFree(p);
    else c->retired.push_back({p, c->n_enqueued});
}

// what a context derives from its configuration's parameters, once d.CAP and d.geom stand (ctx_create, stage_reconfigure)
static void derive_from_config(svo_context* c, const svo_config& cfg) {
    DevBuffers& d = c->d;
    c->lk_grid = (cfg.max_features > 0 && cfg.max_features < d.CAP) ? cfg.max_features : d.CAP;
    d.lk_crit = lk_make_crit(cfg, d.geom);
    double pc = (double)cfg.ransac_confidence; pc = pc > 0. ? pc : 0.; pc = pc < 1. ? pc : 1.;
    d.ransac_log_num = log(1. - pc > 2.2250738585072014e-308 ? 1. - pc : 2.2250738585072014e-308);
}

static int ctx_create(const svo_config* cfg_in, int device, int n_seq, int width, int height, int cap_override, svo_context** out) {
    if (!out) return fail_arg("out is null");
    *out = nullptr;
    svo_config cfg;
    if (cfg_in) cfg = *cfg_in; else svo_config_default(&cfg);
    if (n_seq < 1 || width < 16 || height < 16) return fail_arg("n_seq >= 1 and width/height >= 16 required");
    if (cfg.win_w != cfg.win_h || !lk_window_supported(cfg.win_w)) return fail_arg("unsupported LK window (square, 5 .. 31)");
    if (width <= cfg.win_w || height <= cfg.win_h) return fail_arg("image must be larger than the LK window");
    if (cfg.features_per_bucket < 1 || cfg.features_per_bucket > 64) return fail_arg("features_per_bucket must be 1 .. 64");
    if (cfg.buckets_along_height < 1 || cfg.buckets_along_width < 1 || cfg.ransac_iterations < 1) return fail_arg("bad bucket grid / ransac_iterations");
    if (cfg.channels == 0) cfg.channels = 1;
    if (cfg.channels != 1 && cfg.channels != 3) return fail_arg("channels must be 1 or 3");
    if (cfg.lk_float_sums != 0 && cfg.lk_float_sums != 1) return fail_arg("lk_float_sums must be 0 or 1");
    if (!lk_window_supported_cn(cfg.win_w, cfg.channels)) return fail_arg("this LK window is not built for 3-channel input (5 .. 21 are)");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail_arg("no such HIP device");
    HIPCHK(hipSetDevice(device));
    svo_context* c = new svo_context();
    struct Undo { svo_context* c; ~Undo() { if (c) svo_destroy(c); } } undo{c};     // every early return below frees what exists so far
    c->device = device;
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    DevBuffers& d = c->d;
    d.B = n_seq; d.cfg = cfg; d.K = cfg.ransac_iterations; d.CN = cfg.channels; c->k_alloc = d.K;
    d.NB = cfg.buckets_along_height * cfg.buckets_along_width;
    d.bucket_h = (height + cfg.buckets_along_height - 1) / cfg.buckets_along_height;     // feature_set.cpp:91-93,103-104
    d.bucket_w = (width + cfg.buckets_along_width - 1) / cfg.buckets_along_width;
    int rows = cfg.buckets_along_height - cfg.bucket_start_row; if (rows < 0) rows = 0;
    d.CAP = rows * cfg.buckets_along_width * cfg.features_per_bucket;
    if (d.CAP < 64) d.CAP = 64;
    if (cap_override > d.CAP) d.CAP = cap_override;
    make_geometry(d.geom, width, height, cfg.win_w, cfg.max_level, lk_pad_for(cfg.win_w));
    derive_from_config(c, cfg);
    const size_t B = n_seq, CAP = d.CAP;
    int rc;
#define ALLOC(ptr, count) if ((rc = dev_alloc(c, &(ptr), (count))) != SVO_OK) return rc;
    ALLOC(d.st, B);
    ALLOC(d.pyr, B * 2 * SVO_PYR_SLOTS * (size_t)d.CN * (size_t)d.geom.pyr_bytes + 256);   // + slack: the LK kernel's unaligned dword loads may read a few bytes past a row
    // The derivative pyramid of the levels >= 1 (svo_internal.hpp), for the contexts whose pyramids the image stream builds ahead:
    // many sequences, grey, exact sums.  Cleared here — that IS its constant-zero border, nothing writes there again.  Every other
    // context keeps the null pointer and its LK kernel differentiates in registers.  SVO_LK_DERIV=0 switches the planes off (A/B).
    {
        static const bool off = getenv("SVO_LK_DERIV") && atoi(getenv("SVO_LK_DERIV")) == 0;
        if (!off && ingest_ahead_applies(d) && !cfg.lk_float_sums)
            ALLOC(d.deriv, B * 2 * SVO_PYR_SLOTS * 2 * (size_t)deriv_samples(d.geom) + 128);   // + slack: the last row's over-read
    }
    if (d.CN == 3) ALLOC(d.fastimg, B * SVO_PYR_SLOTS * (size_t)width * (size_t)height + 256);
    for (int k = 0; k < 2; k++) { ALLOC(d.feat_xy[k], B * CAP); ALLOC(d.feat_age[k], B * CAP); ALLOC(d.feat_str[k], B * CAP); }
    ALLOC(d.bucket_keys, B * (size_t)d.NB);
    ALLOC(d.bucket_rowcnt, B * (size_t)cfg.buckets_along_height); ALLOC(d.emit_ticket, B);
    if (cfg.features_per_bucket > 1) {
        d.KPCAP = d.CAP + ((width + 1) / 2) * ((height + 1) / 2);       // strict 3x3 NMS: at most one keypoint per 2x2 block
        const size_t KC = (size_t)d.KPCAP, SL = (size_t)d.NB * cfg.features_per_bucket;
        ALLOC(d.score, B * (size_t)width * height); ALLOC(d.kp_rows, B * (size_t)height);
        ALLOC(d.cand_xy, B * KC); ALLOC(d.cand_age, B * KC); ALLOC(d.cand_str, B * KC); ALLOC(d.n_cand, B);
        ALLOC(d.slot_xy, B * SL); ALLOC(d.slot_age, B * SL); ALLOC(d.slot_str, B * SL); ALLOC(d.slot_n, B * (size_t)d.NB);
    }
    ALLOC(d.pl0, B * CAP); ALLOC(d.pl1, B * CAP); ALLOC(d.pr1, B * CAP); ALLOC(d.pr0, B * CAP); ALLOC(d.plc, B * CAP);
    ALLOC(d.okmask, B * CAP); ALLOC(d.lk_work, B * CAP);
    ALLOC(d.tl0, B * CAP); ALLOC(d.tr0, B * CAP); ALLOC(d.tl1, B * CAP); ALLOC(d.tr1, B * CAP);
    ALLOC(d.world, B * CAP * 3); ALLOC(d.inlier, B * CAP); ALLOC(d.inl_idx, B * CAP);
    ALLOC(d.subsets, B * (size_t)d.K * 5); ALLOC(d.hyp, B * (size_t)d.K * 12); ALLOC(d.hyp_good, B * (size_t)d.K);
    {
        double* lam = nullptr;
        ALLOC(lam, 33);
        double h[33];
        const double LOG10 = log(10.);
        for (int k = -16; k <= 16; k++) h[k + 16] = exp(k * LOG10);      // CvLevMarq: lambda = exp(lambdaLg10 * log(10))
        HIPCHK(hipMemcpyAsync(lam, h, sizeof(h), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));                          // h is a stack array
        d.lm_lambda = lam;
    }
#undef ALLOC
    // the results ring lives in pinned HOST memory that the device can write: k_frame_end stores the B records there directly
    // (180 B per sequence over PCIe) instead of a device buffer plus a copy operation per frame; the pointer tables are read in
    // place by k_ingest: no per-frame upload
    HIPCHK(rings_alloc(c, {ring_spec(c->results, B, RING_MAPPED), ring_spec(c->ptrs, 2 * B, RING_MAPPED), ring_spec(c->act, 2 * B, RING_UPLOADED),
                           ring_spec(c->maps, 2 * B, RING_MAPPED)}));
    d.results = c->results.m; d.img_ptrs = c->ptrs.m;
    c->own_map.assign(2 * B, nullptr);
    for (RingSlot& r : c->ring) for (hipEvent_t& e : r.ev) HIPCHK(hipEventCreate(&e));
    // initial state: rotation = I, translation = 0, last_transform = I (vo.h:266-268); no slots in use
    std::vector<SeqState> hs(B);
    memset(hs.data(), 0, sizeof(SeqState) * B);
    for (size_t i = 0; i < B; i++) {
        hs[i].slot_img_t0 = -1; hs[i].slot_pyr_t0 = -1;
        for (int k = 0; k < 9; k++) hs[i].R[k] = (k % 4 == 0);
        for (int k = 0; k < 16; k++) hs[i].last_T[k] = (k % 5 == 0);
    }
    HIPCHK(hipMemcpyAsync(d.st, hs.data(), sizeof(SeqState) * B, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    // SVO_GRAPH=1 replays every frame as a captured hipGraph.  Measured on MI355X, one sequence, synchronous, host images
    // (scratch/graph_ab.py, same box): 0.718 ms per frame pair with the launch list, 0.737 ms with the graph — the ~25 launches
    // are issued ahead of the GPU anyway and the graph's dispatch is not cheaper on this runtime — so the launch list stays
    // the default and the graph is the option.
    c->use_graph = env_on("SVO_GRAPH");
    c->lk_room = lk_registers_left(c->d);
    if (device >= 0 && device < SVO_MAX_DEVICES && n_seq > SVO_LONE_MAX_SEQ) {
        std::lock_guard<std::mutex> lock(g_lk_gate[device].mu);
        g_lk_gate[device].contexts++; c->counted = true;
    }
    c->stage_timing = env_on("SVO_STAGE_TIMING");
    undo.c = nullptr;
    *out = c;
    return SVO_OK;
}

extern "C" int svo_create(const svo_config* cfg, int device, int n_seq, int width, int height, svo_context** out) {
    return ctx_create(cfg, device, n_seq, width, height, 0, out);
}

// Several many-sequence contexts on one device.  Two answers, both read ONCE per frame (enqueue_frame) and passed down;
// `contexts` is an atomic: contexts are created and destroyed on other threads while this one enqueues frames.
//  * shared: the contexts' LK launches wait for each other (one event per device).  Always, when the device is shared: two
//    LK grids resident together only share the CUs — measured the same whole-job rate either way at w = 21 (18 370 vs 18 390
//    frame-pairs/s) — and unchained each launch's duration contains a part of the other's (12.7 ms per launch chained, 13.3-16.4
//    unchained, varying from run to run), which makes the per-launch figure of the dominant kernel, the one the bench line's
//    roofline is computed from, meaningless.
//  * lean: the f64 kernels run as 96-register builds under the OTHER context's LK grid — only if those builds fit beside it
//    (lk_registers_left >= 96: w = 22 grey, w = 17 / 23 / 31 grey and w = 10 / 12 BGR with float sums; not w = 21 since round 3,
//    nor w = 10 / 15 grey, nor w = 31 in the default mode).
// SVO_LK_GATE=0 switches both off (measurement).
struct DeviceSharing { bool shared, lean; };
static DeviceSharing device_sharing(const svo_context* c) {
    static const bool off = getenv("SVO_LK_GATE") && atoi(getenv("SVO_LK_GATE")) == 0;
    const bool shared = !off && c->counted && g_lk_gate[c->device].contexts.load(std::memory_order_relaxed) > 1;
    return {shared, shared && c->lk_room >= 96};
}

extern "C" void svo_destroy(svo_context* c) {
    if (!c) return;
    if (c->counted) {
        LkGate& g = g_lk_gate[c->device];
        std::lock_guard<std::mutex> lock(g.mu);
        if (--g.contexts == 0 && g.ev) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->stream); (void)hipEventDestroy(g.ev); g.ev = nullptr; g.armed = false; }
    }
    // teardown is best effort: errors here have nowhere to go, the calls are (void)ed on purpose
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (void* p : c->allocs) (void)hipFree(p);
    for (void* p : c->pinned) (void)hipHostFree(p);
    // the buffers with owners of their own (svo_context, Ownership)
    for (uint8_t* p : {c->shared_map[0], c->shared_map[1], c->shared_mask.buf[0], c->shared_mask.buf[1], c->clahe_buf, c->clahe_lut}) if (p) (void)hipFree(p);
    for (uint8_t* p : c->own_map) if (p) (void)hipFree(p);
    for (const MaskPair& m : c->own_mask) for (uint8_t* p : m.buf) if (p) (void)hipFree(p);
    for (const auto& r : c->retired) (void)hipFree(r.p);
    if (c->ev_mask_stage) (void)hipEventDestroy(c->ev_mask_stage);
    for (RingSlot& r : c->ring) {
        for (hipEvent_t e : r.ev) if (e) (void)hipEventDestroy(e);
        if (r.ev_img) (void)hipEventDestroy(r.ev_img);
        if (r.gexec) (void)hipGraphExecDestroy(r.gexec);
    }
    if (c->ev_begin) (void)hipEventDestroy(c->ev_begin);
    if (c->img_stream) (void)hipStreamDestroy(c->img_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" void* svo_get_stream(svo_context* c) { return c ? (void*)c->stream : nullptr; }

extern "C" int svo_get_lk_registers_left(svo_context* c) { return c ? c->lk_room : -1; }

extern "C" int svo_get_last_frame_path(svo_context* c) { return c ? c->last_path : g_stage_path; }

extern "C" int svo_set_projection(svo_context* c, int seq, const float Pl[12], const float Pr[12]) {
    if (!c || !Pl || !Pr) return fail_arg("null argument");
    int s0, s1;
    if (const int rc = seq_range(c, seq, &s0, &s1)) return rc;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    // Pl, Pr, K are adjacent members of SeqState: one strided 2-D copy writes them into every selected sequence's record
    // (row = the 33 floats, pitch = sizeof(SeqState)) instead of three blocking copies per sequence
    static_assert(offsetof(SeqState, Pr) == offsetof(SeqState, Pl) + sizeof(float) * 12 && offsetof(SeqState, K) == offsetof(SeqState, Pl) + sizeof(float) * 24,
                  "Pl, Pr, K must be contiguous");
    const int ns = s1 - s0;
    std::vector<float> rows((size_t)ns * 33);
    for (int s = 0; s < ns; s++) {
        float* r = rows.data() + (size_t)s * 33;
        memcpy(r, Pl, sizeof(float) * 12); memcpy(r + 12, Pr, sizeof(float) * 12);
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) r[24 + 3 * i + j] = Pl[4 * i + j];   // K = Pl[:, :3]  (vo.cpp:16-25)
    }
    HIPCHK(hipMemcpy2D((char*)(c->d.st + s0) + offsetof(SeqState, Pl), sizeof(SeqState), rows.data(), sizeof(float) * 33, sizeof(float) * 33, (size_t)ns,
                       hipMemcpyHostToDevice));
    c->projection_set = true;
    return SVO_OK;
}

// the size of the frames the caller passes: the raw size when the context rectifies, else the context's own
static int in_width(const svo_context* c) { return c->raw_w > 0 ? c->raw_w : c->d.geom.W; }
static int in_height(const svo_context* c) { return c->raw_w > 0 ? c->raw_h : c->d.geom.H; }
// bytes per pixel of those frames: the channels of a colour context, else the input format's
static int in_bpp(const svo_context* c) { return c->d.CN == 3 ? 3 : c->next.in.bpp > 1 ? c->next.in.bpp : 1; }

// The frame's view of the context's buffers: c->d plus the slot's rows of the active list and of the map table (every other launch
// sees the context's own unmasked, plain DevBuffers).  n_act >= 0: a ragged frame — only the n_act sequences listed in the slot's
// row of the act ring take it (its grids cover those alone, through DevBuffers::act); that row is uploaded on the stream of the
// frame's first kernel (kernels never read host memory for it).
static DevBuffers frame_view(const svo_context* c, int slot, int n_act) {
    DevBuffers f = c->d;
    if (n_act >= 0) { f.act = c->act.dev_row(slot); f.n_act = n_act; }
    if (c->raw_w > 0) f.rmap = c->maps.dev_row(slot);                // the frame's own maps (fill_slot_rows filled the row)
    f.in = c->ring[slot].fs.in;                                      // the format the frame was enqueued with
    return f;
}

// ---- CLAHE (svo.h): geometry, buffers and the two launches in front of an ingest ----
// Rule 1 of the definition for a w x h image: the tile size, or false when the rule rejects the geometry.
static bool clahe_geometry(int w, int h, int tiles_x, int tiles_y, int* tw, int* th) {
    if (w < 1 || h < 1 || tiles_x < 1 || tiles_y < 1) return false;
    int ew = w, eh = h;
    if (w % tiles_x != 0 || h % tiles_y != 0) {
        const int ex = tiles_x - w % tiles_x, ey = tiles_y - h % tiles_y;          // a divisible dimension grows by a whole tiles_*
        if (ex > w - 1 || ey > h - 1) return false;                                // REFLECT_101 undefined
        ew += ex; eh += ey;
    }
    *tw = ew / tiles_x; *th = eh / tiles_y;
    return *tw > 0 && *th > 0;
}
static int check_clahe_params(double clip_limit, int tiles_x, int tiles_y) {
    if (tiles_x < 1 || tiles_x > 16 || tiles_y < 1 || tiles_y > 16) return fail_arg("CLAHE: tiles must be 1 .. 16 in both directions");
    if (!isfinite(clip_limit)) return fail_arg("CLAHE: clip_limit must be finite");
    return SVO_OK;
}
// everything of ClaheArgs the definition derives from (size, tiles, clip limit); false: rule 1 rejects the geometry
static bool clahe_derive(ClaheArgs& a, int w, int h, double clip_limit, int tiles_x, int tiles_y) {
    int tw, th;
    if (!clahe_geometry(w, h, tiles_x, tiles_y, &tw, &th)) return false;
    a.w = w; a.h = h; a.tiles_x = tiles_x; a.tiles_y = tiles_y; a.tw = tw; a.th = th;
    const int area = tw * th;
    a.clip = 0;
    if (clip_limit > 0.) {
        const double v = clip_limit * area / 256.;
        a.clip = v >= (double)area ? area : ((int)v > 1 ? (int)v : 1);             // (no bin exceeds area: a larger clip cuts nothing either)
    }
    a.scale = 255.0f / (float)area; a.inv_tw = 1.0f / (float)tw; a.inv_th = 1.0f / (float)th;
    return true;
}
// The staging frames and LUTs for the context's input size and tile count as they are NOW; buffers of another size that frames in
// flight may still name are retired like replaced rectification maps.
static int clahe_buffers(svo_context* c, const FrameSettings& fs) {
    const int W = in_width(c), H = in_height(c), B = c->d.B;
    if (!c->clahe_buf || c->clahe_w != W || c->clahe_h != H) {
        const size_t table = (sizeof(uint8_t*) * 2 * B + 255) & ~(size_t)255, pitch = ((size_t)W * H + 255) & ~(size_t)255;
        uint8_t* p = nullptr;
        HIPCHK(hipMalloc((void**)&p, table + pitch * 2 * B + 256));
        std::vector<const uint8_t*> ptrs((size_t)2 * B);
        for (int i = 0; i < 2 * B; i++) ptrs[i] = p + table + pitch * i;
        if (hipMemcpy(p, ptrs.data(), sizeof(uint8_t*) * 2 * B, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(p); g_err = "CLAHE: pointer table upload failed"; return SVO_ERR_HIP; }
        retire(c, c->clahe_buf);
        c->clahe_buf = p; c->clahe_pitch = pitch; c->clahe_w = W; c->clahe_h = H;
    }
    const int tiles = fs.clahe_tx * fs.clahe_ty;
    if (!c->clahe_lut || c->clahe_lut_tiles < tiles) {
        uint8_t* p = nullptr;
        HIPCHK(hipMalloc((void**)&p, (size_t)B * 2 * tiles * 256));
        retire(c, c->clahe_lut);
        c->clahe_lut = p; c->clahe_lut_tiles = tiles;
    }
    return SVO_OK;
}
// The frame's two CLAHE launches on st, in front of the ingest that st runs next: srcs / stride are the caller's frames in the format
// f.in; afterwards they name the staging frames and f.in is mono8 — the ingest runs as a mono8 frame's, maps and active list unchanged.
static int clahe_front(svo_context* c, const FrameSettings& fs, DevBuffers& f, const uint8_t* const*& srcs, int& stride, hipStream_t st) {
    ClaheArgs a = {};
    if (!clahe_derive(a, in_width(c), in_height(c), fs.clahe_clip, fs.clahe_tx, fs.clahe_ty)) {
        g_err = "CLAHE: the tiles do not fit the raw size this context now rectifies (svo.h, CLAHE rule 1)";
        return SVO_ERR_STATE;
    }
    if (const int rc = clahe_buffers(c, fs)) return rc;
    const size_t table = (sizeof(uint8_t*) * 2 * c->d.B + 255) & ~(size_t)255;
    a.srcs = srcs; a.act = f.act; a.B = c->d.B; a.ncam = 2; a.stride = stride; a.g = f.in;
    a.lut = c->clahe_lut; a.out = c->clahe_buf + table; a.pitch = c->clahe_pitch;
    launch_clahe(a, launch_seqs(f), st);
    srcs = reinterpret_cast<const uint8_t* const*>(c->clahe_buf); stride = a.w;
    f.in = GreyIn{1, 0, 0, 0, 0, 0, 0};
    return SVO_OK;
}

// The front of a many-sequence frame: its pyramids are built on the IMAGE stream, which only waits for the previous frame's reset —
// so, with frames in flight, they are built while the previous frame sits in its LK kernel.  That kernel fills six of a SIMD's
// eight wave slots and 480 of its 512 registers (svo_kernels_lk.hip): the ingest, pyramid and border kernels (11-17 registers)
// are the ones that still fit beside it.  The frame's own stream then resets the state (ev_begin marks that) and goes on.
static int front_ahead(svo_context* c, DevBuffers& f, int slot, int stride) {
    hipStream_t s = c->stream;
    RingSlot& r = c->ring[slot];
    if (!c->img_stream) {
        HIPCHK(hipStreamCreateWithFlags(&c->img_stream, hipStreamNonBlocking));   // (highest priority measured: same rate, but the two contexts' LK launches then run in lock-step)
        HIPCHK(hipEventCreateWithFlags(&c->ev_begin, hipEventDisableTiming));
        for (RingSlot& q : c->ring) HIPCHK(hipEventCreateWithFlags(&q.ev_img, hipEventDisableTiming));
    }
    if (c->begin_recorded) HIPCHK(hipStreamWaitEvent(c->img_stream, c->ev_begin, 0));   // the fields k_pick_next reads are those of the frame in flight
    else if (c->inflight > 0) {
        // the frame in flight did not come this way (a replayed graph, an all-idle frame): ev_begin does not mark its reset, so
        // k_pick_next could read its slot fields before its reset and pick the slot that frame is building — wait for all of it
        HIPCHK(hipEventRecord(c->ev_begin, s));
        HIPCHK(hipStreamWaitEvent(c->img_stream, c->ev_begin, 0));
    }
    if (c->staged_inputs) HIPCHK(hipStreamWaitEvent(c->img_stream, r.ev[EV_F0], 0));   // host-image call: the H2D copies were queued on `stream` before this frame's start event
    if (f.act) HIPCHK(c->act.upload(slot, c->img_stream));
    const uint8_t* const* srcs = c->ptrs.dev_row(slot);
    if (r.fs.clahe_on) if (const int rc = clahe_front(c, r.fs, f, srcs, stride, c->img_stream)) return rc;   // behind the waits above, like the ingest
    launch_ingest_pyramid(f, srcs, stride, c->img_stream, PYR_NEXT);
    HIPCHK(hipEventRecord(r.ev_img, c->img_stream));
    HIPCHK(hipStreamWaitEvent(s, r.ev_img, 0));
    launch_frame_begin(f, s);
    HIPCHK(hipEventRecord(c->ev_begin, s));
    return SVO_OK;
}

// What enqueue_frame decides for one frame besides its settings (RingSlot::fs), handed to issue_frame and replay_graph.
// n_act: see frame_view.  mrows: the frame's row of the mask ring's device copy when its detection applies a mask to some sequence
// (take_masks), else null.  pri: the frame's motion priors (take_priors) — rows: its device row when some active sequence has an
// explicit prior or the frame predicts (SVO_PRIOR_LAST_ROTATION), else null; predict: k_prior_predict fills the rows no explicit
// prior filled; uploaded: the explicit rows were copied into the device row.
struct FramePriors { PriorRow* rows = nullptr; bool predict = false, uploaded = false; };
struct FramePlan {
    int slot = 0, stride = 0, gn = 0, n_act = -1;   // gn: the LK grid
    bool with_events = false;                    // record the stage-boundary events (a graph capture records none)
    DeviceSharing share = {};
    const uint8_t* const* mrows = nullptr;
    FramePriors pri;
};
// can the frame run as a replay of its slot's captured graph?  (a ragged, rectifying, masked, CLAHE, track-ids or motion-prior frame: no)
static bool graph_replayable(const svo_context* c, const FrameSettings& fs, int n_act) {
    return c->use_graph && n_act < 0 && c->raw_w == 0 && !fs.has_masks && !fs.clahe_on && !fs.track_on && !fs.has_priors;
}

// The launch list of one frame (vo.cpp:41-137 as kernels), between the slot's start and done events.
static int issue_frame(svo_context* c, const FramePlan& p) {
    hipStream_t s = c->stream;
    const int slot = p.slot, n_act = p.n_act;
    const FrameSettings& fs = c->ring[slot].fs;
    const PriorRow* const prow = p.pri.rows;
    int stride = p.stride;
    const auto record = [&](StageEvent which) { return p.with_events && !c->capturing ? hipEventRecord(c->ring[slot].ev[which], s) : hipSuccess; };
    if (n_act == 0) {                                                  // all idle: the result rows are the whole frame
        HIPCHK(c->act.upload(slot, s));
        HIPCHK(record(EV_PYR)); HIPCHK(record(EV_LK0)); HIPCHK(record(EV_LK1)); HIPCHK(record(EV_TRI));
        launch_frame_end(frame_view(c, slot, 0), slot, s);
        c->begin_recorded = false; c->last_path = 0;
        return SVO_OK;
    }
    // the predicted priors first: SeqState::ok and R are the previous frame's (k_pnp_final ran on this stream) until the per-frame
    // reset below clears ok — the PYR_BEGIN ingest, the fused front, or launch_frame_begin behind front_ahead
    if (p.pri.predict)
        launch_prior_predict(c->d, n_act >= 0 ? c->prior_act.mapped_row(slot) : nullptr, n_act >= 0 ? n_act : c->d.B, p.pri.uploaded,
                             p.pri.rows, c->prior.mapped_row(slot), s);
    HIPCHK(choose_pnp_build(c->d, p.share.lean));
    DevBuffers f = frame_view(c, slot, n_act);                         // after the build choice: co_resident travels in the view
    int path = (f.co_resident ? SVO_PATH_LEAN : 0) | settings_path(fs);
    const bool ids = fs.track_on;
    const uint8_t* const* dp = c->ptrs.dev_row(slot);                  // the slot's pointer table: pinned host memory the kernel reads in place
    const bool ahead = !c->capturing && ingest_ahead_applies(f);
    bool detected = false;
    if (ahead) {
        if (const int rc = front_ahead(c, f, slot, stride)) return rc;
        path |= SVO_PATH_INGEST_AHEAD;
    } else {
        if (f.act) HIPCHK(c->act.upload(slot, s));
        if (fs.clahe_on) if (const int rc = clahe_front(c, fs, f, dp, stride, s)) return rc;   // the front below then ingests the staging frames as mono8
        detected = !p.mrows && !ids && launch_front_fused(f, dp, stride, s);   // lone stream: ingest + pyramid beside detection, two launches (a masked or ids frame: the unfused front)
        if (detected) path |= SVO_PATH_FRONT_FUSED;
        else launch_ingest_pyramid(f, dp, stride, s, PYR_BEGIN);       // + the per-frame reset
    }
    c->begin_recorded = ahead;
    HIPCHK(record(EV_PYR));                                            // (fused front: ms[0] = the whole front, ms[1] ~ 0)
    if (ids) {                                                         // both passes with the ids build of the emit, masked or not
        const MaskArgs m = {p.mrows, f.geom.W};
        launch_detect_ids(f, c->ids, p.mrows ? &m : nullptr, 0, -1, s); launch_detect_ids(f, c->ids, p.mrows ? &m : nullptr, 1, -1, s);
        if (p.mrows) path |= SVO_PATH_DETECT_MASKED;
    } else if (p.mrows) {                                                // both passes behind the masks of the image they scan
        const MaskArgs m = {p.mrows, f.geom.W};
        launch_detect_masked(f, m, 0, -1, s); launch_detect_masked(f, m, 1, -1, s);
        path |= SVO_PATH_DETECT_MASKED;
    } else if (!detected) { launch_detect(f, 0, -1, s); launch_detect(f, 1, -1, s); }
    // chained LK launches (a captured graph cannot wait for another stream's event): wait before the launch, record after it
    LkGate* const gate = !c->capturing && p.share.shared ? &g_lk_gate[c->device] : nullptr;
    if (gate) {
        std::lock_guard<std::mutex> lock(gate->mu);
        if (gate->armed) HIPCHK(hipStreamWaitEvent(s, gate->ev, 0));
        path |= SVO_PATH_LK_CHAINED;
    }
    HIPCHK(record(EV_LK0));
    if (!launch_lk_chain(f, p.gn, s, 1, prow)) { g_err = "no LK kernel is built for this window / channel count"; return SVO_ERR_STATE; }   // with priors: k_lk_chain_prior, the LK launch of this frame in every respect
    if (prow) path |= SVO_PATH_MOTION_PRIOR | (p.pri.predict ? SVO_PATH_PRIOR_PREDICTED : 0);
    HIPCHK(record(EV_LK1));
    if (gate) {
        std::lock_guard<std::mutex> lock(gate->mu);
        if (!gate->ev) HIPCHK(hipEventCreateWithFlags(&gate->ev, hipEventDisableTiming));
        HIPCHK(hipEventRecord(gate->ev, s));
        gate->armed = true;
    }
    launch_compact(f, s);
    if (ids) launch_ids_compact(f, c->ids, s);
    const bool tri_epnp = launch_triangulate_epnp_fused(f, s);          // lone stream: the first EPnP chunk runs beside the triangulation
    if (tri_epnp) path |= SVO_PATH_TRI_EPNP_FUSED;
    else launch_triangulate(f, s);
    HIPCHK(record(EV_TRI));                                            // (fused: the stage timers count that chunk with the triangulation)
    launch_pnp(f, s, tri_epnp);
    if (fs.cov_mode) launch_pose_cov(f, CovArgs{c->cov.dev_row(slot), fs.cov_mode, fs.cov_sigma2}, s);   // into the pinned ring, like the record below
    if (ids) launch_track_obs(f, c->ids, TrackObsArgs{c->obs.dev_row(slot), c->obs_hdr.dev_row(slot), c->track_rows}, s);
    if (fs.desc())                     // every observation row's descriptor, on the T1 pyramid k_frame_end is about to rename
        launch_track_desc(f, DescArgs{c->desc.dev_row(slot), c->track_rows}, s);
    launch_frame_end(f, slot, s);      // writes the result records straight into the pinned host ring (d.results is host memory mapped into the device)
    c->last_path = path;
    return SVO_OK;
}

// The one check of a frame's arguments (svo_last_error shows which failed first: the order is part of the interface).  Without a
// mask both arrays must be there; with one every ACTIVE sequence needs both image pointers — an idle one's are never read, and the
// arrays may be NULL when no sequence is active.  pointers_last: svo_submit_batch_masked looks at a masked frame's pointers last.
static int check_stride(const svo_context* c, int stride) {
    return stride < in_width(c) * in_bpp(c) ? fail_arg("stride < width * channels (raw width when rectifying; bytes per pixel of the input format)") : SVO_OK;
}
static int check_frame_args(const svo_context* c, const uint8_t* const* left, const uint8_t* const* right, int stride, const uint8_t* active,
                            bool pointers_last = false) {
    const auto pointers = [&]() {
        if (!active) return left && right ? SVO_OK : fail_arg("null argument");
        for (int i = 0; i < c->d.B; i++)
            if (active[i] && (!left || !right || !left[i] || !right[i])) return fail_arg("null image pointer for an active sequence");
        return (int)SVO_OK;
    };
    int rc;
    if (!pointers_last && (rc = pointers()) != SVO_OK) return rc;
    if (!c->projection_set) { g_err = "svo_set_projection must be called first"; return SVO_ERR_STATE; }
    if ((rc = check_stride(c, stride)) != SVO_OK) return rc;
    return pointers_last ? pointers() : SVO_OK;
}

// the rectification map of (sequence, camera): its own, else the context's shared one (nullptr: none installed)
static const uint8_t* map_of(const svo_context* c, int seq, int cam) {
    const uint8_t* own = c->own_map[2 * seq + cam];
    return own ? own : c->shared_map[cam];
}

// The slot's rows of the pinned rings for one frame: image pointers, the active list and flags of a masked frame, the maps of a
// rectifying context (free: the slot's previous frame has been collected).  *n_act = -1 for a frame every sequence takes — a mask
// with every flag set is the unmasked frame — else the number of active sequences.
static int fill_slot_rows(svo_context* c, int slot, const uint8_t* const* left_dev, const uint8_t* const* right_dev, const uint8_t* active, int* n_act) {
    const int B = c->d.B;
    const uint8_t** hp = c->ptrs.row(slot);
    *n_act = -1;
    if (active) {
        int* ha = c->act.row(slot);
        int n = 0;
        for (int i = 0; i < B; i++) { ha[B + i] = active[i] ? 1 : 0; if (active[i]) ha[n++] = i; }
        if (n < B) *n_act = n;
    }
    const uint8_t** hm = c->raw_w > 0 ? c->maps.row(slot) : nullptr;
    for (int i = 0; i < B; i++) {
        const bool on = !active || active[i];
        hp[i] = on ? left_dev[i] : nullptr; hp[B + i] = on ? right_dev[i] : nullptr;
        for (int cam = 0; hm && cam < 2; cam++) {
            const uint8_t* m = map_of(c, i, cam);
            if (on && !m) { g_err = "rectifying context: a sequence has no rectification map (svo_set_rectification_maps)"; return SVO_ERR_STATE; }
            hm[cam * B + i] = on ? m : nullptr;
        }
    }
    return SVO_OK;
}

// SVO_GRAPH=1: the frame as a replay of the slot's captured launch list, re-captured when its GraphKey differs: the capture bakes
// in the stride, the LK grid and which builds of the f64 kernels run (a context captured while it had the device to itself would
// keep the full-register builds that cannot start beside another many-sequence context's LK grid).  *replayed = false: the
// capture failed and the option is now off — capture is an optimisation, the caller issues the same launches directly.
static int replay_graph(svo_context* c, const FramePlan& p, bool* replayed) {
    hipStream_t s = c->stream;
    RingSlot& r = c->ring[p.slot];
    HIPCHK(choose_pnp_build(c->d, p.share.lean));                      // before the capture: issue_frame then finds the lean EPnP prepared
    const GraphKey now = {r.fs, p.stride, p.gn, c->d.co_resident};
    if (!r.gexec || !(r.key == now)) {
        if (r.gexec) { (void)hipGraphExecDestroy(r.gexec); r.gexec = nullptr; }
        hipGraph_t g = nullptr;
        bool ok = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            c->capturing = true;
            const int rc = issue_frame(c, p);
            c->capturing = false;
            ok = (hipStreamEndCapture(s, &g) == hipSuccess) && rc == SVO_OK && g;
        }
        if (ok) ok = hipGraphInstantiate(&r.gexec, g, nullptr, nullptr, 0) == hipSuccess;
        if (g) (void)hipGraphDestroy(g);
        if (ok) { r.key = now; r.g_path = c->last_path; }
        else { (void)hipGetLastError(); r.gexec = nullptr; c->use_graph = false; }
    }
    *replayed = c->use_graph;
    if (!c->use_graph) return SVO_OK;
    HIPCHK(hipGraphLaunch(r.gexec, s));
    c->begin_recorded = false;
    c->last_path = r.g_path | SVO_PATH_GRAPH;
    return SVO_OK;
}

// Detection masks of one frame.  The detection of this call scans each active sequence's PREVIOUS left image, so it applies the mask
// recorded with that image (img_mask); the mask in force now — the sequence's own, else the shared one — is recorded with this
// frame's left image for the next call.  Idle sequences keep their record.  p->mrows: the frame's row of the device table (uploaded
// here, on the frame's stream) when some active sequence's detection is masked, else null — the frame is then an unmasked one.
static int take_masks(svo_context* c, const uint8_t* active, FramePlan* p) {
    p->mrows = nullptr;
    if (c->img_mask.empty()) return SVO_OK;                           // no mask was ever set
    const int B = c->d.B;
    const uint8_t** row = c->mask_rows.row(p->slot);
    bool any = false;
    for (int i = 0; i < B; i++) {
        const bool on = !active || active[i];
        row[i] = on ? c->img_mask[i] : nullptr;
        any |= row[i] != nullptr;
        if (!on) continue;
        MaskPair& m = c->own_mask[i].cur >= 0 ? c->own_mask[i] : c->shared_mask;
        c->img_mask[i] = m.cur >= 0 ? m.buf[m.cur] : nullptr;
        if (m.cur >= 0) m.last = m.cur;
    }
    if (!any) return SVO_OK;
    HIPCHK(c->mask_rows.upload(p->slot, c->stream));
    p->mrows = c->mask_rows.dev_row(p->slot);
    return SVO_OK;
}

// Motion priors of one frame: every active sequence with a pending prior hands it to this frame (one-shot: it is consumed here) —
// idle sequences keep theirs.  p->pri.rows: the frame's device row, filled by one upload on the frame's stream from the slot's pinned
// row, when some active sequence has one; else null, and the frame is an ordinary one.  In SVO_PRIOR_LAST_ROTATION the frame always
// has its device row and k_prior_predict fills what no explicit prior filled: the upload is then made only when one was taken, and
// the slot's list of the sequences that take the frame is written for that kernel.
static int take_priors(svo_context* c, const FrameSettings& fs, const uint8_t* active, FramePlan* p) {
    p->pri = FramePriors();
    const bool predict = fs.prior_mode == SVO_PRIOR_LAST_ROTATION;
    if (c->n_prior == 0 && !predict) return SVO_OK;
    const int B = c->d.B, slot = p->slot;
    PriorRow* row = c->prior.row(slot);
    bool any = false;
    for (int i = 0; i < B; i++) {
        PriorRow& q = c->prior_next[i];
        const bool take = q.has && (!active || active[i]);
        if (take) { row[i] = q; q.has = 0; c->n_prior--; any = true; }
        else { row[i].has = 0; row[i].source = 0; }
    }
    if (!any && !predict) return SVO_OK;
    if (any) HIPCHK(c->prior.upload(slot, c->stream));
    if (predict && active) {
        int* list = c->prior_act.row(slot);
        for (int i = 0, n = 0; i < B; i++) if (active[i]) list[n++] = i;
    }
    p->pri.rows = c->prior.dev_row(slot); p->pri.predict = predict; p->pri.uploaded = any;
    return SVO_OK;
}

// The last collected frame's large rows, wherever they are now: its slot of the rings, or the kept copies.
struct LastRows { const int* hdr; const svo_track_obs* obs; const uint8_t* desc; size_t pitch; };   // pitch: rows per sequence
static LastRows last_rows(const svo_context* c) {
    const LastFrame& l = c->last;
    if (l.obs_slot < 0) return {l.kept_hdr.data(), l.kept_obs.data(), l.kept_desc.data(), (size_t)l.obs_rows};
    return {c->obs_hdr.row(l.obs_slot), c->obs.row(l.obs_slot), l.fs.desc() ? c->desc.row(l.obs_slot) : nullptr, (size_t)l.obs_rows};
}
// one sequence's rows of `elem` bytes each out of `src` (LastRows::obs or ::desc); returns how many were copied
static int copy_last_rows(const LastRows& lr, const void* src, size_t elem, int seq, int cap, void* out, int* n_tracks) {
    if (n_tracks) *n_tracks = lr.hdr[2 * seq];
    const int n = lr.hdr[2 * seq + 1] < cap ? lr.hdr[2 * seq + 1] : cap;
    if (n > 0) memcpy(out, (const uint8_t*)src + (size_t)seq * lr.pitch * elem, elem * (size_t)n);
    return n;
}
// Those rows out of the ring slot that is about to be written again, into the context's own copies (LastFrame, second policy).
static void keep_last_obs(svo_context* c) {
    LastFrame& l = c->last;
    const LastRows lr = last_rows(c);
    const size_t B = c->d.B, R = lr.pitch;
    l.kept_hdr.assign(lr.hdr, lr.hdr + 2 * B);
    l.kept_obs.resize(B * R);
    if (lr.desc) l.kept_desc.resize(B * R * SVO_DESC_BYTES);
    for (size_t i = 0; i < B; i++) {
        copy_last_rows(lr, lr.obs, sizeof(svo_track_obs), (int)i, (int)R, l.kept_obs.data() + i * R, nullptr);
        if (lr.desc) copy_last_rows(lr, lr.desc, SVO_DESC_BYTES, (int)i, (int)R, l.kept_desc.data() + i * R * SVO_DESC_BYTES, nullptr);
    }
    l.obs_slot = -1;
}

// Enqueue one frame.  ptrs: host arrays of B DEVICE image pointers.  active: NULL (every sequence takes the frame) or B flags,
// checked by check_frame_args.
static int enqueue_frame(svo_context* c, const uint8_t* const* left_dev, const uint8_t* const* right_dev, int stride,
                         const uint8_t* active = nullptr) {
    if (c->inflight >= SVO_RING) { g_err = "too many frames in flight (collect first)"; return SVO_ERR_STATE; }
    RingSlot& r = c->ring[c->head];
    FramePlan p;
    p.slot = c->head; p.stride = stride; p.with_events = c->stage_timing;
    int rc;
    if ((rc = fill_slot_rows(c, p.slot, left_dev, right_dev, active, &p.n_act)) != SVO_OK) return rc;
    // LK grid sized from the last feature counts the host has seen (+30 %); the kernel strides, so an underestimate is only slower
    // (tests/test_gpu_count_seams.py, case D: 1025 features on the grid a hint of 20 gives, also in flight and re-captured)
    p.gn = c->lk_grid;
    if (c->lk_hint > 0) {
        int h = c->lk_hint + c->lk_hint / 3 + 64;
        if (c->use_graph) h = (h + 511) / 512 * 512;                 // coarse steps: the graph is re-captured when this changes
        if (h < p.gn) p.gn = h;
    }
    p.share = device_sharing(c);                                     // read once per frame: every use below sees the same answer
    HIPCHK(hipEventRecord(r.ev[EV_F0], c->stream));
    FrameSettings& fs = r.fs = c->next;                              // the frame's own record (the slot is free): a setter called from now on is the next frame's
    fs.ragged = active != nullptr;
    if ((rc = take_masks(c, active, &p)) != SVO_OK) return rc;
    if ((rc = take_priors(c, fs, active, &p)) != SVO_OK) return rc;
    fs.has_masks = p.mrows != nullptr; fs.has_priors = p.pri.rows != nullptr;
    if (fs.track_on && p.slot == c->last.obs_slot) keep_last_obs(c);  // the frame is about to write the slot svo_get_last_track_obs still reads
    bool replayed = false;
    if (graph_replayable(c, fs, p.n_act) && (rc = replay_graph(c, p, &replayed)) != SVO_OK) return rc;
    if (!replayed && (rc = issue_frame(c, p)) != SVO_OK) return rc;
    r.staged = !replayed && c->stage_timing;
    c->staged_inputs = false;
    HIPCHK(hipEventRecord(r.ev[EV_DONE], c->stream));
    HIPCHK(hipGetLastError());
    c->head = (c->head + 1) % SVO_RING; c->inflight++; c->n_enqueued++;
    return SVO_OK;
}

static int collect_frame(svo_context* c, double* T_out, int* ok_out, svo_frame_stats* stats) {
    if (c->inflight <= 0) { g_err = "nothing to collect"; return SVO_ERR_STATE; }
    const int slot = c->tail, B = c->d.B;
    HIPCHK(hipEventSynchronize(c->ring[slot].ev[EV_DONE]));
    const FrameResult* r = c->results.row(slot);
    int mx = 0;
    for (int i = 0; i < B; i++) {
        if (T_out) memcpy(T_out + 16 * i, r[i].T, sizeof(double) * 16);
        if (ok_out) ok_out[i] = r[i].ok;
        if (stats) stats[i] = r[i].stats;
        if (r[i].stats.n_after_detect > mx) mx = r[i].stats.n_after_detect;
    }
    if (mx > 0) c->lk_hint = mx;
    LastFrame& l = c->last;
    const FrameSettings& fs = l.fs = c->ring[slot].fs;
    if (fs.cov_mode) memcpy(l.cov.data(), c->cov.row(slot), sizeof(PoseCovRow) * B);
    if (fs.has_priors) l.prior.assign(c->prior.row(slot), c->prior.row(slot) + B);   // the host's explicit rows, k_prior_predict's in place
    l.obs_slot = fs.track_on ? slot : -1;                            // read in place
    if (fs.track_on) l.obs_rows = c->track_rows;
    const int* flags = c->act.row(slot) + B;
    for (int i = 0; fs.ragged && i < B; i++) {                       // idle sequences took no launch: zero rows, zero headers (their prior rows say has = 0 already)
        if (flags[i]) continue;
        if (fs.cov_mode) memset(&l.cov[i], 0, sizeof(PoseCovRow));
        if (fs.track_on) c->obs_hdr.row(slot)[2 * i] = c->obs_hdr.row(slot)[2 * i + 1] = 0;
    }
    c->last.slot = slot;
    c->tail = (c->tail + 1) % SVO_RING; c->inflight--; c->n_collected++;
    if (!c->retired.empty()) {                                       // buffers no frame in flight can name any more
        size_t k = 0;
        for (const auto& q : c->retired) { if (q.after <= c->n_collected) (void)hipFree(q.p); else c->retired[k++] = q; }
        c->retired.resize(k);
    }
    return SVO_OK;
}

// Is p page-locked host memory the DMA engines can read in place (hipHostMalloc / hipHostRegister / svo_alloc_pinned)?
static bool host_pointer_is_pinned(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // older runtimes: an error for pageable memory
    return a.type == hipMemoryTypeHost;
}
// rows of rowb bytes, `stride` apart, packed: one memcpy when they already are
static void pack_rows(uint8_t* dst, const uint8_t* src, size_t rowb, size_t rows, size_t stride) {
    if (stride == rowb) memcpy(dst, src, rowb * rows);
    else for (size_t y = 0; y < rows; y++) memcpy(dst + y * rowb, src + y * stride, rowb);
}
// Host images -> pinned staging -> device staging (one contiguous H2D copy); fills lp / rp with the device addresses.
// Images that already live in page-locked memory with packed rows skip the staging copy: the DMA reads them in place (the call
// is synchronous, the caller's buffer outlives it) — 40 us of host memcpy less per KITTI-sized pair on the single-stream path.
// active (ragged frame): idle sequences' images are not read (their pointers may be NULL; their staging areas keep old bytes).
static int stage_host_images(svo_context* c, const uint8_t* const* left, const uint8_t* const* right, int stride,
                             std::vector<const uint8_t*>& lp, std::vector<const uint8_t*>& rp, const uint8_t* active = nullptr) {
    const int B = c->d.B, W = in_width(c), H = in_height(c);
    const size_t rowb = (size_t)W * in_bpp(c), img = rowb * H;
    if (c->staging_bytes < img * 2 * B) {                             // no frame in flight reads the staging buffers (synchronous calls only)
        dev_free(c, c->staging); pinned_free(c, c->h_staging);
        c->staging = nullptr; c->h_staging = nullptr; c->staging_bytes = 0;
        if (const int rc = dev_alloc(c, &c->staging, img * 2 * B)) return rc;
        if (const int rc = pinned_alloc(c, &c->h_staging, img * 2 * B)) return rc;
        c->staging_bytes = img * 2 * B;
    }
    // rows are packed into pinned memory on the CPU (handles any stride), then contiguous async H2D copies (a 2-D copy from
    // pageable memory degenerates into per-row transfers: 3.5 ms per 1241x376 image).  All left images first, so that their
    // DMA runs while the CPU packs the right ones.
    lp.resize(B); rp.resize(B);
    c->staged_inputs = true;
    for (int cam = 0; cam < 2; cam++) {
        const uint8_t* const* src = cam ? right : left;
        bool all_direct = (size_t)stride == rowb;
        for (int i = 0; i < B && all_direct; i++) {
            if (active && !active[i]) continue;
            if (!src[i]) return fail_arg("null image pointer");
            all_direct = host_pointer_is_pinned(src[i]);
        }
        for (int i = 0; i < B; i++) {
            (cam ? rp : lp)[i] = c->staging + img * (cam * B + i);
            if (active && !active[i]) continue;
            if (!src[i]) return fail_arg("null image pointer");
            if (all_direct) {
                HIPCHK(hipMemcpyAsync(c->staging + img * (cam * B + i), src[i], img, hipMemcpyHostToDevice, c->stream));
                continue;
            }
            pack_rows(c->h_staging + img * (cam * B + i), src[i], rowb, (size_t)H, (size_t)stride);
        }
        if (!all_direct) HIPCHK(hipMemcpyAsync(c->staging + img * B * cam, c->h_staging + img * B * cam, img * B, hipMemcpyHostToDevice, c->stream));
    }
    return SVO_OK;
}
extern "C" int svo_submit_batch_masked(svo_context* c, const uint8_t* const* left_dev, const uint8_t* const* right_dev, int stride,
                                       const uint8_t* active) {
    if (!c) return fail_arg("null context");
    if (const int rc = check_frame_args(c, left_dev, right_dev, stride, active, active != nullptr)) return rc;
    HIPCHK(hipSetDevice(c->device));
    return enqueue_frame(c, left_dev, right_dev, stride, active);
}

extern "C" int svo_submit_batch(svo_context* c, const uint8_t* const* left_dev, const uint8_t* const* right_dev, int stride) {
    if (!c) return fail_arg("null argument");
    return svo_submit_batch_masked(c, left_dev, right_dev, stride, nullptr);
}

extern "C" int svo_reset_sequence(svo_context* c, int seq, const float Pl[12], const float Pr[12]) {
    if (!c) return fail_arg("null context");
    int s0, s1;
    if (const int rc = seq_range(c, seq, &s0, &s1)) return rc;
    if ((Pl == nullptr) != (Pr == nullptr)) return fail_arg("Pl and Pr must both be given or both be NULL");
    HIPCHK(hipSetDevice(c->device));
    SeqProjection p = {};
    if (Pl) { memcpy(p.Pl, Pl, sizeof(p.Pl)); memcpy(p.Pr, Pr, sizeof(p.Pr)); p.set = 1; }
    launch_reset_seq(c->d, seq, p, c->stream);                       // behind every frame submitted so far, before every later one
    if (c->ids.next_id) launch_ids_reset(c->ids, s0, s1 - s0, c->stream);   // next_id = 0, stream-ordered like the rest
    HIPCHK(hipGetLastError());
    if (Pl && seq < 0) c->projection_set = true;
    for (int i = s0; c->n_prior > 0 && i < s1; i++)   // a pending motion prior belonged to the stream that ends here
        if (c->prior_next[i].has) { c->prior_next[i].has = 0; c->n_prior--; }
    return SVO_OK;
}

extern "C" int svo_collect(svo_context* c, double* T_out, int* ok_out, svo_frame_stats* stats) {
    if (!c) return fail_arg("null context");
    HIPCHK(hipSetDevice(c->device));
    return collect_frame(c, T_out, ok_out, stats);
}

extern "C" int svo_process_batch_masked(svo_context* c, const uint8_t* const* left, const uint8_t* const* right, int stride,
                                        int images_on_device, const uint8_t* active, double* T_out, int* ok_out, svo_frame_stats* stats) {
    if (!c) return fail_arg("null context");
    int rc = check_frame_args(c, left, right, stride, active);
    if (rc != SVO_OK) return rc;
    if (c->inflight != 0) { g_err = "svo_process_batch with frames in flight"; return SVO_ERR_STATE; }
    HIPCHK(hipSetDevice(c->device));
    if (images_on_device) {
        rc = enqueue_frame(c, left, right, stride, active);
    } else {
        // the caller's buffers are only borrowed for the duration of the call: copy to the device first (SURVEY.md §8b "Ownership")
        std::vector<const uint8_t*> lp, rp;
        if ((rc = stage_host_images(c, left, right, stride, lp, rp, active)) != SVO_OK) return rc;
        rc = enqueue_frame(c, lp.data(), rp.data(), in_width(c) * in_bpp(c), active);
    }
    if (rc != SVO_OK) return rc;
    return collect_frame(c, T_out, ok_out, stats);
}

extern "C" int svo_process_batch(svo_context* c, const uint8_t* const* left, const uint8_t* const* right, int stride,
                                 int images_on_device, double* T_out, int* ok_out, svo_frame_stats* stats) {
    if (!c) return fail_arg("null argument");
    return svo_process_batch_masked(c, left, right, stride, images_on_device, nullptr, T_out, ok_out, stats);
}

extern "C" int svo_process(svo_context* c, const uint8_t* left, const uint8_t* right, int stride, double T_out[16], svo_frame_stats* stats) {
    if (!c) return fail_arg("null context");
    if (c->d.B != 1) return fail_arg("svo_process needs a context created with n_seq == 1");
    int ok = 0;
    const uint8_t* l[1] = {left}; const uint8_t* r[1] = {right};
    int rc = svo_process_batch(c, l, r, stride, 0, T_out, &ok, stats);
    return rc != SVO_OK ? rc : ok;
}

extern "C" void* svo_alloc_pinned(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
extern "C" void svo_free_pinned(void* p) { if (p) (void)hipHostFree(p); }

// ---- motion priors (svo.h): the host arithmetic, the buffers, the setters ----
// One prior as the kernels take it (svo_prior.hpp has the arithmetic): H checked, Hi the caller's or H's inverse rounded to f32.
static int make_prior_row(const float* H, const float* Hi, PriorRow* out) {
    if (const char* err = prior_make(H, Hi, out->H, out->Hi)) return fail_arg(err);
    out->has = 1; out->source = 0;
    return SVO_OK;
}
// can this context take a prior at all?  (k_lk_chain_prior is the grey, exact-sums build)
static int check_prior_context(const svo_context* c) {
    if (c->d.CN != 1) return fail_arg("motion priors need a channels == 1 context");
    if (c->d.cfg.lk_float_sums) return fail_arg("motion priors need lk_float_sums == 0 (that mode reproduces the reference's recording, which has no prior)");
    return SVO_OK;
}
// the prior ring and the list ring of the predicting frames, at first use
static int prior_buffers(svo_context* c) {
    if (c->prior.h) return SVO_OK;
    HIPCHK(hipSetDevice(c->device));
    const size_t B = (size_t)c->d.B;
    if (rings_alloc(c, {ring_spec(c->prior, B, RING_MAPPED | RING_UPLOADED), ring_spec(c->prior_act, B, RING_MAPPED)}) != hipSuccess) {
        (void)hipGetLastError(); g_err = "motion prior: buffer allocation failed"; return SVO_ERR_HIP;
    }
    c->prior_next.assign(B, PriorRow{});
    return SVO_OK;
}
static void set_pending(svo_context* c, int seq, const PriorRow* row /* null: clear */) {
    PriorRow& p = c->prior_next[seq];
    c->n_prior += (row ? 1 : 0) - (p.has ? 1 : 0);
    if (row) p = *row; else p.has = 0;
}

extern "C" int svo_set_motion_prior(svo_context* c, int seq, const float H[9], const float Hi[9]) {
    if (!c) return fail_arg("null context");
    int rc = check_prior_context(c); if (rc != SVO_OK) return rc;
    int s0, s1;
    if ((rc = seq_range(c, seq, &s0, &s1)) != SVO_OK) return rc;
    if (!H) {                                                                     // clear: nothing to do before the first prior
        for (int i = s0; c->prior.h && i < s1; i++) set_pending(c, i, nullptr);
        return SVO_OK;
    }
    PriorRow row;
    if ((rc = make_prior_row(H, Hi, &row)) != SVO_OK) return rc;
    if ((rc = prior_buffers(c)) != SVO_OK) return rc;
    for (int i = s0; i < s1; i++) set_pending(c, i, &row);
    return SVO_OK;
}

extern "C" int svo_set_motion_priors(svo_context* c, const float* H, const float* Hi, const uint8_t* has) {
    if (!c || !H) return fail_arg("null argument");
    int rc = check_prior_context(c); if (rc != SVO_OK) return rc;
    const int B = c->d.B;
    std::vector<PriorRow> rows((size_t)B);
    for (int i = 0; i < B; i++)                                                   // every used row is checked before anything changes
        if ((!has || has[i]) && (rc = make_prior_row(H + 9 * i, Hi ? Hi + 9 * i : nullptr, &rows[i])) != SVO_OK) return rc;
    if ((rc = prior_buffers(c)) != SVO_OK) return rc;
    for (int i = 0; i < B; i++) set_pending(c, i, (!has || has[i]) ? &rows[i] : nullptr);
    return SVO_OK;
}

extern "C" int svo_get_motion_prior(svo_context* c, int seq, float H[9], float Hi[9], int* pending) {
    if (!c || seq < 0 || seq >= c->d.B) return fail_arg("bad context / seq");
    const bool on = c->n_prior > 0 && c->prior_next[seq].has;
    if (pending) *pending = on ? 1 : 0;
    if (on && H) memcpy(H, c->prior_next[seq].H, sizeof(float) * 9);
    if (on && Hi) memcpy(Hi, c->prior_next[seq].Hi, sizeof(float) * 9);
    return SVO_OK;
}

extern "C" int svo_set_motion_prior_mode(svo_context* c, int mode) {
    if (!c) return fail_arg("null context");
    if (mode != SVO_PRIOR_EXPLICIT && mode != SVO_PRIOR_LAST_ROTATION) return fail_arg("unknown motion prior mode");
    int rc = check_prior_context(c); if (rc != SVO_OK) return rc;
    if (mode == SVO_PRIOR_LAST_ROTATION && (rc = prior_buffers(c)) != SVO_OK) return rc;
    c->next.prior_mode = mode;
    return SVO_OK;
}

extern "C" int svo_get_motion_prior_mode(svo_context* c, int* mode) {
    if (!c || !mode) return fail_arg("null argument");
    *mode = c->next.prior_mode;
    return SVO_OK;
}

extern "C" int svo_get_last_motion_prior(svo_context* c, int seq, float H[9], float Hi[9], int* source) {
    if (!c || !source || seq < 0 || seq >= c->d.B) return fail_arg("bad context / seq / null source");
    if (c->last.slot < 0) { g_err = "svo_get_last_motion_prior: no frame collected yet"; return SVO_ERR_STATE; }
    *source = 0;
    if (!c->last.fs.has_priors || !c->last.prior[seq].has) return SVO_OK;        // the frame had no prior rows, or none for seq
    const PriorRow& p = c->last.prior[seq];
    *source = p.source == PRIOR_SOURCE_PREDICTED ? 2 : 1;
    if (H) memcpy(H, p.H, sizeof(float) * 9);
    if (Hi) memcpy(Hi, p.Hi, sizeof(float) * 9);
    return SVO_OK;
}

extern "C" int svo_motion_prior_from_rotation(const float Pl[12], const double R[9], float H[9], float Hi[9]) {
    if (!Pl || !R) return fail_arg("null argument");
    if (const char* err = prior_from_rotation(Pl, R, H, Hi)) return fail_arg(err);
    return SVO_OK;
}

// the end of both circularMatching entry points (vo.cpp:203-230): the four LK passes, then every pass's raw points and the mask
// (prior: the device row of a motion prior — svo_circular_match_prior — or null)
static int circular_tail(svo_context* c, int n, float* pl1, float* pr1, float* pr0, float* pl0_circle, uint8_t* ok, const PriorRow* prior = nullptr) {
    const DevBuffers& d = c->d;
    if (!launch_lk_chain(d, n, c->stream, 0, prior)) { g_err = "no LK kernel is built for this window / channel count"; return SVO_ERR_STATE; }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(pl1, d.pl1, sizeof(float2) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(pr1, d.pr1, sizeof(float2) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(pr0, d.pr0, sizeof(float2) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(pl0_circle, d.plc, sizeof(float2) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(ok, d.okmask, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; i++) ok[i] &= 1;                                       // bit0 = status0..3 && loop closure (vo.cpp:227-230)
    return SVO_OK;
}

// VisualOdometry::circularMatching as a member call on the context's own state (vo.h:374-379, vo.cpp:169-240 without the
// compaction): the T0 side is the pyramid pair the context cached (lastLeftPyramid / lastRightPyramid, vo.h:257-258), the
// T1 pyramids are built from the given images and BECOME the cached pair (vo.cpp:231-232) — so the next stereo_callback
// tracks against them, exactly as in the reference, where both entry points share those members.  Empty input returns
// before anything is cached (vo.cpp:179-181).  currentVOFeatures, the cached T0 images and frame_id are left alone.
extern "C" int svo_circular_matching(svo_context* c, const uint8_t* left_t1, const uint8_t* right_t1, int stride, int n,
                                     const float* pl0, float* pl1, float* pr1, float* pr0, float* pl0_circle, uint8_t* ok) {
    if (!c || !left_t1 || !right_t1 || n < 0) return fail_arg("bad arguments");
    if (n > 0 && (!pl0 || !pl1 || !pr1 || !pr0 || !pl0_circle || !ok)) return fail_arg("null arrays");
    if (c->d.B != 1) return fail_arg("svo_circular_matching needs a context created with n_seq == 1");
    int rc = check_stride(c, stride); if (rc != SVO_OK) return rc;
    if (c->inflight != 0) { g_err = "svo_circular_matching with frames in flight"; return SVO_ERR_STATE; }
    if (c->next.track_on) { g_err = "svo_circular_matching with the track output on: it overwrites the feature set behind the ids (svo_set_track_output(ctx, 0, 0) first)"; return SVO_ERR_STATE; }
    if (c->n_prior > 0) { g_err = "svo_circular_matching with a motion prior pending: priors belong to the frame pipeline (svo_set_motion_prior(ctx, -1, NULL, NULL) clears them; svo_circular_match_prior is the stage call)"; return SVO_ERR_STATE; }
    if (n == 0) return SVO_OK;                                                    // vo.cpp:179-181
    if (n > c->d.CAP) { g_err = "more points than the context's feature capacity"; return SVO_ERR_CAPACITY; }
    HIPCHK(hipSetDevice(c->device));
    SeqState hs; if ((rc = read_state(c, 0, &hs)) != SVO_OK) return rc;
    if (hs.frame_id < 1 || hs.slot_pyr_t0 < 0) { g_err = "no cached pyramids: call svo_process first (the reference primes them in stereo_callback, vo.cpp:47-56)"; return SVO_ERR_STATE; }
    const SeqState keep = hs;
    // every error return below leaves the context's tracking state as it was: the guard writes `keep` back unless the call
    // completes (then the state with the new cached pyramids is written instead)
    struct Restore {
        svo_context* c; const SeqState* st; bool armed = true;
        ~Restore() { if (armed) { (void)hipMemcpyAsync(c->d.st, st, sizeof(SeqState), hipMemcpyHostToDevice, c->stream); (void)hipStreamSynchronize(c->stream); } }
    } restore{c, &keep};
    const int t1 = free_slot(hs);
    // the points go into the idle half of the feature double-buffer (scratch between frames); the state is put back below
    hs.slot_t1 = t1; hs.active = 1; hs.feat_buf = keep.feat_buf ^ 1; hs.n_feat = n;
    HIPCHK(hipMemcpyAsync(c->d.feat_xy[hs.feat_buf], pl0, sizeof(float2) * n, hipMemcpyHostToDevice, c->stream));
    if ((rc = set_state(c, hs)) != SVO_OK) return rc;
    std::vector<const uint8_t*> lp, rp;
    const uint8_t* l[1] = {left_t1}; const uint8_t* r[1] = {right_t1};
    if ((rc = stage_host_images(c, l, r, stride, lp, rp)) != SVO_OK) return rc;
    const uint8_t** hp = c->ptrs.row(0);                                          // no frame in flight: ring slot 0's rows and record are free
    hp[0] = lp[0]; hp[1] = rp[0];
    const FrameSettings& fs = c->ring[0].fs = c->next;
    if (c->raw_w > 0) {
        const uint8_t** hm = c->maps.row(0);
        for (int cam = 0; cam < 2; cam++) hm[cam] = map_of(c, 0, cam);
        if (!hm[0] || !hm[1]) { g_err = "rectifying context without rectification maps"; return SVO_ERR_STATE; }
    }
    DevBuffers f = frame_view(c, 0, -1);
    const uint8_t* const* srcs = c->ptrs.dev_row(0);
    int packed = in_width(c) * in_bpp(c);
    if (fs.clahe_on && (rc = clahe_front(c, fs, f, srcs, packed, c->stream)) != SVO_OK) return rc;
    launch_ingest_pyramid(f, srcs, packed, c->stream, PYR_T1);                                            // vo.cpp:200-201
    if ((rc = circular_tail(c, n, pl1, pr1, pr0, pl0_circle, ok)) != SVO_OK) return rc;
    SeqState out = keep;
    out.slot_pyr_t0 = t1;                                                         // lastLeftPyramid = pyramidl1 (vo.cpp:231-232)
    rc = set_state(c, out);
    if (rc == SVO_OK) restore.armed = false;
    return rc;
}

extern "C" int svo_set_stage_timing(svo_context* c, int on) {
    if (!c) return fail_arg("null context");
    c->stage_timing = on != 0;
    return SVO_OK;
}

extern "C" int svo_get_last_timing(svo_context* c, float* lk_ms, float* frame_ms) {
    if (!c || c->last.slot < 0) return fail_arg("no frame collected yet");
    HIPCHK(hipSetDevice(c->device));
    const RingSlot& r = c->ring[c->last.slot];
    if (lk_ms) {
        if (!r.staged) { g_err = "no stage events for this frame: call svo_set_stage_timing(ctx, 1) first (and SVO_GRAPH must be off)"; return SVO_ERR_STATE; }
        HIPCHK(hipEventElapsedTime(lk_ms, r.ev[EV_LK0], r.ev[EV_LK1]));
    }
    if (frame_ms) HIPCHK(hipEventElapsedTime(frame_ms, r.ev[EV_F0], r.ev[EV_DONE]));
    return SVO_OK;
}

extern "C" int svo_get_stage_timing(svo_context* c, float ms[5]) {
    if (!c || !ms || c->last.slot < 0) return fail_arg("no frame collected yet");
    HIPCHK(hipSetDevice(c->device));
    const RingSlot& r = c->ring[c->last.slot];
    if (!r.staged) { g_err = "no stage events for this frame: call svo_set_stage_timing(ctx, 1) first (and SVO_GRAPH must be off)"; return SVO_ERR_STATE; }
    for (int i = 0; i + 1 < EV_COUNT; i++) HIPCHK(hipEventElapsedTime(&ms[i], r.ev[i], r.ev[i + 1]));
    return SVO_OK;
}

extern "C" int svo_get_features(svo_context* c, int seq, int cap, float* xy, int* ages, int* strengths) {
    if (!c || seq < 0 || seq >= c->d.B) return fail_arg("bad context / seq");
    SeqState hs; int rc = read_state(c, seq, &hs); if (rc != SVO_OK) return rc;
    int n = hs.n_feat < cap ? hs.n_feat : cap;
    const size_t o = (size_t)seq * c->d.CAP;
    if (n > 0) {
        if (xy) HIPCHK(hipMemcpy(xy, c->d.feat_xy[hs.feat_buf] + o, sizeof(float2) * n, hipMemcpyDeviceToHost));
        if (ages) HIPCHK(hipMemcpy(ages, c->d.feat_age[hs.feat_buf] + o, sizeof(int) * n, hipMemcpyDeviceToHost));
        if (strengths) HIPCHK(hipMemcpy(strengths, c->d.feat_str[hs.feat_buf] + o, sizeof(int) * n, hipMemcpyDeviceToHost));
    }
    return hs.n_feat;
}

extern "C" int svo_get_last_tracks(svo_context* c, int seq, int cap, float* pl0, float* pr0, float* pl1, float* pr1, float* world, uint8_t* inlier) {
    if (!c || seq < 0 || seq >= c->d.B) return fail_arg("bad context / seq");
    SeqState hs; int rc = read_state(c, seq, &hs); if (rc != SVO_OK) return rc;
    int n = hs.n_tracks < cap ? hs.n_tracks : cap;
    const size_t o = (size_t)seq * c->d.CAP;
    if (n > 0) {
        if (pl0) HIPCHK(hipMemcpy(pl0, c->d.tl0 + o, sizeof(float2) * n, hipMemcpyDeviceToHost));
        if (pr0) HIPCHK(hipMemcpy(pr0, c->d.tr0 + o, sizeof(float2) * n, hipMemcpyDeviceToHost));
        if (pl1) HIPCHK(hipMemcpy(pl1, c->d.tl1 + o, sizeof(float2) * n, hipMemcpyDeviceToHost));
        if (pr1) HIPCHK(hipMemcpy(pr1, c->d.tr1 + o, sizeof(float2) * n, hipMemcpyDeviceToHost));
        if (world) HIPCHK(hipMemcpy(world, c->d.world + 3 * o, sizeof(float) * 3 * n, hipMemcpyDeviceToHost));
        if (inlier) HIPCHK(hipMemcpy(inlier, c->d.inlier + o, (size_t)n, hipMemcpyDeviceToHost));
    }
    return hs.n_tracks;
}

// the descriptor ring at the track output's max_rows: allocated at first use, re-allocated when max_rows has changed.  The caller
// has kept the last collected frame's rows (keep_last_obs) if the old ring still held them, and no frame is in flight.
static int desc_ring(svo_context* c) {
    const size_t pitch = (size_t)c->d.B * c->track_rows * SVO_DESC_BYTES;
    if (c->desc.pitch == pitch) return SVO_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    ring_free(c, c->desc);
    HIPCHK(rings_alloc(c, {ring_spec(c->desc, pitch, RING_MAPPED)}));
    return SVO_OK;
}

// ---- track ids and observation rows (svo.h) ----
extern "C" int svo_set_track_output(svo_context* c, int on, int max_rows) {
    if (!c) return fail_arg("null context");
    if (c->inflight != 0) { g_err = "svo_set_track_output with frames in flight: switching is a setup action (collect first)"; return SVO_ERR_STATE; }
    if (!on) { c->next.track_on = false; c->next.desc_on = false; return SVO_OK; }   // the descriptors ride on the track output
    if (c->d.cfg.features_per_bucket > 1) return fail_arg("track ids need features_per_bucket == 1 (the general bucket walk carries no ids)");
    if (max_rows < 1 || max_rows > c->d.CAP) return fail_arg("max_rows must be 1 .. the context's feature capacity");
    HIPCHK(hipSetDevice(c->device));
    const size_t B = c->d.B, CAP = c->d.CAP;
    if (!c->ids.next_id) {                                           // allocated last: next_id marks the set complete
        int rc;
        if ((rc = dev_alloc(c, &c->ids.feat_id[0], B * CAP)) != SVO_OK || (rc = dev_alloc(c, &c->ids.feat_id[1], B * CAP)) != SVO_OK ||
            (rc = dev_alloc(c, &c->ids.track_id, B * CAP)) != SVO_OK || (rc = dev_alloc(c, &c->ids.next_id, B)) != SVO_OK) return rc;
    }
    if (!c->obs.h || c->track_rows != max_rows) {
        if (c->last.obs_slot >= 0) keep_last_obs(c);                 // the last collected frame's rows outlive the ring they were in
        HIPCHK(hipStreamSynchronize(c->stream));
        ring_free(c, c->obs); ring_free(c, c->obs_hdr); c->track_rows = 0;
        HIPCHK(rings_alloc(c, {ring_spec(c->obs, B * (size_t)max_rows, RING_MAPPED), ring_spec(c->obs_hdr, 2 * B, RING_MAPPED)}));
        c->track_rows = max_rows;
        if (c->next.desc_on) if (const int rc = desc_ring(c)) { c->next.desc_on = false; return rc; }   // the descriptor ring follows max_rows
    }
    if (!c->next.track_on) launch_ids_assign(c->d, c->ids, c->stream);     // the features held now: next_id + index
    HIPCHK(hipGetLastError());
    c->next.track_on = true;
    return SVO_OK;
}

extern "C" int svo_get_last_track_obs(svo_context* c, int seq, int cap, svo_track_obs* rows, int* n_tracks) {
    if (!c || seq < 0 || seq >= c->d.B || cap < 0 || (cap > 0 && !rows)) return fail_arg("bad context / seq / cap / rows");
    if (c->last.slot < 0 || !c->last.fs.track_on) { g_err = "the last collected frame was issued with the track output off (or none was collected yet)"; return SVO_ERR_STATE; }
    const LastRows lr = last_rows(c);
    return copy_last_rows(lr, lr.obs, sizeof(svo_track_obs), seq, cap, rows, n_tracks);
}

// ---- binary descriptors (svo.h) ----
extern "C" int svo_set_descriptor_output(svo_context* c, int on) {
    if (!c) return fail_arg("null context");
    if (c->inflight != 0) { g_err = "svo_set_descriptor_output with frames in flight: switching is a setup action (collect first)"; return SVO_ERR_STATE; }
    if (!on) { c->next.desc_on = false; return SVO_OK; }
    if (c->d.CN != 1) return fail_arg("svo_set_descriptor_output: descriptors are defined on a grey image (channels = 1 contexts only)");
    if (c->d.geom.W < 16 || c->d.geom.H < 16) return fail_arg("svo_set_descriptor_output: the image must be at least 16 x 16");
    if (!c->next.track_on) { g_err = "svo_set_descriptor_output with the track output off: a descriptor row describes an observation row (svo_set_track_output first)"; return SVO_ERR_STATE; }
    if (const int rc = desc_ring(c)) return rc;
    c->next.desc_on = true;
    return SVO_OK;
}

extern "C" int svo_get_last_track_descriptors(svo_context* c, int seq, int cap, uint8_t* desc, int* n_tracks) {
    if (!c || seq < 0 || seq >= c->d.B || cap < 0 || (cap > 0 && !desc)) return fail_arg("bad context / seq / cap / desc");
    if (c->last.slot < 0 || !c->last.fs.desc()) { g_err = "the last collected frame was issued with the descriptor output off (or none was collected yet)"; return SVO_ERR_STATE; }
    const LastRows lr = last_rows(c);
    return copy_last_rows(lr, lr.desc, SVO_DESC_BYTES, seq, cap, desc, n_tracks);
}

// the same rows where they lie, for the index's batched insertion (svo_internal.hpp)
int svo_last_rows_view(svo_context* c, SvoLastRowsView* v) {
    if (!c || !v) return fail_arg("bad context");
    *v = SvoLastRowsView{};
    v->B = c->d.B; v->device = c->device;
    const LastFrame& l = c->last;
    v->track_on = l.slot >= 0 && l.fs.track_on; v->desc_on = l.slot >= 0 && l.fs.desc();
    if (!v->desc_on) { g_err = "the last collected frame was issued with the descriptor output off (or none was collected yet)"; return SVO_ERR_STATE; }
    const LastRows lr = last_rows(c);
    v->hdr = lr.hdr; v->obs_h = lr.obs; v->desc_h = lr.desc; v->pitch = lr.pitch;
    v->in_ring = l.obs_slot >= 0;
    if (v->in_ring) { v->obs_m = c->obs.mapped_row(l.obs_slot); v->desc_m = c->desc.mapped_row(l.obs_slot); }
    return SVO_OK;
}

extern "C" int svo_get_feature_ids(svo_context* c, int seq, int cap, int64_t* ids) {
    if (!c || seq < 0 || seq >= c->d.B || cap < 0) return fail_arg("bad context / seq / cap");
    if (!c->next.track_on) { g_err = "svo_get_feature_ids with the track output off"; return SVO_ERR_STATE; }
    SeqState hs; int rc = read_state(c, seq, &hs); if (rc != SVO_OK) return rc;
    const int n = hs.n_feat < cap ? hs.n_feat : cap;
    static_assert(sizeof(long long) == sizeof(int64_t), "ids are 64-bit");
    if (n > 0 && ids) HIPCHK(hipMemcpy(ids, c->ids.feat_id[hs.feat_buf] + (size_t)seq * c->d.CAP, sizeof(int64_t) * n, hipMemcpyDeviceToHost));
    return hs.n_feat;
}

// the slot a diagnostic read-out (svo_get_pyramid, svo_get_derivatives) reads, and its refusals; synchronises the context's stream
static int readable_slot(svo_context* c, int seq, int which, int* slot) {
    if (c->inflight > 0) { g_err = "pyramid read-out with frames in flight (collect first)"; return SVO_ERR_STATE; }
    SeqState hs; int rc = read_state(c, seq, &hs); if (rc != SVO_OK) return rc;
    if (hs.frame_id == 0) { g_err = "the sequence has no frame since its creation or its last reset"; return SVO_ERR_STATE; }
    *slot = which == SVO_PYR_T1 ? hs.slot_t1 : hs.slot_pyr_t0;
    if (*slot < 0 || *slot >= SVO_PYR_SLOTS) { g_err = "no cached lastLeftPyramid yet"; return SVO_ERR_STATE; }
    return SVO_OK;
}

extern "C" int svo_get_pyramid(svo_context* c, int seq, int which, int cam, int plane, int level,
                               uint8_t* out, int64_t cap, int* w, int* h, int* pad, int* n_levels) {
    if (!c || seq < 0 || seq >= c->d.B) return fail_arg("bad context / seq");
    if (which != SVO_PYR_T1 && which != SVO_PYR_LAST_LEFT) return fail_arg("which must be SVO_PYR_T1 or SVO_PYR_LAST_LEFT");
    if (cam < 0 || cam > 1 || plane < 0 || plane >= c->d.CN) return fail_arg("bad camera / plane");
    const Geometry& g = c->d.geom;
    if (level < 0 || level >= g.nlevels) return fail_arg("level out of range");
    const LevelInfo& L = g.lv[level];
    if (w) *w = L.w;
    if (h) *h = L.h;
    if (pad) *pad = g.pad;
    if (n_levels) *n_levels = g.nlevels;
    if (!out) return SVO_OK;
    const size_t pw = (size_t)L.w + 2 * g.pad, ph = (size_t)L.h + 2 * g.pad;
    if (cap < (int64_t)(pw * ph)) return fail_arg("out too small: (h + 2 pad) * (w + 2 pad) bytes needed");
    int slot; const int rc = readable_slot(c, seq, which, &slot); if (rc != SVO_OK) return rc;
    const uint8_t* src = c->d.pyr + pyr_index(c->d, seq, slot, cam) + (size_t)plane * g.pyr_bytes + L.off - (size_t)g.pad * L.stride - g.pad;
    HIPCHK(hipMemcpy2D(out, pw, src, (size_t)L.stride, pw, ph, hipMemcpyDeviceToHost));
    return SVO_OK;
}

extern "C" int svo_get_derivatives(svo_context* c, int seq, int which, int cam, int level,
                                   int16_t* ix, int16_t* iy, int64_t cap, int* w, int* h, int* pad, int* n_levels) {
    if (!c || seq < 0 || seq >= c->d.B) return fail_arg("bad context / seq");
    if (which != SVO_PYR_T1 && which != SVO_PYR_LAST_LEFT) return fail_arg("which must be SVO_PYR_T1 or SVO_PYR_LAST_LEFT");
    if (cam < 0 || cam > 1) return fail_arg("bad camera");
    const Geometry& g = c->d.geom;
    if (pad) *pad = g.pad;
    if (n_levels) *n_levels = g.nlevels;
    if (!c->d.deriv || g.nlevels < 2) { g_err = "no planes: this context keeps no derivative pyramid (its LK kernel differentiates every window itself)"; return SVO_ERR_STATE; }
    if (level < 1 || level >= g.nlevels) return fail_arg("level out of range: the planes cover the levels 1 .. n_levels - 1");
    const LevelInfo& L = g.lv[level];
    if (w) *w = L.w;
    if (h) *h = L.h;
    if (!ix && !iy) return SVO_OK;
    const size_t pw = (size_t)L.w + 2 * g.pad, ph = (size_t)L.h + 2 * g.pad;
    if (cap < (int64_t)(pw * ph)) return fail_arg("arrays too small: (h + 2 pad) * (w + 2 pad) samples each needed");
    int slot; const int rc = readable_slot(c, seq, which, &slot); if (rc != SVO_OK) return rc;
    // sample (-pad, -pad) of the level: the planes are laid out like the image pyramid behind level 0 (svo_internal.hpp)
    const int16_t* src = c->d.deriv + deriv_index(c->d, seq, slot, cam) + (L.off - deriv_origin(g)) - (ptrdiff_t)g.pad * L.stride - g.pad;
    if (ix) HIPCHK(hipMemcpy2D(ix, pw * sizeof(int16_t), src, (size_t)L.stride * sizeof(int16_t), pw * sizeof(int16_t), ph, hipMemcpyDeviceToHost));
    if (iy) HIPCHK(hipMemcpy2D(iy, pw * sizeof(int16_t), src + deriv_samples(g), (size_t)L.stride * sizeof(int16_t), pw * sizeof(int16_t), ph, hipMemcpyDeviceToHost));
    return SVO_OK;
}

// ================================================================================================
// Stage-level entry points
// ================================================================================================
struct DevTmp {                                   // RAII-ish scratch allocations for the stage calls
    std::vector<void*> p;
    ~DevTmp() { for (void* q : p) (void)hipFree(q); }
    template <typename T> hipError_t get(T** out, size_t count) {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, count * sizeof(T) > 0 ? count * sizeof(T) : 16);
        if (e == hipSuccess) { p.push_back(q); *out = (T*)q; }
        return e;
    }
    // allocate and fill from host memory: count elements, or `rows` packed rows of rowb bytes that lie `stride` apart there
    template <typename T> hipError_t put(T** out, const void* host, size_t count) {
        const hipError_t e = get(out, count);
        return e != hipSuccess ? e : hipMemcpy(*out, host, count * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t put_rows(uint8_t** out, const uint8_t* host, size_t rowb, size_t rows, size_t stride) {
        const hipError_t e = get(out, rowb * rows);
        return e != hipSuccess ? e : hipMemcpy2D(*out, rowb, host, stride, rowb, rows, hipMemcpyHostToDevice);
    }
    template <typename T> static hipError_t download(void* host, const T* dev, size_t count) { return hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost); }
};

static int use_device(int device) {
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail_arg("no such HIP device");
    HIPCHK(hipSetDevice(device));
    return SVO_OK;
}

struct CtxGuard { svo_context* c = nullptr; ~CtxGuard() { svo_destroy(c); } };

// The stage entry points need a context's worth of device buffers (pyramid slots, track arrays, RANSAC workspaces).  Creating
// and destroying one per call costs milliseconds of hipMalloc / hipFree, fine for a test and slow for a caller that uses them
// as an API (e.g. calcOpticalFlowPyrLK per frame), so the last one is kept per thread and reused when device, image size and
// configuration match and its capacity suffices.  Every call overwrites the whole sequence record, so nothing leaks from one
// call into the next.  svo_stage_cache_clear() frees it (it is deliberately not freed at thread exit: the HIP runtime may be
// gone by then).
// Every field of svo_config is named exactly once, in one of two lists: the fields that size or shape a context's device
// buffers, and the parameters kernels only read.  A new field belongs in one of them: the size check stops the build until it is
// there.  (Compared field by field, not as bytes: a caller's struct may carry uninitialised padding.)
#define SVO_CFG_SHAPE_FIELDS(X) \
    X(bucket_start_row) X(buckets_along_height) X(buckets_along_width) X(features_per_bucket) X(win_w) X(win_h) X(max_level) X(channels)
#define SVO_CFG_PARAM_FIELDS(X) \
    X(features_threshold) X(pre_matching_feature_threshold) X(age_threshold) X(fast_threshold) X(ransac_reprojection_error) \
    X(ransac_iterations) X(optical_flow_min_eig_threshold) X(circular_matching_success_threshold) X(max_translation_norm) \
    X(max_rotation_norm) X(lk_max_count) X(lk_epsilon) X(ransac_confidence) X(max_features) X(lk_float_sums)
static_assert(sizeof(svo_config) == 112, "svo_config changed: name the new field in SVO_CFG_SHAPE_FIELDS or SVO_CFG_PARAM_FIELDS");
#define SVO_CFG_SAME(field) && a.field == b.field
static bool cfg_same_shape(const svo_config& a, const svo_config& b) { return true SVO_CFG_SHAPE_FIELDS(SVO_CFG_SAME); }
static bool cfg_equal(const svo_config& a, const svo_config& b) { return cfg_same_shape(a, b) SVO_CFG_PARAM_FIELDS(SVO_CFG_SAME); }
#undef SVO_CFG_SAME
// A cached stage context takes a new configuration IN PLACE when only parameters changed (thresholds, iteration counts up to the
// allocated number, confidence, termination criteria, ...): callers that alternate such parameters between calls keep their
// buffers instead of paying a context's worth of hipMalloc / hipFree per call.
static bool stage_reconfigure(svo_context* c, const svo_config& cfg) {
    if (!cfg_same_shape(c->d.cfg, cfg) || cfg.ransac_iterations < 1 || cfg.ransac_iterations > c->k_alloc) return false;
    DevBuffers& d = c->d;
    d.cfg = cfg; d.K = cfg.ransac_iterations;
    derive_from_config(c, cfg);
    c->lk_room = lk_registers_left(d);
    return true;
}
// One cached context per calling thread; the context itself holds the key it was made for (device, image size, capacity, d.cfg).
// The thread_local slot holds the entry for speed; a mutex-protected registry owns the contexts, so that (a) a thread that exits
// hands its context back (its slot's destructor marks the entry free — the context is then REUSED by the next thread that needs
// one of the same shape, or freed by svo_stage_cache_clear_all), and (b) nothing is destroyed from a thread-exit destructor,
// where the HIP runtime may already be gone.  Short-lived worker threads therefore cost at most one context per concurrently
// LIVE thread, not one per thread ever started.
struct StageEntry { svo_context* c = nullptr; bool in_use = false; };
static std::mutex g_stage_mu;
static std::vector<StageEntry*> g_stage_all;
struct StageSlot {
    StageEntry* e = nullptr;
    ~StageSlot() { if (e) { std::lock_guard<std::mutex> lock(g_stage_mu); e->in_use = false; e = nullptr; } }
};
static thread_local StageSlot g_stage_slot;
// can the cached context serve a call on this device, at this image size, with this many points?
static bool stage_fits(const svo_context* c, int device, int w, int h, int cap) {
    return c && c->device == device && c->d.geom.W == w && c->d.geom.H == h && c->d.CAP >= cap;
}
static svo_context*& stage_cache_of_this_thread(int device, int w, int h, int cap) {
    if (!g_stage_slot.e) {
        std::lock_guard<std::mutex> lock(g_stage_mu);
        StageEntry* pick = nullptr;
        for (StageEntry* e : g_stage_all)                              // an orphan that fits first, then any orphan
            if (!e->in_use && stage_fits(e->c, device, w, h, cap)) { pick = e; break; }
        if (!pick) for (StageEntry* e : g_stage_all) if (!e->in_use) { pick = e; break; }
        if (!pick) { pick = new StageEntry(); g_stage_all.push_back(pick); }
        pick->in_use = true;
        g_stage_slot.e = pick;
    }
    return g_stage_slot.e->c;
}
static int stage_ctx(const svo_config& cfg_in, int device, int w, int h, int cap, svo_context** out) {
    svo_config cfg = cfg_in;
    if (cfg.channels == 0) cfg.channels = 1;                          // as ctx_create stores it: d.cfg is what the next call is compared with
    svo_context*& sc = stage_cache_of_this_thread(device, w, h, cap);
    bool keep = false;
    if (stage_fits(sc, device, w, h, cap)) {
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipStreamSynchronize(sc->stream));
        keep = cfg_equal(sc->d.cfg, cfg) || stage_reconfigure(sc, cfg);
    }
    if (!keep) {
        if (sc) { svo_destroy(sc); sc = nullptr; }
        if (const int rc = ctx_create(&cfg, device, 1, w, h, cap, &sc)) return rc;   // (leaves sc null when it fails)
    }
    HIPCHK(choose_pnp_build(sc->d, false));   // a stage context never shares the device with another's LK: lean only under the test knob
    *out = sc;
    return SVO_OK;
}
extern "C" void svo_stage_cache_clear(void) {                       // this thread's cached context
    if (g_stage_slot.e && g_stage_slot.e->c) { svo_destroy(g_stage_slot.e->c); g_stage_slot.e->c = nullptr; }
}
extern "C" int svo_stage_cache_clear_all(void) {                    // every cached context no live call is using (exited threads' too); returns how many were freed
    std::lock_guard<std::mutex> lock(g_stage_mu);
    int freed = 0;
    for (StageEntry* e : g_stage_all)
        if (e->c && (!e->in_use || e == g_stage_slot.e)) { svo_destroy(e->c); e->c = nullptr; freed++; }
    return freed;
}

// Level 0 of (slot, cam) <- a host image.  Rows are packed into pinned memory first: a 2-D copy from pageable memory degenerates
// into per-row transfers (3.5 ms per 1241x376 image), the contiguous pinned copy takes ~20 us.  One pinned buffer per
// (slot, camera), so the copies of one call never overwrite each other before they have run.
static int upload_image(svo_context* c, int slot, int cam, const uint8_t* img, int stride) {
    const size_t W = c->d.geom.W, H = c->d.geom.H;
    if (!c->h_upload) if (const int rc = pinned_alloc(c, &c->h_upload, W * H * 6)) return rc;
    uint8_t* h = c->h_upload + W * H * (size_t)(slot * 2 + cam);
    pack_rows(h, img, W, H, (size_t)stride);
    const LevelInfo& L0 = c->d.geom.lv[0];
    uint8_t* dst = c->d.pyr + pyr_index(c->d, 0, slot, cam) + L0.off;
    HIPCHK(hipMemcpy2DAsync(dst, (size_t)L0.stride, h, W, W, H, hipMemcpyHostToDevice, c->stream));   // from pinned memory: one strided DMA
    return SVO_OK;
}
static int build_pyramid_in_slot(svo_context* c, SeqState& hs, int slot) {
    hs.slot_t1 = slot;
    int rc = set_state(c, hs); if (rc != SVO_OK) return rc;
    launch_pyramid(c->d, c->stream);
    return SVO_OK;
}

extern "C" int svo_fast_score_map(int device, const uint8_t* img, int w, int h, int stride, int threshold, uint8_t* score) {
    if (!img || !score || w < 7 || h < 7 || stride < w) return fail_arg("bad image arguments");
    int rc = use_device(device); if (rc != SVO_OK) return rc;
    DevTmp t; uint8_t *dimg, *dsc;
    HIPCHK(t.put_rows(&dimg, img, w, h, stride)); HIPCHK(t.get(&dsc, (size_t)w * h));
    launch_fast_score_map(dimg, w, h, threshold, dsc, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(t.download(score, dsc, (size_t)w * h));
    return SVO_OK;
}

static int fast_detect_stage(int device, const uint8_t* img, int w, int h, int stride, int threshold, const uint8_t* mask, int mask_stride,
                             int cap, float* xy, float* resp, int* n_out) {
    if (!img || !n_out || w < 7 || h < 7 || stride < w || cap < 0) return fail_arg("bad arguments");
    if (mask && mask_stride < w) return fail_arg("mask_stride < w");
    int rc = use_device(device); if (rc != SVO_OK) return rc;
    DevTmp t; uint8_t *dimg, *dsc, *dmask = nullptr; int *rows, *dn; float2* dxy; float* dresp;
    HIPCHK(t.put_rows(&dimg, img, w, h, stride)); HIPCHK(t.get(&dsc, (size_t)w * h)); HIPCHK(t.get(&rows, (size_t)h));
    HIPCHK(t.get(&dn, 1)); HIPCHK(t.get(&dxy, (size_t)cap)); HIPCHK(t.get(&dresp, (size_t)cap));
    if (mask) HIPCHK(t.put_rows(&dmask, mask, w, h, mask_stride));
    if (mask) launch_fast_score_map_masked(dimg, w, h, threshold, dmask, w, dsc, 0);
    else launch_fast_score_map(dimg, w, h, threshold, dsc, 0);
    launch_score_compact(dsc, w, h, cap, rows, dxy, dresp, dn, 0);
    HIPCHK(hipGetLastError());
    int n = 0;
    HIPCHK(t.download(&n, dn, 1));
    int m = n < cap ? n : cap;
    if (m > 0 && xy) HIPCHK(t.download(xy, dxy, m));
    if (m > 0 && resp) HIPCHK(t.download(resp, dresp, m));
    *n_out = n;
    return SVO_OK;
}
extern "C" int svo_fast_detect(int device, const uint8_t* img, int w, int h, int stride, int threshold,
                               int cap, float* xy, float* resp, int* n_out) {
    return fast_detect_stage(device, img, w, h, stride, threshold, nullptr, 0, cap, xy, resp, n_out);
}
extern "C" int svo_fast_detect_masked(int device, const uint8_t* img, int w, int h, int stride, int threshold,
                                      const uint8_t* mask, int mask_stride, int cap, float* xy, float* resp, int* n_out) {
    if (!mask) return fail_arg("null mask");
    return fast_detect_stage(device, img, w, h, stride, threshold, mask, mask_stride, cap, xy, resp, n_out);
}

extern "C" int svo_bucket_filter(int device, int img_w, int img_h, int* n_io, float* xy, int* ages, int* strengths,
                                 int bah, int baw, int start_row, int per_bucket, int age_thr, int fast_thr) {
    if (!n_io || *n_io < 0 || bah < 1 || baw < 1 || per_bucket < 0 || img_w < 1 || img_h < 1) return fail_arg("bad arguments");
    int n = *n_io;
    if (n > 0 && (!xy || !ages || !strengths)) return fail_arg("null arrays");
    int rc = use_device(device); if (rc != SVO_OK) return rc;
    if (n == 0 || per_bucket == 0) { *n_io = 0; return SVO_OK; }
    const int nb = bah * baw;
    DevTmp t; float2 *dxy, *sxy, *oxy; int *dag, *dst_, *sag, *sst, *sn, *oag, *ost, *dn;
    const size_t outcap = (size_t)n;
    HIPCHK(t.put(&dxy, xy, n)); HIPCHK(t.put(&dag, ages, n)); HIPCHK(t.put(&dst_, strengths, n));
    HIPCHK(t.get(&sxy, (size_t)nb * per_bucket)); HIPCHK(t.get(&sag, (size_t)nb * per_bucket)); HIPCHK(t.get(&sst, (size_t)nb * per_bucket));
    HIPCHK(t.get(&sn, (size_t)nb)); HIPCHK(t.get(&oxy, outcap)); HIPCHK(t.get(&oag, outcap)); HIPCHK(t.get(&ost, outcap)); HIPCHK(t.get(&dn, 1));
    const BucketGrid g = {(img_h + bah - 1) / bah, (img_w + baw - 1) / baw, bah, baw, start_row, age_thr, fast_thr};
    launch_bucket_general(g, per_bucket, n, dxy, dag, dst_, sxy, sag, sst, sn, oxy, oag, ost, dn, 0);
    HIPCHK(hipGetLastError());
    int m = 0;
    HIPCHK(t.download(&m, dn, 1));
    if (m > 0) { HIPCHK(t.download(xy, oxy, m)); HIPCHK(t.download(ages, oag, m)); HIPCHK(t.download(strengths, ost, m)); }
    *n_io = m;
    return SVO_OK;
}

// mask: null (svo_append_features_from_image), or the caller's host mask (svo_append_features_from_image_masked)
static int append_features_stage(int device, const svo_config* cfg_in, const uint8_t* img, int w, int h, int stride, int fast_threshold,
                                 const uint8_t* mask, int mask_stride, int cap, int* n_io, float* xy, int* ages, int* strengths) {
    if (!img || !n_io || *n_io < 0 || stride < w || cap < *n_io) return fail_arg("bad arguments");
    svo_config cfg; if (cfg_in) cfg = *cfg_in; else svo_config_default(&cfg);
    cfg.channels = 1;                                                             // stage entry points are single-channel
    if (mask && mask_stride < w) return fail_arg("mask_stride < w");
    if (mask && cfg.features_per_bucket > 1) return fail_arg("detection masks need features_per_bucket == 1 (the general bucket walk takes none)");
    svo_context* c = nullptr; int rc = stage_ctx(cfg, device, w, h, *n_io, &c); if (rc != SVO_OK) return rc;
    const int n = *n_io;
    if (n > 0) {
        if (!xy || !ages || !strengths) return fail_arg("null arrays");
        HIPCHK(hipMemcpyAsync(c->d.feat_xy[0], xy, sizeof(float2) * n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->d.feat_age[0], ages, sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->d.feat_str[0], strengths, sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
    }
    rc = upload_image(c, 0, 0, img, stride); if (rc != SVO_OK) return rc;
    SeqState hs; memset(&hs, 0, sizeof(hs));
    hs.frame_id = 1; hs.active = 1; hs.slot_img_t0 = 0; hs.slot_pyr_t0 = 0; hs.slot_t1 = 1; hs.n_feat = n; hs.n_old = n; hs.feat_buf = 0;
    rc = set_state(c, hs); if (rc != SVO_OK) return rc;
    // Only detection pass 0 runs here.  When it keeps fewer than pre_matching_feature_threshold features its last emit block
    // offers them to the grid for a pass 1 that this entry point never launches, and the cached context would carry those keys
    // and row counts into the next call (phantom / wrong features): the grid state is cleared per call.
    HIPCHK(hipMemsetAsync(c->d.bucket_keys, 0, sizeof(unsigned long long) * (size_t)c->d.NB, c->stream));
    HIPCHK(hipMemsetAsync(c->d.bucket_rowcnt, 0, sizeof(int) * (size_t)c->d.cfg.buckets_along_height, c->stream));
    HIPCHK(hipMemsetAsync(c->d.emit_ticket, 0, sizeof(int), c->stream));
    DevTmp t;
    if (mask) {
        uint8_t* dmask; const uint8_t** drow;
        HIPCHK(hipStreamSynchronize(c->stream));                                  // the uploads below are synchronous copies on the null stream
        HIPCHK(t.put_rows(&dmask, mask, w, h, mask_stride));
        HIPCHK(t.put(&drow, &dmask, 1));
        launch_detect_masked(c->d, MaskArgs{drow, w}, 0, fast_threshold, c->stream);
    } else launch_detect(c->d, 0, fast_threshold, c->stream);
    HIPCHK(hipGetLastError());
    int m = svo_get_features(c, 0, cap, xy, ages, strengths);                     // synchronises the stream: the scratch mask may go
    if (m < 0) return m;
    *n_io = m;
    g_stage_path = mask ? SVO_PATH_DETECT_MASKED : 0;
    return SVO_OK;
}
extern "C" int svo_append_features_from_image(int device, const svo_config* cfg, const uint8_t* img, int w, int h, int stride,
                                              int fast_threshold, int cap, int* n_io, float* xy, int* ages, int* strengths) {
    return append_features_stage(device, cfg, img, w, h, stride, fast_threshold, nullptr, 0, cap, n_io, xy, ages, strengths);
}
extern "C" int svo_append_features_from_image_masked(int device, const svo_config* cfg, const uint8_t* img, int w, int h, int stride,
                                                     int fast_threshold, const uint8_t* mask, int mask_stride, int cap, int* n_io,
                                                     float* xy, int* ages, int* strengths) {
    if (!mask) return fail_arg("null mask");
    return append_features_stage(device, cfg, img, w, h, stride, fast_threshold, mask, mask_stride, cap, n_io, xy, ages, strengths);
}

extern "C" int svo_build_pyramid(int device, const uint8_t* img, int w, int h, int stride, int win, int max_level,
                                 uint8_t* levels_out, int64_t levels_cap, int* n_levels_out) {
    if (!img || !levels_out || !n_levels_out || stride < w) return fail_arg("bad arguments");
    svo_config cfg; svo_config_default(&cfg);
    cfg.win_w = cfg.win_h = lk_window_supported(win) ? win : 10; cfg.max_level = max_level;
    CtxGuard g; int rc = ctx_create(&cfg, device, 1, w, h, 0, &g.c); if (rc != SVO_OK) return rc;
    svo_context* c = g.c;
    const int pad = c->d.geom.pad;
    make_geometry(c->d.geom, w, h, win, max_level, pad);  // honour the caller's window for the level-stop rule
    // (pyramid buffers were sized with a window >= 7, which never yields fewer bytes than a larger window)
    Geometry chk; make_geometry(chk, w, h, cfg.win_w, max_level, pad);
    if (c->d.geom.pyr_bytes > chk.pyr_bytes) return fail_arg("window too small for this entry point");
    rc = upload_image(c, 0, 0, img, stride); if (rc != SVO_OK) return rc;
    SeqState hs; memset(&hs, 0, sizeof(hs));
    rc = build_pyramid_in_slot(c, hs, 0); if (rc != SVO_OK) return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    int64_t off = 0;
    for (int l = 0; l < c->d.geom.nlevels; l++) {
        const LevelInfo& L = c->d.geom.lv[l];
        int64_t sz = (int64_t)L.w * L.h;
        if (off + sz > levels_cap) return fail_arg("levels_out too small");
        HIPCHK(hipMemcpy2D(levels_out + off, (size_t)L.w, c->d.pyr + pyr_index(c->d, 0, 0, 0) + L.off, (size_t)L.stride, (size_t)L.w, (size_t)L.h, hipMemcpyDeviceToHost));
        off += sz;
    }
    *n_levels_out = c->d.geom.nlevels;
    return SVO_OK;
}

// both forms of the cv::calcOpticalFlowPyrLK-shaped call: guess_pts null is flags = 0, else OPTFLOW_USE_INITIAL_FLOW
static int lk_track_stage(int device, const uint8_t* prev_img, const uint8_t* next_img, int w, int h, int stride,
                          int n, const float* prev_pts, const float* guess_pts, float* next_pts, uint8_t* status,
                          int win, int max_level, int max_count, double epsilon, double min_eig_threshold) {
    if (!prev_img || !next_img || n < 0 || stride < w) return fail_arg("bad arguments");
    if (n > 0 && (!prev_pts || !next_pts || !status)) return fail_arg("null arrays");
    svo_config cfg; svo_config_default(&cfg);
    cfg.win_w = cfg.win_h = win; cfg.max_level = max_level; cfg.lk_max_count = max_count; cfg.lk_epsilon = epsilon;
    cfg.optical_flow_min_eig_threshold = min_eig_threshold;
    svo_context* c = nullptr; int rc = stage_ctx(cfg, device, w, h, n, &c); if (rc != SVO_OK) return rc;
    if (n == 0) return SVO_OK;
    if ((rc = upload_image(c, 0, 0, prev_img, stride)) != SVO_OK) return rc;
    if ((rc = upload_image(c, 1, 0, next_img, stride)) != SVO_OK) return rc;
    SeqState hs; memset(&hs, 0, sizeof(hs));
    if ((rc = build_pyramid_in_slot(c, hs, 0)) != SVO_OK) return rc;
    if ((rc = build_pyramid_in_slot(c, hs, 1)) != SVO_OK) return rc;
    HIPCHK(hipMemcpyAsync(c->d.pl0, prev_pts, sizeof(float2) * n, hipMemcpyHostToDevice, c->stream));
    if (guess_pts) HIPCHK(hipMemcpyAsync(c->d.pr1, guess_pts, sizeof(float2) * n, hipMemcpyHostToDevice, c->stream));   // (pr1: scratch of this call)
    launch_lk_single(c->d, 0, 0, 1, 0, n, c->d.pl0, c->d.pl1, c->d.okmask, c->stream, guess_pts ? c->d.pr1 : nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(next_pts, c->d.pl1, sizeof(float2) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(status, c->d.okmask, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SVO_OK;
}

extern "C" int svo_lk_track(int device, const uint8_t* prev_img, const uint8_t* next_img, int w, int h, int stride,
                            int n, const float* prev_pts, float* next_pts, uint8_t* status,
                            int win, int max_level, int max_count, double epsilon, double min_eig_threshold) {
    return lk_track_stage(device, prev_img, next_img, w, h, stride, n, prev_pts, nullptr, next_pts, status, win, max_level, max_count, epsilon, min_eig_threshold);
}

extern "C" int svo_lk_track_guess(int device, const uint8_t* prev_img, const uint8_t* next_img, int w, int h, int stride,
                                  int n, const float* prev_pts, const float* guess_pts, float* next_pts, uint8_t* status,
                                  int win, int max_level, int max_count, double epsilon, double min_eig_threshold) {
    if (n > 0 && !guess_pts) return fail_arg("null arrays");
    return lk_track_stage(device, prev_img, next_img, w, h, stride, n, prev_pts, n > 0 ? guess_pts : nullptr, next_pts, status, win, max_level, max_count, epsilon,
                          min_eig_threshold);
}

// both forms of the stage call: prior null is svo_circular_match, else the row of svo_circular_match_prior (k_lk_chain_prior)
static int circular_match_stage(int device, const svo_config* cfg_in, const uint8_t* l0, const uint8_t* r0,
                                const uint8_t* l1, const uint8_t* r1, int w, int h, int stride,
                                int n, const float* pl0, const PriorRow* prior, float* pl1, float* pr1, float* pr0, float* pl0_circle, uint8_t* ok) {
    if (!l0 || !r0 || !l1 || !r1 || n < 0 || stride < w) return fail_arg("bad arguments");
    if (n > 0 && (!pl0 || !pl1 || !pr1 || !pr0 || !pl0_circle || !ok)) return fail_arg("null arrays");
    svo_config cfg; if (cfg_in) cfg = *cfg_in; else svo_config_default(&cfg);
    cfg.max_features = 0; cfg.channels = 1;
    if (prior) cfg.lk_float_sums = 0;
    svo_context* c = nullptr; int rc = stage_ctx(cfg, device, w, h, n, &c); if (rc != SVO_OK) return rc;
    if (n == 0) return SVO_OK;                                                    // vo.cpp:179-181
    const PriorRow* drow = nullptr;
    if (prior) {                                                                  // the context's first rows: nothing of it is in flight
        if ((rc = prior_buffers(c)) != SVO_OK) return rc;
        c->prior.row(0)[0] = *prior;
        HIPCHK(c->prior.upload(0, c->stream));
        drow = c->prior.dev_row(0);
    }
    if ((rc = upload_image(c, 0, 0, l0, stride)) != SVO_OK) return rc;
    if ((rc = upload_image(c, 0, 1, r0, stride)) != SVO_OK) return rc;
    if ((rc = upload_image(c, 1, 0, l1, stride)) != SVO_OK) return rc;
    if ((rc = upload_image(c, 1, 1, r1, stride)) != SVO_OK) return rc;
    SeqState hs; memset(&hs, 0, sizeof(hs));
    if ((rc = build_pyramid_in_slot(c, hs, 0)) != SVO_OK) return rc;
    hs.frame_id = 1; hs.active = 1; hs.slot_img_t0 = 0; hs.slot_pyr_t0 = 0; hs.n_feat = n; hs.feat_buf = 0;
    if ((rc = build_pyramid_in_slot(c, hs, 1)) != SVO_OK) return rc;             // leaves slot_t1 = 1
    HIPCHK(hipMemcpyAsync(c->d.feat_xy[0], pl0, sizeof(float2) * n, hipMemcpyHostToDevice, c->stream));
    return circular_tail(c, n, pl1, pr1, pr0, pl0_circle, ok, drow);
}

extern "C" int svo_circular_match(int device, const svo_config* cfg_in, const uint8_t* l0, const uint8_t* r0,
                                  const uint8_t* l1, const uint8_t* r1, int w, int h, int stride,
                                  int n, const float* pl0, float* pl1, float* pr1, float* pr0, float* pl0_circle, uint8_t* ok) {
    return circular_match_stage(device, cfg_in, l0, r0, l1, r1, w, h, stride, n, pl0, nullptr, pl1, pr1, pr0, pl0_circle, ok);
}

extern "C" int svo_circular_match_prior(int device, const svo_config* cfg_in, const uint8_t* l0, const uint8_t* r0,
                                        const uint8_t* l1, const uint8_t* r1, int w, int h, int stride,
                                        int n, const float* pl0, const float H[9], const float Hi[9],
                                        float* pl1, float* pr1, float* pr0, float* pl0_circle, uint8_t* ok) {
    if (!H) return fail_arg("null argument");
    PriorRow row;
    if (const int rc = make_prior_row(H, Hi, &row)) return rc;
    return circular_match_stage(device, cfg_in, l0, r0, l1, r1, w, h, stride, n, pl0, &row, pl1, pr1, pr0, pl0_circle, ok);
}

extern "C" int svo_find_close_points(int device, int n, const float* p1, const float* p2, float threshold, uint8_t* ok) {
    if (n < 0 || (n > 0 && (!p1 || !p2 || !ok))) return fail_arg("bad arguments");
    int rc = use_device(device); if (rc != SVO_OK) return rc;
    if (n == 0) return SVO_OK;
    DevTmp t; float2 *a, *b; uint8_t* o;
    HIPCHK(t.put(&a, p1, n)); HIPCHK(t.put(&b, p2, n)); HIPCHK(t.get(&o, (size_t)n));
    launch_find_close(n, a, b, threshold, o, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(t.download(ok, o, n));
    return SVO_OK;
}

extern "C" int svo_triangulate(int device, const float Pl[12], const float Pr[12], int n, const float* pts_l, const float* pts_r, float* xyz) {
    if (!Pl || !Pr || n < 0 || (n > 0 && (!pts_l || !pts_r || !xyz))) return fail_arg("bad arguments");
    svo_config cfg; svo_config_default(&cfg);
    svo_context* c = nullptr; int rc = stage_ctx(cfg, device, 64, 64, n, &c); if (rc != SVO_OK) return rc;
    if (n == 0) return SVO_OK;
    SeqState hs; memset(&hs, 0, sizeof(hs));
    hs.active = 1; hs.fail_reason = 0; hs.n_tracks = n;
    memcpy(hs.Pl, Pl, sizeof(float) * 12); memcpy(hs.Pr, Pr, sizeof(float) * 12);
    HIPCHK(hipMemcpyAsync(c->d.tl0, pts_l, sizeof(float2) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d.tr0, pts_r, sizeof(float2) * n, hipMemcpyHostToDevice, c->stream));
    if ((rc = set_state(c, hs)) != SVO_OK) return rc;
    launch_triangulate(c->d, c->stream);
    HIPCHK(hipGetLastError());
    g_stage_path = c->d.co_resident ? SVO_PATH_LEAN : 0;
    HIPCHK(hipMemcpyAsync(xyz, c->d.world, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return SVO_OK;
}

// the stage context of a stand-alone RANSAC-PnP over up to cap points: svo_camera_to_world's, and the relocaliser's
static svo_config pnp_stage_config(int ransac_iterations, float reproj_error, float confidence) {
    svo_config cfg; svo_config_default(&cfg);
    cfg.ransac_iterations = ransac_iterations > 1 ? ransac_iterations : 1;
    cfg.ransac_reprojection_error = reproj_error; cfg.ransac_confidence = confidence;
    cfg.features_threshold = 0;                                                  // cameraToWorld itself has no inlier-count gate
    cfg.max_translation_norm = 1e300; cfg.max_rotation_norm = 1e300;             // nor motion gates
    return cfg;
}
static int pnp_stage_ctx(int device, int cap, int ransac_iterations, float reproj_error, float confidence, svo_context** out) {
    return stage_ctx(pnp_stage_config(ransac_iterations, reproj_error, confidence), device, 64, 64, cap, out);
}
// svo_reloc_internal.hpp: the same context for svo_desc_index_localize (svo_match_api.hip), which enqueues on its index's stream
int svo_reloc_stage_ctx(int device, int cap, int ransac_iterations, float reproj_error, float confidence, const DevBuffers** d) {
    svo_context* c = nullptr;
    const int rc = pnp_stage_ctx(device, cap, ransac_iterations, reproj_error, confidence, &c);
    if (rc != SVO_OK) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));   // a context created just now may still be clearing its buffers on its own stream; otherwise idle
    g_stage_path = c->d.co_resident ? SVO_PATH_LEAN : 0;
    *d = &c->d;
    return SVO_OK;
}
// svo_reloc_batch_internal.hpp: the index's own context of n_seq sequences for svo_desc_index_localize_batch, through the same
// configuration.  It takes no part in the device's LK gate: it never runs an LK grid, and a many-sequence context beside it must
// launch what it launches alone.
int svo_reloc_batch_ctx(int device, int n_seq, int cap, int ransac_iterations, float reproj_error, float confidence, svo_context** held,
                        svo_context** outgrown, DevBuffers* d) {
    svo_config cfg = pnp_stage_config(ransac_iterations, reproj_error, confidence);
    if (cfg.channels == 0) cfg.channels = 1;
    svo_context* c = *held;
    *outgrown = nullptr;
    HIPCHK(hipSetDevice(device));
    const bool fits = c && c->d.B >= n_seq && c->d.CAP >= cap;
    if (!fits || !(cfg_equal(c->d.cfg, cfg) || stage_reconfigure(c, cfg))) {
        int seqs = n_seq, room = cap;
        if (c) {                                                                 // what was outgrown at least doubles; the rest stays
            seqs = c->d.B >= n_seq ? c->d.B : std::max(n_seq, 2 * c->d.B);
            room = c->d.CAP >= cap ? c->d.CAP : std::max(cap, 2 * c->d.CAP);
        }
        svo_context* fresh = nullptr;
        if (const int rc = ctx_create(&cfg, device, seqs, 64, 64, room, &fresh)) return rc;
        if (fresh->counted) {
            std::lock_guard<std::mutex> lock(g_lk_gate[device].mu);
            g_lk_gate[device].contexts--; fresh->counted = false;
        }
        HIPCHK(hipStreamSynchronize(fresh->stream));                             // it may still be clearing its buffers on its own stream
        *outgrown = c; *held = c = fresh;
    }
    HIPCHK(choose_pnp_build(c->d, false));
    *d = c->d;
    d->B = n_seq;
    return SVO_OK;
}

extern "C" int svo_camera_to_world(int device, const float K[9], int n, const float* cam_pts, const float* world_pts,
                                   double R[9], double t[3], int* inliers, int* n_inliers, int* success,
                                   int ransac_iterations, float reproj_error, float confidence, int* iters_run) {
    if (!K || !R || !t || !n_inliers || !success || n < 0 || (n > 0 && (!cam_pts || !world_pts))) return fail_arg("bad arguments");
    *n_inliers = 0; *success = 0; if (iters_run) *iters_run = 0;
    if (n < 4) return fail_arg("cameraToWorld needs at least 4 points (cv::solvePnPRansac asserts npoints >= 4)");
    svo_context* c = nullptr; int rc = pnp_stage_ctx(device, n, ransac_iterations, reproj_error, confidence, &c); if (rc != SVO_OK) return rc;
    SeqState hs; memset(&hs, 0, sizeof(hs));
    hs.active = 1; hs.fail_reason = 0; hs.n_tracks = n; hs.n_feat = n; hs.feat_buf = 0;
    memcpy(hs.K, K, sizeof(float) * 9); memcpy(hs.R, R, sizeof(double) * 9); memcpy(hs.t, t, sizeof(double) * 3);
    HIPCHK(hipMemcpyAsync(c->d.tl1, cam_pts, sizeof(float2) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d.world, world_pts, sizeof(float) * 3 * n, hipMemcpyHostToDevice, c->stream));
    if ((rc = set_state(c, hs)) != SVO_OK) return rc;
    if (n == 4) launch_pnp_p3p(c->d, c->stream);                                 // solvepnp.cpp: npoints == 4 -> one direct P3P
    else { launch_pnp_subsets(c->d, c->stream); launch_pnp(c->d, c->stream); }   // n == 5: one direct EPnP (handled on the device)
    HIPCHK(hipGetLastError());
    g_stage_path = n > 4 && c->d.co_resident ? SVO_PATH_LEAN : 0;               // (P3P has one build)
    if ((rc = read_state(c, 0, &hs)) != SVO_OK) return rc;
    if (iters_run) *iters_run = hs.pnp_iters;
    if (hs.pnp_best < 0) return SVO_OK;                                          // success = false: R, t untouched (vo.cpp:307-311)
    memcpy(R, hs.R, sizeof(double) * 9); memcpy(t, hs.t, sizeof(double) * 3);
    *success = 1; *n_inliers = hs.n_inliers;
    if (inliers && hs.n_inliers > 0)
        HIPCHK(hipMemcpy(inliers, c->d.inl_idx, sizeof(int) * hs.n_inliers, hipMemcpyDeviceToHost));
    return SVO_OK;
}

extern "C" int svo_inverse_transform(int device, const double R[9], const double t[3], double T[16]) {
    if (!R || !t || !T) return fail_arg("null argument");
    int rc = use_device(device); if (rc != SVO_OK) return rc;
    DevTmp tmp; double* buf;
    HIPCHK(tmp.get(&buf, 9 + 3 + 16));
    HIPCHK(hipMemcpy(buf, R, sizeof(double) * 9, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(buf + 9, t, sizeof(double) * 3, hipMemcpyHostToDevice));
    launch_inverse_transform(buf, buf + 9, buf + 12, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(tmp.download(T, buf + 12, 16));
    return SVO_OK;
}

// ================================================================================================
// Rectification (svo.h): map generation (host, f64), map installation, and the remap stage entry point
// ================================================================================================
// cv::initUndistortRectifyMap(K, D, R, P[:, :3], (w, h), CV_16SC2, map1, map2) restated as its scalar loop (plumb_bob and
// rational_polynomial; no thin-prism / tilt terms, whose identity forms it reduces to exactly).  The order of every f64 operation
// is OpenCV's: iR = (P33 R)^-1 by the explicit adjugate / determinant (Matx's fast 3x3 inverse), the row start, then the
// column walk by repeated addition.  No FMA contraction anywhere in it (the pragma and the Makefile's -ffp-contract=off), so
// it equals a numpy restatement (tests/rectify_ref.py) bit for bit.
static int rect_round(double v) {                  // cvRound: round half to even; out of range (or NaN) gives INT_MIN, as cvtsd2si does
    const double r = nearbyint(v);
    return (r >= -2147483648.0 && r <= 2147483647.0) ? (int)r : (-2147483647 - 1);
}
extern "C" int svo_init_rectify_map(const double K[9], const double* D, int n_d, const double R[9], const double P[12], int w, int h,
                                    int16_t* map1, uint16_t* map2) {
#pragma clang fp contract(off)
    if (!K || !map1 || !map2 || w < 1 || h < 1) return fail_arg("svo_init_rectify_map: null argument or empty size");
    if (!(n_d == 0 || n_d == 4 || n_d == 5 || n_d == 8) || (n_d > 0 && !D)) return fail_arg("svo_init_rectify_map: n_d must be 0, 4, 5 (plumb_bob) or 8 (rational_polynomial)");
    double k[8] = {0, 0, 0, 0, 0, 0, 0, 0};        // k1 k2 p1 p2 k3 k4 k5 k6
    for (int i = 0; i < n_d; i++) k[i] = D[i];
    const double Rd[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double* Rm = R ? R : Rd;
    double A[9];                                   // P[:, :3] (K when P is NULL) times R, Matx order: ((a0 b0 + a1 b1) + a2 b2)
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double a0 = P ? P[4 * i] : K[3 * i], a1 = P ? P[4 * i + 1] : K[3 * i + 1], a2 = P ? P[4 * i + 2] : K[3 * i + 2];
            A[3 * i + j] = a0 * Rm[j] + a1 * Rm[3 + j] + a2 * Rm[6 + j];
        }
#define a(r, c) A[3 * (r) + (c)]
    double det = a(0, 0) * (a(1, 1) * a(2, 2) - a(2, 1) * a(1, 2)) - a(0, 1) * (a(1, 0) * a(2, 2) - a(2, 0) * a(1, 2)) +
                 a(0, 2) * (a(1, 0) * a(2, 1) - a(2, 0) * a(1, 1));
    if (det == 0.) return fail_arg("svo_init_rectify_map: P[:, :3] * R is singular");
    det = 1. / det;
    const double ir[9] = {
        (a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1)) * det, (a(0, 2) * a(2, 1) - a(0, 1) * a(2, 2)) * det, (a(0, 1) * a(1, 2) - a(0, 2) * a(1, 1)) * det,
        (a(1, 2) * a(2, 0) - a(1, 0) * a(2, 2)) * det, (a(0, 0) * a(2, 2) - a(0, 2) * a(2, 0)) * det, (a(0, 2) * a(1, 0) - a(0, 0) * a(1, 2)) * det,
        (a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0)) * det, (a(0, 1) * a(2, 0) - a(0, 0) * a(2, 1)) * det, (a(0, 0) * a(1, 1) - a(0, 1) * a(1, 0)) * det};
#undef a
    const double fx = K[0], fy = K[4], u0 = K[2], v0 = K[5];
    const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4], k4 = k[5], k5 = k[6], k6 = k[7];
    for (int i = 0; i < h; i++) {
        double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
        int16_t* m1 = map1 + (size_t)i * w * 2;
        uint16_t* m2 = map2 + (size_t)i * w;
        for (int j = 0; j < w; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
            const double ww = 1. / _w, x = _x * ww, y = _y * ww;
            const double x2 = x * x, y2 = y * y;
            const double r2 = x2 + y2, _2xy = 2 * x * y;
            const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
            const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2);
            const double yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy;
            const double u = fx * xd + u0, v = fy * yd + v0;
            const int iu = rect_round(u * 32), iv = rect_round(v * 32);
            m1[2 * j] = (int16_t)(iu >> 5);
            m1[2 * j + 1] = (int16_t)(iv >> 5);
            m2[j] = (uint16_t)((iv & 31) * 32 + (iu & 31));
        }
    }
    return SVO_OK;
}

static int upload_map(svo_context* c, const int16_t* m1, const uint16_t* m2, uint8_t** out) {
    const size_t n = (size_t)c->d.geom.W * c->d.geom.H;
    uint8_t* p = nullptr;
    HIPCHK(hipMalloc((void**)&p, n * 6));
    if (hipMemcpy(p, m1, n * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(p + n * 4, m2, n * 2, hipMemcpyHostToDevice) != hipSuccess) {
        g_err = "svo_set_rectification_maps: map upload failed";
        (void)hipFree(p);
        return SVO_ERR_HIP;
    }
    *out = p;
    return SVO_OK;
}

extern "C" int svo_set_rectification_maps(svo_context* c, int seq, int raw_w, int raw_h, const int16_t* map1_l, const uint16_t* map2_l,
                                          const int16_t* map1_r, const uint16_t* map2_r) {
    if (!c) return fail_arg("null context");
    if (const int rc = seq_range(c, seq)) return rc;
    if (!map1_l || !map2_l || !map1_r || !map2_r) return fail_arg("null map");
    if (raw_w < 1 || raw_h < 1 || raw_w > 32767 || raw_h > 32767) return fail_arg("raw size must be 1 .. 32767");
    if (c->raw_w > 0 && (raw_w != c->raw_w || raw_h != c->raw_h)) return fail_arg("raw size differs from the one this context rectifies (svo_clear_rectification first)");
    HIPCHK(hipSetDevice(c->device));
    uint8_t* m[2] = {nullptr, nullptr};
    int rc = upload_map(c, map1_l, map2_l, &m[0]);
    if (rc == SVO_OK) rc = upload_map(c, map1_r, map2_r, &m[1]);
    if (rc != SVO_OK) { if (m[0]) (void)hipFree(m[0]); return rc; }
    for (int cam = 0; cam < 2; cam++) {
        uint8_t*& slot = seq < 0 ? c->shared_map[cam] : c->own_map[2 * seq + cam];
        retire(c, slot);
        slot = m[cam];
    }
    c->raw_w = c->d.raw_w = raw_w; c->raw_h = c->d.raw_h = raw_h;
    return SVO_OK;
}

extern "C" int svo_set_rectification(svo_context* c, int seq, const svo_camera_info* left, const svo_camera_info* right) {
    if (!c || !left || !right) return fail_arg("null argument");
    if (left->width != right->width || left->height != right->height) return fail_arg("left and right camera_info differ in raw size");
    const size_t n = (size_t)c->d.geom.W * c->d.geom.H;
    std::vector<int16_t> m1[2]; std::vector<uint16_t> m2[2];
    for (int cam = 0; cam < 2; cam++) {
        const svo_camera_info* ci = cam ? right : left;
        m1[cam].resize(2 * n); m2[cam].resize(n);
        const int rc = svo_init_rectify_map(ci->K, ci->D, ci->n_d, ci->R, ci->P, c->d.geom.W, c->d.geom.H, m1[cam].data(), m2[cam].data());
        if (rc != SVO_OK) return rc;
    }
    return svo_set_rectification_maps(c, seq, left->width, left->height, m1[0].data(), m2[0].data(), m1[1].data(), m2[1].data());
}

extern "C" int svo_clear_rectification(svo_context* c) {
    if (!c) return fail_arg("null context");
    HIPCHK(hipSetDevice(c->device));
    for (int cam = 0; cam < 2; cam++) { retire(c, c->shared_map[cam]); c->shared_map[cam] = nullptr; }
    for (uint8_t*& p : c->own_map) { retire(c, p); p = nullptr; }
    c->raw_w = c->raw_h = c->d.raw_w = c->d.raw_h = 0;
    return SVO_OK;
}

extern "C" int svo_rectify_image(int device, const int16_t* map1, const uint16_t* map2, int w, int h, const uint8_t* raw, int raw_w, int raw_h,
                                 int raw_stride, int channels, uint8_t* out) {
    if (!map1 || !map2 || !raw || !out || w < 1 || h < 1 || raw_w < 1 || raw_h < 1) return fail_arg("bad arguments");
    if (channels != 1 && channels != 3) return fail_arg("channels must be 1 or 3");
    if (raw_stride < raw_w * channels) return fail_arg("raw_stride < raw_w * channels");
    int rc = use_device(device); if (rc != SVO_OK) return rc;
    const size_t n = (size_t)w * h, rowb = (size_t)raw_w * channels;
    DevTmp t; short2* dm1; uint16_t* dm2; uint8_t *draw, *dout;
    HIPCHK(t.put(&dm1, map1, n)); HIPCHK(t.put(&dm2, map2, n)); HIPCHK(t.put_rows(&draw, raw, rowb, raw_h, raw_stride)); HIPCHK(t.get(&dout, n * channels));
    launch_rectify_image(dm1, dm2, w, h, draw, raw_w, raw_h, (int)rowb, channels, dout, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(t.download(out, dout, n * channels));
    return SVO_OK;
}

// ================================================================================================
// Input formats (svo.h): the format table, the setter and the conversion stage entry point
// ================================================================================================
// grey = (B 1868 + G 9617 + R 4899 + 8192) >> 14: the one place the weights are written down.  The
// kernels weigh bytes 0, 1, 2 of a pixel with w0, w1, w2, so the byte order of a format is the order of its weights.
static bool grey_in_of(int format, GreyIn* g) {
    const int WB = 1868, WG = 9617, WR = 4899, RND = 8192, SH = 14;
    switch (format) {
        case SVO_INPUT_MONO8: *g = GreyIn{1, 0, 0, 0, 0, 0, 0}; return true;
        case SVO_INPUT_BGR8:  *g = GreyIn{3, WB, WG, WR, RND, SH, 0}; return true;
        case SVO_INPUT_RGB8:  *g = GreyIn{3, WR, WG, WB, RND, SH, 0}; return true;
        case SVO_INPUT_BGRA8: *g = GreyIn{4, WB, WG, WR, RND, SH, 0}; return true;
        case SVO_INPUT_RGBA8: *g = GreyIn{4, WR, WG, WB, RND, SH, 0}; return true;
        case SVO_INPUT_UYVY:  *g = GreyIn{2, 0, 0, 0, 0, 0, 1}; return true;
        case SVO_INPUT_YUY2:  *g = GreyIn{2, 0, 0, 0, 0, 0, 0}; return true;
    }
    return false;
}

extern "C" int svo_set_input_format(svo_context* c, int format) {
    if (!c) return fail_arg("null context");
    if (c->d.CN != 1) return fail_arg("svo_set_input_format: a channels = 3 context takes interleaved BGR as it is (svo.h, channels)");
    GreyIn g;
    if (!grey_in_of(format, &g)) return fail_arg("svo_set_input_format: unknown format (SVO_INPUT_*)");
    c->next.in_format = format; c->next.in = g;
    return SVO_OK;
}

// ================================================================================================
// CLAHE (svo.h): the setter and the stage entry point.  The per-frame side is clahe_front.
// ================================================================================================
extern "C" int svo_set_clahe(svo_context* c, int on, double clip_limit, int tiles_x, int tiles_y) {
    if (!c) return fail_arg("null context");
    if (c->d.CN != 1) return fail_arg("svo_set_clahe: a channels = 3 context takes interleaved BGR as it is (svo.h, channels)");
    if (!on) { c->next.clahe_on = false; return SVO_OK; }
    if (const int rc = check_clahe_params(clip_limit, tiles_x, tiles_y)) return rc;
    int tw, th;
    if (!clahe_geometry(in_width(c), in_height(c), tiles_x, tiles_y, &tw, &th)) return fail_arg("svo_set_clahe: the tiles do not fit the context's input size (svo.h, CLAHE rule 1)");
    c->next.clahe_on = true; c->next.clahe_clip = clip_limit; c->next.clahe_tx = tiles_x; c->next.clahe_ty = tiles_y;
    return SVO_OK;
}

extern "C" int svo_clahe(int device, int format, const uint8_t* src, int w, int h, int stride,
                         double clip_limit, int tiles_x, int tiles_y, uint8_t* out) {
    ClaheArgs a = {};
    if (!src || !out || w < 1 || h < 1) return fail_arg("bad arguments");
    if (!grey_in_of(format, &a.g)) return fail_arg("svo_clahe: unknown format (SVO_INPUT_*)");
    const size_t rowb = (size_t)w * a.g.bpp, n = (size_t)w * h;
    if ((size_t)stride < rowb) return fail_arg("stride < w * bytes per pixel");
    int rc = check_clahe_params(clip_limit, tiles_x, tiles_y); if (rc != SVO_OK) return rc;
    if (!clahe_derive(a, w, h, clip_limit, tiles_x, tiles_y)) return fail_arg("svo_clahe: the tiles do not fit the image (svo.h, CLAHE rule 1)");
    rc = use_device(device); if (rc != SVO_OK) return rc;
    // packed rows on the device, at the caller's own misalignment (as svo_convert_gray)
    const size_t mis = (size_t)((uintptr_t)src & 3);
    DevTmp t; uint8_t *dsrc, *dout, *dlut; const uint8_t** dtab;
    HIPCHK(t.get(&dsrc, rowb * h + 4)); HIPCHK(t.get(&dout, n + 4)); HIPCHK(t.get(&dlut, (size_t)tiles_x * tiles_y * 256));
    HIPCHK(hipMemcpy2D(dsrc + mis, rowb, src, (size_t)stride, rowb, (size_t)h, hipMemcpyHostToDevice));
    const uint8_t* first = dsrc + mis;
    HIPCHK(t.put(&dtab, &first, 1));
    a.srcs = dtab; a.act = nullptr; a.B = 1; a.ncam = 1; a.stride = (int)rowb; a.lut = dlut; a.out = dout; a.pitch = n;
    launch_clahe(a, 1, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(t.download(out, dout, n));
    g_stage_path = SVO_PATH_CLAHE | (a.g.bpp > 1 ? SVO_PATH_INPUT_CONVERTED : 0);
    return SVO_OK;
}

// ================================================================================================
// Pose covariance (svo.h): the setter, the getter and the stage entry point
// ================================================================================================
static int check_cov_mode(int mode, double pixel_sigma, bool off_allowed) {
    if (mode != SVO_COV_RESIDUAL && mode != SVO_COV_FIXED_SIGMA && !(off_allowed && mode == SVO_COV_OFF)) return fail_arg("pose covariance: unknown mode (SVO_COV_*)");
    if (mode == SVO_COV_FIXED_SIGMA && !(pixel_sigma > 0. && isfinite(pixel_sigma))) return fail_arg("pose covariance: pixel_sigma must be positive and finite");
    return SVO_OK;
}

extern "C" int svo_set_pose_covariance(svo_context* c, int mode, double pixel_sigma) {
    if (!c) return fail_arg("null context");
    if (const int rc = check_cov_mode(mode, pixel_sigma, true)) return rc;
    if (mode != SVO_COV_OFF && !c->cov.h) {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(rings_alloc(c, {ring_spec(c->cov, (size_t)c->d.B, RING_MAPPED)}));
        c->last.cov.assign((size_t)c->d.B, PoseCovRow{});
    }
    c->next.cov_mode = mode;
    if (mode == SVO_COV_FIXED_SIGMA) c->next.cov_sigma2 = pixel_sigma * pixel_sigma;
    return SVO_OK;
}

extern "C" int svo_get_last_pose_covariance(svo_context* c, double* cov_T, double* cov_p, int* valid) {
    if (!c) return fail_arg("null context");
    if (c->last.slot < 0 || c->last.fs.cov_mode == SVO_COV_OFF) { g_err = "no covariance: the last collected frame was issued with SVO_COV_OFF, or none was collected"; return SVO_ERR_STATE; }
    for (int i = 0; i < c->d.B; i++) {
        const PoseCovRow& r = c->last.cov[i];
        if (cov_T) memcpy(cov_T + 36 * i, r.cov_T, sizeof(r.cov_T));
        if (cov_p) memcpy(cov_p + 36 * i, r.cov_p, sizeof(r.cov_p));
        if (valid) valid[i] = r.valid;
    }
    return SVO_OK;
}

extern "C" int svo_pose_covariance(int device, const float K[9], int n, const float* cam_pts, const float* world_pts,
                                   const int* inliers, const double R[9], const double t[3],
                                   int mode, double pixel_sigma, double cov_p[36], double cov_T[36], int* valid) {
    if (!K || !R || !t || n < 1 || !cam_pts || !world_pts) return fail_arg("bad arguments");
    int rc = check_cov_mode(mode, pixel_sigma, false); if (rc != SVO_OK) return rc;
    svo_config cfg; svo_config_default(&cfg);
    svo_context* c = nullptr; rc = stage_ctx(cfg, device, 64, 64, n, &c); if (rc != SVO_OK) return rc;
    SeqState hs; memset(&hs, 0, sizeof(hs));
    hs.active = 1; hs.fail_reason = 0; hs.ok = 1; hs.n_tracks = n;
    memcpy(hs.K, K, sizeof(float) * 9); memcpy(hs.R, R, sizeof(double) * 9); memcpy(hs.t, t, sizeof(double) * 3);
    std::vector<uint8_t> in((size_t)n, 1);
    for (int i = 0; inliers && i < n; i++) in[i] = inliers[i] != 0;
    DevTmp tmp; PoseCovRow* row;
    HIPCHK(tmp.get(&row, 1));
    HIPCHK(hipMemcpyAsync(c->d.tl1, cam_pts, sizeof(float2) * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d.world, world_pts, sizeof(float) * 3 * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d.inlier, in.data(), (size_t)n, hipMemcpyHostToDevice, c->stream));
    if ((rc = set_state(c, hs)) != SVO_OK) return rc;
    launch_pose_cov(c->d, CovArgs{row, mode, pixel_sigma * pixel_sigma}, c->stream);
    HIPCHK(hipGetLastError());
    g_stage_path = (c->d.co_resident ? SVO_PATH_LEAN : 0) | SVO_PATH_POSE_COV;
    PoseCovRow h;
    HIPCHK(hipMemcpyAsync(&h, row, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (cov_p) memcpy(cov_p, h.cov_p, sizeof(h.cov_p));
    if (cov_T) memcpy(cov_T, h.cov_T, sizeof(h.cov_T));
    if (valid) *valid = h.valid;
    return SVO_OK;
}

// ---- binary descriptors (svo.h): the stage alone, and the tables ----
extern "C" int svo_describe_points(int device, const uint8_t* img, int w, int h, int stride, int n, const float* xy, uint8_t* desc, int* bins) {
    if (!img || n < 0 || (n > 0 && (!xy || !desc))) return fail_arg("bad arguments");
    if (w < 16 || h < 16) return fail_arg("svo_describe_points: the image must be at least 16 x 16");
    if (stride < w) return fail_arg("stride < w");
    for (int i = 0; i < 2 * n; i++) if (!isfinite(xy[i])) return fail_arg("svo_describe_points: a non-finite coordinate");
    int rc = use_device(device); if (rc != SVO_OK) return rc;
    g_stage_path = SVO_PATH_DESCRIPTORS;
    if (n == 0) return SVO_OK;
    DevTmp t; uint8_t *dimg, *ddesc; float2* dxy; int* dbins;
    HIPCHK(t.put_rows(&dimg, img, (size_t)w, (size_t)h, (size_t)stride));
    HIPCHK(t.put(&dxy, xy, (size_t)n)); HIPCHK(t.get(&ddesc, (size_t)n * SVO_DESC_BYTES)); HIPCHK(t.get(&dbins, (size_t)n));
    launch_describe_points(dimg, w, h, w, dxy, n, ddesc, dbins, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(t.download(desc, ddesc, (size_t)n * SVO_DESC_BYTES));
    if (bins) HIPCHK(t.download(bins, dbins, (size_t)n));
    return SVO_OK;
}

extern "C" int svo_descriptor_pattern(int8_t pattern[1024], int32_t cs[60]) {
    if (!pattern && !cs) return fail_arg("null argument");
    desc_copy_tables(pattern, cs);                                   // svo_kernels_desc.hip: the tables live with the kernels
    return SVO_OK;
}

extern "C" int svo_convert_gray(int device, int format, const uint8_t* src, int w, int h, int stride, uint8_t* out) {
    GreyIn g;
    if (!src || !out || w < 1 || h < 1) return fail_arg("bad arguments");
    if (!grey_in_of(format, &g)) return fail_arg("svo_convert_gray: unknown format (SVO_INPUT_*)");
    const size_t rowb = (size_t)w * g.bpp, n = (size_t)w * h;
    if ((size_t)stride < rowb) return fail_arg("stride < w * bytes per pixel");
    int rc = use_device(device); if (rc != SVO_OK) return rc;
    if (g.bpp == 1) { pack_rows(out, src, rowb, (size_t)h, (size_t)stride); return SVO_OK; }
    // packed rows on the device, at the caller's own misalignment: the kernel's unaligned loads see the addresses mod 4 it was given
    const size_t mis = (size_t)((uintptr_t)src & 3);
    DevTmp t; uint8_t *dsrc, *dout;
    HIPCHK(t.get(&dsrc, rowb * h + 4)); HIPCHK(t.get(&dout, n));
    HIPCHK(hipMemcpy2D(dsrc + mis, rowb, src, (size_t)stride, rowb, (size_t)h, hipMemcpyHostToDevice));
    launch_convert_gray(g, dsrc + mis, w, h, (int)rowb, dout, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(t.download(out, dout, n));
    return SVO_OK;
}

// ================================================================================================
// Detection masks (svo.h): the setter and the getter.  The per-frame side is take_masks / issue_frame.
// ================================================================================================
// first use: the tables every masked frame needs.  All or nothing, so that img_mask.empty() says "no mask was ever set".
static int mask_tables(svo_context* c) {
    if (!c->img_mask.empty()) return SVO_OK;
    const size_t B = (size_t)c->d.B, n = (size_t)c->d.geom.W * c->d.geom.H;
    if (!c->mask_rows.h) HIPCHK(rings_alloc(c, {ring_spec(c->mask_rows, B, RING_UPLOADED)}));
    if (!c->h_mask_stage) if (const int rc = pinned_alloc(c, &c->h_mask_stage, n)) return rc;
    if (!c->ev_mask_stage) HIPCHK(hipEventCreateWithFlags(&c->ev_mask_stage, hipEventDisableTiming));
    c->own_mask.assign(B, MaskPair{});
    c->img_mask.assign(B, nullptr);
    return SVO_OK;
}

extern "C" int svo_set_detection_mask(svo_context* c, int seq, const uint8_t* mask, int stride, int on_device) {
    if (!c) return fail_arg("null context");
    if (c->d.CN != 1) return fail_arg("svo_set_detection_mask: a channels = 3 context runs FAST on the bytes of the interleaved rows, where pixel positions mean nothing");
    if (c->d.cfg.features_per_bucket > 1) return fail_arg("svo_set_detection_mask: detection masks need features_per_bucket == 1 (the general bucket walk takes none)");
    if (const int rc = seq_range(c, seq)) return rc;
    if (!mask) {                                                     // clear: the frames submitted from now on record no mask
        if (seq < 0) { c->shared_mask.cur = -1; for (MaskPair& p : c->own_mask) p.cur = -1; }
        else if (!c->own_mask.empty()) c->own_mask[seq].cur = -1;
        return SVO_OK;
    }
    const int W = c->d.geom.W, H = c->d.geom.H;
    if (stride < W) return fail_arg("svo_set_detection_mask: stride < width");
    HIPCHK(hipSetDevice(c->device));
    if (const int rc = mask_tables(c)) return rc;
    MaskPair& p = seq < 0 ? c->shared_mask : c->own_mask[seq];
    const int t = p.last == 0 ? 1 : 0;                               // not the slot the last frame's left image owns
    if (!p.buf[t]) HIPCHK(hipMalloc((void**)&p.buf[t], (size_t)W * H));
    // on the frame stream, as svo_reset_sequence's kernel: behind the detection of every frame submitted so far (the last of them
    // reads the OTHER slot), before that of every later frame
    if (on_device) HIPCHK(hipMemcpy2DAsync(p.buf[t], (size_t)W, mask, (size_t)stride, (size_t)W, (size_t)H, hipMemcpyDeviceToDevice, c->stream));
    else {
        HIPCHK(hipEventSynchronize(c->ev_mask_stage));               // the previous host mask has left the staging buffer (a fresh event is complete)
        pack_rows(c->h_mask_stage, mask, (size_t)W, (size_t)H, (size_t)stride);
        HIPCHK(hipMemcpyAsync(p.buf[t], c->h_mask_stage, (size_t)W * H, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipEventRecord(c->ev_mask_stage, c->stream));
    }
    p.cur = t;
    return SVO_OK;
}

extern "C" int svo_get_detection_mask(svo_context* c, int seq, uint8_t* out, int* present) {
    if (!c) return fail_arg("null context");
    if (const int rc = seq_range(c, seq)) return rc;
    const MaskPair* p = &c->shared_mask;
    if (seq >= 0 && !c->own_mask.empty() && c->own_mask[seq].cur >= 0) p = &c->own_mask[seq];
    if (present) *present = p->cur >= 0;
    if (p->cur < 0 || !out) return SVO_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, p->buf[p->cur], (size_t)c->d.geom.W * c->d.geom.H, hipMemcpyDeviceToHost));
    return SVO_OK;
}
