// svo_internal.hpp — shared declarations for the HIP translation units of libsvo_hip.so.
// Product code (gfx950 only).  Never includes anything from oracle/.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <stdint.h>
#include "../../include/svo.h"

#define SVO_MAX_LEVELS 8
#define SVO_RING 8            // results ring / max frames in flight
#define SVO_MAX_WIN 31
#define SVO_PYR_SLOTS 4       // T1, imageLeftT0_, lastLeftPyramid (which may be a stale third one, vo.cpp:179-181) + the next frame's, built ahead

// A pyramid level is stored WITH its REFLECT_101 border, as cv::buildOpticalFlowPyramid stores it (withDerivatives = false,
// pyrBorder = BORDER_REFLECT_101): `pad` pixels on every side, rows `stride` bytes apart.  The LK kernel then reads every window
// it may visit (origin in [-win, size), lkpyramid.cpp) with plain loads — no per-byte border arithmetic in its loops.
// off: byte offset of pixel (0, 0) of the level inside one pyramid buffer.
struct LevelInfo { int w, h, off, stride; };
struct Geometry {
    int W, H;
    int nlevels;                              // levels actually built (cv::buildOpticalFlowPyramid stop rule)
    int pad;                                  // border pixels on every side of every level (lk_pad_for(win): covers the widest read of the LK kernel)
    LevelInfo lv[SVO_MAX_LEVELS];
    int pyr_bytes;                            // bytes of one pyramid (all levels with their borders; strides are multiples of 16)
};

// What the LK kernels need of a configuration, derived once on the host (lk_make_crit): the normalised termination criteria, the
// minimum-eigenvalue cut-off (lk_mineig_cut), eps_hi / eps_lo bracketing eps2 for the f32 screening of the convergence test, the
// circular-matching threshold and the image limits as floats.
struct LkCrit { int max_count; double eps2; float mineig_cut; float eps_hi, eps_lo; float thr, Wf, Hf; };

// Device-resident state of one sequence = the members of the reference's VisualOdometry (include/vo.h:233-269).
struct SeqState {
    int frame_id;                             // vo.h:234
    int slot_t1, slot_img_t0, slot_pyr_t0;    // which of the SVO_PYR_SLOTS pyramid slots holds T1 / imageLeftT0_ / lastLeftPyramid
    int slot_next;                            // slot the NEXT frame's pyramids were built in ahead of time (image stream of a many-sequence context), else unused
    int active;                               // this frame runs matching (frame_id > 0 when the frame began)
    int feat_buf;                             // which half of the feature double-buffer is current
    int n_feat;                               // currentVOFeatures.size()
    int n_old;                                // feature count offered to the bucket grid by the current detection pass
    int do_second;                            // second FAST pass at threshold/4 required (vo.cpp:327)
    int n_lk;                                 // points entering circularMatching
    int n_tracks;                             // tracks after circular + bounds compaction
    int n_circ;                               // tracks after circular mask only (vo.cpp:239)
    int fail_reason;
    int pnp_best, pnp_iters, pnp_good;
    int pnp_need;                             // hypotheses that may still be consulted by the adaptive RANSAC loop
    int pnp_drawn;                            // RANSAC subsets drawn so far this frame
    unsigned long long pnp_rng;               // cv::RNG state after them (the later subsets are only drawn if the loop can reach them)
    int n_inliers;
    int ok;
    double R[9], t[3], last_T[16];            // vo.h:266-268
    float Pl[12], Pr[12], K[9];               // vo.h:273, :236
    svo_frame_stats stats;
};

struct FrameResult { double T[16]; int ok; svo_frame_stats stats; };

// One sequence's pose covariance of one frame (svo.h, svo_set_pose_covariance) as k_pose_cov writes it into the pinned ring, and the
// arguments of that launch: the frame's row of the ring (indexed by sequence), the mode the frame was issued with, pixel_sigma^2.
// Kernel arguments of their own, not members of DevBuffers: no other kernel's argument block changes.
struct PoseCovRow { double cov_T[36], cov_p[36]; int valid, pad; };
struct CovArgs { PoseCovRow* rows; int mode; double sigma2; };

// Input format of a frame (svo.h, svo_set_input_format): how a channels == 1 context reads the caller's bytes.  bpp = bytes per
// pixel; bpp <= 1 is mono8 — nothing converts and the plain kernels run.  bpp 3 / 4: grey = (byte0 w0 + byte1 w1 + byte2 w2 + rnd)
// >> shift (byte 3 ignored); bpp 2: grey = byte yoff of the pixel's pair (the Y of YUV 4:2:2).  Scalar kernel arguments: the
// weights live here, on the host's format table (svo_api.hip), and nowhere in the kernels.
struct GreyIn { int bpp, w0, w1, w2, rnd, shift, yoff; };

// CLAHE (svo.h, svo_set_clahe): the arguments of the two launches in front of a frame's ingest (k_clahe_lut, k_clahe_apply), kernel
// arguments of their own like CovArgs.  srcs[cam * B + seq]: the caller's frames in the format g (w x h pixels, rows `stride` bytes
// apart); act: the frame's active list or null (seq_of's rule); lut: [B][ncam][tiles_y][tiles_x][256]; out: the mono8 staging frames,
// image (cam * B + seq) at out + that * pitch, packed rows of w bytes.  tw, th, clip (0: none), scale, inv_tw and inv_th are derived
// once on the host (clahe_geometry, svo_api.hip) as svo.h defines them.
struct ClaheArgs {
    const uint8_t* const* srcs; const int* act; int B, ncam;
    int stride, w, h, tiles_x, tiles_y, tw, th, clip;
    float scale, inv_tw, inv_th;
    uint8_t* lut; uint8_t* out; size_t pitch;
    GreyIn g;
};

// All device buffers of a context (B sequences, capacity CAP features each).
struct DevBuffers {
    int B, CAP, NB;                            // NB = buckets_along_height * buckets_along_width
    int CN;                                    // image channels: 1, or 3 (interleaved BGR in, one pyramid per colour plane inside)
    int K;                                     // ransac_iterations
    Geometry geom;
    svo_config cfg;
    int bucket_h, bucket_w;
    LkCrit lk_crit;                            // LK: lk_make_crit(cfg, geom), recomputed whenever cfg changes
    SeqState* st;                              // [B]
    uint8_t* pyr;                              // [B][SVO_PYR_SLOTS][2 cams][CN planes][pyr_bytes]
    int16_t* deriv;                            // [B][SVO_PYR_SLOTS][2 cams][Ix, Iy][deriv_samples(geom)] the Scharr images of the levels >= 1 (below), or
                                               // nullptr: the context keeps none and the LK kernel differentiates every window itself
    uint8_t* fastimg;                          // CN == 3 only: [B][3 slots][W*H] the first W bytes of every interleaved left row —
                                               // the single-channel 'image' cv::FAST sees in a BGR Mat
    float2* feat_xy[2]; int* feat_age[2]; int* feat_str[2];   // [B][CAP] each, double-buffered
    unsigned long long* bucket_keys;           // [B][NB]
    int* bucket_rowcnt;                        // [B][buckets_along_height] occupied buckets per grid row (counted at first fill)
    int* emit_ticket;                          // [B] blocks of k_bucket_emit that have finished; keys, row counts and tickets are all zero between passes
    int co_resident;                           // several many-sequence contexts share this device: launch the 96-register builds
    // features_per_bucket > 1 only (the general Bucket::add_feature walk; the default capacity 1 is an argmax and needs none of it):
    int KPCAP;                                 // candidate capacity per sequence = CAP (existing tracks) + keypoints one FAST pass can return
    uint8_t* score;                            // [B][W*H] NMS-surviving FAST scores of the pass
    int* kp_rows;                              // [B][H] keypoints per image row -> exclusive offsets
    float2* cand_xy; int* cand_age; int* cand_str;   // [B][KPCAP] the pass's input in the reference's order: tracks, then keypoints in raster order
    int* n_cand;                               // [B]
    float2* slot_xy; int* slot_age; int* slot_str;   // [B][NB][features_per_bucket]
    int* slot_n;                               // [B][NB]
    float2 *pl0, *pl1, *pr1, *pr0, *plc;       // [B][CAP] raw LK outputs
    uint8_t* okmask;                           // [B][CAP] bit0 circular ok, bit1 in-bounds
    unsigned* lk_work;                         // [B][CAP] per feature: Newton steps << 8 | (1 + first pass with status 0, or 0) << 6 | level visits (summed by k_compact)
    float2 *tl0, *tr0, *tl1, *tr1;             // [B][CAP] compacted tracks
    float* world;                              // [B][CAP][3]
    uint8_t* inlier;                           // [B][CAP]
    int* subsets;                              // [B][K][5]
    double* hyp;                               // [B][K][12]  (R row-major, t)
    int* hyp_good;                             // [B][K]
    int* inl_idx;                              // [B][CAP]
    double ransac_log_num;                     // log(max(1 - confidence, DBL_MIN)): the numerator of RANSACUpdateNumIters, computed by the host
    const double* lm_lambda;                   // [33] 10^k, k = -16..16 (the damping factors CvLevMarq can reach), computed on the host
    FrameResult* results;                      // [SVO_RING][B]
    const uint8_t** img_ptrs;                  // [SVO_RING][2][B] source image pointers: pinned host memory, read in place
    // Ragged frames (svo_*_batch_masked): act[0 .. n_act) lists the sequences that take the frame, act[B + seq] is the flag of every
    // sequence (k_frame_end writes the idle rows from it) — the frame's row of a device [SVO_RING][2 B] buffer.  nullptr: every
    // sequence takes it, and the grids are those of the unmasked calls.
    const int* act; int n_act;
    // Rectifying contexts (svo_set_rectification_maps): frames are RAW images of raw_w x raw_h pixels; level 0 and the FAST image
    // are their remap through each frame's own maps.  rmap = the frame's row of a pinned [SVO_RING][2][B] table of map pointers
    // (a map = [W*H] short2 integer positions, then [W*H] u16 fractions: OpenCV's CV_16SC2 + CV_16UC1 pair), set for the launches
    // of one frame only, like act.  nullptr: the caller's images are level 0 as they stand, and the plain kernels run.
    const uint8_t* const* rmap; int raw_w, raw_h;
    // Converting contexts (svo_set_input_format): the format of the frame being ingested, set for the launches of one frame only,
    // like rmap.  in.bpp <= 1: the caller's bytes are grey as they stand, and the plain kernels run.
    GreyIn in;
};

// The sequence of the b-th sequence slot of a launch (a block coordinate or a thread index): every per-sequence kernel maps its
// sequence through this, and every grid's sequence dimension is launch_seqs() long.
__device__ __forceinline__ int seq_of(const DevBuffers& d, int b) { return d.act ? d.act[b] : b; }
__host__ __device__ inline int launch_seqs(const DevBuffers& d) { return d.act ? d.n_act : d.B; }

// plane 0 of the pyramid of (sequence, slot, camera); plane k follows at + k * geom.pyr_bytes
__host__ __device__ inline size_t pyr_index(const DevBuffers& d, int seq, int slot, int cam) {
    return ((size_t)(seq * SVO_PYR_SLOTS + slot) * 2 + cam) * (size_t)d.CN * (size_t)d.geom.pyr_bytes;
}
// ---- the derivative pyramid of the levels >= 1 (many-sequence grey contexts in the exact-sums mode; k_deriv_levels writes it, lk_pass
// reads it).  What cv::buildOpticalFlowPyramid keeps with withDerivatives = true, for the coarse levels only: level 0 holds three
// quarters of a pyramid's pixels and a quarter of the LK level visits, the levels above it the reverse.
// A plane (Ix or Iy) is laid out like the part of an image pyramid behind level 0, one int16 sample per pixel: sample (x, y) of level
// l >= 1 sits at int16 index lv[l].off - deriv_origin(g) + y * lv[l].stride + x, so the level table addresses it and the image's
// border (pad >= EXT + 5 on every side) is the derivative's too: wide enough for every window origin in reach ([-W, size) per axis),
// the window plus one sample and one sample of over-read.  A sample is 4 x the Scharr value of the PADDED level (the reflected pixels
// at the edge) — the integer lk_pass computes in registers — inside the level, and zero outside it (derivBorder = BORDER_CONSTANT):
// the buffer is cleared when it is allocated and only the samples inside the levels are ever written.  Row starts and plane bases
// are multiples of 32 bytes.  The planes of (sequence, slot, camera) belong to the pyramid of the same index, whatever the slot rule does.
__host__ __device__ inline int deriv_origin(const Geometry& g) { return g.lv[0].stride * (g.lv[0].h + 2 * g.pad); }   // bytes of level 0 with its border
__host__ __device__ inline int deriv_samples(const Geometry& g) { return g.pyr_bytes - deriv_origin(g); }            // int16 samples of one plane
__host__ __device__ inline size_t deriv_index(const DevBuffers& d, int seq, int slot, int cam) {                      // the Ix plane; Iy follows at + deriv_samples
    return ((size_t)(seq * SVO_PYR_SLOTS + slot) * 2 + cam) * 2 * (size_t)deriv_samples(d.geom);
}
__host__ __device__ inline size_t fastimg_index(const DevBuffers& d, int seq, int slot) {
    return (size_t)(seq * SVO_PYR_SLOTS + slot) * (size_t)d.geom.W * (size_t)d.geom.H;
}

// ---- the bucket grid of FeatureSet::filterByBucketLocationInternal: its rules, each written once.  The frame pipeline takes the
// grid from its context (grid_of), the stage call svo_bucket_filter fills one on the host. ----
struct BucketGrid { int bucket_h, bucket_w, bah, baw, start_row, age_thr, fast_thr; };   // bucket size in pixels: ceil(image / buckets), feature_set.cpp:91-93, 103-104
__device__ __forceinline__ BucketGrid grid_of(const DevBuffers& d) {
    return {d.bucket_h, d.bucket_w, d.cfg.buckets_along_height, d.cfg.buckets_along_width, d.cfg.bucket_start_row, d.cfg.age_threshold, d.cfg.fast_threshold};
}
// The bucket (bh, bw) of a point (feature_set.cpp:122-123: f32 division, truncated toward zero), and whether the grid takes it.
// The INDEX decides: a coordinate in (-bucket, 0) truncates to 0 and is inside, rows before start_row have no capacity (:113-116).
__device__ __forceinline__ bool bucket_of(const BucketGrid& g, float x, float y, int& bh, int& bw) {
    bh = (int)(y / (float)g.bucket_h); bw = (int)(x / (float)g.bucket_w);
    return bh >= 0 && bw >= 0 && bh >= g.start_row && bh < g.bah && bw < g.baw;
}
// Detection masks (svo.h, svo_set_detection_mask): does the mask (W x H bytes, rows `stride` apart, non-zero = features allowed) keep an
// entry of the list appendFeaturesFromImage hands to the grid?  KeyPointsFilter::runByPixelsMask's rule, written once: the byte at the
// rounded position ((int)(v + 0.5f), truncation toward zero), clamped into the image (the lower clamp only guards the load: the
// frame pipeline's tracks are never negative, vo.cpp:341-359).  Both call sites — the FAST tile's sink and the track offer — use it.
__host__ __device__ inline bool mask_keeps(const uint8_t* mask, int stride, int W, int H, float x, float y) {
    int ix = (int)(x + 0.5f), iy = (int)(y + 0.5f);
    ix = ix < W - 1 ? ix : W - 1; iy = iy < H - 1 ? iy : H - 1;
    ix = ix > 0 ? ix : 0; iy = iy > 0 ? iy : 0;
    return mask[(size_t)iy * (size_t)stride + ix] != 0;
}
// The masks of one detection launch: rows[seq] = the mask of the left image sequence seq's detection scans (library-owned device
// memory), or null: everything allowed there.  Kernel arguments of their own, like CovArgs: no existing kernel's argument block changes.
struct MaskArgs { const uint8_t* const* rows; int stride; };
// Track ids and per-frame observation rows (svo.h, svo_set_track_output).  The ids live in buffers of their own and travel in an
// argument struct of their own, like MaskArgs: DevBuffers, SeqState and every existing kernel's argument block stay as they are.
// feat_id[k]: [B][CAP] the ids of the feature double-buffer's half k (SeqState::feat_buf picks the current one, as for feat_xy);
// track_id: [B][CAP] the ids of the compacted tracks; next_id: [B] the sequence's counter (svo.h, the identity rule).
struct IdArgs { long long* feat_id[2]; long long* track_id; long long* next_id; };
// One frame's rows of the pinned observation ring: rows [B][max_rows], hdr [B] {n_tracks, n_rows} — host memory mapped into the
// device, written in place by k_track_obs like the result records.
struct TrackObsArgs { svo_track_obs* rows; int* hdr; int max_rows; };
// One frame's rows of the pinned descriptor ring (svo.h, svo_set_descriptor_output): rows [B][max_rows][32] bytes, host memory mapped
// into the device, written in place by k_track_desc.  Row i describes observation row i; the row count is k_track_obs's own
// (min(n_tracks, max_rows) of an active sequence), taken from SeqState as that kernel takes it.  Arguments of their own, again.
struct DescArgs { uint8_t* rows; int max_rows; };
// Motion priors (svo.h, svo_set_motion_prior): PriorRow, one sequence's row of a frame's priors, lives in svo_prior.hpp beside the
// arithmetic that fills it, where a host compiler can read it too.
#include "svo_prior.hpp"
// what Bucket::add_feature compares (feature_set.cpp:16-18); the division truncates toward zero, as C's does
__device__ __forceinline__ int bucket_score(int age, int strength, int fast_thr) { return age + (strength - fast_thr) / 20; }
// capacity 1: (score, first come, strength) as one key for a 64-bit atomicMax; order = the candidate's rank in the input list
__device__ __forceinline__ unsigned long long make_bucket_key(int score, unsigned order, int strength) {
    int s = score + 32768; s = s < 1 ? 1 : (s > 65535 ? 65535 : s);
    return ((unsigned long long)s << 48) | ((unsigned long long)(0xFFFFFFFFu - order) << 16) | (unsigned long long)(strength & 0xFFFF);
}

// Hypotheses of the first RANSAC chunk (always solved). 16 when many sequences share the GPU; 32 for a lone stream: the GPU is
// empty then, a wider chunk costs no time, and the adaptive loop (11-27 iterations with 30 % outliers) rarely needs a second
// EPnP launch — which would be another 145 us on the critical path.
#define SVO_LONE_MAX_SEQ 8      // contexts of up to this many sequences are tuned for latency (wider first RANSAC chunk, 16 lanes per hypothesis ...)
#define SVO_MAX_DEVICES 64
__host__ __device__ inline int pnp_first_chunk(const DevBuffers& d) { const int c = d.B <= SVO_LONE_MAX_SEQ ? 32 : 16; return d.K < c ? d.K : c; }

// ---- the pyramid slot rule: which of a sequence's SVO_PYR_SLOTS slots a set of pyramids is built in ----
//   PYR_T1     the T1 slot as it stands (stage entry points; every kernel that follows a frame's reset)
//   PYR_BEGIN  the frame pipeline's own ingest: the free slot, and the ingest also runs the per-frame reset, which names it T1
//   PYR_NEXT   ahead of the frame (image stream): SeqState::slot_next, which k_pick_next chose; nothing of the state is written
enum PyrTarget { PYR_T1, PYR_BEGIN, PYR_NEXT };
// the slot neither cached member refers to: a function of two fields the per-frame reset does not write, so every block of the
// ingest that runs the reset derives it for itself
__host__ __device__ inline int free_slot(const SeqState& s) {
    int t1 = 0;
    for (int c = 0; c < 3; c++) if (c != s.slot_img_t0 && c != s.slot_pyr_t0) { t1 = c; break; }
    return t1;
}
// the slot no field refers to while a frame is in flight: where the NEXT frame's pyramids can be built ahead of time.  Read at any
// moment of the current frame (even while k_frame_end rewrites the fields: the set in use only shrinks there) it is free.
__host__ __device__ inline int next_slot(const SeqState& s) {
    const int a = s.slot_img_t0, b = s.slot_pyr_t0, t = s.slot_t1;
    for (int c = 0; c < SVO_PYR_SLOTS; c++) if (c != a && c != b && c != t) return c;
    return 0;
}
__host__ __device__ inline int pyr_slot(const SeqState& s, PyrTarget target) {
    return target == PYR_NEXT ? s.slot_next : target == PYR_BEGIN ? free_slot(s) : s.slot_t1;
}

// ---- launchers (each enqueues on `s`; none synchronises) ----
void launch_pyramid(const DevBuffers& d, hipStream_t s);                 // levels 1.. of the T1 slot from its level 0, then the borders of all levels
int lk_pad_for(int win);                                                 // border width the LK kernel's reads need at this window (svo_kernels_lk.hip)
// Ingest + every pyramid level + the borders, into the target's slot.  PYR_NEXT is the NEXT frame's, on another stream, while the
// current frame is still being processed (single-channel contexts with >= 2 levels: ingest_ahead_applies): k_pick_next names the
// slot first, and launch_frame_begin (on the frame's own stream, after that work) then performs the per-frame reset with it as T1.
void launch_ingest_pyramid(const DevBuffers& d, const uint8_t* const* left_right_dev_ptrs /* [2][B] device-readable array */, int stride_bytes, hipStream_t s,
                           PyrTarget target);
bool ingest_ahead_applies(const DevBuffers& d);
void launch_frame_begin(const DevBuffers& d, hipStream_t s);
// svo_reset_sequence (seq = -1: all): the constructor's fields, and the projection when `set`; stream-ordered, no host sync
struct SeqProjection { float Pl[12], Pr[12]; int set; };
void launch_reset_seq(const DevBuffers& d, int seq, const SeqProjection& p, hipStream_t s);
void launch_detect(const DevBuffers& d, int pass, int th_override, hipStream_t s);   // pass 0: FAST_THRESHOLD, pass 1: /4 if needed; th_override >= 0 replaces it
// the same pass with detection masks (features_per_bucket == 1 only): k_fast_masked / k_fast_strided_masked, then the plain emit
void launch_detect_masked(const DevBuffers& d, const MaskArgs& m, int pass, int th_override, hipStream_t s);
// grid_n = max features that can enter LK; early_out: a feature stops at its first pass with status 0 (frame pipeline) or runs all four (member call)
// prior: the frame's rows of motion priors (device, [B]) — k_lk_chain_prior then runs in k_lk_chain's place — or null
bool launch_lk_chain(const DevBuffers& d, int grid_n, hipStream_t s, int early_out, const PriorRow* prior = nullptr);   // false: no kernel built for this (window, channels, summation mode) — nothing ran
// SVO_PRIOR_LAST_ROTATION: k_prior_predict (svo_kernels_prior.hip) over the n sequences listed in act (mapped host memory; null:
// sequences 0 .. n-1), first thing on the frame's stream.  rows / host_rows: the frame's device row and its row of the pinned ring;
// uploaded: explicit priors were copied into `rows` in front of it
void launch_prior_predict(const DevBuffers& d, const int* act, int n, bool uploaded, PriorRow* rows, PriorRow* host_rows, hipStream_t s);
void launch_compact(const DevBuffers& d, hipStream_t s);
void launch_triangulate(const DevBuffers& d, hipStream_t s);
void launch_pnp(const DevBuffers& d, hipStream_t s, bool first_chunk_solved = false);   // expects the subsets drawn (launch_triangulate / k_compact do it)
hipError_t prepare_pnp_lean();   // before the first launch_pnp with co_resident on the current device (the lean EPnP's dynamic LDS)
bool launch_triangulate_epnp_fused(const DevBuffers& d, hipStream_t s);   // lone stream: triangulation || first EPnP chunk in one launch; false = not applicable
void launch_pnp_subsets(const DevBuffers& d, hipStream_t s);
void launch_pose_cov(const DevBuffers& d, const CovArgs& a, hipStream_t s);   // after launch_pnp: the covariance of the refined pose, one block per launched sequence
// ---- track ids (svo_set_track_output; features_per_bucket == 1 only) ----
// a detection pass that carries ids: the pass's FAST kernel (masked when m is given), then the ids build of the emit
void launch_detect_ids(const DevBuffers& d, const IdArgs& ia, const MaskArgs* m, int pass, int th_override, hipStream_t s);
void launch_ids_compact(const DevBuffers& d, const IdArgs& ia, hipStream_t s);     // behind launch_compact: the ids through its stable ranks
// behind launch_pnp, before launch_frame_end: the inlier compaction's id move, then the frame's header and rows into the pinned ring
void launch_track_obs(const DevBuffers& d, const IdArgs& ia, const TrackObsArgs& oa, hipStream_t s);
// ---- binary descriptors (svo_set_descriptor_output; svo_kernels_desc.hip) ----
// behind launch_track_obs, before launch_frame_end: the descriptor of every observation row, into the frame's rows of the pinned ring
void launch_track_desc(const DevBuffers& d, const DescArgs& a, hipStream_t s);
// svo_describe_points: n points of a plain image (device pointers; bins may be null); n <= 0 launches nothing
void launch_describe_points(const uint8_t* img, int w, int h, int stride, const float2* xy, int n, uint8_t* desc, int* bins, hipStream_t s);
void desc_copy_tables(int8_t* pattern /* [1024] or null */, int32_t* cs /* [60]: cos, then sin; or null */);   // svo_descriptor_pattern; host only
void launch_ids_assign(const DevBuffers& d, const IdArgs& ia, hipStream_t s);      // switching on: held features get next_id + index
void launch_ids_reset(const IdArgs& ia, int seq0, int n, hipStream_t s);           // svo_reset_sequence: next_id = 0
void launch_pnp_p3p(const DevBuffers& d, hipStream_t s);                // exactly four points: one P3P, no RANSAC (stage API only)
void launch_inverse_transform(const double* R, const double* t, double* T, hipStream_t s);   // device pointers
// the front of a lone stream's frame as two fused launches (ingest + level 1 || FAST pass 0; levels 2-3 || emit), then the second
// detection pass; false = not applicable to this context, nothing was launched
bool launch_front_fused(const DevBuffers& d, const uint8_t* const* left_right_dev_ptrs, int stride, hipStream_t s);
void launch_frame_end(const DevBuffers& d, int ring_slot, hipStream_t s);
// svo_rectify_image: out (w x h x cn, packed) = the remap of raw through (map1, map2); all device pointers
void launch_rectify_image(const short2* map1, const uint16_t* map2, int w, int h, const uint8_t* raw, int raw_w, int raw_h, int raw_stride,
                          int cn, uint8_t* out, hipStream_t s);

// svo_convert_gray: out (w x h, packed) = the grey image of src in the format g; device pointers
void launch_convert_gray(const GreyIn& g, const uint8_t* src, int w, int h, int stride, uint8_t* out, hipStream_t s);

// CLAHE: the per-tile LUTs, then the interpolation into the staging frames, for n_seq launched sequences (a.act lists them, or null)
void launch_clahe(const ClaheArgs& a, int n_seq, hipStream_t s);

// stage helpers
void launch_fast_score_map(const uint8_t* img_dev, int w, int h, int threshold, uint8_t* score_dev, hipStream_t s);
// the score map of the keypoints a mask keeps (the mask applied to the NMS survivors): svo_fast_detect_masked
void launch_fast_score_map_masked(const uint8_t* img_dev, int w, int h, int threshold, const uint8_t* mask_dev, int mask_stride, uint8_t* score_dev, hipStream_t s);
void launch_score_compact(const uint8_t* score_dev, int w, int h, int cap, int* row_counts_dev, float2* xy_dev, float* resp_dev, int* n_dev, hipStream_t s);
void launch_bucket_general(const BucketGrid& g, int per_bucket, int n, const float2* xy, const int* ages, const int* strs,
                           float2* slot_xy, int* slot_age, int* slot_str, int* slot_n,
                           float2* out_xy, int* out_age, int* out_str, int* n_out, hipStream_t s);
// guess: the points the top level's search starts at (k_lk_single_guess), or null: the points themselves (k_lk_single)
void launch_lk_single(const DevBuffers& d, int slotA, int camA, int slotB, int camB, int n, const float2* prev, float2* next,
                      uint8_t* status, hipStream_t s, const float2* guess = nullptr);
void launch_find_close(int n, const float2* a, const float2* b, float thr, uint8_t* ok, hipStream_t s);
bool lk_window_supported(int win);
int lk_registers_left(const DevBuffers& d);   // VGPRs per SIMD lane beside a full set of this context's LK waves (-1: unknown)
bool lk_window_supported_cn(int win, int cn);
float lk_mineig_cut(int win, double min_eig_threshold);
LkCrit lk_make_crit(const svo_config& cfg, const Geometry& g);

// ------------------------------------------------------------------------------------------------ subsets (cv::RNG, getSubset)
// All K 5-subsets of one sequence, drawn with cv::RNG's multiply-with-carry recurrence from the seed (uint64)-1; the number
// of draws never depends on model quality.  The first SVO_RNG_TABLE_N states of that stream are tabulated (svo_rng_table.hpp).
#include "svo_rng_table.hpp"
#define SVO_RNG_SEED 0xFFFFFFFFFFFFFFFFull                               // RNG rng((uint64)-1)
// uniform(0, n) = next() % n of a raw draw x: the remainder is taken through the 64-bit reciprocal ceil(2^64 / n) (exact for 32-bit
// operands: the error term x e / (n 2^64) stays below 2^-32 < 1/n), 6 instructions instead of the 32-bit division sequence.
static __device__ __forceinline__ unsigned long long pnp_recip(unsigned n) { return 0xFFFFFFFFFFFFFFFFull / n + 1ull; }
static __device__ __forceinline__ int pnp_uniform(unsigned x, unsigned n, unsigned long long recip) {
    return (int)(x - (unsigned)__umul64hi((unsigned long long)x, recip) * n);
}
// One getSubset: five distinct indices, each redrawn while it repeats an earlier one.  A raw draw is the next step of the
// recurrence — or, for a caller that knows how many draws t were made since the seed (TABLE), a table entry while the table lasts.
template <bool TABLE>
static __device__ inline void pnp_draw_subset(unsigned long long& state, int& t, unsigned n, unsigned long long recip, int* out) {
    int idx[5];
    for (int i = 0; i < 5; i++) {
        int v; bool dup;
        do {
            state = TABLE && t < SVO_RNG_TABLE_N ? SVO_RNG_STATES[t] : (unsigned long long)(unsigned)state * 4164903690ull + (unsigned)(state >> 32);
            t++;
            v = pnp_uniform((unsigned)state, n, recip);
            dup = false;
            for (int k = 0; k < i; k++) dup |= (idx[k] == v);
        } while (dup);
        idx[i] = v;
    }
    for (int i = 0; i < 5; i++) out[i] = idx[i];
}
// Draws subsets [s.pnp_drawn, upto) and leaves the generator state in s.pnp_rng: the first chunk is drawn beside the
// triangulation, the rest only as far as the adaptive loop can still reach (k_pnp_decide) — with a static scene that is never.
static __device__ inline void pnp_draw_subsets(const DevBuffers& d, SeqState& s, int seq, int upto) {
    const unsigned n = (unsigned)s.n_tracks;
    if (n < 2) return;
    if (upto > d.K) upto = d.K;
    int* out = d.subsets + (size_t)seq * d.K * 5;
    if (n == 5) {                                                    // model_points == npoints: one direct solve on all five (solvepnp.cpp)
        for (int i = 0; i < 5; i++) out[i] = i;
        s.pnp_drawn = d.K;
        return;
    }
    unsigned long long state = s.pnp_drawn == 0 ? SVO_RNG_SEED : s.pnp_rng;
    const unsigned long long recip = pnp_recip(n);
    int t = 0;                                                       // (the position in the stream is not kept between calls)
    for (int it = s.pnp_drawn; it < upto; it++) pnp_draw_subset<false>(state, t, n, recip, out + it * 5);
    if (upto > s.pnp_drawn) s.pnp_drawn = upto;
    s.pnp_rng = state;
}

// The first chunk of a lone stream, drawn by the 64 lanes of ONE wave (k_compact's first) from the table: lane h takes subset h at
// its no-duplicate position (raw draws 5h .. 5h+4), which is right for every subset up to the first one that meets a duplicate
// (getSubset redraws and the stream shifts); from that subset on lane 0 walks the stream serially, as pnp_draw_subsets does.  Same
// subsets, same generator state afterwards.  With ~900 tracks no subset of the 32 has a duplicate in two frames of three.  Call
// with all 64 lanes.
static __device__ inline void pnp_draw_first_chunk_wave(const DevBuffers& d, SeqState& s, int seq, int n_tracks, int upto) {
    const int lane = threadIdx.x & 63;
    const unsigned n = (unsigned)n_tracks;
    if (upto > d.K) upto = d.K;
    if (n < 6 || upto > 32 || upto * 5 + 8 > SVO_RNG_TABLE_N) {                 // n == 5: the direct solve; tiny sets: not worth a second path
        if (lane == 0) { s.n_tracks = n_tracks; pnp_draw_subsets(d, s, seq, upto); }
        return;
    }
    int* out = d.subsets + (size_t)seq * d.K * 5;
    const unsigned long long recip = pnp_recip(n);
    int v[5]; bool dup = false;
    if (lane < upto) {
#pragma unroll
        for (int i = 0; i < 5; i++) v[i] = pnp_uniform((unsigned)SVO_RNG_STATES[lane * 5 + i], n, recip);
#pragma unroll
        for (int i = 1; i < 5; i++)
#pragma unroll
            for (int k = 0; k < i; k++) dup |= v[i] == v[k];
    }
    const unsigned long long dm = __ballot(dup);
    const int first_bad = dm ? __ffsll((long long)dm) - 1 : upto;              // subsets [0, first_bad) stand as drawn
    if (lane < first_bad) {
#pragma unroll
        for (int i = 0; i < 5; i++) out[lane * 5 + i] = v[i];
    }
    if (lane == 0) {
        int t = first_bad * 5;                                                 // raw draws consumed so far
        unsigned long long state = t > 0 ? SVO_RNG_STATES[t - 1] : SVO_RNG_SEED;
        for (int it = first_bad; it < upto; it++) pnp_draw_subset<true>(state, t, n, recip, out + it * 5);
        s.pnp_drawn = upto;
        s.pnp_rng = state;
    }
}

// The last collected frame's observation and descriptor rows as the descriptor index's batched insertion reads them (svo_api.hip;
// for svo_match_api.hip, not exported through include/svo.h).  hdr: {n_tracks, n_rows} per sequence; the rows of sequence i begin at
// row i * pitch of obs and desc.  in_ring: the rows are still in their slot of the host-mapped rings and obs_m, desc_m are that
// slot's device addresses on `device`; otherwise they are in the context's kept copies (plain host memory) and obs_m, desc_m are null.
// desc_h and desc_m are null when the frame had no descriptor rows.  B and device are filled for every context; the return is
// SVO_ERR_ARG for a null context, SVO_ERR_STATE exactly where svo_get_last_track_descriptors gives it, else SVO_OK.
struct SvoLastRowsView {
    int B, device;
    bool track_on, desc_on, in_ring;
    const int* hdr;
    const svo_track_obs *obs_h, *obs_m;
    const uint8_t *desc_h, *desc_m;
    size_t pitch;
};
int svo_last_rows_view(svo_context* c, SvoLastRowsView* v);
