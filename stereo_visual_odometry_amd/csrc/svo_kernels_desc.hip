// svo_kernels_desc.hip — the steered BRIEF-256 descriptor of a point (include/svo.h, "Binary descriptors"; the integer rules are in
// svo_desc.hpp): k_track_desc / k_track_desc_lean describe a frame's tracks at l1 on level 0 of the T1 pyramid, straight into the
// pinned descriptor ring; k_describe_points is the same device function over a plain image (svo_describe_points).
//
// One wave per point, four points per 256-thread block.  A wave
//   1. loads the 31 x 31 patch into LDS (rows 32 bytes apart, as the rows of the sum planes are 32 samples apart), REFLECT_101 done
//      by index arithmetic on the load — the stored border of a pyramid level is lk_pad_for(win) wide, 12 at win = 5, so it cannot be
//      relied on for 15; the bytes are the same either way;
//   2. sums m10, m01 over the disc, lane-strided, and reduces across the wave in int32;
//   3. scores one bin per lane (0 .. 29) in int64 and takes the wave's arg-max, the lowest bin at equal scores;
//   4. builds the 27 x 27 plane of 5 x 5 box sums in LDS, separably, in u16 (a sum is at most 6375);
//   5. evaluates tests lane, lane + 64, lane + 128, lane + 192: four ballots are the row's four 64-bit words.
// The block's rows are staged in LDS and leave as 16-byte stores, two lanes per row: the ring is host memory.
// LDS per block: 4 x (32 * 32 + 31 * 32 * 2 + 27 * 32 * 2) + 4 * 32 = 19072 bytes; eight blocks fit a CU's 160 KiB.
#include "svo_internal.hpp"
#include "svo_desc.hpp"
#include <string.h>

#define DESC_THREADS 256
#define DESC_WAVES (DESC_THREADS / 64)
#define DESC_SIDE (2 * SVO_DESC_HALF + 1)             // 31
#define DESC_PLANE (2 * SVO_DESC_REACH + 1)           // 27: box centres -13 .. 13
#define DESC_PITCH 32                                 // samples between rows of the patch and of the two sum planes

// LDS writes of one phase before the reads of the next, within a wave
static __device__ __forceinline__ void desc_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The descriptor of the point (x, y) of the w x h image img (rows `stride` bytes apart), by the 64 lanes of one wave with the wave's
// LDS: words[0 .. 3] on every lane, and the bin.  x, y finite; w, h >= 16.
static __device__ __forceinline__ int desc_wave(const uint8_t* __restrict__ img, int w, int h, int stride, float x, float y,
                                                uint8_t* patch, uint16_t* hs, uint16_t* box, unsigned long long words[4]) {
    const int lane = threadIdx.x & 63;
    const int cx = desc_centre(x, w), cy = desc_centre(y, h);
    int m10 = 0, m01 = 0;
    // every plane is 32 samples wide: sample i = 64 * pass + lane is (row i >> 5, column i & 31), two rows per pass
#pragma unroll 4
    for (int i = lane; i < DESC_SIDE * DESC_PITCH; i += 64) {
        const int r = i >> 5, c = i & 31;
        const int dx = c - SVO_DESC_HALF, dy = r - SVO_DESC_HALF;
        if (c < DESC_SIDE) {
            const int p = img[(size_t)desc_reflect(cy + dy, h) * (size_t)stride + desc_reflect(cx + dx, w)];
            patch[i] = (uint8_t)p;
            if (dx * dx + dy * dy <= SVO_DESC_DISC) { m10 += dx * p; m01 += dy * p; }
        }
    }
    for (int o = 32; o > 0; o >>= 1) { m10 += __shfl_xor(m10, o); m01 += __shfl_xor(m01, o); }
    // the bin: lane k < 30 holds bin k's score, the rest hold bin 0's under the index 64 + lane, which never wins a tie
    int bin = lane < SVO_DESC_BINS ? lane : 64 + lane;
    long long top = desc_score(m10, m01, lane < SVO_DESC_BINS ? lane : 0);
    for (int o = 32; o > 0; o >>= 1) {
        const long long s = __shfl_xor(top, o);
        const int k = __shfl_xor(bin, o);
        if (desc_beats(s, k, top, bin)) { top = s; bin = k; }
    }
    desc_wave_sync();
#pragma unroll 2
    for (int i = lane; i < DESC_SIDE * DESC_PITCH; i += 64) {        // 5-sums along rows: hs[r][c] = P[r][c .. c + 4], c < 27
        if ((i & 31) < DESC_PLANE) {
            const uint8_t* q = patch + i;
            hs[i] = (uint16_t)(q[0] + q[1] + q[2] + q[3] + q[4]);
        }
    }
    desc_wave_sync();
#pragma unroll 2
    for (int i = lane; i < DESC_PLANE * DESC_PITCH; i += 64) {       // then along columns: box[v][u] = B(u - 13, v - 13)
        if ((i & 31) < DESC_PLANE) {
            const uint16_t* q = hs + i;
            box[i] = (uint16_t)(q[0] + q[DESC_PITCH] + q[2 * DESC_PITCH] + q[3 * DESC_PITCH] + q[4 * DESC_PITCH]);
        }
    }
    desc_wave_sync();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int8_t* t = SVO_BRIEF_PATTERN + 4 * (lane + 64 * k);
        int ax, ay, bx, by;
        desc_rotate(t[0], t[1], bin, ax, ay);
        desc_rotate(t[2], t[3], bin, bx, by);
        const int a = box[(ay + SVO_DESC_REACH) * DESC_PITCH + ax + SVO_DESC_REACH], b = box[(by + SVO_DESC_REACH) * DESC_PITCH + bx + SVO_DESC_REACH];
        words[k] = __ballot(a < b);
    }
    return bin;
}

// One block: points first .. first + 3 of `n` (a point = xy[i]), rows to out + 32 i, bins (when not null) to bins[i].
static __device__ __forceinline__ void desc_block(const uint8_t* __restrict__ img, int w, int h, int stride, const float2* __restrict__ xy, int n,
                                                  uint8_t* __restrict__ out, int* __restrict__ bins) {
    __shared__ uint8_t sh_patch[DESC_WAVES][(DESC_SIDE + 1) * DESC_PITCH];
    __shared__ uint16_t sh_hs[DESC_WAVES][DESC_SIDE * DESC_PITCH];
    __shared__ uint16_t sh_box[DESC_WAVES][DESC_PLANE * DESC_PITCH];
    __shared__ unsigned long long sh_rows[DESC_WAVES][4];
    const int first = blockIdx.x * DESC_WAVES;
    if (first >= n) return;                                          // the whole block: no wave is left at the barrier below
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = first + wv;
    if (i < n) {
        const float2 p = xy[i];
        unsigned long long words[4];
        const int bin = desc_wave(img, w, h, stride, p.x, p.y, sh_patch[wv], sh_hs[wv], sh_box[wv], words);
        if (lane < 4) sh_rows[wv][lane] = lane == 0 ? words[0] : lane == 1 ? words[1] : lane == 2 ? words[2] : words[3];
        if (bins && lane == 0) bins[i] = bin;
    }
    __syncthreads();
    const int left = n - first;                                      // rows of this block: 1 .. 4, 16-byte halves 0 .. 2 * rows - 1
    const int rows = left < DESC_WAVES ? left : DESC_WAVES;
    if (threadIdx.x < 2 * rows)
        reinterpret_cast<uint4*>(out + (size_t)first * SVO_DESC_BYTES)[threadIdx.x] = reinterpret_cast<const uint4*>(&sh_rows[0][0])[threadIdx.x];
}

// The frame pipeline's launch, behind k_track_obs: grid (ceil(max_rows / 4), launch_seqs).  Row i of a sequence describes track i
// (d.tl1, the observation ring's order) on plane 0, camera 0 of the T1 pyramid's level 0; rows >= min(n_tracks, max_rows) are not
// touched.
static __device__ __forceinline__ void track_desc_body(const DevBuffers& d, const DescArgs& a) {
    const int seq = seq_of(d, blockIdx.y);
    const SeqState& s = d.st[seq];
    int n = s.active ? s.n_tracks : 0;
    n = n < a.max_rows ? n : a.max_rows;
    n = n < d.CAP ? n : d.CAP;
    const LevelInfo L0 = d.geom.lv[0];
    const uint8_t* img = d.pyr + pyr_index(d, seq, s.slot_t1, 0) + L0.off;
    desc_block(img, L0.w, L0.h, L0.stride, d.tl1 + (size_t)seq * d.CAP, n, a.rows + (size_t)seq * a.max_rows * SVO_DESC_BYTES, nullptr);
}
__global__ __launch_bounds__(DESC_THREADS) void k_track_desc(DevBuffers d, DescArgs a) { track_desc_body(d, a); }
// the 48-register build a co-resident context launches beside another's LK grid, as k_track_obs_lean
__global__ __launch_bounds__(DESC_THREADS) __attribute__((amdgpu_num_vgpr(48))) void k_track_desc_lean(DevBuffers d, DescArgs a) { track_desc_body(d, a); }
void launch_track_desc(const DevBuffers& d, const DescArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(d.co_resident ? k_track_desc_lean : k_track_desc, dim3((a.max_rows + DESC_WAVES - 1) / DESC_WAVES, launch_seqs(d)), dim3(DESC_THREADS), 0, st, d, a);
}

// The stage alone: n points of a plain w x h image, rows to desc, bins to bins (or null).  Device pointers.
__global__ __launch_bounds__(DESC_THREADS) void k_describe_points(const uint8_t* img, int w, int h, int stride, const float2* xy, int n, uint8_t* desc, int* bins) {
    desc_block(img, w, h, stride, xy, n, desc, bins);
}
void launch_describe_points(const uint8_t* img, int w, int h, int stride, const float2* xy, int n, uint8_t* desc, int* bins, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_describe_points, dim3((n + DESC_WAVES - 1) / DESC_WAVES), dim3(DESC_THREADS), 0, st, img, w, h, stride, xy, n, desc, bins);
}

// svo_descriptor_pattern: the host's copy of the tables the kernels index
void desc_copy_tables(int8_t* pattern, int32_t* cs) {
    if (pattern) memcpy(pattern, SVO_BRIEF_PATTERN, sizeof(SVO_BRIEF_PATTERN));
    if (cs) { memcpy(cs, SVO_DESC_COS, sizeof(SVO_DESC_COS)); memcpy(cs + SVO_DESC_BINS, SVO_DESC_SIN, sizeof(SVO_DESC_SIN)); }
}
